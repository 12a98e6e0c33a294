"""GPU: bounding boxes of packed masks (csrc/seg_box.hip, mpf_seg_bits_boxes via mp_former_amd.inference.mask_boxes) against
``np.any`` over each axis of the dense masks (tests/_box_restate.py).  The packed input is numpy's (tests/_ap_restate.pack_columns),
so neither side depends on the code under test.  Integer results, compared for equality."""
import functools

import numpy as np
import pytest
import torch

import _ap_restate as R
import _box_restate as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (H, W): many columns per word; a column is exactly one word; every column straddles a word boundary; the tail word partly past
# H * W; a column spans three words; more words (1057) than the workgroup has threads, so that a thread takes a second word; and
# more (4137) than the 4 x 1024 of one pass, so that a thread takes a second pass
SHAPES = [(5, 7), (64, 3), (65, 4), (37, 50), (130, 9), (130, 520), (257, 1030)]
DENSITIES = (0.5, 0.01)
N_RANDOM = 16


@functools.lru_cache(maxsize=None)
def _masks(H, W):
    """-> (names, dense bool [M, H, W]) of one shape, made once"""
    names, ms = [], []

    def add(name, m):
        names.append(name)
        ms.append(m)
    z = lambda: np.zeros((H, W), dtype=bool)       # noqa: E731
    add("empty", z())
    add("full", np.ones((H, W), dtype=bool))
    for name, (y, x) in {"corner00": (0, 0), "corner0W": (0, W - 1), "cornerH0": (H - 1, 0), "cornerHW": (H - 1, W - 1)}.items():
        m = z()
        m[y, x] = True
        add(name, m)
    m = z()
    m[H - 1, :] = True
    m[:, W - 1] = True
    add("last row and column", m)
    m = z()
    m[1 % H, 0] = True
    m[H - 2, W - 1] = True
    add("two far pixels", m)
    g = np.random.default_rng(H * 1000 + W)
    for p in DENSITIES:
        for i in range(N_RANDOM):
            add(f"random {p} #{i}", g.random((H, W)) < p)
    for i in range(N_RANDOM):                            # three pixels anywhere: at the large shapes the densities fill the box
        m = z()
        m.reshape(-1)[g.integers(0, H * W, 3)] = True
        add(f"three pixels #{i}", m)
    return tuple(names), np.stack(ms)


@functools.lru_cache(maxsize=None)
def _want(H, W):
    return X.boxes_of(_masks(H, W)[1])


def _dev_bits(dense):
    return torch.from_numpy(R.pack_columns(dense).view(np.int64)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda o: f"{o[0]}x{o[1]}")
def test_mask_boxes_equal_the_dense_restatement(hw):
    from mp_former_amd import _lib
    from mp_former_amd.inference import mask_boxes
    H, W = hw
    names, dense = _masks(H, W)
    want = _want(H, W)
    assert want[0].tolist() == [0, 0, 0, 0] and want[1].tolist() == [0, 0, W, H] and want[6].tolist() == [0, 0, W, H]
    assert want[5].tolist() == [W - 1, H - 1, W, H]
    bits = _dev_bits(dense)
    before = bits.clone()
    got = mask_boxes(bits, (H, W))
    assert "seg_bits_boxes_kernel" in _lib.last_kernel()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(names), 4) and got.device == DEV
    assert torch.equal(bits, before), "the input was modified"
    got = _np(got)
    for n, name in enumerate(names):
        assert got[n].tolist() == want[n].tolist(), f"{H}x{W} {name}"
    # one mask alone, and a view that is not contiguous
    np.testing.assert_array_equal(_np(mask_boxes(bits[7:8], (H, W))), want[7:8])
    wide = torch.zeros((len(names), 2 * bits.shape[1]), dtype=torch.int64, device=DEV)
    wide[:, ::2] = bits
    np.testing.assert_array_equal(_np(mask_boxes(wide[:, ::2], (H, W))), want)


def test_no_mask_gives_an_empty_result():
    from mp_former_amd.inference import mask_boxes
    H, W = 37, 50
    got = mask_boxes(torch.zeros((0, (H * W + 63) // 64), dtype=torch.int64, device=DEV), (H, W))
    assert tuple(got.shape) == (0, 4) and got.dtype == torch.int32 and got.device == DEV


def test_tubes_equal_the_flat_call():
    from mp_former_amd.inference import mask_boxes
    H, W = 37, 50
    _, dense = _masks(H, W)
    pick = dense[[9, 0, 25, 1, 7, 30]]                   # random, empty, sparse, full, two pixels, sparse
    bits = _dev_bits(pick)
    flat = mask_boxes(bits, (H, W))
    tubes = mask_boxes(bits.view(3, 2, -1), (H, W))
    assert tuple(tubes.shape) == (3, 2, 4) and tubes.dtype == torch.int32
    assert torch.equal(tubes.view(6, 4), flat)
    np.testing.assert_array_equal(_np(flat), X.boxes_of(pick))
    empty = mask_boxes(bits.view(3, 2, -1)[:0], (H, W))
    assert tuple(empty.shape) == (0, 2, 4)


def test_packed_by_the_device_and_checked_arguments():
    """the bits of pack_masks give the same boxes; a size that does not fit the words and a CPU tensor are refused"""
    from mp_former_amd.inference import mask_boxes, pack_masks
    H, W = 65, 4
    _, dense = _masks(H, W)
    got = mask_boxes(pack_masks(torch.from_numpy(dense).to(DEV)), (H, W))
    np.testing.assert_array_equal(_np(got), _want(H, W))
    bits = _dev_bits(dense)
    with pytest.raises(ValueError, match="does not fit"):
        mask_boxes(bits, (H, W + 20))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        mask_boxes(bits, None)
    with pytest.raises(ValueError, match="int64"):
        mask_boxes(bits.to(torch.int32), (H, W))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_boxes(bits.cpu(), (H, W))
