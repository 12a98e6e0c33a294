"""CPU: the host logic of mask_fused.FactoredClipMasks on CPU tensors (nothing is evaluated): shape, dim-1 slicing, detach,
row_offsets and same_factors."""
import numpy as np
import pytest
import torch

B, R, T, h, w = 2, 14, 3, 4, 8


def _factors():
    from mp_former_amd.mask_fused import FactoredClipMasks
    parent = torch.zeros(R + 2, B, 256, dtype=torch.bfloat16)                   # sequence-first: row stride B * 256
    me = parent[1:R + 1].transpose(0, 1).requires_grad_(True)                   # [B, R, 256]
    mf4 = torch.zeros(B, T * h, w, 256, dtype=torch.bfloat16).permute(0, 3, 1, 2)
    return FactoredClipMasks, me, mf4


def test_shape_is_the_clip_tensors():
    FC, me, mf4 = _factors()
    fm = FC(me, mf4, T)
    assert fm.shape == torch.Size((B, R, T, h, w)) and fm.dim() == 5 and fm.size(2) == T and fm.size() == fm.shape
    assert fm.dtype == torch.bfloat16 and not fm.is_cuda and fm.requires_grad and fm.device == me.device
    assert FC(me, mf4, T, 3, 10).shape == torch.Size((B, 7, T, h, w))
    with pytest.raises(RuntimeError, match="frames"):
        FC(me, mf4, 5)


def test_dim1_slices_keep_the_factors():
    FC, me, mf4 = _factors()
    fm = FC(me, mf4, T)
    a = fm[:, 7:14]
    assert isinstance(a, FC) and (a.q0, a.q1, a.T) == (7, 14, T) and a.me is me and a.mf is mf4
    b = a[:, 2:5]
    assert (b.q0, b.q1) == (9, 12) and b.shape == torch.Size((B, 3, T, h, w))
    assert (fm[:, -3:].q0, fm[:, -3:].q1) == (11, 14) and fm[:, 5:2].shape[1] == 0 and fm[:, :100].q1 == R
    assert fm.same_factors(a) and a.same_factors(b) and b.same_factors(fm)


def test_same_factors_needs_the_same_objects_frames_and_class():
    from mp_former_amd.mask_fused import FactoredMasks
    FC, me, mf4 = _factors()
    fm = FC(me, mf4, T)
    assert not fm.same_factors(FC(me.detach(), mf4, T)) and not fm.same_factors(FC(me, mf4.detach(), T))
    assert not fm.same_factors(FC(me, mf4, 1)) and not fm.same_factors(FC(me, mf4, 2))
    assert not fm.same_factors(FactoredMasks(me, mf4)) and not fm.same_factors(torch.zeros(B, R, T, h, w))
    assert not fm.same_factors(fm.detach())


def test_detach_keeps_the_view_and_drops_the_graph():
    FC, me, mf4 = _factors()
    d = FC(me, mf4, T, 2, 9).detach()
    assert isinstance(d, FC) and (d.q0, d.q1, d.T) == (2, 9, T) and not d.requires_grad
    assert d.me.data_ptr() == me.data_ptr() and d.mf.data_ptr() == mf4.data_ptr()


def test_row_offsets_address_the_embedding_rows_of_the_view():
    FC, me, mf4 = _factors()
    v = FC(me, mf4, T)[:, 7:14]
    assert me.stride(0) == 256 and me.stride(1) == B * 256
    assert v.row_offsets(1, 0) == 256 + 7 * B * 256
    q = np.arange(3)
    assert np.array_equal(v.row_offsets(np.array([0, 1, 1]), q), np.array([0, 256, 256]) + (7 + q) * B * 256)
