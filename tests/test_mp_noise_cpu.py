"""CPU: the contract of the native point noise of the mask-piloted rows (include/mpformer_hip.h, mpf_mp_noise_rows), restated
in numpy.  The restatement is checked against known answers of Philox4x32-10 that do not come from it; the GPU tests
(test_mp_noise_gpu.py) import it and compare the kernel with it byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

# ---- the restatement ---------------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MP_NOISE_KEY = 0x4D50466F726D6572          # MPF_MP_NOISE_KEY of the header ("MPFormer")
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 broadcastable uint32 arrays, key: 2 python ints -> 4 uint32 arrays (Salmon et al., SC'11)."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def noise_u(seed, draw, rows, HW):
    """u(r, j) for r in ``rows`` (1-D ints), j < HW -> float32 [len(rows), HW]."""
    key = (int(seed) ^ MP_NOISE_KEY) & 0xFFFFFFFFFFFFFFFF
    draw = int(draw) & 0xFFFFFFFFFFFFFFFF
    quads = (HW + 3) // 4
    q = np.arange(quads, dtype=np.uint32)[None, :]
    r = np.asarray(rows, dtype=np.uint32)[:, None]
    words = philox4x32_10((q, r, np.uint32(draw & 0xFFFFFFFF), np.uint32(draw >> 32)), (key & 0xFFFFFFFF, key >> 32))
    w = np.stack(words, axis=-1).reshape(len(rows), quads * 4)[:, :HW]           # position j: word j & 3 of block j >> 2
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def noise_ratio(base, noise_scale):
    """ratio[r]: the open count and noise_scale / HW each rounded to fp32, then one fp32 multiply."""
    counts = (np.asarray(base) == 0).sum(1)
    return counts.astype(np.float32) * np.float32(noise_scale / base.shape[1]), counts


def noise_rows_ref(base, src_of, N, pad, noise_scale, seed, draw):
    """base uint8 [R, HW] (0 / 1), src_of int [N * pad] -> uint8 [N, pad, HW]."""
    base = np.asarray(base, dtype=np.uint8)
    R, HW = base.shape
    ratio, _ = noise_ratio(base, noise_scale)
    noised = base ^ (noise_u(seed, draw, np.arange(R), HW) < ratio[:, None]).astype(np.uint8)
    out = np.ones((N * pad, HW), dtype=np.uint8)
    src_of = np.asarray(src_of).reshape(-1)
    used = (src_of >= 0) & (src_of < R)
    out[used] = noised[src_of[used]]
    return out.reshape(N, pad, HW)


def src_of_table(num, scalar):
    """the rows ``prepare_for_dn_v5`` fills (:1022-1037): image b, copy s, instance t -> slot s * max_num + t, showing row
    s * sum(num) + first[b] + t of the repeated ground-truth rows; -1 elsewhere.  -> (int32 [N * pad], pad)"""
    max_num, total = max(num), sum(num)
    pad = scalar * max_num
    t = np.full((len(num), pad), -1, dtype=np.int32)
    first = 0
    for b, n in enumerate(num):
        for s in range(scalar):
            t[b, s * max_num:s * max_num + n] = s * total + first + np.arange(n)
        first += n
    return t.reshape(-1), pad


def rect_rows(T, h, w, rng, min_cover=0.0):
    """T rectangle instances on an h x w grid as MP rows: 0 inside (attend), 1 outside -> uint8 [T, h * w]"""
    rows = np.ones((T, h, w), dtype=np.uint8)
    for t in range(T):
        while True:
            hh, ww = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
            if hh * ww >= min_cover * h * w:
                break
        y0, x0 = int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1))
        rows[t, y0:y0 + hh, x0:x0 + ww] = 0
    return rows.reshape(T, h * w)


# the flip-rate case of the GPU test, pinned: config B's finest level, N = 2 images of 20 instances, scalar 5 -> 200 rows
FLIP_CASE = dict(h=128, w=128, num=(20, 20), scalar=5, noise_scale=0.2, seed=20260116, draw=8, layout_seed=7)


def flip_case_rows():
    c = FLIP_CASE
    rows = rect_rows(sum(c["num"]), c["h"], c["w"], np.random.default_rng(c["layout_seed"]), min_cover=0.01)
    return np.tile(rows, (c["scalar"], 1))


def check_flip_rate(base, noised_rows, noise_scale):
    """per base row: |k - p HW| <= 5 sqrt(HW p (1 - p)) with k the observed flips; every row must be in the normal regime
    (p HW >= 25).  noised_rows uint8 [R, HW], row r the noised version of base row r."""
    HW = base.shape[1]
    ratio, counts = noise_ratio(base, noise_scale)
    p = ratio.astype(np.float64)
    assert (p * HW >= 25).all() and (counts >= 125).all(), "an instance of the flip-rate case is too small for the normal bound"
    k = (base != noised_rows).sum(1).astype(np.float64)
    dev = np.abs(k - p * HW)
    bound = 5.0 * np.sqrt(HW * p * (1.0 - p))
    worst = int(np.argmax(dev / bound))
    print(f"flip rate: {len(p)} rows, worst row {worst}: k = {k[worst]:.0f}, p HW = {p[worst] * HW:.1f}, "
          f"|dev| = {dev[worst]:.1f} <= {bound[worst]:.1f}")
    assert (dev <= bound).all(), (worst, k[worst], p[worst] * HW, bound[worst])


# ---- tests -------------------------------------------------------------------------------------------------------------------
# known answers of philox4x32_10 (counter, key, result): the three vectors Random123 ships in examples/kat_vectors.  The
# result words were confirmed with the same generator's implementation in rocRAND (rocrand/rocrand_philox4x32_10.h,
# philox4x32_10_engine::ten_rounds compiled for the host) before they were written here; none comes from this file's code.
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),      # the digits of pi
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_restatement_known_answers(ctr, key, want):
    got = philox4x32_10([np.uint32(c) for c in ctr], key)
    assert tuple(int(g) for g in got) == want


def test_philox_restatement_is_elementwise():
    """the vectorised call gives each lane what a call of its own gives (the kernel tests rely on whole-array calls)"""
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint32)
    got = philox4x32_10([ctrs[:, i] for i in range(4)], KAT[2][1])
    for lane in range(3):
        one = philox4x32_10([np.uint32(c) for c in KAT[lane][0]], KAT[2][1])
        assert [int(g[lane]) for g in got] == [int(o) for o in one]
    assert tuple(int(g[2]) for g in got) == KAT[2][2]


def test_noise_u_layout():
    """counter = (j >> 2, r, draw lo, draw hi), key = halves of seed ^ MPF_MP_NOISE_KEY, position j takes word j & 3"""
    seed, draw, r, HW = 0x1234_5678_9ABC_DEF0, (7 << 32) | 12, 5, 23
    u = noise_u(seed, draw, [r], HW)[0]
    key = seed ^ MP_NOISE_KEY
    for j in (0, 3, 4, 22):
        words = philox4x32_10([np.uint32(j >> 2), np.uint32(r), np.uint32(12), np.uint32(7)], (key & 0xFFFFFFFF, key >> 32))
        assert u[j] == np.float32(int(words[j & 3]) >> 8) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    # a row's draws do not depend on which other rows are asked for, or on the row length
    both = noise_u(seed, draw, [2, r], 64)
    assert np.array_equal(both[1, :HW], u)
    assert not np.array_equal(noise_u(seed, draw + 4, [r], HW)[0], u)
    assert not np.array_equal(noise_u(seed + 1, draw, [r], HW)[0], u)


def test_src_of_table_is_the_inverse_of_bid_slot():
    """against the (bid, slot) index pair of transformer_decoder._mp_setup / reference :1022-1037"""
    num, scalar = [3, 0, 2], 4
    src_of, pad = src_of_table(num, scalar)
    max_num = max(num)
    bid = np.tile(np.concatenate([np.full(n, i) for i, n in enumerate(num)]), scalar)
    slot = np.concatenate([np.concatenate([np.arange(n) for n in num]) + max_num * i for i in range(scalar)])
    want = np.full((len(num), pad), -1)
    want[bid, slot] = np.arange(len(bid))
    assert np.array_equal(src_of.reshape(len(num), pad), want)


def test_flip_rate_of_the_pinned_case():
    """the GPU test's flip-rate case, here with the restatement's rows: the pinned seed is inside the binomial bound on every
    row, and every instance is large enough for the bound to apply (no row excluded)"""
    c = FLIP_CASE
    base = flip_case_rows()
    assert base.shape == (200, 128 * 128)
    src_of = np.arange(base.shape[0])
    rows = noise_rows_ref(base, src_of, 1, base.shape[0], c["noise_scale"], c["seed"], c["draw"])[0]
    check_flip_rate(base, rows, c["noise_scale"])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    m = re.search(r"#define\s+MPF_MP_NOISE_KEY\s+0x([0-9A-Fa-f]+)ULL", src)
    assert m and int(m.group(1), 16) == MP_NOISE_KEY
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in ("mpf_mp_open_counts", "mpf_mp_noise_rows"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "mp_noise.hip"))
    from mp_former_amd import transformer_decoder as TD
    assert callable(TD.mp_noise_rows) and callable(TD.mp_open_counts)


def test_argument_errors_without_a_gpu(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: the arguments are checked before any GPU call
    assert lib.mpf_mp_open_counts(None, 4, 64, one, None) == -3
    assert lib.mpf_mp_open_counts(one, 4, 64, None, None) == -3
    assert lib.mpf_mp_open_counts(one, 0, 64, one, None) == -2
    assert lib.mpf_mp_open_counts(one, 4, -1, one, None) == -2 and b"mpf_mp_open_counts" in lib.mpf_last_error()
    good = [one, one, one, 4, 64, 2, 3, 0.2, 1, 0, one, None]
    for i in (0, 1, 2, 10):
        assert lib.mpf_mp_noise_rows(*(good[:i] + [None] + good[i + 1:])) == -3
    for i in (3, 4, 5, 6):
        assert lib.mpf_mp_noise_rows(*(good[:i] + [0] + good[i + 1:])) == -2
        assert lib.mpf_mp_noise_rows(*(good[:i] + [-5] + good[i + 1:])) == -2
    assert lib.mpf_mp_noise_rows(*(good[:7] + [-0.1] + good[8:])) == -2
    assert lib.mpf_mp_noise_rows(*(good[:7] + [float("nan")] + good[8:])) == -2 and b"mpf_mp_noise_rows" in lib.mpf_last_error()
    assert lib.mpf_mp_noise_rows(*(good[:4] + [1 << 20, 1 << 6, 1 << 6] + good[7:])) == -4


def test_python_entry_points_reject_cpu_tensors(built):
    import torch
    from mp_former_amd import transformer_decoder as TD
    base = torch.zeros(2, 16, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU only"):
        TD.mp_open_counts(base)
    with pytest.raises(RuntimeError, match="GPU only"):
        TD.mp_noise_rows(base, torch.zeros(2, dtype=torch.int32), 1, 2, 0.2, 0, 0)
