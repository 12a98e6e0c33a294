"""The key-exact attention checks of tests/_attn_cases.py, tested without a GPU: the builder's invariants for every row of the case
table, the torch emulation of the kernels' arithmetic passing every assertion, and every single fault of `_attn_cases.FAULTS`
failing at least one assertion on every case where it can apply — the assertions of tests/test_attn_keys_gpu.py are sharp without
a wrong kernel ever running on a device."""
import math

import pytest
import torch

import _attn_cases as A


@pytest.fixture(scope="module")
def problems():
    return {c.name: A.build(c) for c in A.CASES}


def test_case_table_covers_the_split_shapes():
    """one wave; several waves in one workgroup; 2..8 workgroups with a trailing empty wave slot; more than 8 workgroups; kpw 512;
    the default rows at Lk 1100 / 257 / 1032; both mask kinds; an odd-offset mask with Lk % 8 == 0; no-mask rows only at 1, 3, 8, 9"""
    geo = {c.name: A.split_of(c) for c in A.CASES}
    for c in A.CASES:
        kpw, nw, wg, ranges = geo[c.name]
        assert wg == c.wg and c.Lq <= 81 and c.Lk <= 1100 and c.N <= 2
        assert (c.kpw == 0 and c.nw == 8) or c.kpw == c.kpw_eff
    forced = [c for c in A.CASES if c.kpw]
    assert any(len(geo[c.name][3]) == 1 for c in forced)
    assert any(geo[c.name][2] == 1 and geo[c.name][1] > 1 for c in forced)
    assert any(2 <= geo[c.name][2] <= 8 and geo[c.name][3][-1][0] == geo[c.name][3][-1][1] for c in forced)
    assert any(geo[c.name][2] > 8 for c in forced)
    assert any(c.kpw == 512 for c in forced)
    assert {c.Lk for c in A.CASES if not c.kpw and c.mask != "none"} >= {1100, 257, 1032}
    assert {c.mask for c in A.CASES} == {"image", "shared", "none"}
    assert any(c.odd and c.Lk % 8 == 0 for c in A.CASES)
    assert {c.Lk for c in A.CASES if c.mask == "none"} == {1, 3, 8, 9}
    assert all(c.family == "nomask" for c in A.CASES if c.Lk in (3, 9))
    assert {c.Lq for c in A.CASES} == {1, 33, 64, 81}
    assert {c.Lk for c in A.CASES if c.mask != "none"} <= {1, 8, 63, 64, 65, 257, 453, 600, 1032, 1100}
    for fam in ("fullmask",):
        assert {geo[c.name][2] == 1 for c in A.CASES if c.family == fam} == {True, False}
        assert any(geo[c.name][2] > 8 for c in A.CASES if c.family == fam)
    assert sum(c.family == "few_scaled" for c in A.CASES) * 3 >= sum(c.family in ("few", "few_scaled") for c in A.CASES)


@pytest.mark.parametrize("name", [c.name for c in A.CASES if c.mask != "none"])
def test_builder_invariants(problems, name):
    prob = problems[name]
    c = prob["case"]
    kpw, nw, wg, ranges = A.split_of(c)
    imgs = c.N
    opened = {k for rows in prob["open"] for ks in rows for k in ks}
    dec = set(prob["decoys"])
    # the mask is exactly the open lists
    m = prob["mask"] if prob["mask"].dim() == 3 else prob["mask"][None].expand(c.N, c.Lq, c.Lk)
    for n in range(imgs):
        for r in range(c.Lq):
            assert sorted((~m[n, r]).nonzero().flatten().tolist()) == sorted(prob["open"][n][r])
    # open keys per row
    full = A.full_rows(c)
    for rows in prob["open"]:
        for r, ks in enumerate(rows):
            if r in full:
                assert ks == []
            elif c.family == "selector":
                assert len(ks) == 1
            else:
                assert 1 <= len(ks) <= 4
    if c.family == "selector":
        for rows in prob["open"]:                       # each key opened by at most one row (of an image)
            flat = [ks[0] for ks in rows]
            assert len(set(flat)) == len(flat)
    else:
        counts = [len(ks) for rows in prob["open"] for r, ks in enumerate(rows) if r not in full]
        if c.Lk >= 64 and c.Lq > 1:
            assert min(counts) >= 2 and {2, 3, 4} <= set(counts)
            flat = [k for rows in prob["open"][:1] for ks in rows for k in ks]
            assert len(set(flat)) < len(flat)             # some keys shared between rows
        if wg > 1:                                        # rows whose keys all lie in one workgroup's range: every other partial is (-inf, 0)
            span = kpw * nw
            assert any(len({k // span for k in ks}) == 1 for rows in prob["open"] for ks in rows if len(ks) > 1)
            assert any(len({k // span for k in ks}) > 1 for rows in prob["open"] for ks in rows if len(ks) > 1)
    # boundary coverage: all of the boundary set where the rows suffice, else as many boundary keys as the rows can open, in order
    B = prob["boundary"]
    live_rows = (c.Lq - len(full)) * (c.N if c.mask == "image" else 1)
    cap = live_rows * (1 if c.family == "selector" else 4)
    assert set(B[:cap]) <= opened
    if cap < len(B):
        assert opened <= set(B)
    assert c.Lq == 1 or cap >= len(B), "only the single-query rows may be too small for their boundary set"
    # the covering rows open boundary keys
    for r in A.cover_rows(c):
        assert any(set(rows[r]) & set(B) for rows in prob["open"])
    assert set(A.cover_rows(c)) | set(full) >= {r for r in (0, 15, 16, 31, 32, c.Lq - 1) if r < c.Lq}
    # decoys: never open, at every offset from every boundary key and at the clamp positions unless a row opens that key
    assert not (dec & opened) and m[:, :, sorted(dec)].all()
    for b in B:
        for off in A.OFFSETS + (kpw,):
            for k in (b - off, b + off):
                if 0 <= k < c.Lk:
                    assert k in dec or k in opened
    for k in A.clamp_keys(c):
        assert k in dec or k in opened
    # score gap in fp64: every decoy at least 20 above every open key, in every row and head; large finite |v|
    if dec:
        s = A.scores64(prob["q"], prob["k"])
        top_open = s.masked_fill(m[:, None], -math.inf).amax(-1)                 # [N, H, Lq]
        low_dec = s[..., sorted(dec)].amin(-1)
        live = torch.isfinite(top_open)
        assert (low_dec[live] - top_open[live] >= A.GAP).all()
        assert (prob["v"][sorted(dec)].abs() >= 2.0 ** 20).all()
    if c.family == "few_scaled":                                                 # open scores of a row up to ~30 apart
        s = A.scores64(prob["q"], prob["k"]).masked_fill(m[:, None], math.nan)
        spread = torch.nan_to_num(s, nan=-math.inf).amax(-1) - torch.nan_to_num(s, nan=math.inf).amin(-1)
        assert 20.0 <= float(spread.max()) <= 45.0, float(spread.max())
    for t in ("q", "k", "v", "dO"):
        assert torch.isfinite(prob[t]).all() and torch.equal(prob[t], prob[t].bfloat16().float())


@pytest.mark.parametrize("name", A.CASE_IDS)
def test_emulation_passes_every_assertion(problems, name):
    prob = problems[name]
    ratios = A.evaluate(prob, A.emulate(prob))
    print(f"[attn keys] emulation {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("fault", A.FAULTS)
@pytest.mark.parametrize("name", A.CASE_IDS)
def test_single_faults_fail_an_assertion(problems, name, fault):
    prob = problems[name]
    if not A.fault_applies(prob, fault):
        # nothing to see: the faulty emulation is then the correct one (checked, so that `fault_applies` cannot hide a case)
        good, bad = A.emulate(prob), A.emulate(prob, fault=fault)
        assert all(torch.equal(good[k], bad[k]) for k in good)
        return
    with pytest.raises(AssertionError):
        A.evaluate(prob, A.emulate(prob, fault=fault))


def test_faults_apply_where_the_issue_expects_them():
    """the fault classes are not vacuous: every masked case with more than one row sees the range faults and the decoy fault, every
    multi-workgroup case the ignored partial"""
    for c in A.CASES:
        prob = A.build(c)
        app = {f for f in A.FAULTS if A.fault_applies(prob, f)}
        if c.mask != "none" and c.Lq > 1:
            assert {"drop_last", "admit_after", "mask_shift", "double", "admit_decoy_kv"} <= app, (c.name, app)
        if c.wg > 1:
            assert "skip_last_wg" in app
        if c.mask == "none":
            assert {"drop_last", "admit_after", "double"} <= app
