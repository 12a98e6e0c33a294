"""Argument validation of the residual LayerNorm entry points (csrc/elementwise.hip: mpf_res_ln256_*, mpf_ln_partial_reduce):
the status code and the mpf_last_error text of every rejection, the rows == 0 no-op, and the two workspace size queries
against the grid rule restated here.  Only rejected calls: validation runs before any HIP call, the pointers are never
dereferenced and nothing is launched."""
import pytest

E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
ONE = 16            # a non-NULL pointer that is never dereferenced
ROWS = (1, 5, 125, 901, 1024, 1025, 4097)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


def _partial_bytes(rows):
    """the grid rule: rows per workgroup = ceil(rows / 1024) rounded up to 4; [workgroup][2][256] floats"""
    rpb = (-(-rows // 1024) + 3) // 4 * 4
    return -(-rows // rpb) * 512 * 4


_HEAD = ("s", "mean", "rstd", "gamma", "gy32", "gy16", "gy_plus", "ds32", "ds16")
_TAIL = {
    "mpf_res_ln256_backward": ("dgamma", "dbeta", "rows", "stream"),
    "mpf_res_ln256_backward_ws": ("dgamma", "dbeta", "rows", "workspace", "bytes", "stream"),
    "mpf_res_ln256_backward_ws_amax": ("dgamma", "dbeta", "rows", "workspace", "bytes", "ds_amax", "stream"),
    "mpf_res_ln256_backward_partial": ("rows", "workspace", "bytes", "stream"),
    "mpf_res_ln256_backward_partial_amax": ("rows", "workspace", "bytes", "ds_amax", "stream"),
    "mpf_res_ln256_backward_det": ("dgamma", "rows", "workspace", "bytes", "stream"),
}
_FWD = ("x", "t", "t_dtype", "gamma", "beta", "s_out", "y32", "y16", "mean", "rstd", "rows", "eps", "padd", "padd_rows", "y_plus")
_FWD_TAIL = {"mpf_res_ln256_forward": ("stream",), "mpf_res_ln256_forward_b": ("y_bound", "padd_amax", "yplus_bound", "stream")}


def _backward_args(name, **kw):
    """a call that would be accepted (gy32 -> ds32, 5 rows, a workspace of exactly the size needed) with `kw` replaced;
    short: bytes added to the workspace size"""
    short = kw.pop("short", 0)
    a = dict.fromkeys(_HEAD + _TAIL[name], ONE)
    a.update(gy16=None, gy_plus=None, ds16=None, rows=5, stream=None)
    a.update(kw)
    a["bytes"] = _partial_bytes(a["rows"]) + (256 if name.endswith("_det") else 0) + short if a["rows"] > 0 else 0
    return [a[k] for k in _HEAD + _TAIL[name]]


def _forward_args(name, **kw):
    a = dict.fromkeys(_FWD + _FWD_TAIL[name], ONE)
    a.update(t=None, t_dtype=0, rows=5, eps=1e-5, padd=None, padd_rows=0, y_plus=None, padd_amax=None, yplus_bound=None, stream=None)
    a.update(kw)
    return [a[k] for k in _FWD + _FWD_TAIL[name]]


def _rejected(lib, name, args, code, text):
    assert getattr(lib, name)(*args) == code, name
    assert lib.mpf_last_error().decode() == text


@pytest.mark.parametrize("name,label,shape_text", [
    ("mpf_res_ln256_backward", "res_ln256_backward", "bad rows"),
    ("mpf_res_ln256_backward_ws", "res_ln256_backward_ws", "bad rows / workspace too small"),
    ("mpf_res_ln256_backward_ws_amax", "res_ln256_backward_ws", "bad rows / workspace too small"),
    ("mpf_res_ln256_backward_partial", "res_ln256_backward_partial", "bad rows / buffer too small"),
    ("mpf_res_ln256_backward_partial_amax", "res_ln256_backward_partial", "bad rows / buffer too small"),
    ("mpf_res_ln256_backward_det", "res_ln256_backward_det", "bad rows / workspace too small"),
])
def test_backward_rejections(lib, name, label, shape_text):
    null, shape = f"{label}: NULL buffer", f"{label}: {shape_text}"
    own = [k for k in _TAIL[name] if k in ("dgamma", "dbeta", "workspace")]
    for missing in ("s", "mean", "rstd", "gamma") + tuple(own):                   # a required buffer
        _rejected(lib, name, _backward_args(name, **{missing: None}), E_NULL, null)
    _rejected(lib, name, _backward_args(name, gy32=None), E_NULL, null)           # no gradient operand
    _rejected(lib, name, _backward_args(name, ds32=None), E_NULL, null)           # no ds output
    _rejected(lib, name, _backward_args(name, rows=-1), E_SHAPE, shape)
    if "workspace" in _TAIL[name]:
        for rows in (5, 4097):
            _rejected(lib, name, _backward_args(name, rows=rows, short=-1), E_SHAPE, shape)       # one byte short
    if name == "mpf_res_ln256_backward_ws_amax":
        _rejected(lib, name, _backward_args(name, ds_amax=None), E_NULL, "res_ln256_backward_ws_amax: NULL amax slot")


def test_forward_rejections(lib):
    null, shape = "res_ln256_forward: NULL buffer", "res_ln256_forward: bad rows / missing addend"
    for name in _FWD_TAIL:                  # _forward_b reports the shared rejections under the name of _forward
        for missing in ("x", "gamma", "beta", "mean", "rstd"):
            _rejected(lib, name, _forward_args(name, **{missing: None}), E_NULL, null)
        _rejected(lib, name, _forward_args(name, y32=None, y16=None), E_NULL, null)
        _rejected(lib, name, _forward_args(name, rows=-1), E_SHAPE, shape)
        _rejected(lib, name, _forward_args(name, y_plus=ONE), E_SHAPE, shape)                     # y_plus without padd
        _rejected(lib, name, _forward_args(name, y_plus=ONE, padd=ONE, padd_rows=0), E_SHAPE, shape)
        _rejected(lib, name, _forward_args(name, t=ONE, t_dtype=99), E_DTYPE, "res_ln256_forward: t dtype must be MPF_F32 or MPF_BF16")
    name, slot = "mpf_res_ln256_forward_b", "res_ln256_forward_b: NULL amax slot"
    _rejected(lib, name, _forward_args(name, y_bound=None), E_NULL, slot)
    plus = dict(y_plus=ONE, padd=ONE, padd_rows=3, yplus_bound=ONE, padd_amax=ONE)
    _rejected(lib, name, _forward_args(name, **dict(plus, padd_amax=None)), E_NULL, slot)
    _rejected(lib, name, _forward_args(name, **dict(plus, y_plus=None)), E_NULL, slot)


def test_partial_reduce_rejections(lib):
    f = "mpf_ln_partial_reduce"
    ok = dict(partials=ONE, stride=_partial_bytes(5), rows=5, n_ln=3, out=ONE, stream=None)
    call = lambda **kw: list(dict(ok, **kw).values())
    _rejected(lib, f, call(partials=None), E_NULL, "ln_partial_reduce: NULL buffer")
    _rejected(lib, f, call(out=None), E_NULL, "ln_partial_reduce: NULL buffer")
    for bad in (dict(rows=0), dict(rows=-1), dict(n_ln=0), dict(n_ln=65536), dict(stride=_partial_bytes(5) + 2)):
        _rejected(lib, f, call(**bad), E_SHAPE, "ln_partial_reduce: bad sizes")


def test_no_rows_is_a_no_op_before_any_check(lib):
    for name in _TAIL:
        assert getattr(lib, name)(*[0 if k in ("rows", "bytes") else None for k in _HEAD + _TAIL[name]]) == 0, name
    for name in _FWD_TAIL:
        assert getattr(lib, name)(*[0 if k in ("t_dtype", "rows", "eps", "padd_rows") else None for k in _FWD + _FWD_TAIL[name]]) == 0, name


def test_size_queries_follow_the_grid_rule(lib):
    for rows in ROWS:
        assert lib.mpf_res_ln256_backward_workspace_bytes(rows) == _partial_bytes(rows)
        assert lib.mpf_res_ln256_backward_det_workspace_bytes(rows) == 256 + _partial_bytes(rows)
    assert _partial_bytes(1024) == 256 * 2048 and _partial_bytes(1025) == 257 * 2048 and _partial_bytes(4097) == 513 * 2048
    for rows in (0, -1):
        assert lib.mpf_res_ln256_backward_workspace_bytes(rows) == 0 and lib.mpf_res_ln256_backward_det_workspace_bytes(rows) == 0
