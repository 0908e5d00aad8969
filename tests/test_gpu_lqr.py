"""GPU: mgx_lqr_backward (ilqr.lqr_backward_fused) against the numpy box-QP Riccati recursion of
tests/boxqp_reference.py at sizes no model has and at soccer's and construction's, plain and
box-constrained; its mask, determinism, pivot report, fp32 accuracy and argument errors.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mujoco_gymnasium_environments_amd import cabi, ilqr
from mujoco_gymnasium_environments_amd.native import lib
from tests import boxqp_reference as bq
from tests.test_gpu_rollout import _batch, _np

pytestmark = pytest.mark.gpu

N, MU = 2, 0.5
SIZES = ((5, 3, 4), (80, 33, 3), (198, 33, 2))  # edge tiles; soccer's size; construction's (the workspace path)
ARGS = ("A", "B", "lx", "lxx", "lu", "luu", "lux", "Vx_T", "Vxx_T")


def _native(prec="f64"):
    return _batch("soccer", prec).native


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """The shared inputs of one size and the reference's plain and box passes per env (read-only)."""
    d = bq.make_inputs(n, m, T, N=N, seed=bq.SEED)
    return d, {box: [bq.reference(d, MU, box, e) for e in range(N)] for box in (False, True)}


def _dev(d, dtype=torch.float64):
    return {k: torch.tensor(v, dtype=dtype, device="cuda") for k, v in d.items()}


def _fused(native, t, box, **kw):
    lim = dict(lo=t["lo"], hi=t["hi"]) if box else {}
    return ilqr.lqr_backward_fused(native, *[t[k] for k in ARGS], MU, **lim, **kw)


@pytest.mark.parametrize("box", [False, True], ids=["plain", "box"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_fused_pass_matches_the_numpy_reference(size, box):
    d, refs = _case(*size)
    got = _fused(_native(), _dev(d), box)
    torch.cuda.synchronize()
    assert got.info.tolist() == [0] * N
    for e in range(N):
        ref = refs[box][e]
        margin, share, cond = bq.check_conditions(ref, box)
        k, K, free = _np(got.k_ff[e]), _np(got.gain[e]), _np(got.free[e])
        err = bq.compare(ref, k, K, _np(got.expected[e]), free)
        bq.check_kkt(ref, k, free, d["lo"][e] if box else None, d["hi"][e] if box else None)
        assert (K[free == 0] == 0).all()
        print(f"{size} {'box' if box else 'plain'} env {e}: error {err:.3g}, min margin {margin:.3g}, "
              f"clamped share {share:.2f}, cond {cond:.3g}")


def test_diagonal_terms_and_null_matrices():
    """lxx_diag / luu_diag with lxx = luu = NULL give what the dense diagonal matrices give, and a
    NULL lux what a zero one gives (the form ilqr.solve(backward="fused") uses)."""
    d, _ = _case(80, 33, 3)
    t = _dev(d)
    t["lux"] = torch.zeros_like(t["lux"])
    dense = _fused(_native(), t, True)
    diag = ilqr.lqr_backward_fused(_native(), t["A"], t["B"], t["lx"], None, t["lu"], None, None, t["Vx_T"], t["Vxx_T"], MU,
                                   lo=t["lo"], hi=t["hi"], lxx_diag=t["lxx_diag"], luu_diag=t["luu_diag"])
    torch.cuda.synchronize()
    scale = max(1.0, float(dense.gain.abs().max()), float(dense.k_ff.abs().max()))
    assert float((dense.k_ff - diag.k_ff).abs().max()) <= 1e-12 * scale
    assert float((dense.gain - diag.gain).abs().max()) <= 1e-12 * scale
    assert torch.equal(dense.free, diag.free) and diag.info.tolist() == [0] * N


def _sentinel_out(n, m, T, dtype=torch.float64):
    f = lambda *s: torch.full(s, -7.0, dtype=dtype, device="cuda")  # noqa: E731
    return ilqr.LqrBackward(f(N, T, m), f(N, T, m, n), f(N, 2), torch.full((N,), 77, dtype=torch.int32, device="cuda"),
                            torch.full((N, T, m), 9, dtype=torch.uint8, device="cuda"))


def test_mask_and_determinism():
    n, m, T = 5, 3, 4
    d, _ = _case(n, m, T)
    t = _dev(d)
    full = _fused(_native(), t, True)
    out = _fused(_native(), t, True, out=_sentinel_out(n, m, T), mask=torch.tensor([1, 0], dtype=torch.uint8, device="cuda"))
    again = _fused(_native(), t, True)
    torch.cuda.synchronize()
    sent = _sentinel_out(n, m, T)
    for f in out._fields:
        assert torch.equal(getattr(out, f)[0], getattr(full, f)[0]), f
        assert torch.equal(getattr(out, f)[1], getattr(sent, f)[1]), f  # the deselected env keeps the sentinel
        assert torch.equal(getattr(again, f), getattr(full, f)), f  # two calls, the same bits


def test_pivot_failure_is_reported_per_env():
    d, _ = _case(5, 3, 4)
    t = _dev(d)
    t["luu"] = t["luu"].clone()
    t["luu"][1] = -1e6 * torch.eye(3, dtype=torch.float64, device="cuda")
    for box in (False, True):
        got = _fused(_native(), t, box)
        torch.cuda.synchronize()
        assert got.info.tolist() == [0, 1], box
        assert bool(torch.isfinite(got.k_ff[0]).all()) and bool(torch.isfinite(got.gain[0]).all())


def test_fp32_error_against_the_torch_fp32_pass():
    """(80, 33, 3) on an f32 handle, the plain pass: the error against the float64 numpy reference is
    at most 8 x the error of the torch float32 pass on the same inputs. Both are float32 sums of
    equal length in different orders, so the bound scales alike and only the constant differs."""
    d, refs = _case(80, 33, 3)
    t = _dev(d, torch.float32)
    got = _fused(_native("f32"), t, False)
    tor = ilqr.lqr_backward(*[t[k] for k in ARGS], torch.full((N,), MU, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert got.k_ff.dtype == torch.float32 and got.info.tolist() == [0] * N

    def error(r, e):
        ref = refs[False][e]
        scale = max(1.0, np.abs(ref["K"]).max(), np.abs(ref["k"]).max())
        return max(np.abs(_np(r.k_ff[e]).astype(np.float64) - ref["k"]).max() / scale,
                   np.abs(_np(r.gain[e]).astype(np.float64) - ref["K"]).max() / scale,
                   np.abs(_np(r.expected[e]).astype(np.float64) - ref["expected"]).max() / max(1.0, np.abs(ref["expected"]).max()))
    for e in range(N):
        mine, theirs = error(got, e), error(tor, e)
        print(f"fp32 env {e}: fused error {mine:.3g}, torch float32 error {theirs:.3g}, bound {8 * theirs:.3g}")
        assert mine <= 8 * theirs


def test_argument_errors():
    n, m, T = 5, 3, 4
    d, _ = _case(n, m, T)
    t = _dev(d)
    native = _native()
    need = int(lib().mgx_lqr_backward_bytes(native.handle, n, m, N))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = _sentinel_out(n, m, T)
    mu = torch.full((N,), MU, dtype=torch.float64, device="cuda")

    def call(**change):
        io = cabi.MgxLqrIO()
        io.n, io.m, io.T, io.flags = n, m, T, cabi.MGX_LQR_BOX
        for f in ARGS + ("lo", "hi"):
            setattr(io, f, t[f].data_ptr())
        io.mu = mu.data_ptr()
        io.k_ff, io.gain, io.expected, io.info, io.free_set = (x.data_ptr() for x in out)
        io.workspace, io.workspace_bytes = ws.data_ptr(), need
        for f, v in change.items():
            setattr(io, f, v)
        return lib().mgx_lqr_backward(native.handle, C.byref(io), N, None, None)

    assert call(workspace_bytes=need - 1) == cabi.MGX_E_ARG
    assert call(m=cabi.MGX_LQR_MAX_CTRL + 1) == cabi.MGX_E_ARG
    assert call(T=0) == cabi.MGX_E_ARG
    assert call(lo=None) == cabi.MGX_E_ARG
    assert call(flags=4) == cabi.MGX_E_ARG
    assert int(lib().mgx_lqr_backward_bytes(native.handle, n, cabi.MGX_LQR_MAX_CTRL + 1, N)) == cabi.MGX_E_ARG
    torch.cuda.synchronize()
    sent = _sentinel_out(n, m, T)
    for f in out._fields:
        assert torch.equal(getattr(out, f), getattr(sent, f)), f  # a refused call writes nothing
    assert call() == 0  # and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert out.info.tolist() == [0] * N


def test_side_stream_and_mask_validation():
    """A call on a side stream, with inputs that need a contiguous copy (temporaries recorded on that
    stream), gives the bits of the call on the current stream; a mask of the wrong type is a ValueError."""
    d, _ = _case(5, 3, 4)
    t = _dev(d)
    full = _fused(_native(), t, True)
    torch.cuda.synchronize()
    strided = dict(t)
    strided["A"] = t["A"].transpose(2, 3).contiguous().transpose(2, 3)  # same values, not contiguous
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = _fused(_native(), strided, True, stream=side)
    side.synchronize()
    for f in got._fields:
        assert torch.equal(getattr(got, f), getattr(full, f)), f
    with pytest.raises(ValueError):
        _fused(_native(), t, True, mask=torch.ones(N, dtype=torch.bool, device="cuda"))
