"""CPU: the box-constrained backward pass of ilqr.lqr_backward against the numpy box-QP Riccati
recursion of tests/boxqp_reference.py, its KKT conditions, the +-inf case, the C-ABI of
mgx_lqr_backward (include/mgx.h against cabi.py and native.py), and ilqr.solve(box=True) on a linear
stand-in with control limits against the bound-constrained least-squares optimum
(scipy.optimize.lsq_linear).
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from mujoco_gymnasium_environments_amd import cabi, ilqr, native
from tests import boxqp_reference as bq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("A", "B", "lx", "lxx", "lu", "luu", "lux", "Vx_T", "Vxx_T")
tt = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731


def test_lqr_io_layout_matches_the_header(tmp_path):
    """mgx_lqr_io's size and every field offset, and the MGX_LQR_* constants, of include/mgx.h
    against cabi.py; the ABI version is unchanged (the section only adds)."""
    fields = [f for f, _ in cabi.MgxLqrIO._fields_]
    prog = tmp_path / "lqr.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                    'int main(void){printf("%zu %d %d %d", sizeof(mgx_lqr_io), MGX_LQR_BOX, MGX_LQR_MAX_CTRL, MGX_ABI_VERSION);\n'
                    + "".join(f'printf(" %zu", offsetof(mgx_lqr_io, {f}));\n' for f in fields) + 'return 0;}\n')
    exe = tmp_path / "lqr"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[:4] == [C.sizeof(cabi.MgxLqrIO), cabi.MGX_LQR_BOX, cabi.MGX_LQR_MAX_CTRL, cabi.MGX_ABI_VERSION]
    assert cabi.MGX_ABI_VERSION == 6
    assert vals[4:] == [getattr(cabi.MgxLqrIO, f).offset for f in fields]
    assert "mgx_lqr_backward" in native.EXPORTS and "mgx_lqr_backward_bytes" in native.EXPORTS
    assert "mgx_lqr.hip" in native.SOURCES and "mgx_lqr.h" in native.TU_HEADERS["mgx_lqr.hip"]
    assert hasattr(native.lib(), "mgx_lqr_backward")


def test_box_pass_matches_the_numpy_reference():
    """(n, m, T) = (5, 3, 4), two envs, mu = 0.5: k, K, expected within 1e-9 max(1, |k|, |K|), equal
    free sets, KKT on the returned k, and the inputs' conditions (nothing is excluded)."""
    d = bq.make_inputs(5, 3, 4, seed=bq.SEED)
    got = ilqr.lqr_backward(*[tt(d[k]) for k in ARGS], torch.full((2,), 0.5, dtype=torch.float64), lo=tt(d["lo"]), hi=tt(d["hi"]))
    assert got.info.tolist() == [0, 0] and got.free.dtype == torch.bool
    for e in range(2):
        ref = bq.reference(d, 0.5, True, e)
        margin, share, cond = bq.check_conditions(ref, True)
        k, K, free = got.k_ff[e].numpy(), got.gain[e].numpy(), got.free[e].numpy()
        err = bq.compare(ref, k, K, got.expected[e].numpy(), free)
        bq.check_kkt(ref, k, free, d["lo"][e], d["hi"][e])
        assert (K[~free] == 0).all()
        print(f"env {e}: error {err:.3g}, min margin {margin:.3g}, clamped share {share:.2f}, cond {cond:.3g}")


def test_infinite_bounds_give_the_unconstrained_pass():
    d = bq.make_inputs(5, 3, 4, seed=bq.SEED)
    mu = torch.full((2,), 0.5, dtype=torch.float64)
    plain = ilqr.lqr_backward(*[tt(d[k]) for k in ARGS], mu)
    assert plain.free is None  # without bounds the pass is the one it was
    inf = torch.full((2, 4, 3), float("inf"), dtype=torch.float64)
    got = ilqr.lqr_backward(*[tt(d[k]) for k in ARGS], mu, lo=-inf, hi=inf)
    scale = max(1.0, float(plain.k_ff.abs().max()), float(plain.gain.abs().max()))
    assert float((got.k_ff - plain.k_ff).abs().max()) <= 1e-12 * scale
    assert float((got.gain - plain.gain).abs().max()) <= 1e-12 * scale
    assert bool(got.free.all()) and got.info.tolist() == [0, 0]
    one_sided = ilqr.lqr_backward(*[tt(d[k]) for k in ARGS], mu, hi=inf)
    assert torch.equal(one_sided.k_ff, got.k_ff) and torch.equal(one_sided.gain, got.gain)


def test_box_pass_reports_a_failed_pivot_per_env():
    d = bq.make_inputs(5, 3, 4, seed=bq.SEED)
    d["luu"] = d["luu"].copy()
    d["luu"][1] = -1e6 * np.eye(3)
    got = ilqr.lqr_backward(*[tt(d[k]) for k in ARGS], 0.0, lo=tt(d["lo"]), hi=tt(d["hi"]))
    assert got.info.tolist()[0] == 0 and got.info.tolist()[1] & ilqr.PIVOT
    assert bool(torch.isfinite(got.k_ff[0]).all())


# ------------------------------------------------------------------ the solver on a linear stand-in
N, NX, NU, T = 3, 4, 2, 6  # the sizes of tests/test_ilqr_cpu.py
LIMIT = 0.15


def _system_matrices(seed):
    rng = np.random.default_rng(seed)
    return np.eye(NX) + 0.1 * rng.normal(size=(N, T, NX, NX)), rng.normal(size=(N, T, NX, NU))


def _problem(seed):
    rng = np.random.default_rng(seed)  # the draws of tests/test_ilqr_cpu.py's _problem, in its order
    w = rng.uniform(0.5, 2, NX), rng.uniform(1, 4, NX), rng.uniform(0.5, 2, NU)
    x0 = np.concatenate([np.zeros((N, 1)), rng.normal(size=(N, NX))], axis=1)
    goal = np.concatenate([np.zeros((N, 1)), rng.normal(size=(N, NX))], axis=1)
    return x0, goal, w


class LinearSystem:
    """LinearSystem of tests/test_ilqr_cpu.py with control limits: every actuator is limited to
    +-LIMIT and rollout_feedback clamps the control it applies, as the library's does."""

    def __init__(self, A, B):
        self.A, self.B = torch.tensor(A), torch.tensor(B)
        self.model = types.SimpleNamespace(nv=NX // 2, nu=NU, actuator_ctrllimited=np.ones(NU, dtype=np.int32),
                                           actuator_ctrlrange=np.tile([-LIMIT, LIMIT], (NU, 1)))
        self.state_size = 1 + NX

    def state_difference(self, xa, xb):
        return xa[..., 1:] - xb[..., 1:]

    def transition_fd_along(self, state0, ctrl, warmstart=None, nsub=1, centered=False):
        return types.SimpleNamespace(A=self.A, B=self.B)

    def rollout_feedback(self, u_nom, x_nom=None, k_ff=None, alpha=None, gain=None, initial_state=None,
                         initial_warmstart=None, nsub=1):
        K = initial_state.shape[1]
        x = initial_state.clone()
        states, ctrls = [], []
        for t in range(T):
            u = u_nom[:, None, t].expand(N, K, NU).clone()
            if k_ff is not None:
                u = u + alpha[:, :, None] * k_ff[:, None, t]
            if gain is not None:
                u = u + torch.einsum("nij,nkj->nki", gain[:, t], x[..., 1:] - x_nom[:, None, t, 1:])
            u = u.clamp(-LIMIT, LIMIT)
            nxt = torch.einsum("nij,nkj->nki", self.A[:, t], x[..., 1:]) + torch.einsum("nij,nkj->nki", self.B[:, t], u)
            x = torch.cat([x[..., :1] + 1.0, nxt], dim=-1)
            states.append(x)
            ctrls.append(u)
        return types.SimpleNamespace(state=torch.stack(states, 2), ctrl=torch.stack(ctrls, 2),
                                     warmstart=torch.zeros(N, K, T, NX // 2, dtype=torch.float64),
                                     n_done=torch.full((N, K), T, dtype=torch.int32))


def _bounded_optimum(A, B, x0, goal, w_x, w_xf, w_u):
    """The minimiser of one env's cost over |u| <= LIMIT: a bounded linear least-squares problem."""
    from scipy.optimize import lsq_linear

    def traj(u):
        xs, x = [x0], x0
        for t in range(T):
            x = A[t] @ x + B[t] @ u[t]
            xs.append(x)
        return np.array(xs)
    base = traj(np.zeros((T, NU)))
    G = np.array([(traj(e.reshape(T, NU)) - base).reshape(-1) for e in np.eye(T * NU)]).T
    W = np.concatenate([np.tile(w_x, T), w_xf])
    M = np.concatenate([np.sqrt(W)[:, None] * G, np.diag(np.sqrt(np.tile(w_u, T)))])
    rhs = np.concatenate([-np.sqrt(W) * (base - goal).reshape(-1), np.zeros(T * NU)])
    sol = lsq_linear(M, rhs, bounds=(-LIMIT, LIMIT), method="bvls", tol=1e-15, max_iter=1000)
    u = sol.x.reshape(T, NU)
    dx = traj(u) - goal
    return u, 0.5 * (w_x * dx[:T] ** 2).sum() + 0.5 * (w_u * u ** 2).sum() + 0.5 * (w_xf * dx[T] ** 2).sum()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_box_solve_reaches_the_bounded_optimum(seed):
    """ilqr.solve(box=True) reaches the lsq_linear optimum (cost within 1e-8 relative, controls
    within 1e-6, in every env) in at most 10 iterations, and the clamp-only solver, which can never
    be below it, ends at least 1 % above it in some env of every problem (a seed is one problem of
    N = 3 envs, drawn as tests/test_ilqr_cpu.py draws its own). Per env the clamp-only gap is, with
    the solver's Levenberg schedule, 2.11, 0.01, 5.32 % (seed 0), 1.00, 1.80, 0.13 % (seed 1) and
    11.66, 7.50, 2.40 % (seed 2): an env whose optimum barely saturates (seed 0, env 1: 8 % of its
    controls) has nothing to gain from the bounds, and one that saturates almost everywhere (seed 1,
    env 2: 83 %) little, so the 1 % is not asked of every env. This is the capability: without
    box=True the first assertion cannot hold."""
    A, B = _system_matrices(seed)
    x0, goal, (w_x, w_xf, w_u) = _problem(seed)
    prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u)
    box = ilqr.solve(LinearSystem(A, B), prob, mu0=0.0, max_iter=10, tol=1e-14, box=True)
    clamp = ilqr.solve(LinearSystem(A, B), prob, mu0=0.0, max_iter=10, tol=1e-14)
    assert box.free.shape == (N, T, NU) and box.free.dtype == torch.bool
    assert int(box.iters.max()) <= 10 and float(box.ctrl.abs().max()) <= LIMIT
    assert (box.cost_history[1:] <= box.cost_history[:-1]).all()
    gaps = []
    for e in range(N):
        u, J = _bounded_optimum(A[e], B[e], x0[e, 1:], goal[e, 1:], w_x, w_xf, w_u)
        gaps.append(float(clamp.cost[e]) / J - 1)
        saturated = float((np.abs(u) == LIMIT).mean())
        print(f"seed {seed} env {e}: optimum {J:.9g} box {float(box.cost[e]):.9g} clamp-only {float(clamp.cost[e]):.9g} "
              f"(+{(float(clamp.cost[e]) / J - 1) * 100:.2f} %), iters {int(box.iters[e])}, saturated {saturated:.2f}")
        assert abs(float(box.cost[e]) - J) <= 1e-8 * J
        assert np.abs(box.ctrl[e].numpy() - u).max() <= 1e-6
        assert float(clamp.cost[e]) >= J * (1 - 1e-12)
        # a control the last backward pass clamped has no feedback
        assert (box.gain[e][~box.free[e]] == 0).all()
    assert max(gaps) >= 0.01, gaps


def test_default_keywords_change_nothing():
    A, B = _system_matrices(0)
    x0, goal, (w_x, w_xf, w_u) = _problem(0)
    prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u)
    a = ilqr.solve(LinearSystem(A, B), prob, max_iter=4)
    b = ilqr.solve(LinearSystem(A, B), prob, max_iter=4, box=False, backward="torch")
    for f in a._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert bool(a.free.all())
    with pytest.raises(ValueError):
        ilqr.solve(LinearSystem(A, B), prob, backward="fused")  # no library handle
    with pytest.raises(ValueError):
        ilqr.solve(LinearSystem(A, B), prob, backward="eager")
