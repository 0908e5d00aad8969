"""CPU: ilqr.lqr_backward against the numpy Riccati recursion (tests/feedback_reference.py), and
ilqr.solve driven by a linear stand-in system on CPU tensors, where one iteration is exact LQR.
"""
import types

import numpy as np
import torch

from mujoco_gymnasium_environments_amd import ilqr
from tests import feedback_reference as fb

N, NX, NU, T = 3, 4, 2, 6  # NX = 2 nv


def _system_matrices(seed):
    rng = np.random.default_rng(seed)
    A = np.eye(NX) + 0.1 * rng.normal(size=(N, T, NX, NX))
    B = rng.normal(size=(N, T, NX, NU))
    return A, B


def _cost_terms(rng):
    w_x, w_xf, w_u = rng.uniform(0.5, 2, NX), rng.uniform(1, 4, NX), rng.uniform(0.5, 2, NU)
    return w_x, w_xf, w_u


def test_lqr_backward_matches_numpy_riccati():
    A, B = _system_matrices(1)
    rng = np.random.default_rng(2)
    w_x, w_xf, w_u = _cost_terms(rng)
    lx, lu = rng.normal(size=(N, T, NX)), rng.normal(size=(N, T, NU))
    lux = 0.1 * rng.normal(size=(N, T, NU, NX))
    Vx = rng.normal(size=(N, NX))
    lxx, luu, Vxx = np.tile(np.diag(w_x), (N, T, 1, 1)), np.tile(np.diag(w_u), (N, T, 1, 1)), np.tile(np.diag(w_xf), (N, 1, 1))
    tt = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    for mu in (0.0, 0.5):
        got = ilqr.lqr_backward(tt(A), tt(B), tt(lx), tt(lxx), tt(lu), tt(luu), tt(lux), tt(Vx), tt(Vxx),
                                torch.full((N,), mu, dtype=torch.float64))
        assert int(got.info.abs().max()) == 0
        for e in range(N):
            k, K, exp, conds = fb.lqr_backward(A[e], B[e], lx[e], lxx[e], lu[e], luu[e], lux[e], Vx[e], Vxx[e], mu)
            # the input may not hide a failure: the reference's Q_uu stays well conditioned
            assert max(conds) < 1e3, conds
            scale = max(1.0, np.abs(K).max(), np.abs(k).max())
            assert np.abs(got.k_ff[e].numpy() - k).max() <= 1e-9 * scale
            assert np.abs(got.gain[e].numpy() - K).max() <= 1e-9 * scale
            assert np.abs(got.expected[e].numpy() - exp).max() <= 1e-9 * max(1.0, np.abs(exp).max())
    # a non-positive pivot is reported per env, not raised
    luu_bad = luu.copy()
    luu_bad[1] = -1e6 * np.eye(NU)
    got = ilqr.lqr_backward(tt(A), tt(B), tt(lx), tt(lxx), tt(lu), tt(luu_bad), tt(lux), tt(Vx), tt(Vxx), 0.0)
    assert got.info.tolist()[0] == 0 and got.info.tolist()[1] != 0 and got.info.tolist()[2] == 0


class LinearSystem:
    """x_(t+1) = A_t x_t + B_t u_t on rows [time, x]: the duck type ilqr.solve asks for, without
    quaternions (state_difference subtracts) and without control limits."""

    def __init__(self, A, B):
        self.A, self.B = torch.tensor(A), torch.tensor(B)
        self.model = types.SimpleNamespace(nv=NX // 2, nu=NU)
        self.state_size = 1 + NX
        self.rollouts = 0

    def state_difference(self, xa, xb):
        return xa[..., 1:] - xb[..., 1:]

    def transition_fd_along(self, state0, ctrl, warmstart=None, nsub=1, centered=False):
        return types.SimpleNamespace(A=self.A, B=self.B)

    def rollout_feedback(self, u_nom, x_nom=None, k_ff=None, alpha=None, gain=None, initial_state=None,
                         initial_warmstart=None, nsub=1):
        self.rollouts += 1
        K = initial_state.shape[1]
        x = initial_state.clone()
        states, ctrls = [], []
        for t in range(T):
            u = u_nom[:, None, t].expand(N, K, NU).clone()
            if k_ff is not None:
                u = u + alpha[:, :, None] * k_ff[:, None, t]
            if gain is not None:
                u = u + torch.einsum("nij,nkj->nki", gain[:, t], x[..., 1:] - x_nom[:, None, t, 1:])
            nxt = torch.einsum("nij,nkj->nki", self.A[:, t], x[..., 1:]) + torch.einsum("nij,nkj->nki", self.B[:, t], u)
            x = torch.cat([x[..., :1] + 1.0, nxt], dim=-1)
            states.append(x)
            ctrls.append(u)
        return types.SimpleNamespace(state=torch.stack(states, 2), ctrl=torch.stack(ctrls, 2),
                                     warmstart=torch.zeros(N, K, T, NX // 2, dtype=torch.float64),
                                     n_done=torch.full((N, K), T, dtype=torch.int32))


def _lqr_optimum(A, B, x0, goal, w_x, w_xf, w_u):
    """The minimiser of the quadratic cost of one env as a dense least-squares problem in u."""
    def traj(u):
        xs, x = [x0], x0
        for t in range(T):
            x = A[t] @ x + B[t] @ u[t]
            xs.append(x)
        return np.array(xs)
    base = traj(np.zeros((T, NU)))
    cols = []
    for i in range(T * NU):
        e = np.zeros(T * NU)
        e[i] = 1.0
        cols.append((traj(e.reshape(T, NU)) - base).reshape(-1))
    G = np.array(cols).T  # d(states)/du
    W = np.concatenate([np.tile(w_x, T), w_xf])
    r = (base - goal).reshape(-1)
    H = G.T @ (W[:, None] * G) + np.diag(np.tile(w_u, T))
    u = np.linalg.solve(H, -G.T @ (W * r)).reshape(T, NU)
    dx = traj(u) - goal
    return u, 0.5 * (w_x * dx[:T] ** 2).sum() + 0.5 * (w_u * u ** 2).sum() + 0.5 * (w_xf * dx[T] ** 2).sum()


def _problem(seed=3):
    rng = np.random.default_rng(seed)
    w = _cost_terms(rng)
    x0 = np.concatenate([np.zeros((N, 1)), rng.normal(size=(N, NX))], axis=1)
    goal = np.concatenate([np.zeros((N, 1)), rng.normal(size=(N, NX))], axis=1)
    return x0, goal, w


def test_one_iteration_is_exact_lqr():
    A, B = _system_matrices(1)
    x0, goal, (w_x, w_xf, w_u) = _problem()
    sys = LinearSystem(A, B)
    prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u)
    one = ilqr.solve(sys, prob, alphas=(1,), mu0=0.0, max_iter=1)
    assert one.status.tolist() == [ilqr.MAX_ITER] * N and one.iters.tolist() == [1] * N
    assert one.cost_history.shape == (2, N)
    for e in range(N):
        u, J = _lqr_optimum(A[e], B[e], x0[e, 1:], goal[e, 1:], w_x, w_xf, w_u)
        assert np.abs(one.ctrl[e].numpy() - u).max() <= 1e-9 * max(1.0, np.abs(u).max())
        assert abs(float(one.cost[e]) - J) <= 1e-9 * J
        assert float(one.cost_history[1, e]) < float(one.cost_history[0, e])
    # a second iteration has nothing left to gain: converged, the cost where it was
    two = ilqr.solve(sys, prob, alphas=(1,), mu0=0.0, max_iter=5, tol=1e-6)
    assert two.status.tolist() == [ilqr.CONVERGED] * N and two.iters.tolist() == [2] * N
    assert (torch.abs(two.cost - one.cost) <= 1e-6 * one.cost).all()
    assert (two.cost_history[1:] <= two.cost_history[:-1]).all()
    # the result is the rollout of its own controls
    again = sys.rollout_feedback(two.ctrl, initial_state=torch.tensor(x0)[:, None, :])
    assert torch.equal(again.state[:, 0], two.state[:, 1:])


def test_no_step_accepted_ends_at_the_mu_cap():
    A, B = _system_matrices(1)
    x0, goal, (w_x, w_xf, w_u) = _problem()
    sys = LinearSystem(A, B)
    prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u)
    res = ilqr.solve(sys, prob, alphas=(0,), mu0=0.0, max_iter=40)
    assert res.status.tolist() == [ilqr.STALLED] * N
    assert torch.equal(res.ctrl, torch.zeros(N, T, NU, dtype=torch.float64))
    assert torch.equal(res.cost_history[0], res.cost) and (res.cost_history == res.cost_history[0]).all()
    first = sys.rollout_feedback(torch.zeros(N, T, NU, dtype=torch.float64), initial_state=torch.tensor(x0)[:, None, :])
    assert torch.equal(res.state[:, 1:], first.state[:, 0])
