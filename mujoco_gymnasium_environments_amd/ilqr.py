"""Batched iLQR on top of the closed-loop rollouts (``rollout_feedback``), the trajectory
linearisation (``transition_fd_along``) and the state manifold (``state_difference``).

``lqr_backward`` is the Riccati recursion and ``solve`` the driver; ``IlqrMethods`` gives
:class:`~.batch.PhysicsBatch` its ``solve_ilqr`` and ``IlqrForwarding`` the ``*VectorEnv`` classes
theirs.

The backward pass is batched torch ON PURPOSE: per iteration it is T small dense solves per env
(nu x nu Cholesky factors and a handful of 2nv x 2nv products), beside the (1 + 2nv + nu) T physics
steps per env of the finite-difference linearisation and the K T steps of the line search, which
run in the library's HIP kernels. It is plumbing, not the hot path, and it runs on CPU tensors as
well, so a CPU stand-in for the system can drive the solver in the tests.

The cost is the diagonal quadratic

    J = sum_{t<T} 1/2 (dx_t' diag(w_x) dx_t + u_t' diag(w_u) u_t) + 1/2 dx_T' diag(w_xf) dx_T,
    dx_t = state_difference(x_t, goal_t),

and its derivatives take d(dx)/dx = I: the Gauss-Newton form, exact for models without quaternion
joints and near the goal (the Jacobian of the rotation-vector difference is I + O(|dx|)).

With ``sensor_goal`` / ``w_s`` / ``w_sf`` the cost adds a residual on the sensors,

    sum_{t=1..T-1} 1/2 r_t' diag(w_s) r_t + 1/2 r_T' diag(w_sf) r_T,   r_t = s(x_t) - s*_t,

x_t the state after recorded step t (x_0 is fixed: its term is a constant and is left out) and s the
``sensordata()`` row. The line search reads r_t from the closed-loop rollout's own ``sensordata``
output; the backward pass takes the Gauss-Newton terms ``C_t' (w o r_t)`` and ``C_t' diag(w) C_t``
with ``C_t = ds/dx`` from ``sensor_fd_along`` at the trajectory's states (``only=("C",)``: no ctrl
columns). Rows of accelerometer, force, torque and touch sensors may not be weighted: they read
``ctrl`` and the solver, so a cost on them couples x_{t+1} with u_t, which this backward pass does
not model (and the rollout records them with the ctrl of the step that led to x_t).
Not provided: any other cost, costs on acceleration-stage sensors, constraints beyond the control
clamp of ``rollout_feedback`` and box-DDP.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import torch

DEFAULT_ALPHAS = (1, .5, .25, .125, .0625, .03125, .015625, .0078125)
MU_MIN, MU_MAX = 1e-6, 1e10  # the first nonzero Levenberg parameter, and the cap that ends an env with status 2

CONVERGED, MAX_ITER, STALLED = 0, 1, 2

LqrBackward = namedtuple("LqrBackward", "k_ff gain expected info")
IlqrResult = namedtuple("IlqrResult", "ctrl state gain k_ff cost cost_history iters status")


def lqr_backward(A, B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu):
    """The time-varying LQR backward pass, batched over the leading dim N, looping over T.

    A [N, T, n, n], B [N, T, n, m]; the cost's derivatives lx [N, T, n], lxx [N, T, n, n],
    lu [N, T, m], luu [N, T, m, m], lux [N, T, m, n]; the terminal Vx_T [N, n], Vxx_T [N, n, n];
    mu [N] (or a scalar): the Levenberg parameter, relative to the size of Q_uu: the gains (only)
    come from Q_uu + mu max(1, tr Q_uu / m) I. The value function is that of the policy
    du = k + K dx itself (closed-loop form), which keeps V_xx positive semi-definite in floating
    point even where A has eigenvalues of 1e5, as the stiff contacts of the assembly scene give.
    Returns ``LqrBackward(k_ff [N, T, m], gain [N, T, m, n], expected [N, 2], info [N])``: the step
    ``du_t = alpha k_ff_t + gain_t dx_t`` is expected to lower the cost by
    ``-(alpha expected[:, 0] + alpha^2 expected[:, 1])``; ``info`` is nonzero where some Q_uu + mu I
    had a non-positive pivot (``torch.linalg.cholesky_ex``): that env's gains are meaningless."""
    N, T, n, m = B.shape
    mu = torch.as_tensor(mu, dtype=A.dtype, device=A.device).expand(N)
    eye = torch.eye(m, dtype=A.dtype, device=A.device)
    Vx, Vxx = Vx_T, Vxx_T
    k_ff = torch.zeros(N, T, m, dtype=A.dtype, device=A.device)
    gain = torch.zeros(N, T, m, n, dtype=A.dtype, device=A.device)
    expected = torch.zeros(N, 2, dtype=A.dtype, device=A.device)
    info = torch.zeros(N, dtype=torch.int32, device=A.device)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], B[:, t]
        AtT, BtT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qu = lu[:, t] + (BtT @ Vx[:, :, None])[:, :, 0]
        Qux = lux[:, t] + BtT @ Vxx @ At
        Quu = luu[:, t] + BtT @ Vxx @ Bt
        scale = torch.clamp(torch.diagonal(Quu, dim1=1, dim2=2).mean(1), min=1.0)
        L, inf_t = torch.linalg.cholesky_ex(Quu + (mu * scale)[:, None, None] * eye)
        info = torch.maximum(info, inf_t.to(torch.int32))
        kK = -torch.cholesky_solve(torch.cat([Qu[:, :, None], Qux], dim=2), L)
        k, K = kK[:, :, 0], kK[:, :, 1:]
        KT = K.transpose(1, 2)
        expected[:, 0] += (k * Qu).sum(1)
        expected[:, 1] += 0.5 * (k * (Quu @ k[:, :, None])[:, :, 0]).sum(1)
        # the cost-to-go of the policy du = k + K dx under the model, in the closed-loop form: a sum
        # of congruences, so Vxx stays positive semi-definite in floating point whatever the gains
        Acl = At + Bt @ K
        AclT = Acl.transpose(1, 2)
        luxT = lux[:, t].transpose(1, 2)
        Bk = (Bt @ k[:, :, None])[:, :, 0]
        Vx = (lx[:, t] + (KT @ (lu[:, t] + (luu[:, t] @ k[:, :, None])[:, :, 0])[:, :, None])[:, :, 0]
              + (luxT @ k[:, :, None])[:, :, 0] + (AclT @ (Vx + (Vxx @ Bk[:, :, None])[:, :, 0])[:, :, None])[:, :, 0])
        Vxx = lxx[:, t] + KT @ luu[:, t] @ K + KT @ lux[:, t] + luxT @ K + AclT @ Vxx @ Acl
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        k_ff[:, t], gain[:, t] = k, K
    return LqrBackward(k_ff, gain, expected, info)


class IlqrProblem:
    """x0 [N, nstate] (the start), goal [N, nstate] or [N, T + 1, nstate], the horizon T, the
    weights w_x, w_xf [2nv] and w_u [nu] (each [n] or [N, n]) and u_init [N, T, nu] (None: zeros).
    The sensor residual: sensor_goal [N, ns] or [N, T, ns] (row t - 1 is s*_t, the goal of the state
    after recorded step t) and the weights w_s, w_sf [ns] or [N, ns] (None: zeros); all three None:
    no sensor cost."""

    def __init__(self, x0, goal, horizon, w_x, w_xf, w_u, u_init=None, sensor_goal=None, w_s=None, w_sf=None):
        self.x0, self.goal, self.horizon = x0, goal, int(horizon)
        self.w_x, self.w_xf, self.w_u, self.u_init = w_x, w_xf, w_u, u_init
        self.sensor_goal, self.w_s, self.w_sf = sensor_goal, w_s, w_sf


def trajectory_cost(system, problem, state, ctrl, w):
    """J [..] of trajectories state [N, ..., T + 1, nstate] under ctrl [N, ..., T, nu] (the cost of
    the module docstring), and dx [N, ..., T + 1, 2nv]. ``w`` = (w_x, w_xf, w_u) as [N, n]."""
    N, T = state.shape[0], problem.horizon
    goal = problem.goal
    goal = goal[:, None, :] if goal.dim() == 2 else goal
    extra = state.dim() - 3
    goal = goal.reshape((N,) + (1,) * extra + tuple(goal.shape[1:]))
    dx = system.state_difference(state.contiguous(), goal)
    lead = lambda x: x.reshape((N,) + (1,) * (extra + 1) + (x.shape[-1],))  # noqa: E731
    w_x, w_xf, w_u = (lead(x) for x in w)
    run = 0.5 * (w_x * dx[..., :T, :] ** 2).sum((-1, -2)) + 0.5 * (w_u * ctrl ** 2).sum((-1, -2))
    return run + 0.5 * (w_xf[..., 0, :] * dx[..., T, :] ** 2).sum(-1), dx


ACC_SENSOR_TYPES = ("accelerometer", "force", "torque", "touch")


def sensor_weights(model, problem, N, dtype, device):
    """(sensor_goal [N, 1 | T, ns], w_s [N, ns], w_sf [N, ns]) of a problem with a sensor cost.
    ValueError for a nonzero weight on a row of an acceleration-stage sensor, naming the sensor."""
    from .mjcf import SENSOR_TYPES
    ns, T = int(model.nsensordata), problem.horizon
    if problem.sensor_goal is None:
        raise ValueError("w_s / w_sf need a sensor_goal")
    goal = torch.as_tensor(problem.sensor_goal, dtype=dtype, device=device)
    if tuple(goal.shape) == (N, ns):
        goal = goal[:, None, :]
    elif tuple(goal.shape) != (N, T, ns):
        raise ValueError(f"sensor_goal must be [N, ns] or [N, T, ns] = {[N, T, ns]}, got {tuple(goal.shape)}")
    zero = torch.zeros(ns, dtype=dtype, device=device)
    w_s, w_sf = (torch.as_tensor(zero if x is None else x, dtype=dtype, device=device).expand(N, ns).contiguous()
                 for x in (problem.w_s, problem.w_sf))
    used = ((w_s != 0) | (w_sf != 0)).any(0).cpu()
    for name, typ, adr, dim in zip(model.sensor_names, model.sensor_type, model.sensor_adr, model.sensor_dim):
        if SENSOR_TYPES[int(typ)] in ACC_SENSOR_TYPES and bool(used[int(adr):int(adr) + int(dim)].any()):
            raise ValueError(f"sensor {name!r} ({SENSOR_TYPES[int(typ)]}) reads ctrl and the solver: a cost on it "
                             f"couples x_(t+1) with u_t, which the backward pass does not model; its weights must be 0")
    return goal, w_s, w_sf


def sensor_cost(sens, sw):
    """(J_s [..], r [N, ..., T, ns]) of recorded sensordata sens [N, ..., T, ns] (row t - 1: the
    sensors at the state after recorded step t); ``sw`` = (goal, w_s, w_sf) of ``sensor_weights``."""
    goal, w_s, w_sf = sw
    N, extra = sens.shape[0], sens.dim() - 3
    lead = lambda x: x.reshape((N,) + (1,) * extra + tuple(x.shape[1:]))  # noqa: E731
    r = sens - lead(goal)
    run = 0.5 * (lead(w_s[:, None, :]) * r[..., :-1, :] ** 2).sum((-1, -2))
    return run + 0.5 * (lead(w_sf) * r[..., -1, :] ** 2).sum(-1), r


def solve(system, problem: IlqrProblem, nsub: int = 1, alphas: Sequence[float] = DEFAULT_ALPHAS, mu0: float = 1e-6,
          mu_factor: float = 10.0, max_iter: int = 20, tol: float = 1e-6, centered: bool = False) -> IlqrResult:
    """iLQR for every env of ``system`` at once. ``system`` is duck-typed: ``rollout_feedback``,
    ``transition_fd_along``, ``state_difference``, ``state_size`` and ``model.nv`` / ``model.nu`` as
    :class:`~.batch.PhysicsBatch` has them. One iteration:

    1. linearise along the current trajectory from its recorded warm starts;
    2. ``lqr_backward`` with Levenberg parameter mu on Q_uu; a non-positive pivot raises that env's
       mu (to at least 1e-6; by ``mu_factor``, and by one more power of it for every rise in a row,
       the schedule of Tassa, Erez and Todorov 2012) and repeats the pass;
    3. ONE ``rollout_feedback`` call whose K rollouts are the step sizes ``alphas``: the line search;
    4. the costs from ``state_difference``; a rollout that diverged (n_done < T) costs +inf;
    5. per env the best alpha is accepted if its cost is lower (mu falls, by the same schedule);
       otherwise the trajectory is kept and mu raised.

    An env ends with status 0 when an accepted step lowered the cost by less than ``tol`` relative,
    or when, with no rejection since the last accepted step, the decrease the quadratic model expects
    of the full step is below ``tol`` relative; with status 2 when mu passes 1e10 without an accepted
    step; with status 1 after ``max_iter`` iterations. Returns ``IlqrResult(ctrl [N, T, nu], state
    [N, T + 1, nstate], gain [N, T, nu, 2nv], k_ff [N, T, nu], cost [N], cost_history [iters + 1, N],
    iters [N], status [N])``: ``state`` is what ``ctrl`` produces from ``x0`` (the applied, clamped
    control), ``gain`` and ``k_ff`` belong to the last accepted step. Nothing is written to the
    system's state.

    A problem with a sensor cost (module docstring) also needs ``sensor_fd_along``, the
    ``sensordata`` output of ``rollout_feedback`` and the model's sensor tables; without one none
    of them is touched and the result is bit for bit that of the plain solve."""
    x0 = problem.x0
    N, T, ns = x0.shape[0], problem.horizon, system.state_size
    nv, nu = int(system.model.nv), int(system.model.nu)
    dt, dev = x0.dtype, x0.device
    K = len(alphas)
    w = tuple(torch.as_tensor(x, dtype=dt, device=dev).expand(N, n).contiguous()
              for x, n in ((problem.w_x, 2 * nv), (problem.w_xf, 2 * nv), (problem.w_u, nu)))
    alpha = torch.tensor([float(a) for a in alphas], dtype=dt, device=dev).repeat(N, 1).contiguous()
    u = torch.zeros(N, T, nu, dtype=dt, device=dev) if problem.u_init is None else problem.u_init.to(dt).contiguous()
    inf = torch.tensor(float("inf"), dtype=dt, device=dev)
    sw = None
    if problem.sensor_goal is not None or problem.w_s is not None or problem.w_sf is not None:
        sw = sensor_weights(system.model, problem, N, dt, dev)
    rec = dict(sensordata=True) if sw else {}  # the rollouts record the sensors only for a sensor cost

    r = system.rollout_feedback(u, initial_state=x0[:, None, :].contiguous(), nsub=nsub, **rec)
    state = torch.cat([x0[:, None, :], r.state[:, 0]], dim=1)
    ctrl, warm = r.ctrl[:, 0].clone(), r.warmstart[:, 0].clone()
    cost, _ = trajectory_cost(system, problem, state, ctrl, w)
    if sw:
        sens = r.sensordata[:, 0].clone()
        cost = cost + sensor_cost(sens, sw)[0]
    cost = torch.where(r.n_done[:, 0] < T, inf, cost)
    k_ff = torch.zeros(N, T, nu, dtype=dt, device=dev)
    gain = torch.zeros(N, T, nu, 2 * nv, dtype=dt, device=dev)
    mu = torch.full((N,), float(mu0), dtype=dt, device=dev)
    status = torch.full((N,), MAX_ITER, dtype=torch.int32, device=dev)
    iters = torch.zeros(N, dtype=torch.int32, device=dev)
    active = torch.ones(N, dtype=torch.bool, device=dev)
    fresh = torch.ones(N, dtype=torch.bool, device=dev)  # no rejection since the last accepted step
    history = [cost.clone()]
    eye_x = torch.eye(2 * nv, dtype=dt, device=dev)
    eye_u = torch.eye(nu, dtype=dt, device=dev)
    x0k = x0[:, None, :].repeat(1, K, 1).contiguous()
    w0k = warm[:, None, 0, :].repeat(1, K, 1).contiguous()

    grow = torch.ones(N, dtype=dt, device=dev)  # the factor of the last change of mu (Tassa et al. 2012)

    def raise_mu(which):
        # consecutive rises compound: x mu_factor, x mu_factor^2, ... so that a few rejected
        # iterations reach the damping a stiff scene needs; an accepted step unwinds it the same way
        nonlocal mu, grow, status, active
        grow = torch.where(which, torch.clamp(grow * mu_factor, min=mu_factor), grow)
        mu = torch.where(which, torch.clamp(mu * grow, min=MU_MIN), mu)
        capped = which & (mu > MU_MAX)
        status = torch.where(capped, torch.full_like(status, STALLED), status)
        active = active & ~capped

    for _ in range(int(max_iter)):
        if not bool(active.any()):
            break
        iters += active.to(torch.int32)
        lin = system.transition_fd_along(state[:, :T].contiguous(), ctrl, warmstart=warm, nsub=nsub, centered=centered)
        _, dx = trajectory_cost(system, problem, state, ctrl, w)
        lx, lu = w[0][:, None, :] * dx[:, :T], w[2][:, None, :] * ctrl
        lxx = (w[0][:, None, :, None] * eye_x).expand(N, T, 2 * nv, 2 * nv)
        luu = (w[2][:, None, :, None] * eye_u).expand(N, T, nu, nu)
        lux = torch.zeros(N, T, nu, 2 * nv, dtype=dt, device=dev)
        Vx_T, Vxx_T = w[1] * dx[:, T], w[1][:, :, None] * eye_x
        if sw:
            # C at x_1 .. x_T, each with the ctrl of the step that led to it, as the rollout recorded
            # its sensors (the weighted rows read neither ctrl nor the warm start)
            Cs = system.sensor_fd_along(state[:, 1:].contiguous(), ctrl, centered=centered, only=("C",)).C
            res = sensor_cost(sens, sw)[1]
            CT = Cs.transpose(2, 3)
            wr = torch.cat([sw[1][:, None, :].expand(N, T - 1, -1), sw[2][:, None, :]], dim=1)  # [N, T, ns]
            gx = (CT @ (wr * res)[..., None])[..., 0]  # [N, T, 2nv]: row t - 1 belongs to x_t
            gxx = CT @ (wr[..., None] * Cs)
            lx, lxx = lx.clone(), lxx.clone()
            lx[:, 1:] += gx[:, :T - 1]
            lxx[:, 1:] += gxx[:, :T - 1]
            Vx_T, Vxx_T = Vx_T + gx[:, T - 1], Vxx_T + gxx[:, T - 1]
        while True:
            bw = lqr_backward(lin.A, lin.B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu)
            bad = active & ((bw.info != 0) | ~torch.isfinite(bw.k_ff).all(-1).all(-1))
            if not bool(bad.any()):
                break
            raise_mu(bad)
            fresh = fresh & ~bad
        # an env that has ended takes the zero step: its trajectory is rolled again and discarded
        new_k = torch.where(active[:, None, None], bw.k_ff, torch.zeros_like(bw.k_ff)).contiguous()
        new_g = torch.where(active[:, None, None, None], bw.gain, torch.zeros_like(bw.gain)).contiguous()
        predicted = -(bw.expected[:, 0] + bw.expected[:, 1])
        done = active & fresh & torch.isfinite(cost) & (predicted <= tol * cost.abs())
        status = torch.where(done, torch.full_like(status, CONVERGED), status)
        active = active & ~done
        rr = system.rollout_feedback(ctrl, x_nom=state[:, :T].contiguous(), k_ff=new_k, alpha=alpha, gain=new_g,
                                     initial_state=x0k, initial_warmstart=w0k, nsub=nsub, **rec)
        cand = torch.cat([x0k[:, :, None, :], rr.state], dim=2)
        costs, _ = trajectory_cost(system, problem, cand, rr.ctrl, w)
        if sw:
            costs = costs + sensor_cost(rr.sensordata, sw)[0]
        costs = torch.where((rr.n_done < T) | ~torch.isfinite(costs), inf, costs)
        best_cost, best = costs.min(dim=1)
        accept = active & (best_cost < cost)
        pick = lambda x: x[torch.arange(N, device=dev), best]  # noqa: E731
        sel = lambda m, a, b: torch.where(m.reshape((N,) + (1,) * (a.dim() - 1)), a, b)  # noqa: E731
        state = sel(accept, pick(cand), state)
        ctrl = sel(accept, pick(rr.ctrl), ctrl)
        warm = sel(accept, pick(rr.warmstart), warm)
        if sw:
            sens = sel(accept, pick(rr.sensordata), sens)
        k_ff, gain = sel(accept, new_k, k_ff), sel(accept, new_g, gain)
        small = accept & ((cost - best_cost) < tol * cost.abs())
        cost = torch.where(accept, best_cost, cost)
        status = torch.where(small, torch.full_like(status, CONVERGED), status)
        grow = torch.where(accept, torch.clamp(grow / mu_factor, max=1.0 / mu_factor), grow)
        mu = torch.where(accept, mu * grow, mu)
        fresh = fresh | accept
        rejected = active & ~accept
        active = active & ~small
        fresh = fresh & ~rejected
        raise_mu(rejected)
        history.append(cost.clone())
    return IlqrResult(ctrl, state, gain, k_ff, cost, torch.stack(history), iters, status)


class IlqrMethods:
    """Mixin of PhysicsBatch (uses rollout_feedback, transition_fd_along, state_difference, get_state)."""

    def solve_ilqr(self, goal_state: torch.Tensor, horizon: int, w_x, w_xf, w_u, u_init: Optional[torch.Tensor] = None,
                   nsub: int = 1, alphas: Sequence[float] = DEFAULT_ALPHAS, mu0: float = 1e-6, mu_factor: float = 10.0,
                   max_iter: int = 20, tol: float = 1e-6, centered: bool = False, sensor_goal=None, w_s=None,
                   w_sf=None) -> IlqrResult:
        """``ilqr.solve`` from every env's current state towards ``goal_state`` [N, nstate] or
        [N, T + 1, nstate] over ``horizon`` = T recorded steps of ``nsub`` mj_steps, with the
        diagonal quadratic cost of :mod:`~.ilqr` (weights [n] or [N, n]; the Gauss-Newton gradient
        takes d(dx)/dx = I) and, with ``sensor_goal`` [N, ns] or [N, T, ns] and the weights ``w_s``,
        ``w_sf`` ([ns] or [N, ns]), its sensor residual (``sensor_slices`` maps names to rows;
        accelerometer, force, torque and touch rows may not be weighted). See ``ilqr.solve`` for
        the iteration and the result. The batch's state is not written."""
        problem = IlqrProblem(self.get_state(), goal_state.to(self.dtype), horizon, w_x, w_xf, w_u, u_init,
                              sensor_goal=sensor_goal, w_s=w_s, w_sf=w_sf)
        return solve(self, problem, nsub=nsub, alphas=alphas, mu0=mu0, mu_factor=mu_factor, max_iter=max_iter, tol=tol,
                     centered=centered)


class IlqrForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``solve_ilqr`` (raw actuator ctrl, as
    ``physics_rollout``; pass ``nsub`` = the env's frame skip)."""

    def solve_ilqr(self, goal_state, horizon, w_x, w_xf, w_u, **kw):
        return self.batch.solve_ilqr(goal_state, horizon, w_x, w_xf, w_u, **kw)
