"""Batched sampling MPC on top of the fused rollout cost (``rollout(..., cost=)``, mgx_rollout_cost):
MPPI (Williams et al. 2017) and, with ``lam = 0``, predictive sampling (Howell et al. 2022).

``solve`` is the driver; ``SamplingMethods`` gives :class:`~.batch.PhysicsBatch` its ``solve_mppi``
and ``SamplingForwarding`` the ``*VectorEnv`` classes theirs.

The planner differentiates nothing: per iteration it scores K sampled control sequences per env with
ONE ``rollout`` call, whose K T physics steps per env run in the library's HIP kernels and whose
cost [N, K] is accumulated inside that call, so no trajectory tensor [N, K, T, nstate] exists. The
update is a handful of torch ops on [N, K] and [N, K, J, nu]: plumbing, like the Riccati pass of
:mod:`~.ilqr`, not a kernel, and it runs on CPU tensors as well, so a CPU stand-in for the system
can drive the planner in the tests.

The cost is :class:`~.rollouts.RolloutCost`: the diagonal quadratic of :mod:`~.ilqr`
(``trajectory_cost + sensor_cost``). Having no backward pass, the planner may weight accelerometer,
force, torque and touch rows, which ``solve_ilqr`` must refuse.

One iteration, with J = ceil(T / hold) knots (zero-order hold, ``hold`` recorded steps each):

1. sample: sample 0 is the nominal itself, samples 1 .. K-1 are ``nominal + sigma z`` clamped to
   ``actuator_ctrlrange`` where the actuator is limited; ``z`` ~ N(0, 1) from ``torch.randn`` with
   the given generator, or the explicit ``noise`` [N, K-1, J, nu] (the same in every iteration);
2. score: ``rollout(ctrl=, hold=, cost=, only=("cost", "n_done"))``; a diverged rollout costs +inf;
3. update: ``w_k = exp(-(c_k - c_min) / lam)`` normalised over k, +inf costs weigh 0, the new nominal
   is ``sum_k w_k knots_k``; ``lam = 0`` takes the arg-min sample (the first on ties) bit for bit.
   An env none of whose samples is finite keeps its nominal and ends with status 2.

Not provided: CEM's elite refit, spline (non zero-order-hold) knots, rollouts through a task's fused
env step (task rewards as the cost), and switching ``solve_ilqr``'s line search to the fused cost.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Callable, Optional

import torch

from .ilqr import IlqrProblem
from .rollouts import RolloutCost

OK, NO_FINITE_SAMPLE = 0, 2

SamplingResult = namedtuple("SamplingResult", "knots ctrl cost cost_history best ess n_finite status")
MppiWeights = namedtuple("MppiWeights", "w best ess n_finite")


class SamplingProblem(IlqrProblem):
    """The fields of :class:`~.ilqr.IlqrProblem`; ``u_init`` is the nominal's knots [N, J, nu],
    J = ceil(horizon / hold) (None: zeros)."""


def mppi_weights(cost: torch.Tensor, lam: float) -> MppiWeights:
    """The update weights of costs [N, K] (float64; non-finite entries count as +inf):
    ``w`` [N, K] = softmax(-(c - c_min) / lam) over the finite samples (``lam = 0``: 1 at the first
    arg-min), ``best`` [N] that arg-min, ``ess`` [N] = 1 / sum w^2 and ``n_finite`` [N]. A row
    without a finite sample has w = 0, best = 0, ess = 0."""
    finite = torch.isfinite(cost)
    c = torch.where(finite, cost, torch.full_like(cost, float("inf")))
    n_finite = finite.sum(1).to(torch.int32)
    ok = n_finite > 0
    best = torch.argmin(c, dim=1)  # the first minimal value
    c_min = torch.where(ok, c.gather(1, best[:, None])[:, 0], torch.zeros_like(c[:, 0]))
    if lam > 0:
        e = torch.where(finite, torch.exp(-(torch.where(finite, c, c_min[:, None]) - c_min[:, None]) / lam),
                        torch.zeros_like(c))
        w = e / torch.clamp(e.sum(1, keepdim=True), min=1.0)  # the arg-min contributes exp(0) = 1
    else:
        w = torch.zeros_like(c).scatter_(1, best[:, None], 1.0)
    w = torch.where(ok[:, None], w, torch.zeros_like(w))
    ess = torch.where(ok, 1.0 / torch.clamp((w * w).sum(1), min=1e-300), torch.zeros_like(c_min))
    return MppiWeights(w, best, ess, n_finite)


def hold_controls(knots: torch.Tensor, hold: int, horizon: int) -> torch.Tensor:
    """[..., J, nu] knots as the per-step controls [..., T, nu] of a zero-order hold."""
    return knots.repeat_interleave(int(hold), dim=-2)[..., :int(horizon), :]


def solve(system, problem: SamplingProblem, samples: int = 256, iters: int = 2, sigma=1.0, lam: float = 1.0,
          hold: int = 4, nsub: int = 1, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None,
          cost_fn: Optional[Callable] = None, slots: Optional[int] = None) -> SamplingResult:
    """MPPI for every env of ``system`` at once (module docstring). ``system`` is duck-typed:
    ``rollout(ctrl=, nstep=, hold=, initial_state=, nsub=, slots=, cost=, only=)`` returning ``cost``
    and ``n_done``, and ``model.nu`` / ``model.actuator_ctrlrange`` / ``model.actuator_ctrllimited``
    (a model without the last two has no limits) as :class:`~.batch.PhysicsBatch` has them.

    ``sigma`` is a scalar or [nu]. ``cost_fn(state [N, K, T + 1, nstate], sensordata [N, K, T, ns] or
    None, ctrl [N, K, T, nu]) -> [N, K]`` switches to the materialised path for an arbitrary cost:
    the rollout then records ``state`` (row 0 of what ``cost_fn`` sees is x_0) and, when the problem
    has a ``sensor_goal``, ``sensordata``.

    Returns ``SamplingResult(knots [N, J, nu], ctrl [N, T, nu], cost [N], cost_history
    [N, iters + 1], best [N, iters], ess [N, iters], n_finite [N, iters], status [N])``:
    ``cost_history[:, i]`` is the cost of sample 0, the nominal, in iteration i, and the last column
    (= ``cost``) that of the result, from one closing K = 1 cost rollout; ``best`` is the arg-min
    sample, ``ess`` the effective sample size 1 / sum w^2, ``n_finite`` the samples that did not
    diverge; ``status`` 0, or 2 where some iteration had no finite sample (the nominal was kept).
    Nothing is written to the system's state."""
    x0 = problem.x0
    N, T, K, hold = x0.shape[0], problem.horizon, int(samples), int(hold)
    if K < 1 or T < 1 or hold < 1 or iters < 0 or lam < 0:
        raise ValueError("samples, horizon and hold must be >= 1, iters and lam >= 0")
    nu = int(system.model.nu)
    J = -(-T // hold)
    dt, dev = x0.dtype, x0.device
    nominal = (torch.zeros(N, J, nu, dtype=dt, device=dev) if problem.u_init is None
               else torch.as_tensor(problem.u_init, dtype=dt, device=dev).clone())
    if tuple(nominal.shape) != (N, J, nu):
        raise ValueError(f"u_init must be the knots [N, ceil(T / hold), nu] = {[N, J, nu]}, got {tuple(nominal.shape)}")
    if noise is not None and tuple(noise.shape) != (N, K - 1, J, nu):
        raise ValueError(f"noise must be [N, K - 1, J, nu] = {[N, K - 1, J, nu]}, got {tuple(noise.shape)}")
    sigma = torch.as_tensor(sigma, dtype=dt, device=dev)
    lo = torch.full((nu,), float("-inf"), dtype=dt, device=dev)
    hi = torch.full((nu,), float("inf"), dtype=dt, device=dev)
    limited = getattr(system.model, "actuator_ctrllimited", None)
    if limited is not None and nu > 0:
        lim = torch.as_tensor(limited).to(dev).reshape(-1) != 0
        rng = torch.as_tensor(system.model.actuator_ctrlrange).to(device=dev, dtype=dt).reshape(-1, 2)
        lo, hi = torch.where(lim, rng[:, 0], lo), torch.where(lim, rng[:, 1], hi)
    rc = RolloutCost(goal=problem.goal, w_x=problem.w_x, w_xf=problem.w_xf, w_u=problem.w_u,
                     sensor_goal=problem.sensor_goal, w_s=problem.w_s, w_sf=problem.w_sf)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)

    def score(knots):
        k = knots.shape[1]
        start = x0[:, None, :].expand(N, k, x0.shape[1]).contiguous()
        kw = dict(ctrl=knots, nstep=T, hold=hold, initial_state=start, nsub=nsub, slots=slots)
        if cost_fn is None:
            r = system.rollout(cost=rc, only=("cost", "n_done"), **kw)
            c = r.cost.clone()
        else:
            r = system.rollout(sensordata=problem.sensor_goal is not None, **kw)
            c = cost_fn(torch.cat([start[:, :, None, :], r.state], dim=2), r.sensordata, hold_controls(knots, hold, T))
            c = c.to(torch.float64)
        return torch.where((r.n_done < T) | ~torch.isfinite(c), inf, c)

    status = torch.zeros(N, dtype=torch.int32, device=dev)
    history, bests, esss, nfin = [], [], [], []
    rows = torch.arange(N, device=dev)
    for _ in range(int(iters)):
        knots = nominal[:, None]
        if K > 1:
            if noise is not None:
                z = torch.as_tensor(noise, dtype=dt, device=dev)
            else:
                gdev = dev if generator is None else generator.device
                z = torch.randn((N, K - 1, J, nu), generator=generator, dtype=dt, device=gdev).to(dev)
            pert = torch.minimum(torch.maximum(nominal[:, None] + sigma * z, lo), hi)
            knots = torch.cat([knots, pert], dim=1)
        knots = knots.contiguous()
        c = score(knots)
        mw = mppi_weights(c, float(lam))
        if lam > 0:
            new = (mw.w.to(dt)[:, :, None, None] * knots).sum(1)
        else:
            new = knots[rows, mw.best]  # the sample itself, bit for bit
        ok = mw.n_finite > 0
        nominal = torch.where(ok[:, None, None], new, nominal)
        status = torch.where(ok, status, torch.full_like(status, NO_FINITE_SAMPLE))
        history.append(c[:, 0])
        bests.append(mw.best)
        esss.append(mw.ess)
        nfin.append(mw.n_finite)
    cost = score(nominal[:, None].contiguous())[:, 0]
    history.append(cost)
    stack = lambda xs, dtype: (torch.stack(xs, dim=1) if xs else torch.zeros(N, 0, dtype=dtype, device=dev))  # noqa: E731
    return SamplingResult(nominal, hold_controls(nominal, hold, T), cost, torch.stack(history, dim=1),
                          stack(bests, torch.int64), stack(esss, torch.float64), stack(nfin, torch.int32), status)


class SamplingMethods:
    """Mixin of PhysicsBatch (uses rollout, get_state and the model's control range)."""

    def solve_mppi(self, goal_state: Optional[torch.Tensor], horizon: int, w_x=None, w_xf=None, w_u=None,
                   samples: int = 256, iters: int = 2, sigma=1.0, lam: float = 1.0, hold: int = 4,
                   u_init: Optional[torch.Tensor] = None, sensor_goal=None, w_s=None, w_sf=None, nsub: int = 1,
                   generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None,
                   cost_fn: Optional[Callable] = None, slots: Optional[int] = None) -> SamplingResult:
        """``sampling.solve`` from every env's current state: MPPI (``lam = 0``: predictive sampling)
        towards ``goal_state`` [N, nstate] or [N, T + 1, nstate] over ``horizon`` = T recorded steps
        of ``nsub`` mj_steps, ``samples`` = K control sequences of ceil(T / hold) knots per env and
        iteration, scored by the fused rollout cost (:class:`~.rollouts.RolloutCost`: weights [n] or
        [N, n]; ``sensor_goal`` [N, ns] or [N, T, ns] with ``w_s``, ``w_sf``, on any sensor row).
        ``u_init`` [N, J, nu] is the nominal's knots. See ``sampling.solve`` for the iteration, the
        result and what is not provided. The batch's state is not written."""
        goal = None if goal_state is None else goal_state.to(self.dtype)
        problem = SamplingProblem(self.get_state(), goal, horizon, w_x, w_xf, w_u, u_init, sensor_goal=sensor_goal,
                                  w_s=w_s, w_sf=w_sf)
        return solve(self, problem, samples=samples, iters=iters, sigma=sigma, lam=lam, hold=hold, nsub=nsub,
                     generator=generator, noise=noise, cost_fn=cost_fn, slots=slots)


class SamplingForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``solve_mppi`` (raw actuator ctrl, as
    ``physics_rollout``; pass ``nsub`` = the env's frame skip)."""

    def solve_mppi(self, goal_state, horizon, **kw):
        return self.batch.solve_mppi(goal_state, horizon, **kw)
