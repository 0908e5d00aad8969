"""Batched open-loop rollouts on the device (mgx_rollout, include/mgx.h): MuJoCo's
``mujoco.rollout``.

``RolloutMethods`` gives :class:`~.batch.PhysicsBatch` its ``rollout`` / ``get_state`` /
``set_state``; ``RolloutForwarding`` gives the ``*VectorEnv`` classes the same call, forwarded to
their batch.

From every env's state (or from given initial states), K rollouts of T recorded steps under K
control sequences: ``state`` [N, K, T, nstate] with the state vector ``[time, qpos, qvel]``
(mjSTATE_FULLPHYSICS; the models have no activations), optionally ``sensordata`` [N, K, T,
nsensordata], and ``n_done`` [N, K]. The call steps virtual copies of the envs in a workspace of
its own with the library's own step, so a rollout is bit for bit what ``step()`` would do; it writes
nothing to the batch's state.

With ``cost=RolloutCost(...)`` the same calls go through mgx_rollout_cost and also return ``cost``
[N, K] (and ``cost_terms`` [N, K, 3]), accumulated on the device while the rollout runs: the score a
sampling planner (:mod:`~.sampling`) needs, without recording a trajectory.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import cabi
from .native import check, lib
from .sensors import _ptr, _stream

ROLLOUT_OUTPUTS = ("state", "sensordata", "n_done")
COST_OUTPUTS = ("cost", "cost_terms")  # present with cost=RolloutCost(...) only
WORKSPACE_LIMIT = 1 << 30  # slots=None keeps the workspace under this many bytes (one virtual env at least)


class RolloutResult:
    """state [N, K, T, nstate] (row t: ``[time, qpos, qvel]`` after recorded step t), sensordata
    [N, K, T, nsensordata] (the sensors at that state, as ``sensordata()`` gives them after a
    ``step()``) and n_done int32 [N, K]: the recorded steps completed before the rollout diverged
    (a bad-state auto-reset), T if it did not; rows n_done .. T-1 repeat what the diverging step
    left behind. A field the call did not request is None. Tensors the call allocated are owned by
    the batch and overwritten by the next call of the same shape. With a ``cost`` given: cost
    float64 [N, K] and cost_terms float64 [N, K, 3] (its state, control and sensor parts), +inf for a
    rollout that diverged."""

    __slots__ = ROLLOUT_OUTPUTS + COST_OUTPUTS

    def __init__(self, **fields):
        for f in self.__slots__:
            setattr(self, f, fields.get(f))

    def rows(self, a: int, b: int) -> "RolloutResult":
        return RolloutResult(**{f: None if getattr(self, f) is None else getattr(self, f)[a:b] for f in self.__slots__})


class RolloutCost:
    """The diagonal quadratic cost of :mod:`~.ilqr` (``trajectory_cost + sensor_cost``), scored inside
    the rollout (mgx_rollout_cost, include/mgx.h):

        J = sum_{t<T} 1/2 (w_x . dx_t^2 + w_u . u_t^2) + 1/2 w_xf . dx_T^2
          + sum_{t=1..T-1} 1/2 w_s . r_t^2 + 1/2 w_sf . r_T^2,
        dx_t = state_difference(x_t, goal_t),  r_t = sensordata(x_t) - sensor_goal_t,

    x_0 the rollout's initial state, x_t the state after recorded step t, u_t the control handed to
    step t (open loop: the knot as given, not clamped). ``goal`` [N, nstate] or [N, T + 1, nstate];
    ``sensor_goal`` [N, ns] or [N, T, ns] (row t - 1 belongs to x_t); the weights ``w_x``, ``w_xf``
    [2nv], ``w_u`` [nu], ``w_s``, ``w_sf`` [ns], each [n] or [N, n], None: zeros. Unlike
    ``solve_ilqr``, rows of accelerometer, force, torque and touch sensors may be weighted."""

    __slots__ = ("goal", "w_x", "w_xf", "w_u", "sensor_goal", "w_s", "w_sf")

    def __init__(self, goal=None, w_x=None, w_xf=None, w_u=None, sensor_goal=None, w_s=None, w_sf=None):
        self.goal, self.w_x, self.w_xf, self.w_u = goal, w_x, w_xf, w_u
        self.sensor_goal, self.w_s, self.w_sf = sensor_goal, w_s, w_sf


def alloc_rollout(n, k, t, nstate, nsensordata, dtype, device, sensordata=True) -> RolloutResult:
    z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return RolloutResult(state=z(n, k, t, nstate), sensordata=z(n, k, t, nsensordata) if sensordata else None,
                         n_done=torch.zeros(n, k, dtype=torch.int32, device=device))


def rollout_shape(n, nu, ctrl, nstep, initial_state, initial_warmstart, hold, shared_ctrl):
    """(K, T) of a rollout call, inferred from ``ctrl`` / ``initial_state`` / ``initial_warmstart``.
    ``ctrl`` is [N, K, ceil(T / hold), nu] ([K, ceil(T / hold), nu] when shared): without ``nstep``,
    T is its knots times ``hold``."""
    k = None
    lead = 0 if shared_ctrl else 1
    if ctrl is not None:
        if ctrl.dim() != 3 + lead or ctrl.shape[-1] != nu or (lead and ctrl.shape[0] != n):
            raise ValueError(f"ctrl must be {'[K' if shared_ctrl else '[N, K'}, ceil(T / hold), nu], got {tuple(ctrl.shape)}")
        k = int(ctrl.shape[lead])
        if nstep is None:
            nstep = int(ctrl.shape[lead + 1]) * int(hold)
    for name, t in (("initial_state", initial_state), ("initial_warmstart", initial_warmstart)):
        if t is None:
            continue
        if t.dim() != 3 or t.shape[0] != n or (k is not None and t.shape[1] != k):
            raise ValueError(f"{name} must be [N, K, width] with the K of the other arguments, got {tuple(t.shape)}")
        k = int(t.shape[1])
    if nstep is None:
        raise ValueError("nstep is required when ctrl is None")
    nstep = int(nstep)
    if ctrl is not None and hold >= 1 and nstep >= 1 and int(ctrl.shape[lead + 1]) != -(-nstep // int(hold)):
        raise ValueError(f"ctrl holds {int(ctrl.shape[lead + 1])} knots, nstep = {nstep} with hold = {hold} needs "
                         f"{-(-nstep // int(hold))}")
    return (1 if k is None else k), nstep


class RolloutMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and state)."""

    @property
    def state_size(self) -> int:
        """nstate = 1 + nq + nv: ``[time, qpos, qvel]``."""
        return 1 + int(self.model.nq) + int(self.model.nv)

    def get_state(self) -> torch.Tensor:
        """The envs' state vectors ``[time, qpos, qvel]``, a new tensor [N, nstate]."""
        return torch.cat([self.time[:, None], self.qpos, self.qvel], dim=1)

    def set_state(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Writes ``[time, qpos, qvel]`` rows [N, nstate] into the batch (the rows of envs that
        ``mask``, uint8 or bool [N], selects). qacc_warmstart, ctrl and the applied forces stay."""
        nq = int(self.model.nq)
        assert tuple(x.shape) == (self.n, self.state_size), x.shape
        x = x.to(device=self.device, dtype=self.dtype)
        parts = ((self.time, x[:, 0]), (self.qpos, x[:, 1:1 + nq]), (self.qvel, x[:, 1 + nq:]))
        if mask is None:
            for dst, src in parts:
                dst.copy_(src)
        else:
            sel = mask.to(device=self.device).bool()
            for dst, src in parts:
                dst.copy_(torch.where(sel if dst.dim() == 1 else sel[:, None], src, dst))

    def _rollout_workspace(self, slots: Optional[int], sensordata: bool, total: int):
        if slots is None:
            one = int(lib().mgx_rollout_bytes(self.native.handle, 1, int(sensordata)))
            check(min(one, 0), "mgx_rollout_bytes")
            slots = max(1, min(total, WORKSPACE_LIMIT // one))
        slots = int(slots)
        cache = self.__dict__.setdefault("_rollout_ws", {})
        key = (slots, bool(sensordata))
        if key not in cache:
            # below one slot no workspace size is defined: the library refuses the call
            nbytes = int(lib().mgx_rollout_bytes(self.native.handle, max(slots, 1), int(sensordata)))
            check(min(nbytes, 0), "mgx_rollout_bytes")
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return slots, cache[key]

    def _rollout_cost_io(self, cost: RolloutCost, k: int, t: int, out, res, ws) -> "cabi.MgxCostIO":
        """The mgx_cost_io of ``cost`` for K = k rollouts of T = t steps; sets res.cost / res.cost_terms
        (those of ``out`` when it carries them, else tensors the batch owns per K)."""
        n, m = self.n, self.model
        nv, nu, nsd, ns = int(m.nv), int(m.nu), int(m.nsensordata), self.state_size
        dev = lambda x: torch.as_tensor(x, dtype=self.dtype, device=self.device)  # noqa: E731
        keep = []  # the converted inputs must outlive the asynchronous call: held until the next one

        def rows(name, x, width, many):
            if x is None:
                return None, 1
            x = dev(x)
            if tuple(x.shape) == (n, width):
                x = x[:, None, :]
            elif tuple(x.shape) != (n, many, width):
                raise ValueError(f"{name} must be [N, {width}] or [N, {many}, {width}], got {tuple(x.shape)}")
            x = x.contiguous()
            keep.append(x)
            return x, int(x.shape[1])

        def weight(name, x, width, needs, given):
            if x is None:
                return None
            if not given:
                raise ValueError(f"{name} needs {needs}")
            x = dev(x)
            if tuple(x.shape) not in ((width,), (n, width)):
                raise ValueError(f"{name} must be [{width}] or [N, {width}], got {tuple(x.shape)}")
            x = x.expand(n, width).contiguous()
            keep.append(x)
            return x

        goal, goal_rows = rows("goal", cost.goal, ns, t + 1)
        sgoal, sensor_rows = rows("sensor_goal", cost.sensor_goal, nsd, t)
        cio = cabi.MgxCostIO()
        ptr = lambda x: None if x is None else (x.data_ptr() or ws.data_ptr())  # noqa: E731  (width 0: no bytes)
        cio.goal, cio.goal_rows, cio.sensor_goal, cio.sensor_rows = ptr(goal), goal_rows, ptr(sgoal), sensor_rows
        cio.w_x = ptr(weight("w_x", cost.w_x, 2 * nv, "goal", goal is not None))
        cio.w_xf = ptr(weight("w_xf", cost.w_xf, 2 * nv, "goal", goal is not None))
        cio.w_u = ptr(weight("w_u", cost.w_u, nu, "", True))
        cio.w_s = ptr(weight("w_s", cost.w_s, nsd, "sensor_goal", sgoal is not None))
        cio.w_sf = ptr(weight("w_sf", cost.w_sf, nsd, "sensor_goal", sgoal is not None))
        own = self.__dict__.setdefault("_rollout_cost_out", {})
        if k not in own and k >= 1:
            own[k] = (torch.zeros(n, k, dtype=torch.float64, device=self.device),
                      torch.zeros(n, k, 3, dtype=torch.float64, device=self.device))
        c = getattr(out, "cost", None)
        terms = getattr(out, "cost_terms", None)
        if c is None and k in own:
            c, terms = own[k][0], (own[k][1] if terms is None else terms)
        if c is not None:  # bad K: the library names the argument
            assert c.dtype == torch.float64 and c.is_contiguous() and tuple(c.shape) == (n, k), tuple(c.shape)
            cio.cost = c.data_ptr()
        if terms is not None:
            assert terms.dtype == torch.float64 and terms.is_contiguous() and tuple(terms.shape) == (n, k, 3)
            cio.terms = terms.data_ptr()
        res.cost, res.cost_terms = c, terms
        self.__dict__["_rollout_cost_keep"] = keep
        return cio

    def _rollout_n_done(self, k: int) -> torch.Tensor:
        """n_done [N, K] of a cost call that records no trajectory (owned by the batch per K)."""
        cache = self.__dict__.setdefault("_rollout_cost_n_done", {})
        if k not in cache:
            cache[k] = torch.zeros(self.n, k, dtype=torch.int32, device=self.device)
        return cache[k]

    def rollout(self, ctrl: Optional[torch.Tensor] = None, nstep: Optional[int] = None,
                initial_state: Optional[torch.Tensor] = None, initial_warmstart: Optional[torch.Tensor] = None,
                nsub: int = 1, hold: int = 1, shared_ctrl: bool = False, sensordata: bool = False,
                mask: Optional[torch.Tensor] = None, stream=None, slots: Optional[int] = None,
                only: Optional[Sequence[str]] = None, out: Optional[RolloutResult] = None,
                cost: Optional[RolloutCost] = None) -> RolloutResult:
        """``RolloutResult(state, sensordata, n_done)``: K open-loop rollouts of T recorded steps
        per (masked) env, asynchronously on the stream; each recorded step is ``nsub`` mj_steps.

        ``ctrl`` [N, K, ceil(T / hold), nu] (``shared_ctrl``: [K, ceil(T / hold), nu] for all envs)
        is the raw actuator control, one knot per ``hold`` recorded steps; None holds each env's
        current ctrl and needs ``nstep``. ``initial_state`` [N, K, nstate] / ``initial_warmstart``
        [N, K, nv] default to each env's current state / qacc_warmstart. K and T are inferred from
        these tensors (K = 1 when none is given). ``sensordata=True`` also records the sensors.
        ``slots`` bounds the workspace (virtual envs held at once; default: all N K in one pass up to
        1 GiB); the workspace is allocated once per (slots, sensordata). ``only`` names the outputs
        wanted; rows of envs that ``mask`` (uint8 [N]) deselects are left as they were.

        ``cost`` (a :class:`RolloutCost`) also scores every rollout on the device: the result carries
        ``cost`` [N, K] and ``cost_terms`` [N, K, 3] in float64, whatever ``only`` names, and
        ``only=("cost",)`` or ``("cost", "n_done")`` allocates and records no trajectory at all."""
        n, m = self.n, self.model
        nq, nv, nu = int(m.nq), int(m.nv), int(m.nu)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()
        want = [f for f in ROLLOUT_OUTPUTS if sensordata or f != "sensordata"] if only is None else list(only)
        want = _without_cost_names(want, cost)
        for f in want:
            if f not in ROLLOUT_OUTPUTS:
                raise KeyError(f"unknown rollout output {f!r}; there are {list(ROLLOUT_OUTPUTS)}")
        sensordata = "sensordata" in want
        k, t = rollout_shape(n, nu, ctrl, nstep, initial_state, initial_warmstart, hold, shared_ctrl)
        for name, x, width in (("ctrl", ctrl, nu), ("initial_state", initial_state, self.state_size),
                               ("initial_warmstart", initial_warmstart, nv)):
            if x is not None:
                assert x.dtype == self.dtype and x.is_cuda and x.is_contiguous() and x.shape[-1] == width, name
        nsd = int(m.nsensordata)
        sensor_term = cost is not None and cost.sensor_goal is not None  # needs the staging rows
        if sensordata or sensor_term:
            self._sensor_ready()
        if out is None and cost is not None and all(f == "n_done" for f in want):
            out = RolloutResult(n_done=self._rollout_n_done(k) if want and k >= 1 else None)
        if out is None:
            cache = self.__dict__.setdefault("_rollout_out", {})
            key = (k, t, sensordata)
            if key not in cache and k >= 1 and t >= 1:
                cache[key] = alloc_rollout(n, k, t, 1 + nq + nv, nsd, self.dtype, self.device, sensordata)
            out = cache.get(key) or RolloutResult()
        slots, ws = self._rollout_workspace(slots, sensordata or sensor_term, max(n * k, 1))
        io = cabi.MgxRolloutIO()
        io.n_roll, io.n_step, io.nsub, io.hold = k, t, int(nsub), int(hold)
        io.flags = cabi.MGX_ROLLOUT_SHARED_CTRL if shared_ctrl else 0
        io.slots, io.workspace, io.workspace_bytes = slots, ws.data_ptr(), ws.numel()
        io.initial_state = None if initial_state is None else initial_state.data_ptr()
        io.initial_warmstart = None if initial_warmstart is None else initial_warmstart.data_ptr()
        io.ctrl = None if ctrl is None or nu == 0 else ctrl.data_ptr()
        res = RolloutResult()
        widths = {"state": (k, t, 1 + nq + nv), "sensordata": (k, t, nsd), "n_done": (k,)}
        for f in want:
            x = getattr(out, f)
            if x is None:
                continue  # bad K / T: the library names the argument
            assert x.is_contiguous() and tuple(x.shape) == (n,) + widths[f], (f, tuple(x.shape))
            assert x.dtype == (torch.int32 if f == "n_done" else self.dtype)
            # a model without sensors has no bytes to write; the request still reaches the library,
            # which refuses it for the models mgx_forward refuses
            setattr(io, f, x.data_ptr() or ws.data_ptr())
            setattr(res, f, x)
        if cost is None:
            check(lib().mgx_rollout(self.native.handle, C.byref(self._state), C.byref(io), n, _ptr(mask),
                                    _stream(stream)), "mgx_rollout")
            return res
        cio = self._rollout_cost_io(cost, k, t, out, res, ws)
        check(lib().mgx_rollout_cost(self.native.handle, C.byref(self._state), C.byref(io), None, C.byref(cio), n,
                                     _ptr(mask), _stream(stream)), "mgx_rollout_cost")
        return res


    def rollout_feedback(self, u_nom: torch.Tensor, x_nom: Optional[torch.Tensor] = None,
                         k_ff: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
                         gain: Optional[torch.Tensor] = None, clamp: bool = True,
                         initial_state: Optional[torch.Tensor] = None, initial_warmstart: Optional[torch.Tensor] = None,
                         nsub: int = 1, sensordata: bool = False, mask: Optional[torch.Tensor] = None, stream=None,
                         slots: Optional[int] = None, only: Optional[Sequence[str]] = None,
                         out: Optional["FeedbackRolloutResult"] = None,
                         cost: Optional[RolloutCost] = None) -> "FeedbackRolloutResult":
        """``FeedbackRolloutResult(state, sensordata, n_done, ctrl, warmstart)``: K closed-loop
        rollouts of T recorded steps per (masked) env. ``rollout`` with the control of every step
        computed on the device from the rollout's own state entering that step:

            u[n, k, t] = u_nom[n, t] + alpha[n, k] k_ff[n, t] + gain[n, t] @ (x[n, k, t] (-) x_nom[n, t])

        ``u_nom`` [N, T, nu]; ``x_nom`` [N, T, nstate] (row t: the nominal state ENTERING step t,
        required with ``gain``); ``k_ff`` [N, T, nu]; ``alpha`` [N, K] (default 1); ``gain``
        [N, T, nu, 2nv]; ``(-)`` is ``state_difference``. ``clamp`` clamps u to the control range of
        limited actuators before it is recorded and applied. K comes from ``alpha`` or
        ``initial_state`` / ``initial_warmstart``, else 1; T from ``u_nom``. ``ctrl`` [N, K, T, nu]
        is the control applied at step t, ``warmstart`` [N, K, T, nv] the qacc_warmstart entering
        it; after a divergence at step n_done their later rows are zero. Everything else
        (``initial_state``, ``nsub``, ``sensordata``, ``mask``, ``slots``, ``only``, ``out``) is
        ``rollout``'s, ``cost`` included (u_t is then the recorded ``ctrl``); nothing is written to the
        batch's state."""
        n, m = self.n, self.model
        nq, nv, nu, ns = int(m.nq), int(m.nv), int(m.nu), self.state_size
        if u_nom.dim() != 3 or u_nom.shape[0] != n or u_nom.shape[2] != nu:
            raise ValueError(f"u_nom must be [N, T, nu], got {tuple(u_nom.shape)}")
        t = int(u_nom.shape[1])
        if gain is not None and x_nom is None:
            raise ValueError("gain needs x_nom")
        for name, x, shape in (("x_nom", x_nom, (n, t, ns)), ("k_ff", k_ff, (n, t, nu)), ("gain", gain, (n, t, nu, 2 * nv))):
            if x is not None and tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, got {tuple(x.shape)}")
        if alpha is not None and (alpha.dim() != 2 or alpha.shape[0] != n):
            raise ValueError(f"alpha must be [N, K], got {tuple(alpha.shape)}")
        k = None if alpha is None else int(alpha.shape[1])
        for name, x in (("initial_state", initial_state), ("initial_warmstart", initial_warmstart)):
            if x is None:
                continue
            if x.dim() != 3 or x.shape[0] != n or (k is not None and x.shape[1] != k):
                raise ValueError(f"{name} must be [N, K, width] with the K of the other arguments, got {tuple(x.shape)}")
            k = int(x.shape[1])
        k = 1 if k is None else k
        for name, x, width in (("u_nom", u_nom, nu), ("x_nom", x_nom, ns), ("k_ff", k_ff, nu), ("alpha", alpha, k),
                               ("gain", gain, 2 * nv), ("initial_state", initial_state, ns),
                               ("initial_warmstart", initial_warmstart, nv)):
            if x is not None:
                assert x.dtype == self.dtype and x.is_cuda and x.is_contiguous() and x.shape[-1] == width, name
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()
        fields = ROLLOUT_OUTPUTS + FEEDBACK_OUTPUTS
        want = [f for f in fields if sensordata or f != "sensordata"] if only is None else list(only)
        want = _without_cost_names(want, cost)
        for f in want:
            if f not in fields:
                raise KeyError(f"unknown rollout output {f!r}; there are {list(fields)}")
        sensordata = "sensordata" in want
        nsd = int(m.nsensordata)
        sensor_term = cost is not None and cost.sensor_goal is not None
        if sensordata or sensor_term:
            self._sensor_ready()
        if out is None and cost is not None and all(f == "n_done" for f in want):
            out = FeedbackRolloutResult(n_done=self._rollout_n_done(k) if want and k >= 1 else None)
        if out is None:
            cache = self.__dict__.setdefault("_feedback_out", {})
            key = (k, t, sensordata)
            if key not in cache and t >= 1:
                cache[key] = alloc_feedback_rollout(n, k, t, ns, nsd, nv, nu, self.dtype, self.device, sensordata)
            out = cache.get(key) or FeedbackRolloutResult()
        slots, ws = self._rollout_workspace(slots, sensordata or sensor_term, max(n * k, 1))
        io = cabi.MgxRolloutIO()
        io.n_roll, io.n_step, io.nsub, io.hold, io.flags = k, t, int(nsub), 1, 0
        io.slots, io.workspace, io.workspace_bytes = slots, ws.data_ptr(), ws.numel()
        io.initial_state = None if initial_state is None else initial_state.data_ptr()
        io.initial_warmstart = None if initial_warmstart is None else initial_warmstart.data_ptr()
        ptr = lambda x: None if x is None else (x.data_ptr() or ws.data_ptr())  # noqa: E731  (nu = 0: no bytes)
        fb = cabi.MgxFeedbackIO()
        fb.u_nom, fb.x_nom, fb.k_ff, fb.alpha, fb.gain = ptr(u_nom), ptr(x_nom), ptr(k_ff), ptr(alpha), ptr(gain)
        fb.flags = cabi.MGX_FEEDBACK_CLAMP if clamp else 0
        res = FeedbackRolloutResult()
        widths = {"state": (k, t, ns), "sensordata": (k, t, nsd), "n_done": (k,), "ctrl": (k, t, nu), "warmstart": (k, t, nv)}
        native_name = {"ctrl": "ctrl_out", "warmstart": "warm_out"}
        for f in want:
            x = getattr(out, f)
            if x is None:
                continue
            assert x.is_contiguous() and tuple(x.shape) == (n,) + widths[f], (f, tuple(x.shape))
            assert x.dtype == (torch.int32 if f == "n_done" else self.dtype)
            setattr(fb if f in native_name else io, native_name.get(f, f), x.data_ptr() or ws.data_ptr())
            setattr(res, f, x)
        if cost is None:
            check(lib().mgx_rollout_feedback(self.native.handle, C.byref(self._state), C.byref(io), C.byref(fb), n,
                                             _ptr(mask), _stream(stream)), "mgx_rollout_feedback")
            return res
        cio = self._rollout_cost_io(cost, k, t, out, res, ws)
        check(lib().mgx_rollout_cost(self.native.handle, C.byref(self._state), C.byref(io), C.byref(fb), C.byref(cio), n,
                                     _ptr(mask), _stream(stream)), "mgx_rollout_cost")
        return res


def _without_cost_names(want, cost):
    """``only`` without "cost" / "cost_terms": with a cost given both are always produced."""
    if cost is None and any(f in COST_OUTPUTS for f in want):
        raise ValueError("only names a cost output, but no cost= was given")
    return [f for f in want if f not in COST_OUTPUTS]


FEEDBACK_OUTPUTS = ("ctrl", "warmstart")


class FeedbackRolloutResult:
    """The fields of :class:`RolloutResult` plus ctrl [N, K, T, nu] (the control applied at recorded
    step t) and warmstart [N, K, T, nv] (the qacc_warmstart entering it); rows after a divergence
    (t > n_done) of these two are zero."""

    __slots__ = ROLLOUT_OUTPUTS + FEEDBACK_OUTPUTS + COST_OUTPUTS

    def __init__(self, **fields):
        for f in self.__slots__:
            setattr(self, f, fields.get(f))

    def rows(self, a: int, b: int) -> "FeedbackRolloutResult":
        return FeedbackRolloutResult(**{f: None if getattr(self, f) is None else getattr(self, f)[a:b]
                                        for f in self.__slots__})


def alloc_feedback_rollout(n, k, t, nstate, nsensordata, nv, nu, dtype, device, sensordata=True) -> FeedbackRolloutResult:
    base = alloc_rollout(n, k, t, nstate, nsensordata, dtype, device, sensordata)
    z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return FeedbackRolloutResult(state=base.state, sensordata=base.sensordata, n_done=base.n_done, ctrl=z(n, k, t, nu),
                                 warmstart=z(n, k, t, nv))


class RolloutForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's open-loop rollouts under the env's name.

    The method is ``physics_rollout``: ``rollout`` on an env is its tensor of running episode sums.
    ``ctrl`` is the RAW ACTUATOR CONTROL of the physics model (``batch.ctrl``), not the task's
    action: the env's action clipping / scaling and its scripted actuators (goalkeeper, obstacle
    motors ...) are not applied, and no reward, observation or termination is computed. Pass
    ``nsub`` = the env's frame skip (10 for parkour and assembly, 1 otherwise) for one recorded step
    to span the physics of one env step."""

    @property
    def state_size(self) -> int:
        return self.batch.state_size

    def get_state(self):
        return self.batch.get_state()

    def set_state(self, x, mask=None):
        return self.batch.set_state(x, mask=mask)

    def physics_rollout(self, **kw):
        """PhysicsBatch.rollout of this env's batch (raw actuator ctrl; ``nsub`` = frame skip)."""
        return self.batch.rollout(**kw)

    def physics_rollout_feedback(self, u_nom, **kw):
        """PhysicsBatch.rollout_feedback of this env's batch (closed-loop: the control of every step
        from the rollout's own state; raw actuator ctrl; ``nsub`` = frame skip)."""
        return self.batch.rollout_feedback(u_nom, **kw)
