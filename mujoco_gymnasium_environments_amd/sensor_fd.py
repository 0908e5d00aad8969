"""Batched finite-difference sensor derivatives on the device (mgx_sensor_fd, include/mgx.h): the
``C`` and ``D`` of MuJoCo's ``mjd_transitionFD``.

``SensorFdMethods`` gives :class:`~.batch.PhysicsBatch` its ``sensor_fd`` / ``sensor_fd_along``;
``SensorFdForwarding`` gives the ``*VectorEnv`` classes the same calls, forwarded to their batch.

``C = d sensordata / dx`` [N, ns, 2nv] and ``D = d sensordata / dctrl`` [N, ns, nu] at the CURRENT
state, with the state tangent ``x = (dq, qvel)`` and the columns, perturbations and control-limit
rule of ``transition_fd``. No step is taken: the sensors (``sensordata()``) are evaluated at the
perturbed current states, in virtual copies of the envs held in a workspace of the call's own; it
writes nothing to the batch's state. Rows are plain component differences, a ``framequat``'s four
included: which of q / -q the sensor reports is the caller's concern.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import cabi
from .native import check, lib
from .sensors import _ptr, _stream
from .transitions import WORKSPACE_LIMIT, default_eps

SENSOR_FD_OUTPUTS = ("C", "D", "sensordata")


class SensorFdResult:
    """C [N, ns, 2nv], D [N, ns, nu] and sensordata [N, ns] (the nominal row: that of the control
    clamped to its range). A field the call did not request is None. Tensors are owned by the batch
    and overwritten by the next call."""

    __slots__ = SENSOR_FD_OUTPUTS

    def __init__(self, **fields):
        for f in SENSOR_FD_OUTPUTS:
            setattr(self, f, fields.get(f))

    def rows(self, a: int, b: int) -> "SensorFdResult":
        return SensorFdResult(**{f: None if getattr(self, f) is None else getattr(self, f)[a:b] for f in SENSOR_FD_OUTPUTS})


def alloc_sensor_fd(n, ns, nv, nu, dtype, device) -> SensorFdResult:
    z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return SensorFdResult(C=z(n, ns, 2 * nv), D=z(n, ns, nu), sensordata=z(n, ns))


class SensorFdMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype, state and _sensor_ready)."""

    def sensor_fd_columns(self, centered: bool = False, with_d: bool = True) -> int:
        """Virtual envs one env's sensor derivatives take: 1 + K, centred 1 + 2 K, with
        K = 2 nv + nu, or 2 nv when D is not requested."""
        k = 2 * int(self.model.nv) + (int(self.model.nu) if with_d else 0)
        return 1 + (2 * k if centered else k)

    def _sensor_fd_workspace(self, slots: Optional[int], centered: bool, with_d: bool):
        c = self.sensor_fd_columns(centered, with_d)
        if slots is None:
            one = int(lib().mgx_sensor_fd_bytes(self.native.handle, c))
            check(min(one, 0), "mgx_sensor_fd_bytes")
            slots = max(1, min(self.n, WORKSPACE_LIMIT // one)) * c
        slots = int(slots)
        cache = self.__dict__.setdefault("_sensor_fd_ws", {})
        key = (slots, bool(centered), bool(with_d))
        if key not in cache:
            # below one env's columns no workspace size is defined: the library refuses the call
            nbytes = int(lib().mgx_sensor_fd_bytes(self.native.handle, max(slots, 1)))
            check(min(nbytes, 0), "mgx_sensor_fd_bytes")
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return slots, cache[key]

    def sensor_fd(self, eps: Optional[float] = None, centered: bool = False, mask: Optional[torch.Tensor] = None,
                  stream=None, slots: Optional[int] = None, only: Optional[Sequence[str]] = None,
                  out: Optional[SensorFdResult] = None) -> SensorFdResult:
        """``SensorFdResult(C, D, sensordata)`` of every (masked) env: finite differences of
        ``sensordata()`` at the current state, asynchronously on the stream. ``eps`` defaults to
        1e-6 (fp64) / 2**-10 (fp32); ``centered`` differences the +eps and -eps states at twice the
        cost. ``slots`` bounds the workspace (virtual envs held at once, at least
        ``sensor_fd_columns(centered, with_d)``; default: every env in one pass up to 1 GiB); the
        workspace is allocated once per (slots, centered, with D). ``only`` names the outputs
        wanted: without ``"D"`` the control columns are not evaluated at all. Rows of envs that
        ``mask`` (uint8 [N]) deselects are left as they were."""
        n, m = self.n, self.model
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()
        want = list(SENSOR_FD_OUTPUTS) if only is None else list(only)
        for f in want:
            if f not in SENSOR_FD_OUTPUTS:
                raise KeyError(f"unknown sensor derivative output {f!r}; there are {list(SENSOR_FD_OUTPUTS)}")
        self._sensor_ready()
        ns = int(m.nsensordata)
        if out is None:
            if getattr(self, "_sensor_fd_out", None) is None:
                self._sensor_fd_out = alloc_sensor_fd(n, ns, int(m.nv), int(m.nu), self.dtype, self.device)
            out = self._sensor_fd_out
        res = SensorFdResult()
        io = cabi.MgxSensorFdIO()
        for f in want:
            t = getattr(out, f)
            assert t is not None and t.is_contiguous() and t.shape[0] == n and t.dtype == self.dtype
            setattr(io, f, t.data_ptr())
            setattr(res, f, t)
        if ns == 0:
            return res  # a model without sensors: [N, 0, .] and nothing to launch
        slots, ws = self._sensor_fd_workspace(slots, centered, "D" in want)
        io.eps = default_eps(self.dtype) if eps is None else float(eps)
        io.flags = cabi.MGX_FD_CENTERED if centered else 0
        io.workspace, io.workspace_bytes, io.slots = ws.data_ptr(), ws.numel(), slots
        check(lib().mgx_sensor_fd(self.native.handle, C.byref(self._state), C.byref(io), n, _ptr(mask),
                                  _stream(stream)), "mgx_sensor_fd")
        return res

    def sensor_fd_along(self, state0: torch.Tensor, ctrl: torch.Tensor, warmstart: Optional[torch.Tensor] = None,
                        eps: Optional[float] = None, centered: bool = False, slots: Optional[int] = None,
                        only: Optional[Sequence[str]] = None) -> SensorFdResult:
        """``sensor_fd`` at the T states of a trajectory per env: ``state0`` [N, T, nstate], ``ctrl``
        [N, T, nu] and ``warmstart`` [N, T, nv] (default: the env's own at every t). Returns C
        [N, T, ns, 2nv], D [N, T, ns, nu] and sensordata [N, T, ns] (``only`` as in ``sensor_fd``).

        Built like ``transition_fd_along``: mgx_sensor_fd runs over the N T stacked rows, held in a
        second batch that shares this one's compiled model, with each env's qfrc_applied and
        xfrc_applied repeated. Nothing is written to this batch's state. Tensors are owned by the
        batch and overwritten by the next call with the same T."""
        from .batch import PhysicsBatch
        n, m = self.n, self.model
        nq, nv, nu, nst = int(m.nq), int(m.nv), int(m.nu), 1 + int(m.nq) + int(m.nv)
        if state0.dim() != 3 or state0.shape[0] != n or state0.shape[2] != nst:
            raise ValueError(f"state0 must be [N, T, nstate], got {tuple(state0.shape)}")
        t = int(state0.shape[1])
        if tuple(ctrl.shape) != (n, t, nu):
            raise ValueError(f"ctrl must be [N, T, nu] = {[n, t, nu]}, got {tuple(ctrl.shape)}")
        if warmstart is not None and tuple(warmstart.shape) != (n, t, nv):
            raise ValueError(f"warmstart must be [N, T, nv] = {[n, t, nv]}, got {tuple(warmstart.shape)}")
        self._sensor_ready()
        cache = self.__dict__.setdefault("_sensor_fd_along", {})
        if t not in cache:
            cache[t] = PhysicsBatch(m, n * t, precision="f64" if self.dtype == torch.float64 else "f32",
                                    device=str(self.device), native=self.native)
        tb = cache[t]
        x = state0.to(self.dtype).reshape(n * t, nst)
        tb.time.copy_(x[:, 0])
        tb.qpos.copy_(x[:, 1:1 + nq])
        tb.qvel.copy_(x[:, 1 + nq:])
        tb.ctrl[:, :nu] = ctrl.to(self.dtype).reshape(n * t, nu)
        tb.qacc_warmstart.copy_(self.qacc_warmstart.repeat_interleave(t, dim=0) if warmstart is None
                                else warmstart.to(self.dtype).reshape(n * t, nv))
        tb.qfrc_applied.copy_(self.qfrc_applied.repeat_interleave(t, dim=0))
        tb.xfrc_applied.copy_(self.xfrc_applied.repeat_interleave(t, dim=0))
        r = tb.sensor_fd(eps=eps, centered=centered, slots=slots, only=only)
        view = lambda x: None if x is None else x.view((n, t) + tuple(x.shape[1:]))  # noqa: E731
        return SensorFdResult(C=view(r.C), D=view(r.D), sensordata=view(r.sensordata))


class SensorFdForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``sensor_fd`` under the env's name."""

    def sensor_fd(self, **kw):
        """PhysicsBatch.sensor_fd of this env's batch (sensor derivatives at its current state)."""
        return self.batch.sensor_fd(**kw)

    def sensor_fd_along(self, state0, ctrl, **kw):
        """PhysicsBatch.sensor_fd_along of this env's batch."""
        return self.batch.sensor_fd_along(state0, ctrl, **kw)

    def sensor_fd_columns(self, centered: bool = False, with_d: bool = True) -> int:
        return self.batch.sensor_fd_columns(centered, with_d)
