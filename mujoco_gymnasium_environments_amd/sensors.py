"""Batched sensors, mj_forward and contact forces on the device (mgx_sensor / mgx_forward,
include/mgx.h).

``SensorMethods`` gives :class:`~.batch.PhysicsBatch` its ``sensors`` / ``sensor_slices`` /
``sensordata`` / ``sensor`` / ``forward``; ``SensorForwarding`` gives the ``*VectorEnv`` classes
the same calls, forwarded to their batch.

Every value is that of the CURRENT state (``qpos``, ``qvel``, ``ctrl``, applied forces): what
``mj_forward(model, data)`` would put in ``data.sensordata`` / ``data.qacc`` / ``data.contact``
now. It is not the pre-integration value an ``mj_step`` leaves in ``data.sensordata``, the same
choice ``rays.py`` makes for geom poses. No call writes to the batch's state.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import cabi, mjcf
from .native import check, lib

# sensor types that read the acceleration stage (qacc, contacts and their forces): these make
# sensordata() run the forward kernel first
ACC_SENSORS = tuple(mjcf.SENSOR_TYPES.index(t) for t in ("accelerometer", "force", "torque", "touch"))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class ForwardResult:
    """Outputs of ``PhysicsBatch.forward()``: views of tensors the batch owns and overwrites on
    the next ``forward()`` / ``sensordata()``. ``C`` is the model's contact capacity; slots at
    ``ncon`` and above hold 0 (``contact_geom``: -1).

    qacc, qfrc_constraint [N, nv]; ncon [N] int32; contact_geom [N, C, 2] int32; contact_dist
    [N, C]; contact_pos [N, C, 3]; contact_frame [N, C, 9] (rows: normal, two tangents);
    contact_force [N, C, 6]: mj_contactForce, the wrench in the contact frame."""

    __slots__ = ("qacc", "qfrc_constraint", "ncon", "contact_geom", "contact_dist", "contact_pos", "contact_frame",
                 "contact_force")

    def __init__(self, n, nv, ncon_max, dtype, device):
        z = lambda *shape, dt=dtype: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        self.qacc, self.qfrc_constraint = z(n, nv), z(n, nv)
        self.ncon = z(n, dt=torch.int32)
        self.contact_geom = z(n, ncon_max, 2, dt=torch.int32)
        self.contact_dist, self.contact_pos = z(n, ncon_max), z(n, ncon_max, 3)
        self.contact_frame, self.contact_force = z(n, ncon_max, 9), z(n, ncon_max, 6)

    def desc(self) -> cabi.MgxForwardOut:
        return cabi.MgxForwardOut(*[getattr(self, f).data_ptr() for f in self.__slots__])


class SensorMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and state)."""

    @property
    def sensors(self) -> List[str]:
        """Names of the model's sensors, in document order."""
        return list(self.model.sensor_names)

    @property
    def sensor_slices(self) -> Dict[str, slice]:
        """Sensor name -> its slice of a sensordata row."""
        m = self.model
        return {n: slice(int(a), int(a) + int(d)) for n, a, d in zip(m.sensor_names, m.sensor_adr, m.sensor_dim)}

    # ------------------------------------------------------------------ set-up, once
    def _forward_buffers(self) -> ForwardResult:
        if getattr(self, "_fwd_out", None) is None:
            self._fwd_out = ForwardResult(self.n, self.model.nv, int(self.native.info.max_ncon), self.dtype,
                                          self.device)
            self._fwd_desc = self._fwd_out.desc()
        return self._fwd_out

    def _sensor_ready(self) -> None:
        nat = self.native
        if getattr(nat, "_sensor_packed", None) is None:
            packed = cabi.PackedSensor(self.model)
            check(lib().mgx_sensor_configure(nat.handle, C.byref(packed.desc)), "mgx_sensor_configure")
            nat._sensor_packed = packed
        if getattr(self, "_sensor_out", None) is None:
            self._sensor_acc = bool(np.isin(np.asarray(self.model.sensor_type), ACC_SENSORS).any())
            self._sensor_out = torch.zeros(self.n, int(self.model.nsensordata), dtype=self.dtype, device=self.device)

    @staticmethod
    def _check_sensor_mask(mask, n):
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()

    # ------------------------------------------------------------------ API
    def forward(self, mask: Optional[torch.Tensor] = None, stream=None) -> ForwardResult:
        """mj_forward for every (masked) env at the current state, asynchronously on the stream:
        accelerations, constraint forces, the contact list and mj_contactForce of every contact
        (``ForwardResult``). The solver is warm-started from ``qacc_warmstart`` but nothing of the
        batch's state is written. Rows of envs that ``mask`` (uint8 [N]) deselects keep their
        previous contents."""
        self._check_sensor_mask(mask, self.n)
        out = self._forward_buffers()
        check(lib().mgx_forward(self.native.handle, C.byref(self._state), C.byref(self._fwd_desc), self.n, _ptr(mask),
                                _stream(stream)), "mgx_forward")
        return out

    def sensordata(self, mask: Optional[torch.Tensor] = None, stream=None, out: Optional[torch.Tensor] = None
                   ) -> torch.Tensor:
        """``data.sensordata`` of every (masked) env at the current state, [N, nsensordata] in the
        batch dtype (``sensor_slices`` maps names to columns). Runs the forward kernel first only
        when the model has an accelerometer, force, torque or touch sensor. The tensor is
        allocated once and overwritten by the next call (``out`` writes into a caller tensor
        instead); rows of envs that ``mask`` deselects are left as they were."""
        self._sensor_ready()
        self._check_sensor_mask(mask, self.n)
        if out is None:
            out = self._sensor_out
        else:
            assert out.dtype == self.dtype and tuple(out.shape) == tuple(self._sensor_out.shape) and out.is_contiguous()
        if out.shape[1] == 0:
            return out
        fwd = None
        if self._sensor_acc:
            self.forward(mask=mask, stream=stream)
            fwd = C.byref(self._fwd_desc)
        check(lib().mgx_sensor(self.native.handle, C.byref(self._state), fwd, _ptr(out), self.n, _ptr(mask),
                               _stream(stream)), "mgx_sensor")
        return out

    def sensor(self, name: str, mask: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """One sensor's columns of a fresh ``sensordata()``: a view [N, dim]."""
        sl = self.sensor_slices
        if name not in sl:
            raise KeyError(f"unknown sensor {name!r}; the model has {self.sensors}")
        return self.sensordata(mask=mask, stream=stream)[:, sl[name]]


class SensorForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's sensor calls under the env's name."""

    @property
    def sensors(self) -> List[str]:
        return self.batch.sensors

    @property
    def sensor_slices(self) -> Dict[str, slice]:
        return self.batch.sensor_slices

    def sensordata(self, **kw):
        """PhysicsBatch.sensordata of this env's batch (sensors at the current state)."""
        return self.batch.sensordata(**kw)

    def sensor(self, name, **kw):
        """PhysicsBatch.sensor of this env's batch."""
        return self.batch.sensor(name, **kw)

    def forward(self, **kw):
        """PhysicsBatch.forward of this env's batch (mj_forward at the current state)."""
        return self.batch.forward(**kw)
