"""Batched Jacobians, mass matrix, inverse dynamics and energy on the device (mgx_jac /
mgx_dynamics, include/mgx.h).

``DynamicsMethods`` gives :class:`~.batch.PhysicsBatch` its ``jac_points`` / ``jac`` /
``jac_world`` / ``dynamics`` / ``mass_matrix`` / ``energy``; ``DynamicsForwarding`` gives the
``*VectorEnv`` classes the same calls, forwarded to their batch.

Every value is that of the CURRENT state (``qpos``, ``qvel``, ``ctrl``, applied forces), as after
``mj_forward(model, data)``: the choice ``rays.py`` and ``sensors.py`` make. No call writes to the
batch's state. What MuJoCo users get from ``mj_jac*``, ``mj_fullM``, ``data.qfrc_bias`` /
``qfrc_passive`` / ``qfrc_actuator``, ``mj_inverse``'s sum and ``mj_energyPos`` / ``mj_energyVel``.
The constraint force of the inverse dynamics is an input (``forward().qfrc_constraint``): there is
no analytic constraint inverse. ``mj_mulM`` / ``mj_solveM`` are ``torch.bmm`` /
``torch.linalg.solve`` on the dense ``M``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import cabi
from .native import check, lib
from .sensors import _ptr, _stream

DYN_OUTPUTS = ("M", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qfrc_external", "qfrc_inverse", "energy")


class JacPoints:
    """The points of a ``jac()`` call: device tables built once by ``PhysicsBatch.jac_points``.

    names: the ordered point names (``body:torso``, ``site:ee_site``, ``com:pelvis`` ...);
    body, kind: int32 [P] on the device; pos: [P, 3] in the batch dtype (body-frame offsets)."""

    __slots__ = ("names", "body", "kind", "pos", "result")

    def __init__(self, names, body, kind, pos):
        self.names, self.body, self.kind, self.pos = list(names), body, kind, pos
        self.result = None  # the batch's JacResult for these points, allocated by the first jac()

    def __len__(self):
        return len(self.names)

    def index(self, name: str) -> int:
        return self.names.index(name)


class JacResult:
    """jacp, jacr [N, P, 3, nv] (translational / rotational, MuJoCo's layout per point) and point
    [N, P, 3], the world point used. Owned by the batch per points object and overwritten by the
    next call."""

    __slots__ = ("jacp", "jacr", "point")

    def __init__(self, n, p, nv, dtype, device):
        self.jacp = torch.zeros(n, p, 3, nv, dtype=dtype, device=device)
        self.jacr = torch.zeros(n, p, 3, nv, dtype=dtype, device=device)
        self.point = torch.zeros(n, p, 3, dtype=dtype, device=device)

    def rows(self, a: int, b: int) -> "JacResult":
        r = object.__new__(JacResult)
        r.jacp, r.jacr, r.point = self.jacp[a:b], self.jacr[a:b], self.point[a:b]
        return r


class DynamicsResult:
    """M [N, nv, nv]; qfrc_bias, qfrc_passive, qfrc_actuator, qfrc_external, qfrc_inverse [N, nv]
    (qfrc_inverse is None when no qacc was given); energy [N, 2] (potential, kinetic). A field the
    call did not request is None. Tensors are owned by the batch and overwritten by the next call."""

    __slots__ = DYN_OUTPUTS

    def __init__(self, **fields):
        for f in DYN_OUTPUTS:
            setattr(self, f, fields.get(f))

    def rows(self, a: int, b: int) -> "DynamicsResult":
        return DynamicsResult(**{f: None if getattr(self, f) is None else getattr(self, f)[a:b] for f in DYN_OUTPUTS})


def alloc_dynamics(n, nv, dtype, device) -> DynamicsResult:
    z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return DynamicsResult(M=z(n, nv, nv), energy=z(n, 2),
                          **{f: z(n, nv) for f in DYN_OUTPUTS if f not in ("M", "energy")})


def _resolve(names: Sequence[str], what: str, x) -> int:
    """id of a body / site / geom given by name or id; KeyError names what the model has."""
    if isinstance(x, (int, np.integer)):
        if not 0 <= int(x) < len(names):
            raise KeyError(f"{what} id {int(x)} out of range: the model has {len(names)}")
        return int(x)
    names = list(names)
    if x not in names:
        raise KeyError(f"unknown {what} {x!r}; the model has {names}")
    return names.index(x)


def _check_mask(mask, n):
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()


def _as_list(x):
    return [x] if isinstance(x, (str, int, np.integer)) else list(x)


class DynamicsMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and state)."""

    # ------------------------------------------------------------------ Jacobians
    def jac_points(self, body=(), site=(), geom=(), com=(), subtree_com=()) -> JacPoints:
        """The points of later ``jac()`` calls, by name or id, in this order: body frame origins
        (mj_jacBody), sites (mj_jacSite), geom centres (mj_jacGeom), body centres of mass
        (mj_jacBodyCom) and subtree centres of mass (mj_jacSubtreeCom, a body). Unknown names raise
        KeyError."""
        m = self.model
        names: List[str] = []
        bodies: List[int] = []
        kinds: List[int] = []
        pos: List[Sequence[float]] = []

        def add(label, b, kind, p=(0.0, 0.0, 0.0)):
            names.append(label)
            bodies.append(int(b))
            kinds.append(kind)
            pos.append([float(v) for v in p])

        for x in _as_list(body):
            b = _resolve(m.body_names, "body", x)
            add(f"body:{m.body_names[b]}", b, cabi.MGX_JAC_LOCAL)
        for x in _as_list(site):
            s = _resolve(m.site_names, "site", x)
            add(f"site:{m.site_names[s]}", m.site_bodyid[s], cabi.MGX_JAC_LOCAL, np.asarray(m.site_pos).reshape(-1, 3)[s])
        for x in _as_list(geom):
            g = _resolve(m.geom_names, "geom", x)
            add(f"geom:{m.geom_names[g]}", m.geom_bodyid[g], cabi.MGX_JAC_LOCAL, np.asarray(m.geom_pos).reshape(-1, 3)[g])
        for x in _as_list(com):
            b = _resolve(m.body_names, "body", x)
            add(f"com:{m.body_names[b]}", b, cabi.MGX_JAC_BODYCOM)
        for x in _as_list(subtree_com):
            b = _resolve(m.body_names, "body", x)
            add(f"subtree_com:{m.body_names[b]}", b, cabi.MGX_JAC_SUBTREECOM)
        if not names:
            raise ValueError("jac_points needs at least one point")
        dev = self.device
        return JacPoints(names, torch.tensor(bodies, dtype=torch.int32, device=dev),
                         torch.tensor(kinds, dtype=torch.int32, device=dev),
                         torch.tensor(pos, dtype=self.dtype, device=dev).reshape(-1, 3).contiguous())

    def _jac_call(self, body, kind, pos, per_env, res: JacResult, mask, stream):
        _check_mask(mask, res.point.shape[0])
        for t in (res.jacp, res.jacr, res.point):
            assert t.dtype == self.dtype and t.is_contiguous()
        check(lib().mgx_jac(self.native.handle, C.byref(self._state), int(body.numel()), _ptr(body), _ptr(kind),
                            _ptr(pos), int(per_env), _ptr(res.jacp), _ptr(res.jacr), _ptr(res.point),
                            int(res.point.shape[0]), _ptr(mask), _stream(stream)), "mgx_jac")
        return res

    def jac(self, points: JacPoints, mask: Optional[torch.Tensor] = None, stream=None,
            out: Optional[JacResult] = None) -> JacResult:
        """The Jacobians of ``points`` for every (masked) env at the current state, asynchronously
        on the stream: ``JacResult(jacp, jacr, point)``. Column d of a point is zero unless dof d
        moves it; jacr of a subtree-COM point is 0. The tensors are allocated once per points
        object and overwritten by the next call (``out`` writes into a caller's JacResult); rows
        of envs that ``mask`` (uint8 [N]) deselects are left as they were."""
        if out is None:
            if points.result is None:
                points.result = JacResult(self.n, len(points), self.model.nv, self.dtype, self.device)
            out = points.result
        assert tuple(out.point.shape) == (self.n, len(points), 3)
        return self._jac_call(points.body, points.kind, points.pos, 0, out, mask, stream)

    def jac_world(self, body_ids, pos: torch.Tensor, mask: Optional[torch.Tensor] = None, stream=None,
                  out: Optional[JacResult] = None) -> JacResult:
        """mj_jac for per-env world points: ``pos`` [N, P, 3] on the device (contact points for
        instance), each attached to body ``body_ids[p]`` (ids, or an int32 device tensor [P])."""
        nb = int(self.model.nbody)
        if isinstance(body_ids, torch.Tensor):
            body = body_ids.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            ids = [int(b) for b in _as_list(body_ids)]
            if any(not 0 <= b < nb for b in ids):
                raise KeyError(f"body id out of range: the model has {nb} bodies")
            body = torch.tensor(ids, dtype=torch.int32, device=self.device)
        p = int(body.numel())
        if p < 1:
            raise ValueError("jac_world needs at least one point")
        assert pos.dtype == self.dtype and tuple(pos.shape) == (self.n, p, 3) and pos.is_cuda and pos.is_contiguous()
        cache = self.__dict__.setdefault("_jac_world", {})
        if p not in cache:
            cache[p] = (torch.zeros(p, dtype=torch.int32, device=self.device),
                        JacResult(self.n, p, self.model.nv, self.dtype, self.device))
        kind, res = cache[p]  # kind: all MGX_JAC_WORLD (0)
        return self._jac_call(body, kind, pos, 1, res if out is None else out, mask, stream)

    # ------------------------------------------------------------------ dynamics
    def _dyn_buffers(self) -> DynamicsResult:
        if getattr(self, "_dyn_out", None) is None:
            self._dyn_out = alloc_dynamics(self.n, self.model.nv, self.dtype, self.device)
        return self._dyn_out

    def dynamics(self, qacc: Optional[torch.Tensor] = None, qfrc_constraint: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, stream=None, only: Optional[Sequence[str]] = None,
                 out: Optional[DynamicsResult] = None) -> DynamicsResult:
        """Mass matrix, force vectors, inverse dynamics and energy of every (masked) env at the
        current state, asynchronously on the stream (``DynamicsResult``). ``qfrc_inverse`` = M qacc
        + qfrc_bias - qfrc_passive - qfrc_constraint needs ``qacc`` [N, nv] (None without it;
        ``qfrc_constraint`` None means 0); with the ``qacc`` / ``qfrc_constraint`` of ``forward()``
        at the same state it equals qfrc_actuator + qfrc_external. ``only`` names the outputs to
        compute (the kernel skips the stages nothing needs); rows of envs that ``mask`` deselects
        are left as they were."""
        n, nv = self.n, int(self.model.nv)
        _check_mask(mask, n)
        want = list(DYN_OUTPUTS) if only is None else list(only)
        for f in want:
            if f not in DYN_OUTPUTS:
                raise KeyError(f"unknown dynamics output {f!r}; there are {list(DYN_OUTPUTS)}")
        if qacc is None and only is None:
            want.remove("qfrc_inverse")  # asked for by name without qacc, the library refuses it (MGX_E_ARG)
        for t in (qacc, qfrc_constraint):
            if t is not None:
                assert t.dtype == self.dtype and tuple(t.shape) == (n, nv) and t.is_cuda and t.is_contiguous()
        buf = self._dyn_buffers() if out is None else out
        io = cabi.MgxDynIO()
        io.qacc = None if qacc is None else qacc.data_ptr()
        io.qfrc_constraint = None if qfrc_constraint is None else qfrc_constraint.data_ptr()
        res = DynamicsResult()
        for f in want:
            t = getattr(buf, f)
            assert t is not None and t.dtype == self.dtype and t.is_contiguous() and t.shape[0] == n
            setattr(io, f, t.data_ptr())
            setattr(res, f, t)
        check(lib().mgx_dynamics(self.native.handle, C.byref(self._state), C.byref(io), n, _ptr(mask),
                                 _stream(stream)), "mgx_dynamics")
        return res

    def mass_matrix(self, mask: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """The dense joint-space inertia matrix [N, nv, nv] (mj_fullM); only that output is computed."""
        return self.dynamics(mask=mask, stream=stream, only=("M",)).M

    def energy(self, mask: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """[N, 2]: potential and kinetic energy (mj_energyPos / mj_energyVel); only that output."""
        return self.dynamics(mask=mask, stream=stream, only=("energy",)).energy


class DynamicsForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's Jacobian and dynamics calls under the env's
    name."""

    def jac_points(self, **kw):
        """PhysicsBatch.jac_points of this env's batch."""
        return self.batch.jac_points(**kw)

    def jac(self, points, **kw):
        """PhysicsBatch.jac of this env's batch (Jacobians at the current state)."""
        return self.batch.jac(points, **kw)

    def jac_world(self, body_ids, pos, **kw):
        """PhysicsBatch.jac_world of this env's batch."""
        return self.batch.jac_world(body_ids, pos, **kw)

    def dynamics(self, **kw):
        """PhysicsBatch.dynamics of this env's batch."""
        return self.batch.dynamics(**kw)

    def mass_matrix(self, **kw):
        return self.batch.mass_matrix(**kw)

    def energy(self, **kw):
        return self.batch.energy(**kw)
