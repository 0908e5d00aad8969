"""Batched inverse kinematics on the device (mgx_ik, include/mgx.h): damped least squares, the
whole iteration loop of every env in one launch.

``IkMethods`` gives :class:`~.batch.PhysicsBatch` its ``ik_targets`` / ``solve_ik``; ``IkForwarding``
gives the ``*VectorEnv`` classes the same calls, forwarded to their batch.

The targets are the points of ``jac_points`` (a site, a body frame, a geom centre ...): each gets a
world position and, with a rotation weight, a world orientation. The start is the CURRENT ``qpos``
unless ``qpos_init`` is given, and nothing in the batch's state is written unless ``apply=True``.
What the algorithm does, step by step, and what it does not provide (posture objectives, collision
avoidance, per-env weights, velocity IK, a line search) is in include/mgx.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import cabi
from .dynamics import JacPoints, _as_list, _check_mask, _resolve
from .native import check, lib
from .sensors import _ptr, _stream

IK_STATUS = ("converged", "max_iter", "failed")  # IkResult.status codes 0, 1, 2 (include/mgx.h MGX_IK_*)


class IkTargets:
    """The targets of a ``solve_ik()`` call, built once by ``PhysicsBatch.ik_targets``: the points,
    their orientation offsets in the body frame (``quat`` [P, 4] on the device: a site's or geom's
    own orientation), the weights (host, one per point) and ``dof_mask`` (uint8 [nv] on the device,
    or None: every dof may move)."""

    __slots__ = ("points", "quat", "pos_weight", "rot_weight", "dof_mask", "result")

    def __init__(self, points, quat, pos_weight, rot_weight, dof_mask):
        self.points, self.quat, self.dof_mask = points, quat, dof_mask
        self.pos_weight, self.rot_weight = list(pos_weight), list(rot_weight)
        self.result = None  # the batch's IkResult for these targets, allocated by the first solve_ik()

    def __len__(self):
        return len(self.points)


class IkResult:
    """qpos [N, nq]; residual [N], the weighted error norm at ``qpos``; iters [N] int32, the updates
    applied; status [N] int32: 0 converged (residual <= tol), 1 max_iter reached, 2 failed (a
    non-finite residual or pivot). Owned by the batch per targets object and overwritten by the
    next call."""

    __slots__ = ("qpos", "residual", "iters", "status")

    def __init__(self, n, nq, dtype, device):
        self.qpos = torch.zeros(n, nq, dtype=dtype, device=device)
        self.residual = torch.zeros(n, dtype=dtype, device=device)
        self.iters = torch.zeros(n, dtype=torch.int32, device=device)
        self.status = torch.zeros(n, dtype=torch.int32, device=device)

    def rows(self, a: int, b: int) -> "IkResult":
        r = object.__new__(IkResult)
        r.qpos, r.residual, r.iters, r.status = self.qpos[a:b], self.residual[a:b], self.iters[a:b], self.status[a:b]
        return r


def _per_point(x, n: int, what: str):
    w = [float(x)] * n if isinstance(x, (int, float, np.integer, np.floating)) else [float(v) for v in x]
    if len(w) != n:
        raise ValueError(f"{what}: {len(w)} weights for {n} points")
    return w


class IkMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype, qpos and state)."""

    def ik_targets(self, points: JacPoints, pos_weight=1.0, rot_weight=0.0,
                   dofs: Optional[Sequence] = None) -> IkTargets:
        """Targets of later ``solve_ik()`` calls from the points of ``jac_points``. The weights are
        scalars or one per point, >= 0; a zero weight drops those three rows. A rotation weight
        needs a point with a frame (body, site, geom): on a ``com`` / ``subtree_com`` point it raises
        ValueError. ``dofs``: joint names or ids whose dofs may move (None: all); unknown names
        raise KeyError naming what the model has."""
        m, n = self.model, len(points)
        if not 1 <= n <= cabi.MGX_IK_MAX_POINT:
            raise ValueError(f"an IK problem takes 1 to {cabi.MGX_IK_MAX_POINT} points, not {n}")
        wp, wr = _per_point(pos_weight, n, "pos_weight"), _per_point(rot_weight, n, "rot_weight")
        quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
        for p, name in enumerate(points.names):
            what, _, label = name.partition(":")
            if what in ("com", "subtree_com"):
                if wr[p] > 0:
                    raise ValueError(f"{name} has no orientation: rot_weight must be 0 for com / subtree_com points")
            elif what == "site":
                quat[p] = np.asarray(m.site_quat).reshape(-1, 4)[list(m.site_names).index(label)]
            elif what == "geom":
                quat[p] = np.asarray(m.geom_quat).reshape(-1, 4)[list(m.geom_names).index(label)]
        mask = None
        if dofs is not None:
            host = np.zeros(int(m.nv), dtype=np.uint8)
            dofnum = {0: 6, 1: 3}  # free, ball; slide and hinge: 1
            for x in _as_list(dofs):
                j = _resolve(m.jnt_names, "joint", x)
                a = int(m.jnt_dofadr[j])
                host[a:a + dofnum.get(int(m.jnt_type[j]), 1)] = 1
            mask = torch.from_numpy(host).to(self.device)
        return IkTargets(points, torch.tensor(quat, dtype=self.dtype, device=self.device).contiguous(), wp, wr, mask)

    def solve_ik(self, targets: IkTargets, target_pos: torch.Tensor, target_quat: Optional[torch.Tensor] = None,
                 qpos_init: Optional[torch.Tensor] = None, damping: float = 0.05, max_step: float = 0.3,
                 tol: float = 1e-6, max_iter: int = 50, clamp_limits: bool = True, apply: bool = False,
                 mask: Optional[torch.Tensor] = None, stream=None, out: Optional[IkResult] = None) -> IkResult:
        """Damped-least-squares IK for every (masked) env, asynchronously on the stream:
        ``IkResult(qpos, residual, iters, status)``. ``target_pos`` [N, P, 3] and ``target_quat``
        [N, P, 4] (needed with a rotation weight; normalised by the kernel) are world poses on the
        device; ``qpos_init`` [N, nq] replaces the current ``qpos`` as the start. Per iteration the
        update solves (J J' + damping^2 I) y = e, limits max |J' y| to ``max_step`` and integrates
        it into qpos (``clamp_limits``: limited hinges and slides stay in their range); it stops at
        a weighted error norm <= ``tol`` or after ``max_iter`` updates. The tensors are allocated
        once per targets object and overwritten by the next call (``out`` writes into a caller's
        IkResult); rows of envs that ``mask`` (uint8 [N]) deselects are left as they were.
        ``apply=True`` also copies the result into the batch's ``qpos`` for the selected envs."""
        n, p, nq = self.n, len(targets), int(self.model.nq)
        _check_mask(mask, n)
        if out is None:
            if targets.result is None:
                targets.result = IkResult(n, nq, self.dtype, self.device)
            out = targets.result
        assert tuple(out.qpos.shape) == (n, nq)
        for t, dt in ((out.qpos, self.dtype), (out.residual, self.dtype), (out.iters, torch.int32),
                      (out.status, torch.int32)):
            assert t.dtype == dt and t.is_contiguous() and t.is_cuda and t.shape[0] == n
        for t, shape in ((target_pos, (n, p, 3)), (target_quat, (n, p, 4)), (qpos_init, (n, nq))):
            if t is not None:
                assert t.dtype == self.dtype and tuple(t.shape) == shape and t.is_cuda and t.is_contiguous()
        io = cabi.MgxIkIO()
        for i in range(p):
            io.pos_weight[i], io.rot_weight[i] = targets.pos_weight[i], targets.rot_weight[i]
        io.damping, io.max_step, io.tol, io.max_iter = float(damping), float(max_step), float(tol), int(max_iter)
        io.flags = cabi.MGX_IK_CLAMP_LIMITS if clamp_limits else 0
        io.target_pos = None if target_pos is None else target_pos.data_ptr()
        io.target_quat = None if target_quat is None else target_quat.data_ptr()
        io.dof_mask = None if targets.dof_mask is None else targets.dof_mask.data_ptr()
        io.qpos_init = None if qpos_init is None else qpos_init.data_ptr()
        io.qpos, io.residual = out.qpos.data_ptr(), out.residual.data_ptr()
        io.iters, io.status = out.iters.data_ptr(), out.status.data_ptr()
        pts = targets.points
        check(lib().mgx_ik(self.native.handle, C.byref(self._state), p, _ptr(pts.body), _ptr(pts.kind), _ptr(pts.pos),
                           _ptr(targets.quat), C.byref(io), n, _ptr(mask), _stream(stream)), "mgx_ik")
        if apply:
            cs = stream if stream is not None else torch.cuda.current_stream(self.device)
            with torch.cuda.stream(cs):
                if mask is None:
                    self.qpos.copy_(out.qpos)
                else:
                    torch.where(mask.bool()[:, None], out.qpos, self.qpos, out=self.qpos)
        return out


class IkForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's IK calls under the env's name."""

    def ik_targets(self, points, **kw):
        """PhysicsBatch.ik_targets of this env's batch."""
        return self.batch.ik_targets(points, **kw)

    def solve_ik(self, targets, target_pos, **kw):
        """PhysicsBatch.solve_ik of this env's batch (the start is the current qpos)."""
        return self.batch.solve_ik(targets, target_pos, **kw)
