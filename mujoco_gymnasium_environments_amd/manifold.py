"""The two operations of the state manifold on the device (mgx_state_diff, mgx_state_integrate,
include/mgx.h): MuJoCo's ``mj_differentiatePos`` / ``mj_integratePos`` on whole state rows.

``ManifoldMethods`` gives :class:`~.batch.PhysicsBatch` its ``state_difference`` /
``state_integrate``; ``ManifoldForwarding`` gives the ``*VectorEnv`` classes the same calls.

A state row is ``[time, qpos, qvel]`` (``state_size`` reals, as ``get_state`` and ``rollout`` give
it); its tangent is ``(dq [nv], dqvel [nv])``, the coordinates of ``transition_fd``'s A and B. Every
model here has a free joint, so costs and feedback written with plain subtraction on ``qpos`` are
wrong: a quaternion contributes the rotation vector of ``conj(q_b) o q_a``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .native import check, lib
from .sensors import _stream


class ManifoldMethods:
    """Mixin of PhysicsBatch (uses its model, native, device, dtype and state_size)."""

    def _rows(self, x: torch.Tensor, width: int, name: str) -> torch.Tensor:
        if x.shape[-1] != width:
            raise ValueError(f"{name} must be [..., {width}], got {tuple(x.shape)}")
        assert x.dtype == self.dtype and x.is_cuda, name
        return x

    def state_difference(self, xa: torch.Tensor, xb: torch.Tensor, out: Optional[torch.Tensor] = None,
                         stream=None) -> torch.Tensor:
        """``xa (-) xb`` [..., 2nv]: ``(mj_differentiatePos(qpos_a from qpos_b), qvel_a - qvel_b)``
        of state rows [..., nstate]; time is ignored. ``xb`` broadcasts over leading dims of size 1
        (and over missing leading dims): a single row is read in place, anything else is expanded."""
        ns, nv = self.state_size, int(self.model.nv)
        xa = self._rows(xa, ns, "xa").contiguous()
        xb = self._rows(xb, ns, "xb")
        rows = xa.numel() // ns
        if xb.numel() == ns and rows != 1:
            xb, xb_rows = xb.contiguous(), 1
        else:
            xb, xb_rows = xb.expand(xa.shape).contiguous(), rows
        if out is None:
            out = torch.empty(xa.shape[:-1] + (2 * nv,), dtype=self.dtype, device=self.device)
        assert out.is_contiguous() and out.dtype == self.dtype and tuple(out.shape) == tuple(xa.shape[:-1]) + (2 * nv,)
        check(lib().mgx_state_diff(self.native.handle, xa.data_ptr(), xb.data_ptr(), out.data_ptr(), rows, xb_rows,
                                   _stream(stream)), "mgx_state_diff")
        return out

    def state_integrate(self, x: torch.Tensor, dx: torch.Tensor, out: Optional[torch.Tensor] = None,
                        stream=None) -> torch.Tensor:
        """``x (+) dx`` [..., nstate]: qpos moved along ``dx[..., :nv]`` by ``mj_integratePos`` (as
        the step does it), qvel plus ``dx[..., nv:]``, time kept. ``out`` may be ``x`` itself."""
        ns, nv = self.state_size, int(self.model.nv)
        x = self._rows(x, ns, "x")
        dx = self._rows(dx, 2 * nv, "dx").contiguous()
        if tuple(x.shape[:-1]) != tuple(dx.shape[:-1]):
            raise ValueError(f"x {tuple(x.shape)} and dx {tuple(dx.shape)} must have the same leading shape")
        if out is None:
            x = x.contiguous()
            out = torch.empty_like(x)
        assert x.is_contiguous() and out.is_contiguous() and out.dtype == self.dtype and out.shape == x.shape
        check(lib().mgx_state_integrate(self.native.handle, x.data_ptr(), dx.data_ptr(), out.data_ptr(), x.numel() // ns,
                                        _stream(stream)), "mgx_state_integrate")
        return out


class ManifoldForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's state-manifold operations."""

    def state_difference(self, xa, xb, **kw):
        return self.batch.state_difference(xa, xb, **kw)

    def state_integrate(self, x, dx, **kw):
        return self.batch.state_integrate(x, dx, **kw)
