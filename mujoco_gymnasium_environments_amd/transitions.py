"""Batched finite-difference transition derivatives on the device (mgx_transition_fd,
include/mgx.h): MuJoCo's ``mjd_transitionFD``.

``TransitionMethods`` gives :class:`~.batch.PhysicsBatch` its ``transition_fd``;
``TransitionForwarding`` gives the ``*VectorEnv`` classes the same call, forwarded to their batch.

``A = dx'/dx`` [N, 2nv, 2nv] and ``B = dx'/dctrl`` [N, 2nv, nu] linearise ``nsub`` ``mj_step``s
from the CURRENT state, with the state tangent ``x = (dq, qvel)``: quaternion coordinates are
perturbed and differenced in the tangent space (``mj_integratePos`` / ``mj_differentiatePos``). The
call steps virtual copies of the envs in a workspace of its own with the library's own step; it
writes nothing to the batch's state.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import cabi
from .native import check, lib
from .sensors import _ptr, _stream

FD_OUTPUTS = ("A", "B", "next_qpos", "next_qvel", "warning")
WORKSPACE_LIMIT = 1 << 30  # slots=None keeps the workspace under this many bytes (one env at least)


def default_eps(dtype) -> float:
    """1e-6 in fp64 (MuJoCo's own default) and 2**-10 in fp32. The step's rounding error, some tens
    of ulp of x', is divided by eps while the truncation error grows with eps: in fp32 (ulp 6e-8)
    1e-6 would leave no correct digit, and 2**-10, near the square root of the ulp, balances the
    two at about 1e-3 of max(1, |x'|); a power of two makes the perturbing add and the division
    exact in the exponent."""
    return 1e-6 if dtype == torch.float64 else 2.0 ** -10


class TransitionResult:
    """A [N, 2nv, 2nv], B [N, 2nv, nu], next_qpos [N, nq], next_qvel [N, nv] (the nominal next
    state) and warning int32 [N] (bad-state resets among the env's steps: 0 means every column is
    valid). A field the call did not request is None. Tensors are owned by the batch and overwritten
    by the next call."""

    __slots__ = FD_OUTPUTS

    def __init__(self, **fields):
        for f in FD_OUTPUTS:
            setattr(self, f, fields.get(f))

    def rows(self, a: int, b: int) -> "TransitionResult":
        return TransitionResult(**{f: None if getattr(self, f) is None else getattr(self, f)[a:b] for f in FD_OUTPUTS})


def alloc_transition(n, nq, nv, nu, dtype, device) -> TransitionResult:
    z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return TransitionResult(A=z(n, 2 * nv, 2 * nv), B=z(n, 2 * nv, nu), next_qpos=z(n, nq), next_qvel=z(n, nv),
                            warning=torch.zeros(n, dtype=torch.int32, device=device))


class TransitionMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and state)."""

    def fd_columns(self, centered: bool = False) -> int:
        """Virtual envs one env's linearisation takes: 1 + K, centred 1 + 2 K, K = 2 nv + nu."""
        k = 2 * int(self.model.nv) + int(self.model.nu)
        return 1 + (2 * k if centered else k)

    def _fd_workspace(self, slots: Optional[int], centered: bool):
        c = self.fd_columns(centered)
        if slots is None:
            one = int(lib().mgx_transition_fd_bytes(self.native.handle, c))
            check(min(one, 0), "mgx_transition_fd_bytes")
            slots = max(1, min(self.n, WORKSPACE_LIMIT // one)) * c
        slots = int(slots)
        cache = self.__dict__.setdefault("_fd_ws", {})
        key = (slots, bool(centered))
        if key not in cache:
            # below one env's columns no workspace size is defined: the library refuses the call
            nbytes = int(lib().mgx_transition_fd_bytes(self.native.handle, max(slots, 1)))
            check(min(nbytes, 0), "mgx_transition_fd_bytes")
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return slots, cache[key]

    def transition_fd(self, eps: Optional[float] = None, centered: bool = False, nsub: int = 1,
                      mask: Optional[torch.Tensor] = None, stream=None, slots: Optional[int] = None,
                      only: Optional[Sequence[str]] = None, out: Optional[TransitionResult] = None) -> TransitionResult:
        """``TransitionResult(A, B, next_qpos, next_qvel, warning)`` of every (masked) env:
        finite differences of ``nsub`` mj_steps from the current state, asynchronously on the
        stream. ``eps`` defaults to 1e-6 (fp64) / 2**-10 (fp32); ``centered`` averages the +eps and
        -eps steps at twice the cost. ``slots`` bounds the workspace (virtual envs held at once,
        at least ``fd_columns(centered)``; default: every env in one pass up to 1 GiB); the
        workspace is allocated once per (slots, centered). ``only`` names the outputs wanted; rows
        of envs that ``mask`` (uint8 [N]) deselects are left as they were."""
        n, m = self.n, self.model
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()
        want = list(FD_OUTPUTS) if only is None else list(only)
        for f in want:
            if f not in FD_OUTPUTS:
                raise KeyError(f"unknown transition output {f!r}; there are {list(FD_OUTPUTS)}")
        if out is None:
            if getattr(self, "_fd_out", None) is None:
                self._fd_out = alloc_transition(n, int(m.nq), int(m.nv), int(m.nu), self.dtype, self.device)
            out = self._fd_out
        slots, ws = self._fd_workspace(slots, centered)
        io = cabi.MgxFdIO()
        io.eps = default_eps(self.dtype) if eps is None else float(eps)
        io.flags = cabi.MGX_FD_CENTERED if centered else 0
        io.nsub = int(nsub)
        io.workspace, io.workspace_bytes, io.slots = ws.data_ptr(), ws.numel(), slots
        res = TransitionResult()
        for f in want:
            t = getattr(out, f)
            assert t is not None and t.is_contiguous() and t.shape[0] == n
            assert t.dtype == (torch.int32 if f == "warning" else self.dtype)
            setattr(io, f, t.data_ptr())
            setattr(res, f, t)
        check(lib().mgx_transition_fd(self.native.handle, C.byref(self._state), C.byref(io), n, _ptr(mask),
                                      _stream(stream)), "mgx_transition_fd")
        return res


    def transition_fd_along(self, state0: torch.Tensor, ctrl: torch.Tensor, warmstart: Optional[torch.Tensor] = None,
                            eps: Optional[float] = None, centered: bool = False, nsub: int = 1,
                            slots: Optional[int] = None) -> "TrajectoryTransitionResult":
        """``transition_fd`` at the T states of a trajectory per env: ``state0`` [N, T, nstate] (the
        state ENTERING each step, e.g. a rollout's initial state followed by its ``state[:, k, :-1]``),
        ``ctrl`` [N, T, nu] and ``warmstart`` [N, T, nv] (a closed-loop rollout's ``warmstart``; the
        solvers run a bounded number of iterations from it, so a linearisation of the step the
        rollout took must start from the one it had; default: the env's own at every t). Returns A
        [N, T, 2nv, 2nv], B [N, T, 2nv, nu], next_state [N, T, nstate] and warning int32 [N, T].

        The existing mgx_transition_fd runs over the N T stacked rows, held in a second batch that
        shares this one's compiled model, with each env's qfrc_applied and xfrc_applied repeated.
        Nothing is written to this batch's state. Tensors are owned by the batch and overwritten by
        the next call with the same T."""
        from .batch import PhysicsBatch
        n, m = self.n, self.model
        nq, nv, nu, ns = int(m.nq), int(m.nv), int(m.nu), 1 + int(m.nq) + int(m.nv)
        if state0.dim() != 3 or state0.shape[0] != n or state0.shape[2] != ns:
            raise ValueError(f"state0 must be [N, T, nstate], got {tuple(state0.shape)}")
        t = int(state0.shape[1])
        if tuple(ctrl.shape) != (n, t, nu):
            raise ValueError(f"ctrl must be [N, T, nu] = {[n, t, nu]}, got {tuple(ctrl.shape)}")
        if warmstart is not None and tuple(warmstart.shape) != (n, t, nv):
            raise ValueError(f"warmstart must be [N, T, nv] = {[n, t, nv]}, got {tuple(warmstart.shape)}")
        cache = self.__dict__.setdefault("_fd_along", {})
        if t not in cache:
            cache[t] = PhysicsBatch(m, n * t, precision="f64" if self.dtype == torch.float64 else "f32",
                                    device=str(self.device), native=self.native)
        tb = cache[t]
        x = state0.to(self.dtype).reshape(n * t, ns)
        tb.time.copy_(x[:, 0])
        tb.qpos.copy_(x[:, 1:1 + nq])
        tb.qvel.copy_(x[:, 1 + nq:])
        tb.ctrl[:, :nu] = ctrl.to(self.dtype).reshape(n * t, nu)
        tb.qacc_warmstart.copy_(self.qacc_warmstart.repeat_interleave(t, dim=0) if warmstart is None
                                else warmstart.to(self.dtype).reshape(n * t, nv))
        tb.qfrc_applied.copy_(self.qfrc_applied.repeat_interleave(t, dim=0))
        tb.xfrc_applied.copy_(self.xfrc_applied.repeat_interleave(t, dim=0))
        r = tb.transition_fd(eps=eps, centered=centered, nsub=nsub, slots=slots)
        # the step advances time by nsub timesteps, as mgx_step does it: one add in T per substep
        time = x[:, 0].clone()
        for _ in range(int(nsub)):
            time += torch.tensor(float(m.timestep), dtype=self.dtype, device=self.device)
        nxt = torch.cat([time[:, None], r.next_qpos, r.next_qvel], dim=1)
        return TrajectoryTransitionResult(A=r.A.view(n, t, 2 * nv, 2 * nv), B=r.B.view(n, t, 2 * nv, nu),
                                          next_state=nxt.view(n, t, ns), warning=r.warning.view(n, t))


class TrajectoryTransitionResult:
    """A [N, T, 2nv, 2nv], B [N, T, 2nv, nu], next_state [N, T, nstate] (the nominal state after each
    step) and warning int32 [N, T] of ``transition_fd_along``."""

    __slots__ = ("A", "B", "next_state", "warning")

    def __init__(self, A, B, next_state, warning):
        self.A, self.B, self.next_state, self.warning = A, B, next_state, warning


class TransitionForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``transition_fd`` under the env's name."""

    def transition_fd_along(self, state0, ctrl, **kw):
        """PhysicsBatch.transition_fd_along of this env's batch."""
        return self.batch.transition_fd_along(state0, ctrl, **kw)

    def transition_fd(self, **kw):
        """PhysicsBatch.transition_fd of this env's batch (derivatives of its physics step; pass
        ``nsub`` = the env's frame skip for one env step's physics)."""
        return self.batch.transition_fd(**kw)

    def fd_columns(self, centered: bool = False) -> int:
        return self.batch.fd_columns(centered)
