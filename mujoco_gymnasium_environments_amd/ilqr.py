"""Batched iLQR on top of the closed-loop rollouts (``rollout_feedback``), the trajectory
linearisation (``transition_fd_along``) and the state manifold (``state_difference``).

``lqr_backward`` is the Riccati recursion and ``solve`` the driver; ``IlqrMethods`` gives
:class:`~.batch.PhysicsBatch` its ``solve_ilqr`` and ``IlqrForwarding`` the ``*VectorEnv`` classes
theirs.

The default backward pass is batched torch: per iteration it is T small dense solves per env
(nu x nu Cholesky factors and a handful of 2nv x 2nv products), beside the (1 + 2nv + nu) T physics
steps per env of the finite-difference linearisation and the K T steps of the line search, which
run in the library's HIP kernels. It runs on CPU tensors as well, so a CPU stand-in for the system
can drive the solver in the tests. ``lqr_backward_fused`` is the same recursion in ONE HIP kernel
(``mgx_lqr_backward``, include/mgx.h "LQR backward pass"): ``solve(backward="fused")``.

Control limits: ``solve(box=True)`` plans with the model's own control range (box-DDP: Tassa, Mansard
and Todorov 2014). The bounds on the step are ``lo_t = ctrl_lo - u_t`` and ``hi_t = ctrl_hi - u_t``
around the applied nominal; the feed-forward step solves the box QP ``min 1/2 k' Q_uu k + Q_u' k``
inside them by projected Newton and the gains of the controls it clamps are zero, so ``expected`` is
the decrease of a step the rollout can take. Without ``box`` the limits act through the clamp of
``rollout_feedback`` alone.

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
Not provided: any other cost, costs on acceleration-stage sensors, state constraints, any box other
than the model's own control range, and the calls on ``StreamSharded*Env``.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import torch

DEFAULT_ALPHAS = (1, .5, .25, .125, .0625, .03125, .015625, .0078125)
MU_MIN, MU_MAX = 1e-6, 1e10  # the first nonzero Levenberg parameter, and the cap that ends an env with status 2

CONVERGED, MAX_ITER, STALLED = 0, 1, 2

LqrBackward = namedtuple("LqrBackward", "k_ff gain expected info free", defaults=(None,))
IlqrResult = namedtuple("IlqrResult", "ctrl state gain k_ff cost cost_history iters status free", defaults=(None,))

QP_ITERS, LS_STEPS, ARMIJO, LS_SHRINK = 100, 60, 0.1, 0.6  # the box QP (include/mgx.h "LQR backward pass")
PIVOT, QP_CAP = 1, 2  # ``info`` of the box pass and of the fused pass: bit 0 (value 1) and bit 1 (value 2)


def lqr_backward(A, B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu, lo=None, hi=None):
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
    had a non-positive pivot (``torch.linalg.cholesky_ex``): that env's gains are meaningless.

    With ``lo`` / ``hi`` [N, T, m] (either may be None: no bound on that side; +-inf entries: none
    for that control) the step is box-constrained, ``lo_t <= k_t <= hi_t``: ``k_t`` solves the box QP
    of the regularised Q_uu by projected Newton from the clamped ``k`` of step t + 1, the gains are
    ``-(Q_uu)_ff^-1 (Q_ux)_f`` on the free controls and zero on the clamped ones, and the result also
    carries ``free`` bool [N, T, m]. ``info`` then holds bits: bit 0 (``PIVOT``, value 1) a non-positive
    pivot, bit 1 (``QP_CAP``, value 2) a QP that hit its iteration cap. The QPs run env by env: this is the CPU and reference path
    (``lqr_backward_fused`` is the kernel)."""
    if lo is not None or hi is not None:
        return _lqr_backward_box(A, B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu, lo, hi)
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


def box_qp(H, q, lo, hi, x0):
    """argmin 1/2 x' H x + q' x over lo <= x <= hi for ONE problem (H [m, m] symmetric positive
    definite, the rest [m]) by the projected Newton method of include/mgx.h "LQR backward pass",
    from clamp(x0). Returns (x, free bool [m], bits, idx, L): ``idx`` the free controls and ``L`` the
    Cholesky factor of H[idx][:, idx] (None when no control is free or the pivot failed)."""
    zero = torch.zeros_like(q)
    clamp = lambda v: torch.minimum(torch.maximum(v, lo), hi)  # noqa: E731
    x = clamp(x0)
    have, idx, L, full, done, bits = None, None, None, False, False, 0
    free = torch.ones_like(q, dtype=torch.bool)
    for _ in range(QP_ITERS):
        g = q + H @ x
        cl = ((x == lo) & (g > 0)) | ((x == hi) & (g < 0))
        free = ~cl
        if not bool(free.any()):
            idx, L, done = None, None, True
            break
        if have is None or not torch.equal(free, have):
            idx = free.nonzero()[:, 0]
            L, bad = torch.linalg.cholesky_ex(H[idx][:, idx])
            if int(bad) != 0:
                return x, free, PIVOT, None, None
            have = free
        elif full:  # a full Newton step inside the box kept the set
            done = True
            break
        gc = q + H @ torch.where(cl, x, zero)
        y = x.clone()
        y[idx] = -torch.cholesky_solve(gc[idx, None], L)[:, 0]
        d = torch.where(free, y - x, zero)
        sdotg = (d * g).sum()
        if not bool(sdotg < 0):
            done = True
            break
        step, ok = 1.0, False
        for _ls in range(LS_STEPS):
            xn = y if step == 1.0 else x + step * d
            xc = clamp(xn)
            dx = xc - x
            gdx = (dx * g).sum()  # the first-order decrease along the projected step
            if bool(gdx < 0) and bool(gdx + 0.5 * (dx * (H @ dx)).sum() <= ARMIJO * gdx):
                ok = True
                break
            step *= LS_SHRINK
        if not ok:
            break
        full = step == 1.0 and bool((xc == xn).all())
        x = xc
    if not done:
        bits |= QP_CAP
    return x, free, bits, idx, L


def _lqr_backward_box(A, B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu, lo, hi):
    """``lqr_backward`` with bounds on the step (its docstring): the same recursion, the Cholesky
    solve replaced by one box QP per env and step."""
    N, T, n, m = B.shape
    dt, dev = A.dtype, A.device
    mu = torch.as_tensor(mu, dtype=dt, device=dev).expand(N)
    big = torch.full((N, T, m), float("inf"), dtype=dt, device=dev)
    lo = -big if lo is None else lo.to(dt)
    hi = big if hi is None else hi.to(dt)
    eye = torch.eye(m, dtype=dt, device=dev)
    Vx, Vxx = Vx_T, Vxx_T
    k_ff = torch.zeros(N, T, m, dtype=dt, device=dev)
    gain = torch.zeros(N, T, m, n, dtype=dt, device=dev)
    free = torch.ones(N, T, m, dtype=torch.bool, device=dev)
    expected = torch.zeros(N, 2, dtype=dt, device=dev)
    info = torch.zeros(N, dtype=torch.int32, device=dev)
    k_next = torch.zeros(N, m, dtype=dt, device=dev)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], B[:, t]
        AtT, BtT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qu = lu[:, t] + (BtT @ Vx[:, :, None])[:, :, 0]
        Qux = lux[:, t] + BtT @ Vxx @ At
        Quu = luu[:, t] + BtT @ Vxx @ Bt
        scale = torch.clamp(torch.diagonal(Quu, dim1=1, dim2=2).mean(1), min=1.0)
        H = Quu + (mu * scale)[:, None, None] * eye
        H = torch.tril(H) + torch.tril(H, -1).transpose(1, 2)  # the lower triangle, as a Cholesky factorisation reads it
        k = torch.zeros(N, m, dtype=dt, device=dev)
        K = torch.zeros(N, m, n, dtype=dt, device=dev)
        for e in range(N):
            if int(info[e]) & PIVOT:  # the pass of this env has ended: its outputs are meaningless
                k[e], K[e] = float("nan"), float("nan")
                continue
            x, fr, bits, idx, L = box_qp(H[e], Qu[e], lo[e, t], hi[e, t], k_next[e])
            info[e] |= bits
            k[e], free[e, t] = x, fr
            if bits & PIVOT:
                k[e], K[e] = float("nan"), float("nan")
            elif idx is not None:
                K[e, idx] = -torch.cholesky_solve(Qux[e, idx], L)
        k_next = k
        KT = K.transpose(1, 2)
        expected[:, 0] += (k * Qu).sum(1)
        expected[:, 1] += 0.5 * (k * (Quu @ k[:, :, None])[:, :, 0]).sum(1)
        Acl = At + Bt @ K
        AclT = Acl.transpose(1, 2)
        luxT = lux[:, t].transpose(1, 2)
        Bk = (Bt @ k[:, :, None])[:, :, 0]
        Vx = (lx[:, t] + (KT @ (lu[:, t] + (luu[:, t] @ k[:, :, None])[:, :, 0])[:, :, None])[:, :, 0]
              + (luxT @ k[:, :, None])[:, :, 0] + (AclT @ (Vx + (Vxx @ Bk[:, :, None])[:, :, 0])[:, :, None])[:, :, 0])
        Vxx = lxx[:, t] + KT @ luu[:, t] @ K + KT @ lux[:, t] + luxT @ K + AclT @ Vxx @ Acl
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        k_ff[:, t], gain[:, t] = k, K
    return LqrBackward(k_ff, gain, expected, info, free)


def lqr_backward_fused(batch_or_native, A, B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu, lo=None, hi=None,
                       lxx_diag=None, luu_diag=None, mask=None, stream=None, out=None):
    """``lqr_backward`` in one HIP kernel (``mgx_lqr_backward``, include/mgx.h "LQR backward pass"):
    the same arguments and the same result, on device tensors of the handle's precision.
    ``batch_or_native`` is a :class:`~.batch.PhysicsBatch` or its ``NativeModel``; it supplies the
    precision and the device only, so n and m need not be a model's. ``lxx``, ``luu`` and ``lux``
    may be None (zero); ``lxx_diag`` [N, T, n] and ``luu_diag`` [N, T, m] are added to the diagonals,
    so a diagonal cost needs no [N, T, n, n] tensor. ``info`` holds bits: bit 0 (value 1) a non-positive
    pivot, bit 1 (value 2) a QP that hit its iteration cap; ``free`` (uint8 0 / 1 here) is all ones
    without bounds. ``mask`` uint8 [N] deselects envs: their rows of ``out`` (an ``LqrBackward`` of
    tensors to write into; default: new zeros) are left untouched.

    Asynchronous on ``stream`` (a ``torch.cuda.Stream``; default: the current one). Inputs that had to
    be converted or made contiguous are temporaries: they are recorded on the stream
    (``Tensor.record_stream``), so their memory is not reused before the kernel has read them; the
    caller orders its own tensors against the stream as for any torch work on a side stream. The
    workspace is allocated once per (n, m, N) and kept on the handle, and every call with those sizes
    uses it: calls of one handle and one (n, m, N) must not run concurrently on different streams."""
    import ctypes as C

    from . import cabi
    from .native import check, lib
    from .sensors import _ptr, _stream
    native = getattr(batch_or_native, "native", batch_or_native)
    dt = native.dtype
    N, T, n, m = B.shape
    dev = B.device
    prep = lambda x, shape: None if x is None else _dense(x, shape, dt, dev)  # noqa: E731
    box = lo is not None or hi is not None
    if box:
        big = torch.full((N, T, m), float("inf"), dtype=dt, device=dev)
        lo, hi = (-big if lo is None else lo), (big if hi is None else hi)
    ten = dict(A=prep(A, (N, T, n, n)), B=prep(B, (N, T, n, m)), lx=prep(lx, (N, T, n)), lxx=prep(lxx, (N, T, n, n)),
               lu=prep(lu, (N, T, m)), luu=prep(luu, (N, T, m, m)), lux=prep(lux, (N, T, m, n)),
               lxx_diag=prep(lxx_diag, (N, T, n)), luu_diag=prep(luu_diag, (N, T, m)), Vx_T=prep(Vx_T, (N, n)),
               Vxx_T=prep(Vxx_T, (N, n, n)), lo=prep(lo, (N, T, m)), hi=prep(hi, (N, T, m)),
               mu=torch.as_tensor(mu, dtype=dt, device=dev).expand(N).contiguous())
    if out is None:
        out = LqrBackward(torch.zeros(N, T, m, dtype=dt, device=dev), torch.zeros(N, T, m, n, dtype=dt, device=dev),
                          torch.zeros(N, 2, dtype=dt, device=dev), torch.zeros(N, dtype=torch.int32, device=dev),
                          torch.ones(N, T, m, dtype=torch.uint8, device=dev))
    for x, shape, typ in ((out.k_ff, (N, T, m), dt), (out.gain, (N, T, m, n), dt), (out.expected, (N, 2), dt),
                          (out.info, (N,), torch.int32), (out.free, (N, T, m), torch.uint8)):
        if x is not None and (tuple(x.shape) != shape or x.dtype != typ or not x.is_contiguous() or x.device != dev):
            raise ValueError(f"out: a contiguous {typ} tensor of shape {list(shape)} on {dev} is needed")
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != N or mask.device != dev or not mask.is_contiguous()):
        raise ValueError(f"mask: a contiguous uint8 tensor of {N} entries on {dev} is needed")
    if stream is not None:
        for x in ten.values():
            if x is not None:
                x.record_stream(stream)
    cache = native.__dict__.setdefault("_lqr_ws", {})
    key = (n, m, N, str(dev))
    if key not in cache:
        nbytes = int(lib().mgx_lqr_backward_bytes(native.handle, n, m, N))
        check(min(nbytes, 0), "mgx_lqr_backward_bytes")
        cache[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ws = cache[key]
    io = cabi.MgxLqrIO()
    io.n, io.m, io.T, io.flags = n, m, T, cabi.MGX_LQR_BOX if box else 0
    for f, x in ten.items():
        setattr(io, f, None if x is None else x.data_ptr())
    io.k_ff, io.gain, io.expected, io.info = (x.data_ptr() for x in (out.k_ff, out.gain, out.expected, out.info))
    io.free_set = None if out.free is None else out.free.data_ptr()
    io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
    check(lib().mgx_lqr_backward(native.handle, C.byref(io), N, _ptr(mask), _stream(stream)), "mgx_lqr_backward")
    return out


def _dense(x, shape, dt, dev):
    x = torch.as_tensor(x, device=dev)
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"expected a tensor of shape {list(shape)}, got {list(x.shape)}")
    return x.to(dt).contiguous()


def control_range(model, nu, dtype, device):
    """(lo, hi) [nu] of the model's control range, -inf / +inf where an actuator is not limited; a
    model without ``actuator_ctrllimited`` has no limits (as sampling.py reads them)."""
    lo = torch.full((nu,), float("-inf"), dtype=dtype, device=device)
    hi = torch.full((nu,), float("inf"), dtype=dtype, device=device)
    limited = getattr(model, "actuator_ctrllimited", None)
    if limited is not None and nu > 0:
        lim = torch.as_tensor(limited).to(device).reshape(-1) != 0
        rng = torch.as_tensor(model.actuator_ctrlrange).to(device=device, dtype=dtype).reshape(-1, 2)
        lo, hi = torch.where(lim, rng[:, 0], lo), torch.where(lim, rng[:, 1], hi)
    return lo, hi


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
          mu_factor: float = 10.0, max_iter: int = 20, tol: float = 1e-6, centered: bool = False, box: bool = False,
          backward: str = "torch") -> IlqrResult:
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
    iters [N], status [N], free [N, T, nu])``: ``state`` is what ``ctrl`` produces from ``x0`` (the
    applied, clamped control), ``gain``, ``k_ff`` and ``free`` belong to the last accepted step. Nothing
    is written to the system's state.

    ``box=True`` plans inside the model's control range (module docstring): the backward pass gets
    ``lo_t = ctrl_lo - u_t``, ``hi_t = ctrl_hi - u_t`` from ``model.actuator_ctrlrange`` where
    ``actuator_ctrllimited`` (a model without them has no limits), ``u_t`` the applied nominal, and
    ``free`` bool is False where the step's QP clamped a control (all True without ``box``).
    ``backward="fused"`` runs the backward pass in ``lqr_backward_fused`` (the system must have a
    ``native`` handle: ValueError otherwise); the cost's diagonal terms then go in as diagonals.
    With the defaults neither changes anything.

    A problem with a sensor cost (module docstring) also needs ``sensor_fd_along``, the
    ``sensordata`` output of ``rollout_feedback`` and the model's sensor tables; without one none
    of them is touched and the result is bit for bit that of the plain solve."""
    if backward not in ("torch", "fused"):
        raise ValueError(f"backward must be 'torch' or 'fused', got {backward!r}")
    fused = backward == "fused"
    if fused and getattr(system, "native", None) is None:
        raise ValueError("backward='fused' needs a system with the library's handle (a PhysicsBatch)")
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
    free = torch.ones(N, T, nu, dtype=torch.bool, device=dev)
    c_lo, c_hi = control_range(system.model, nu, dt, dev) if box else (None, None)
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
        lim = dict(lo=c_lo - ctrl, hi=c_hi - ctrl) if box else {}  # bounds on the step around the applied nominal
        while True:
            if fused:
                # the diagonal terms as diagonals; a sensor cost makes lxx dense and it goes in as it is
                bw = lqr_backward_fused(system, lin.A, lin.B, lx, lxx if sw else None, lu, None, None, Vx_T, Vxx_T, mu,
                                        lxx_diag=None if sw else w[0][:, None, :].expand(N, T, 2 * nv),
                                        luu_diag=w[2][:, None, :].expand(N, T, nu), **lim)
            elif box:
                bw = lqr_backward(lin.A, lin.B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu, **lim)
            else:
                bw = lqr_backward(lin.A, lin.B, lx, lxx, lu, luu, lux, Vx_T, Vxx_T, mu)
            # a QP that stopped at its iteration cap (bit 1 of ``info`` of the box and the fused pass) still returns a feasible step
            failed = (bw.info & PIVOT) != 0 if (fused or box) else bw.info != 0
            bad = active & (failed | ~torch.isfinite(bw.k_ff).all(-1).all(-1))
            if not bool(bad.any()):
                break
            raise_mu(bad)
            fresh = fresh & ~bad
        # an env that has ended takes the zero step: its trajectory is rolled again and discarded
        new_k = torch.where(active[:, None, None], bw.k_ff, torch.zeros_like(bw.k_ff)).contiguous()
        new_g = torch.where(active[:, None, None, None], bw.gain, torch.zeros_like(bw.gain)).contiguous()
        predicted = -(bw.expected[:, 0] + bw.expected[:, 1])
        done = active & fresh & torch.isfinite(cost) & (predicted <= tol * cost.abs())
        if fused or box:
            done = done & ((bw.info & QP_CAP) == 0)  # a QP that did not finish says nothing about convergence
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
        if box:
            free = sel(accept, bw.free != 0, free)
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
    return IlqrResult(ctrl, state, gain, k_ff, cost, torch.stack(history), iters, status, free)


class IlqrMethods:
    """Mixin of PhysicsBatch (uses rollout_feedback, transition_fd_along, state_difference, get_state)."""

    def solve_ilqr(self, goal_state: torch.Tensor, horizon: int, w_x, w_xf, w_u, u_init: Optional[torch.Tensor] = None,
                   nsub: int = 1, alphas: Sequence[float] = DEFAULT_ALPHAS, mu0: float = 1e-6, mu_factor: float = 10.0,
                   max_iter: int = 20, tol: float = 1e-6, centered: bool = False, sensor_goal=None, w_s=None,
                   w_sf=None, box: bool = False, backward: str = "torch") -> IlqrResult:
        """``ilqr.solve`` from every env's current state towards ``goal_state`` [N, nstate] or
        [N, T + 1, nstate] over ``horizon`` = T recorded steps of ``nsub`` mj_steps, with the
        diagonal quadratic cost of :mod:`~.ilqr` (weights [n] or [N, n]; the Gauss-Newton gradient
        takes d(dx)/dx = I) and, with ``sensor_goal`` [N, ns] or [N, T, ns] and the weights ``w_s``,
        ``w_sf`` ([ns] or [N, ns]), its sensor residual (``sensor_slices`` maps names to rows;
        accelerometer, force, torque and touch rows may not be weighted). ``box=True`` plans inside
        the model's control range (box-DDP) and ``backward="fused"`` runs the backward pass in the
        ``mgx_lqr_backward`` kernel. See ``ilqr.solve`` for the iteration and the result. The
        batch's state is not written."""
        problem = IlqrProblem(self.get_state(), goal_state.to(self.dtype), horizon, w_x, w_xf, w_u, u_init,
                              sensor_goal=sensor_goal, w_s=w_s, w_sf=w_sf)
        return solve(self, problem, nsub=nsub, alphas=alphas, mu0=mu0, mu_factor=mu_factor, max_iter=max_iter, tol=tol,
                     centered=centered, box=box, backward=backward)


class IlqrForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``solve_ilqr`` (raw actuator ctrl, as
    ``physics_rollout``; pass ``nsub`` = the env's frame skip)."""

    def solve_ilqr(self, goal_state, horizon, w_x, w_xf, w_u, **kw):
        return self.batch.solve_ilqr(goal_state, horizon, w_x, w_xf, w_u, **kw)
