"""Batched extended Kalman filtering on top of the two linearisations the library ships:
``transition_fd`` (A) and ``sensor_fd`` (C), with the correction applied on the state manifold
(``state_integrate``).

``kalman_step`` is the covariance recursion in batched torch (CPU or device), ``kalman_step_fused``
the same recursion in ONE HIP kernel (``mgx_ekf_step``, include/mgx.h "Kalman covariance step") and
``Ekf`` the filter; ``EstimationMethods`` gives :class:`~.batch.PhysicsBatch` its ``ekf`` and
``EstimationForwarding`` the ``*VectorEnv`` classes theirs.

The state estimate is a state row ``[time, qpos, qvel]`` and its covariance P [2nv, 2nv] lives in the
tangent ``(dq, dqvel)`` of ``transition_fd``'s A: every model here has a free joint, so the
correction is ``state_integrate(x, dx)``, never ``qpos += dx``. One step is

    predict:  x <- step(x, ctrl);  P <- A P A' + diag(Q);  P <- (P + P') / 2
    update:   r = z - h(x);  G = P H';  S = H G + diag(R) = L L';  K = G S^-1;  dx = K r;
              x <- x (+) dx;  F = I - K H;  P <- F P F' + K diag(R) K' (Joseph);  P <- (P + P') / 2

with rows that are not measured (``row_mask`` 0) taken out by zeroing their row of H, residual and R
and giving S the identity's row and column there. The Joseph form is a sum of congruences and stays
positive semidefinite in fp32, which ``P - K S K'`` does not. ``nis = (r' S^-1 r, log det S)`` over
the measured rows is the innovation statistic (chi-square with as many degrees of freedom as
measured rows when the filter is consistent) and the Gaussian log-likelihood's determinant term.
Not provided: a full (non-diagonal) R, a square-root or UD form, smoothing, an iterated update, and
the calls on ``StreamSharded*Env``.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import torch

KalmanStep = namedtuple("KalmanStep", "P dx gain nis info")
EkfResult = namedtuple("EkfResult", "state P dx nis status")

PIVOT, WARNING = 1, 2  # ``status`` bits: a failed pivot of S (``info`` bit 0); a bad-state reset in the predict step


def _expand(x, shape, dt, dev):
    x = torch.as_tensor(x, device=dev).to(dt)
    if x.dim() == len(shape) - 1:
        x = x.expand(shape)
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"expected a tensor of shape {list(shape)} (or without the leading dim), got {list(x.shape)}")
    return x


def kalman_step(P, A=None, Q=None, Q_diag=None, H=None, R_diag=None, resid=None, row_mask=None) -> KalmanStep:
    """One covariance predict (``A`` given) and / or one Joseph measurement update (``H``, ``R_diag``
    and ``resid`` given) in batched torch over the leading dim N, on the tensors' own device; the
    documented fallback of ``kalman_step_fused`` and the recursion of include/mgx.h "Kalman
    covariance step".

    P [N, n, n]; A [N, n, n]; Q [N, n, n] and Q_diag [N, n] (either or both; default zero);
    H [N, p, n]; R_diag [N, p] (> 0); resid [N, p] = z - h(x); row_mask [N, p] (0 / False = the row
    is not measured). Returns ``KalmanStep(P, dx [N, n], gain [N, n, p], nis [N, 2], info int32 [N])``
    (dx, gain and nis are None without an update). ``info`` bit 0: S had a pivot that is not positive
    and finite; that env's update is skipped (P the predicted covariance, dx = 0, gain = 0,
    nis = NaN). With every row masked dx is exactly 0 and P its symmetric part."""
    N, n, _ = P.shape
    dt, dev = P.dtype, P.device
    info = torch.zeros(N, dtype=torch.int32, device=dev)
    if A is not None:
        P = A @ P @ A.transpose(1, 2)
        if Q is not None:
            P = P + Q
        if Q_diag is not None:
            P = P + torch.diag_embed(Q_diag)
        P = 0.5 * (P + P.transpose(1, 2))
    elif Q is not None or Q_diag is not None:
        raise ValueError("Q and Q_diag belong to the predict step: A is needed")
    if H is None:
        return KalmanStep(P, None, None, None, info)
    if R_diag is None or resid is None:
        raise ValueError("the update needs H, R_diag and resid")
    p = H.shape[1]
    on = torch.ones(N, p, dtype=torch.bool, device=dev) if row_mask is None else row_mask.to(dev) != 0
    zero = torch.zeros((), dtype=dt, device=dev)
    Hm = torch.where(on[:, :, None], H, zero)
    r = torch.where(on, resid, zero)
    Rm = torch.where(on, R_diag, zero)
    G = P @ Hm.transpose(1, 2)
    S = Hm @ G + torch.diag_embed(Rm + (~on).to(dt))
    L, bad = torch.linalg.cholesky_ex(S)
    bad = (bad != 0) | ~torch.isfinite(torch.diagonal(L, dim1=1, dim2=2)).all(1)
    L = torch.where(bad[:, None, None], torch.eye(p, dtype=dt, device=dev), L)
    K = torch.cholesky_solve(G.transpose(1, 2), L).transpose(1, 2)
    y = torch.linalg.solve_triangular(L, r[:, :, None], upper=False)[:, :, 0]
    nis = torch.stack([(y * y).sum(1), 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)], dim=1)
    dx = (K @ r[:, :, None])[:, :, 0]
    F = torch.eye(n, dtype=dt, device=dev) - K @ Hm
    Pn = F @ P @ F.transpose(1, 2) + (K * Rm[:, None, :]) @ K.transpose(1, 2)
    Pn = 0.5 * (Pn + Pn.transpose(1, 2))
    nan = torch.full((), float("nan"), dtype=dt, device=dev)
    return KalmanStep(torch.where(bad[:, None, None], P, Pn), torch.where(bad[:, None], zero, dx),
                      torch.where(bad[:, None, None], zero, K), torch.where(bad[:, None], nan, nis),
                      info | bad.to(torch.int32))


def kalman_step_fused(batch_or_native, P, A=None, Q=None, Q_diag=None, H=None, R_diag=None, resid=None, row_mask=None,
                      mask=None, stream=None, out: Optional[KalmanStep] = None) -> KalmanStep:
    """``kalman_step`` in one HIP kernel (``mgx_ekf_step``): the same arguments and the same result,
    on device tensors of the handle's precision. ``batch_or_native`` is a
    :class:`~.batch.PhysicsBatch` or its ``NativeModel``; it supplies the precision and the device
    only, so n and p need not be a model's (1 <= p <= 64). ``out`` is a ``KalmanStep`` of tensors to
    write into (default: new ones; ``gain`` may be None: not wanted); the kernel updates ``out.P`` in
    place, so ``P`` is first copied there unless ``out.P`` is ``P`` itself. ``mask`` uint8 [N]
    deselects envs: their rows of ``out``, P included, are left untouched. Without an update dx,
    gain and nis are not written.

    Asynchronous on ``stream`` (a ``torch.cuda.Stream``; default: the current one); temporaries are
    recorded on it. The workspace is allocated once per (n, p, N) and kept on the handle: calls of
    one handle and one (n, p, N) must not run concurrently on different streams."""
    import ctypes as C

    from . import cabi
    from .native import check, lib
    from .sensors import _ptr, _stream
    native = getattr(batch_or_native, "native", batch_or_native)
    dt = native.dtype
    N, n, _ = P.shape
    dev = P.device
    predict, update = A is not None, H is not None
    if not predict and (Q is not None or Q_diag is not None):
        raise ValueError("Q and Q_diag belong to the predict step: A is needed")
    if update and (R_diag is None or resid is None):
        raise ValueError("the update needs H, R_diag and resid")
    p = int(H.shape[1]) if update else 1

    def prep(x, shape, typ=dt):
        if x is None:
            return None
        x = torch.as_tensor(x, device=dev)
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"expected a tensor of shape {list(shape)}, got {list(x.shape)}")
        return x.to(typ).contiguous()

    ten = dict(A=prep(A, (N, n, n)), Q=prep(Q, (N, n, n)), Q_diag=prep(Q_diag, (N, n)), H=prep(H, (N, p, n)),
               R_diag=prep(R_diag, (N, p)), resid=prep(resid, (N, p)),
               row_mask=None if row_mask is None else prep(row_mask != 0, (N, p), torch.uint8))
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != N or mask.device != dev or not mask.is_contiguous()):
        raise ValueError(f"mask: a contiguous uint8 tensor of {N} entries on {dev} is needed")
    if out is None:
        z = lambda *s: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        out = KalmanStep(prep(P, (N, n, n)).clone(), z(N, n) if update else None, z(N, n, p) if update else None,
                         z(N, 2) if update else None, torch.zeros(N, dtype=torch.int32, device=dev))
    else:
        for x, shape, typ, need in ((out.P, (N, n, n), dt, True), (out.dx, (N, n), dt, update), (out.gain, (N, n, p), dt, False),
                                    (out.nis, (N, 2), dt, update), (out.info, (N,), torch.int32, True)):
            if x is None and not need:
                continue
            if x is None or tuple(x.shape) != shape or x.dtype != typ or not x.is_contiguous() or x.device != dev:
                raise ValueError(f"out: a contiguous {typ} tensor of shape {list(shape)} on {dev} is needed")
        if out.P.data_ptr() != P.data_ptr():
            src = prep(P, (N, n, n))
            out.P.copy_(src if mask is None else torch.where(mask.bool()[:, None, None], src, out.P))
    if stream is not None:
        for x in ten.values():
            if x is not None:
                x.record_stream(stream)
    cache = native.__dict__.setdefault("_ekf_ws", {})
    key = (n, p, N, str(dev))
    if key not in cache:
        nbytes = int(lib().mgx_ekf_bytes(native.handle, n, p, N))
        check(min(nbytes, 0), "mgx_ekf_bytes")
        cache[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ws = cache[key]
    io = cabi.MgxEkfIO()
    io.n, io.p = n, p
    io.flags = (cabi.MGX_EKF_PREDICT if predict else 0) | (cabi.MGX_EKF_UPDATE if update else 0)
    for f, x in ten.items():
        setattr(io, f, None if x is None else x.data_ptr())
    io.P, io.info = out.P.data_ptr(), out.info.data_ptr()
    for f in ("dx", "gain", "nis"):
        x = getattr(out, f)
        setattr(io, f, None if x is None or not update else x.data_ptr())
    io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
    check(lib().mgx_ekf_step(native.handle, C.byref(io), N, _ptr(mask), _stream(stream)), "mgx_ekf_step")
    return out


class Ekf:
    """An extended Kalman filter per env: ``predict(ctrl)``, ``update(z)`` or ``step(ctrl, z)`` once
    per control step; each returns ``EkfResult(state [N, nstate], P [N, 2nv, 2nv], dx [N, 2nv],
    nis [N, 2], status int32 [N])``. ``P`` is the filter's own tensor, updated in place by the next
    call; ``status`` holds bits: 1 (``PIVOT``) S had a non-positive pivot and the update was skipped,
    2 (``WARNING``) the predict step met a bad-state reset (``transition_fd``'s ``warning``): that
    env's belief and covariance are left as they were.

    ``system`` is a :class:`~.batch.PhysicsBatch`, or any object with the duck-typed calls the filter
    uses, so a linear stand-in can drive it on the CPU: ``model`` (``nq``, ``nv``, ``nu``,
    ``timestep``; ``sensor_type`` optional), ``n``, ``state_size``, ``ctrl`` [N, >= nu],
    ``get_state()``, ``set_state(x, mask=)``, ``state_integrate(x, dx)``, ``sensor_slices``,
    ``transition_fd(only=, nsub=, centered=)`` -> (A, next_qpos, next_qvel, warning) and
    ``sensor_fd(only=, centered=)`` -> (C, sensordata). On a real batch (one with a ``native``
    handle) the filter owns a second, "belief" ``PhysicsBatch`` that shares the compiled model and
    starts with the batch's warm start and applied forces: the user's batch is never written. A
    stand-in is used as the belief itself. The belief's ``qacc_warmstart`` is not advanced by
    ``predict`` (``transition_fd`` does not return it).

    x0 [N, nstate] is the first estimate, P0 [2nv, 2nv] or [N, 2nv, 2nv] its covariance, Q_diag
    [2nv] or [N, 2nv] the process noise added per ``predict``, R_diag [p] or [N, p] the measurement
    noise of the selected rows. ``sensors`` names the sensors measured (keys of ``sensor_slices``;
    default: every row); z and row_mask are given either as whole ``sensordata()`` rows
    [N, nsensordata] or as the selected rows [N, p]. A ``framequat`` measurement is first flipped
    into the hemisphere of the predicted quaternion (q and -q are one rotation, and the residual is a
    plain component difference). ``backend="fused"`` runs the covariance part in ``mgx_ekf_step``
    (``step``: predict and update in ONE call); ``"torch"`` in ``kalman_step``."""

    def __init__(self, system, x0, P0, Q_diag, R_diag, sensors: Optional[Sequence[str]] = None, nsub: int = 1,
                 backend: str = "torch", centered: bool = False):
        if backend not in ("torch", "fused"):
            raise ValueError(f"backend must be 'torch' or 'fused', got {backend!r}")
        native = getattr(system, "native", None)
        if backend == "fused" and native is None:
            raise ValueError("backend='fused' needs a system with a native handle (a PhysicsBatch)")
        if native is not None:
            from .batch import PhysicsBatch
            b = PhysicsBatch(system.model, system.n, precision="f64" if system.dtype == torch.float64 else "f32",
                             device=str(system.device), native=native)
            for f in ("qacc_warmstart", "qfrc_applied", "xfrc_applied", "ctrl"):
                getattr(b, f).copy_(getattr(system, f))
        else:
            b = system
        self.belief, self.native, self.backend, self.nsub, self.centered = b, native, backend, int(nsub), bool(centered)
        m = b.model
        self.N, self.n = int(b.n), 2 * int(m.nv)
        x0 = torch.as_tensor(x0)
        dt, dev = (b.dtype, b.device) if native is not None else (x0.dtype, x0.device)
        self.dtype, self.device = dt, dev
        b.set_state(x0.to(device=dev, dtype=dt))
        slices = b.sensor_slices
        names = list(slices) if sensors is None else list(sensors)
        rows, quats = [], []
        quat_type = None
        if getattr(m, "sensor_type", None) is not None:
            from . import mjcf
            quat_type = mjcf.SENSOR_TYPES.index("framequat")
            types = dict(zip(m.sensor_names, m.sensor_type))
        for name in names:
            if name not in slices:
                raise KeyError(f"unknown sensor {name!r}; the model has {list(slices)}")
            sl = slices[name]
            if quat_type is not None and int(types[name]) == quat_type:
                quats.append(list(range(len(rows), len(rows) + 4)))
            rows.extend(range(sl.start, sl.stop))
        self.nsensordata = max([s.stop for s in slices.values()], default=0)
        self.rows = torch.tensor(rows, dtype=torch.long, device=dev)
        self.quats = [torch.tensor(q, dtype=torch.long, device=dev) for q in quats]
        self.p = len(rows)
        if self.p < 1:
            raise ValueError("the filter needs at least one measurement row")
        self.P = _expand(P0, (self.N, self.n, self.n), dt, dev).clone().contiguous()
        self.Q_diag = _expand(Q_diag, (self.N, self.n), dt, dev).contiguous()
        self.R_diag = _expand(R_diag, (self.N, self.p), dt, dev).contiguous()
        z = lambda *s: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        self._out = KalmanStep(self.P, z(self.N, self.n), None, z(self.N, 2), torch.zeros(self.N, dtype=torch.int32, device=dev))

    # ------------------------------------------------------------------ the three parts of a step
    def _move(self, ctrl):
        """The belief through ``nsub`` steps under ``ctrl``; returns (A, ok bool [N])."""
        b, m = self.belief, self.belief.model
        nu = int(m.nu)
        b.ctrl[:, :nu] = torch.as_tensor(ctrl, device=self.device).to(self.dtype)
        r = b.transition_fd(only=("A", "next_qpos", "next_qvel", "warning"), nsub=self.nsub, centered=self.centered)
        ok = r.warning == 0
        # the step advances time by nsub timesteps, as the step itself does it: one add per substep
        time = b.get_state()[:, 0].clone()
        for _ in range(self.nsub):
            time += torch.tensor(float(m.timestep), dtype=self.dtype, device=self.device)
        b.set_state(torch.cat([time[:, None], r.next_qpos, r.next_qvel], dim=1), mask=ok)
        return r.A, ok

    def _select(self, x, name):
        x = torch.as_tensor(x, device=self.device)
        if x.dim() == 2 and x.shape[0] == self.N and x.shape[1] == self.nsensordata:
            return x[:, self.rows]
        if tuple(x.shape) != (self.N, self.p):
            raise ValueError(f"{name} must be [N, nsensordata] = {[self.N, self.nsensordata]} or [N, p] = "
                             f"{[self.N, self.p]}, got {list(x.shape)}")
        return x

    def _measure(self, z):
        """(H [N, p, 2nv], resid [N, p]) at the belief."""
        r = self.belief.sensor_fd(only=("C", "sensordata"), centered=self.centered)
        h = r.sensordata[:, self.rows]
        z = self._select(z, "z").to(self.dtype).clone()
        for q in self.quats:  # q and -q are one rotation: compare in the predicted quaternion's hemisphere
            flip = (z[:, q] * h[:, q]).sum(1, keepdim=True) < 0
            z[:, q] = torch.where(flip, -z[:, q], z[:, q])
        return r.C[:, self.rows, :].contiguous(), z - h

    def _covariance(self, A=None, H=None, resid=None, row_mask=None, ok=None):
        """One kalman_step on self.P in place; envs that ``ok`` deselects keep P and get dx = 0."""
        upd = H is not None
        kw = dict(A=A, Q_diag=self.Q_diag if A is not None else None, H=H, R_diag=self.R_diag if upd else None,
                  resid=resid, row_mask=None if row_mask is None or not upd else self._select(row_mask, "row_mask"))
        o = self._out
        o.info.zero_()
        if upd:
            o.dx.zero_()
            o.nis.zero_()
        if self.backend == "fused":
            kalman_step_fused(self.native, self.P, mask=None if ok is None else ok.to(torch.uint8), out=o, **kw)
        else:
            r = kalman_step(self.P, **kw)
            sel = torch.ones(self.N, dtype=torch.bool, device=self.device) if ok is None else ok
            self.P.copy_(torch.where(sel[:, None, None], r.P, self.P))
            o.info.copy_(torch.where(sel, r.info, o.info))
            if upd:
                o.dx.copy_(torch.where(sel[:, None], r.dx, o.dx))
                o.nis.copy_(torch.where(sel[:, None], r.nis, o.nis))
        return o

    def _result(self, o, ok, updated):
        b = self.belief
        if updated:
            b.set_state(b.state_integrate(b.get_state(), o.dx))
        status = o.info.clone()
        if ok is not None:
            status = status | torch.where(ok, 0, WARNING).to(torch.int32)
        return EkfResult(b.get_state(), self.P, o.dx if updated else None, o.nis if updated else None, status)

    # ------------------------------------------------------------------ API
    def predict(self, ctrl) -> EkfResult:
        """The belief through one control step (``nsub`` physics steps) under ``ctrl`` [N, nu] and
        ``P <- A P A' + diag(Q_diag)`` with the A of that very step."""
        A, ok = self._move(ctrl)
        return self._result(self._covariance(A=A, ok=ok), ok, False)

    def update(self, z, row_mask=None) -> EkfResult:
        """The measurement update at the belief with ``z`` (see the class for its two shapes)."""
        H, resid = self._measure(z)
        return self._result(self._covariance(H=H, resid=resid, row_mask=row_mask), None, True)

    def step(self, ctrl, z, row_mask=None) -> EkfResult:
        """``predict(ctrl)`` then ``update(z)``, the covariance part as one ``kalman_step`` (one
        kernel with ``backend="fused"``). An env whose predict step met a bad-state reset is left as
        it was altogether (status bit 2)."""
        A, ok = self._move(ctrl)
        H, resid = self._measure(z)
        return self._result(self._covariance(A=A, H=H, resid=resid, row_mask=row_mask, ok=ok), ok, True)

    @property
    def state(self) -> torch.Tensor:
        return self.belief.get_state()


class EstimationMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and get_state)."""

    def ekf(self, P0, Q_diag, R_diag, x0: Optional[torch.Tensor] = None, **kw) -> Ekf:
        """An :class:`~.estimation.Ekf` for this batch's model, starting at ``x0`` [N, nstate]
        (default: the batch's current state) with covariance ``P0``; ``sensors``, ``nsub``,
        ``backend`` and ``centered`` as in ``Ekf``. The filter keeps its own belief batch: this one
        is never written."""
        return Ekf(self, self.get_state() if x0 is None else x0, P0, Q_diag, R_diag, **kw)


class EstimationForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ``ekf`` (raw actuator ctrl, as
    ``physics_rollout``; pass ``nsub`` = the env's frame skip)."""

    def ekf(self, P0, Q_diag, R_diag, **kw) -> Ekf:
        return self.batch.ekf(P0, Q_diag, R_diag, **kw)
