"""numpy float64 restatement of mgx_rollout_cost's cost and of the MPPI update, written against the
text of include/mgx.h ("rollout costs") and of sampling.py's module docstring, not the HIP code.

The cost of one rollout, from its tangent differences dx_0 .. dx_T, its controls u_0 .. u_(T-1) and
its sensor residuals r_1 .. r_T:

    J = 1/2 w_x.dx_0^2 + sum_{t=1..T-1} 1/2 w_x.dx_t^2 + 1/2 w_xf.dx_T^2
      + sum_{t=0..T-1} 1/2 w_u.u_t^2
      + sum_{t=1..T-1} 1/2 w_s.r_t^2 + 1/2 w_sf.r_T^2

Every term p = (0.5 w) (d d) is formed in float64 exactly as the header states it (two roundings);
the terms are then summed EXACTLY (math.fsum), so the only difference a correct implementation may
show is its own summation error.
"""
import math

import numpy as np


def _terms(w, d):
    """p[i] = (0.5 w[i]) (d[i] d[i]) in float64, flat."""
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), np.shape(d))
    d = np.asarray(d, dtype=np.float64)
    return ((0.5 * w) * (d * d)).reshape(-1)


def rollout_cost(dx=None, u=None, r=None, w_x=None, w_xf=None, w_u=None, w_s=None, w_sf=None):
    """(J, parts [3], sum |p|, count) of one rollout: dx [T + 1, 2nv], u [T, nu], r [T, ns] (row
    t - 1 belongs to x_t); a None operand or weight drops its terms. ``parts`` are the state, control
    and sensor sums, each exact; ``count`` the number of terms p."""
    groups = [[], [], []]
    if dx is not None:
        if w_x is not None:
            groups[0].append(_terms(w_x, dx[:-1]))
        if w_xf is not None:
            groups[0].append(_terms(w_xf, dx[-1]))
    if u is not None and w_u is not None:
        groups[1].append(_terms(w_u, u))
    if r is not None:
        if w_s is not None:
            groups[2].append(_terms(w_s, r[:-1]))
        if w_sf is not None:
            groups[2].append(_terms(w_sf, r[-1]))
    flat = [np.concatenate(g) if g else np.zeros(0) for g in groups]
    every = np.concatenate(flat)
    return (math.fsum(every), np.array([math.fsum(f) for f in flat]), math.fsum(np.abs(every)), int(every.size))


def mppi_update(cost, knots, lam):
    """(new nominal [J, nu] or None, w [K], best) of one env: cost [K] (+inf: diverged), knots
    [K, J, nu]. w_k = exp(-(c_k - c_min) / lam) normalised, 0 for +inf; lam = 0: the first arg-min
    sample itself. None when no sample is finite (the caller keeps its nominal)."""
    cost = np.asarray(cost, dtype=np.float64)
    finite = np.isfinite(cost)
    if not finite.any():
        return None, np.zeros_like(cost), 0
    c = np.where(finite, cost, np.inf)
    best = int(np.argmin(c))
    if lam == 0:
        w = np.zeros_like(c)
        w[best] = 1.0
        return np.array(knots[best], dtype=np.float64), w, best
    e = np.where(finite, np.exp(-(np.where(finite, c, c[best]) - c[best]) / lam), 0.0)
    w = e / e.sum()
    return np.tensordot(w, np.asarray(knots, dtype=np.float64), axes=1), w, best
