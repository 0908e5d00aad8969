"""Numpy float64 reference of the box-constrained LQR backward pass (TEST INFRASTRUCTURE ONLY),
written against the text of include/mgx.h ("LQR backward pass") and Tassa, Mansard and Todorov 2014,
not against the HIP code or ilqr.py: the box QP here is the paper's projected Newton with its
value-based Armijo test and a gradient-norm stop, followed by one exact solve on the final free set,
so it shares neither the stopping rule nor the line search of the implementations under test. The
QP is strictly convex, so its minimiser is unique and any converged method gives it.

Also the input recipe the CPU and the GPU tests share, and the checks that need no reference (KKT)
or that guard the inputs (conditioning, margins, the clamped share).
"""
import numpy as np


def box_qp(H, q, lo, hi, x0, max_iter=500, min_grad=1e-14):
    """argmin 1/2 x'Hx + q'x over lo <= x <= hi. Returns (x, free bool [m])."""
    x = np.clip(x0, lo, hi)
    value = lambda v: 0.5 * v @ H @ v + q @ v  # noqa: E731
    free = np.ones(len(q), dtype=bool)
    for _ in range(max_iter):
        g = q + H @ x
        clamped = ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
        free = ~clamped
        if not free.any():
            break
        if np.abs(g[free]).max() <= min_grad * max(1.0, np.abs(q).max()):
            break
        gc = q + H @ np.where(clamped, x, 0.0)
        search = np.zeros_like(x)
        search[free] = -np.linalg.solve(H[np.ix_(free, free)], gc[free]) - x[free]
        sdotg = search @ g
        if sdotg >= 0:
            break
        step, v0 = 1.0, value(x)
        while True:
            xc = np.clip(x + step * search, lo, hi)
            if value(xc) - v0 <= 0.1 * step * sdotg or step < 1e-10:
                break
            step *= 0.6
        x = xc
    if free.any():
        # the exact minimiser on the final free set, kept when it stays inside the box
        xc = np.where(free, 0.0, x)
        y = x.copy()
        y[free] = -np.linalg.solve(H[np.ix_(free, free)], (q + H @ xc)[free])
        if ((y >= lo) & (y <= hi)).all():
            x = y
    return x, free


def lqr_backward_box(A, B, lx, lxx, lu, luu, lux, Vx, Vxx, mu, lo=None, hi=None):
    """One env: the recursion of tests/feedback_reference.lqr_backward with the step bounded by
    lo [T, m] <= k_t <= hi [T, m] (None: unbounded, the plain pass). Returns a dict: k [T, m],
    K [T, m, n], expected [2], free bool [T, m], conds (of the regularised Q_uu), Qu [T, m] and
    Qr [T, m, m] (the QP of every step, for the KKT check) and margin [T, m]: |g_i| / max(1, |Q_u|)
    on a clamped control, the distance to the nearer bound over the bound width on a free one (inf
    for an unbounded control)."""
    T, n, m = B.shape
    box = lo is not None
    lo = np.full((T, m), -np.inf) if lo is None else lo
    hi = np.full((T, m), np.inf) if hi is None else hi
    out = dict(k=np.zeros((T, m)), K=np.zeros((T, m, n)), expected=np.zeros(2), free=np.ones((T, m), dtype=bool),
               conds=[], Qu=np.zeros((T, m)), Qr=np.zeros((T, m, m)), margin=np.full((T, m), np.inf))
    k_next = np.zeros(m)
    for t in range(T - 1, -1, -1):
        Qu = lu[t] + B[t].T @ Vx
        Qux, Quu = lux[t] + B[t].T @ Vxx @ A[t], luu[t] + B[t].T @ Vxx @ B[t]
        Qr = Quu + mu * max(1.0, np.trace(Quu) / m) * np.eye(m)
        Qr = np.tril(Qr) + np.tril(Qr, -1).T
        out["conds"].append(np.linalg.cond(Qr))
        if box:
            k, free = box_qp(Qr, Qu, lo[t], hi[t], k_next)
        else:
            k, free = -np.linalg.solve(Qr, Qu), np.ones(m, dtype=bool)
        K = np.zeros((m, n))
        if free.any():
            K[free] = -np.linalg.solve(Qr[np.ix_(free, free)], Qux[free])
        g = Qu + Qr @ k
        with np.errstate(invalid="ignore"):
            width = hi[t] - lo[t]
            inside = np.where(np.isfinite(width), np.minimum(k - lo[t], hi[t] - k) / width, np.inf)
        out["margin"][t] = np.where(free, inside, np.abs(g) / max(1.0, np.abs(Qu).max()))
        out["expected"] += [k @ Qu, 0.5 * k @ Quu @ k]
        Acl = A[t] + B[t] @ K
        Vx = lx[t] + K.T @ (lu[t] + luu[t] @ k) + lux[t].T @ k + Acl.T @ (Vx + Vxx @ (B[t] @ k))
        Vxx = lxx[t] + K.T @ luu[t] @ K + K.T @ lux[t] + lux[t].T @ K + Acl.T @ Vxx @ Acl
        Vxx = 0.5 * (Vxx + Vxx.T)
        out["k"][t], out["K"][t], out["free"][t], out["Qu"][t], out["Qr"][t] = k, K, free, Qu, Qr
        k_next = k
    return out


GRAD_SCALE = 1.0  # of lx, lu and Vx_T: plain randn, as tests/test_ilqr_cpu.py draws them
SEED = 2  # of the shared cases: check_conditions holds for both envs at every size the tests use


def make_inputs(n, m, T, N=2, seed=0):
    """The recipe of the box tests: A = I + 0.1/sqrt(n) randn, B = randn/sqrt(n), lux = 0.1 randn/sqrt(n),
    diagonal lxx, luu in U(.5, 2) and Vxx_T in U(1, 4), lo = -0.3 |randn| - 0.05, hi = 0.3 |randn| + 0.05;
    lx, lu, Vx_T = GRAD_SCALE randn. float64 arrays with a leading env dim."""
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(n)
    d = dict(A=np.eye(n) + 0.1 * s * rng.normal(size=(N, T, n, n)), B=s * rng.normal(size=(N, T, n, m)),
             lux=0.1 * s * rng.normal(size=(N, T, m, n)))
    d["lxx_diag"], d["luu_diag"] = rng.uniform(0.5, 2, (N, T, n)), rng.uniform(0.5, 2, (N, T, m))
    d["lxx"] = d["lxx_diag"][..., None] * np.eye(n)
    d["luu"] = d["luu_diag"][..., None] * np.eye(m)
    d["Vxx_T"] = rng.uniform(1, 4, (N, n))[..., None] * np.eye(n)
    d["lo"] = -0.3 * np.abs(rng.normal(size=(N, T, m))) - 0.05
    d["hi"] = 0.3 * np.abs(rng.normal(size=(N, T, m))) + 0.05
    d["lx"], d["lu"] = GRAD_SCALE * rng.normal(size=(N, T, n)), GRAD_SCALE * rng.normal(size=(N, T, m))
    d["Vx_T"] = GRAD_SCALE * rng.normal(size=(N, n))
    return d


def reference(d, mu, box, e):
    """lqr_backward_box of env e of make_inputs' arrays."""
    return lqr_backward_box(d["A"][e], d["B"][e], d["lx"][e], d["lxx"][e], d["lu"][e], d["luu"][e], d["lux"][e],
                            d["Vx_T"][e], d["Vxx_T"][e], mu, d["lo"][e] if box else None, d["hi"][e] if box else None)


def check_conditions(ref, box):
    """What the inputs must satisfy for the comparison to mean something (asserted, not measured):
    cond(Q_uu) < 1e3, and with bounds a smallest margin >= 1e-4 and 20-60 % of the entries clamped."""
    assert max(ref["conds"]) < 1e3, ref["conds"]
    if box:
        share = 1.0 - ref["free"].mean()
        assert ref["margin"].min() >= 1e-4, ref["margin"].min()
        assert 0.2 <= share <= 0.6, share
        return float(ref["margin"].min()), float(share), float(max(ref["conds"]))
    return float("inf"), 0.0, float(max(ref["conds"]))


def check_kkt(ref, k, free, lo, hi):
    """KKT of the returned k on the reference's QPs (Q_u and the regularised Q_uu of every step):
    |g_i| <= 1e-9 max(1, |Q_u|) on free controls, g_i >= 0 at a lower and <= 0 at an upper bound within
    that tolerance, and k inside the box. ``free`` is the implementation's own set."""
    T, m = k.shape
    for t in range(T):
        g = ref["Qu"][t] + ref["Qr"][t] @ k[t]
        tol = 1e-9 * max(1.0, np.abs(ref["Qu"][t]).max())
        fr = free[t].astype(bool)
        assert (np.abs(g[fr]) <= tol).all(), (t, np.abs(g[fr]).max(), tol)
        if lo is not None:
            assert ((k[t] >= lo[t]) & (k[t] <= hi[t])).all(), t
            at_lo, at_hi = ~fr & (k[t] == lo[t]), ~fr & (k[t] == hi[t])
            assert (at_lo | at_hi)[~fr].all(), t  # a clamped control sits on a bound
            assert (g[at_lo] >= -tol).all() and (g[at_hi] <= tol).all(), t


def compare(ref, k, K, expected, free):
    """k, K and expected within 1e-9 max(1, |k|, |K|) of the reference (the rule of
    tests/test_ilqr_cpu.py), the free sets equal. Returns the largest scaled error."""
    scale = max(1.0, np.abs(ref["K"]).max(), np.abs(ref["k"]).max())
    ek, eK = np.abs(k - ref["k"]).max(), np.abs(K - ref["K"]).max()
    ee = np.abs(expected - ref["expected"]).max() / max(1.0, np.abs(ref["expected"]).max())
    assert ek <= 1e-9 * scale and eK <= 1e-9 * scale and ee <= 1e-9, (ek, eK, ee, scale)
    assert np.array_equal(free.astype(bool), ref["free"])
    return max(ek / scale, eK / scale, ee)
