"""A numpy float64 restatement of one Kalman covariance step (include/mgx.h "Kalman covariance
step") that shares no formula with the code under test: the INFORMATION form, restricted to the
measured rows by index selection (the code under test zeroes rows and never compacts),

    P- = A P A' + Q,   P+ = (P-^-1 + H' R^-1 H)^-1,   dx = P+ H' R^-1 r,   K = P+ H' R^-1,

with nis = r' S^-1 r by ``np.linalg.solve`` on S = H P- H' + R and log det S by ``slogdet``.
"""
import numpy as np

SEED = 0
COND_P, COND_S = 30.0, 20.0  # the conditions the tests assert on their inputs
TOL64 = 1e-12  # of max(1, |ref|): 400 x the disagreement of two float64 formulations on these inputs


def make_inputs(n, p, N, seed=SEED):
    """P = G G'/n + 0.5 I, H = N(0,1)/sqrt(n), R ~ U[0.5, 1.5], A = I + 0.3 N(0,1)/sqrt(n),
    Q_diag ~ U[0.01, 0.1], r ~ N(0,1), row_mask: each row on with probability 0.75, at least one on;
    Q (full) = J J'/n scaled to 0.05, for the calls that take it."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, n, n))
    d = dict(P=G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n),
             H=rng.standard_normal((N, p, n)) / np.sqrt(n),
             R_diag=rng.uniform(0.5, 1.5, (N, p)),
             A=np.eye(n) + 0.3 * rng.standard_normal((N, n, n)) / np.sqrt(n),
             Q_diag=rng.uniform(0.01, 0.1, (N, n)),
             resid=rng.standard_normal((N, p)))
    mask = rng.uniform(size=(N, p)) < 0.75
    for e in range(N):
        if not mask[e].any():
            mask[e, 0] = True
    d["row_mask"] = mask.astype(np.uint8)
    J = rng.standard_normal((N, n, n))
    d["Q"] = 0.05 * J @ J.transpose(0, 2, 1) / n
    return d


def reference(d, e, predict=True, update=True, use_mask=True, full_q=False):
    """The step of env ``e``: dict(P, Pm (the predicted covariance), dx, gain, nis [2], cond_P, cond_S,
    measured). dx, gain and nis are None without an update; gain has zero columns at masked rows."""
    n = d["P"].shape[1]
    P = d["P"][e]
    if predict:
        A = d["A"][e]
        P = A @ P @ A.T + np.diag(d["Q_diag"][e]) + (d["Q"][e] if full_q else 0.0)
    out = dict(Pm=P, P=P, dx=None, gain=None, nis=None, cond_P=np.linalg.cond(P), cond_S=1.0, measured=0)
    if not update:
        return out
    p = d["H"].shape[1]
    idx = np.flatnonzero(d["row_mask"][e]) if use_mask else np.arange(p)
    H, R, r = d["H"][e][idx], d["R_diag"][e][idx], d["resid"][e][idx]
    Pp = np.linalg.inv(np.linalg.inv(P) + H.T @ (H / R[:, None]))
    K = Pp @ H.T / R[None, :]
    S = H @ P @ H.T + np.diag(R)
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    gain = np.zeros((n, p))
    gain[:, idx] = K
    out.update(P=Pp, dx=K @ r, gain=gain, nis=np.array([r @ np.linalg.solve(S, r), logdet]),
               cond_S=np.linalg.cond(S), measured=len(idx))
    return out


def check_conditions(ref):
    assert ref["cond_P"] <= COND_P, ref["cond_P"]
    assert ref["cond_S"] <= COND_S, ref["cond_S"]


def errors(ref, P, dx=None, gain=None, nis=None):
    """The largest error of each output over max(1, |ref|), as a dict."""
    rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, np.abs(want).max()))  # noqa: E731
    out = dict(P=rel(P, ref["P"]))
    if ref["dx"] is not None:
        out.update(dx=rel(dx, ref["dx"]), nis=rel(nis[0], ref["nis"][0]), logdet=rel(nis[1], ref["nis"][1]))
        if gain is not None:
            out["gain"] = rel(gain, ref["gain"])
    return out
