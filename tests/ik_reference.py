"""numpy float64 reference for mgx_ik (TEST INFRASTRUCTURE ONLY): the damped-least-squares
iteration of include/mgx.h "inverse kinematics", restated step by step from the header — written
against the text, not the HIP code.

Kinematics come from the CPU oracle (``RefSim.forward()`` at each iterate) and the Jacobian rows
from ``dyn_reference.jac``; the error rows, A = J J' + lambda^2 I, the Cholesky factor, the two
triangular solves, the step limit, mj_integratePos and the joint-limit clamp are computed here and
pinned by tests/test_ik_cpu.py (closed forms on tiny models).
"""
import numpy as np

from tests import dyn_reference as dr

CONVERGED, MAX_ITER, FAILED = 0, 1, 2  # include/mgx.h MGX_IK_*
KIN_FIELDS = ("cdof", "subtree_com", "xpos", "xmat", "xipos", "xquat")


def quat_mul(a, b):
    return dr._quat_mul(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def quat_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def normalize4(q):
    """mju_normalize4: a zero quaternion becomes the identity."""
    q = np.array(q, dtype=np.float64)
    n = np.linalg.norm(q)
    return np.array([1.0, 0.0, 0.0, 0.0]) if n < 1e-15 else q / n


def rotvec(q):
    """The rotation vector of quaternion q: angle 2 atan2(|v|, w) wrapped to (-pi, pi]; 0 for a zero
    vector part (mgx_transition_fd's convention)."""
    n = np.linalg.norm(q[1:])
    if n == 0:
        return np.zeros(3)
    ang = 2.0 * np.arctan2(n, q[0])
    if ang > np.pi:
        ang -= 2.0 * np.pi
    return q[1:] / n * ang


def _quat_integrate(q, w):
    """quat <- normalize(quat) o exp(w): the rotation vector w in the local frame."""
    ang = np.linalg.norm(w)
    q = normalize4(q)
    if ang < 1e-15:  # mju_normalize3 puts the axis on x; the angle is 0 to rounding
        ang, ax = float(ang), np.array([1.0, 0.0, 0.0])
    else:
        ax = w / ang
    if ang == 0:
        return q
    return quat_mul(q, np.array([np.cos(0.5 * ang), *(np.sin(0.5 * ang) * ax)]))


def integrate_pos(model, qpos, delta):
    """mj_integratePos(qpos, delta, 1): hinge, slide and free translation add; free and ball
    rotations compose the quaternion with exp(delta) in the local frame."""
    m, q = model, np.array(qpos, dtype=np.float64)
    for j in range(m.njnt):
        t, a, d = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        if t == 0:
            q[a:a + 3] += delta[d:d + 3]
            q[a + 3:a + 7] = _quat_integrate(q[a + 3:a + 7], delta[d + 3:d + 6])
        elif t == 1:
            q[a:a + 4] = _quat_integrate(q[a:a + 4], delta[d:d + 3])
        else:
            q[a] += delta[d]
    return q


def clamp_limits(model, qpos, dof_mask=None):
    """Limited hinge and slide coordinates whose dof may move, clamped to jnt_range."""
    m, q = model, np.array(qpos, dtype=np.float64)
    rng = np.asarray(m.jnt_range, dtype=np.float64).reshape(-1, 2)
    for j in range(m.njnt):
        if int(m.jnt_type[j]) not in (2, 3) or not int(m.jnt_limited[j]):
            continue
        if dof_mask is not None and not dof_mask[int(m.jnt_dofadr[j])]:
            continue
        a = int(m.jnt_qposadr[j])
        q[a] = min(max(q[a], rng[j, 0]), rng[j, 1]) if np.isfinite(q[a]) else q[a]
    return q


def restore_masked(model, q, before, dof_mask):
    """What a masked dof owns keeps the bits of ``before`` (include/mgx.h): hinge, slide and free
    translation coordinates, and a quaternion whose three rotational dofs are all masked."""
    m = model
    for j in range(m.njnt):
        t, a, d = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        if t in (2, 3):
            if not dof_mask[d]:
                q[a] = before[a]
            continue
        ro = 3 if t == 0 else 0
        if t == 0:
            for c in range(3):
                if not dof_mask[d + c]:
                    q[a + c] = before[a + c]
        if not dof_mask[d + ro:d + ro + 3].any():
            q[a + ro:a + ro + 4] = before[a + ro:a + ro + 4]
    return q


def kinematics(sim, q):
    """The oracle's kinematic fields at qpos = q."""
    sim.qpos[:] = q
    sim.forward()
    return {f: sim.field(f).copy() for f in KIN_FIELDS}


def error_rows(model, F, entries, quats, pos_weight, rot_weight, target_pos, target_quat):
    """e: per point its weighted position rows, then its weighted orientation rows."""
    rows = []
    for p, (kind, body, pos) in enumerate(entries):
        if pos_weight[p] > 0:
            rows.append(pos_weight[p] * (target_pos[p] - dr.point_of(model, F, kind, body, pos)))
        if rot_weight[p] > 0:
            cur = quat_mul(F["xquat"].reshape(-1, 4)[int(body)], quats[p])
            rows.append(rot_weight[p] * rotvec(quat_mul(normalize4(target_quat[p]), quat_conj(cur))))
    return np.concatenate(rows)


def jacobian_rows(model, F, entries, pos_weight, rot_weight, dof_mask):
    rows = []
    for p, (kind, body, pos) in enumerate(entries):
        jp, jr, _ = dr.jac(model, F, kind, body, pos)
        if pos_weight[p] > 0:
            rows.append(pos_weight[p] * jp)
        if rot_weight[p] > 0:
            rows.append(rot_weight[p] * jr)
    J = np.concatenate(rows)
    if dof_mask is not None:
        J[:, ~np.asarray(dof_mask, dtype=bool)] = 0.0
    return J


def cholesky_solve(A, e):
    """y = A^-1 e through A = L L' column by column; None when a pivot is not positive and finite."""
    m = len(e)
    L = np.zeros((m, m))
    for j in range(m):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not (s[0] > 0 and np.isfinite(s[0])):
            return None
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    z = np.array(e, dtype=np.float64)
    for j in range(m):
        z[j] /= L[j, j]
        z[j + 1:] -= L[j + 1:, j] * z[j]
    for j in range(m - 1, -1, -1):
        z[j] /= L[j, j]
        z[:j] -= L[j, :j] * z[j]
    return z


def step(model, J, e, damping, max_step):
    """delta of one update (None on a bad pivot)."""
    y = cholesky_solve(J @ J.T + damping * damping * np.eye(len(e)), e)
    if y is None:
        return None
    delta = J.T @ y
    s = float(np.max(np.abs(delta)))
    return delta * (max_step / s) if s > max_step else delta


def solve(model, sim, qpos, entries, target_pos, target_quat=None, quats=None, pos_weight=1.0, rot_weight=0.0,
          dof_mask=None, damping=0.05, max_step=0.3, tol=1e-6, max_iter=50, clamp=True, trace=None):
    """mgx_ik for one env: (qpos, residual, iters, status). ``entries``: [(kind, body, pos)] as
    dyn_reference.jac_entries gives them; ``quats`` [P, 4] the body-frame orientation offsets (None:
    identity); the weights are scalars or one per point; ``sim`` is a RefSim of the model (its qpos
    is overwritten). ``trace``: a list that receives the residual of every iteration."""
    P = len(entries)
    wp = np.broadcast_to(np.asarray(pos_weight, dtype=np.float64), (P,))
    wr = np.broadcast_to(np.asarray(rot_weight, dtype=np.float64), (P,))
    quats = np.tile([1.0, 0.0, 0.0, 0.0], (P, 1)) if quats is None else np.asarray(quats, dtype=np.float64)
    mask = None if dof_mask is None else np.asarray(dof_mask, dtype=bool)
    q = np.array(qpos, dtype=np.float64)
    if clamp:
        q = clamp_limits(model, q, mask)
    it = 0
    while True:
        F = kinematics(sim, q)
        e = error_rows(model, F, entries, quats, wp, wr, target_pos, target_quat)
        r = float(np.sqrt(np.sum(e * e)))
        if trace is not None:
            trace.append(r)
        if not np.isfinite(r):
            return q, r, it, FAILED
        if r <= tol:
            return q, r, it, CONVERGED
        if it == max_iter:
            return q, r, it, MAX_ITER
        delta = step(model, jacobian_rows(model, F, entries, wp, wr, mask), e, damping, max_step)
        if delta is None:
            return q, r, it, FAILED
        before = q
        q = integrate_pos(model, q, delta)
        if mask is not None:
            q = restore_masked(model, q, before, mask)
        if clamp:
            q = clamp_limits(model, q, mask)
        it += 1


# ---------------------------------------------------------------------------- task cases
def local_points(task):
    """The LOCAL points of dyn_reference.POINTS[task]: (jac_points keywords, names in its order)."""
    kw = {k: v for k, v in dr.POINTS[task][0].items() if k in ("body", "site", "geom")}
    return kw, [f"{k}:{kw[k]}" for k in ("body", "site", "geom") if k in kw]


def local_entries(task, model):
    """[(kind, body, pos)] and the orientation offsets [P, 4] of local_points(task)."""
    m, (kw, _) = model, local_points(task)
    entries, quats = [], []
    if "body" in kw:
        entries.append((dr.LOCAL, list(m.body_names).index(kw["body"]), np.zeros(3)))
        quats.append([1.0, 0.0, 0.0, 0.0])
    if "site" in kw:
        s = list(m.site_names).index(kw["site"])
        entries.append((dr.LOCAL, int(m.site_bodyid[s]), np.asarray(m.site_pos).reshape(-1, 3)[s].copy()))
        quats.append(np.asarray(m.site_quat).reshape(-1, 4)[s])
    if "geom" in kw:
        g = list(m.geom_names).index(kw["geom"])
        entries.append((dr.LOCAL, int(m.geom_bodyid[g]), np.asarray(m.geom_pos).reshape(-1, 3)[g].copy()))
        quats.append(np.asarray(m.geom_quat).reshape(-1, 4)[g])
    return entries, np.array(quats, dtype=np.float64)


def pose_of(model, F, entries, quats):
    """(pos [P, 3], quat [P, 4]) of the target frames at the oracle fields F."""
    pos = np.array([dr.point_of(model, F, k, b, p) for k, b, p in entries])
    quat = np.array([quat_mul(F["xquat"].reshape(-1, 4)[int(b)], quats[i]) for i, (_, b, _) in enumerate(entries)])
    return pos, quat


def reachable_target(model, sim, qpos, entries, quats, rng, spread, dof_mask=None):
    """A target that some qpos reaches: the frames' poses at qpos integrated by U(+-spread) on every
    (unmasked) dof, then clamped to the joint limits."""
    d = rng.uniform(-spread, spread, model.nv)
    if dof_mask is not None:
        d = d * np.asarray(dof_mask, dtype=np.float64)
    q = clamp_limits(model, integrate_pos(model, clamp_limits(model, qpos), d))
    return pose_of(model, kinematics(sim, q), entries, quats)


# ---------------------------------------------------------------------------- the convergence set
CONV_SEED, CONV_TOL, CONV_MAX_ITER = 7, 1e-6, 50
ARM_JOINTS = ("j1_shoulder_pan", "j2_shoulder_tilt", "j3_elbow", "j4_wrist_roll", "j5_wrist_pitch", "j6_wrist_yaw",
              "j7_gripper_base")  # robotic_arm_assembly's seven arm dofs
# group -> (task, jac_points keywords, rot_weight, joints that may move or None, damping, target spread)
CONV_GROUPS = {f"{t}-pos": (t, None, 0.0, None, 0.05, 0.3) for t in dr.TASKS}
CONV_GROUPS["construction-pose"] = ("construction", None, 1.0, None, 0.05, 0.3)
CONV_GROUPS["assembly-arm"] = ("assembly", dict(site="ee_site"), 1.0, ARM_JOINTS, 0.01, 0.4)
# the groups whose every env must be in the set (a condition on the reference, asserted by
# tests/test_ik_cpu.py): the others join env by env if the reference converges on them
CONV_REQUIRED = ("parkour-pos", "bipedal-pos", "dancing-pos", "construction-pos", "construction-pose", "assembly-arm")
_conv_cache = {}


def group_setup(group):
    """(task, jac_points keywords, entries, quats, rot_weight, dof_mask or None, joints, damping, spread)"""
    task, kw, rot, joints, damping, spread = CONV_GROUPS[group]
    model = dr.case(task)[0]
    if kw is None:
        kw = local_points(task)[0]
        entries, quats = local_entries(task, model)
    else:
        s = list(model.site_names).index(kw["site"])
        entries = [(dr.LOCAL, int(model.site_bodyid[s]), np.asarray(model.site_pos).reshape(-1, 3)[s].copy())]
        quats = np.asarray(model.site_quat, dtype=np.float64).reshape(-1, 4)[s][None]
    mask = None
    if joints is not None:
        mask = np.zeros(model.nv, dtype=bool)
        for name in joints:
            mask[int(model.jnt_dofadr[list(model.jnt_names).index(name)])] = True
    return task, kw, entries, quats, rot, mask, joints, damping, spread


def convergence_group(group):
    """Per env of dyn_reference.case(task): dict(target_pos, target_quat, ref=(qpos, residual, iters,
    status), member). An env is a member when the reference reaches CONV_TOL within half of
    CONV_MAX_ITER. Computed once and shared (treat as read-only)."""
    if group not in _conv_cache:
        from oracle.mjref import RefSim
        task, _, entries, quats, rot, mask, _, damping, spread = group_setup(group)
        model, packed, states, _ = dr.case(task)
        sim = RefSim(packed)
        rng = np.random.default_rng([CONV_SEED, sorted(CONV_GROUPS).index(group)])
        out = []
        for s in states:
            tp, tq = reachable_target(model, sim, s["qpos"], entries, quats, rng, spread, mask)
            ref = solve(model, sim, s["qpos"], entries, tp, tq, quats, 1.0, rot, mask, damping=damping, tol=CONV_TOL,
                        max_iter=CONV_MAX_ITER)
            out.append(dict(target_pos=tp, target_quat=tq, ref=ref,
                            member=ref[3] == CONVERGED and ref[2] <= CONV_MAX_ITER // 2))
        _conv_cache[group] = out
    return _conv_cache[group]
