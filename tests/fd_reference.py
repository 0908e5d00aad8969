"""numpy reference for mgx_transition_fd (TEST INFRASTRUCTURE ONLY): MuJoCo's mjd_transitionFD
[ext] as include/mgx.h restates it — written against that text, not the HIP code.

A "virtual env" list is the nominal state followed by one state per perturbed column, in the order
the library documents: forward mode K = 2 nv + nu states (+eps, or what the control-limit rule
takes instead), centred mode K with +eps then K with -eps. ``virtual_steps`` gives each one's
(column, signed step); ``perturb`` builds its state; ``difference`` turns the stepped states into
(A, B). ``oracle_fd`` runs them through the CPU oracle in float64; the GPU tests run them through
``PhysicsBatch.step`` instead (the hand-built composition the library call replaces).
tests/test_fd_cpu.py pins this file by closed forms.
"""
import numpy as np

from tests import dyn_reference as dr
from tests.helpers import STATE_FIELDS

FREE, BALL = 0, 1  # jnt_type

# ---------------------------------------------------------------------------- small models
# one slide joint with a spring, a damper and a motor, no gravity: the step is linear in (q, v, u)
MASS, STIFF, DAMP, GEAR, H = 2.0, 30.0, 2.0, 5.0, 0.01
SLIDE = """<mujoco><option timestep="0.01" gravity="0 0 0"{integrator}/><worldbody><body name="cart">
  <joint name="x" type="slide" axis="1 0 0" stiffness="30" damping="2"/><geom type="sphere" size="0.1" mass="2"/>
  </body></worldbody><actuator><motor joint="x" gear="5"/></actuator></mujoco>"""
SLIDE_STATE = (0.3, -0.7, 0.4)  # q, v, u
# a free box carrying a ball-jointed capsule, no contact, no actuator
FREE_BALL = """<mujoco><option gravity="0 0 -9.81"/><worldbody><body name="box" pos="0 0 1"><freejoint/>
  <geom type="box" size="0.1 0.2 0.15" mass="1.5"/><body name="link" pos="0.1 0 0"><joint type="ball"/>
  <geom type="capsule" size="0.04" fromto="0 0 0 0.3 0 0" mass="0.4"/></body></body></worldbody></mujoco>"""
# two hinges, the first motor limited to [-1, 1]
TWO_ACT = """<mujoco><worldbody><body name="a" pos="0 0 1"><joint name="j0" type="hinge" axis="0 1 0" damping="0.1"/>
  <geom type="capsule" size="0.03" fromto="0 0 0 0.4 0 0" mass="1"/><body name="b" pos="0.4 0 0">
  <joint name="j1" type="hinge" axis="0 1 0" damping="0.1"/><geom type="capsule" size="0.03" fromto="0 0 0 0.3 0 0" mass="0.5"/>
  </body></body></worldbody><actuator><motor joint="j0" gear="2" ctrllimited="true" ctrlrange="-1 1"/>
  <motor joint="j1" gear="3"/></actuator></mujoco>"""


def quat_dofs(model):
    """[(qpos address of the quaternion, address of its first tangent dof)] of free and ball joints."""
    m, out = model, []
    for j in range(m.njnt):
        t, a, d = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        if t == FREE:
            out.append((a + 3, d + 3))
        elif t == BALL:
            out.append((a, d))
    return out


def scalar_map(model):
    """int [nv]: the qpos index of a hinge, slide or free-translation dof; -1 for a quaternion dof."""
    m = model
    qi = np.full(m.nv, -1, dtype=np.int64)
    for d in range(m.nv):
        j = int(m.dof_jntid[d])
        t, k = int(m.jnt_type[j]), d - int(m.jnt_dofadr[j])
        if t in (2, 3) or (t == FREE and k < 3):
            qi[d] = int(m.jnt_qposadr[j]) + k
    return qi


def quat_rotvec(q1, q0):
    """The rotation vector of conj(q0) o q1: angle 2 atan2(|v|, w) wrapped to (-pi, pi]; 0 for v = 0."""
    c = np.array([q0[0], -q0[1], -q0[2], -q0[3]], dtype=np.float64)
    d = dr._quat_mul(c, np.asarray(q1, dtype=np.float64))
    n = float(np.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]))
    if n == 0.0:
        return np.zeros(3)
    ang = 2.0 * np.arctan2(n, d[0])
    if ang > np.pi:
        ang -= 2.0 * np.pi
    return d[1:] / n * ang


def differentiate_pos(model, q1, q0):
    """mj_differentiatePos: float64 [nv], the tangent-space difference q1 - q0 (unit time)."""
    q1, q0 = np.asarray(q1, dtype=np.float64), np.asarray(q0, dtype=np.float64)
    out = np.zeros(model.nv)
    qi = scalar_map(model)
    s = qi >= 0
    out[s] = q1[qi[s]] - q0[qi[s]]
    for a, d in quat_dofs(model):
        out[d:d + 3] = quat_rotvec(q1[a:a + 4], q0[a:a + 4])
    return out


def ctrl_sides(model, ctrl, eps, dtype=np.float64):
    """(nominal, plus_ok, minus_ok): the ctrl the step uses (clamped to actuator_ctrlrange where
    ctrllimited) and, per actuator, whether nominal + eps / nominal - eps stays inside the range of
    a limited actuator (always, for an unlimited one); arithmetic in ``dtype``."""
    m = model
    c = np.asarray(ctrl, dtype=np.float64)[:m.nu].astype(dtype)
    e = dtype(eps)
    lim = np.asarray(m.actuator_ctrllimited).reshape(-1).astype(bool)[:m.nu]
    rng = np.asarray(m.actuator_ctrlrange, dtype=np.float64).reshape(-1, 2).astype(dtype)[:m.nu]
    nom = np.where(lim, np.minimum(np.maximum(c, rng[:, 0]), rng[:, 1]), c).astype(dtype)
    plus = ~lim | ((nom + e).astype(dtype) <= rng[:, 1])
    minus = ~lim | ((nom - e).astype(dtype) >= rng[:, 0])
    return nom, plus, minus


def virtual_steps(model, ctrl, eps, centered, dtype=np.float64):
    """[(column, signed step)] of the virtual envs after the nominal one. The control-limit rule:
    forward mode takes +eps if it stays inside, else -eps, else no step (0); centred mode takes each
    side that stays inside."""
    m = model
    K = 2 * m.nv + m.nu
    _, plus, minus = ctrl_sides(m, ctrl, eps, dtype)
    e = float(dtype(eps))
    out = []
    for k in range(K):
        u = k - 2 * m.nv
        if u < 0 or plus[u]:
            out.append((k, e))
        elif centered:
            out.append((k, 0.0))
        else:
            out.append((k, -e if minus[u] else 0.0))
    if centered:
        for k in range(K):
            u = k - 2 * m.nv
            out.append((k, -e if (u < 0 or minus[u]) else 0.0))
    return out


def perturb(model, state, column, signed_eps, dtype=np.float64):
    """The state of one virtual env: ``state`` (a dict of tests.helpers.STATE_FIELDS) rounded to
    ``dtype``, its ctrl clamped to the nominal one, and ``column`` moved by ``signed_eps``: a scalar
    coordinate, qvel or ctrl entry by one add in ``dtype``, a quaternion dof by
    dyn_reference.integrate_pos. column None (or a zero step) gives the nominal state. Values are
    returned as float64 arrays holding ``dtype`` numbers (quaternions: float64, rounded on load)."""
    m = model
    s = {f: np.asarray(state[f], dtype=np.float64).astype(dtype).astype(np.float64) for f in STATE_FIELDS}
    h = dtype(signed_eps)
    s["ctrl"][:m.nu] = ctrl_sides(m, s["ctrl"], 1.0, dtype)[0]  # the nominal ctrl does not depend on eps
    if column is None or h == 0:
        return s
    if column < m.nv:
        qi = scalar_map(m)[column]
        if qi >= 0:
            s["qpos"][qi] = dtype(s["qpos"][qi]) + h
        else:
            s["qpos"] = dr.integrate_pos(m, s["qpos"], column, float(h))
    elif column < 2 * m.nv:
        s["qvel"][column - m.nv] = dtype(s["qvel"][column - m.nv]) + h
    else:
        s["ctrl"][column - 2 * m.nv] = dtype(s["ctrl"][column - 2 * m.nv]) + h
    return s


def virtual_states(model, state, eps, centered, dtype=np.float64):
    """(states [C], steps [C - 1]): the nominal state and every perturbed one, in the library's order."""
    steps = virtual_steps(model, np.asarray(state["ctrl"], dtype=np.float64).astype(dtype), eps, centered, dtype)
    return [perturb(model, state, None, 0.0, dtype)] + [perturb(model, state, k, h, dtype) for k, h in steps], steps


def difference(model, qpos, qvel, steps, eps, centered, dtype=np.float64):
    """(A [2nv, 2nv], B [2nv, nu]) in ``dtype`` from the stepped virtual envs' qpos [C, nq] and qvel
    [C, nv] (arrays of ``dtype``): every entry is (a - b) / step in ``dtype``; quaternion rows are
    the float64 rotation vector, rounded to ``dtype`` before the division. Centred columns with both
    sides taken divide their difference by 2 eps; one side taken is that one-sided difference."""
    m = model
    nv, K = m.nv, 2 * m.nv + m.nu
    qpos, qvel = np.asarray(qpos, dtype=dtype), np.asarray(qvel, dtype=dtype)
    qi = scalar_map(m)
    sc = qi >= 0
    quats = quat_dofs(m)

    def delta(i, j):
        out = np.zeros(2 * nv, dtype=dtype)
        out[:nv][sc] = qpos[i, qi[sc]] - qpos[j, qi[sc]]
        for a, d in quats:
            out[d:d + 3] = quat_rotvec(qpos[i, a:a + 4].astype(np.float64), qpos[j, a:a + 4].astype(np.float64)).astype(dtype)
        out[nv:] = qvel[i] - qvel[j]
        return out

    M = np.zeros((2 * nv, K), dtype=dtype)
    two_eps = dtype(2) * dtype(eps)
    for k in range(K):
        hp = dtype(steps[k][1])
        if not centered:
            if hp != 0:
                M[:, k] = delta(1 + k, 0) / hp
            continue
        hm = dtype(steps[K + k][1])
        if hp != 0 and hm != 0:
            M[:, k] = delta(1 + k, 1 + K + k) / two_eps
        elif hp != 0:
            M[:, k] = delta(1 + k, 0) / hp
        elif hm != 0:
            M[:, k] = delta(1 + K + k, 0) / hm
    return M[:, :2 * nv].copy(), M[:, 2 * nv:].copy()


def oracle_fd(model, packed, state, eps=1e-6, centered=False, nsub=1, reverse=False):
    """(A, B, next_qpos, next_qvel) of the CPU oracle in float64: one RefSim, reloaded with each
    virtual env's state and stepped ``nsub`` times. reverse: the oracle's twin (set_pgs_reverse)."""
    from oracle.mjref import RefSim
    sim = RefSim(packed)
    if reverse:
        sim.set_pgs_reverse(True)
    states, steps = virtual_states(model, state, eps, centered)
    qpos, qvel = [], []
    for s in states:
        for f in STATE_FIELDS:
            sim.field(f)[:] = s[f]
        sim.step(nsub)
        qpos.append(sim.qpos.copy())
        qvel.append(sim.qvel.copy())
    A, B = difference(model, np.stack(qpos), np.stack(qvel), steps, eps, centered)
    return A, B, qpos[0], qvel[0]
