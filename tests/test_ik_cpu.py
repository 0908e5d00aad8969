"""CPU: tests/ik_reference.py (the numpy reference the GPU inverse-kinematics tests compare with)
against known answers on tiny hand-written models, the C-ABI of mgx_ik against cabi.py, and the
membership of the convergence set the GPU convergence test runs on.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mujoco_gymnasium_environments_amd import cabi, mjcf, native
from tests import dyn_reference as dr
from tests import ik_reference as ir


def _sim(xml):
    from oracle.mjref import RefSim
    model = mjcf.compile_xml(xml)
    return model, RefSim(cabi.pack_model(model))


def _site(model, name):
    s = model.site_names.index(name)
    return (dr.LOCAL, int(model.site_bodyid[s]), np.asarray(model.site_pos).reshape(-1, 3)[s].copy())


# ---------------------------------------------------------------- C-ABI and plumbing
IK_FIELDS = ("pos_weight", "rot_weight", "damping", "max_step", "tol", "max_iter", "flags", "target_pos", "target_quat",
             "dof_mask", "qpos_init", "qpos", "residual", "iters", "status")


def test_header_matches_ctypes(tmp_path):
    """mgx_ik_io's size and every field offset, and the MGX_IK_* constants, of include/mgx.h against
    cabi.py; the ABI version is unchanged (the section only adds)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    offs = "".join(f' printf("%zu ", offsetof(mgx_ik_io, {f}));' for f in IK_FIELDS)
    prog = tmp_path / "ik.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                    'int main(void){printf("%zu ", sizeof(mgx_ik_io));' + offs +
                    ' printf("%d %d %d %d %d %d\\n", MGX_IK_MAX_POINT, MGX_IK_CLAMP_LIMITS, MGX_IK_CONVERGED,'
                    ' MGX_IK_MAX_ITER, MGX_IK_FAILED, MGX_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "ik"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [C.sizeof(cabi.MgxIkIO)] + [getattr(cabi.MgxIkIO, f).offset for f in IK_FIELDS] + \
        [cabi.MGX_IK_MAX_POINT, cabi.MGX_IK_CLAMP_LIMITS, cabi.MGX_IK_CONVERGED, cabi.MGX_IK_MAX_ITER,
         cabi.MGX_IK_FAILED, 6]
    assert [f for f, _ in cabi.MgxIkIO._fields_] == list(IK_FIELDS) and cabi.MGX_ABI_VERSION == 6
    assert (ir.CONVERGED, ir.MAX_ITER, ir.FAILED) == (cabi.MGX_IK_CONVERGED, cabi.MGX_IK_MAX_ITER, cabi.MGX_IK_FAILED)


def test_library_exports_and_sources():
    assert "mgx_ik" in native.EXPORTS
    assert "mgx_ik.hip" in native.SOURCES and "mgx_ik.h" in native.TU_HEADERS["mgx_ik.hip"]
    assert os.path.exists(os.path.join(native.CSRC, "mgx_ik.hip"))


# ---------------------------------------------------------------- known answers
PEND_L = 0.7
PENDULUM = f"""<mujoco><compiler angle="radian"/><worldbody><body name="arm" pos="0 0 1">
  <joint name="hinge" type="hinge" axis="0 0 1" limited="true" range="-1 1"/>
  <geom type="sphere" size="0.05" pos="{PEND_L} 0 0" mass="2"/><site name="tip" pos="{PEND_L} 0 0"/></body>
</worldbody></mujoco>"""


def _tip(q):
    return np.array([PEND_L * np.cos(q), PEND_L * np.sin(q), 1.0])


def test_single_iteration_closed_form():
    """One hinge, one update: delta = J'e / (J J' + lambda^2) with J = z x r a single column."""
    model, sim = _sim(PENDULUM)
    q0, lam = 0.2, 0.05
    target = _tip(0.5)
    r0 = _tip(q0) - [0, 0, 1]
    j = np.cross([0, 0, 1.0], r0)
    e = target - _tip(q0)
    delta = (j @ e) / (j @ j + lam * lam)
    q, res, it, status = ir.solve(model, sim, [q0], [_site(model, "tip")], target[None], damping=lam, max_step=10.0,
                                  tol=0.0, max_iter=1, clamp=False)
    assert it == 1 and status == ir.MAX_ITER
    assert abs(q[0] - (q0 + delta)) < 1e-14
    assert abs(res - np.linalg.norm(target - _tip(q0 + delta))) < 1e-14   # the residual is that of the last q


def test_max_iter_zero_only_computes_the_residual():
    model, sim = _sim(PENDULUM)
    target = _tip(0.5)
    q, res, it, status = ir.solve(model, sim, [0.2], [_site(model, "tip")], target[None], max_iter=0, tol=0.0)
    assert it == 0 and status == ir.MAX_ITER and q[0] == 0.2
    assert abs(res - np.linalg.norm(target - _tip(0.2))) < 1e-15
    # a start on the target stops converged before any update, whatever max_iter is
    q, res, it, status = ir.solve(model, sim, [0.5], [_site(model, "tip")], target[None], max_iter=7, tol=1e-12)
    assert (it, status) == (0, ir.CONVERGED) and q[0] == 0.5


def test_target_beyond_a_joint_limit():
    """The target asks for q = 1.4 with the hinge limited to [-1, 1]: the joint ends on the limit."""
    model, sim = _sim(PENDULUM)
    q, res, it, status = ir.solve(model, sim, [0.2], [_site(model, "tip")], _tip(1.4)[None], max_iter=30, tol=1e-6)
    assert status == ir.MAX_ITER and it == 30
    assert q[0] == 1.0
    assert abs(res - np.linalg.norm(_tip(1.4) - _tip(1.0))) < 1e-12
    # a start outside the range is clamped before the first iteration (max_iter = 0: nothing else moves it)
    q, _, _, _ = ir.solve(model, sim, [1.7], [_site(model, "tip")], _tip(0.0)[None], max_iter=0)
    assert q[0] == 1.0
    q, _, _, _ = ir.solve(model, sim, [1.7], [_site(model, "tip")], _tip(0.0)[None], max_iter=0, clamp=False)
    assert q[0] == 1.7


L1, L2 = 0.5, 0.4
TWO_LINK = f"""<mujoco><worldbody><body name="l1"><joint name="j1" type="hinge" axis="0 1 0"/>
  <geom type="sphere" size="0.05" pos="{L1} 0 0" mass="1.3"/>
  <body name="l2" pos="{L1} 0 0"><joint name="j2" type="hinge" axis="0 1 0"/>
    <geom type="sphere" size="0.05" pos="{L2} 0 0" mass="0.7"/><site name="tip" pos="{L2} 0 0"/></body></body>
</worldbody></mujoco>"""


def _two_link_tip(q):
    # hinges about +y: a positive angle turns x towards -z
    a, b = q[0], q[0] + q[1]
    return np.array([L1 * np.cos(a) + L2 * np.cos(b), 0.0, -L1 * np.sin(a) - L2 * np.sin(b)])


def test_planar_two_link_arm_reaches_an_analytic_branch():
    model, sim = _sim(TWO_LINK)
    target = _two_link_tip([0.9, -1.1])
    tol = 1e-10
    q, res, it, status = ir.solve(model, sim, [0.3, -0.4], [_site(model, "tip")], target[None], damping=0.01, tol=tol,
                                  max_iter=200)
    assert status == ir.CONVERGED and res <= tol and it < 200
    assert np.linalg.norm(_two_link_tip(q) - target) <= tol + 1e-14
    # the two branches of the planar problem: elbow angle +-acos(...), shoulder from the triangle
    x, z = target[0], -target[2]
    c2 = (x * x + z * z - L1 * L1 - L2 * L2) / (2 * L1 * L2)
    branches = []
    for q2 in (np.arccos(c2), -np.arccos(c2)):
        q1 = np.arctan2(z, x) - np.arctan2(L2 * np.sin(q2), L1 + L2 * np.cos(q2))
        branches.append(np.array([q1, q2]))
    wrapped = (q + np.pi) % (2 * np.pi) - np.pi
    assert min(np.abs(wrapped - b).max() for b in branches) < 1e-8
    assert any(np.abs(np.array([0.9, -1.1]) - b).max() < 1e-12 for b in branches)   # the formula is the arm's


FREE = """<mujoco><option gravity="0 0 0"/><worldbody><body name="b" pos="0 0 2"><freejoint/>
  <geom type="box" size="0.1 0.2 0.3" mass="1.5"/><site name="s" pos="0.1 0.05 -0.2" quat="0.5 0.5 -0.5 0.5"/></body>
</worldbody></mujoco>"""


def test_free_box_reaches_a_pose():
    """Position and orientation of a site on a free box: the site's world orientation
    xquat[body] o site_quat matches the target up to sign, its position to tol."""
    model, sim = _sim(FREE)
    s = model.site_names.index("s")
    squat = np.asarray(model.site_quat, dtype=np.float64).reshape(-1, 4)[s][None]
    tq = np.array([0.3, -0.5, 0.7, 0.4])   # not normalised: the solver normalises it
    tp = np.array([[0.4, -0.3, 1.5]])
    q0 = np.array([0.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0])
    tol = 1e-9
    q, res, it, status = ir.solve(model, sim, q0, [_site(model, "s")], tp, tq[None], squat, 1.0, 1.0, damping=0.01,
                                  max_step=0.5, tol=tol, max_iter=100)
    assert status == ir.CONVERGED and res <= tol
    F = ir.kinematics(sim, q)
    pos, quat = ir.pose_of(model, F, [_site(model, "s")], squat)
    assert np.linalg.norm(pos[0] - tp[0]) <= tol
    tn = tq / np.linalg.norm(tq)
    assert min(np.abs(quat[0] - tn).max(), np.abs(quat[0] + tn).max()) < 1e-8
    assert abs(np.linalg.norm(q[3:7]) - 1) < 1e-12


def test_rotvec_convention():
    """2 atan2(|v|, w) wrapped to (-pi, pi]; zero vector part gives 0; q and -q give the same rotation."""
    ax = np.array([1.0, 2.0, -2.0]) / 3
    for ang in (0.3, 3.0, -2.5):
        q = np.array([np.cos(ang / 2), *(np.sin(ang / 2) * ax)])
        np.testing.assert_allclose(ir.rotvec(q), ang * ax, atol=1e-14)
        np.testing.assert_allclose(ir.rotvec(-q), ang * ax, atol=1e-14)
    assert not ir.rotvec(np.array([1.0, 0, 0, 0])).any() and not ir.rotvec(np.array([-1.0, 0, 0, 0])).any()


def test_step_clamp_and_dof_mask():
    """One update on the two-link arm: max |delta| is max_step when the raw step is larger, and a
    masked dof's coordinate keeps its bits while the free one does all the work."""
    model, sim = _sim(TWO_LINK)
    site, q0 = [_site(model, "tip")], np.array([0.3, -0.4])
    target = _two_link_tip([1.4, 0.6])[None]
    free, _, _, _ = ir.solve(model, sim, q0, site, target, max_step=10.0, tol=0.0, max_iter=1)
    assert np.abs(free - q0).max() > 0.05
    lim, _, _, _ = ir.solve(model, sim, q0, site, target, max_step=0.05, tol=0.0, max_iter=1)
    assert abs(np.abs(lim - q0).max() - 0.05) < 1e-15
    np.testing.assert_allclose((lim - q0) / 0.05, (free - q0) / np.abs(free - q0).max(), atol=1e-12)  # same direction
    mask = np.array([0, 1], dtype=np.uint8)
    q, _, it, _ = ir.solve(model, sim, q0, site, target, dof_mask=mask, tol=0.0, max_iter=5)
    assert it == 5 and q[0].tobytes() == q0[0].tobytes() and q[1] != q0[1]
    # a masked free joint: translation and quaternion keep their bits even where mj_integratePos
    # would renormalise the quaternion
    fm, fs = _sim(FREE)
    q0 = np.array([0.1, 0.2, 2.0, 0.6, 0.0, 0.8, 1e-9])   # norm 1 + 5e-19: not exactly normalised
    q, _, it, _ = ir.solve(fm, fs, q0, [_site(fm, "s")], np.array([[0.4, -0.3, 1.5]]),
                           dof_mask=np.array([1, 1, 1, 0, 0, 0], dtype=np.uint8), tol=0.0, max_iter=3)
    assert it == 3 and q[3:].tobytes() == q0[3:].tobytes() and np.abs(q[:3] - q0[:3]).max() > 0.01


# ---------------------------------------------------------------- the convergence set
@pytest.mark.parametrize("group", sorted(ir.CONV_GROUPS))
def test_convergence_set_membership(group):
    """The reference alone reaches tol = 1e-6 within half of max_iter = 50 on every env of the
    required groups (a change of seed or of the reference cannot silently empty the set the GPU
    convergence test runs on); the other groups join env by env."""
    cases = ir.convergence_group(group)
    print(group, [(c["ref"][2], c["ref"][3], f"{c['ref'][1]:.2e}", c["member"]) for c in cases])
    assert len(cases) == dr.CASE_N
    for c in cases:
        assert c["member"] == (c["ref"][3] == ir.CONVERGED and c["ref"][2] <= ir.CONV_MAX_ITER // 2)
        if group in ir.CONV_REQUIRED:
            assert c["member"], (group, c["ref"][1:])
            assert c["ref"][1] <= ir.CONV_TOL and c["ref"][2] >= 1   # it had to move to get there
