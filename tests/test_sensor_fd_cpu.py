"""CPU: tests/sensor_fd_reference.py (the numpy reference the GPU sensor-derivative tests compare
with) against known answers on the CPU oracle alone; cabi.MgxSensorFdIO against include/mgx.h; and
the sensor-residual cost of ilqr.solve on a linear stand-in system.

Known answers, eps = 1e-6:
* the slide model of tests/test_fd_cpu.py with a jointpos and a jointvel sensor: C is the 2 x 2
  identity and D is 0 (bar: the rounding floor of tests/test_fd_cpu.py, 1e-8);
* on martial and soccer the [:, :nv] block of a body framepos sensor's rows, and the [:, nv:] block
  of a body framelinvel's, are jacp of the body's inertial frame (mj_jacBodyCom,
  dyn_reference.jac). Centred, at the known-answer bar of DESIGN §10, 100 u max(1, |s|inf) / eps
  with u = 2^-53: both sides round the sensor within tens of ulp and the difference divides that
  by eps;
* D is exactly 0 on every position- and velocity-stage row (they do not read ctrl), and nonzero on
  the force / torque / accelerometer rows of martial and bipedal.
"""
import types

import numpy as np
import pytest
import torch

from mujoco_gymnasium_environments_amd import cabi, ilqr, mjcf
from tests import dyn_reference as dr
from tests import fd_reference as fr
from tests import sensor_fd_reference as sfr
from tests import sensor_reference as sr
from tests.test_fd_cpu import TOL
from tests.test_ilqr_cpu import NU, NX, LinearSystem, N, T, _problem, _system_matrices

U64, EPS = 2.0 ** -53, 1e-6
SLIDE_SENSORS = fr.SLIDE.format(integrator="").replace(
    "</mujoco>", '<sensor><jointpos name="p" joint="x"/><jointvel name="v" joint="x"/></sensor></mujoco>')


# ---------------------------------------------------------------- C-ABI
def test_header_matches_ctypes(tmp_path):
    """mgx_sensor_fd_io of include/mgx.h against cabi.py; the ABI version is unchanged (the section
    only adds)."""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in cabi.MgxSensorFdIO._fields_]
    assert fields == ["eps", "flags", "slots", "C", "D", "sensordata", "workspace", "workspace_bytes"]
    prog = tmp_path / "sensor_fd.c"
    offs = "".join(f' printf("%zu ", offsetof(mgx_sensor_fd_io, {f}));' for f in fields)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
                    'int main(void){printf("%zu ", sizeof(mgx_sensor_fd_io));' + offs +
                    ' printf("%d %d\\n", MGX_FD_CENTERED, MGX_ABI_VERSION); return 0;}\n')
    exe = tmp_path / "sensor_fd"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(cabi.MgxSensorFdIO)] + [getattr(cabi.MgxSensorFdIO, f).offset for f in fields]
    assert vals == want + [cabi.MGX_FD_CENTERED, 6] and cabi.MGX_ABI_VERSION == 6
    from mujoco_gymnasium_environments_amd import native
    assert "mgx_sensor_fd" in native.EXPORTS and "mgx_sensor_fd_bytes" in native.EXPORTS
    assert "mgx_sensor.h" in native.TU_HEADERS["mgx_fd.hip"]


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("centered", [False, True], ids=["forward", "centered"])
def test_slide_identity(centered):
    from oracle.mjref import RefSim
    from tests.helpers import STATE_FIELDS
    model = mjcf.compile_xml(SLIDE_SENSORS)
    packed = cabi.pack_model(model)
    s = RefSim(packed)
    s.qpos[0], s.qvel[0], s.ctrl[0] = fr.SLIDE_STATE
    state = {f: s.field(f).copy() for f in STATE_FIELDS}
    C, D, row = sfr.oracle_sensor_fd(model, packed, state, eps=EPS, centered=centered)
    assert C.shape == (2, 2) and D.shape == (2, 1)
    assert list(row) == [fr.SLIDE_STATE[0], fr.SLIDE_STATE[1]]
    assert np.abs(C - np.eye(2)).max() <= TOL and not D.any()
    # without D the ctrl columns take no part and C is the same
    C2, D2, _ = sfr.oracle_sensor_fd(model, packed, state, eps=EPS, centered=centered, with_d=False)
    assert D2 is None and np.array_equal(C, C2)
    states, steps = sfr.virtual_states(model, state, EPS, centered, with_d=False)
    assert len(states) == 1 + (4 if centered else 2) and [k for k, _ in steps] == [0, 1] * (2 if centered else 1)


def _body_frame_rows(model):
    """[(sensor name, slice of its rows, body, 'pos' | 'vel')] of the framepos / framelinvel sensors
    whose object is a body's inertial frame."""
    out = []
    for i, name in enumerate(model.sensor_names):
        t, ot = int(model.sensor_type[i]), int(model.sensor_objtype[i])
        if ot == sr.BODY and t in (sr.T["framepos"], sr.T["framelinvel"]):
            a = int(model.sensor_adr[i])
            out.append((name, slice(a, a + 3), int(model.sensor_objid[i]), "pos" if t == sr.T["framepos"] else "vel"))
    return out


@pytest.mark.parametrize("task", ["martial", "soccer"])
def test_frame_rows_are_the_body_com_jacobian(task):
    model, packed, states, F = sr.oracle_case(task)
    nv = model.nv
    rows = _body_frame_rows(model)
    assert {k for _, _, _, k in rows} == ({"pos", "vel"} if task == "martial" else {"pos"})
    worst = 0.0
    for e, st in enumerate(states):
        C, _, s0 = sfr.oracle_sensor_fd(model, packed, st, eps=EPS, centered=True, with_d=False)
        assert C.shape == (model.nsensordata, 2 * nv)
        for name, sl, body, kind in rows:
            bar = 100 * U64 * max(1.0, float(np.abs(s0[sl]).max())) / EPS
            jp = dr.jac(model, F[e], dr.BODYCOM, body)[0]
            got = C[sl, :nv] if kind == "pos" else C[sl, nv:]
            err = float(np.abs(got - jp).max())
            worst = max(worst, err)
            print(f"{task} env {e} {name}: |C - jacp| {err:.3g} (bar {bar:.3g})")
            assert err <= bar, (name, err, bar)
            if kind == "pos":
                assert not C[sl, nv:].any(), "a position does not depend on qvel"
    assert worst > 0


@pytest.mark.parametrize("task", ["martial", "bipedal", "soccer"])
def test_d_is_zero_below_the_acceleration_stage(task):
    model, packed, states, _ = sr.oracle_case(task)
    acc = np.zeros(int(model.nsensordata), dtype=bool)
    for i, on in enumerate(sr.acc_stage(model)):
        acc[int(model.sensor_adr[i]):int(model.sensor_adr[i]) + int(model.sensor_dim[i])] = on
    dmax = 0.0
    for st in states:
        _, D, _ = sfr.oracle_sensor_fd(model, packed, st, eps=EPS, centered=False)
        assert D.shape == (model.nsensordata, model.nu)
        assert not D[~acc].any(), "position- and velocity-stage sensors do not read ctrl"
        dmax = max(dmax, float(np.abs(D[acc]).max(initial=0.0)))
    print(f"{task}: |D|max on acceleration-stage rows {dmax:.3g}")
    assert (dmax > 0) == (task != "soccer")


# ---------------------------------------------------------------- iLQR with a sensor residual
NS = NX + 1  # s_i = 2 x_i, and one row of an acceleration-stage sensor that may not be weighted


class SensorLinearSystem(LinearSystem):
    """LinearSystem with sensors s = H x, H = [2 I; 1'], and an exact sensor_fd_along."""

    def __init__(self, A, B):
        super().__init__(A, B)
        self.H = torch.cat([2.0 * torch.eye(NX, dtype=torch.float64), torch.ones(1, NX, dtype=torch.float64)])
        self.model = types.SimpleNamespace(
            nv=NX // 2, nu=NU, nsensordata=NS, sensor_names=["pos", "accel"],
            sensor_type=[mjcf.SENSOR_TYPES.index("framepos"), mjcf.SENSOR_TYPES.index("accelerometer")],
            sensor_adr=[0, NX], sensor_dim=[NX, 1])
        self.sensor_calls = 0

    def sensor_fd_along(self, state0, ctrl, centered=False, only=None):
        assert tuple(only) == ("C",) and state0.shape[:2] == (N, T)
        self.sensor_calls += 1
        return types.SimpleNamespace(C=self.H.expand(N, T, NS, NX), D=None, sensordata=None)

    def rollout_feedback(self, u_nom, sensordata=False, **kw):
        r = super().rollout_feedback(u_nom, **kw)
        r.sensordata = r.state[..., 1:] @ self.H.T if sensordata else None
        return r


def test_sensor_cost_reproduces_the_state_cost():
    """s_i = 2 x_i: the sensor cost w_s is the state cost w_x = 4 w_s (the x_0 term of the state cost
    is a constant). One iteration of either is the exact LQR optimum of tests/test_ilqr_cpu.py."""
    A, B = _system_matrices(1)
    x0, goal, (w_x, w_xf, w_u) = _problem()
    zeros = np.zeros(NX)
    pad = lambda w: np.concatenate([w, [0.0]])  # noqa: E731
    s_goal = torch.cat([2.0 * torch.tensor(goal[:, 1:]), torch.zeros(N, 1, dtype=torch.float64)], dim=1)
    plain = ilqr.solve(LinearSystem(A, B), ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u),
                       alphas=(1,), mu0=0.0, max_iter=1)
    sys = SensorLinearSystem(A, B)
    prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, zeros, zeros, w_u, sensor_goal=s_goal,
                            w_s=pad(w_x / 4), w_sf=pad(w_xf / 4))
    got = ilqr.solve(sys, prob, alphas=(1,), mu0=0.0, max_iter=1)
    assert sys.sensor_calls == 1
    const = 0.5 * (w_x * (x0[:, 1:] - goal[:, 1:]) ** 2).sum(1)  # the x_0 term the sensor cost leaves out
    for e in range(N):
        u = plain.ctrl[e].numpy()
        assert np.abs(got.ctrl[e].numpy() - u).max() <= 1e-9 * max(1.0, np.abs(u).max())
        assert abs(float(got.cost[e]) + const[e] - float(plain.cost[e])) <= 1e-9 * float(plain.cost[e])
        assert float(got.cost_history[1, e]) < float(got.cost_history[0, e])
    # the goal as [N, T, ns] and the weights as [N, ns] mean the same
    prob2 = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, zeros, zeros, w_u,
                             sensor_goal=s_goal[:, None, :].repeat(1, T, 1), w_s=torch.tensor(pad(w_x / 4)).repeat(N, 1),
                             w_sf=torch.tensor(pad(w_xf / 4)).repeat(N, 1))
    got2 = ilqr.solve(SensorLinearSystem(A, B), prob2, alphas=(1,), mu0=0.0, max_iter=1)
    assert torch.equal(got2.ctrl, got.ctrl) and torch.equal(got2.cost, got.cost)


def test_sensor_cost_refuses_acceleration_stage_rows():
    A, B = _system_matrices(1)
    x0, goal, (w_x, w_xf, w_u) = _problem()
    zeros = np.zeros(NX)
    bad = np.zeros(NS)
    bad[NX] = 1.0
    for kw in (dict(w_s=bad), dict(w_sf=bad), dict(w_s=np.zeros(NS), w_sf=torch.tensor(bad).repeat(N, 1))):
        prob = ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, zeros, zeros, w_u,
                                sensor_goal=torch.zeros(N, NS, dtype=torch.float64), **kw)
        with pytest.raises(ValueError, match="accel"):
            ilqr.solve(SensorLinearSystem(A, B), prob, alphas=(1,), mu0=0.0, max_iter=1)
    with pytest.raises(ValueError, match="sensor_goal"):
        ilqr.solve(SensorLinearSystem(A, B), ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, zeros, zeros, w_u,
                                                              w_s=np.zeros(NS)), max_iter=1)


def test_none_arguments_change_nothing():
    A, B = _system_matrices(1)
    x0, goal, (w_x, w_xf, w_u) = _problem()
    a = ilqr.solve(LinearSystem(A, B), ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u), max_iter=3)
    sys = SensorLinearSystem(A, B)
    b = ilqr.solve(sys, ilqr.IlqrProblem(torch.tensor(x0), torch.tensor(goal), T, w_x, w_xf, w_u, sensor_goal=None,
                                         w_s=None, w_sf=None), max_iter=3)
    assert sys.sensor_calls == 0
    for f in ilqr.IlqrResult._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
