"""GPU: PhysicsBatch.solve_ilqr / ilqr.solve on the device (fp64): what the acceptance rule promises,
that the result is the rollout of its own controls, and one iteration against the numpy iLQR of
tests/feedback_reference.py driven by the CPU oracle.

No absolute cost is asserted: there is no MuJoCo here to pin one against, and contact-rich
trajectories of the oracle and the device separate (tests/test_gpu_rollout.test_against_oracle).
"""
import functools

import numpy as np
import pytest
import torch

from tests import dyn_reference as dr
from tests import feedback_reference as fb
from tests import fd_reference as fr
from tests import rollout_reference as rr
from tests.helpers import STATE_FIELDS
from tests.test_gpu_rollout import STATE_TENSORS, _batch, _batch_of, _np

pytestmark = pytest.mark.gpu

N = 2
ARM = ("j1_shoulder_pan", "j2_shoulder_tilt", "j3_elbow", "j4_wrist_roll", "j5_wrist_pitch", "j6_wrist_yaw",
       "j7_gripper_base")
ASSEMBLY = dict(horizon=8, nsub=10, max_iter=4)
SOCCER = dict(horizon=6, nsub=1, max_iter=4)


def _two(task):
    model, packed, states, _ = dr.case(task)
    return _batch_of(model, states[:N], "f64", native=_batch(task, "f64").native), model, packed, states


def _assembly_problem(b):
    """The start with the seven arm joints offset by 0.1 rad; weights on the arm's dofs only."""
    m = b.model
    goal = b.get_state()
    w_x = np.zeros(2 * m.nv)
    for name in ARM:
        j = m.name2id("joint", name)
        goal[:, 1 + int(m.jnt_qposadr[j])] += 0.1
        w_x[int(m.jnt_dofadr[j])] = 10.0
        w_x[m.nv + int(m.jnt_dofadr[j])] = 0.01
    return goal.contiguous(), w_x, 10.0 * w_x, np.full(m.nu, 1e-2)


def _soccer_problem(b):
    """The start raised 2 cm in root z."""
    m = b.model
    j = m.name2id("joint", "root_z")  # the humanoid's root is three slides and a hinge
    goal = b.get_state()
    goal[:, 1 + int(m.jnt_qposadr[j])] += 0.02
    w_x = np.concatenate([np.full(m.nv, 1.0), np.full(m.nv, 0.01)])
    w_x[int(m.jnt_dofadr[j])] = 1000.0
    return goal.contiguous(), w_x, 10.0 * w_x, np.full(m.nu, 1e-5)


def _check(b, res, T, nsub, strict):
    torch.cuda.synchronize()
    m = b.model
    hist = _np(res.cost_history)
    print("cost history per env:", hist.T.tolist(), "status", res.status.tolist(), "iters", res.iters.tolist())
    assert res.ctrl.shape == (N, T, m.nu) and res.state.shape == (N, T + 1, b.state_size)
    assert res.gain.shape == (N, T, m.nu, 2 * m.nv) and res.k_ff.shape == (N, T, m.nu)
    assert hist.shape[1] == N and hist.shape[0] == int(res.iters.max()) + 1 and np.isfinite(hist).all()
    assert (hist[1:] <= hist[:-1]).all()  # the acceptance rule
    assert np.array_equal(hist[-1], _np(res.cost))
    if strict:
        assert (hist[-1] < hist[0]).all()  # some step was accepted, and an accepted step lowers the cost
    x0 = b.get_state()
    assert torch.equal(res.state[:, 0], x0)
    # the result is the open-loop rollout of its controls, and the closed-loop one on its own nominal
    again = b.rollout(ctrl=res.ctrl[:, None].contiguous(), nsub=nsub)
    torch.cuda.synchronize()
    assert torch.equal(again.state[:, 0], res.state[:, 1:])
    closed = b.rollout_feedback(res.ctrl.contiguous(), x_nom=res.state[:, :-1].contiguous(), gain=res.gain.contiguous(),
                                nsub=nsub)
    torch.cuda.synchronize()
    assert torch.equal(closed.state[:, 0], res.state[:, 1:]) and torch.equal(closed.ctrl[:, 0], res.ctrl)


@functools.lru_cache(maxsize=None)
def _assembly_solution():
    """The assembly problem solved once on the device, shared by the tests below (read-only)."""
    b, model, packed, states = _two("assembly")
    goal, w_x, w_xf, w_u = _assembly_problem(b)
    before = {f: getattr(b, f).clone() for f in STATE_TENSORS}
    res = b.solve_ilqr(goal, w_x=w_x, w_xf=w_xf, w_u=w_u, **ASSEMBLY)
    torch.cuda.synchronize()
    return b, before, res


def test_assembly_reach():
    b, before, res = _assembly_solution()
    _check(b, res, ASSEMBLY["horizon"], ASSEMBLY["nsub"], strict=True)
    for f in STATE_TENSORS:
        assert torch.equal(before[f], getattr(b, f)), f


def test_soccer_raise_root():
    b, _, _, _ = _two("soccer")
    goal, w_x, w_xf, w_u = _soccer_problem(b)
    before = {f: getattr(b, f).clone() for f in STATE_TENSORS}
    res = b.solve_ilqr(goal, w_x=w_x, w_xf=w_xf, w_u=w_u, **SOCCER)
    _check(b, res, SOCCER["horizon"], SOCCER["nsub"], strict=False)
    for f in STATE_TENSORS:
        assert torch.equal(before[f], getattr(b, f)), f


def test_vector_env_forwards():
    from mujoco_gymnasium_environments_amd.envs.assembly import AssemblyVectorEnv
    env = AssemblyVectorEnv(N, precision="f64")
    env.reset()
    goal, w_x, w_xf, w_u = _assembly_problem(env.batch)
    kw = dict(w_x=w_x, w_xf=w_xf, w_u=w_u, horizon=3, nsub=10, max_iter=1)
    a = env.solve_ilqr(goal, **kw)
    bb = env.batch.solve_ilqr(goal, **kw)
    torch.cuda.synchronize()
    for f in a._fields:
        assert torch.equal(getattr(a, f), getattr(bb, f)), f
    x = env.get_state()
    dx = env.state_difference(env.state_integrate(x, torch.full((N, 2 * env.batch.model.nv), 0.01, dtype=x.dtype, device=x.device)), x)
    assert dx.shape == (N, 2 * env.batch.model.nv) and float((dx - 0.01).abs().max()) < 1e-12
    r = env.physics_rollout_feedback(a.ctrl.contiguous(), nsub=10)
    assert torch.equal(r.state[:, 0], a.state[:, 1:])
    lin = env.transition_fd_along(a.state[:, :-1].contiguous(), a.ctrl.contiguous(), nsub=10)
    assert lin.A.shape[:2] == (N, 3)


def test_first_iteration_against_the_oracle():
    """Env 0 of the assembly problem, one iteration, in numpy on the CPU oracle: the initial cost and
    the sign of the first step's cost change only: on the device that is the first accepted step of
    the problem as test_assembly_reach runs it (its first iterations may be rejected while mu rises:
    the linearisation of this scene's stiff contacts holds over some 1e-6 only). The bound on the initial cost is the rule of
    tests/test_gpu_rollout.test_against_oracle carried to the cost: beside the oracle runs a twin
    whose start qpos is perturbed by 1e-12, and the device is within max(1e-4, 20 x their relative
    spread). 1e-4: state parity of 1e-6 relative against offsets of 0.1 rad in a sum of squares is
    2e-5, with the factor those tests leave. Most of this test's time (about 12 s) is the oracle's
    finite differences: 8 steps x 136 perturbed states x 10 substeps on one CPU core."""
    b, _, dev = _assembly_solution()
    model, packed, states, _ = dr.case("assembly")
    goal, w_x, w_xf, w_u = _assembly_problem(b)
    T, nsub = ASSEMBLY["horizon"], ASSEMBLY["nsub"]
    nq, nv = model.nq, model.nv

    def linearise(x, u, warm):
        st = dict(states[0])
        st.update(qpos=x[1:1 + nq].copy(), qvel=x[1 + nq:].copy(), qacc_warmstart=np.array(warm), ctrl=np.array(u))
        A, B, _, _ = fr.oracle_fd(model, packed, st, nsub=nsub)
        return A, B

    x0 = _np(b.get_state())[0].astype(np.float64)
    hist, _, _ = fb.ilqr(lambda: rr.oracle_sim(packed, states[0]), model, linearise, x0, _np(goal)[0], T, w_x, w_xf, w_u,
                         nsub=nsub, alphas=(1, .5, .25, .125, .0625, .03125, .015625, .0078125), mu=1e-6, iters=1,
                         ctrlrange=np.asarray(model.actuator_ctrlrange).reshape(-1, 2), ctrllimited=model.actuator_ctrllimited)
    got = _np(dev.cost_history)[:, 0]
    x1 = x0.copy()
    x1[1:1 + nq] += np.random.default_rng(0).normal(scale=1e-12, size=nq)
    tw, nd, _, _ = fb.rollout_feedback(lambda: rr.oracle_sim(packed, states[0]), model, T, np.zeros((T, model.nu)),
                                       initial_state=[x1], nsub=nsub)
    twin = fb.quadratic_cost(model, np.concatenate([[x1], tw[0]]), np.zeros((T, model.nu)), _np(goal)[0], w_x, w_xf, w_u)[0]
    spread = abs(twin - hist[0]) / hist[0]
    print(f"oracle twin initial cost {twin:.9g}: relative spread {spread:.3g}")
    print(f"initial cost device {got[0]:.9g} oracle {hist[0]:.9g}; device history {got.tolist()}, oracle after one iteration {hist[1]:.9g}")
    assert abs(got[0] - hist[0]) <= max(1e-4, 20 * spread) * hist[0]
    steps = np.diff(got)
    assert (steps != 0).any(), "no step accepted on the device"
    first = steps[np.flatnonzero(steps)[0]]
    assert (first < 0) == (hist[1] < hist[0]) and first < 0
    assert set(STATE_FIELDS) <= set(states[0])
