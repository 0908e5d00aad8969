"""GPU: PhysicsBatch.solve_ilqr with a sensor-residual cost (fp64) on the martial-arts model: keep
the torso 2 cm higher and as upright as it is, stated on the ``torso_pos`` / ``torso_quat`` sensors.

As tests/test_gpu_ilqr.py, no absolute cost is asserted; what is asserted is what the acceptance
rule promises, that a step is accepted at all, and that the result is the rollout of its own
controls.
"""
import numpy as np
import pytest
import torch

from tests import dyn_reference as dr
from tests.test_gpu_rollout import STATE_TENSORS, _batch, _batch_of, _np

pytestmark = pytest.mark.gpu

N, T, MAX_ITER = 2, 4, 3


def _problem():
    model, _, states, _ = dr.case("martial")
    b = _batch_of(model, states[:N], "f64", native=_batch("martial", "f64").native)
    m = b.model
    sl = b.sensor_slices
    s_goal = b.sensordata().clone()
    s_goal[:, sl["torso_pos"].start + 2] += 0.02
    w_s = np.zeros(int(m.nsensordata))
    w_s[sl["torso_pos"]] = 1000.0
    w_s[sl["torso_quat"]] = 100.0
    kw = dict(w_x=np.concatenate([np.zeros(m.nv), np.full(m.nv, 1e-3)]), w_xf=np.concatenate([np.zeros(m.nv), np.full(m.nv, 1e-2)]),
              w_u=np.full(m.nu, 1e-5), horizon=T, max_iter=MAX_ITER)
    return b, s_goal, w_s, kw


def test_torso_height_and_upright():
    b, s_goal, w_s, kw = _problem()
    m = b.model
    before = {f: getattr(b, f).clone() for f in STATE_TENSORS}
    res = b.solve_ilqr(b.get_state(), sensor_goal=s_goal, w_s=w_s, w_sf=10.0 * w_s, **kw)
    torch.cuda.synchronize()
    hist = _np(res.cost_history)
    print("cost history per env:", hist.T.tolist(), "status", res.status.tolist(), "iters", res.iters.tolist())
    assert res.ctrl.shape == (N, T, m.nu) and res.state.shape == (N, T + 1, b.state_size)
    assert np.isfinite(hist).all() and hist.shape == (int(res.iters.max()) + 1, N)
    assert (hist[1:] <= hist[:-1]).all(), "cost_history is non-increasing"
    assert (np.diff(hist, axis=0) < 0).any(), "a step was accepted"
    assert (hist[-1] < hist[0]).all() and np.array_equal(hist[-1], _np(res.cost))
    assert all(s in (0, 1) for s in res.status.tolist())
    for f in STATE_TENSORS:
        assert torch.equal(before[f], getattr(b, f)), f
    # the result is the rollout of its own controls, and its cost is the one recomputed from that rollout's sensors
    again = b.rollout_feedback(res.ctrl.contiguous(), sensordata=True)
    torch.cuda.synchronize()
    assert torch.equal(again.state[:, 0], res.state[:, 1:]) and torch.equal(again.ctrl[:, 0], res.ctrl)
    r = _np(again.sensordata[:, 0]) - _np(s_goal)[:, None, :]
    xv = _np(res.state)[:, :, 1 + m.nq:] - _np(b.qvel)[:, None, :]  # the state goal is the start
    J = (0.5 * (w_s * r[:, :T - 1] ** 2).sum((1, 2)) + 0.5 * (10.0 * w_s * r[:, T - 1] ** 2).sum(1)
         + 0.5 * (kw["w_x"][m.nv:] * xv[:, :T] ** 2).sum((1, 2)) + 0.5 * (kw["w_xf"][m.nv:] * xv[:, T] ** 2).sum(1)
         + 0.5 * (kw["w_u"] * _np(res.ctrl) ** 2).sum((1, 2)))
    assert np.abs(J - hist[-1]).max() <= 1e-9 * np.abs(J).max(), (J, hist[-1])
    # the goal per step [N, T, ns] and the weights per env [N, ns] mean the same
    res2 = b.solve_ilqr(b.get_state(), sensor_goal=s_goal[:, None, :].repeat(1, T, 1), w_s=torch.tensor(w_s).repeat(N, 1),
                        w_sf=torch.tensor(10.0 * w_s).repeat(N, 1), **kw)
    torch.cuda.synchronize()
    assert torch.equal(res2.ctrl, res.ctrl) and torch.equal(res2.cost_history, res.cost_history)


def test_acceleration_stage_weights_raise():
    b, s_goal, w_s, kw = _problem()
    bad = w_s.copy()
    bad[b.sensor_slices["right_foot_force"]] = 1.0
    for a in (dict(w_s=bad, w_sf=w_s), dict(w_s=w_s, w_sf=bad), dict(w_s=bad)):
        with pytest.raises(ValueError, match="right_foot_force"):
            b.solve_ilqr(b.get_state(), sensor_goal=s_goal, **a, **kw)


def test_without_sensor_arguments_nothing_changes():
    b, _, _, kw = _problem()
    goal = b.get_state()
    goal[:, 1 + 2] += 0.02
    kw = dict(kw, w_x=np.concatenate([np.full(b.model.nv, 10.0), np.full(b.model.nv, 1e-3)]))
    a = b.solve_ilqr(goal, **kw)
    torch.cuda.synchronize()
    a = {f: getattr(a, f).clone() for f in a._fields}
    c = b.solve_ilqr(goal, sensor_goal=None, w_s=None, w_sf=None, **kw)
    torch.cuda.synchronize()
    for f, x in a.items():
        assert torch.equal(x, getattr(c, f)), f
    assert getattr(b, "_sensor_fd_along", None) is None, "no sensor code ran"
