"""GPU: mgx_rollout (PhysicsBatch.rollout) against the hand-built composition it replaces, against
the batch's own step, and against the CPU oracle (tests/rollout_reference.py).

Setup (dyn_reference.case): N = 3 envs per task at the oracle states of tests/test_gpu_dyn.py, K = 3
rollouts of T = 4 recorded steps, all seven task models, fp64 and fp32.

1. The hand-built composition: a second PhysicsBatch of N K envs, a Python loop of "write ctrl,
   step(nsub, frames=False), read" (and sensordata() on soccer and bipedal), with the header's
   stop-and-pad rule applied on the host. On the six models with nv <= 64 state, sensordata and
   n_done must be BIT-EQUAL: the same step kernel runs on the same inputs, one wave per env without
   atomics, and the record kernel only copies. humanoid_construction runs the two-wave wide kernel,
   for which DESIGN §6 records an unexplained intermittent bit difference: the composition is built
   twice in separately allocated batches and the bound is
       max(16 x their spread, 64 u_T max(1, |x|inf)),   u_T = 2^-53 | 2^-24
   (the spread is printed; DESIGN §11 records the measured value).
2. K = 1, T = 1, every input NULL: the batch's state after its own step(), bit for bit.
3. Divergence on fd_reference.TWO_ACT, 4. the oracle (fp64, soccer and bipedal: indexing and order;
   the tolerance of those tasks' multi-step parity tests), 5. chunking, 6. behaviour.
"""
import functools

import numpy as np
import pytest
import torch

from mujoco_gymnasium_environments_amd import cabi, mjcf
from tests import dyn_reference as dr
from tests import fd_reference as fr
from tests import rollout_reference as rr
from tests.helpers import STATE_FIELDS, load_states

pytestmark = pytest.mark.gpu

N, K, T = dr.CASE_N, 3, 4
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
STATE_TENSORS = STATE_FIELDS + ("time", "warning", "overflow")
SENSOR_TASKS = ("soccer", "bipedal")


def _np(t):
    return t.detach().cpu().numpy()


def _batch_of(model, states, prec, native=None):
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
    b = PhysicsBatch(model, len(states), precision=prec, native=native)
    load_states(b, states)
    return b


def _new_batch(task, prec):
    model, _, states, _ = dr.case(task)
    return _batch_of(model, states, prec, native=_batch(task, prec).native)


@functools.lru_cache(maxsize=None)
def _batch(task, prec):
    """Shared batch at the oracle states; rollout does not write to it (test_state_untouched)."""
    model, _, states, _ = dr.case(task)
    return _batch_of(model, states, prec)


def _get(res):
    torch.cuda.synchronize()
    return {f: None if getattr(res, f) is None else _np(getattr(res, f)).copy() for f in ("state", "sensordata", "n_done")}


def _inputs(b, task, variant, hold, seed=0):
    """Keyword arguments of one rollout call (device tensors in the batch dtype).
    'plain': ctrl [N, K, knots, nu], every other input NULL; 'given': initial_state and
    initial_warmstart rows that differ per rollout, and a ctrl schedule shared by the envs."""
    m = b.model
    scale = dr.CASES[task][1] if task in dr.CASES else 1.0
    g = torch.Generator(device="cpu").manual_seed(seed)
    knots = rr.n_knots(T, hold)
    shared = variant == "given"
    shape = (K, knots, m.nu) if shared else (N, K, knots, m.nu)
    kw = dict(ctrl=((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(b.dtype).to(b.device).contiguous(),
              hold=hold, shared_ctrl=shared)
    if variant == "given":
        f = torch.arange(K, dtype=b.dtype, device=b.device)
        x = b.get_state()[:, None, :].repeat(1, K, 1)
        x[:, :, 0] = 0.5 + f                                 # time
        x[:, :, 1 + m.nq:] *= (1.0 + 0.125 * f)[None, :, None]  # qvel
        kw["initial_state"] = x.contiguous()
        kw["initial_warmstart"] = (b.qacc_warmstart[:, None, :] * (0.5 + f)[None, :, None]).contiguous()
    return kw


def hand_built(b, kw, nsub=1, sensors=False):
    """The composition the call replaces: the N K virtual envs in one PhysicsBatch (separately
    allocated), stepped in a Python loop with the existing step(); the stop-and-pad rule on the host.
    Returns state, sensordata, n_done as the call lays them out, and warned [N, K, T]."""
    m = b.model
    big = _batch_of(m, [_state_of(b, i) for i in range(N) for _ in range(K)],
                    "f64" if b.dtype == torch.float64 else "f32", native=b.native)
    big.time.copy_(b.time.repeat_interleave(K))
    if kw.get("initial_state") is not None:
        big.set_state(kw["initial_state"].reshape(N * K, -1))
    if kw.get("initial_warmstart") is not None:
        big.qacc_warmstart.copy_(kw["initial_warmstart"].reshape(N * K, -1))
    ctrl, hold = kw.get("ctrl"), kw.get("hold", 1)
    if ctrl is not None and kw.get("shared_ctrl"):
        ctrl = ctrl[None].expand(N, *ctrl.shape)
    rows, sens, warn = [], [], [np.zeros(N * K, dtype=np.int32)]
    for t in range(T):
        if ctrl is not None:
            big.ctrl[:, :m.nu] = ctrl[:, :, t // hold, :].reshape(N * K, m.nu)
        big.step(nsub, frames=False)
        rows.append(_np(big.get_state()))
        if sensors:
            sens.append(_np(big.sensordata()).copy())
        torch.cuda.synchronize()
        warn.append(_np(big.warning).copy())
    state = np.stack(rows, axis=1)                   # [NK, T, nstate]
    sd = np.stack(sens, axis=1) if sensors else None
    warned = np.diff(np.stack(warn, axis=1), axis=1) > 0  # [NK, T]
    n_done = np.full(N * K, T, dtype=np.int32)
    for v in range(N * K):
        hit = np.flatnonzero(warned[v])
        if hit.size:
            t = int(hit[0])
            n_done[v] = t
            state[v, t:] = state[v, t]
            if sensors:
                sd[v, t:] = sd[v, t]
            warned[v, t + 1:] = False
    shape = lambda a: None if a is None else a.reshape((N, K) + a.shape[1:])  # noqa: E731
    return {"state": shape(state), "sensordata": shape(sd), "n_done": shape(n_done), "warned": shape(warned)}


def _state_of(b, i):
    """Env i of a batch as a tests.helpers state dict (exact: the values are the batch dtype's)."""
    return {f: _np(getattr(b, f)[i]).astype(np.float64).reshape(-1) for f in STATE_FIELDS}


def _compare(task, prec, got, ref, label, twin=None):
    """Bit-equal for nv <= 64; the two-wave kernel's bound from its own spread (`twin`)."""
    assert np.array_equal(got["n_done"], ref["n_done"]), (label, got["n_done"], ref["n_done"])
    for f in ("state", "sensordata"):
        if ref[f] is None:
            continue
        assert got[f] is not None and got[f].shape == ref[f].shape and np.isfinite(got[f]).all(), (label, f)
        if twin is None:
            nbad = int((got[f] != ref[f]).sum())
            assert nbad == 0, f"{label}: {nbad} entries of {f} differ from the hand-built composition"
        else:
            spread = float(np.abs(ref[f].astype(np.float64) - twin[f].astype(np.float64)).max())
            bound = max(16 * spread, 64 * U[prec] * max(1.0, float(np.abs(ref[f]).max())))
            err = float(np.abs(got[f].astype(np.float64) - ref[f].astype(np.float64)).max())
            print(f"{label}: {f} spread of two hand-built compositions {spread:.3g}, |rollout - hand-built| {err:.3g} "
                  f"(bound {bound:.3g})")
            assert err <= bound, (label, f, err, bound)


# ------------------------------------------------------------------ 1. the hand-built composition
@pytest.mark.parametrize("variant,hold", [("plain", 1), ("given", 2)], ids=["ctrl-only", "given-shared-hold2"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("task", dr.TASKS)
def test_equals_hand_built_composition(task, prec, variant, hold):
    b = _batch(task, prec)
    m = b.model
    sensors = task in SENSOR_TASKS
    kw = _inputs(b, task, variant, hold)
    got = _get(b.rollout(sensordata=sensors, **kw))
    assert got["state"].shape == (N, K, T, 1 + m.nq + m.nv) and b.state_size == 1 + m.nq + m.nv
    assert got["n_done"].shape == (N, K) and (got["sensordata"] is not None) == sensors
    ref = hand_built(b, kw, sensors=sensors)
    twin = hand_built(b, kw, sensors=sensors) if m.nv > 64 else None
    _compare(task, prec, got, ref, f"{task}-{prec}-{variant}", twin)
    if sensors:
        assert got["sensordata"].shape == (N, K, T, m.nsensordata) and np.abs(got["sensordata"]).max() > 0


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_equals_hand_built_composition_nsub10(prec):
    """The physics of one parkour env step per recorded step: 10 substeps."""
    b = _batch("parkour", prec)
    kw = _inputs(b, "parkour", "plain", 1, seed=1)
    got = _get(b.rollout(nsub=10, **kw))
    _compare("parkour", prec, got, hand_built(b, kw, nsub=10), f"parkour-{prec}-nsub10")


# ------------------------------------------------------------------ 2. the env's own step
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("task", [t for t in dr.TASKS if t != "construction"])
def test_one_step_equals_own_step(task, prec):
    b = _new_batch(task, prec)
    res = b.rollout(nstep=1)
    got = _get(res)
    assert got["state"].shape[:3] == (N, 1, 1) and (got["n_done"] == 1).all() and res.sensordata is None
    b.step()
    torch.cuda.synchronize()
    assert np.array_equal(got["state"][:, 0, 0], _np(b.get_state()))


# ------------------------------------------------------------------ 3. divergence
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_divergence_stops_and_pads(prec):
    """Rollout 0 starts at qvel[0] = 2e10 (mj_checkVel), rollout 1 gets ctrl = 1e16 on the unlimited
    motor at step 2 (mj_checkAcc), rollout 2 is undisturbed. The hand-built composition first shows
    that `warning` rises at exactly those steps: the documented auto-reset, no fault."""
    model = mjcf.compile_xml(fr.TWO_ACT)
    st = {f: np.zeros(n) for f, n in zip(STATE_FIELDS, (2, 2, 2, 2, 2, 6 * model.nbody))}
    st["qpos"][:] = [0.3, -0.5]
    st["qvel"][:] = [0.2, 0.1]
    b = _batch_of(model, [st] * N, prec)
    ctrl = torch.tensor([0.25, 0.7], dtype=b.dtype, device=b.device).repeat(N, K, T, 1)
    ctrl[:, 1, 2, 1] = 1e16
    x = b.get_state()[:, None, :].repeat(1, K, 1)
    x[:, 0, 1 + model.nq] = 2e10
    kw = dict(ctrl=ctrl.contiguous(), initial_state=x.contiguous(), hold=1)
    ref = hand_built(b, kw)
    want = np.zeros((N, K, T), dtype=bool)
    want[:, 0, 0] = True
    want[:, 1, 2] = True
    assert np.array_equal(ref["warned"], want), ref["warned"]
    got = _get(b.rollout(**kw))
    assert got["n_done"].tolist() == [[0, 2, 4]] * N
    s = got["state"]
    assert np.isfinite(s).all()
    for t in range(1, T):
        assert np.array_equal(s[:, 0, t], s[:, 0, 0])          # padded from the first step on
    assert np.array_equal(s[:, 1, :2], s[:, 2, :2])            # the same controls until step 2
    assert np.array_equal(s[:, 1, 3], s[:, 1, 2]) and not np.array_equal(s[:, 1, 2], s[:, 2, 2])
    assert np.array_equal(s, ref["state"])                     # rows 2-3: what step 2 left behind


# ------------------------------------------------------------------ 4. the oracle
def _rel_err(x, ref):
    """max difference of [qpos, qvel] relative to max(1, |x|), as tests/test_gpu_soccer._state_err"""
    return float(np.max(np.abs(x[1:] - ref[1:]) / np.maximum(1.0, np.abs(ref[1:]))))


@pytest.mark.parametrize("task", SENSOR_TASKS)
def test_against_oracle(task):
    """The rule of test_vector_env_end_to_end_f64_bench_actions (tests/test_gpu_soccer.py,
    tests/test_gpu_bipedal.py): beside the oracle run a twin with qpos perturbed by 1e-12 and one
    summing the PGS residuals in reverse; while their spread is <= 1e-6 the device is within
    max(1e-6, 20 x spread). Step parity is those tests' job; this one is for indexing and order, so
    every rollout must be compared on its first row at least and half of all rows overall."""
    model, packed, states, _ = dr.case(task)
    b = _batch(task, "f64")
    kw = _inputs(b, task, "given", 2, seed=2)
    got = _get(b.rollout(**kw))
    ctrl = _np(kw["ctrl"]).astype(np.float64)
    x0, w0 = _np(kw["initial_state"]), _np(kw["initial_warmstart"])
    compared, worst = np.zeros((N, K), dtype=int), 0.0
    for i in range(N):
        args = dict(ctrl=ctrl, hold=2, initial_warmstart=w0[i])
        ref, done, _ = rr.oracle_rollout(model, packed, states[i], T, initial_state=x0[i], **args)
        x1 = x0[i].copy()
        x1[:, 1:1 + model.nq] += np.random.default_rng(i).normal(scale=1e-12, size=(K, model.nq))
        tw1, _, _ = rr.oracle_rollout(model, packed, states[i], T, initial_state=x1, **args)

        def reverse_sim(i=i):
            sim = rr.oracle_sim(packed, states[i])
            sim.set_pgs_reverse(True)
            return sim
        tw2, _, _ = rr.rollout(reverse_sim, model.nq, model.nv, model.nu, T, initial_state=x0[i], **args)
        assert list(done) == [T] * K and got["n_done"][i].tolist() == [T] * K
        for k in range(K):
            for t in range(T):
                assert abs(got["state"][i, k, t, 0] - ref[k, t, 0]) <= 1e-12  # time
                spread = max(_rel_err(tw1[k, t], ref[k, t]), _rel_err(tw2[k, t], ref[k, t]))
                if spread > 1e-6:
                    break
                err = _rel_err(got["state"][i, k, t], ref[k, t])
                assert err <= max(1e-6, 20 * spread), (i, k, t, err, spread)
                compared[i, k] += 1
                worst = max(worst, err)
    print(f"{task}: rows compared per rollout {compared.tolist()}, worst device error {worst:.3g}")
    assert compared.min() >= 1 and compared.sum() >= N * K * T // 2


# ------------------------------------------------------------------ 5. chunking
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("task", SENSOR_TASKS)
def test_chunking(task, prec):
    """slots = 4 over 9 virtual envs: three passes, the last partial, against one pass."""
    b = _batch(task, prec)
    kw = _inputs(b, task, "given", 2, seed=3)
    one = _get(b.rollout(sensordata=True, slots=N * K, **kw))
    three = _get(b.rollout(sensordata=True, slots=4, **kw))
    for f in one:
        assert np.array_equal(one[f], three[f]), f
    with pytest.raises(Exception) as ei:
        b.rollout(slots=0, **kw)
    assert getattr(ei.value, "code", None) == cabi.MGX_E_ARG


# ------------------------------------------------------------------ 6. behaviour
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_state_untouched_and_repeatable(prec):
    b = _new_batch("soccer", prec)
    b.warning.fill_(3)
    b.overflow.fill_(2)
    b.time.fill_(0.5)
    before = {f: getattr(b, f).clone() for f in STATE_TENSORS}
    kw = _inputs(b, "soccer", "plain", 1, seed=4)
    first = _get(b.rollout(sensordata=True, **kw))
    second = _get(b.rollout(sensordata=True, **kw))
    for f in STATE_TENSORS:
        assert torch.equal(before[f], getattr(b, f)), f
    for f in first:
        assert np.array_equal(first[f], second[f]), f
    # U(+-150) controls may drive a rollout into the bad-state reset: whatever happens is what the
    # composition does from the same (time 0.5) state
    assert np.isfinite(first["state"]).all()
    _compare("soccer", prec, first, hand_built(b, kw, sensors=True), f"soccer-{prec}-repeat")
    assert (first["state"][:, :, 0, 0] > 0.5).all()  # the rollout's clock starts at the env's time
    only = b.rollout(only=("n_done",), **kw)
    assert only.state is None and only.sensordata is None
    assert np.array_equal(_get(only)["n_done"], first["n_done"])
    with pytest.raises(KeyError):
        b.rollout(only=("qacc",), **kw)


@pytest.mark.parametrize("task", SENSOR_TASKS)
def test_workspace_contents_do_not_matter(task):
    """NaN- and zero-prefilled workspaces (solver scratch included, on bipedal) give the same bits."""
    b = _new_batch(task, "f64")
    kw = _inputs(b, task, "plain", 1, seed=5)
    b.rollout(sensordata=True, **kw)
    (ws,) = b._rollout_ws.values()
    out = []
    for fill in (0, 0xFF):
        ws.fill_(fill)  # 0xFF bytes: NaN reals, -1 counters, nonzero live flags
        out.append(_get(b.rollout(sensordata=True, **kw)))
    for f in out[0]:
        assert np.array_equal(out[0][f], out[1][f]), f
    assert np.isfinite(out[0]["state"]).all() and np.isfinite(out[0]["sensordata"]).all()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_mask_keeps_rows(prec):
    from mujoco_gymnasium_environments_amd.rollouts import alloc_rollout
    b = _batch("soccer", prec)
    m = b.model
    kw = _inputs(b, "soccer", "plain", 1, seed=6)
    full = _get(b.rollout(sensordata=True, **kw))
    out = alloc_rollout(N, K, T, b.state_size, m.nsensordata, b.dtype, b.device)
    out.state.fill_(float("nan"))
    out.sensordata.fill_(float("nan"))
    out.n_done.fill_(-7)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=b.device)
    got = _get(b.rollout(sensordata=True, mask=mask, out=out, **kw))
    for f in ("state", "sensordata"):
        assert np.isnan(got[f][1]).all(), f
        assert np.array_equal(got[f][[0, 2]], full[f][[0, 2]]), f
    assert np.array_equal(got["n_done"][[0, 2]], full["n_done"][[0, 2]]) and got["n_done"][1].tolist() == [-7] * K


def test_get_set_state_round_trip():
    b = _new_batch("soccer", "f64")
    m = b.model
    x = b.get_state()
    assert x.shape == (N, 1 + m.nq + m.nv) and torch.equal(x[:, 0], b.time) and torch.equal(x[:, 1:1 + m.nq], b.qpos)
    y = (x * 1.5 + 0.25).contiguous()
    warm = b.qacc_warmstart.clone()
    b.set_state(y, mask=torch.tensor([0, 1, 0], dtype=torch.uint8, device=b.device))
    z = b.get_state()
    assert torch.equal(z[1], y[1]) and torch.equal(z[[0, 2]], x[[0, 2]])
    b.set_state(y)
    assert torch.equal(b.get_state(), y) and torch.equal(b.qacc_warmstart, warm)


def test_vector_env_forwards_and_errors():
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv, StreamShardedSoccerEnv
    env = SoccerVectorEnv(4, precision="f64", seed=11)
    many = StreamShardedSoccerEnv(4, n_streams=2, precision="f64", seed=11)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    for e in (env, many):
        e.reset()
    for _ in range(2):
        act = (torch.rand(4, 33, device="cuda:0", generator=g) * 300 - 150).contiguous()
        env.step(act)
        many.step(act)
    nu = env.batch.model.nu
    ctrl = ((torch.rand(4, K, T, nu, device="cuda:0", generator=g, dtype=torch.float64) * 2 - 1) * 150).contiguous()
    kw = dict(ctrl=ctrl, sensordata=True)
    a, bb, c = _get(env.physics_rollout(**kw)), _get(env.batch.rollout(**kw)), _get(many.physics_rollout(**kw))
    for f in a:
        assert np.array_equal(a[f], bb[f]) and np.array_equal(a[f], c[f]), f
    assert a["state"].shape == (4, K, T, env.state_size) and np.isfinite(a["state"]).all()
    assert torch.equal(many.get_state(), env.get_state())
    assert env.rollout.shape == (4, 8)  # the env's episode sums keep their name
    for bad in (dict(nsub=0), dict(hold=0), dict(slots=0), dict(nstep=0, ctrl=None)):
        with pytest.raises(Exception) as ei:
            env.physics_rollout(**{**kw, **bad})
        assert getattr(ei.value, "code", None) == cabi.MGX_E_ARG, bad
    with pytest.raises(ValueError):
        env.physics_rollout(sensordata=True)  # neither ctrl nor nstep
    with pytest.raises(ValueError):
        env.physics_rollout(ctrl=ctrl, nstep=T + 1)  # the knots do not cover T + 1 steps


def test_construction_sensordata_is_unsupported():
    b = _batch("construction", "f64")
    with pytest.raises(Exception) as ei:
        b.rollout(nstep=1, sensordata=True)
    assert getattr(ei.value, "code", None) == cabi.MGX_E_UNSUPPORTED
