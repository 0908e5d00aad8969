"""GPU: the fused bipedal_rescue kernel (one RK4 mj_step + env logic) against the reference
golden vectors and the CPU oracle (mjref physics + oracle/bipedal_logic.py).

Bars: logic kernel fp64 — obs, reward, flags, ctrl, victim masks, energy, the persisting
_prev_* / _fall_timer attributes and the stats bit-exact against the reference's own step()
outputs (2-D distances use numpy's FMA dot, energy numpy's float32 pairwise sum); fp32 —
obs atol 2e-5, reward rtol 1e-6 (+inf where the reference has +inf), flags exact.
End-to-end fp64 (reset with numpy-seeded draws + 10 settle steps, then 15 steps) on the
trajectories where the oracle itself is well-conditioned (see _well_conditioned): obs atol
1e-5, reward atol 1e-3 (identical where infinite) and identical terminated/truncated flags.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _t(x, dtype, dev="cuda:0"):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dtype).contiguous()


def _mask(rows):
    return np.array([sum(1 << int(v) for v in r if v >= 0) for r in rows], dtype=np.int32)


@pytest.mark.parametrize("prec", ["f64", "f32", "f64_actions"])
def test_bipedal_logic_kernel_matches_reference(bipedal_model, prec):
    from mujoco_gymnasium_environments_amd import cabi
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.native import check, lib
    # f64_actions: the fp64 kernel on the float64-action vectors (make_fixtures.py main_f64),
    # mgx_bipedal_env.action_f64 = 1 — the reference keeps a float64 action float64 through np.clip
    act64 = prec == "f64_actions"
    prec = "f64" if act64 else prec
    g = dict(np.load("tests/golden/bipedal_envlogic" + ("_f64" if act64 else "") + ".npz"))
    n = g["obs"].shape[0]
    env = BipedalVectorEnv(n, precision=prec, autoreset=False)
    dt = env.batch.dtype
    env.step_count.copy_(_t(g["current_step_in"], torch.int32))
    env.energy.copy_(_t(g["energy_in"], torch.float32))
    env.rescued.copy_(_t(_mask(g["rescued_in"]), torch.int32))
    env.carried.copy_(_t(_mask(g["carried_in"]), torch.int32))
    env.carrying.copy_(_t(g["carrying_in"], torch.uint8))
    env.closest.copy_(_t(g["closest_in"], torch.float64))
    env.prev_rescued.copy_(_t(g["prev_rescued_in"], torch.int32))
    env.prev_carried.copy_(_t(g["prev_carried_in"], torch.int32))
    env.prev_sz.copy_(_t(g["prev_sz_in"], torch.float64))
    env.fall_timer.copy_(_t(g["fall_timer_in"], torch.int32))
    st = g["stats_in"]
    env.victims_rescued.copy_(_t(st[:, 0], torch.int32))
    env.distance.copy_(_t(st[:, 1], torch.float64))
    env.energy_used.copy_(_t(st[:, 2], torch.float32))
    env.ttfr.copy_(_t(st[:, 3], torch.float64))
    env.falls.copy_(_t(st[:, 4], torch.int32))
    env.collisions.copy_(_t(st[:, 5], torch.int32))
    env.prev_robot_pos.copy_(_t(g["prev_robot_pos_in"], torch.float64))
    mc = g["con_dist"].shape[1]
    T = dict(qpos=_t(g["qpos"], dt), qvel=_t(g["qvel"], dt), xpos=_t(g["xpos"], dt), xquat=_t(g["xquat"], dt),
             ncon=_t(g["ncon"], torch.int32), con_dist=_t(g["con_dist"], dt),
             ctrl=torch.zeros(n, bipedal_model.nu, dtype=dt, device="cuda:0"), action=_t(g["action"], torch.float64 if act64 else torch.float32),
             obs=torch.zeros(n, 102, dtype=torch.float32, device="cuda:0"),
             reward=torch.zeros(n, dtype=torch.float64, device="cuda:0"),
             term=torch.zeros(n, dtype=torch.uint8, device="cuda:0"),
             trunc=torch.zeros(n, dtype=torch.uint8, device="cuda:0"),
             up=torch.zeros(n, dtype=torch.uint8, device="cuda:0"))
    io = cabi.MgxBipedalLogicIO(T["qpos"].data_ptr(), T["qvel"].data_ptr(), T["xpos"].data_ptr(),
                                T["xquat"].data_ptr(), T["ncon"].data_ptr(), T["con_dist"].data_ptr(), mc, 0,
                                T["ctrl"].data_ptr(), T["action"].data_ptr(), T["obs"].data_ptr(),
                                T["reward"].data_ptr(), T["term"].data_ptr(), T["trunc"].data_ptr(), T["up"].data_ptr())
    env._env.action_f64 = 1 if act64 else 0
    check(lib().mgx_bipedal_logic_test(env.native.handle, C.byref(io), C.byref(env._env), n, None), "logic_test")
    torch.cuda.synchronize()
    obs, rew = T["obs"].cpu().numpy(), T["reward"].cpu().numpy()
    np.testing.assert_array_equal(T["term"].cpu().numpy().astype(bool), g["terminated"])
    np.testing.assert_array_equal(T["trunc"].cpu().numpy().astype(bool), g["truncated"])
    np.testing.assert_array_equal(T["up"].cpu().numpy().astype(bool), g["upright"])
    np.testing.assert_array_equal(env.rescued.cpu().numpy(), _mask(g["rescued_out"]))
    np.testing.assert_array_equal(env.carried.cpu().numpy(), _mask(g["carried_out"]))
    np.testing.assert_array_equal(env.carrying.cpu().numpy().astype(bool), g["carrying_out"])
    np.testing.assert_array_equal(env.step_count.cpu().numpy(), g["current_step_out"])
    np.testing.assert_array_equal(env.energy.cpu().numpy().astype(np.float64), g["energy_out"])
    np.testing.assert_array_equal(env.prev_rescued.cpu().numpy(), g["prev_rescued_out"])
    np.testing.assert_array_equal(env.prev_carried.cpu().numpy(), g["prev_carried_out"])
    np.testing.assert_array_equal(env.fall_timer.cpu().numpy(), g["fall_timer_out"])
    so = g["stats_out"]
    np.testing.assert_array_equal(env.victims_rescued.cpu().numpy(), so[:, 0])
    np.testing.assert_array_equal(env.energy_used.cpu().numpy().astype(np.float64), so[:, 2])
    np.testing.assert_array_equal(env.ttfr.cpu().numpy(), so[:, 3])
    np.testing.assert_array_equal(env.falls.cpu().numpy(), so[:, 4])
    np.testing.assert_array_equal(env.collisions.cpu().numpy(), so[:, 5])
    np.testing.assert_array_equal(T["ctrl"].cpu().numpy()[:, :26], g["ctrl_out"][:, :26])
    if prec == "f64":
        np.testing.assert_array_equal(obs, g["obs"])
        np.testing.assert_array_equal(rew, g["reward"])
        np.testing.assert_array_equal(env.closest.cpu().numpy(), g["closest_out"])
        np.testing.assert_array_equal(env.prev_sz.cpu().numpy(), g["prev_sz_out"])
        np.testing.assert_array_equal(env.distance.cpu().numpy(), so[:, 1])
        np.testing.assert_array_equal(env.prev_robot_pos.cpu().numpy(), g["prev_robot_pos_out"])
    else:
        np.testing.assert_allclose(obs, g["obs"], atol=2e-5, rtol=1e-6)
        fin = np.isfinite(g["reward"])
        np.testing.assert_array_equal(rew[~fin], g["reward"][~fin])
        np.testing.assert_allclose(rew[fin], g["reward"][fin], rtol=1e-6, atol=1e-3)


class _OracleBipedal:
    """CPU oracle of one bipedal env: mjref physics (RK4) + numpy logic, reset from explicit draws."""

    def __init__(self, packed, tables, draws):
        from oracle.bipedal_logic import BipedalLogic, BipedalTables
        from oracle.mjref import RefSim
        self.sim = RefSim(packed)
        self.L = BipedalLogic(BipedalTables(packed.model))
        self.s = dict(prev_rescued=-1, prev_carried=-1, prev_sz=float("nan"), fall_timer=-1)
        self.reset(draws)

    def view(self):
        sim, s = self.sim, self.s
        s.update(qpos=sim.qpos, qvel=sim.qvel, ctrl=sim.ctrl, xpos=sim.xpos.reshape(-1, 3),
                 xquat=sim.xquat.reshape(-1, 4), con_dist=sim.contacts()["dist"])

    def reset(self, draws):
        self.sim.reset()
        self.view()
        self.L.apply_reset(self.s, draws)
        self.sim.step(10)
        self.view()
        self.L.after_reset(self.s)
        return self.L.obs(self.s)

    def step(self, action):
        a = self.L.pre(self.s, action)
        self.sim.step()
        self.view()
        return self.L.post(self.s, a)


def _well_conditioned(packed, tables, draws, actions, tol=1e-6):
    """The oracle's own sensitivity along the trajectory: the same reset + action stream with
    qpos perturbed by 1e-12 after the reset. Bipedal states with light victim links in deep,
    unconverged (50-sweep PGS) contact amplify 1e-13 input noise by ~1e6 per step; on such
    trajectories no two fp64 implementations (kernel and oracle, or two MuJoCo builds) agree,
    so the end-to-end bar applies to the well-conditioned ones."""
    a, b = _OracleBipedal(packed, tables, draws), _OracleBipedal(packed, tables, draws)
    b.sim.qpos[:] += np.random.default_rng(0).normal(scale=1e-12, size=b.sim.qpos.shape)
    for act in actions:
        oa, _, _, _ = a.step(act)
        ob, _, _, _ = b.step(act)
        if np.max(np.abs(oa - ob)) > tol:
            return False
    return True


@pytest.mark.parametrize("staged", [True, False])
def test_bipedal_end_to_end_f64_matches_oracle(bipedal_model, bipedal_packed, staged):
    """staged=True: the staged RK4 step (row builder -> lane-group PGS -> stage finisher per RK4
    stage; reset settled by the same stages); staged=False: one wave per env."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.seeding import np_random
    n, steps = 12, 15
    env = BipedalVectorEnv(n, precision="f64", autoreset=False, staged=staged)
    draws = np.stack([env.tables.reset_draws(np_random(200 + i)[0]) for i in range(n)])
    rng = np.random.default_rng(11)
    acts = (rng.uniform(-1, 1, (steps, n, 26)) * 100.0 * 0.1).astype(np.float32)
    good = [i for i in range(n) if _well_conditioned(bipedal_packed, env.tables, draws[i], acts[:, i])]
    assert len(good) >= 4, f"only envs {good} are well-conditioned"
    obs, _ = env.reset(draws=draws)
    oracles = [_OracleBipedal(bipedal_packed, env.tables, draws[i]) for i in range(n)]
    o0 = obs.cpu().numpy()
    for i in good:
        np.testing.assert_allclose(o0[i], oracles[i].L.obs(oracles[i].s), atol=1e-5, err_msg=f"reset obs env {i}")
    # the ill-conditioned trajectories are still compared up to the step where their obs leave
    # the 1e-5 band (flags exact, reward within 1e-3 on every step before that)
    tracking = {i for i in range(n) if i not in good
                and np.max(np.abs(o0[i] - oracles[i].L.obs(oracles[i].s))) <= 1e-5}
    compared = 0
    for k in range(steps):
        obs, rew, term, trunc, _ = env.step(_t(acts[k], torch.float32))
        torch.cuda.synchronize()
        ob, rw = obs.cpu().numpy(), rew.cpu().numpy()
        te, tr = term.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool)
        for i in good:
            o, r, t1, t2 = oracles[i].step(acts[k, i])
            np.testing.assert_allclose(ob[i], o, atol=1e-5, err_msg=f"obs env {i} step {k}")
            assert (rw[i] == r) if not np.isfinite(r) else abs(rw[i] - r) < 1e-3, (i, k, rw[i], r)
            assert te[i] == t1 and tr[i] == t2, (i, k)
        for i in sorted(tracking):
            o, r, t1, t2 = oracles[i].step(acts[k, i])
            if not np.max(np.abs(ob[i] - o)) <= 1e-5:
                tracking.discard(i)  # diverged: the oracle itself is sensitive here
                continue
            assert (rw[i] == r) if not np.isfinite(r) else abs(rw[i] - r) < 1e-3, (i, k, rw[i], r)
            assert te[i] == t1 and tr[i] == t2, (i, k)
            compared += 1
    print(f"ill-conditioned envs: {compared} (env, step) pairs compared before divergence")


def test_bipedal_end_to_end_f64_bench_actions(bipedal_packed):
    """Bench conditions (BASELINE configs[3]): U(-100, 100) actions, the staged fp64 step of 8 envs
    x 20 steps against the oracle for as long as the oracle determines the trajectory. Two twins
    run beside the oracle on the same actions — qpos perturbed by 1e-12 after the reset (the
    model has no free joint; its joint ranges are effectively unlimited, quirk B2) and the PGS
    residuals summed in reverse order (another fp64 rounding of the same solve). While the larger
    twin spread is <= 1e-6 the device must be within max(1e-6, 20 x spread) of the oracle (qpos,
    qvel relative to max(1, |x|)), the reward within 1e-3 (identical where infinite) and the flags
    exact; every env is compared until the spread leaves that band or the episode ends."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.seeding import np_random
    n, steps = 8, 20
    env = BipedalVectorEnv(n, precision="f64", autoreset=False)
    draws = np.stack([env.tables.reset_draws(np_random(300 + i)[0]) for i in range(n)])
    rng = np.random.default_rng(29)
    acts = (rng.uniform(-1, 1, (steps, n, 26)) * 100.0).astype(np.float32)
    env.reset(draws=draws)
    runs = []
    for i in range(n):
        trio = [_OracleBipedal(bipedal_packed, env.tables, draws[i]) for _ in range(3)]
        trio[1].sim.qpos[:] += np.random.default_rng(i).normal(scale=1e-12, size=trio[1].sim.qpos.shape)
        trio[2].sim.set_pgs_reverse(True)
        runs.append(trio)

    def err(q, v, o):
        x = np.concatenate([o.sim.qpos, o.sim.qvel])
        return float(np.max(np.abs(x - np.concatenate([q, v])) / np.maximum(1.0, np.abs(x))))

    live = set(range(n))
    horizon = np.zeros(n, dtype=int)
    worst = np.zeros(n)
    for k in range(steps):
        obs, rew, term, trunc, _ = env.step(_t(acts[k], torch.float32))
        torch.cuda.synchronize()
        rw, te, tr = rew.cpu().numpy(), term.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool)
        qg, vg = env.batch.qpos.cpu().numpy(), env.batch.qvel.cpu().numpy()
        for i in sorted(live):
            out = [o.step(acts[k, i]) for o in runs[i]]
            o = runs[i][0]
            spread = max(err(x.sim.qpos, x.sim.qvel, o) for x in runs[i][1:])
            if spread > 1e-6:
                live.discard(i)
                continue
            e = err(qg[i], vg[i], o)
            assert e <= max(1e-6, 20 * spread), (k, i, e, spread)
            _, r, t1, t2 = out[0]
            assert (rw[i] == r) if not np.isfinite(r) else abs(rw[i] - r) < 1e-3, (i, k, rw[i], r)
            assert te[i] == t1 and tr[i] == t2, (i, k)
            horizon[i] += 1
            worst[i] = max(worst[i], e)
            if t1 or t2:
                live.discard(i)
    print(f"\nbipedal U(+-100): steps compared per env {horizon.tolist()}; "
          f"worst device error {[f'{w:.1e}' for w in worst]}")
    assert horizon.min() >= 5 and horizon.sum() >= 80, horizon


def test_bipedal_autoreset_and_sharding_invariance():
    """Global env index keys the reset draws: a 2-env shard at offset 2 reproduces envs 2..3
    of a 4-env run bit for bit, through truncations and same-step autoresets."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    full = BipedalVectorEnv(4, precision="f32", seed=9, max_episode_steps=5)
    shard = BipedalVectorEnv(2, precision="f32", seed=9, max_episode_steps=5, env_offset=2)
    full.reset()
    shard.reset()
    rng = np.random.default_rng(3)
    ends = 0
    for k in range(12):
        act = (rng.uniform(-1, 1, (4, 26)) * 100.0).astype(np.float32)
        fo, fr, ft, fu, _ = full.step(_t(act, torch.float32))
        so, sr, st, su, _ = shard.step(_t(act[2:], torch.float32))
        torch.cuda.synchronize()
        assert torch.equal(fo[2:], so) and torch.equal(fr[2:], sr)
        assert torch.equal(ft[2:], st) and torch.equal(fu[2:], su)
        ends += int((fu | ft).sum())
    assert ends >= 8
    assert int(full.episode.min()) >= 3
    assert torch.isfinite(full.obs).all()
    # quirk B3: the lazily created attributes survive the autoresets
    assert int(full.prev_rescued.min()) >= 0 and int(full.fall_timer.min()) >= 0


def test_bipedal_f32_rollout_finite_and_counted():
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    n = 256
    env = BipedalVectorEnv(n, precision="f32", seed=1)
    env.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    for _ in range(30):
        a = (torch.rand(n, 26, device="cuda:0", generator=g) * 2 - 1) * 100.0
        env.step(a)
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs).all()
    assert int(env.rollout[:, 3].sum()) == 30 * n


def _bip_trajectory(n, banks, steps, seed=9, prec="f64", max_steps=6, staged=True):
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    env = BipedalVectorEnv(n, precision=prec, seed=seed, max_episode_steps=max_steps, staged=staged, banks=banks)
    o, _ = env.reset()
    out = [o.cpu().numpy().copy()]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    for _ in range(steps):
        a = ((torch.rand(n, 26, device="cuda:0", generator=g) * 2 - 1) * 100.0).contiguous()
        obs, rew, term, trunc, _ = env.step(a)
        out.append(np.concatenate([obs.cpu().numpy().ravel(), rew.cpu().numpy().ravel(),
                                   term.cpu().numpy().ravel().astype(np.float64),
                                   trunc.cpu().numpy().ravel().astype(np.float64),
                                   env.batch.qpos.cpu().numpy().ravel()]))
    torch.cuda.synchronize()
    return out, env.episode.cpu().numpy().copy(), int(env.batch.warning.sum())


@pytest.mark.parametrize("banks", [1, 2])
def test_bipedal_bank_count_does_not_change_trajectories(banks):
    """Staged RK4 step: the bank count is a performance knob only. banks = 0 (every autoreset
    settled by k_rk_settle) and banks = R (ready banks installed, not-ready ones settled by
    k_rk_settle: episodes of 6 steps are shorter than a bank's 10 settle steps) give the same
    trajectories bit for bit."""
    ref, e0, w0 = _bip_trajectory(8, 0, 14)
    got, e1, w1 = _bip_trajectory(8, banks, 14)
    assert int(e0.sum()) >= 8 * 3
    for t, (x, y) in enumerate(zip(ref, got)):
        np.testing.assert_array_equal(x, y, err_msg=f"step {t}")
    np.testing.assert_array_equal(e0, e1)
    assert w0 == w1


def test_bipedal_reset_and_masked_step_mid_run():
    """A masked reset() and a masked step in the middle of a run with 3-step episodes, banks = 2
    against banks = 0: the settle kernel's reset mode under a mask, its bank prefill, the ready-bank
    install (an env's first two autoresets) and the fixup list (its third: the bank restarted six
    steps earlier needs ten to settle) all give the same bits, and masked envs stay put. Every
    output of every step and every state tensor at the end is compared bytewise."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from tests.helpers import assert_runs_bit_equal, reset_and_masked_step_run
    runs = [reset_and_masked_step_run(
        BipedalVectorEnv(4, precision="f64", seed=9, max_episode_steps=3, staged=True, banks=b), 26, 100.0)
        for b in (0, 2)]
    assert runs[0][2] >= 12
    assert_runs_bit_equal(*runs)


def _obs_close(x, y, tol=1e-6):
    """Within tol absolute plus tol relative: the observation is float32, whose rounding of an
    entry near 30 (positions, distances) moves by 2-4e-6 when its fp64 source moves by 1e-12."""
    return bool(np.all(np.abs(np.asarray(x, np.float64) - y) <= tol * (1 + np.abs(y))))


def _conditioned_through_reset(packed, tables, draws, actions, tol=1e-5):
    """_well_conditioned from before the settle: the twin's qpos is perturbed by 1e-12 right after
    the reset draws are applied, so the ten settle steps are part of the probed trajectory; obs
    compared as _obs_close."""
    a = _OracleBipedal(packed, tables, draws)
    b = _OracleBipedal.__new__(_OracleBipedal)
    from oracle.bipedal_logic import BipedalLogic, BipedalTables
    from oracle.mjref import RefSim
    b.sim = RefSim(packed)
    b.L = BipedalLogic(BipedalTables(packed.model))
    b.s = dict(prev_rescued=-1, prev_carried=-1, prev_sz=float("nan"), fall_timer=-1)
    b.sim.reset()
    b.view()
    b.L.apply_reset(b.s, draws)
    b.sim.qpos[:] += np.random.default_rng(1).normal(scale=1e-12, size=b.sim.qpos.shape)
    b.sim.step(10)
    b.view()
    b.L.after_reset(b.s)
    if not _obs_close(a.L.obs(a.s), b.L.obs(b.s), tol):
        return False
    for act in actions:
        oa, _, _, _ = a.step(act)
        ob, _, _, _ = b.step(act)
        if not _obs_close(oa, ob, tol):
            return False
    return True


def test_bipedal_staged_matches_monolithic(bipedal_packed):
    """The staged RK4 step and the one-wave-per-env kernel compute the same mj_step (the solver's
    summation order differs): 8 envs from host draws, reset + 6 steps at 0.3 x the action range.
    The envs compared are chosen by the oracle alone (a 1e-12 twin from before the settle stays
    within 1e-5, absolute + relative, through the reset and every step:
    _conditioned_through_reset — the settle leaves velocities near 0 that a 1e-12 input moves by
    ~3e-6, so 1e-6 is below the oracle's own resolution here); on them obs agree to the same bar
    at the reset and every step and the flags exactly, and at least 4 of 8 qualify."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.seeding import np_random
    n, steps = 8, 6
    a = BipedalVectorEnv(n, precision="f64", seed=3, staged=True, autoreset=False)
    b = BipedalVectorEnv(n, precision="f64", seed=3, staged=False, autoreset=False)
    draws = np.stack([a.tables.reset_draws(np_random(300 + i)[0]) for i in range(n)])
    rng = np.random.default_rng(5)
    acts = (rng.uniform(-1, 1, (steps, n, 26)) * 100.0 * 0.3).astype(np.float32)
    good = [i for i in range(n) if _conditioned_through_reset(bipedal_packed, a.tables, draws[i], acts[:, i])]
    assert len(good) >= 4, f"only envs {good} are well-conditioned"
    oa, _ = a.reset(draws=draws)
    ob, _ = b.reset(draws=draws)
    torch.cuda.synchronize()
    np.testing.assert_allclose(oa.cpu().numpy()[good], ob.cpu().numpy()[good], rtol=1e-5, atol=1e-5, err_msg="reset obs")
    for k in range(steps):
        act = _t(acts[k], torch.float32)
        ra = a.step(act)
        rb = b.step(act)
        torch.cuda.synchronize()
        np.testing.assert_allclose(ra[0].cpu().numpy()[good], rb[0].cpu().numpy()[good], rtol=1e-5, atol=1e-5,
                                   err_msg=f"obs step {k}")
        for f in (2, 3):
            np.testing.assert_array_equal(ra[f].cpu().numpy()[good], rb[f].cpu().numpy()[good])
    print(f"staged vs monolithic compared on envs {good}")


def test_bipedal_f32_distribution_matches_f64():
    """Bench conditions (U(-100, 100) actions, autoreset): the staged fp32 step against the staged
    fp64 step over 512 envs x 130 steps (past the 101-step fall timer, so episodes end and reset).
    fp32 cannot follow an fp64 trajectory of this stiff model for long, so the statistics are
    compared: mean reward per env step within 3%, the termination rate per env within 5 binomial
    sigma (+ 0.02)."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    n, steps = 512, 130
    stats = {}
    for prec in ("f64", "f32"):
        env = BipedalVectorEnv(n, precision=prec, seed=17)
        env.reset()
        g = torch.Generator(device="cuda:0")
        g.manual_seed(23)
        rsum = torch.zeros((), dtype=torch.float64, device="cuda:0")
        rcnt = torch.zeros((), dtype=torch.float64, device="cuda:0")
        for _ in range(steps):
            a = ((torch.rand(n, 26, device="cuda:0", generator=g) * 2 - 1) * 100.0).contiguous()
            _, r, _, _, _ = env.step(a)
            # the first step after a reset can be +inf (closest_victim_distance restarts at +inf,
            # quirk B3): averaged over the finite rewards
            fin = torch.isfinite(r)
            rsum += torch.where(fin, r, torch.zeros_like(r)).sum()
            rcnt += fin.sum()
        torch.cuda.synchronize()
        ro = env.rollout.double().sum(0).cpu().numpy()
        stats[prec] = dict(reward=float(rsum / rcnt), term=ro[1] / n, steps=ro[3],
                           finite=bool(torch.isfinite(env.obs).all()))
    a, b = stats["f64"], stats["f32"]
    print(f"\nbipedal fp64 {a}\nbipedal fp32 {b}")
    assert a["finite"] and b["finite"] and a["steps"] == b["steps"] == n * steps
    assert abs(a["reward"] - b["reward"]) <= 0.03 * abs(a["reward"]) + 1.0
    p = min(max(a["term"], 0.01), 0.99)
    assert abs(a["term"] - b["term"]) <= 5 * np.sqrt(p * (1 - p) / n) + 0.02, (a["term"], b["term"])


@pytest.mark.parametrize("serial", [False, True], ids=["streams", "sub_batches"])
def test_bipedal_stream_shards_equal_single_batch(serial):
    """The generic StreamShardedEnv (envs/sharded.py; bench.py --streams / --sub-batches) over
    BipedalVectorEnv: 2 shards on 2 HIP streams, or 2 sub-batches one after another on one
    stream, reproduce one batch bit for bit (fp64, U(+-100) actions)."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.envs.sharded import StreamShardedEnv
    n = 101
    one = BipedalVectorEnv(n, precision="f64", seed=4)
    sh = StreamShardedEnv(lambda k, off: BipedalVectorEnv(k, precision="f64", seed=4, env_offset=off), n, 2,
                          serial=serial)
    one.reset()
    sh.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2)
    for t in range(40):
        a = ((torch.rand(n, 26, device="cuda:0", generator=g) * 2 - 1) * 100.0).contiguous()
        s1 = one.step(a)
        s2 = sh.step(a)
        for x, y, name in zip(s1[:4], s2[:4], ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), (t, name)
    torch.cuda.synchronize()
    assert torch.equal(one.episode, sh.episode)
    assert torch.equal(one.rollout, sh.rollout)
