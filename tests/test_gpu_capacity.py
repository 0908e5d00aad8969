"""GPU: contact / row capacity of the staged soccer step (MuJoCo keeps every contact: its arena
has no 64-contact / 192-row cap).

The staged step (the default SoccerVectorEnv) stores up to EFC_CAPACITY = 384 rows / 96 contacts
per env; full_capacity=False keeps 192 / 64 and counts the overflow. Its main
solver launch solves every slot (row scalars read from the pipe, make_staged_pipe `sqg`); the
test hook MGX_PGS_LDS_ROWS instead gives the main launch that many LDS-scalar rows per slot and
lists a slot with more for the wide launch (B, scalars and table in LDS, one slot per wave)
instead of truncating it. The hooks are read once, when the env's model is created (mgx_model_create,
Hooks); a low value sends ordinary bench-condition states — 40..120 rows — through the wide launch
on every step:
  * bit-identical to the default launch (which launch solves a slot changes nothing);
  * fp64 end to end against the oracle (no cap) with every slot over the lowered threshold;
  * a model whose own row capacity is below a state's rows truncates in MuJoCo's row order and
    counts the step in mgx_state.overflow (the documented behaviour past the storage capacity);
    MGX_MAX_NEFC can raise a model's capacity, never lower it (refused).
"""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_soccer import _oracle_env, _sync_view

pytestmark = pytest.mark.gpu


class _LdsRows:
    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.old = os.environ.get("MGX_PGS_LDS_ROWS")
        os.environ["MGX_PGS_LDS_ROWS"] = str(self.rows)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MGX_PGS_LDS_ROWS", None)
        else:
            os.environ["MGX_PGS_LDS_ROWS"] = self.old


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_wide_solver_launch_bit_identical(soccer_model, prec):
    """Under the default split threshold the slots over the hook's 16 rows go to the row-split waves,
    which this test pins; test_wide_and_single_launch_bit_identical reaches the wide launch."""
    from mujoco_gymnasium_environments_amd.envs.soccer import EFC_CAPACITY, SoccerVectorEnv
    n, steps = 64, 30
    a = SoccerVectorEnv(n, precision=prec, seed=21, full_capacity=True)
    with _LdsRows(16):  # read when b's model is created
        b = SoccerVectorEnv(n, precision=prec, seed=21, full_capacity=True)
    assert a.native.info.max_nefc == 192  # the monolithic layout (reset settle, debug) keeps 192
    a.reset()
    b.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(4)
    nefc_sum = 0.0
    for t in range(steps):
        act = torch.rand(n, soccer_model.nu, device="cuda:0", generator=g) * 300 - 150
        ra = a.step(act)
        rb = b.step(act)
        torch.cuda.synchronize()
        for x, y, name in zip(ra[:4], rb[:4], ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), (t, name)
        assert torch.equal(a.batch.qpos, b.batch.qpos) and torch.equal(a.batch.qvel, b.batch.qvel), t
    nefc_sum = float(b.rollout[:, 4].sum())
    steps_done = float(b.rollout[:, 3].sum())
    assert nefc_sum / steps_done > 16  # the wide launch solved (nearly) every slot
    assert EFC_CAPACITY == 384


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_WIDE = {"MGX_PGS_SPLIT_BLOCKS": "0", "MGX_PGS_LDS_ROWS": "16"}


@pytest.mark.parametrize("hooks,prec", [
    pytest.param(_WIDE, "f64", id="wide-side-f64"),
    pytest.param(_WIDE, "f32", id="wide-side-f32"),
    pytest.param({**_WIDE, "MGX_SIDE_STREAM": "0"}, "f64", id="wide-seq"),
    pytest.param({**_WIDE, "MGX_PGS_WIDE_LDS": "0"}, "f64", id="wide-globalB"),
    pytest.param({"MGX_PGS_SPLIT_BLOCKS": "0", "MGX_PGS_SINGLE": "1"}, "f64", id="single"),
])
def test_wide_and_single_launch_bit_identical(soccer_model, hooks, prec):
    """The host branches of the soccer step that the row-split default leaves dormant, each against
    an env with no hook set, bit for bit over 40 steps (3 banks, same-step autoreset): without split
    waves, 16 LDS rows send most slots to the wide launch, which runs on the side stream beside the
    main launch (wide-side), after it on the caller's stream (wide-seq), or with B read from global
    memory (wide-globalB); MGX_PGS_SINGLE=1 is the one main launch over every slot (single). The
    wide ids also read the pipe's counters: the wide launch had the listed slots, split mode none."""
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    from tests.test_gpu_pgs_split import _counters
    n, steps = 16, 40
    a = SoccerVectorEnv(n, precision=prec, seed=71, banks=3, full_capacity=True)
    with _Env(**hooks):  # read when b's model is created
        b = SoccerVectorEnv(n, precision=prec, seed=71, banks=3, full_capacity=True)
    a.reset()
    b.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    for t in range(steps):
        act = torch.rand(n, soccer_model.nu, device="cuda:0", generator=g) * 300 - 150
        ra = a.step(act)
        rb = b.step(act)
        torch.cuda.synchronize()
        for x, y, name in zip(ra[:4], rb[:4], ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), (t, name)
        assert torch.equal(a.batch.qpos, b.batch.qpos) and torch.equal(a.batch.qvel, b.batch.qvel), t
    if "MGX_PGS_LDS_ROWS" in hooks:
        split, listed, capE = _counters(b)
        assert capE == 16
        assert listed > 20 * n, listed  # the wide launch really had work
        assert split == 0, split


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_lds_arena_solver_bit_identical(soccer_model, prec):
    """The main solver launch with B copied into an LDS arena (MGX_PGS_LDS_B=1; a small arena so
    that some waves do not fit and go to the global-B launch) runs the identical arithmetic as
    the default global-B launch: the same states, bit for bit."""
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    n, steps = 64, 25
    a = SoccerVectorEnv(n, precision=prec, seed=33)
    with _Env(MGX_PGS_LDS_B="1", MGX_PGS_ARENA="24576"):  # read when b's model is created
        b = SoccerVectorEnv(n, precision=prec, seed=33)
    a.reset()
    b.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    for t in range(steps):
        act = torch.rand(n, soccer_model.nu, device="cuda:0", generator=g) * 300 - 150
        ra = a.step(act)
        rb = b.step(act)
        torch.cuda.synchronize()
        for x, y, name in zip(ra[:4], rb[:4], ("obs", "reward", "terminated", "truncated")):
            assert torch.equal(x, y), (t, name)
        assert torch.equal(a.batch.qpos, b.batch.qpos) and torch.equal(a.batch.qvel, b.batch.qvel), t


def test_rows_over_main_launch_match_oracle(soccer_model, soccer_packed):
    """fp64 end to end (reset draws + 25 random-action steps, obs 1e-5, reward 1e-6 relative,
    flags exact) with every slot over the lowered LDS threshold."""
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    from mujoco_gymnasium_environments_amd.seeding import np_random
    m = soccer_model
    n = 4
    with _LdsRows(8):  # read when the env's model is created
        env = SoccerVectorEnv(n, precision="f64", autoreset=False, full_capacity=True)
    draws = np.stack([env.tables.reset_draws(np_random(100 + i)[0]) for i in range(n)])
    env.reset(draws=draws)
    torch.cuda.synchronize()
    oracles = [_oracle_env(soccer_packed, env.tables, draws[i]) for i in range(n)]
    for sim, L, s in oracles:
        _sync_view(sim, s, m)
        s["prev_ball_pos"] = s["xpos"][env.tables.ball].copy()
        s["prev_robot_pos"] = s["xpos"][env.tables.torso].copy()
    rng = np.random.default_rng(5)  # test_gpu_soccer's end-to-end trajectory
    over = 0
    for t in range(25):
        act = rng.uniform(-20, 20, (n, m.nu)).astype(np.float32)
        obs, rew, term, _, _ = env.step(torch.from_numpy(act).cuda())
        torch.cuda.synchronize()
        og, rg, tg = obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
        for i, (sim, L, s) in enumerate(oracles):
            a = L.pre(s, act[i])
            sim.step()
            _sync_view(sim, s, m)
            over += int(sim.nefc[0]) > 8
            o_obs, r, te, tr, _, _ = L.post(s, a, t + 1)
            np.testing.assert_allclose(og[i], o_obs, atol=1e-5, err_msg=f"step {t} env {i}")
            assert abs(rg[i] - r) <= 1e-6 * max(1.0, abs(r)), (t, i, rg[i], r)
            assert bool(tg[i]) == te, (t, i)
    assert over >= 80, over
    assert int(env.batch.overflow.sum()) == 0


def test_storage_capacity_truncates_and_counts(soccer_model, monkeypatch):
    """Past the storage capacity (here a model whose own row capacity is 40) rows are dropped in
    MuJoCo's order and the step is counted in mgx_state.overflow; below it nothing is counted.
    MGX_MAX_NEFC below a model's capacity is refused at model creation."""
    import copy

    from mujoco_gymnasium_environments_amd.envs import soccer as soccer_mod
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    from mujoco_gymnasium_environments_amd.native import NativeError
    m40 = copy.deepcopy(soccer_model)
    m40.efc_capacity = 40
    monkeypatch.setattr(soccer_mod, "soccer_model", lambda full_capacity=False: m40)
    small = SoccerVectorEnv(32, precision="f64", seed=3, full_capacity=False)
    monkeypatch.undo()
    monkeypatch.setenv("MGX_MAX_NEFC", "40")
    with pytest.raises(NativeError, match="MGX_MAX_NEFC below"):
        SoccerVectorEnv(2, precision="f64", seed=3)
    monkeypatch.delenv("MGX_MAX_NEFC")
    full = SoccerVectorEnv(32, precision="f64", seed=3, full_capacity=True)
    small.reset()
    full.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(2)
    for _ in range(10):
        act = torch.rand(32, soccer_model.nu, device="cuda:0", generator=g) * 300 - 150
        small.step(act)
        full.step(act)
    torch.cuda.synchronize()
    assert int(small.batch.overflow.sum()) > 0
    assert int(full.batch.overflow.sum()) == 0


@pytest.mark.parametrize("wpc", [6])
def test_solver_occupancy_hook_bit_identical(soccer_model, wpc):
    """MGX_PGS_WPC sizes the main solver launch's LDS rows for more waves per CU; slots beyond
    them run in the same launch with their row scalars read from the pipe (Pipe.hmain) — the same
    arithmetic, so the same states bit for bit at bench actions (fp64, full capacity), and the
    staged parkour step likewise."""
    from mujoco_gymnasium_environments_amd.envs.parkour import ParkourVectorEnv, action_limits
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    n, steps = 256, 30
    a = SoccerVectorEnv(n, precision="f64", seed=41)
    pa = ParkourVectorEnv(n, precision="f64", seed=41)
    with _Env(MGX_PGS_WPC=str(wpc)):  # read when b's model is created
        b = SoccerVectorEnv(n, precision="f64", seed=41)
        pb = ParkourVectorEnv(n, precision="f64", seed=41)
    assert pb.staged
    for e in (a, b, pa, pb):
        e.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    lim = torch.as_tensor(action_limits(), dtype=torch.float32, device="cuda:0")
    for t in range(steps):
        act = torch.rand(n, soccer_model.nu, device="cuda:0", generator=g) * 300 - 150
        pact = ((torch.rand(n, 16, device="cuda:0", generator=g) * 2 - 1) * lim).contiguous()
        for (x, y), ac in (((a, b), act), ((pa, pb), pact)):
            rx, ry = x.step(ac), y.step(ac)
            for u, v, name in zip(rx[:4], ry[:4], ("obs", "reward", "terminated", "truncated")):
                assert torch.equal(u, v), (type(x).__name__, t, name)
    torch.cuda.synchronize()
    assert torch.equal(a.batch.qpos, b.batch.qpos) and torch.equal(pa.batch.qpos, pb.batch.qpos)
    assert int(a.batch.overflow.sum()) == 0 and int(pa.batch.overflow.sum()) == 0


def test_broadphase_prefilters_bit_identical():
    """The broadphase's bounding-box prefilters (Layout.tight_bp, on by default for models with more
    than 200 candidate pairs) only drop pairs the narrowphase would return no contact for: soccer (staged,
    fp64) and bipedal (staged RK4, fp64) step bit-identically with them off (MGX_TIGHT_BROADPHASE=0)
    at bench actions (tests/test_broadphase_prefilter.py checks the same on the oracle's states)."""
    from mujoco_gymnasium_environments_amd.envs.bipedal import BipedalVectorEnv
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    n, steps = 128, 30
    a = SoccerVectorEnv(n, precision="f64", seed=51)
    pa = BipedalVectorEnv(n, precision="f64", seed=51)
    with _Env(MGX_TIGHT_BROADPHASE="0"):  # read when b's model is created
        b = SoccerVectorEnv(n, precision="f64", seed=51)
        pb = BipedalVectorEnv(n, precision="f64", seed=51)
    for e in (a, b, pa, pb):
        e.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(8)
    for t in range(steps):
        act = torch.rand(n, a.model.nu, device="cuda:0", generator=g) * 300 - 150
        bact = ((torch.rand(n, 26, device="cuda:0", generator=g) * 2 - 1) * 100).contiguous()
        for (x, y), ac in (((a, b), act), ((pa, pb), bact)):
            rx, ry = x.step(ac), y.step(ac)
            for u, v, name in zip(rx[:4], ry[:4], ("obs", "reward", "terminated", "truncated")):
                assert torch.equal(u, v), (type(x).__name__, t, name)
    torch.cuda.synchronize()
    assert torch.equal(a.batch.qpos, b.batch.qpos) and torch.equal(pa.batch.qpos, pb.batch.qpos)
