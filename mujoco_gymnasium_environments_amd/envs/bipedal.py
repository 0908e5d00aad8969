"""bipedal_rescue_env on MI355X (BASELINE configs[3]): a batched VectorEnv and a drop-in
gymnasium-style Env.

Mirrors the reference interface bipedal_rescue_env/rescue_env.py:
  * ``BipedalRescueEnv`` — same constructor / ``reset(seed, options)`` / ``step(action)`` /
    spaces / ``metadata`` / ``render`` / ``close`` / ``info`` surface as the reference class
    (rescue_env.py:28-793), batch size 1, gymnasium seeding (PCG64 over SeedSequence) and the
    same 12 position draws per reset (:473-508).
  * ``BipedalVectorEnv`` — N envs on one GPU, device tensors ``[N, ...]``, same-step autoreset
    with Philox reset draws keyed by (seed, global env index, episode).
Both run one fused HIP launch per env step (libmgx.so ``mgx_bipedal_step``): clip, float32
energy, one RK4 mj_step, victim pickup / rescue, observation / reward / termination / stats.

The composed model is the output of the reference's own composition code
(rescue_env.py:121-277, tests/golden/make_fixtures.py): RK4 integrator (rescue_env.py:148),
PGS, nq = nv = 63, 41 bodies, 89 geoms, 3185 candidate pairs including static cylinders.
Under random actions it holds up to ~130 contacts / ~520 constraint rows (oracle rollouts),
so its rows live in global scratch (Layout.gB) rather than LDS.
"""
from __future__ import annotations

import functools
import os
from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import cabi, mjcf
from ..spaces import Box
from .base import TaskEnv, TaskVectorEnv

ASSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "bipedal_rescue.xml")
# MuJoCo keeps every contact (no arena limit at these sizes). Measured at bench conditions (U(-100,
# 100) actions, autoreset, 28k oracle env steps): up to 146 contacts / 585 rows, above 128 / 512 on
# 3 of them; 192 / 768 keep every row (the staged RK4 step holds up to 192 contacts / 1024 rows)
EFC_CAPACITY = 768
CON_CAPACITY = 192

# rescue_env.py:298-308
JOINT_NAMES = [
    'neck_pitch', 'neck_yaw',
    'right_shoulder_pitch', 'right_shoulder_roll', 'right_elbow', 'right_wrist',
    'right_finger1_joint', 'right_finger2_joint',
    'left_shoulder_pitch', 'left_shoulder_roll', 'left_elbow', 'left_wrist',
    'left_finger1_joint', 'left_finger2_joint',
    'right_hip_roll', 'right_hip_pitch', 'right_hip_yaw', 'right_knee_joint',
    'right_ankle_pitch', 'right_ankle_roll',
    'left_hip_roll', 'left_hip_pitch', 'left_hip_yaw', 'left_knee_joint',
    'left_ankle_pitch', 'left_ankle_roll']
OBS_DIM = 102
N_ACT = 26
MAX_EPISODE_STEPS = 10000          # rescue_env.py:41
ACTION_LIMIT = 100.0               # rescue_env.py:328-333
SAFE_ZONE_POS = np.array([20.0, 0.0, 0.0])
ENERGY_LIMIT = 1000.0


@functools.lru_cache(maxsize=None)
def bipedal_model() -> mjcf.Model:
    with open(ASSET) as f:
        m = mjcf.compile_xml(f.read())
    m.efc_capacity = EFC_CAPACITY
    m.con_capacity = CON_CAPACITY
    return m


class BipedalTables:
    """Index tables looked up exactly as rescue_env.py:280-323 and :473-508 do."""

    def __init__(self, m: mjcf.Model, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.model = m
        self.torso = m.name2id("body", "torso")
        self.victims = [m.name2id("body", f"victim{i}") for i in range(1, 6)]
        self.joints = [m.name2id("joint", n) for n in JOINT_NAMES]
        q = lambda name: int(m.jnt_qposadr[m.name2id("joint", name)])  # noqa: E731
        self.root_x, self.root_y, self.root_z = q("root_x"), q("root_y"), q("root_z")
        self.root_dof = int(m.jnt_dofadr[m.name2id("joint", "root_x")])
        self.victim_x = [q(f"victim{i}_x") for i in range(1, 6)]
        self.victim_y = [q(f"victim{i}_y") for i in range(1, 6)]
        self.max_episode_steps = max_episode_steps

    def ids_struct(self) -> cabi.MgxBipedalIds:
        m, s = self.model, cabi.MgxBipedalIds()
        s.torso = self.torso
        for i in range(5):
            s.victims[i] = self.victims[i]
            s.victim_x[i] = self.victim_x[i]
            s.victim_y[i] = self.victim_y[i]
        for i, j in enumerate(self.joints):
            s.obs_qposadr[i] = int(m.jnt_qposadr[j])
            s.obs_dofadr[i] = int(m.jnt_dofadr[j])
        s.root_x, s.root_y, s.root_z, s.root_dof = self.root_x, self.root_y, self.root_z, self.root_dof
        s.n_act = N_ACT
        s.max_episode_steps = self.max_episode_steps
        return s

    @staticmethod
    def reset_draws(rng: np.random.Generator) -> np.ndarray:
        """The 12 uniform draws of one reset, in reference order (rescue_env.py:476-508)."""
        d = [rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0)]
        for _ in range(5):
            d += [rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0)]
        return np.array(d)


class BipedalVectorEnv(TaskVectorEnv):
    """``num_envs`` bipedal_rescue envs stepping in lockstep on one GPU, one RK4 mj_step per env
    step. ``step(actions)`` takes [N, 26] float32, or float64: a float64 action is clipped and
    applied in float64 and its energy terms follow in float64 (rescue_env.py:420-429, :650);
    ``reset(draws=)`` takes [N, 12]."""

    metadata = {'render_modes': [], 'render_fps': 50}
    TASK, ENV_STRUCT, OBS_DIM, N_DRAWS = "bipedal", cabi.MgxBipedalEnv, OBS_DIM, 12

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0,
                 staged: bool = True, banks: int = 1):
        """``staged`` selects the staged RK4 step (csrc/mgx_rk_staged.hip: per RK4 stage a row
        builder, the lane-group PGS and a stage finisher, with ``banks`` reset states settled ahead
        per env); ``staged=False`` runs one wave per env for the whole step. An episode lasts at
        least 101 steps unless truncated earlier (the fall timer, rescue_env.py:670-697), so one
        bank, ready 10 steps after it restarts, covers every autoreset.

        Capacity: the staged step holds the model's 192 contacts / 768 rows (the oracle census
        peaks at 585 rows, so no row is dropped at bench actions); the monolithic step
        (``staged=False``) keeps its rows in per-env scratch sized for 512 rows and drops rows past
        that in MuJoCo's order, counted in ``batch.overflow`` — the two paths compute the same
        physics on every env step under 512 rows (tests/test_gpu_bipedal.py)."""
        model = bipedal_model()
        self._setup(num_envs, device, precision, model, BipedalTables(model, max_episode_steps), autoreset, seed,
                    env_offset)
        dev, N = self.device, num_envs
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.step_count = torch.zeros(N, **i32)
        # current_energy / energy_used hold float32 values (numpy's float32 arithmetic for float32
        # actions) or float64 ones after a float64 action; energy_kind records which (include/mgx.h)
        self.energy = torch.full((N,), ENERGY_LIMIT, **f64)
        self.energy_used = torch.zeros(N, **f64)
        self.energy_kind = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.rescued = torch.zeros(N, **i32)
        self.carried = torch.zeros(N, **i32)
        self.carrying = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.closest = torch.full((N,), float("inf"), **f64)
        # attributes the reference creates lazily and never clears (quirk B3): -1 / NaN = absent
        self.prev_rescued = torch.full((N,), -1, **i32)
        self.prev_carried = torch.full((N,), -1, **i32)
        self.prev_sz = torch.full((N,), float("nan"), **f64)
        self.fall_timer = torch.full((N,), -1, **i32)
        self.victims_rescued = torch.zeros(N, **i32)
        self.distance = torch.zeros(N, **f64)
        self.ttfr = torch.full((N,), float("nan"), **f64)
        self.falls = torch.zeros(N, **i32)
        self.collisions = torch.zeros(N, **i32)
        self.prev_robot_pos = torch.zeros(N, 3, **f64)
        self.rollout = torch.zeros(N, 4, dtype=self.batch.dtype, device=dev)
        self._bind(self.step_count, self.energy, self.energy_used, self.rescued, self.carried, self.carrying,
                   self.closest, self.prev_rescued, self.prev_carried, self.prev_sz, self.fall_timer,
                   self.victims_rescued, self.distance, self.ttfr, self.falls, self.collisions, self.prev_robot_pos,
                   self.episode, self.rollout, energy_kind=self.energy_kind)
        if staged:
            self._stage(banks)
        self.action_space = Box(low=-ACTION_LIMIT, high=ACTION_LIMIT, shape=(N_ACT,), dtype=np.float32)

    def info(self) -> Dict[str, Any]:
        """Device-tensor views of the reference's info dict (rescue_env.py:447-456); views only, so
        the step path launches no extra kernels."""
        return {
            'victims_rescued': self.victims_rescued,
            'distance_traveled': self.distance,
            'energy_used': self.energy_used,
            'time_to_first_rescue': self.ttfr,
            'falls': self.falls,
            'collisions': self.collisions,
            'robot_position': self.prev_robot_pos,
            'victims_rescued_mask': self.rescued,   # victims_remaining = 5 - popcount (views only)
            'victims_carried_mask': self.carried,
            'energy_remaining': self.energy,
            'final_observation': self.final_obs,
            'episode': self.episode,
            'bad_state_resets': self.batch.warning,
        }


def _popcount5(x: torch.Tensor) -> torch.Tensor:
    c = torch.zeros_like(x)
    for b in range(5):
        c += (x >> b) & 1
    return c


class BipedalRescueEnv(TaskEnv):
    """Drop-in for bipedal_rescue_env.rescue_env.BipedalRescueEnv, simulated by libmgx."""

    metadata = {'render_modes': ['human', 'rgb_array', 'depth_array'], 'render_fps': 50}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64",
                 render_camera=None, render_size=(480, 640), **kwargs):
        super().__init__()
        self._render_setup(render_camera, render_size)
        self.render_mode = render_mode
        self.dt = 0.02
        self.max_episode_steps = MAX_EPISODE_STEPS
        self.world_size = 50.0
        self.safe_zone_radius = 3.0
        self.safe_zone_pos = SAFE_ZONE_POS.copy()
        self.robot_height = 1.2
        self.carry_capacity = 2
        self.energy_limit = ENERGY_LIMIT
        self.num_victims = 5
        self.victim_weights = [60, 30, 50, 55, 65]
        self.victim_priorities = [0.8, 1.0, 0.7, 0.9, 1.0]
        self.fire_zones = [{'pos': np.array([-5.0, -3.0, 0.0]), 'radius': 1.5},
                           {'pos': np.array([8.0, 6.0, 0.0]), 'radius': 1.2}]
        # one env on the staged RK4 pipeline at the model's full capacity (192 contacts / 768 rows; the
        # monolithic kernel holds 512 rows), reset() settled by the same stages, no reset banks
        self._vec = BipedalVectorEnv(1, device=device, precision=precision, autoreset=False,
                                     max_episode_steps=self.max_episode_steps, staged=True, banks=0)
        self.model = self._vec.model
        self.num_actuators = N_ACT
        self.action_space = Box(low=-ACTION_LIMIT, high=ACTION_LIMIT, shape=(N_ACT,), dtype=np.float32)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(OBS_DIM,), dtype=np.float32)
        self.viewer = None
        self.np_random = None
        self.current_step = 0
        self.seed()

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        obs = self._reset_vec(seed)
        self.current_step = 0
        info = self._info()
        return obs, {k: info[k] for k in ('episode_stats', 'robot_position', 'victims_remaining', 'energy_remaining')}

    def step(self, action: np.ndarray):
        out = self._step_vec(action)
        self.current_step = int(self._vec.step_count[0])
        return (*out, self._info())

    def _info(self) -> Dict[str, Any]:
        v = self._vec
        ttfr = float(v.ttfr[0])
        stats = {'victims_rescued': int(v.victims_rescued[0]), 'distance_traveled': float(v.distance[0]),
                 'energy_used': self._energy_type()(v.energy_used[0].item()),
                 'time_to_first_rescue': None if np.isnan(ttfr) else ttfr,
                 'falls': int(v.falls[0]), 'collisions': int(v.collisions[0])}
        up = v.obs[0, 55:59].double().cpu().numpy()
        w, x, y, z = up
        return {'episode_stats': stats, 'robot_position': v.prev_robot_pos[0].cpu().numpy().copy(),
                'victims_remaining': 5 - bin(int(v.rescued[0])).count("1"),
                'victims_carried': bin(int(v.carried[0])).count("1"),
                'energy_remaining': self._energy_type()(v.energy[0].item()),
                'robot_upright': bool(w * w - x * x - y * y + z * z > 0.7)}

    def _energy_type(self):
        """numpy type of current_energy / energy_used: a Python float after reset, np.float32 after
        float32 actions, np.float64 once a float64 action's cost was subtracted"""
        return {0: float, 1: np.float64, 2: np.float32}[int(self._vec.energy_kind[0])]


def register_envs() -> bool:
    """Register BipedalRescue-v0 with gymnasium when installed (rescue_env.py:793-804)."""
    try:
        import gymnasium as gym  # type: ignore
    except Exception:  # noqa: BLE001
        return False
    try:
        gym.register(id='BipedalRescue-v0', entry_point='mujoco_gymnasium_environments_amd.envs.bipedal:BipedalRescueEnv',
                     max_episode_steps=10000, reward_threshold=20000.0)
    except Exception:  # noqa: BLE001 - already registered
        pass
    return True
