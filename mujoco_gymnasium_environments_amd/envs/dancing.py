"""humanoid_dancing_env on MI355X (a BASELINE configs[4] task): a batched VectorEnv and a drop-in
gymnasium-style Env.

Mirrors the reference interface humanoid_dancing_env/dancing_env.py:
  * ``HumanoidDancingEnv`` — same constructor / ``reset(seed, options)`` / ``step(action)`` /
    spaces / ``metadata`` / ``render`` / ``close`` / ``info`` surface as the reference class
    (dancing_env.py:33-1306), batch size 1, gymnasium seeding (PCG64 over SeedSequence) and the
    same 40 sequence draws per reset (:896-905; Generator.choice over the 10 move names draws
    integers(0, 10)).
  * ``DancingVectorEnv`` — N envs on one GPU, device tensors ``[N, ...]``, same-step autoreset
    with Philox reset draws keyed by (seed, global env index, episode).
Both run one fused HIP launch per env step (libmgx.so ``mgx_dancing_step``): clip, rhythm,
spotlight, one RK4 mj_step, observation / reward / termination / stats / crowd / move transition.

The composed model is the string the reference constructor compiles (dancing_env.py:156-678,
tests/golden/make_fixtures.py): RK4 (dancing_env.py:179), PGS, nq = nv = nu = 29 (no root
joint: the torso hangs from the world through the abdomen hinges), 16 bodies, 17 geoms
(cylinder dance floor and stage), 106 candidate pairs.
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

ASSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "humanoid_dancing.xml")
MOVES = ['basic_step', 'spin', 'jump', 'moonwalk', 'robot_wave', 'freeze', 'hip_hop_bounce', 'breakdance_toprock',
         'salsa_basic', 'ballet_pirouette']                         # dancing_env.py:57-68
DIFFICULTY = [1, 2, 2, 3, 2, 1, 2, 3, 2, 4]
STYLE_POINTS = [10, 20, 25, 40, 30, 15, 25, 35, 28, 50]
ENERGY = [0.5, 1.0, 1.5, 0.8, 0.6, 0.2, 0.7, 1.2, 0.8, 1.0]
JOINT_NAMES = [
    'abdomen_x', 'abdomen_y', 'abdomen_z', 'neck_x', 'neck_y',
    'right_shoulder1', 'right_shoulder2', 'right_elbow', 'right_wrist_x', 'right_wrist_y', 'right_wrist_z',
    'left_shoulder1', 'left_shoulder2', 'left_elbow', 'left_wrist_x', 'left_wrist_y', 'left_wrist_z',
    'right_hip_x', 'right_hip_y', 'right_hip_z', 'right_knee', 'right_ankle_x', 'right_ankle_y',
    'left_hip_x', 'left_hip_y', 'left_hip_z', 'left_knee', 'left_ankle_x', 'left_ankle_y']   # :684-694
OBS_DIM = 94
N_ACT = 29
SEQ_LEN = 20
MAX_EPISODE_STEPS = 3600            # dancing_env.py:42
ACTION_LIMIT = 200.0                # dancing_env.py:725-730
DT = 0.01667
BEAT = 0.5


def dancing_model(rows_in_scratch: Optional[bool] = None) -> mjcf.Model:
    """The compiled model; rows_in_scratch None = the MGX_DANCING_ROWS_LDS environment variable, read at
    each call (not once per process), and part of the cache key."""
    if rows_in_scratch is None:
        rows_in_scratch = os.environ.get("MGX_DANCING_ROWS_LDS", "0") != "1"
    return _dancing_model(bool(rows_in_scratch))


@functools.lru_cache(maxsize=None)
def _dancing_model(rows_in_scratch: bool) -> mjcf.Model:
    with open(ASSET) as f:
        m = mjcf.compile_xml(f.read())
    # constraint rows in per-env global scratch: 41 -> 25 KiB LDS per env (fp32), six envs per CU
    # instead of three. MGX_DANCING_ROWS_LDS=1 keeps them in LDS.
    if rows_in_scratch:
        m.layout_flags = cabi.MGX_ROWS_IN_SCRATCH
    # contact / row capacity: the library default, 64 contacts / 192 rows. The oracle census at the
    # bench's U(-200, 200) actions (tools/capacity_census.py --task dancing: 32 envs x 500 env steps,
    # autoreset) peaks at 29 contacts / 121 rows, so MuJoCo's arena never holds more than this does
    # (Capacity); the bench line counts any overflowing step.
    return m


class DancingTables:
    """Index tables looked up exactly as dancing_env.py:680-720 does."""

    def __init__(self, m: mjcf.Model, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.model = m
        self.torso = m.name2id("body", "torso")
        self.right_foot = m.name2id("geom", "right_foot")
        self.left_foot = m.name2id("geom", "left_foot")
        self.floor = m.name2id("geom", "dance_floor")
        self.stage = m.name2id("geom", "stage")
        self.joints = [m.name2id("joint", n) for n in JOINT_NAMES]
        self.max_episode_steps = max_episode_steps

    def ids_struct(self) -> cabi.MgxDancingIds:
        m, s = self.model, cabi.MgxDancingIds()
        s.torso, s.right_foot, s.left_foot, s.floor, s.stage = (self.torso, self.right_foot, self.left_foot,
                                                                self.floor, self.stage)
        s.n_act = N_ACT
        s.max_episode_steps = self.max_episode_steps
        # observation slot i normalises qpos[7 + i] with the range of joint_indices[i]
        s.n_range = min(len(self.joints), m.njnt)
        for i, j in enumerate(self.joints[:s.n_range]):
            s.jnt_lo[i], s.jnt_hi[i] = float(m.jnt_range[j][0]), float(m.jnt_range[j][1])
        return s

    @staticmethod
    def reset_draws(rng: np.random.Generator) -> np.ndarray:
        """The 40 draws of one reset in reference order: (move index, duration) x 20."""
        d = []
        for _ in range(SEQ_LEN):
            d += [float(rng.integers(0, 10)), rng.uniform(1.0, 3.0)]
        return np.array(d)


class DancingVectorEnv(TaskVectorEnv):
    """``num_envs`` humanoid_dancing envs stepping in lockstep on one GPU, one RK4 mj_step per env
    step. ``step(actions)`` takes [N, 29]; ``reset(draws=)`` takes [N, 40]."""

    metadata = {'render_modes': [], 'render_fps': 60}
    TASK, ENV_STRUCT, OBS_DIM, N_DRAWS = "dancing", cabi.MgxDancingEnv, OBS_DIM, 2 * SEQ_LEN

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0,
                 rows_in_scratch: Optional[bool] = None):
        model = dancing_model(rows_in_scratch)
        self._setup(num_envs, device, precision, model, DancingTables(model, max_episode_steps), autoreset, seed,
                    env_offset)
        dev, N = self.device, num_envs
        self.scal = torch.zeros(N, 18, dtype=torch.float64, device=dev)
        self.scal[:, 2:5] = torch.tensor([0.0, 0.0, 5.0], dtype=torch.float64)   # spotlight (dancing_env.py:95)
        self.scal[:, 5] = 1.0
        self.scal[:, 8] = 0.5
        self.ints = torch.zeros(N, 8, dtype=torch.int32, device=dev)
        self.hist = torch.full((N, 3), -1, dtype=torch.int32, device=dev)
        self.moves = torch.zeros(N, SEQ_LEN, dtype=torch.int32, device=dev)
        self.durations = torch.zeros(N, SEQ_LEN, dtype=torch.float64, device=dev)
        self.prev_jvel = torch.zeros(N, self.model.nv - 6, dtype=torch.float64, device=dev)
        self.rollout = torch.zeros(N, 4, dtype=self.batch.dtype, device=dev)
        self._bind(self.scal, self.ints, self.hist, self.moves, self.durations, self.prev_jvel, self.episode,
                   self.rollout)
        self.action_space = Box(low=-ACTION_LIMIT, high=ACTION_LIMIT, shape=(N_ACT,), dtype=np.float32)

    @property
    def step_count(self) -> torch.Tensor:
        return self.ints[:, 0]

    def info(self) -> Dict[str, Any]:
        """Device-tensor views of the reference's info dict (dancing_env.py:868-878)."""
        return {
            'time_since_last_beat': self.scal[:, 0],   # beat_phase = / 0.5 (views only)
            'combo_multiplier': self.scal[:, 5],
            'crowd_excitement': self.scal[:, 8],
            'performance_score': self.scal[:, 6],
            'energy_used': self.scal[:, 10],
            'time_on_beat': self.scal[:, 11],
            'longest_combo': self.scal[:, 12],
            'current_move_idx': self.ints[:, 3],
            'final_observation': self.final_obs,
            'episode': self.episode,
            'bad_state_resets': self.batch.warning,
        }


class HumanoidDancingEnv(TaskEnv):
    """Drop-in for humanoid_dancing_env.dancing_env.HumanoidDancingEnv, simulated by libmgx."""

    metadata = {'render_modes': ['human', 'rgb_array'], 'render_fps': 60}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64",
                 render_camera=None, render_size=(480, 640), **kwargs):
        super().__init__()
        self._render_setup(render_camera, render_size)
        self.render_mode = render_mode
        self.dt = DT
        self.max_episode_steps = MAX_EPISODE_STEPS
        self.floor_radius = 10.0
        self.stage_height = 0.5
        self.bpm = 120
        self.beat_interval = BEAT
        self.dance_moves = {n: {'difficulty': DIFFICULTY[i], 'energy': ENERGY[i], 'style_points': STYLE_POINTS[i]}
                            for i, n in enumerate(MOVES)}
        self._vec = DancingVectorEnv(1, device=device, precision=precision, autoreset=False,
                                     max_episode_steps=self.max_episode_steps)
        self.model = self._vec.model
        self.num_joints = N_ACT
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
        return obs, {'episode_stats': info['episode_stats'], 'current_move': self.dance_moves[MOVES[0]],
                     'beat_phase': 0.0, 'combo_multiplier': info['combo_multiplier']}

    def step(self, action: np.ndarray):
        out = self._step_vec(action)
        self.current_step = int(self._vec.ints[0, 0])
        return (*out, self._info())

    def _info(self) -> Dict[str, Any]:
        v = self._vec
        sc = v.scal[0].cpu().numpy()
        it = v.ints[0].cpu().numpy()
        stats = {'total_score': float(sc[14]), 'perfect_moves': 0, 'good_moves': 0, 'missed_beats': 0,
                 'longest_combo': int(sc[12]), 'energy_used': float(sc[10]), 'time_on_beat': float(sc[11]),
                 'creativity_score': 0.0, 'crowd_rating': float(sc[13])}
        return {'episode_stats': stats, 'current_move': self.dance_moves[MOVES[int(it[3]) % len(MOVES)]],
                'beat_phase': float(sc[0]) / BEAT, 'combo_multiplier': float(sc[5]),
                'crowd_excitement': float(sc[8]), 'performance_score': float(sc[6])}


def register_envs() -> bool:
    """Register HumanoidDancing-v0 with gymnasium when installed (dancing_env.py:1308-1320)."""
    try:
        import gymnasium as gym  # type: ignore
    except Exception:  # noqa: BLE001
        return False
    try:
        gym.register(id='HumanoidDancing-v0',
                     entry_point='mujoco_gymnasium_environments_amd.envs.dancing:HumanoidDancingEnv',
                     max_episode_steps=3600, reward_threshold=5000.0)
    except Exception:  # noqa: BLE001 - already registered
        pass
    return True
