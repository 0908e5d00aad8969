"""quadruped_parkour_env on MI355X: a batched VectorEnv and a drop-in gymnasium-style Env.

Mirrors the reference interface quadruped_parkour_env/parkour_env.py:
  * ``QuadrupedParkourEnv`` — same constructor / ``reset(seed, options)`` / ``step(action)`` /
    spaces / ``metadata`` / ``render`` / ``close`` surface as ``QuadrupedParkourEnv``
    (parkour_env.py:20-866), batch size 1, gymnasium seeding (PCG64 over SeedSequence) and the
    same two obstacle draws per reset (:757-774).
  * ``ParkourVectorEnv`` — N envs on one GPU, device tensors ``[N, ...]``, same-step autoreset
    with Philox reset draws keyed by (seed, global env index, episode).
Both run one fused HIP launch per env step (libmgx.so ``mgx_parkour_step``): action clip,
10 mj_step's of 1 ms, obstacle motors, observation / reward / termination for every env.
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
from .sharded import StreamShardedEnv

ASSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "quadruped_parkour.xml")

# parkour_env.py:194-199
JOINT_NAMES = [
    'fl_hip_abduction', 'fl_hip_flexion', 'fl_knee', 'fl_ankle',
    'fr_hip_abduction', 'fr_hip_flexion', 'fr_knee', 'fr_ankle',
    'bl_hip_abduction', 'bl_hip_flexion', 'bl_knee', 'bl_ankle',
    'br_hip_abduction', 'br_hip_flexion', 'br_knee', 'br_ankle']
OBS_DIM = 95
MAX_EPISODE_STEPS = 6000          # parkour_env.py:41
START_POS = np.array([2.0, 0.0, 0.6])
FINISH_POS = np.array([98.0, 0.0, 0.0])


def parkour_model(rows_in_scratch: Optional[bool] = None) -> mjcf.Model:
    """The compiled model; rows_in_scratch None = the MGX_PARKOUR_ROWS_LDS environment variable, read at
    each call (not once per process), and part of the cache key."""
    if rows_in_scratch is None:
        rows_in_scratch = os.environ.get("MGX_PARKOUR_ROWS_LDS", "0") != "1"
    return _parkour_model(bool(rows_in_scratch))


# Contact / row capacity. MuJoCo keeps every contact; the oracle census at the bench's actions
# (tools/capacity_census.py --task parkour: 128 envs x 1000 env steps, 1.28M mj_steps, U(-lim, lim),
# autoreset) peaks at 80 contacts / 338 rows — the qpos0 pile-up after each of MuJoCo's bad-state
# resets (8.6% of env steps) — against 15 rows at the median, so the round-1 default of 64 / 192
# dropped rows on every such step. 96 / 384 holds the census maximum (Capacity).
CON_CAPACITY = 96
EFC_CAPACITY = 384


@functools.lru_cache(maxsize=None)
def _parkour_model(rows_in_scratch: bool) -> mjcf.Model:
    with open(ASSET) as f:
        m = mjcf.compile_xml(f.read())
    m.con_capacity = CON_CAPACITY
    m.efc_capacity = EFC_CAPACITY
    # constraint rows in per-env global scratch: 48 -> 32 KiB LDS per env (fp32), five envs per CU
    # instead of three; 27.6 -> 22.2 ms per step at 4096 envs.
    # MGX_PARKOUR_ROWS_LDS=1 keeps them in LDS.
    if rows_in_scratch:
        m.layout_flags = cabi.MGX_ROWS_IN_SCRATCH
    return m


def action_limits() -> np.ndarray:
    """hip +-80, knee +-60, ankle +-40 N m (parkour_env.py:236-249)"""
    return np.array([80.0 if 'hip' in n else 60.0 if 'knee' in n else 40.0 for n in JOINT_NAMES])


class ParkourTables:
    """Index tables looked up exactly as parkour_env.py:180-222 and :757-795 do."""

    def __init__(self, m: mjcf.Model, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.model = m
        self.torso = m.name2id("body", "torso")
        self.feet = [m.name2id("body", f"{k}_foot") for k in ("fl", "fr", "bl", "br")]
        self.joint_ids = [m.name2id("joint", n) for n in JOINT_NAMES]
        self.actuator_ids = [m.name2id("actuator", n + "_motor") for n in JOINT_NAMES]
        # joint ids used as qpos indices by _randomize_obstacles (quirk P1)
        self.platform_qpos = m.name2id("joint", "platform_slide")
        self.pendulum_qpos = m.name2id("joint", "pendulum_swing")
        self.platform_act = m.name2id("actuator", "platform_motor")
        self.pendulum_act = m.name2id("actuator", "pendulum_motor")
        self.max_episode_steps = max_episode_steps

    def ids_struct(self) -> cabi.MgxParkourIds:
        s = cabi.MgxParkourIds()
        s.torso = self.torso
        for i, f in enumerate(self.feet):
            s.feet[i] = f
        s.platform_qpos, s.pendulum_qpos = self.platform_qpos, self.pendulum_qpos
        s.platform_act, s.pendulum_act = self.platform_act, self.pendulum_act
        s.n_leg = 16
        s.max_episode_steps = self.max_episode_steps
        for i, v in enumerate(action_limits()):
            s.act_lim[i] = float(v)
        return s

    @staticmethod
    def reset_draws(rng: np.random.Generator) -> np.ndarray:
        """The 2 uniform draws of one reset, in reference order (parkour_env.py:764,772)."""
        return np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0)])


class ParkourVectorEnv(TaskVectorEnv):
    """``num_envs`` quadruped_parkour envs stepping in lockstep on one GPU, 10 physics substeps per
    env step. ``step(actions)`` takes [N, 16] float32, or float64: a float64 action is clipped and
    applied in float64 and its effort term follows in float64 (parkour_env.py:360-364, :702);
    ``reset(draws=)`` takes [N, 2]."""

    metadata = {'render_modes': [], 'render_fps': 100}
    TASK, ENV_STRUCT, OBS_DIM, N_DRAWS = "parkour", cabi.MgxParkourEnv, OBS_DIM, 2

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0,
                 rows_in_scratch: Optional[bool] = None, staged: bool = True, banks: int = 1):
        """``staged`` selects the per-substep row builder / lane-group PGS / finisher kernels with
        ``banks`` precomputed resets per env (one covers every autoreset: a bank settles within one
        env step); ``staged=False`` runs one wave per env for the whole env step. Both compute the
        same step (tests/test_gpu_parkour.py)."""
        model = parkour_model(rows_in_scratch)
        self._setup(num_envs, device, precision, model, ParkourTables(model, max_episode_steps), autoreset, seed,
                    env_offset)
        dt, dev, N = self.batch.dtype, self.device, num_envs
        self.last_position = torch.zeros(N, 3, dtype=dt, device=dev)
        self.max_progress = torch.zeros(N, dtype=dt, device=dev)
        self.episode_reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.er_kind = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.reached = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fall_count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.stuck = torch.zeros(N, dtype=torch.int32, device=dev)
        self.step_count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rollout = torch.zeros(N, 4, dtype=dt, device=dev)
        self._bind(self.last_position, self.max_progress, self.episode_reward, self.er_kind, self.reached,
                   self.fall_count, self.stuck, self.step_count, self.episode, self.rollout)
        if staged:
            # not for a model / hook configuration the staged pipeline does not take (e.g. a solver
            # layout that would need a second launch): the monolithic step computes the same physics
            # at the same capacity (tests/test_gpu_parkour.py runs both)
            self._stage(banks, optional=True)
        lim = action_limits()
        self.action_space = Box(low=-lim, high=lim, dtype=np.float32)

    def info(self) -> Dict[str, Any]:
        """Device-tensor views of the reference's info dict (parkour_env.py:797-815). Views only
        (no kernels on the step path): ``reached_mask`` holds checkpoints_reached as a bitmask
        (``checkpoints_reached()`` counts it) and ``last_position`` the torso position
        course_completion derives from (``course_completion()``)."""
        return {
            'step_count': self.step_count,
            'episode_reward': self.episode_reward,
            'max_forward_progress': self.max_progress,
            'reached_mask': self.reached,
            'fall_count': self.fall_count,
            'last_position': self.last_position,
            'final_observation': self.final_obs,
            'episode': self.episode,
            'bad_state_resets': self.batch.warning,
        }

    def checkpoints_reached(self) -> torch.Tensor:
        return _popcount(self.reached)

    def course_completion(self) -> torch.Tensor:
        x = self.last_position[:, 0].double()
        return ((x - START_POS[0]) / (FINISH_POS[0] - START_POS[0])).clamp(0.0, 1.0)


class StreamShardedParkourEnv(StreamShardedEnv):
    """``num_envs`` parkour envs as ``n_streams`` shards on their own HIP streams (envs/sharded.py):
    one shard's row builder fills the CUs another shard's solver leaves idle while its few
    heaviest slots (up to 338 rows at bench conditions) finish their Gauss–Seidel chains. Same
    trajectories as one ParkourVectorEnv over all envs (tests/test_gpu_parkour.py)."""

    def __init__(self, num_envs: int, n_streams: int = 2, device: str = "cuda:0", precision: str = "f64",
                 seed: int = 0, max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True,
                 env_offset: int = 0, staged: bool = True, banks: int = 1):
        super().__init__(lambda n, off: ParkourVectorEnv(n, device=device, precision=precision, seed=seed,
                                                         max_episode_steps=max_episode_steps, autoreset=autoreset,
                                                         env_offset=env_offset + off, staged=staged, banks=banks),
                         num_envs, n_streams, device)

    def checkpoints_reached(self) -> torch.Tensor:
        return torch.cat([s.checkpoints_reached() for s in self.shards])

    def course_completion(self) -> torch.Tensor:
        return torch.cat([s.course_completion() for s in self.shards])


def _popcount(x: torch.Tensor) -> torch.Tensor:
    c = torch.zeros_like(x)
    for b in range(18):
        c += (x >> b) & 1
    return c


class QuadrupedParkourEnv(TaskEnv):
    """Drop-in for quadruped_parkour_env.parkour_env.QuadrupedParkourEnv, simulated by libmgx."""

    metadata = {'render_modes': ['human', 'rgb_array'], 'render_fps': 100}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64",
                 render_camera=None, render_size=(480, 640), **kwargs):
        super().__init__()
        self._render_setup(render_camera, render_size)
        self.render_mode = render_mode
        self.dt = 0.01
        self.frame_skip = 10
        self.max_episode_steps = MAX_EPISODE_STEPS
        self.course_length = 100.0
        self.course_width = 20.0
        self.start_pos = START_POS.copy()
        self.finish_pos = FINISH_POS.copy()
        self._vec = ParkourVectorEnv(1, device=device, precision=precision, autoreset=False,
                                     max_episode_steps=self.max_episode_steps)
        self.model = self._vec.model
        self.checkpoint_positions = [15, 30, 45, 60, 75, 90]
        lim = action_limits()
        self.action_space = Box(low=-lim, high=lim, dtype=np.float32)
        low = np.full(OBS_DIM, -np.inf, dtype=np.float32)
        high = np.full(OBS_DIM, np.inf, dtype=np.float32)
        # parkour_env.py:266-291 (declared bounds; lidar bounds sit at 64:88 as in the reference)
        low[0:16], high[0:16] = -np.pi, np.pi
        low[16:32], high[16:32] = -20.0, 20.0
        low[32:36], high[32:36] = -1.0, 1.0
        low[48:52], high[48:52] = 0.0, 1.0
        low[64:88], high[64:88] = 0.0, 10.0
        self.observation_space = Box(low=low, high=high, dtype=np.float32)
        self.viewer = None
        self.np_random = None
        self.step_count = 0
        self.seed()

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        obs = self._reset_vec(seed)
        self.step_count = 0
        return obs, self._info()

    def step(self, action: np.ndarray):
        out = self._step_vec(action)
        self.step_count = int(self._vec.step_count[0])
        return (*out, self._info())

    def _info(self) -> Dict[str, Any]:
        v = self._vec
        x = float(v.last_position[0, 0])
        return {
            'step_count': int(v.step_count[0]),
            'episode_reward': float(v.episode_reward[0]),
            'max_forward_progress': float(v.max_progress[0]),
            'checkpoints_reached': int(bin(int(v.reached[0])).count("1")),
            'fall_count': int(v.fall_count[0]),
            'course_completion': min(1.0, max(0.0, (x - self.start_pos[0]) / (self.finish_pos[0] - self.start_pos[0]))),
        }

    def render(self):
        if self._render_camera is not None:
            return super().render()
        if self.render_mode == 'rgb_array':
            return np.zeros((480, 640, 3), dtype=np.uint8)  # parkour_env.py:835-837
        return None


def register_envs() -> bool:
    """Register QuadrupedParkour-v0/v1 with gymnasium when installed (quadruped_parkour_env/__init__.py:16-34)."""
    try:
        import gymnasium as gym  # type: ignore
    except Exception:  # noqa: BLE001
        return False
    for vid, thr, mode in (('QuadrupedParkour-v0', 8000.0, None), ('QuadrupedParkour-v1', 10000.0, 'human')):
        try:
            gym.register(id=vid, entry_point='mujoco_gymnasium_environments_amd.envs.parkour:QuadrupedParkourEnv',
                         max_episode_steps=6000, reward_threshold=thr, kwargs={'render_mode': mode})
        except Exception:  # noqa: BLE001 - already registered
            pass
    return True
