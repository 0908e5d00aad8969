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

import ctypes as C
import functools
import os
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from .. import cabi, mjcf
from ..batch import PhysicsBatch, _ptr, stream_handle
from ..native import NativeError, check, lib
from ..dynamics import DynamicsForwarding
from ..rollouts import RolloutForwarding
from ..transitions import TransitionForwarding
from ..rays import RayForwarding
from ..sensors import SensorForwarding
from ..seeding import np_random
from ..spaces import Box, EnvBase, policy_action
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


class ParkourVectorEnv(RayForwarding, SensorForwarding, DynamicsForwarding, TransitionForwarding, RolloutForwarding):
    """``num_envs`` quadruped_parkour envs stepping in lockstep on one GPU."""

    metadata = {'render_modes': [], 'render_fps': 100}

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0,
                 rows_in_scratch: Optional[bool] = None, staged: bool = True, banks: int = 1):
        """``staged`` selects the per-substep row builder / lane-group PGS / finisher kernels with
        ``banks`` precomputed resets per env (one covers every autoreset: a bank settles within one
        env step); ``staged=False`` runs one wave per env for the whole env step. Both compute the
        same step (tests/test_gpu_parkour.py)."""
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.model = parkour_model(rows_in_scratch)
        self.tables = ParkourTables(self.model, max_episode_steps)
        self.batch = PhysicsBatch(self.model, num_envs, precision=precision, device=device)
        self.native = self.batch.native
        self.autoreset = autoreset
        self.seed_value = int(seed) & ((1 << 64) - 1)
        self.env_offset = env_offset
        dt, dev, N = self.batch.dtype, self.device, num_envs
        self.last_position = torch.zeros(N, 3, dtype=dt, device=dev)
        self.max_progress = torch.zeros(N, dtype=dt, device=dev)
        self.episode_reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.er_kind = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.reached = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fall_count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.stuck = torch.zeros(N, dtype=torch.int32, device=dev)
        self.step_count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.episode = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rollout = torch.zeros(N, 4, dtype=dt, device=dev)
        self.obs = torch.zeros(N, OBS_DIM, dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros(N, OBS_DIM, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.terminated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._env = cabi.MgxParkourEnv(*[t.data_ptr() for t in (
            self.last_position, self.max_progress, self.episode_reward, self.er_kind, self.reached, self.fall_count,
            self.stuck, self.step_count, self.episode, self.rollout)])
        ids = self.tables.ids_struct()
        check(lib().mgx_parkour_configure(self.native.handle, C.byref(ids)), "mgx_parkour_configure")
        self.workspace = None
        nb = int(lib().mgx_parkour_workspace_bytes(self.native.handle, N, banks)) if staged else 0
        if staged and nb == cabi.MGX_E_UNSUPPORTED:
            # a model / hook configuration the staged pipeline does not take (e.g. a solver layout
            # that would need a second launch): the monolithic step computes the same physics at
            # the same capacity (tests/test_gpu_parkour.py runs both)
            staged = False
        self.staged = staged
        if staged:
            if nb <= 0:
                raise NativeError(f"mgx_parkour_workspace_bytes: {lib().mgx_last_error().decode()}")
            self.workspace = torch.empty(nb, dtype=torch.uint8, device=dev)
            check(lib().mgx_parkour_workspace_init(self.native.handle, _ptr(self.workspace), nb, N, banks, None),
                  "mgx_parkour_workspace_init")
            self._env.workspace = self.workspace.data_ptr()
            self._env.workspace_bytes = nb
            self._env.banks = banks
        lim = action_limits()
        self.action_space = Box(low=-lim, high=lim, dtype=np.float32)

    def reset(self, seed: Optional[int] = None, env_mask: Optional[torch.Tensor] = None,
              draws: Optional[np.ndarray] = None, stream=None) -> Tuple[torch.Tensor, Dict[str, Any]]:
        """reset() for all (or masked) envs. ``draws`` [N,2] (host, reference order) gives exact
        gymnasium seeding; otherwise device Philox draws keyed by (seed, env, episode)."""
        if seed is not None:
            self.seed_value = int(seed) & ((1 << 64) - 1)
            self.episode.zero_()
        d = None
        if draws is not None:
            d = torch.as_tensor(np.asarray(draws).reshape(self.num_envs, 2), dtype=self.batch.dtype).to(self.device)
        check(lib().mgx_parkour_reset(self.native.handle, C.byref(self.batch.state), C.byref(self._env), _ptr(d),
                                      _ptr(self.obs), self.seed_value, self.env_offset, self.num_envs, _ptr(env_mask),
                                      stream_handle(stream)), "mgx_parkour_reset")
        return self.obs, self.info()

    def step(self, actions: torch.Tensor, stream=None):
        """One env step (10 physics substeps) for every env. ``actions`` [N, 16] float32, or float64:
        a float64 action is clipped and applied in float64 and its effort term follows in float64,
        as the reference's np.clip keeps a float64 policy's dtype (parkour_env.py:360-364, :702)."""
        dt = torch.float64 if actions.dtype == torch.float64 else torch.float32
        if actions.dtype != dt or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=dt).contiguous()
        assert actions.shape == (self.num_envs, 16), actions.shape
        self._env.action_f64 = 1 if dt == torch.float64 else 0
        check(lib().mgx_parkour_step(self.native.handle, C.byref(self.batch.state), C.byref(self._env),
                                     _ptr(actions), _ptr(self.obs), _ptr(self.reward), _ptr(self.terminated),
                                     _ptr(self.truncated), _ptr(self.final_obs) if self.autoreset else None,
                                     1 if self.autoreset else 0, self.seed_value, self.env_offset, self.num_envs,
                                     None, stream_handle(stream)), "mgx_parkour_step")
        return self.obs, self.reward, self.terminated, self.truncated, self.info()

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

    def close(self):
        pass


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


class QuadrupedParkourEnv(EnvBase):
    """Drop-in for quadruped_parkour_env.parkour_env.QuadrupedParkourEnv, simulated by libmgx."""

    metadata = {'render_modes': ['human', 'rgb_array'], 'render_fps': 100}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64", **kwargs):
        super().__init__()
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

    def seed(self, seed: Optional[int] = None) -> list:
        self.np_random, seed = np_random(seed)
        return [seed]

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        if seed is not None:
            self.seed(seed)
        draws = self._vec.tables.reset_draws(self.np_random)[None]
        obs, _ = self._vec.reset(draws=draws)
        torch.cuda.synchronize(self._vec.device)
        self.step_count = 0
        return obs[0].cpu().numpy().copy(), self._info()

    def step(self, action: np.ndarray):
        a = torch.from_numpy(policy_action(action).reshape(1, -1)).to(self._vec.device)  # clipped on the device
        obs, rew, term, trunc, _ = self._vec.step(a)
        torch.cuda.synchronize(self._vec.device)
        self.step_count = int(self._vec.step_count[0])
        return obs[0].cpu().numpy().copy(), float(rew[0]), bool(term[0]), bool(trunc[0]), self._info()

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
        if self.render_mode == 'rgb_array':
            return np.zeros((480, 640, 3), dtype=np.uint8)  # parkour_env.py:835-837
        return None

    def close(self):
        self.viewer = None


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
