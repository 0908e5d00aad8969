"""humanoid_martial_arts_env on MI355X: a batched VectorEnv and a drop-in gymnasium-style Env.

Mirrors the reference interface humanoid_martial_arts_env/martial_arts_env.py:
  * ``HumanoidMartialArtsEnv`` — same constructor / ``reset(seed, options)`` / ``step(action)`` /
    spaces / ``metadata`` / ``render`` / ``close`` surface (martial_arts_env.py:23-651), batch
    size 1, gymnasium seeding (PCG64 over SeedSequence) and the same two draws per reset (:460-463).
  * ``MartialArtsVectorEnv`` — N envs on one GPU, device tensors ``[N, ...]``, same-step autoreset
    with Philox reset draws keyed by (seed, global env index, episode).
Both run one fused HIP launch per env step (libmgx.so ``mgx_martial_step``): clip, ctrl =
action x ctrlrange, one mj_step with the Newton solver (martial_arts_scene.xml:163), observation /
reward / termination / statistics for every env.
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

ASSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets",
                     "humanoid_martial_arts.xml")
OBS_DIM = 113                 # what _get_observation returns (quirk M2)
DECLARED_OBS_DIM = 85         # observation_space (:408-420): 29 + 2 * nu
MAX_EPISODE_STEPS = 6000      # martial_arts_env.py:46
STAT_KEYS = ('techniques_performed', 'successful_combos', 'balance_maintained', 'max_power_generated',
             'total_distance_moved', 'falls')


def martial_model(rows_in_scratch: Optional[bool] = None) -> mjcf.Model:
    """The compiled model; rows_in_scratch None = the MGX_MARTIAL_ROWS_LDS environment variable, read at
    each call (not once per process), and part of the cache key."""
    if rows_in_scratch is None:
        rows_in_scratch = os.environ.get("MGX_MARTIAL_ROWS_LDS", "0") != "1"
    return _martial_model(bool(rows_in_scratch))


CON_CAPACITY = 96
EFC_CAPACITY = 384


@functools.lru_cache(maxsize=None)
def _martial_model(rows_in_scratch: bool) -> mjcf.Model:
    """The scene the reference's _generate_xml_files writes (martial_arts_env.py:150-381)."""
    with open(ASSET) as f:
        m = mjcf.compile_xml(f.read())
    m.layout_flags = cabi.MGX_KEEP_CVEL  # the observation and reward read cvel (:536-589)
    # contact / row capacity: the oracle census at the bench's U(-1, 1) actions
    # (tools/capacity_census.py --task martial: 128 envs x 1000 env steps, autoreset) peaks at 75
    # contacts / 320 rows, p99 208 rows — above the 64 / 192 default on ~1.5% of steps. MuJoCo keeps
    # them all; 96 / 384 holds the census maximum (Capacity).
    m.con_capacity = CON_CAPACITY
    m.efc_capacity = EFC_CAPACITY
    # constraint rows in per-env global scratch: the env's LDS drops from 65 to 30 KiB (fp32),
    # five envs per CU instead of two; MGX_MARTIAL_ROWS_LDS=1 keeps them in LDS
    if rows_in_scratch:
        m.layout_flags |= cabi.MGX_ROWS_IN_SCRATCH
    return m


class MartialTables:
    """Index tables looked up exactly as _get_model_indices does (martial_arts_env.py:383-395)."""

    def __init__(self, m: mjcf.Model, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.model = m
        self.torso = m.name2id("body", "torso")
        self.right_hand = m.name2id("body", "right_hand")
        self.left_hand = m.name2id("body", "left_hand")
        self.right_foot = m.name2id("body", "right_ankle")
        self.left_foot = m.name2id("body", "left_ankle")
        self.dummy1 = m.name2id("body", "dummy1")
        self.dummy2 = m.name2id("body", "dummy2")
        self.max_episode_steps = max_episode_steps

    def ids_struct(self) -> cabi.MgxMartialIds:
        m = self.model
        s = cabi.MgxMartialIds()
        s.torso, s.right_hand, s.left_hand = self.torso, self.right_hand, self.left_hand
        s.right_foot, s.left_foot, s.dummy1, s.dummy2 = self.right_foot, self.left_foot, self.dummy1, self.dummy2
        s.n_act = m.nu
        s.max_episode_steps = self.max_episode_steps
        for u in range(m.nu):
            s.ctrl_scale[u] = float(m.actuator_ctrlrange[u][1])
        return s

    @staticmethod
    def reset_draws(rng: np.random.Generator) -> np.ndarray:
        """The 2 uniform draws of one reset, in reference order (martial_arts_env.py:462-463)."""
        return np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])


class MartialArtsVectorEnv(TaskVectorEnv):
    """``num_envs`` humanoid_martial_arts envs stepping in lockstep on one GPU. ``step(actions)``
    takes [N, nu] in [-1, 1] (clipped); ``reset(draws=)`` takes [N, 2]."""

    metadata = {'render_modes': [], 'render_fps': 60}
    TASK, ENV_STRUCT, OBS_DIM, N_DRAWS = "martial", cabi.MgxMartialEnv, OBS_DIM, 2

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0,
                 rows_in_scratch: Optional[bool] = None):
        model = martial_model(rows_in_scratch)
        self._setup(num_envs, device, precision, model, MartialTables(model, max_episode_steps), autoreset, seed,
                    env_offset)
        dev, N = self.device, num_envs
        # stance_stability_time, total_distance_moved, prev_torso_pos[3] (fp64)
        self.scal = torch.zeros(N, 5, dtype=torch.float64, device=dev)
        # current_step, techniques_performed, falls, has prev_torso_pos
        self.ints = torch.zeros(N, 4, dtype=torch.int32, device=dev)
        self.rollout = torch.zeros(N, 4, dtype=torch.float64, device=dev)
        self._bind(self.scal, self.ints, self.episode, self.rollout)
        self.action_space = Box(low=-1.0, high=1.0, shape=(self.model.nu,), dtype=np.float32)

    def info(self) -> Dict[str, Any]:
        """Device-tensor views of the reference's info dict (martial_arts_env.py:623-630)."""
        return {
            'stance_stability': self.scal[:, 0],
            'total_distance_moved': self.scal[:, 1],
            'current_step': self.ints[:, 0],
            'techniques_performed': self.ints[:, 1],
            'falls': self.ints[:, 2],
            'final_observation': self.final_obs,
            'episode': self.episode,
            'bad_state_resets': self.batch.warning,
        }


class HumanoidMartialArtsEnv(TaskEnv):
    """Drop-in for humanoid_martial_arts_env.martial_arts_env.HumanoidMartialArtsEnv on libmgx.
    Actions are taken as float32 (the reference keeps the caller's dtype through np.clip; its
    energy term is float32 for float32 actions, e.g. action_space.sample())."""

    metadata = {'render_modes': ['human', 'rgb_array', 'depth_array'], 'render_fps': 60}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64",
                 render_camera=None, render_size=(480, 640), **kwargs):
        super().__init__()
        self._render_setup(render_camera, render_size)
        self.dt = 0.01667
        self.max_episode_steps = MAX_EPISODE_STEPS
        self.current_step = 0
        self.render_mode = render_mode
        self._vec = MartialArtsVectorEnv(1, device=device, precision=precision, autoreset=False,
                                         max_episode_steps=self.max_episode_steps)
        self.model = self._vec.model
        self.num_joints = self.model.nu
        self.combo_chain = []
        self.action_space = Box(low=-1.0, high=1.0, shape=(self.num_joints,), dtype=np.float32)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(DECLARED_OBS_DIM,), dtype=np.float32)
        self.viewer = None
        self.np_random = None
        self.seed()

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        obs = self._reset_vec(seed)
        self.current_step = 0
        return obs, self._info()

    def step(self, action: np.ndarray):
        out = self._step_vec(action)
        self.current_step = int(self._vec.ints[0, 0])
        return (*out, self._info())

    def _info(self) -> Dict[str, Any]:
        v = self._vec
        sc = v.scal[0].cpu().numpy()
        it = v.ints[0].cpu().numpy()
        stats = dict(zip(STAT_KEYS, [int(it[1]), 0, 0, 0, float(sc[1]), int(it[2])]))
        return {'episode_stats': stats, 'combo_chain': [], 'stance_stability': float(sc[0]),
                'current_step': int(it[0])}
