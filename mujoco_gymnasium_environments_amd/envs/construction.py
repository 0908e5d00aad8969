"""humanoid_construction_env on MI355X: a batched VectorEnv and a drop-in gymnasium-style Env.

Mirrors the reference interface humanoid_construction_env/construction_env.py:
  * ``HumanoidConstructionEnv`` — same constructor / ``reset(seed, options)`` / ``step(action)`` /
    spaces / ``metadata`` / ``render`` / ``close`` surface (construction_env.py:24-768), batch size
    1, gymnasium seeding (PCG64 over SeedSequence) and the same draws per reset (task, then wind /
    rain / temperature, :560, :574-576).
  * ``ConstructionVectorEnv`` — N envs on one GPU, device tensors ``[N, ...]``, same-step autoreset
    with Philox reset draws keyed by (seed, global env index, episode).
Both run one fused HIP launch per env step (libmgx.so ``mgx_construction_step``): clip, ctrl =
action, one RK4 mj_step with MuJoCo's default Newton solver (construction_site.xml:10) on the wide
kernels (nv = 99: two dofs per lane, mgx_wide.h), progress / reward / termination / observation.

Quirks reproduced (oracle/construction_logic.py): the 135-float observation against the declared
125 (C1), the np.float32 reward and running total (C2), progress only from the step counter for
operate_crane / transport_material (C3), reset leaves MuJoCo's qpos0 pose and runs no forward
pass (C4).
"""
from __future__ import annotations

import functools
import os
from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import cabi, mjcf
from ..spaces import Box, policy_action
from .base import TaskEnv, TaskVectorEnv

ASSET = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets",
                     "humanoid_construction.xml")
OBS_DIM = 135                  # what _get_observation returns (quirk C1)
DECLARED_OBS_DIM = 125         # observation_space (construction_env.py:527)
MAX_EPISODE_STEPS = 3000       # construction_env.py:38
ACTION_LIMIT = 200.0           # construction_env.py:522-523
TASKS = ('stack_blocks', 'operate_crane', 'transport_material', 'build_structure')   # :73
STAT_KEYS = ('blocks_placed', 'materials_transported', 'crane_operations', 'safety_violations',
             'tasks_completed', 'total_reward')


@functools.lru_cache(maxsize=None)
def construction_model() -> mjcf.Model:
    """construction_site.xml as the reference's _generate_xml_files writes it (construction_env.py:
    179-494); nv = 99 > 64, so it runs on the wide kernels with rows in global scratch."""
    with open(ASSET) as f:
        m = mjcf.compile_xml(f.read())
    m.layout_flags = cabi.MGX_ROWS_IN_SCRATCH
    # ten free blocks resting on the floor / foundation / platform plus the humanoid: up to ~100
    # contacts; rows beyond the capacities are dropped with a counter (mgx_state.overflow)
    m.con_capacity = 128
    m.efc_capacity = 512
    return m


class ConstructionTables:
    """Index tables looked up as _get_model_indices does (construction_env.py:511-516)."""

    def __init__(self, m: mjcf.Model, max_episode_steps: int = MAX_EPISODE_STEPS):
        self.model = m
        self.humanoid = m.name2id("body", "humanoid")
        self.crane = m.name2id("body", "crane_base")
        self.max_episode_steps = max_episode_steps

    def ids_struct(self) -> cabi.MgxConstructionIds:
        s = cabi.MgxConstructionIds()
        s.humanoid = self.humanoid
        s.n_act = self.model.nu
        s.max_episode_steps = self.max_episode_steps
        s.action_limit = ACTION_LIMIT
        return s

    @staticmethod
    def reset_draws(rng: np.random.Generator) -> np.ndarray:
        """The draws of one reset, in reference order (construction_env.py:560, :574-576): the task
        (np_random.choice over the 4 task names), wind, rain, temperature."""
        task = TASKS.index(str(rng.choice(TASKS)))
        return np.array([task, rng.uniform(0, 5), rng.uniform(0, 0.5), rng.uniform(15, 35)], dtype=np.float64)


class ConstructionVectorEnv(TaskVectorEnv):
    """``num_envs`` humanoid_construction envs stepping in lockstep on one GPU. ``step(actions)``
    takes [N, nu] float32 or float64 (clipped to +-200); ``reset(draws=)`` takes [N, 4]."""

    metadata = {'render_modes': [], 'render_fps': 50}
    TASK, ENV_STRUCT, OBS_DIM, N_DRAWS = "construction", cabi.MgxConstructionEnv, OBS_DIM, 4

    def __init__(self, num_envs: int, device: str = "cuda:0", precision: str = "f64", seed: int = 0,
                 max_episode_steps: int = MAX_EPISODE_STEPS, autoreset: bool = True, env_offset: int = 0):
        model = construction_model()
        self._setup(num_envs, device, precision, model, ConstructionTables(model, max_episode_steps), autoreset, seed,
                    env_offset)
        dev, N = self.device, num_envs
        self.scal = torch.zeros(N, 4, dtype=torch.float64, device=dev)   # progress, wind, rain, temperature
        self.ints = torch.zeros(N, 5, dtype=torch.int32, device=dev)     # task, step, blocks, violations, completed
        # episode_stats['total_reward']: a float32 value (NEP 50 keeps it np.float32 for float32 actions)
        # or float64 once a float64 action's reward was added; total_kind records which (include/mgx.h)
        self.total_reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.total_kind = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.rollout = torch.zeros(N, 4, dtype=torch.float64, device=dev)
        self._bind(self.scal, self.ints, self.total_reward, self.episode, self.rollout, total_kind=self.total_kind)
        self.action_space = Box(low=-ACTION_LIMIT, high=ACTION_LIMIT, shape=(self.model.nu,), dtype=np.float32)

    def info(self) -> Dict[str, Any]:
        """Device-tensor views of the reference's info dict (construction_env.py:739-752)."""
        return {
            'task': self.ints[:, 0],
            'task_progress': self.scal[:, 0],
            'blocks_placed': self.ints[:, 2],
            'safety_violations': self.ints[:, 3],
            'tasks_completed': self.ints[:, 4],
            'total_reward': self.total_reward,
            'weather': self.scal[:, 1:4],
            'current_step': self.ints[:, 1],
            'final_observation': self.final_obs,
            'episode': self.episode,
            'bad_state_resets': self.batch.warning,
        }


class HumanoidConstructionEnv(TaskEnv):
    """Drop-in for humanoid_construction_env.construction_env.HumanoidConstructionEnv on libmgx.
    A float32 action (``action_space.sample()``, float32 policies) is clipped against the float32
    bounds in float32, and the reward is np.float32; a float64 action (or a list of floats) stays
    float64 through the clip, ``ctrl`` and the energy term, and the reward is np.float64, as in the
    reference (construction_env.py:589-592, :691).

    ``info['episode_stats']['total_reward']`` is the running total *before* this step's reward:
    the reference copies ``episode_stats`` into ``info`` (construction_env.py:613-614, :746) and
    only then adds the reward (:617). It is a Python 0.0 until the first reward has been added,
    np.float32 after (NEP 50: Python float + np.float32 stays float32)."""

    metadata = {'render_modes': ['human', 'rgb_array'], 'render_fps': 50}

    def __init__(self, render_mode: Optional[str] = None, device: str = "cuda:0", precision: str = "f64",
                 render_camera=None, render_size=(480, 640), **kwargs):
        super().__init__()
        self._render_setup(render_camera, render_size)
        self.dt = 0.02
        self.max_episode_steps = MAX_EPISODE_STEPS
        self.current_step = 0
        self.render_mode = render_mode
        self._vec = ConstructionVectorEnv(1, device=device, precision=precision, autoreset=False,
                                          max_episode_steps=self.max_episode_steps)
        self.model = self._vec.model
        self.num_joints = self.model.nu
        self.task_types = list(TASKS)
        self.current_task = None
        self.action_space = Box(low=-ACTION_LIMIT * np.ones(self.num_joints), high=ACTION_LIMIT * np.ones(self.num_joints),
                                dtype=np.float32)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(DECLARED_OBS_DIM,), dtype=np.float32)
        self.viewer = None
        self.np_random = None
        self.seed()

    def reset(self, *, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        obs = self._reset_vec(seed)
        self.current_step = 0
        self._total_before = 0.0
        return obs, self._info()

    def step(self, action: np.ndarray):
        act = policy_action(action)
        obs, rew, term, trunc = self._step_vec(act)
        self.current_step = int(self._vec.ints[0, 1])
        info = self._info()  # the total as it was before this step's reward (construction_env.py:614-617)
        kind = int(self._vec.total_kind[0])
        self._total_before = (np.float64 if kind == 1 else np.float32)(self._vec.total_reward[0].item())
        rtype = np.float64 if act.dtype == np.float64 else np.float32
        return obs, rtype(rew), term, trunc, info

    def _info(self) -> Dict[str, Any]:
        v = self._vec
        sc = v.scal[0].cpu().numpy()
        it = v.ints[0].cpu().numpy()
        self.current_task = TASKS[int(it[0])]
        stats = dict(zip(STAT_KEYS, [0, 0, 0, 0, int(it[4]), getattr(self, '_total_before', 0.0)]))
        return {'task': self.current_task, 'task_progress': float(sc[0]), 'blocks_placed': int(it[2]),
                'safety_violations': int(it[3]), 'episode_stats': stats,
                'weather': {'wind': float(sc[1]), 'rain': float(sc[2]), 'temperature': float(sc[3])}}
