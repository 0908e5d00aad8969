"""What the seven tasks' environments share: ``TaskVectorEnv``, the batched env around one task's
``mgx_<task>_configure`` / ``_step`` / ``_reset`` entries, and ``TaskEnv``, the batch-size-1 drop-in
around one of those.

A task's VectorEnv keeps what is its own: the model and its index tables, its state tensors in the
order of its ``mgx_<task>_env`` struct, its action space, ``info()`` and any extras. The device,
model handle, output tensors, the struct binding, the staged-step workspace, ``reset()``, ``step()``
and ``close()`` live here once.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from .. import cabi
from ..batch import PhysicsBatch, _ptr, stream_handle
from ..dynamics import DynamicsForwarding
from ..ik import IkForwarding
from ..ilqr import IlqrForwarding
from ..sampling import SamplingForwarding
from ..estimation import EstimationForwarding
from ..native import NativeError, check, lib
from ..rays import RayForwarding
from ..render import RenderForwarding, env_frame
from ..manifold import ManifoldForwarding
from ..rollouts import RolloutForwarding
from ..seeding import np_random
from ..sensors import SensorForwarding
from ..sensor_fd import SensorFdForwarding
from ..spaces import EnvBase, policy_action
from ..transitions import TransitionForwarding


def device_actions(actions: torch.Tensor, device: torch.device) -> torch.Tensor:
    """A policy's actions as the step kernels read them: contiguous on ``device``, float32, or
    float64 where the policy's are — the references' np.clip keeps a float64 action's dtype, so ctrl
    and the action terms of the reward follow in float64 (include/mgx.h action_f64)."""
    dt = torch.float64 if actions.dtype == torch.float64 else torch.float32
    if actions.dtype != dt or not actions.is_contiguous() or actions.device != device:
        actions = actions.to(device=device, dtype=dt).contiguous()
    return actions


class TaskVectorEnv(RayForwarding, RenderForwarding, SensorForwarding, DynamicsForwarding, IkForwarding, TransitionForwarding,
                    RolloutForwarding, ManifoldForwarding, IlqrForwarding, SensorFdForwarding, SamplingForwarding,
                    EstimationForwarding):
    """``num_envs`` envs of one task stepping in lockstep on one GPU, one fused launch (or one
    staged pipeline) per env step, with same-step autoreset."""

    TASK: str = ""         # the library's entries: mgx_<TASK>_configure, _step, _reset, _workspace_*
    ENV_STRUCT: Any = None  # cabi.Mgx<Task>Env
    OBS_DIM: int = 0
    N_DRAWS: int = 0       # host reset draws per env, in reference order
    SEEDED: bool = True    # resets draw (host draws, or device Philox keyed by (seed, env, episode))

    def _setup(self, num_envs: int, device: str, precision: str, model, tables, autoreset: bool, seed: int = 0,
               env_offset: int = 0) -> None:
        """The part of __init__ before the task's own state tensors."""
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.model = model
        self.tables = tables
        self.batch = PhysicsBatch(model, num_envs, precision=precision, device=device)
        self.native = self.batch.native
        self.autoreset = autoreset
        if self.SEEDED:
            self.seed_value = int(seed) & ((1 << 64) - 1)
            self.env_offset = env_offset
        dev, N = self.device, num_envs
        self.episode = torch.zeros(N, dtype=torch.int32, device=dev)
        self.obs = torch.zeros(N, self.OBS_DIM, dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros(N, self.OBS_DIM, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.terminated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.staged = False
        self.workspace = None
        # the library entries, looked up once (step() runs every env step)
        self._step_name, self._reset_name = f"mgx_{self.TASK}_step", f"mgx_{self.TASK}_reset"
        self._step_fn, self._reset_fn = getattr(lib(), self._step_name), getattr(lib(), self._reset_name)

    def _bind(self, *tensors: torch.Tensor, **named: torch.Tensor) -> None:
        """The env struct from the state tensors (leading fields in order, the others by name),
        then mgx_<task>_configure with the tables' ids."""
        self._env = self.ENV_STRUCT(*[t.data_ptr() for t in tensors])
        for k, t in named.items():
            setattr(self._env, k, t.data_ptr())
        ids = self.tables.ids_struct()
        name = f"mgx_{self.TASK}_configure"
        check(getattr(lib(), name)(self.native.handle, C.byref(ids)), name)

    def _stage(self, banks: int, optional: bool = False) -> bool:
        """Select the staged step: its workspace for (model, num_envs, banks), initialised and
        bound to the env struct. ``optional``: False where the staged pipeline does not take this
        model or hook configuration (the monolithic step computes the same physics)."""
        L, N, name = lib(), self.num_envs, f"mgx_{self.TASK}_workspace_"
        nb = int(getattr(L, name + "bytes")(self.native.handle, N, banks))
        if optional and nb == cabi.MGX_E_UNSUPPORTED:
            return False
        if nb <= 0:
            raise NativeError(f"{name}bytes: {L.mgx_last_error().decode()}")
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
        check(getattr(L, name + "init")(self.native.handle, _ptr(self.workspace), nb, N, banks, None), name + "init")
        self._env.workspace = self.workspace.data_ptr()
        self._env.workspace_bytes = nb
        self._env.banks = banks
        self.staged = True
        return True

    def reset(self, seed: Optional[int] = None, env_mask: Optional[torch.Tensor] = None,
              draws: Optional[np.ndarray] = None, stream=None) -> Tuple[torch.Tensor, Dict[str, Any]]:
        """reset() for all (or masked) envs. ``draws`` [N, N_DRAWS] (host, reference order) gives
        exact gymnasium seeding; otherwise device Philox draws keyed by (seed, env, episode)."""
        if seed is not None:
            if self.SEEDED:
                self.seed_value = int(seed) & ((1 << 64) - 1)
            self.episode.zero_()
        if self.SEEDED:
            d = None
            if draws is not None:
                d = torch.as_tensor(np.asarray(draws).reshape(self.num_envs, self.N_DRAWS),
                                    dtype=self.batch.dtype).to(self.device)
            args = (_ptr(d), _ptr(self.obs), self.seed_value, self.env_offset)
        else:
            args = (_ptr(self.obs),)
        check(self._reset_fn(self.native.handle, C.byref(self.batch.state), C.byref(self._env), *args, self.num_envs,
                             _ptr(env_mask), stream_handle(stream)), self._reset_name)
        return self.obs, self.info()

    def step(self, actions: torch.Tensor, stream=None):
        """One env step for every env. ``actions`` [N, n] float32 or float64 (device_actions)."""
        actions = device_actions(actions, self.device)
        assert actions.shape == (self.num_envs,) + self.action_space.shape, actions.shape
        self._env.action_f64 = 1 if actions.dtype == torch.float64 else 0
        keys = (self.seed_value, self.env_offset) if self.SEEDED else ()
        check(self._step_fn(self.native.handle, C.byref(self.batch.state), C.byref(self._env), _ptr(actions),
                            _ptr(self.obs), _ptr(self.reward), _ptr(self.terminated), _ptr(self.truncated),
                            _ptr(self.final_obs) if self.autoreset else None, 1 if self.autoreset else 0, *keys,
                            self.num_envs, None, stream_handle(stream)), self._step_name)
        return self.obs, self.reward, self.terminated, self.truncated, self.info()

    def info(self) -> Dict[str, Any]:
        raise NotImplementedError

    def close(self):
        pass


class TaskEnv(EnvBase):
    """The gymnasium-style, batch-size-1 surface of a task: ``self._vec`` is its VectorEnv of one
    env; seeding is gymnasium's (PCG64 over SeedSequence) and a reset's draws are the reference's."""

    def seed(self, seed: Optional[int] = None) -> list:
        self.np_random, seed = np_random(seed)
        return [seed]

    def _reset_vec(self, seed: Optional[int]) -> np.ndarray:
        """reset() of the one env from gymnasium-seeded host draws; its observation"""
        v = self._vec
        if not v.SEEDED:
            obs, _ = v.reset(seed=seed)
        else:
            if seed is not None:
                self.seed(seed)
            obs, _ = v.reset(draws=v.tables.reset_draws(self.np_random)[None])
        torch.cuda.synchronize(v.device)
        return obs[0].cpu().numpy().copy()

    def _step_vec(self, action):
        """step() of the one env on the policy's action (policy_action types it as the reference's
        np.clip would; clipped on the device): (obs, reward, terminated, truncated)"""
        v = self._vec
        a = torch.from_numpy(policy_action(action).reshape(1, -1)).to(v.device)
        obs, rew, term, trunc, _ = v.step(a)
        torch.cuda.synchronize(v.device)
        return obs[0].cpu().numpy().copy(), float(rew[0]), bool(term[0]), bool(trunc[0])

    _render_camera = None
    _render_size = (480, 640)

    def _render_setup(self, render_camera, render_size) -> None:
        """The opt-in keywords ``render_camera`` (a camera name or index of the model; None: render()
        stays what the reference's is on a headless node) and ``render_size`` (H, W)."""
        self._render_camera = render_camera
        self._render_size = (int(render_size[0]), int(render_size[1]))

    def render(self):
        if self._render_camera is None:
            return None  # no viewer on a headless GPU node (the references only sync theirs)
        if self.render_mode not in self.metadata['render_modes']:
            return None
        return env_frame(self._vec, self.render_mode, self._render_camera, self._render_size)

    def close(self):
        self.viewer = None
