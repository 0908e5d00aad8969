"""Stream shards: one batch of envs stepped as several contiguous shards, each its own staged
pipeline (own VectorEnv, own workspace) on its own HIP stream (shard 0 on the caller's).

Why: a staged step is a chain of launches per substep (rows -> lane-group PGS -> finish). The
solver launch ends with a tail in which a few waves run the heaviest slots' Gauss–Seidel chains
(parkour's exploding pre-reset states reach 338 rows, DESIGN.md §3 Capacity) while most CUs sit
idle; a second shard's row builder or solver on another stream fills them. Shard i owns global
envs [env_offset + start_i, ...): draws and device Philox streams are keyed by the global env
index, so the trajectories are the ones one VectorEnv over all envs produces
(tests/test_gpu_staged.py, tests/test_gpu_parkour.py). The outputs (obs, reward, flags,
final_obs) are one tensor each; the shards write into row slices of them.
"""
from __future__ import annotations

from collections.abc import Mapping
from typing import Any, Callable, Dict, Optional

import numpy as np
import torch

from .base import device_actions


class _CatInfo(Mapping):
    """info() of a stream-sharded batch: each field is the shards' device views concatenated on
    first access (no kernels are launched for fields the caller never reads). A read-only
    Mapping, so get / items / values / `in` all go through __getitem__ and agree with the
    single-batch VectorEnv.info() dict."""

    def __init__(self, shards):
        self._shards = shards
        self._keys = list(shards[0].info().keys())
        self._cache: Dict[str, Any] = {}

    def __getitem__(self, k):
        if k not in self._cache:
            if k not in self._keys:
                raise KeyError(k)
            self._cache[k] = torch.cat([s.info()[k] for s in self._shards])
        return self._cache[k]

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)


def shard_bounds(num_envs: int, n_streams: int):
    """contiguous [a, b) ranges, the first num_envs % n_streams one env larger"""
    if n_streams < 1 or n_streams > num_envs:
        raise ValueError("need 1 <= n_streams <= num_envs")
    base, extra = divmod(num_envs, n_streams)
    out, a = [], 0
    for i in range(n_streams):
        b = a + base + (1 if i < extra else 0)
        out.append((a, b))
        a = b
    return out


class StreamShardedEnv:
    """``num_envs`` envs of one task as ``n_streams`` shards; ``make_shard(n, offset)`` builds
    the VectorEnv of one shard (n envs, global env offset ``offset`` added to the caller's)."""

    _OUTPUTS = ("obs", "final_obs", "reward", "terminated", "truncated")

    def __init__(self, make_shard: Callable[[int, int], Any], num_envs: int, n_streams: int = 2,
                 device: str = "cuda:0", serial: bool = False):
        """``serial``: the shards run one after another on the caller's stream (sub-batches:
        each shard's whole step — every substep / RK4 stage — before the next shard's, so one
        shard's constraint rows B, written once per stage and re-read every PGS sweep, are the
        only B live in the 256 MiB Infinity Cache at a time)."""
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.bounds = shard_bounds(num_envs, n_streams)
        self.shards = [make_shard(b - a, a) for a, b in self.bounds]
        s0 = self.shards[0]
        self.model, self.tables, self.action_space = s0.model, s0.tables, s0.action_space
        self.nu = int(np.prod(s0.action_space.shape))
        for name in self._OUTPUTS:
            t = getattr(s0, name)
            full = torch.zeros((num_envs,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
            setattr(self, name, full)
            for (a, b), s in zip(self.bounds, self.shards):  # row slices: contiguous
                setattr(s, name, full[a:b])
        self.serial = serial
        # shard 0 runs on the caller's stream, shards 1.. on streams of their own: K shards take K
        # HIP streams, so up to 4 fit the box's 4 hardware queues (GPU_MAX_HW_QUEUES) without a
        # shard's kernels queueing behind the caller stream's wait for all of them
        self.streams = [] if serial else [torch.cuda.Stream(device=self.device) for _ in self.shards[1:]]

    def _fan_out(self, stream, fn):
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self.serial:
            for (a, b), s in zip(self.bounds, self.shards):
                fn(a, b, s, cs)
            return
        for st in self.streams:
            st.wait_stream(cs)
        for (a, b), s, st in zip(self.bounds, self.shards, [cs] + self.streams):
            fn(a, b, s, st)
        for st in self.streams:
            cs.wait_stream(st)

    def reset(self, seed: Optional[int] = None, env_mask: Optional[torch.Tensor] = None,
              draws: Optional[np.ndarray] = None, stream=None):
        """reset over every shard (mask / draws sliced per shard)."""
        d = None if draws is None else np.asarray(draws).reshape(self.num_envs, -1)
        self._fan_out(stream, lambda a, b, s, st: s.reset(seed=seed, env_mask=None if env_mask is None else env_mask[a:b],
                                                           draws=None if d is None else d[a:b], stream=st))
        return self.obs, self.info()

    def step(self, actions: torch.Tensor, stream=None):
        """One env step for every env; actions float32 or float64 [N, nu] on the device."""
        actions = device_actions(actions, self.device)
        assert actions.shape == (self.num_envs, self.nu), actions.shape
        self._fan_out(stream, lambda a, b, s, st: s.step(actions[a:b], stream=st))
        return self.obs, self.reward, self.terminated, self.truncated, self.info()

    @property
    def cameras(self):
        return self.shards[0].cameras

    def render_depth(self, camera, height: int, width: int, segmentation: bool = True,
                     bodyexclude: Optional[int] = None, mask: Optional[torch.Tensor] = None, stream=None):
        """PhysicsBatch.render_depth over every shard: each shard's rows go into slices of one
        [N, H, W] depth (and segmentation) tensor, cached per (H, W). Everything is launched on the
        caller's stream: after step() that stream is already ordered after every shard (_fan_out),
        so no side-stream work is needed."""
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        key = (int(height), int(width))
        cache = self.__dict__.setdefault("_depth_out", {})
        if key not in cache:
            cache[key] = (torch.empty((self.num_envs,) + key, dtype=torch.float32, device=self.device),
                          torch.empty((self.num_envs,) + key, dtype=torch.int32, device=self.device))
        depth, seg = cache[key]
        for (a, b), s in zip(self.bounds, self.shards):
            s.batch.render_depth(camera, height, width, segmentation=segmentation, bodyexclude=bodyexclude,
                                 mask=None if mask is None else mask[a:b], stream=cs, out=(depth[a:b], seg[a:b]))
        return depth, (seg if segmentation else None)

    @property
    def lights(self):
        return self.shards[0].lights

    def render_rgb(self, camera, height: int, width: int, dtype: torch.dtype = torch.uint8, depth: bool = False,
                   segmentation: bool = False, bodyexclude: Optional[int] = None, groups=None, static: bool = True,
                   mask: Optional[torch.Tensor] = None, stream=None):
        """PhysicsBatch.render_rgb over every shard, into slices of one [N, H, W, 3] image (and depth /
        segmentation when asked), each cached per shape and dtype; launched on the caller's stream only, as
        render_depth."""
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        hw = (self.num_envs, int(height), int(width))
        cache = self.__dict__.setdefault("_rgb_out", {})

        def buf(what, shape, dt):  # each output is allocated on the first call that asks for it
            if (what, shape, dt) not in cache:
                cache[(what, shape, dt)] = torch.empty(shape, dtype=dt, device=self.device)
            return cache[(what, shape, dt)]

        rgb = buf("rgb", hw + (3,), dtype)
        dep = buf("depth", hw, torch.float32) if depth else None
        seg = buf("seg", hw, torch.int32) if segmentation else None
        for (a, b), s in zip(self.bounds, self.shards):
            s.batch.render_rgb(camera, height, width, dtype=dtype, depth=depth, segmentation=segmentation,
                               bodyexclude=bodyexclude, groups=groups, static=static,
                               mask=None if mask is None else mask[a:b], stream=cs,
                               out=(rgb[a:b], dep[a:b] if depth else None, seg[a:b] if segmentation else None))
        if not depth and not segmentation:
            return rgb
        return (rgb,) + ((dep,) if depth else ()) + ((seg,) if segmentation else ())

    @property
    def sensors(self):
        return self.shards[0].sensors

    @property
    def sensor_slices(self):
        return self.shards[0].sensor_slices

    def sensordata(self, mask: Optional[torch.Tensor] = None, stream=None):
        """PhysicsBatch.sensordata over every shard: each shard's rows go into slices of one
        [N, nsensordata] tensor, allocated once. Like render_depth, everything (the forward kernel
        included) is launched on the caller's stream."""
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = self.__dict__.get("_sensor_out")
        if out is None:
            b0 = self.shards[0].batch
            out = torch.zeros(self.num_envs, int(self.model.nsensordata), dtype=b0.dtype, device=self.device)
            self._sensor_out = out
        for (a, b), s in zip(self.bounds, self.shards):
            s.batch.sensordata(mask=None if mask is None else mask[a:b], stream=cs, out=out[a:b])
        return out

    def sensor(self, name: str, mask: Optional[torch.Tensor] = None, stream=None):
        """One sensor's columns of a fresh sensordata(): a view [N, dim]."""
        return self.sensordata(mask=mask, stream=stream)[:, self.sensor_slices[name]]

    def jac_points(self, **kw):
        """PhysicsBatch.jac_points (the shards share one model and device, so one points object
        serves them all)."""
        return self.shards[0].batch.jac_points(**kw)

    def _jac_over_shards(self, call, key, n_point, mask, stream):
        from ..dynamics import JacResult
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        cache = self.__dict__.setdefault("_jac_out", {})
        if key not in cache:
            b0 = self.shards[0].batch
            cache[key] = JacResult(self.num_envs, n_point, int(self.model.nv), b0.dtype, self.device)
        full = cache[key]
        for (a, b), s in zip(self.bounds, self.shards):
            call(s.batch, a, b, None if mask is None else mask[a:b], cs, full.rows(a, b))
        return full

    def jac(self, points, mask: Optional[torch.Tensor] = None, stream=None):
        """PhysicsBatch.jac over every shard: each shard's rows go into slices of one JacResult,
        allocated once per points object. Like sensordata, everything is launched on the caller's
        stream."""
        self.__dict__.setdefault("_jac_points", {})[id(points)] = points  # keeps the cache key's id alive
        return self._jac_over_shards(lambda bt, a, b, m, cs, out: bt.jac(points, mask=m, stream=cs, out=out),
                                     ("points", id(points)), len(points), mask, stream)

    def jac_world(self, body_ids, pos: torch.Tensor, mask: Optional[torch.Tensor] = None, stream=None):
        """PhysicsBatch.jac_world over every shard (``pos`` [N, P, 3])."""
        p = int(pos.shape[1])
        return self._jac_over_shards(
            lambda bt, a, b, m, cs, out: bt.jac_world(body_ids, pos[a:b], mask=m, stream=cs, out=out),
            ("world", p), p, mask, stream)

    def dynamics(self, qacc: Optional[torch.Tensor] = None, qfrc_constraint: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, stream=None, only=None):
        """PhysicsBatch.dynamics over every shard: each shard's rows go into slices of one set of
        tensors, allocated once; launched on the caller's stream."""
        from ..dynamics import DYN_OUTPUTS, DynamicsResult, alloc_dynamics
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        full = self.__dict__.get("_dyn_out")
        if full is None:
            b0 = self.shards[0].batch
            full = self._dyn_out = alloc_dynamics(self.num_envs, int(self.model.nv), b0.dtype, self.device)
        part = None
        for (a, b), s in zip(self.bounds, self.shards):
            part = s.batch.dynamics(qacc=None if qacc is None else qacc[a:b],
                                    qfrc_constraint=None if qfrc_constraint is None else qfrc_constraint[a:b],
                                    mask=None if mask is None else mask[a:b], stream=cs, only=only,
                                    out=full.rows(a, b))
        return DynamicsResult(**{f: getattr(full, f) for f in DYN_OUTPUTS if getattr(part, f) is not None})

    def mass_matrix(self, mask: Optional[torch.Tensor] = None, stream=None):
        return self.dynamics(mask=mask, stream=stream, only=("M",)).M

    def energy(self, mask: Optional[torch.Tensor] = None, stream=None):
        return self.dynamics(mask=mask, stream=stream, only=("energy",)).energy

    def ik_targets(self, points, **kw):
        """PhysicsBatch.ik_targets (one targets object serves every shard, as jac_points)."""
        return self.shards[0].batch.ik_targets(points, **kw)

    def solve_ik(self, targets, target_pos: torch.Tensor, target_quat: Optional[torch.Tensor] = None,
                 qpos_init: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, stream=None, **kw):
        """PhysicsBatch.solve_ik over every shard: each shard's rows go into slices of one IkResult,
        allocated once per targets object; launched on the caller's stream."""
        from ..ik import IkResult
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        cache = self.__dict__.setdefault("_ik_out", {})
        if id(targets) not in cache:
            b0 = self.shards[0].batch
            cache[id(targets)] = (targets, IkResult(self.num_envs, int(self.model.nq), b0.dtype, self.device))
        full = cache[id(targets)][1]  # the entry keeps the targets alive, and so the key's id
        cut = lambda x, a, b: None if x is None else x[a:b]  # noqa: E731
        for (a, b), s in zip(self.bounds, self.shards):
            s.batch.solve_ik(targets, target_pos[a:b], target_quat=cut(target_quat, a, b), qpos_init=cut(qpos_init, a, b),
                             mask=cut(mask, a, b), stream=cs, out=full.rows(a, b), **kw)
        return full

    def transition_fd(self, mask: Optional[torch.Tensor] = None, stream=None, only=None, **kw):
        """PhysicsBatch.transition_fd over every shard, into slices of one set of tensors."""
        from ..transitions import FD_OUTPUTS, TransitionResult, alloc_transition
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        full = self.__dict__.get("_fd_out")
        if full is None:
            b0, m = self.shards[0].batch, self.model
            full = self._fd_out = alloc_transition(self.num_envs, int(m.nq), int(m.nv), int(m.nu), b0.dtype, self.device)
        part = None
        for (a, b), s in zip(self.bounds, self.shards):
            part = s.batch.transition_fd(mask=None if mask is None else mask[a:b], stream=cs, only=only,
                                         out=full.rows(a, b), **kw)
        return TransitionResult(**{f: getattr(full, f) for f in FD_OUTPUTS if getattr(part, f) is not None})

    def sensor_fd(self, mask: Optional[torch.Tensor] = None, stream=None, only=None, **kw):
        """PhysicsBatch.sensor_fd over every shard, into slices of one set of tensors."""
        from ..sensor_fd import SENSOR_FD_OUTPUTS, SensorFdResult, alloc_sensor_fd
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        full = self.__dict__.get("_sensor_fd_out")
        if full is None:
            b0, m = self.shards[0].batch, self.model
            full = self._sensor_fd_out = alloc_sensor_fd(self.num_envs, int(m.nsensordata), int(m.nv), int(m.nu),
                                                         b0.dtype, self.device)
        part = None
        for (a, b), s in zip(self.bounds, self.shards):
            part = s.batch.sensor_fd(mask=None if mask is None else mask[a:b], stream=cs, only=only,
                                     out=full.rows(a, b), **kw)
        return SensorFdResult(**{f: getattr(full, f) for f in SENSOR_FD_OUTPUTS if getattr(part, f) is not None})

    def sensor_fd_columns(self, centered: bool = False, with_d: bool = True) -> int:
        return self.shards[0].batch.sensor_fd_columns(centered, with_d)

    @property
    def state_size(self) -> int:
        return self.shards[0].batch.state_size

    def get_state(self) -> torch.Tensor:
        return torch.cat([s.batch.get_state() for s in self.shards])

    def set_state(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        for (a, b), s in zip(self.bounds, self.shards):
            s.batch.set_state(x[a:b], mask=None if mask is None else mask[a:b])

    def physics_rollout(self, ctrl=None, nstep=None, initial_state=None, initial_warmstart=None, hold: int = 1,
                        shared_ctrl: bool = False, sensordata: bool = False, mask: Optional[torch.Tensor] = None,
                        stream=None, only=None, **kw):
        """PhysicsBatch.rollout over every shard, into slices of one set of tensors (allocated once
        per (K, T, sensordata)); launched on the caller's stream. The name and the meaning of
        ``ctrl`` are those of RolloutForwarding.physics_rollout (``rollout`` is the episode sums)."""
        from ..rollouts import ROLLOUT_OUTPUTS, RolloutResult, alloc_rollout, rollout_shape
        cs = stream if stream is not None else torch.cuda.current_stream(self.device)
        b0, m = self.shards[0].batch, self.model
        k, t = rollout_shape(self.num_envs, int(m.nu), ctrl, nstep, initial_state, initial_warmstart, hold, shared_ctrl)
        sensordata = sensordata if only is None else "sensordata" in only
        cache = self.__dict__.setdefault("_rollout_out", {})
        key = (k, t, bool(sensordata))
        if key not in cache:
            if t < 1:
                return b0.rollout(nstep=t, hold=hold, **kw)  # the library refuses it and names the argument
            cache[key] = alloc_rollout(self.num_envs, k, t, b0.state_size, int(m.nsensordata), b0.dtype, self.device,
                                       sensordata)
        full, part = cache[key], None
        cut = lambda x, a, b: None if x is None else x[a:b]  # noqa: E731
        for (a, b), s in zip(self.bounds, self.shards):
            part = s.batch.rollout(ctrl=ctrl if shared_ctrl else cut(ctrl, a, b), nstep=t,
                                   initial_state=cut(initial_state, a, b), initial_warmstart=cut(initial_warmstart, a, b),
                                   hold=hold, shared_ctrl=shared_ctrl, sensordata=sensordata, mask=cut(mask, a, b),
                                   stream=cs, only=only, out=full.rows(a, b), **kw)
        return RolloutResult(**{f: getattr(full, f) for f in ROLLOUT_OUTPUTS if getattr(part, f) is not None})

    def ekf(self, *args, **kw):
        """Not provided on sharded envs: the filter keeps one belief batch for one PhysicsBatch."""
        raise NotImplementedError("ekf is not provided on StreamSharded*Env: build the filter on one shard's env or batch")

    def info(self) -> Dict[str, Any]:
        return _CatInfo(self.shards)

    @property
    def episode(self) -> torch.Tensor:
        return torch.cat([s.episode for s in self.shards])

    @property
    def rollout(self) -> torch.Tensor:
        return torch.cat([s.rollout for s in self.shards])

    def close(self):
        pass
