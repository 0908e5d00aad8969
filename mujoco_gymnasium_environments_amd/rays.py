"""Batched ray casting and depth cameras on the device (mgx_ray_*, include/mgx.h).

``RayMethods`` gives :class:`~.batch.PhysicsBatch` its ``ray`` / ``render_depth`` / ``cameras``;
``RayForwarding`` gives the ``*VectorEnv`` classes the same calls, forwarded to their batch.

Rays see the geom poses of the CURRENT ``qpos`` — what ``mj_kinematics`` would give now: every
call first recomputes the scene (geom and camera world poses) from ``qpos`` on the same stream.
They never read the stale pre-integration frames a step leaves in ``xpos`` / ``xquat``.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import cabi
from .native import check, lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class RayMethods:
    """Mixin of PhysicsBatch (uses its model, native, n, device, dtype and state)."""

    @property
    def cameras(self) -> List[str]:
        """Names of the model's cameras, in model order."""
        return list(self.model.cam_names)

    # ------------------------------------------------------------------ set-up, once
    def _ray_ready(self) -> None:
        nat = self.native
        if getattr(nat, "_ray_packed", None) is None:
            packed = cabi.PackedRay(self.model)
            check(lib().mgx_ray_configure(nat.handle, C.byref(packed.desc)), "mgx_ray_configure")
            nat._ray_packed = packed
        if getattr(self, "_ray_scene", None) is None:
            nb = int(lib().mgx_ray_scene_bytes(nat.handle, self.n))
            check(min(nb, 0), "mgx_ray_scene_bytes")
            self._ray_scene = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device)
            self._ray_masks = {}
            self._ray_out = {}

    def _ray_refresh(self, mask, stream) -> None:
        check(lib().mgx_ray_scene(self.native.handle, C.byref(self._state), _ptr(self._ray_scene),
                                  self._ray_scene.numel(), self.n, _ptr(mask), _stream(stream)), "mgx_ray_scene")

    def _ray_geom_mask(self, groups: Optional[Iterable[int]], static: bool) -> Optional[torch.Tensor]:
        """uint8 [ngeom] device mask of ``groups`` (geom groups to keep; None = all) and ``static``
        (keep the geoms of body 0), built once per combination."""
        if groups is None and static:
            return None
        key = (None if groups is None else frozenset(int(g) for g in groups), bool(static))
        if key not in self._ray_masks:
            m = self.model
            keep = np.ones(m.ngeom, dtype=bool)
            if key[0] is not None:
                keep &= np.isin(np.asarray(m.geom_group), sorted(key[0]))
            if not static:
                keep &= np.asarray(m.geom_bodyid) != 0
            self._ray_masks[key] = torch.from_numpy(keep.astype(np.uint8)).to(self.device)
        return self._ray_masks[key]

    def _ray_buffers(self, key, shapes):
        if key not in self._ray_out:
            self._ray_out[key] = tuple(torch.empty(s, dtype=d, device=self.device) for s, d in shapes)
        return self._ray_out[key]

    @staticmethod
    def _check_env_mask(mask, n):
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.is_cuda and mask.is_contiguous()

    # ------------------------------------------------------------------ API
    def ray(self, pnt: torch.Tensor, vec: torch.Tensor, groups: Optional[Iterable[int]] = None, static: bool = True,
            bodyexclude: int = -1, mask: Optional[torch.Tensor] = None, stream=None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
        """mj_multiRay for every (masked) env: rays ``pnt + x vec`` ([N, R, 3] each, ``vec`` not
        normalised, ``x`` in units of ``|vec|``) against the env's geoms at its current ``qpos``.

        Returns ``(dist [N, R], geomid [N, R] int32)``; a miss is ``-1 / -1``. ``groups`` keeps only
        geoms of those groups, ``static=False`` drops the geoms of body 0, ``bodyexclude`` drops one
        body's geoms (-1: none). Geoms with alpha 0 and no material never count. The two tensors
        are allocated once per R and overwritten by the next call with the same R; rows of envs
        that ``mask`` (uint8 [N]) deselects are left as they were."""
        self._ray_ready()
        dt = self.dtype
        pnt = pnt.to(device=self.device, dtype=dt).contiguous()
        vec = vec.to(device=self.device, dtype=dt).contiguous()
        if pnt.dim() != 3 or pnt.shape[0] != self.n or pnt.shape[2] != 3 or vec.shape != pnt.shape:
            raise ValueError(f"pnt and vec must be [{self.n}, R, 3], got {tuple(pnt.shape)} and {tuple(vec.shape)}")
        self._check_env_mask(mask, self.n)
        R = int(pnt.shape[1])
        dist, geomid = self._ray_buffers(("ray", R), (((self.n, R), dt), ((self.n, R), torch.int32)))
        self._ray_refresh(mask, stream)
        check(lib().mgx_ray_cast(self.native.handle, _ptr(self._ray_scene), _ptr(pnt), _ptr(vec), R,
                                 _ptr(self._ray_geom_mask(groups, static)), int(bodyexclude), _ptr(dist),
                                 _ptr(geomid), self.n, _ptr(mask), _stream(stream)), "mgx_ray_cast")
        return dist, geomid

    def camera_id(self, camera: Union[str, int]) -> int:
        names = self.model.cam_names
        if isinstance(camera, str):
            if camera not in names:
                raise KeyError(f"unknown camera {camera!r}; the model has {names}")
            return names.index(camera)
        if not 0 <= int(camera) < len(names):
            raise KeyError(f"camera index {camera} out of range; the model has {len(names)} cameras")
        return int(camera)

    def render_depth(self, camera: Union[str, int], height: int, width: int, segmentation: bool = True,
                     bodyexclude: Optional[int] = None, mask: Optional[torch.Tensor] = None, stream=None,
                     groups: Optional[Iterable[int]] = None, static: bool = True, out=None
                     ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Depth image of one of the model's cameras for every (masked) env, at the current ``qpos``.

        Returns ``(depth [N, H, W] float32, segmentation [N, H, W] int32 or None)``: the planar
        (z-) depth along the camera's -Z axis as MuJoCo's depth rendering reports it (``+inf``
        where nothing is hit) and the id of the geom hit (-1 for none). Row 0 is the top of the
        image. ``bodyexclude`` defaults to the camera's own body (a head camera sits inside the
        head geom); a camera on the world body excludes nothing. ``out=(depth, seg)`` writes into
        caller tensors instead of the ones cached per (H, W)."""
        self._ray_ready()
        cam = self.camera_id(camera)
        self._check_env_mask(mask, self.n)
        H, W = int(height), int(width)
        if H <= 0 or W <= 0:
            raise ValueError("height and width must be positive")
        if bodyexclude is None:
            body = int(self.model.cam_bodyid[cam])
            bodyexclude = body if body != 0 else -1
        if out is None:
            depth, seg = self._ray_buffers(("cam", H, W), (((self.n, H, W), torch.float32),
                                                           ((self.n, H, W), torch.int32)))
        else:
            depth, seg = out
            for t, d in ((depth, torch.float32), (seg, torch.int32)):
                assert t is None or (t.dtype == d and tuple(t.shape) == (self.n, H, W) and t.is_contiguous())
        if not segmentation:
            seg = None
        self._ray_refresh(mask, stream)
        check(lib().mgx_ray_camera(self.native.handle, _ptr(self._ray_scene), cam, H, W,
                                   _ptr(self._ray_geom_mask(groups, static)), int(bodyexclude), _ptr(depth),
                                   _ptr(seg), self.n, _ptr(mask), _stream(stream)), "mgx_ray_camera")
        return depth, seg


class RayForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's ray calls under the env's name."""

    @property
    def cameras(self) -> List[str]:
        return self.batch.cameras

    def ray(self, pnt, vec, **kw):
        """PhysicsBatch.ray of this env's batch (rays at the current qpos)."""
        return self.batch.ray(pnt, vec, **kw)

    def render_depth(self, camera, height, width, **kw):
        """PhysicsBatch.render_depth of this env's batch (depth / segmentation at the current qpos)."""
        return self.batch.render_depth(camera, height, width, **kw)
