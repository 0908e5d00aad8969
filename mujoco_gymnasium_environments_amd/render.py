"""Batched RGB camera images on the device (mgx_render_*, include/mgx.h "RGB camera images").

``RenderMethods`` gives :class:`~.batch.PhysicsBatch` its ``render_rgb`` / ``lights``;
``RenderForwarding`` gives the ``*VectorEnv`` classes the same calls, forwarded to their batch, and
``env_frame`` is what the drop-in ``Env`` classes' ``render()`` returns when a camera was chosen.

The image is ray traced with the small shading model stated in include/mgx.h: it
is not MuJoCo's OpenGL image. Like the depth camera it shows the CURRENT ``qpos``: every call first
recomputes the scene (geom, camera and light world poses) on the same stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import cabi
from .native import check, lib
from .rays import _ptr, _stream


class RenderMethods:
    """Mixin of PhysicsBatch, beside RayMethods (uses its camera, mask and buffer helpers)."""

    @property
    def lights(self) -> List[str]:
        """Names of the model's lights, in model order."""
        return list(self.model.light_names)

    def _render_ready(self) -> None:
        self._ray_ready()
        nat = self.native
        if getattr(nat, "_render_packed", None) is None:
            packed = cabi.PackedRender(self.model)
            check(lib().mgx_render_configure(nat.handle, C.byref(packed.desc)), "mgx_render_configure")
            nat._render_packed = packed
        if getattr(self, "_render_scene", None) is None:
            nb = int(lib().mgx_render_scene_bytes(nat.handle, self.n))
            check(min(nb, 0), "mgx_render_scene_bytes")
            self._render_scene = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device)

    def render_rgb(self, camera: Union[str, int], height: int, width: int, dtype: torch.dtype = torch.uint8,
                   depth: bool = False, segmentation: bool = False, bodyexclude: Optional[int] = None,
                   groups: Optional[Iterable[int]] = None, static: bool = True, mask: Optional[torch.Tensor] = None,
                   stream=None, out=None):
        """Colour image of one of the model's cameras for every (masked) env, at the current ``qpos``.

        Returns ``rgb [N, H, W, 3]`` — ``torch.uint8``, or with ``dtype=torch.float32`` the same
        colour in [0, 1] before quantisation (``uint8 = floor(255 rgb + 0.5)``) — or, when ``depth``
        and / or ``segmentation`` are asked for, the tuple ``(rgb, depth, seg)`` without the ones
        not asked for; those two are ``render_depth``'s of the same arguments, bit for bit. Row 0 is
        the top of the image. ``bodyexclude``, ``groups``, ``static`` and ``mask`` act as in
        ``render_depth`` (shadow rays see the same geoms). ``out=(rgb, depth, seg)`` writes into
        caller tensors (None for an output not asked for) instead of the cached ones (one per
        output, shape and dtype)."""
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError("dtype must be torch.uint8 or torch.float32")
        self._render_ready()
        cam = self.camera_id(camera)
        self._check_env_mask(mask, self.n)
        H, W = int(height), int(width)
        if H <= 0 or W <= 0:
            raise ValueError("height and width must be positive")
        if bodyexclude is None:
            body = int(self.model.cam_bodyid[cam])
            bodyexclude = body if body != 0 else -1
        shapes = (((self.n, H, W, 3), dtype), ((self.n, H, W), torch.float32), ((self.n, H, W), torch.int32))
        if out is None:  # each output is allocated on the first call that asks for it
            (rgb,) = self._ray_buffers(("rgb", H, W, dtype), shapes[:1])
            dep = self._ray_buffers(("rgb-depth", H, W), shapes[1:2])[0] if depth else None
            seg = self._ray_buffers(("rgb-seg", H, W), shapes[2:])[0] if segmentation else None
        else:
            rgb, dep, seg = out
            for t, (s, d) in zip((rgb, dep, seg), shapes):
                assert t is None or (t.dtype == d and tuple(t.shape) == s and t.is_contiguous())
            assert rgb is not None and (dep is not None or not depth) and (seg is not None or not segmentation)
        if not depth:
            dep = None
        if not segmentation:
            seg = None
        check(lib().mgx_render_scene(self.native.handle, C.byref(self._state), _ptr(self._render_scene),
                                     self._render_scene.numel(), self.n, _ptr(mask), _stream(stream)),
              "mgx_render_scene")
        check(lib().mgx_render_camera(self.native.handle, _ptr(self._render_scene), cam, H, W,
                                      _ptr(self._ray_geom_mask(groups, static)), int(bodyexclude),
                                      _ptr(rgb) if dtype == torch.uint8 else None,
                                      _ptr(rgb) if dtype == torch.float32 else None, _ptr(dep), _ptr(seg), self.n,
                                      _ptr(mask), _stream(stream)), "mgx_render_camera")
        if not depth and not segmentation:
            return rgb
        return (rgb,) + ((dep,) if depth else ()) + ((seg,) if segmentation else ())


class RenderForwarding:
    """Mixin of the ``*VectorEnv`` classes: the batch's render calls under the env's name."""

    @property
    def lights(self) -> List[str]:
        return self.batch.lights

    def render_rgb(self, camera, height, width, **kw):
        """PhysicsBatch.render_rgb of this env's batch (the colour image at the current qpos)."""
        return self.batch.render_rgb(camera, height, width, **kw)


def env_frame(vec, render_mode: Optional[str], camera, size: Tuple[int, int]) -> Optional[np.ndarray]:
    """What a drop-in Env's ``render()`` returns once ``render_camera`` was given: env 0 of ``vec``
    from that camera as a numpy uint8 ``[H, W, 3]`` image ('rgb_array') or float32 ``[H, W]`` depth
    ('depth_array'); None for any other mode."""
    H, W = int(size[0]), int(size[1])
    if render_mode == "rgb_array":
        img = vec.render_rgb(camera, H, W)
    elif render_mode == "depth_array":
        img, _ = vec.render_depth(camera, H, W, segmentation=False)
    else:
        return None
    torch.cuda.synchronize(vec.device)
    return img[0].cpu().numpy().copy()
