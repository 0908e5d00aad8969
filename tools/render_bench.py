"""Throughput of render_rgb beside render_depth of the same camera, size and env count, and beside
the env step, per precision (fp64, fp32):

  humanoid_soccer        head_camera, 64 x 64, 4096 envs (two directional lights, one on the torso)
  humanoid_construction  track, 64 x 64, 4096 envs (three shadow-casting directional lights, nv 99)

Each call is timed with device events over --iters calls after --warmup calls and includes the scene
kernel (kinematics from the current qpos) that every render call runs first. ``--dump DIR`` also
writes the first --dump-envs envs' images as binary .ppm files, for someone to look at. Prints one
JSON line. Run on the GPU box: python tools/render_bench.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.ray_bench import timed  # noqa: E402


def write_ppm(path, img):
    """img: uint8 [H, W, 3] numpy"""
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def measure(env, act, camera, hw, iters, warmup, dump, dump_envs, tag):
    n = env.num_envs
    step_ms = timed(lambda: env.step(act), iters, warmup)
    depth_ms = timed(lambda: env.render_depth(camera, hw, hw), iters, warmup)
    rgb_ms = timed(lambda: env.render_rgb(camera, hw, hw), iters, warmup)
    all_ms = timed(lambda: env.render_rgb(camera, hw, hw, depth=True, segmentation=True), iters, warmup)
    rgb, seg = env.render_rgb(camera, hw, hw, segmentation=True)
    torch.cuda.synchronize()
    if dump:
        os.makedirs(dump, exist_ok=True)
        for i in range(min(dump_envs, n)):
            write_ppm(os.path.join(dump, f"{tag}_{camera}_env{i}.ppm"), rgb[i].cpu().numpy())
    px = n * hw * hw
    return {"envs": n, "camera": camera, "height": hw, "width": hw, "lights": len(env.lights), "geoms": int(env.model.ngeom),
            "step_ms": step_ms, "render_depth_ms": depth_ms, "render_rgb_ms": rgb_ms, "render_rgb_depth_seg_ms": all_ms,
            "render_depth_pixels_per_s": px / depth_ms * 1e3, "render_rgb_pixels_per_s": px / rgb_ms * 1e3,
            "rgb_over_depth": rgb_ms / depth_ms, "rgb_over_step": rgb_ms / step_ms,
            "hit_fraction": float((seg >= 0).float().mean()), "mean_rgb": float(rgb.float().mean() / 255.0)}


def soccer(prec, a):
    from mujoco_gymnasium_environments_amd.envs.soccer import SoccerVectorEnv
    env = SoccerVectorEnv(a.envs, precision=prec, seed=1)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    act = (torch.rand(a.envs, env.model.nu, device="cuda", generator=g) * 300 - 150).contiguous()
    return measure(env, act, "head_camera", a.size, a.iters, a.warmup, a.dump, a.dump_envs, f"soccer_{prec}")


def construction(prec, a):
    from mujoco_gymnasium_environments_amd.envs.construction import ACTION_LIMIT, ConstructionVectorEnv
    env = ConstructionVectorEnv(a.envs, precision=prec, seed=1)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    act = ((torch.rand(a.envs, env.model.nu, device="cuda", generator=g) * 2 - 1) * ACTION_LIMIT).contiguous()
    return measure(env, act, "track", a.size, a.iters, a.warmup, a.dump, a.dump_envs, f"construction_{prec}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dump", default=None, help="directory for a few envs' images as binary .ppm")
    ap.add_argument("--dump-envs", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for prec in ("f64", "f32"):
        out[f"soccer_{prec}"] = soccer(prec, a)
        out[f"construction_{prec}"] = construction(prec, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
