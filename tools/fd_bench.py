"""Cost of transition_fd() beside the work it is made of: a plain PhysicsBatch.step() of N C envs
(C = 1 + 2 nv + nu virtual envs per env), which is what a user had to launch by hand before.

  fd_ms        one transition_fd() call (forward differences, nsub = 1, every output)
  step_ms      PhysicsBatch.step(frames=False) of N C envs holding the same states, same run
  ratio        fd_ms / step_ms
  kernels_ms   the expand and difference kernels' own device times from the torch profiler, when it
               reports device activity

Measured for soccer fp64 at N = 64 and bipedal fp64 at N = 16 after a few random-action env steps.
Each figure is the mean over --iters calls after --warmup calls, timed with device events; the
plain step is restored to the same states before every timed call (outside the timed region).
Prints one JSON line. Run on the GPU box: python tools/fd_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("soccer", "SoccerVectorEnv", 64), ("bipedal", "BipedalVectorEnv", 16))
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "qfrc_applied", "xfrc_applied", "time")


def timed(fn, iters, warmup, before=None):
    total = 0.0
    for i in range(warmup + iters):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            total += t0.elapsed_time(t1)
    return total / iters


def kernel_times(fn, iters):
    """Mean device time per call of the kernels whose name holds k_fd_, by name; {} when the
    profiler reports no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            if "k_fd_" in e.key and t:
                out["expand" if "expand" in e.key else "diff"] = t / 1000.0 / iters
        return out
    except Exception as e:  # noqa: BLE001 - the profiler is optional here
        return {"unavailable": str(e)[:80]}


def run(mod, cls, n, iters, warmup):
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    env = getattr(M, cls)(n, precision="f64", seed=1)
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi).contiguous())
    b = env.batch
    c = b.fd_columns()
    out = {"envs": n, "columns": c, "virtual_envs": n * c}
    out["fd_ms"] = timed(lambda: b.transition_fd(), iters, warmup)
    out["kernels_ms"] = kernel_times(lambda: b.transition_fd(), iters)
    big = PhysicsBatch(b.model, n * c, precision="f64", native=b.native)
    saved = {f: getattr(b, f).repeat_interleave(c, dim=0).contiguous() for f in STATE}

    def restore():
        for f in STATE:
            getattr(big, f).copy_(saved[f])

    out["step_ms"] = timed(lambda: big.step(frames=False), iters, warmup, before=restore)
    out["ratio"] = out["fd_ms"] / out["step_ms"]
    res = b.transition_fd()
    torch.cuda.synchronize()
    out["finite"] = bool(torch.isfinite(res.A).all() and torch.isfinite(res.B).all())
    out["warning"] = int(res.warning.sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for mod, cls, n in CASES:
        out[f"{mod}_f64"] = run(mod, cls, n, a.iters, a.warmup)
        print(f"# {mod}_f64: {out[f'{mod}_f64']}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
