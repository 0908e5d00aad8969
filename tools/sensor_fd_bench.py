"""Cost of sensor_fd() beside the work it is made of: sensordata() of a PhysicsBatch of N C envs
(C = 1 + 2 nv + nu virtual envs per env) holding the same states, which is the composition a user
had to run by hand before (plus the host-side perturbing and differencing, not timed here).

  sensor_fd_ms    one sensor_fd() call (forward differences, every output)
  compose_ms      sensordata() of N C envs, same run; measured twice, before and after sensor_fd,
                  so that the table shows the composition's own run-to-run spread
  ratio           sensor_fd_ms / mean(compose_ms)
  kernels_ms      the expand and k_sens_diff kernels' own device times from the torch profiler, when
                  it reports device activity

Measured for martial fp64 (27 values, the forward kernel runs) and assembly fp64 (16 values, no
forward) after a few random-action env steps, N the smallest with N C >= 4096. Each figure is the
mean over --iters calls after --warmup calls, timed with device events. Prints one JSON line. Run
on the GPU box: python tools/sensor_fd_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("martial", "MartialArtsVectorEnv"), ("assembly", "AssemblyVectorEnv"))
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "qfrc_applied", "xfrc_applied", "time")


def timed(fn, iters, warmup):
    total = 0.0
    for i in range(warmup + iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            total += t0.elapsed_time(t1)
    return total / iters


def kernel_times(fn, iters):
    """Mean device time per call of the expand and difference kernels, by name; {} when the
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
            for key, name in (("k_fd_expand", "expand"), ("k_sens_diff", "sens_diff"), ("k_sensor", "sensor"),
                              ("k_forward", "forward")):
                if key in e.key and t:
                    out[name] = out.get(name, 0.0) + t / 1000.0 / iters
        return out
    except Exception as e:  # noqa: BLE001 - the profiler is optional here
        return {"unavailable": str(e)[:80]}


def run(mod, cls, iters, warmup):
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    model = getattr(M, f"{mod}_model")()
    c = 1 + 2 * int(model.nv) + int(model.nu)
    n = -(-4096 // c)
    env = getattr(M, cls)(n, precision="f64")
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi).contiguous())
    b = env.batch
    assert c == b.sensor_fd_columns()
    out = {"envs": n, "columns": c, "virtual_envs": n * c, "nsensordata": int(b.model.nsensordata)}
    big = PhysicsBatch(b.model, n * c, precision="f64", native=b.native)
    for f in STATE:
        getattr(big, f).copy_(getattr(b, f).repeat_interleave(c, dim=0))
    first = timed(lambda: big.sensordata(), iters, warmup)
    out["sensor_fd_ms"] = timed(lambda: b.sensor_fd(), iters, warmup)
    out["compose_ms"] = [first, timed(lambda: big.sensordata(), iters, warmup)]
    out["ratio"] = out["sensor_fd_ms"] / (sum(out["compose_ms"]) / 2)
    out["kernels_ms"] = kernel_times(lambda: b.sensor_fd(), iters)
    res = b.sensor_fd()
    torch.cuda.synchronize()
    out["finite"] = bool(torch.isfinite(res.C).all() and torch.isfinite(res.D).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for mod, cls in CASES:
        out[f"{mod}_f64"] = run(mod, cls, a.iters, a.warmup)
        print(f"# {mod}_f64: {out[f'{mod}_f64']}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
