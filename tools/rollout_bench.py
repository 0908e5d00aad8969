"""Cost of rollout() beside the work it is made of and beside the Python loop it replaces.

  rollout_ms   (a) one PhysicsBatch.rollout() call: K control sequences of T steps per env, state and
               n_done recorded
  loop_ms      (b) the hand-built composition on the same states: a PhysicsBatch of N K envs and a
               Python loop of T x "write ctrl, step(frames=False), copy time / qpos / qvel out, compare
               warning" (the state reload before each call is outside the timed region)
  step_ms      (c) T plain PhysicsBatch.step(frames=False) calls of those N K envs under the same
               controls (one ctrl write per step, or the steps would follow another, lighter
               trajectory), nothing read back
  ratio_step   (a) / (c);  ratio_loop  (a) / (b)
  spread       max - min over the timed calls of each of the three, ms
  kernels_ms   the begin and record kernels' own device times per call from the torch profiler (the
               record kernel: the sum of its T launches), when it reports device activity

Measured in fp64 for soccer at N = 8, K = 512, T = 32 and bipedal at N = 8, K = 128, T = 32 (a size
whose workspace fits the 1 GiB default) after a few random-action env steps, under controls drawn
uniformly from --ctrl-scale times the action bound (raw controls at the full bound drive most
soccer rollouts into the bad-state reset within 32 steps; `diverged` counts those that ended early).
Each figure is the mean over --iters calls after --warmup calls, timed with device events. Prints
one JSON line.
Run on the GPU box: python tools/rollout_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("soccer", "SoccerVectorEnv", 8, 512, 32), ("bipedal", "BipedalVectorEnv", 8, 128, 32))
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "qfrc_applied", "xfrc_applied", "time")


def timed(fn, iters, warmup, before=None):
    times = []
    for i in range(warmup + iters):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(t0.elapsed_time(t1))
    return sum(times) / len(times), max(times) - min(times)


def kernel_times(fn, iters):
    """Mean device time per call of the kernels whose name holds k_rollout_, by name; {} when the
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
            if "k_rollout_" in e.key and t:
                out["begin" if "begin" in e.key else "record"] = t / 1000.0 / iters
        return out
    except Exception as e:  # noqa: BLE001 - the profiler is optional here
        return {"unavailable": str(e)[:80]}


def run(mod, cls, n, k, t, iters, warmup, ctrl_scale):
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    env = getattr(M, cls)(n, precision="f64", seed=1)
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi).contiguous())
    b = env.batch
    nu = int(b.model.nu)
    lim = float(hi.max()) * ctrl_scale
    ctrl = ((torch.rand(n, k, t, nu, device="cuda", generator=g, dtype=torch.float64) * 2 - 1) * lim).contiguous()
    out = {"envs": n, "rollouts": k, "steps": t, "virtual_envs": n * k}
    call = lambda: b.rollout(ctrl=ctrl, only=("state", "n_done"))  # noqa: E731
    res = call()
    torch.cuda.synchronize()
    out["workspace_MiB"] = sum(w.numel() for w in b._rollout_ws.values()) / 2 ** 20
    out["passes"] = -(-n * k // next(iter(b._rollout_ws))[0])
    out["rollout_ms"], out["rollout_spread"] = timed(call, iters, warmup)
    out["kernels_ms"] = kernel_times(call, 3)
    big = PhysicsBatch(b.model, n * k, precision="f64", native=b.native)
    saved = {f: getattr(b, f).repeat_interleave(k, dim=0).contiguous() for f in STATE}
    flat = ctrl.reshape(n * k, t, nu)
    rec = torch.zeros(n * k, t, b.state_size, dtype=b.dtype, device="cuda")
    done = torch.full((n * k,), t, dtype=torch.int32, device="cuda")

    def restore():
        for f in STATE:
            getattr(big, f).copy_(saved[f])
        big.warning.zero_()
        done.fill_(t)

    def loop():
        for s in range(t):
            big.ctrl[:, :nu] = flat[:, s]
            big.step(frames=False)
            rec[:, s, 0] = big.time
            rec[:, s, 1:1 + big.qpos.shape[1]] = big.qpos
            rec[:, s, 1 + big.qpos.shape[1]:] = big.qvel
            torch.minimum(done, torch.where(big.warning > 0, s, t).to(torch.int32), out=done)

    def plain():
        for s in range(t):
            big.ctrl[:, :nu] = flat[:, s]
            big.step(frames=False)

    out["loop_ms"], out["loop_spread"] = timed(loop, iters, warmup, before=restore)
    loop_state = rec.clone()
    out["step_ms"], out["step_spread"] = timed(plain, iters, warmup, before=restore)
    out["ratio_step"] = out["rollout_ms"] / out["step_ms"]
    out["ratio_loop"] = out["rollout_ms"] / out["loop_ms"]
    torch.cuda.synchronize()
    out["finite"] = bool(torch.isfinite(res.state).all())
    out["diverged"] = int((res.n_done < t).sum())
    # rollouts that never diverged hold the loop's states bit for bit
    ok = (res.n_done.reshape(-1) == t)
    out["equal_loop"] = bool(torch.equal(res.state.reshape(n * k, t, -1)[ok], loop_state[ok]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="soccer | bipedal")
    ap.add_argument("--ctrl-scale", type=float, default=0.2)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for mod, cls, n, k, t in CASES:
        if a.only and a.only != mod:
            continue
        out[f"{mod}_f64"] = run(mod, cls, n, k, t, a.iters, a.warmup, a.ctrl_scale)
        print(f"# {mod}_f64: {out[f'{mod}_f64']}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
