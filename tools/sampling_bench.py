"""Cost of scoring K sampled control sequences per env: the fused rollout cost beside the route it
replaces and beside the steps alone.

  fused_ms   (a) rollout(ctrl=, cost=, only=("cost",)): mgx_rollout_cost, no trajectory recorded
  torch_ms   (b) the route without it: rollout recording `state` [N, K, T, nstate] and n_done, then
             ilqr.trajectory_cost in torch (state_difference, squares, reductions) and the +inf of
             diverged rollouts
  steps_ms   (c) rollout(only=("n_done",)): the same steps, nothing scored, no state recorded
  ratio_steps  (a) / (c);  ratio_torch  (a) / (b)
  spread       max - min over the timed calls of each of the three, ms
  peak_MiB     torch.cuda.max_memory_allocated over the first call of (a), and of (b), above what was
               allocated before it: the outputs the route keeps and its temporaries (the rollout
               workspace, which both share, is allocated before either); state_MiB is
               N K T nstate 8 bytes, the tensor (a) does without
  max_rel_diff the largest relative difference of the two routes' finite costs (summation order)

The three variants alternate inside one loop (a, b, c, a, b, c ...), so a drift of the clocks falls
on all of them. fp64, soccer at N = 8, K = 512, T = 32 and bipedal at N = 8, K = 128, T = 32 after a
few random-action env steps, under controls drawn as in tools/rollout_bench.py. Each figure is the
mean over --iters calls after --warmup calls, timed with device events. Prints one JSON line.
Run on the GPU box: python tools/sampling_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("soccer", "SoccerVectorEnv", 8, 512, 32), ("bipedal", "BipedalVectorEnv", 8, 128, 32))


def timed_alternating(fns, iters, warmup):
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[j].append(t0.elapsed_time(t1))
    return [(sum(t) / len(t), max(t) - min(t)) for t in times]


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def run(mod, cls, n, k, t, iters, warmup, ctrl_scale):
    from mujoco_gymnasium_environments_amd import ilqr
    from mujoco_gymnasium_environments_amd.rollouts import RolloutCost
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    env = getattr(M, cls)(n, precision="f64", seed=1)
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi).contiguous())
    b = env.batch
    nu, nv = int(b.model.nu), int(b.model.nv)
    lim = float(hi.max()) * ctrl_scale
    ctrl = ((torch.rand(n, k, t, nu, device="cuda", generator=g, dtype=torch.float64) * 2 - 1) * lim).contiguous()
    x0 = b.get_state()
    goal = x0.clone()
    goal[:, 1 + int(b.model.nq):] = 0  # come to rest where it stands
    w = tuple(torch.full((n, width), val, dtype=torch.float64, device="cuda")
              for width, val in ((2 * nv, 1.0), (2 * nv, 10.0), (nu, 1e-3)))
    cost = RolloutCost(goal=goal, w_x=w[0], w_xf=w[1], w_u=w[2])
    problem = ilqr.IlqrProblem(x0, goal, t, *w)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device="cuda")
    x0k = x0[:, None, None, :].expand(n, k, 1, x0.shape[1])

    def fused():
        return b.rollout(ctrl=ctrl, cost=cost, only=("cost",)).cost

    def torch_route():
        r = b.rollout(ctrl=ctrl, only=("state", "n_done"))
        c, _ = ilqr.trajectory_cost(b, problem, torch.cat([x0k, r.state], dim=2), ctrl, w)
        return torch.where(r.n_done < t, inf, c)

    def steps():
        return b.rollout(ctrl=ctrl, only=("n_done",)).n_done

    # the workspace both routes share is allocated up front, so that neither peak includes it
    _, ws = b._rollout_workspace(None, False, n * k)
    out = {"envs": n, "rollouts": k, "steps": t, "virtual_envs": n * k, "workspace_MiB": ws.numel() / 2 ** 20,
           "state_MiB": n * k * t * b.state_size * 8 / 2 ** 20}
    out["fused_peak_MiB"], ca = peak_of(fused)
    ca = ca.clone()
    out["torch_peak_MiB"], cb = peak_of(torch_route)
    both = torch.isfinite(ca) & torch.isfinite(cb)
    out["diverged"] = int((~torch.isfinite(ca)).sum())
    out["same_diverged"] = bool(torch.equal(torch.isfinite(ca), torch.isfinite(cb)))
    out["max_rel_diff"] = float(((ca - cb).abs() / cb.abs().clamp(min=1e-300))[both].max()) if bool(both.any()) else None
    (fa, sa), (fb, sb), (fc, sc) = timed_alternating((fused, torch_route, steps), iters, warmup)
    out.update(fused_ms=fa, fused_spread=sa, torch_ms=fb, torch_spread=sb, steps_ms=fc, steps_spread=sc,
               ratio_steps=fa / fc, ratio_torch=fa / fb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
