"""Cost of rollout_feedback() beside the open-loop rollout() and beside the Python loop it replaces,
and the split of one solve_ilqr iteration.

  feedback_ms   (a) one PhysicsBatch.rollout_feedback() call with dense gains, k_ff and alpha: K
                closed-loop rollouts of T steps per env; state, n_done, ctrl and warmstart recorded
  rollout_ms    (b) one PhysicsBatch.rollout() call of the same N, K, T under the controls (a) recorded
  loop_ms       (c) the hand-written loop on a PhysicsBatch of N K envs: per step state_difference,
                the torch feedback (einsum over the gains, clamp), the ctrl write, step(frames=False)
                and the copies of state, ctrl and warm start (the state reload is outside the timing)
  ratio_open    (a) / (b): what closing the loop costs;  ratio_loop  (a) / (c)
  launches      kernel launches the closed-loop call issues beyond the open-loop one, per recorded
                step and pass: counted from the code path (run_rollout launches k_rollout_feedback
                once before each mgx_step when a feedback law is given, and nothing else differs)
  ilqr          one solve_ilqr iteration at N envs, horizon T, split with device events into
                derivatives (transition_fd_along), backward (lqr_backward, torch) and line search
                (one rollout_feedback call of the 8 step sizes, and its costs); beside the torch
                backward pass the fused one (lqr_backward_fused, one mgx_lqr_backward launch) on the
                same inputs, plain (backward_fused) and with the model's control range as bounds on
                the step (backward_fused_box), all at the Levenberg parameter mu: 1e-6 raised by 10
                until the torch and the fused plain pass factorise every Q_uu (a pass that meets a
                failed pivot is not comparable: the kernel ends that env's time loop there), and the largest difference of the plain fused gains
                and k_ff from torch's over max(1, |k_ff|, |gain|) (fused_vs_torch), next to the same
                measure between the torch pass and itself with every entry of A moved by one rounding
                error (torch_vs_torch_rounded_inputs): what the recursion's conditioning alone gives
  spread        max - min over the timed calls, ms

Soccer at N = 8, K = 64, T = 32 and assembly at N = 8, K = 64, T = 16 with nsub = 10, fp64, after a few
random-action env steps; construction (2nv = 198) at N = 8, T = 8 for the backward passes only. Each figure is the mean over --iters calls after --warmup calls, timed
with device events. Prints one JSON line.
Run on the GPU box: python tools/ilqr_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.rollout_bench import STATE, timed  # noqa: E402

# (module, class, N, K, T, nsub, full): full = every figure; otherwise the backward passes only
CASES = (("soccer", "SoccerVectorEnv", 8, 64, 32, 1, True), ("assembly", "AssemblyVectorEnv", 8, 64, 16, 10, True),
         ("construction", "ConstructionVectorEnv", 8, 64, 8, 1, False))


def run(mod, cls, n, k, t, nsub, iters, warmup, full=True):
    from mujoco_gymnasium_environments_amd import ilqr
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    env = getattr(M, cls)(n, precision="f64", **({"seed": 1} if mod == "soccer" else {}))
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi).contiguous())
    b = env.batch
    m = b.model
    nu, nv, nq = int(m.nu), int(m.nv), int(m.nq)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float64)  # noqa: E731
    rng = torch.as_tensor(m.actuator_ctrlrange, dtype=torch.float64, device="cuda").reshape(-1, 2)
    lim = torch.as_tensor(m.actuator_ctrllimited, device="cuda") != 0
    width = torch.where(lim, rng[:, 1] - rng[:, 0], torch.full_like(rng[:, 0], 10.0))
    u_nom = (0.1 * width * rnd(n, t, nu)).contiguous()
    x0 = b.get_state()
    out = {"envs": n, "rollouts": k, "steps": t, "nsub": nsub, "nv": nv, "nu": nu, "launches": 1}
    if full:
        nom = b.rollout(ctrl=u_nom[:, None].contiguous(), nsub=nsub)
        x_nom = torch.cat([x0[:, None], nom.state[:, 0, :-1]], dim=1).contiguous()
        kw = dict(x_nom=x_nom, k_ff=(0.02 * width * rnd(n, t, nu)).contiguous(),
                  alpha=torch.rand(n, k, device="cuda", generator=g, dtype=torch.float64).contiguous(),
                  gain=(0.05 * rnd(n, t, nu, 2 * nv)).contiguous(),
                  initial_state=b.state_integrate(x0[:, None].repeat(1, k, 1).contiguous(), (0.005 * rnd(n, k, 2 * nv)).contiguous()),
                  nsub=nsub)
        closed = lambda: b.rollout_feedback(u_nom, **kw)  # noqa: E731
        res = closed()
        torch.cuda.synchronize()
        ctrl = res.ctrl.clone()
        opened = lambda: b.rollout(ctrl=ctrl, initial_state=kw["initial_state"], nsub=nsub, only=("state", "n_done"))  # noqa: E731
        ref = opened()
        torch.cuda.synchronize()
        out["equal_open"] = bool(torch.equal(ref.state, res.state))
        out["diverged"] = int((res.n_done < t).sum())
        out["feedback_ms"], out["feedback_spread"] = timed(closed, iters, warmup)
        out["rollout_ms"], out["rollout_spread"] = timed(opened, iters, warmup)

        big = PhysicsBatch(m, n * k, precision="f64", native=b.native)
        saved = {f: getattr(b, f).repeat_interleave(k, dim=0).contiguous() for f in STATE}
        start = kw["initial_state"].reshape(n * k, -1)
        saved["time"], saved["qpos"], saved["qvel"] = start[:, 0].clone(), start[:, 1:1 + nq].clone(), start[:, 1 + nq:].clone()
        rec = torch.zeros(n * k, t, b.state_size, dtype=b.dtype, device="cuda")
        rec_u = torch.zeros(n * k, t, nu, dtype=b.dtype, device="cuda")
        rec_w = torch.zeros(n * k, t, nv, dtype=b.dtype, device="cuda")
        e_of = torch.arange(n, device="cuda").repeat_interleave(k)
        al = kw["alpha"].reshape(n * k, 1)

        def restore():
            for f in STATE:
                getattr(big, f).copy_(saved[f])
            big.warning.zero_()

        def loop():
            for s in range(t):
                dx = big.state_difference(big.get_state(), x_nom[e_of, s])
                u = u_nom[e_of, s] + al * kw["k_ff"][e_of, s] + torch.einsum("vij,vj->vi", kw["gain"][e_of, s], dx)
                u = torch.where(lim, torch.minimum(torch.maximum(u, rng[:, 0]), rng[:, 1]), u)
                rec_u[:, s], rec_w[:, s] = u, big.qacc_warmstart
                big.ctrl[:, :nu] = u
                big.step(nsub, frames=False)
                rec[:, s] = big.get_state()

        out["loop_ms"], out["loop_spread"] = timed(loop, iters, warmup, before=restore)
        out["ratio_open"] = out["feedback_ms"] / out["rollout_ms"]
        out["ratio_loop"] = out["feedback_ms"] / out["loop_ms"]

    # one iLQR iteration, split
    goal = x0.clone()
    goal[:, 1:1 + min(nq, 3)] += 0.02
    w = tuple(torch.as_tensor(x, dtype=b.dtype, device="cuda").expand(n, d).contiguous()
              for x, d in ((1.0, 2 * nv), (10.0, 2 * nv), (1e-3, nu)))
    prob = ilqr.IlqrProblem(x0, goal, t, *w)
    one = b.rollout_feedback(u_nom, nsub=nsub)
    state = torch.cat([x0[:, None], one.state[:, 0]], dim=1).contiguous()
    uc, warm = one.ctrl[:, 0].clone(), one.warmstart[:, 0].clone()
    eye_x, eye_u = torch.eye(2 * nv, dtype=b.dtype, device="cuda"), torch.eye(nu, dtype=b.dtype, device="cuda")
    hold = {}

    def derivatives():
        hold["lin"] = b.transition_fd_along(state[:, :t].contiguous(), uc, warmstart=warm, nsub=nsub)

    def backward():
        lin = hold["lin"]
        _, dx = ilqr.trajectory_cost(b, prob, state, uc, w)
        hold["bw"] = ilqr.lqr_backward(lin.A, lin.B, w[0][:, None] * dx[:, :t], (w[0][:, None, :, None] * eye_x).expand(n, t, -1, -1),
                                       w[2][:, None] * uc, (w[2][:, None, :, None] * eye_u).expand(n, t, -1, -1),
                                       torch.zeros(n, t, nu, 2 * nv, dtype=b.dtype, device="cuda"), w[1] * dx[:, t],
                                       w[1][:, :, None] * eye_x, hold["mu"])

    alphas = torch.tensor(ilqr.DEFAULT_ALPHAS, dtype=b.dtype, device="cuda").repeat(n, 1).contiguous()
    x0k = x0[:, None].repeat(1, alphas.shape[1], 1).contiguous()

    def search():
        bw = hold["bw"]
        rr = b.rollout_feedback(uc, x_nom=state[:, :t].contiguous(), k_ff=torch.nan_to_num(bw.k_ff).contiguous(), alpha=alphas,
                                gain=torch.nan_to_num(bw.gain).contiguous(), initial_state=x0k, nsub=nsub)
        ilqr.trajectory_cost(b, prob, torch.cat([x0k[:, :, None], rr.state], dim=2), rr.ctrl, w)

    lo_c, hi_c = ilqr.control_range(m, nu, b.dtype, "cuda")

    def fused(box):
        def fn():
            lin = hold["lin"]
            _, dx = ilqr.trajectory_cost(b, prob, state, uc, w)
            lim = dict(lo=lo_c - uc, hi=hi_c - uc) if box else {}
            hold["fused"] = ilqr.lqr_backward_fused(b, lin.A, lin.B, w[0][:, None] * dx[:, :t], None, w[2][:, None] * uc, None, None,
                                                    w[1] * dx[:, t], w[1][:, :, None] * eye_x, hold["mu"],
                                                    lxx_diag=w[0][:, None].expand(n, t, -1), luu_diag=w[2][:, None].expand(n, t, -1),
                                                    **lim)
        return fn

    # the Levenberg parameter at which the passes are timed: 1e-6, raised by 10 (outside the timing) until
    # both the torch and the fused plain pass factorise every Q_uu of every env, as solve's schedule would
    # raise it: a pass that meets a failed pivot is not comparable (the kernel ends that env's time loop
    # there, torch's cholesky_ex goes on through all T steps)
    it = {}
    derivatives()
    hold["mu"], plain = 1e-6, fused(False)
    while True:
        backward()
        plain()
        torch.cuda.synchronize()
        if (int(hold["bw"].info.abs().max()) == 0 and int(hold["fused"].info.abs().max()) == 0) or hold["mu"] > 1e10:
            break
        hold["mu"] *= 10.0
    it["mu"] = hold["mu"]
    stages = (("derivatives", derivatives), ("backward", backward), ("backward_fused", fused(False)),
              ("backward_fused_box", fused(True)), ("line_search", search))
    for name, fn in stages if full else stages[1:4]:
        it[f"{name}_ms"], it[f"{name}_spread"] = timed(fn, iters, warmup)
        if name == "backward_fused":
            bw, fu = hold["bw"], hold["fused"]
            scale = max(1.0, float(bw.k_ff.abs().max()), float(bw.gain.abs().max()))
            it["fused_vs_torch"] = max(float((bw.k_ff - fu.k_ff).abs().max()), float((bw.gain - fu.gain).abs().max())) / scale
            it["info_torch"], it["info_fused"] = int(bw.info.abs().max()), int(fu.info.abs().max())
            # the yardstick for that difference: the torch pass against itself with every entry of A moved by one
            # rounding error (x (1 +- 2^-52)), by the same measure: what the recursion's conditioning alone gives
            lin, keep = hold["lin"], hold["lin"].A.clone()
            sign = torch.where(torch.rand(keep.shape, device="cuda", generator=g) < 0.5, -1.0, 1.0).to(keep.dtype)
            lin.A.copy_(keep * (1.0 + 2.0 ** -52 * sign))
            backward()
            pert = hold["bw"]
            lin.A.copy_(keep)
            it["torch_vs_torch_rounded_inputs"] = max(float((bw.k_ff - pert.k_ff).abs().max()),
                                                      float((bw.gain - pert.gain).abs().max())) / scale
            backward()
        if name == "backward_fused_box":
            it["box_clamped_share"] = float((hold["fused"].free == 0).float().mean())
            it["box_info"] = int(hold["fused"].info.abs().max())
    it["physics_steps_derivatives"] = n * t * (1 + 2 * nv + nu) * nsub
    it["physics_steps_line_search"] = n * t * alphas.shape[1] * nsub
    it["cholesky_solves_backward"] = n * t
    out["ilqr"] = it
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="soccer | assembly | construction")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for mod, cls, n, k, t, nsub, full in CASES:
        if a.only and a.only != mod:
            continue
        out[f"{mod}_f64"] = run(mod, cls, n, k, t, nsub, a.iters, a.warmup, full)
        print(f"# {mod}_f64: {out[f'{mod}_f64']}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
