"""Cost of solve_ik() beside the Python loop it replaces.

  native_ms   one PhysicsBatch.solve_ik() call: --iters-ik damped-least-squares updates (tol = 0) for
              every env in one launch
  loop_ms     the same updates composed by hand on the same states: per iteration write qpos into a
              work batch, jac(), the error in torch (orientation from a torch quaternion chain over
              the hinges above the target), torch.linalg.solve on J J' + lambda^2 I, the step limit,
              a torch mj_integratePos (hinge, slide and one free joint) and the limit clamp
  ratio       native_ms / loop_ms;  per_iter_us  native_ms / iterations
  spread      max - min over the timed calls, ms
  max_diff    max |qpos_native - qpos_loop| after the last iteration (the two run the same algorithm)
  residual_start / residual_end   [median, max] over the envs of the weighted error norm before and
              after; status_counts: envs that ended converged / at max_iter / failed

Cases, 4096 envs, fp64 and (soccer) fp32, after a few random-action env steps: assembly, one 6-DoF target
(ee_site position + orientation over the arm's seven hinges); soccer, two foot positions over
every dof. Targets: the current poses moved by up to 5 cm and, on the arm, turned by up to 0.2 rad.
Each figure is the mean over --iters calls after --warmup calls, timed with device events. Prints
one JSON line.
Run on the GPU box: python tools/ik_bench.py
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARM = ("j1_shoulder_pan", "j2_shoulder_tilt", "j3_elbow", "j4_wrist_roll", "j5_wrist_pitch", "j6_wrist_yaw",
       "j7_gripper_base")
# module, class, jac_points keywords, rot_weight, joints that may move, damping
CASES = (("assembly", "AssemblyVectorEnv", dict(site="ee_site"), 1.0, ARM, 0.01),
         ("soccer", "SoccerVectorEnv", dict(geom=["left_foot", "right_foot"]), 0.0, None, 0.05))


def timed(fn, iters, warmup):
    times = []
    for i in range(warmup + iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(t0.elapsed_time(t1))
    return sum(times) / len(times), max(times) - min(times)


def qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def rotvec(q):
    v = q[..., 1:]
    n = v.norm(dim=-1, keepdim=True)
    ang = 2 * torch.atan2(n, q[..., :1])
    ang = torch.where(ang > np.pi, ang - 2 * np.pi, ang)
    return torch.where(n > 0, v / n.clamp_min(1e-300) * ang, torch.zeros_like(v))


class Loop:
    """The hand-built iteration on a work batch that shares the env's model."""

    def __init__(self, b, points, tgt, damping, max_step):
        from mujoco_gymnasium_environments_amd.batch import PhysicsBatch
        m = self.m = b.model
        self.work = PhysicsBatch(m, b.n, precision="f32" if b.dtype == torch.float32 else "f64", native=b.native)
        self.points, self.tgt, self.lam2, self.max_step = points, tgt, damping * damping, max_step
        dev, dt = b.device, b.dtype
        t = lambda a, d=dt: torch.as_tensor(np.asarray(a), dtype=d, device=dev)  # noqa: E731
        jt, qa, da = np.asarray(m.jnt_type), np.asarray(m.jnt_qposadr), np.asarray(m.jnt_dofadr)
        assert not (jt == 1).any(), "the torch mj_integratePos here has no ball joints"
        sc = np.flatnonzero(jt >= 2)
        self.sq, self.sd = t(qa[sc], torch.long), t(da[sc], torch.long)
        self.free = [(int(qa[j]), int(da[j])) for j in np.flatnonzero(jt == 0)]
        lim = np.flatnonzero((jt >= 2) & (np.asarray(m.jnt_limited) != 0))
        mask = np.ones(m.nv, bool) if tgt.dof_mask is None else tgt.dof_mask.cpu().numpy().astype(bool)
        lim = lim[mask[da[lim]]]
        rng = np.asarray(m.jnt_range, dtype=np.float64).reshape(-1, 2)
        self.lq, self.lo, self.hi = t(qa[lim], torch.long), t(rng[lim, 0]), t(rng[lim, 1])
        self.mask = t(mask.astype(np.float64))
        self.rot = tgt.rot_weight[0] > 0
        if self.rot:  # the hinge chain from the world to the target's body: (body_quat, axis, qpos address, qpos0)
            chain, body = [], int(points.body[0])
            while body > 0:
                js = [j for j in range(m.njnt) if int(m.jnt_bodyid[j]) == body]
                assert all(int(jt[j]) == 3 for j in js), "orientation chain: hinges only"
                chain.append((t(np.asarray(m.body_quat).reshape(-1, 4)[body]),
                              [(t(np.asarray(m.jnt_axis).reshape(-1, 3)[j]), int(qa[j]), float(m.qpos0[qa[j]])) for j in js]))
                body = int(m.body_parentid[body])
            self.chain = chain[::-1]

    def frame_quat(self, q):
        cur = torch.zeros(q.shape[0], 4, dtype=q.dtype, device=q.device)
        cur[:, 0] = 1
        for bq, joints in self.chain:
            cur = qmul(cur, bq.expand_as(cur))
            for axis, a, q0 in joints:
                half = 0.5 * (q[:, a] - q0)
                cur = qmul(cur, torch.cat([torch.cos(half)[:, None], torch.sin(half)[:, None] * axis], 1))
        return qmul(cur, self.tgt.quat[0].expand_as(cur))

    def integrate(self, q, d):
        q = q.clone()
        q[:, self.sq] += d[:, self.sd]
        for a, da in self.free:
            q[:, a:a + 3] += d[:, da:da + 3]
            w = d[:, da + 3:da + 6]
            ang = w.norm(dim=1, keepdim=True)
            ax = torch.where(ang > 1e-15, w / ang.clamp_min(1e-300), torch.tensor([1.0, 0, 0], dtype=q.dtype, device=q.device))
            dq = torch.cat([torch.cos(0.5 * ang), torch.sin(0.5 * ang) * ax], 1)
            quat = q[:, a + 3:a + 7]
            q[:, a + 3:a + 7] = qmul(quat / quat.norm(dim=1, keepdim=True), dq)
        return q

    def clamp(self, q):
        q[:, self.lq] = torch.minimum(torch.maximum(q[:, self.lq], self.lo), self.hi)
        return q

    def run(self, q0, target_pos, target_quat, iters):
        q = self.clamp(q0.clone())
        n = q.shape[0]
        eye = torch.eye(6 if self.rot else 3 * len(self.points), dtype=q.dtype, device=q.device) * self.lam2
        for _ in range(iters):
            self.work.qpos.copy_(q)
            r = self.work.jac(self.points)
            if self.rot:
                tq = target_quat[:, 0] / target_quat[:, 0].norm(dim=1, keepdim=True)
                cur = self.frame_quat(q)
                er = rotvec(qmul(tq, cur * torch.tensor([1.0, -1, -1, -1], dtype=q.dtype, device=q.device)))
                e = torch.cat([target_pos[:, 0] - r.point[:, 0], er], 1)
                J = torch.cat([r.jacp[:, 0], r.jacr[:, 0]], 1) * self.mask
            else:
                e = (target_pos - r.point).reshape(n, -1)
                J = r.jacp.reshape(n, -1, self.m.nv) * self.mask
            y = torch.linalg.solve(J @ J.transpose(1, 2) + eye, e)
            d = (J.transpose(1, 2) @ y[:, :, None])[:, :, 0]
            s = d.abs().amax(dim=1, keepdim=True)
            d = torch.where(s > self.max_step, d * (self.max_step / s), d)
            q = self.clamp(self.integrate(q, d))
        return q


def run(mod, cls, kw, rot, joints, damping, prec, n, ik_iters, iters, warmup):
    M = importlib.import_module(f"mujoco_gymnasium_environments_amd.envs.{mod}")
    E = getattr(M, cls)
    env = E(n, precision=prec, seed=1) if E.SEEDED else E(n, precision=prec)
    env.reset()
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device="cuda").reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(5):  # a fifth of the action bound: soccer's full-range torques throw some envs far off
        env.step(((torch.rand(n, hi.numel(), device="cuda", generator=g) * 2 - 1) * hi * 0.2).contiguous())
    b = env.batch
    pts = env.jac_points(**kw)
    tgt = env.ik_targets(pts, pos_weight=1.0, rot_weight=rot, dofs=joints)
    loop = Loop(b, pts, tgt, damping, 0.3)
    here = b.jac(pts).point.clone()
    tp = (here + (torch.rand(here.shape, device="cuda", generator=g, dtype=torch.float64).to(b.dtype) - 0.5) * 0.1).contiguous()
    tq = None
    if rot:
        w = (torch.rand(n, 3, device="cuda", generator=g, dtype=torch.float64).to(b.dtype) - 0.5) * 0.4
        ang = w.norm(dim=1, keepdim=True)
        dq = torch.cat([torch.cos(0.5 * ang), torch.sin(0.5 * ang) * w / ang], 1)
        tq = qmul(dq, loop.frame_quat(b.qpos))[:, None].contiguous()
    call = lambda: env.solve_ik(tgt, tp, target_quat=tq, damping=damping, max_step=0.3, tol=0.0, max_iter=ik_iters)  # noqa: E731
    res = call()
    torch.cuda.synchronize()
    out = {"envs": n, "points": len(pts), "rows": 6 if rot else 3 * len(pts), "iterations": ik_iters}
    out["native_ms"], out["native_spread"] = timed(call, iters, warmup)
    q0 = b.qpos.clone()
    hand = lambda: loop.run(q0, tp, tq, ik_iters)  # noqa: E731
    q_loop = hand()
    out["loop_ms"], out["loop_spread"] = timed(hand, iters, warmup)
    out["ratio"] = out["native_ms"] / out["loop_ms"]
    out["per_iter_us"] = 1000.0 * out["native_ms"] / max(ik_iters, 1)
    out["max_diff"] = float((res.qpos - q_loop).abs().max())
    start = env.solve_ik(tgt, tp, target_quat=tq, damping=damping, max_iter=0).residual.clone()
    res = call()
    torch.cuda.synchronize()
    out["residual_start"] = [float(start.median()), float(start.max())]   # median, max over the envs
    out["residual_end"] = [float(res.residual.median()), float(res.residual.max())]
    out["status_counts"] = [int((res.status == k).sum()) for k in range(3)]  # converged, max_iter, failed
    out["short_of_iterations"] = int((res.iters != ik_iters).sum())
    out["qpos_abs_max"] = float(b.qpos.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters-ik", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="assembly | soccer")
    ap.add_argument("--precision", default="f64,f32")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for mod, cls, kw, rot, joints, damping in CASES:
        if a.only and a.only != mod:
            continue
        for prec in a.precision.split(","):
            if mod == "assembly" and prec != "f64":
                continue  # the assembly env runs in fp64 only
            key = f"{mod}_{prec}"
            out[key] = run(mod, cls, kw, rot, joints, damping, prec, a.envs, a.iters_ik, a.iters, a.warmup)
            print(f"# {key}: {out[key]}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
