// mgx_rollout.hip — open-loop rollouts (MuJoCo's mujoco.rollout [ext]) and their C-ABI:
// mgx_rollout_bytes, mgx_rollout (include/mgx.h), and the closed-loop
// mgx_rollout_feedback, which adds k_rollout_feedback before every mgx_step: the
// step's ctrl from the virtual env's own state; and mgx_rollout_cost, either of the
// two with k_rollout_cost_begin after k_rollout_begin and k_rollout_cost before every
// k_rollout_record: the rollout's cost accumulated from the workspace, so that no trajectory has to
// be recorded to score it.
//
// Rollout k of env e is virtual env v = e K + k. A pass materialises a range of v in the caller's
// workspace (the virtual-env workspace of mgx_transition_fd held for T steps instead of one) and
// steps it with mgx_step itself, so a rollout is bit for bit the step() the user runs:
//   k_rollout_begin   one wave per virtual env: copies the env's state rows, or an initial_state /
//                     initial_warmstart row, the applied forces and the step-0 ctrl (coalesced),
//                     zeroes warning / overflow and writes the live flag;
//   per recorded step t:
//     mgx_step        on the workspace's mgx_state, nsub substeps, no frames, masked by the live flags;
//     mgx_forward + mgx_sensor   (sensordata requested) at the new state into the staging rows;
//     k_rollout_record  one wave per virtual env: the state row, the sensordata row, the next
//                     step's ctrl; on divergence n_done, the padding rows and the live flag.
// No atomics anywhere: results are bit-reproducible.
#include "mgx_internal.h"
#include "mgx_manifold.h"
#include "mgx_rollout.h"
#include "mgx_sensor.h"

using namespace mgx;

namespace {

// ------------------------------------------------------------------ begin
// Block b of the pass is virtual env v = v0 + b in slot b.
template <typename T>
__global__ void __launch_bounds__(64) k_rollout_begin(mgx_state s, RolloutBuf<T> w, int v0, const uint8_t* mask) {
  const int b = blockIdx.x, l = threadIdx.x;
  const int v = v0 + b, env = v / w.K, k = v - env * w.K;
  const bool on = !mask || mask[env] != 0;  // one byte, the same for every lane
  if (l == 0) w.live[b] = on ? 1 : 0;
  if (!on) return;
  const int nq = w.nq, nv = w.nv, nu = w.nu, nx = w.nx;
  const size_t nstate = (size_t)1 + nq + nv;
  const T* row = w.in_state ? w.in_state + (size_t)v * nstate : nullptr;
  const T* sq = row ? row + 1 : (const T*)s.qpos + (size_t)env * nq;
  const T* sv = row ? row + 1 + nq : (const T*)s.qvel + (size_t)env * nv;
  const T* sa = w.in_warm ? w.in_warm + (size_t)v * nv : (const T*)s.qacc_warmstart + (size_t)env * nv;
  const T* sf = (const T*)s.qfrc_applied + (size_t)env * nv;
  const T* sx = (const T*)s.xfrc_applied + (size_t)env * nx;
  // knot 0 of the rollout's schedule, or the env's ctrl held throughout
  const T* sc = w.in_ctrl ? w.in_ctrl + (size_t)(w.shared ? k : v) * w.nknot * nu : (const T*)s.ctrl + (size_t)env * nu;
  for (int i = l; i < nq; i += 64) w.qpos[(size_t)b * nq + i] = sq[i];
  for (int i = l; i < nv; i += 64) {
    w.qvel[(size_t)b * nv + i] = sv[i];
    w.qacc[(size_t)b * nv + i] = sa[i];
    w.qfrc[(size_t)b * nv + i] = sf[i];
  }
  for (int i = l; i < nu; i += 64) w.ctrl[(size_t)b * nu + i] = sc[i];
  for (int i = l; i < nx; i += 64) w.xfrc[(size_t)b * nx + i] = sx[i];
  if (l == 0) {
    w.time[b] = row ? row[0] : ((const T*)s.time)[env];
    w.warning[b] = 0;
    w.overflow[b] = 0;
  }
}

// ------------------------------------------------------------------ record
// After recorded step t. The live flag and the warning count are loaded by one lane and broadcast,
// so `live` and `diverged` are scalars and the branches on them are uniform. A rollout that is
// not live (deselected env, or diverged at an earlier step) has every output row already.
template <typename T>
__global__ void __launch_bounds__(64) k_rollout_record(RolloutBuf<T> w, int v0, int t) {
  const int b = blockIdx.x, l = threadIdx.x;
  int flags = 0;
  if (l == 0) flags = (w.live[b] ? 1 : 0) | (w.warning[b] != 0 ? 2 : 0);
  flags = __builtin_amdgcn_readfirstlane(flags);
  if (!(flags & 1)) return;
  const bool diverged = (flags & 2) != 0;
  const int v = v0 + b, nq = w.nq, nv = w.nv, nu = w.nu, nsd = w.nsd, Tn = w.T_steps;
  const int nstate = 1 + nq + nv;
  // rows t .. t_end - 1 take what this step left: one row, or the padding to the end
  const int t_end = diverged ? Tn : t + 1;
  if (w.out_state) {
    const T* q = w.qpos + (size_t)b * nq;
    const T* qv = w.qvel + (size_t)b * nv;
    const T tm = w.time[b];
    for (int i = l; i < nstate; i += 64) {
      const T x = i == 0 ? tm : (i <= nq ? q[i - 1] : qv[i - 1 - nq]);
      for (int r = t; r < t_end; r++) w.out_state[((size_t)v * Tn + r) * nstate + i] = x;
    }
  }
  if (w.out_sens && w.sens) {
    const T* sd = w.sens + (size_t)b * nsd;
    for (int i = l; i < nsd; i += 64) {
      const T x = sd[i];
      for (int r = t; r < t_end; r++) w.out_sens[((size_t)v * Tn + r) * nsd + i] = x;
    }
  }
  if (diverged) {
    // mgx_rollout_feedback: no control is computed after the diverging step, its rows are zero
    if (w.ctrl_out)
      for (size_t i = (size_t)(t + 1) * nu + l; i < (size_t)Tn * nu; i += 64) w.ctrl_out[(size_t)v * Tn * nu + i] = 0;
    if (w.warm_out)
      for (size_t i = (size_t)(t + 1) * nv + l; i < (size_t)Tn * nv; i += 64) w.warm_out[(size_t)v * Tn * nv + i] = 0;
    if (l == 0) {
      if (w.n_done) w.n_done[v] = t;
      w.live[b] = 0;
    }
    return;
  }
  if (t + 1 == Tn) {
    if (l == 0 && w.n_done) w.n_done[v] = Tn;
    return;
  }
  // zero-order hold: the next step changes ctrl only where a new knot begins
  if (w.in_ctrl && (t + 1) % w.hold == 0) {
    const int K = w.K, k = v % K;
    const T* sc = w.in_ctrl + ((size_t)(w.shared ? k : v) * w.nknot + (t + 1) / w.hold) * nu;
    for (int i = l; i < nu; i += 64) w.ctrl[(size_t)b * nu + i] = sc[i];
  }
}

// ------------------------------------------------------------------ feedback
// Before recorded step t (mgx_rollout_feedback): the control of slot b from its own state,
//   u_i = u_nom[e,t,i] + alpha[e,k] k_ff[e,t,i] + sum_j gain[e,t,i,j] dx_j,  dx = state (-) x_nom[e,t].
// One workgroup of 4 waves per live virtual env. dx (2 nv reals) is formed once in LDS, lane =
// tangent row; then wave w owns the actuators i = w, w + 4, ...: its lanes read row i of the gain
// along j (coalesced), multiply by dx from LDS and sum over the lanes with a butterfly of
// cross-lane moves, in an order fixed by the lane numbers: no atomics, bit-reproducible. The K
// rollouts of an env sit in adjacent workgroups and read the same gain[e,t] block, so after the
// first of them it comes from L2.
template <typename T>
__global__ void __launch_bounds__(256) k_rollout_feedback(DevModel<T> m, RolloutBuf<T> w, FeedbackBuf<T> f, int v0, int t) {
  extern __shared__ double fb_smem[];
  T* dxs = (T*)fb_smem;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!__builtin_amdgcn_readfirstlane((int)w.live[b])) return;  // one byte, the same for every wave
  const int v = v0 + b, env = v / w.K, nq = w.nq, nv = w.nv, nu = w.nu, nx2 = 2 * nv, Tn = w.T_steps;
  const size_t et = (size_t)env * Tn + t, vt = (size_t)v * Tn + t;
  if (f.gain) {
    const T* xn = f.x_nom + et * ((size_t)1 + nq + nv);
    const T* q = w.qpos + (size_t)b * nq;
    const T* qv = w.qvel + (size_t)b * nv;
    for (int r = tid; r < nx2; r += 256) dxs[r] = tangent_delta<true>(tangent_row(m, r), q, qv, xn + 1, xn + 1 + nq);
  }
  if (w.warm_out)
    for (int i = tid; i < nv; i += 256) w.warm_out[vt * nv + i] = w.qacc[(size_t)b * nv + i];
  __syncthreads();
  const T al = f.alpha ? f.alpha[v] : (T)1;
  for (int i = wave; i < nu; i += 4) {
    T acc = 0;
    if (f.gain) {
      const T* g = f.gain + (et * nu + i) * nx2;
      for (int j = lane; j < nx2; j += 64) acc += g[j] * dxs[j];
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    }
    if (lane == 0) {
      T u = f.u_nom[et * nu + i];
      if (f.k_ff) u += al * f.k_ff[et * nu + i];
      if (f.gain) u += acc;
      if (f.clamp && m.actuator_ctrllimited[i]) u = clampv(u, m.actuator_ctrlrange[2 * i], m.actuator_ctrlrange[2 * i + 1]);
      w.ctrl[(size_t)b * nu + i] = u;
      if (w.ctrl_out) w.ctrl_out[vt * nu + i] = u;
    }
  }
}

// ------------------------------------------------------------------ cost
// sum_{i < n} 1/2 w[i] d(i)^2 over the wave (mgx_rollout_cost, include/mgx.h): in double from the
// T-valued operands, every operation rounded once (no contraction into fused multiply-adds). Lane
// l sums its entries i = l, l + 64, ... in that order, then a butterfly of cross-lane moves in lane
// order: the order depends on n alone, there are no atomics, and every lane holds the sum.
template <typename T, typename F>
__device__ __forceinline__ double wave_half_wsq(const T* w, int n, int l, F d) {
#pragma clang fp contract(off)
  double acc = 0;
  for (int i = l; i < n; i += 64) {
    const double x = (double)d(i);
    acc = acc + (0.5 * (double)w[i]) * (x * x);
  }
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
  return acc;
}

// 1/2 wx . dx^2 of slot b's state against goal row `row` of its env, dx the entries of mgx_state_diff
template <typename T>
__device__ __forceinline__ double cost_state_part(const DevModel<T>& m, const RolloutBuf<T>& w, const CostBuf<T>& c, int b,
                                                  int env, int row, const T* wx, int l) {
  if (!c.goal || !wx) return 0;
  const int nq = w.nq, nv = w.nv;
  const T* g = c.goal + ((size_t)env * c.goal_rows + (c.goal_rows == 1 ? 0 : row)) * ((size_t)1 + nq + nv);
  const T* q = w.qpos + (size_t)b * nq;
  const T* qv = w.qvel + (size_t)b * nv;
  return wave_half_wsq(wx + (size_t)env * 2 * nv, 2 * nv, l,
                       [&](int r) { return tangent_delta<true>(tangent_row(m, r), q, qv, g + 1, g + 1 + nq); });
}

// After k_rollout_begin: the x_0 term. One wave per virtual env; lane 0 is the single writer of
// cost[v] and terms[v] for the whole call, and here it overwrites whatever they held.
template <typename T>
__global__ void __launch_bounds__(64) k_rollout_cost_begin(DevModel<T> m, RolloutBuf<T> w, CostBuf<T> c, int v0) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (!__builtin_amdgcn_readfirstlane((int)w.live[b])) return;  // one byte, the same for every lane
  const int v = v0 + b, env = v / w.K;
  const double sx = cost_state_part(m, w, c, b, env, 0, c.w_x, l);
  if (l == 0) {
    c.cost[v] = sx;
    if (c.terms) { c.terms[(size_t)v * 3] = sx; c.terms[(size_t)v * 3 + 1] = 0; c.terms[(size_t)v * 3 + 2] = 0; }
  }
}

// After recorded step t and its sensor kernels, before k_rollout_record (which loads the next ctrl
// and clears the live flag of a rollout that diverged): the terms of u_t, x_(t+1) and s(x_(t+1)),
// read from the workspace. The live flag and the warning count are broadcast as record does it, so
// the branches are uniform. The K rollouts of an env read the same goal rows and weights: after
// the first of them they come from L2. A rollout that diverged at this step costs +inf and, no
// longer live after record, is not visited again.
template <typename T>
__global__ void __launch_bounds__(64) k_rollout_cost(DevModel<T> m, RolloutBuf<T> w, CostBuf<T> c, int v0, int t) {
  const int b = blockIdx.x, l = threadIdx.x;
  int flags = 0;
  if (l == 0) flags = (w.live[b] ? 1 : 0) | (w.warning[b] != 0 ? 2 : 0);
  flags = __builtin_amdgcn_readfirstlane(flags);
  if (!(flags & 1)) return;
  const int v = v0 + b, env = v / w.K, nu = w.nu, nsd = w.nsd;
  if (flags & 2) {
    if (l == 0) {
      const double inf = __builtin_huge_val();
      c.cost[v] = inf;
      if (c.terms) { c.terms[(size_t)v * 3] = inf; c.terms[(size_t)v * 3 + 1] = inf; c.terms[(size_t)v * 3 + 2] = inf; }
    }
    return;
  }
  const bool last = t + 1 == w.T_steps;
  const double sx = cost_state_part(m, w, c, b, env, t + 1, last ? c.w_xf : c.w_x, l);
  double su = 0, ss = 0;
  if (c.w_u) {
    const T* u = w.ctrl + (size_t)b * nu;  // still the control handed to step t
    su = wave_half_wsq(c.w_u + (size_t)env * nu, nu, l, [&](int i) { return u[i]; });
  }
  const T* ws = last ? c.w_sf : c.w_s;
  if (c.sgoal && ws && w.sens) {
    const T* sd = w.sens + (size_t)b * nsd;
    const T* sg = c.sgoal + ((size_t)env * c.sensor_rows + (c.sensor_rows == 1 ? 0 : t)) * nsd;
    ss = wave_half_wsq(ws + (size_t)env * nsd, nsd, l, [&](int i) { return (T)(sd[i] - sg[i]); });
  }
  if (l == 0) {
    c.cost[v] = c.cost[v] + ((sx + su) + ss);
    if (c.terms) {
      double* tr = c.terms + (size_t)v * 3;
      tr[0] = tr[0] + sx; tr[1] = tr[1] + su; tr[2] = tr[2] + ss;
    }
  }
}

int rollout_dims(const mgx_model* m, RolloutDims* d) {
  mgx_model_info info;
  const int rc = mgx_model_get_info(m, &info);
  if (rc) return rc;
  *d = RolloutDims{info.nq, info.nv, info.nu, info.nbody, m->precision == MGX_F32 ? 4 : 8, info.max_ncon,
                   m->sensor && !m->sensor->unsupported ? m->sensor->nsensordata : 0,
                   (size_t)info.scratch_bytes_per_env};
  return MGX_OK;
}

template <typename T>
int run_rollout(const mgx_model* m, const DevModel<T>& M, const RolloutDims& d, const mgx_state* s, const mgx_rollout_io* io,
                const mgx_feedback_io* fio, const mgx_cost_io* cio, bool sensors, int n_env, const uint8_t* mask,
                hipStream_t st) {
  const RolloutLayout o = rollout_layout(d, io->slots, sensors);
  char* ws = (char*)io->workspace;
  const int Tn = io->n_step, K = io->n_roll;
  RolloutBuf<T> w{};
  w.qpos = (T*)(ws + o.qpos); w.qvel = (T*)(ws + o.qvel); w.qacc = (T*)(ws + o.qacc); w.ctrl = (T*)(ws + o.ctrl);
  w.qfrc = (T*)(ws + o.qfrc); w.xfrc = (T*)(ws + o.xfrc); w.time = (T*)(ws + o.time);
  w.warning = (int32_t*)(ws + o.warning); w.overflow = (int32_t*)(ws + o.overflow); w.live = (uint8_t*)(ws + o.live);
  w.sens = sensors ? (const T*)(ws + o.sens) : nullptr;
  w.in_state = (const T*)io->initial_state; w.in_warm = (const T*)io->initial_warmstart; w.in_ctrl = (const T*)io->ctrl;
  w.out_state = (T*)io->state; w.out_sens = sensors ? (T*)io->sensordata : nullptr; w.n_done = io->n_done;
  w.nq = d.nq; w.nv = d.nv; w.nu = d.nu; w.nx = 6 * d.nbody; w.nsd = d.nsd;
  w.K = K; w.T_steps = Tn; w.hold = io->hold; w.nknot = (Tn + io->hold - 1) / io->hold;
  w.shared = io->flags & MGX_ROLLOUT_SHARED_CTRL ? 1 : 0;
  FeedbackBuf<T> f{};
  if (fio) {
    w.ctrl_out = (T*)fio->ctrl_out; w.warm_out = (T*)fio->warm_out;
    f.u_nom = (const T*)fio->u_nom; f.x_nom = (const T*)fio->x_nom; f.k_ff = (const T*)fio->k_ff;
    f.alpha = (const T*)fio->alpha; f.gain = (const T*)fio->gain; f.clamp = fio->flags & MGX_FEEDBACK_CLAMP ? 1 : 0;
  }
  CostBuf<T> c{};
  if (cio) {
    c.goal = (const T*)cio->goal; c.w_x = (const T*)cio->w_x; c.w_xf = (const T*)cio->w_xf; c.w_u = (const T*)cio->w_u;
    c.sgoal = (const T*)cio->sensor_goal; c.w_s = (const T*)cio->w_s; c.w_sf = (const T*)cio->w_sf;
    c.goal_rows = cio->goal_rows; c.sensor_rows = cio->sensor_rows;
    c.cost = (double*)cio->cost; c.terms = (double*)cio->terms;
  }
  const size_t fb_lds = (size_t)(2 * d.nv > 0 ? 2 * d.nv : 1) * sizeof(double);
  mgx_state vs{};
  vs.qpos = w.qpos; vs.qvel = w.qvel; vs.qacc_warmstart = w.qacc; vs.ctrl = w.ctrl; vs.qfrc_applied = w.qfrc;
  vs.xfrc_applied = w.xfrc; vs.time = w.time; vs.warning = w.warning; vs.overflow = w.overflow;
  vs.scratch = d.scratch ? ws + o.scratch : nullptr;
  mgx_forward_out fo{};
  if (sensors) {
    fo.qacc = ws + o.f_qacc; fo.qfrc_constraint = ws + o.f_qfrc; fo.ncon = (int32_t*)(ws + o.f_ncon);
    fo.con_geom = (int32_t*)(ws + o.f_geom); fo.con_dist = ws + o.f_dist; fo.con_pos = ws + o.f_pos;
    fo.con_frame = ws + o.f_frame; fo.con_force = ws + o.f_force;
  }
  const bool need_fwd = sensors && m->sensor->need_acc;
  const int64_t total = (int64_t)n_env * K;
  for (int64_t v0 = 0; v0 < total; v0 += io->slots) {
    const int cnt = (int)(total - v0 < io->slots ? total - v0 : io->slots);
    hipLaunchKernelGGL(k_rollout_begin<T>, dim3(cnt), dim3(64), 0, st, *s, w, (int)v0, mask);
    MGX_HIPCHK(hipGetLastError());
    if (cio) {
      hipLaunchKernelGGL(k_rollout_cost_begin<T>, dim3(cnt), dim3(64), 0, st, M, w, c, (int)v0);
      MGX_HIPCHK(hipGetLastError());
    }
    for (int t = 0; t < Tn; t++) {
      // the library's own step, exactly as a caller of mgx_step gets it; rollouts of deselected
      // envs hold no state, and diverged ones are done: both are masked out by the live flags
      if (fio) {
        // the control of this step from the state entering it; the open-loop path launches nothing here
        hipLaunchKernelGGL(k_rollout_feedback<T>, dim3(cnt), dim3(256), fb_lds, st, M, w, f, (int)v0, t);
        MGX_HIPCHK(hipGetLastError());
      }
      int rc = mgx_step(m, &vs, nullptr, cnt, io->nsub, w.live, st);
      if (rc) return rc;
      if (sensors) {
        if (need_fwd) {
          rc = mgx_forward(m, &vs, &fo, cnt, w.live, st);
          if (rc) return rc;
        }
        rc = mgx_sensor(m, &vs, need_fwd ? &fo : nullptr, ws + o.sens, cnt, w.live, st);
        if (rc) return rc;
      }
      if (cio) {
        // u_t, x_(t+1) and its sensors are in the workspace now; record overwrites ctrl and live
        hipLaunchKernelGGL(k_rollout_cost<T>, dim3(cnt), dim3(64), 0, st, M, w, c, (int)v0, t);
        MGX_HIPCHK(hipGetLastError());
      }
      hipLaunchKernelGGL(k_rollout_record<T>, dim3(cnt), dim3(64), 0, st, w, (int)v0, t);
      MGX_HIPCHK(hipGetLastError());
    }
  }
  return MGX_OK;
}

}  // namespace

extern "C" {

int64_t mgx_rollout_bytes(const mgx_model* m, int slots, int with_sensors) {
  if (!m || slots < 1) return host_fail(MGX_E_ARG, "null model or slots < 1");
  RolloutDims d;
  const int rc = rollout_dims(m, &d);
  if (rc) return rc;
  return (int64_t)rollout_layout(d, slots, with_sensors != 0).bytes;
}

}  // extern "C"

namespace {

// mgx_rollout, mgx_rollout_feedback with its checked mgx_feedback_io, and mgx_rollout_cost with its
// checked mgx_cost_io on top of either
int rollout_call(const mgx_model* m, const mgx_state* s, const mgx_rollout_io* io, const mgx_feedback_io* fio,
                 const mgx_cost_io* cio, int n_env, const uint8_t* env_mask, void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (io->flags & ~MGX_ROLLOUT_SHARED_CTRL) return host_fail(MGX_E_ARG, "unknown mgx_rollout_io.flags bits");
  if (io->n_roll < 1 || io->n_step < 1) return host_fail(MGX_E_ARG, "n_roll and n_step must be >= 1");
  if (io->nsub < 1 || io->hold < 1) return host_fail(MGX_E_ARG, "nsub and hold must be >= 1");
  if (io->slots < 1) return host_fail(MGX_E_ARG, "slots must be >= 1");
  if ((int64_t)n_env * io->n_roll > INT32_MAX) return host_fail(MGX_E_ARG, "n_env * n_roll exceeds 2^31 - 1");
  bool sensors = false;
  const bool want_sensors = io->sensordata || (cio && cio->sensor_goal);  // a sensor term needs the staging rows
  if (want_sensors) {
    // what mgx_forward and mgx_sensor would refuse, before anything is launched
    if (m->wide) return host_fail(MGX_E_UNSUPPORTED, std::string("mgx_forward: ") + MGX_WIDE_MSG);
    if ((m->precision == MGX_F32 ? m->mf.cone : m->md.cone) != 0)
      return host_fail(MGX_E_UNSUPPORTED, "mgx_forward decodes pyramidal cones only");
    if (!m->sensor) return host_fail(MGX_E_ARG, "mgx_sensor_configure has not been called for this model");
    if (m->sensor->unsupported) return host_fail(MGX_E_UNSUPPORTED, m->sensor->why);
    sensors = m->sensor->nsensordata > 0;
  }
  RolloutDims d;
  rc = rollout_dims(m, &d);
  if (rc) return rc;
  if (!io->workspace || io->workspace_bytes < rollout_layout(d, io->slots, want_sensors).bytes)
    return host_fail(MGX_E_ARG, "workspace smaller than mgx_rollout_bytes");
  const bool records = fio && (fio->ctrl_out || fio->warm_out);
  if (n_env == 0 || (!io->state && !(sensors && io->sensordata) && !io->n_done && !records && !cio)) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return run_rollout<float>(m, m->mf, d, s, io, fio, cio, sensors, n_env, env_mask, st);
  return run_rollout<double>(m, m->md, d, s, io, fio, cio, sensors, n_env, env_mask, st);
}

}  // namespace

extern "C" {

int mgx_rollout(const mgx_model* m, const mgx_state* s, const mgx_rollout_io* io, int n_env, const uint8_t* env_mask,
                void* stream) {
  return rollout_call(m, s, io, nullptr, nullptr, n_env, env_mask, stream);
}

}  // extern "C"

namespace {

// The checks that concern the feedback law read io and fb only and come first, so a caller's
// mistake in them is named whatever the model and the state are.
int feedback_check(const mgx_rollout_io* io, const mgx_feedback_io* fb) {
  if (!io) return host_fail(MGX_E_ARG, "null mgx_rollout_io");
  if (!fb || !fb->u_nom) return host_fail(MGX_E_ARG, "mgx_rollout_feedback needs an mgx_feedback_io with u_nom");
  if (io->hold != 1) return host_fail(MGX_E_ARG, "mgx_rollout_feedback: hold must be 1");
  if (io->ctrl || (io->flags & MGX_ROLLOUT_SHARED_CTRL))
    return host_fail(MGX_E_ARG, "mgx_rollout_feedback: io->ctrl must be NULL and MGX_ROLLOUT_SHARED_CTRL unset (the nominal control is fb->u_nom)");
  if (fb->gain && !fb->x_nom) return host_fail(MGX_E_ARG, "mgx_feedback_io.gain needs x_nom");
  if (fb->flags & ~MGX_FEEDBACK_CLAMP) return host_fail(MGX_E_ARG, "unknown mgx_feedback_io.flags bits");
  return MGX_OK;
}

}  // namespace

extern "C" {

int mgx_rollout_feedback(const mgx_model* m, const mgx_state* s, const mgx_rollout_io* io, const mgx_feedback_io* fb,
                         int n_env, const uint8_t* env_mask, void* stream) {
  const int rc = feedback_check(io, fb);
  if (rc) return rc;
  return rollout_call(m, s, io, fb, nullptr, n_env, env_mask, stream);
}

// The checks of the cost read io and cost only and come first, then those of the feedback law.
int mgx_rollout_cost(const mgx_model* m, const mgx_state* s, const mgx_rollout_io* io, const mgx_feedback_io* fb,
                     const mgx_cost_io* cost, int n_env, const uint8_t* env_mask, void* stream) {
  if (!io) return host_fail(MGX_E_ARG, "null mgx_rollout_io");
  if (!cost || !cost->cost) return host_fail(MGX_E_ARG, "mgx_rollout_cost needs an mgx_cost_io with cost");
  if (cost->goal && cost->goal_rows != 1 && cost->goal_rows != (int64_t)io->n_step + 1)
    return host_fail(MGX_E_ARG, "mgx_cost_io.goal_rows must be 1 or n_step + 1");
  if (cost->sensor_goal && cost->sensor_rows != 1 && cost->sensor_rows != io->n_step)
    return host_fail(MGX_E_ARG, "mgx_cost_io.sensor_rows must be 1 or n_step");
  if ((cost->w_s || cost->w_sf) && !cost->sensor_goal) return host_fail(MGX_E_ARG, "mgx_cost_io.w_s / w_sf need sensor_goal");
  if ((cost->w_x || cost->w_xf) && !cost->goal) return host_fail(MGX_E_ARG, "mgx_cost_io.w_x / w_xf need goal");
  if (cost->flags) return host_fail(MGX_E_ARG, "unknown mgx_cost_io.flags bits");
  if (fb) {
    const int rc = feedback_check(io, fb);
    if (rc) return rc;
  }
  return rollout_call(m, s, io, fb, cost, n_env, env_mask, stream);
}

}  // extern "C"
