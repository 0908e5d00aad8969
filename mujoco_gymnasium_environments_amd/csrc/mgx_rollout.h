// mgx_rollout.h — workspace layout of mgx_rollout (include/mgx.h "open-loop rollouts";
// DESIGN.md §11).
#pragma once
#include "../../include/mgx.h"
#include "mgx_common.h"

namespace mgx {

// The workspace: `slots` virtual envs, each a complete mgx_state (env-major arrays, as mgx_step
// reads them), per virtual env the live flag (the env mask of every step / forward / sensor launch
// of the pass) and, where the model needs it, the solver scratch; with sensors also the buffers of
// an mgx_forward_out and one sensordata staging row per virtual env. Byte offsets, each a multiple
// of 256.
struct RolloutLayout {
  size_t qpos, qvel, qacc, ctrl, qfrc, xfrc, time, warning, overflow, live, scratch;
  size_t f_qacc, f_qfrc, f_ncon, f_geom, f_dist, f_pos, f_frame, f_force, sens;  // with sensors only
  size_t bytes;
};

struct RolloutDims {
  int nq, nv, nu, nbody, real_bytes, max_ncon, nsd;
  size_t scratch;  // solver scratch bytes per env
};

inline RolloutLayout rollout_layout(const RolloutDims& d, int slots, bool with_sensors) {
  RolloutLayout o{};
  size_t p = 0;
  const size_t V = (size_t)slots, rb = (size_t)d.real_bytes, C = (size_t)d.max_ncon;
  auto take = [&](size_t n) { size_t r = p; p += (n + 255) / 256 * 256; return r; };
  o.qpos = take(V * d.nq * rb); o.qvel = take(V * d.nv * rb); o.qacc = take(V * d.nv * rb);
  o.ctrl = take(V * (d.nu > 0 ? d.nu : 1) * rb); o.qfrc = take(V * d.nv * rb); o.xfrc = take(V * 6 * d.nbody * rb);
  o.time = take(V * rb); o.warning = take(V * 4); o.overflow = take(V * 4); o.live = take(V);
  o.scratch = take(V * d.scratch);
  if (with_sensors) {
    o.f_qacc = take(V * d.nv * rb); o.f_qfrc = take(V * d.nv * rb); o.f_ncon = take(V * 4);
    o.f_geom = take(V * C * 2 * 4); o.f_dist = take(V * C * rb); o.f_pos = take(V * C * 3 * rb);
    o.f_frame = take(V * C * 9 * rb); o.f_force = take(V * C * 6 * rb); o.sens = take(V * d.nsd * rb);
  }
  o.bytes = p;
  return o;
}

// Caller buffers, workspace arrays and sizes of one call, typed.
template <typename T>
struct RolloutBuf {
  T *qpos, *qvel, *qacc, *ctrl, *qfrc, *xfrc, *time;  // the virtual envs of the pass (slot-major)
  int32_t *warning, *overflow;
  uint8_t *live;
  const T* sens;  // staging rows [slots][nsd]; NULL: no sensors recorded
  const T *in_state, *in_warm, *in_ctrl;  // inputs (mgx_rollout_io), indexed by v
  T *out_state, *out_sens;                // outputs, indexed by v
  int32_t* n_done;
  int nq, nv, nu, nx, nsd;  // nx = 6 nbody
  int K, T_steps, hold, nknot, shared;
  T *ctrl_out, *warm_out;  // mgx_rollout_feedback's records [v][T][nu], [v][T][nv]; NULL in mgx_rollout
};

// The control law of mgx_rollout_feedback (mgx_feedback_io), typed; indexed by env e, rollout k, step t.
template <typename T>
struct FeedbackBuf {
  const T *u_nom, *x_nom, *k_ff, *alpha, *gain;  // [e][t][nu], [e][t][nstate], [e][t][nu], [e][k], [e][t][nu][2nv]
  int clamp;
};

// The cost of mgx_rollout_cost (mgx_cost_io), typed; goals and weights indexed by env e, the two
// outputs by v. A NULL goal / sgoal drops the term, a NULL weight is zeros.
template <typename T>
struct CostBuf {
  const T *goal, *w_x, *w_xf, *w_u;  // [e][goal_rows][nstate], [e][2nv], [e][2nv], [e][nu]
  const T *sgoal, *w_s, *w_sf;       // [e][sensor_rows][nsd], [e][nsd], [e][nsd]
  int goal_rows, sensor_rows;
  double *cost, *terms;  // [v], [v][3] (nullable)
};

}  // namespace mgx
