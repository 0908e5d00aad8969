// mgx_fd.h — workspace layouts of mgx_transition_fd (include/mgx.h "finite-difference transition
// derivatives") and mgx_sensor_fd ("finite-difference sensor derivatives"; §15).
#pragma once
#include "../../include/mgx.h"
#include "mgx_common.h"

namespace mgx {

#define MGX_FD_TILE 64  // k_fd_diff transposes MGX_FD_TILE columns x MGX_FD_TILE rows through LDS

// The workspace: `slots` virtual envs, each a complete mgx_state (env-major arrays, as mgx_step
// reads them), then per virtual env the signed step its perturbation took (0: none taken), the
// env mask of the step launch and, where the model needs it, the solver scratch. Byte offsets,
// each a multiple of 256.
struct FdLayout {
  size_t qpos, qvel, qacc, ctrl, qfrc, xfrc, time, warning, overflow, step, vmask, scratch, bytes;
};

inline FdLayout fd_layout(int nq, int nv, int nu, int nbody, int real_bytes, size_t scratch_bytes_per_env, int slots) {
  FdLayout o;
  size_t p = 0;
  const size_t V = (size_t)slots, rb = (size_t)real_bytes;
  auto take = [&](size_t n) { size_t r = p; p += (n + 255) / 256 * 256; return r; };
  o.qpos = take(V * nq * rb); o.qvel = take(V * nv * rb); o.qacc = take(V * nv * rb);
  o.ctrl = take(V * (nu > 0 ? nu : 1) * rb); o.qfrc = take(V * nv * rb); o.xfrc = take(V * 6 * nbody * rb);
  o.time = take(V * rb); o.warning = take(V * 4); o.overflow = take(V * 4); o.step = take(V * rb);
  o.vmask = take(V); o.scratch = take(V * scratch_bytes_per_env);
  o.bytes = p;
  return o;
}

// Caller buffers and workspace arrays of one pass, typed.
template <typename T>
struct FdBuf {
  T *qpos, *qvel, *qacc, *ctrl, *qfrc, *xfrc, *time, *step;  // the virtual envs
  int32_t *warning, *overflow;
  uint8_t *vmask;
  T *A, *B, *next_qpos, *next_qvel;  // outputs (mgx_fd_io)
  int32_t *out_warning;
};

// The workspace of mgx_sensor_fd: mgx_transition_fd's for `slots` virtual envs, then
// per virtual env the buffers of an mgx_forward_out (as mgx_rollout's sensor workspace holds them)
// and one sensordata staging row. Byte offsets, each a multiple of 256.
struct SensFdLayout {
  FdLayout fd;
  size_t f_qacc, f_qfrc, f_ncon, f_geom, f_dist, f_pos, f_frame, f_force, sens, bytes;
};

inline SensFdLayout sens_fd_layout(int nq, int nv, int nu, int nbody, int real_bytes, size_t scratch_bytes_per_env,
                                   int max_ncon, int nsd, int slots) {
  SensFdLayout o;
  o.fd = fd_layout(nq, nv, nu, nbody, real_bytes, scratch_bytes_per_env, slots);
  size_t p = o.fd.bytes;
  const size_t V = (size_t)slots, rb = (size_t)real_bytes, C = (size_t)max_ncon;
  auto take = [&](size_t n) { size_t r = p; p += (n + 255) / 256 * 256; return r; };
  o.f_qacc = take(V * nv * rb); o.f_qfrc = take(V * nv * rb); o.f_ncon = take(V * 4);
  o.f_geom = take(V * C * 2 * 4); o.f_dist = take(V * C * rb); o.f_pos = take(V * C * 3 * rb);
  o.f_frame = take(V * C * 9 * rb); o.f_force = take(V * C * 6 * rb); o.sens = take(V * nsd * rb);
  o.bytes = p;
  return o;
}

// Staging rows, steps and outputs of one k_sens_diff launch, typed.
template <typename T>
struct SensFdBuf {
  const T *sens, *step;     // [slots][ns], [slots] (the signed step each virtual env took; 0: none)
  T *C, *D, *sensordata;    // outputs (mgx_sensor_fd_io)
  int ns, nv, nu;
};

}  // namespace mgx
