// mgx_fd.h — workspace layout of mgx_transition_fd (include/mgx.h "finite-difference transition
// derivatives").
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

}  // namespace mgx
