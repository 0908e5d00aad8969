// mgx_manifold.hip — the two operations of the state manifold and their C-ABI: mgx_state_diff
// (MuJoCo's mj_differentiatePos [ext] on state rows) and mgx_state_integrate (mj_integratePos [ext])
// (include/mgx.h).
//
// Both are thin: one state row [time, qpos, qvel] per wave, four rows per workgroup, the lanes over
// the tangent rows (diff) or over the joints and dofs (integrate), so a row is read along its
// contiguous index. No LDS, no atomics.
#include "mgx_internal.h"
#include "mgx_manifold.h"
#include "mgx_physics.h"

using namespace mgx;

namespace {

constexpr int ROWS_PER_BLOCK = 4;

// dx[row] = (mj_differentiatePos(qpos_a from qpos_b), qvel_a - qvel_b); xb has one row or n_rows
template <typename T>
__global__ void __launch_bounds__(64 * ROWS_PER_BLOCK) k_state_diff(DevModel<T> m, const T* xa, const T* xb, T* dx,
                                                                    int64_t n_rows, int64_t xb_rows) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int nq = m.nq, nv = m.nv;
  const size_t nstate = (size_t)1 + nq + nv;
  const T* a = xa + (size_t)row * nstate;
  const T* b = xb + (xb_rows == 1 ? (size_t)0 : (size_t)row * nstate);
  T* d = dx + (size_t)row * 2 * nv;
  for (int r = l; r < 2 * nv; r += 64) d[r] = tangent_delta<true>(tangent_row(m, r), a + 1, a + 1 + nq, b + 1, b + 1 + nq);
}

// out[row] = (time, mj_integratePos(qpos, dx[:nv], 1), qvel + dx[nv:]). A lane reads only the
// entries it writes, so out may alias x.
template <typename T>
__global__ void __launch_bounds__(64 * ROWS_PER_BLOCK) k_state_integrate(DevModel<T> m, const T* x, const T* dx, T* out,
                                                                         int64_t n_rows) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int nq = m.nq, nv = m.nv;
  const size_t nstate = (size_t)1 + nq + nv;
  const T* s = x + (size_t)row * nstate;
  const T* d = dx + (size_t)row * 2 * nv;
  T* o = out + (size_t)row * nstate;
  if (l == 0) o[0] = s[0];
  // the joint loop of integrate_pos (mgx_physics.h) with h = 1, from one array into another
  for (int j = l; j < m.njnt; j += 64) {
    const int a = m.jnt_qposadr[j], da = m.jnt_dofadr[j], t = m.jnt_type[j];
    if (t == JFREE || t == JBALL) {
      int qa = a;
      const T* w = d + da;
      if (t == JFREE) {
        for (int k = 0; k < 3; k++) o[1 + a + k] = s[1 + a + k] + d[da + k];
        qa = a + 3;
        w = d + da + 3;
      }
      T q[4] = {s[1 + qa], s[1 + qa + 1], s[1 + qa + 2], s[1 + qa + 3]};
      quat_integrate(q, w, (T)1);
      for (int k = 0; k < 4; k++) o[1 + qa + k] = q[k];
    } else {
      o[1 + a] = s[1 + a] + d[da];
    }
  }
  for (int k = l; k < nv; k += 64) o[1 + nq + k] = s[1 + nq + k] + d[nv + k];
}

}  // namespace

extern "C" {

int mgx_state_diff(const mgx_model* m, const void* xa, const void* xb, void* dx, int64_t n_rows, int64_t xb_rows,
                   void* stream) {
  if (!m || n_rows < 0) return host_fail(MGX_E_ARG, "null model or n_rows < 0");
  if (n_rows == 0) return MGX_OK;
  if (!xa || !xb || !dx) return host_fail(MGX_E_ARG, "null xa, xb or dx");
  if (xb_rows != 1 && xb_rows != n_rows) return host_fail(MGX_E_ARG, "xb_rows must be 1 or n_rows");
  const int64_t blocks = (n_rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > INT32_MAX) return host_fail(MGX_E_ARG, "n_rows exceeds 2^33 - 4");
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32)
    hipLaunchKernelGGL(k_state_diff<float>, dim3((unsigned)blocks), dim3(64 * ROWS_PER_BLOCK), 0, st, m->mf,
                       (const float*)xa, (const float*)xb, (float*)dx, n_rows, xb_rows);
  else
    hipLaunchKernelGGL(k_state_diff<double>, dim3((unsigned)blocks), dim3(64 * ROWS_PER_BLOCK), 0, st, m->md,
                       (const double*)xa, (const double*)xb, (double*)dx, n_rows, xb_rows);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

int mgx_state_integrate(const mgx_model* m, const void* x, const void* dx, void* out, int64_t n_rows, void* stream) {
  if (!m || n_rows < 0) return host_fail(MGX_E_ARG, "null model or n_rows < 0");
  if (n_rows == 0) return MGX_OK;
  if (!x || !dx || !out) return host_fail(MGX_E_ARG, "null x, dx or out");
  const int64_t blocks = (n_rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > INT32_MAX) return host_fail(MGX_E_ARG, "n_rows exceeds 2^33 - 4");
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32)
    hipLaunchKernelGGL(k_state_integrate<float>, dim3((unsigned)blocks), dim3(64 * ROWS_PER_BLOCK), 0, st, m->mf,
                       (const float*)x, (const float*)dx, (float*)out, n_rows);
  else
    hipLaunchKernelGGL(k_state_integrate<double>, dim3((unsigned)blocks), dim3(64 * ROWS_PER_BLOCK), 0, st, m->md,
                       (const double*)x, (const double*)dx, (double*)out, n_rows);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

}  // extern "C"
