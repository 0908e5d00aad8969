// mgx_ik.hip — batched inverse kinematics by damped least squares (include/mgx.h "inverse
// kinematics").
//
// One kernel, one wave per env, the whole iteration loop in one launch over the slim Env binding of
// k_jac: kinematics / com_crb / integrate_pos of mgx_physics.h unchanged, the points and Jacobian
// columns of mgx_dyn.h, and per iteration, all in LDS:
//   e, r      one lane per target; r summed by every lane from the LDS copy in row order (uniform)
//   J         lane = dof (strided by 64), rows coalesced along nv
//   A         lane = element of the packed lower triangle, a dot over nv in dof order
//   Cholesky  column by column, lane = row (m <= 48 fits the wave); the pivot by readlane
//   solves    lane = row, y in a register, the solved entry broadcast by readlane
//   delta     lane = dof, summed in row order; max |delta| by a wave reduction
// Every sum runs in a fixed order, so results are bit-reproducible and independent of the batch
// size; no atomics. Every stop decision is wave-uniform (a readfirstlane / readlane value).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "mgx_internal.h"
#include "mgx_physics.h"
#include "mgx_ik.h"

using namespace mgx;

#define MGX_IK_LDS_LIMIT (160 * 1024)
#define MGX_IK_MAX_ROW (6 * MGX_IK_MAX_POINT)
static_assert(MGX_IK_MAX_ROW <= 64, "one lane per row of A");

namespace {

// limited hinge and slide coordinates whose dof may move, clamped to jnt_range
template <typename T>
__device__ __forceinline__ void ik_clamp(const DevModel<T>& m, T* qpos, const uint8_t* dmask) {
  for (int j = lane_id(); j < m.njnt; j += 64) {
    const int t = m.jnt_type[j];
    if (!m.jnt_limited[j] || (t != JHINGE && t != JSLIDE)) continue;
    if (dmask && !dmask[m.jnt_dofadr[j]]) continue;
    const int a = m.jnt_qposadr[j];
    qpos[a] = clampv(qpos[a], m.jnt_range[2 * j], m.jnt_range[2 * j + 1]);
  }
  wsync();
}

// the world-frame rotation vector of qt o conj(qc): angle 2 atan2(|v|, w) wrapped to (-pi, pi]
template <typename T>
__device__ __forceinline__ void ik_rotvec(T* rv, const T* qt, const T* qc) {
  const T cc[4] = {qc[0], -qc[1], -qc[2], -qc[3]};
  T d[4];
  mulquat(d, qt, cc);
  const T n = sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  rv[0] = rv[1] = rv[2] = 0;
  if (n == 0) return;
  T ang = (T)2 * atan2(n, d[0]);
  if (ang > (T)3.14159265358979323846) ang -= (T)6.28318530717958647692;
  for (int c = 0; c < 3; c++) rv[c] = d[1 + c] / n * ang;
}

template <typename T>
__global__ void __launch_bounds__(64) k_ik(DevModel<T> m, const T* gqpos, IkArgs<T> a, const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the rows stay untouched
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* R = reinterpret_cast<T*>(smem);
  const int nq = m.nq, nv = m.nv, l = lane_id(), P = a.P, M = a.m;
  Env<T> e;
  int o = dyn_bind(m, e, R, false);
  auto take = [&](int n) { T* r = R + o; o += n; return r; };
  T* qprev = take(nq);
  T* J = take(M * nv);
  T* ev = take(M);
  T* A = take(M * (M + 1) / 2);
  T* y = take(M);
  T* delta = take(nv);
  T* pt = take(4 * P);     // the world point, 1 / subtree mass
  T* tpos = take(3 * P);
  T* tquat = take(4 * P);
  T* qoff = take(4 * P);
  T* wt = take(4 * P);     // pos weight, rot weight, first position row, first orientation row

  const T* q0 = (a.qpos_init ? a.qpos_init : gqpos) + (size_t)env * nq;
  for (int k = l; k < nq; k += 64) e.qpos[k] = q0[k];
#pragma unroll
  for (int p = 0; p < MGX_IK_MAX_POINT; p++)
    if (l == p && p < P) {
      wt[4 * p] = a.pos_weight[p]; wt[4 * p + 1] = a.rot_weight[p];
      wt[4 * p + 2] = (T)a.row_pos[p]; wt[4 * p + 3] = (T)a.row_rot[p];
    }
  if (l < P) {
    const size_t at = (size_t)env * P + l;
    for (int c = 0; c < 3; c++) tpos[3 * l + c] = a.target_pos[at * 3 + c];
    T tq[4] = {1, 0, 0, 0}, qo[4] = {1, 0, 0, 0};
    if (a.target_quat) {
      for (int c = 0; c < 4; c++) tq[c] = a.target_quat[at * 4 + c];
      normalize4(tq);
    }
    if (a.quat)
      for (int c = 0; c < 4; c++) qo[c] = a.quat[4 * l + c];
    for (int c = 0; c < 4; c++) { tquat[4 * l + c] = tq[c]; qoff[4 * l + c] = qo[c]; }
  }
  wsync();
  if (a.clamp) ik_clamp(m, e.qpos, a.dof_mask);

  int it = 0, status = MGX_IK_FAILED;
  T r = 0;
  for (;;) {
    kinematics(m, e);  // m.L.late_geom == 1 (set by the launcher): no geom poses
    com_crb(m, e);
    if (l < P) {
      const int b = a.body[l], k = a.kind[l];
      T lp[3] = {0, 0, 0}, x[3], w;
      if (a.pos)
        for (int c = 0; c < 3; c++) lp[c] = a.pos[3 * l + c];
      jac_point(m, e, b, k, lp, x, w);
      for (int c = 0; c < 3; c++) pt[4 * l + c] = x[c];
      pt[4 * l + 3] = w;
      const int rp = (int)wt[4 * l + 2], rr = (int)wt[4 * l + 3];
      if (rp >= 0)
        for (int c = 0; c < 3; c++) ev[rp + c] = wt[4 * l] * (tpos[3 * l + c] - x[c]);
      if (rr >= 0) {
        T rv[3] = {0, 0, 0};
        if ((unsigned)b < (unsigned)m.nbody) {
          T cur[4];
          mulquat(cur, e.xquat + 4 * b, qoff + 4 * l);
          ik_rotvec(rv, tquat + 4 * l, cur);
        }
        for (int c = 0; c < 3; c++) ev[rr + c] = wt[4 * l + 1] * rv[c];
      }
    }
    wsync();
    // r: the same sum on every lane; the decision is taken from lane 0's copy
    T ss = 0;
    for (int i = 0; i < M; i++) ss += ev[i] * ev[i];
    r = sqrt(ss);
    int code = !isfinite(r) ? MGX_IK_FAILED : (r <= a.tol ? MGX_IK_CONVERGED : (it == a.max_iter ? MGX_IK_MAX_ITER : -1));
    code = __builtin_amdgcn_readfirstlane(code);
    if (code >= 0) { status = code; break; }

    // J: the weighted rows of mgx_jac, masked columns 0
    for (int p = 0; p < P; p++) {
      const int b = a.body[p], k = a.kind[p];
      const T px[3] = {pt[4 * p], pt[4 * p + 1], pt[4 * p + 2]}, w = pt[4 * p + 3];
      const T wp = wt[4 * p], wr = wt[4 * p + 1];
      const int rp = (int)wt[4 * p + 2], rr = (int)wt[4 * p + 3];
      for (int d = l; d < nv; d += 64) {
        T jp[3], jr[3];
        jac_column(m, e, b, k, px, w, d, jp, jr);
        const bool moves = !a.dof_mask || a.dof_mask[d];
        if (rp >= 0)
          for (int c = 0; c < 3; c++) J[(rp + c) * nv + d] = moves ? wp * jp[c] : (T)0;
        if (rr >= 0)
          for (int c = 0; c < 3; c++) J[(rr + c) * nv + d] = moves ? wr * jr[c] : (T)0;
      }
    }
    wsync();
    // A = J J' + lambda^2 I, the packed lower triangle: element (i, j <= i) at i (i + 1) / 2 + j
    const int nA = M * (M + 1) / 2;
    for (int idx = l; idx < nA; idx += 64) {
      int i = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
      while (i * (i + 1) / 2 > idx) i--;
      while ((i + 1) * (i + 2) / 2 <= idx) i++;
      const int j = idx - i * (i + 1) / 2;
      const T *Ji = J + i * nv, *Jj = J + j * nv;
      T s = 0;
      for (int d = 0; d < nv; d++) s += Ji[d] * Jj[d];
      if (i == j) s += a.damping2;
      A[idx] = s;
    }
    wsync();
    // Cholesky in place (left-looking): lane = row; the pivot of column j comes from lane j
    const bool row = l < M;
    bool bad = false;
    for (int j = 0; j < M; j++) {
      T s = 0;
      if (row && l >= j) {
        const T *Li = A + l * (l + 1) / 2, *Lj = A + j * (j + 1) / 2;
        s = Li[j];
        for (int k = 0; k < j; k++) s -= Li[k] * Lj[k];
      }
      const T pv = readlane(s, j);
      if (!(pv > 0) || !isfinite(pv)) { bad = true; break; }
      const T ljj = sqrt(pv);
      if (row && l >= j) A[l * (l + 1) / 2 + j] = l == j ? ljj : s / ljj;
      wsync();
    }
    if (bad) break;  // status MGX_IK_FAILED
    // L z = e, then L' y = z: lane = row, the solved entry broadcast
    T yi = row ? ev[l] : (T)0;
    for (int j = 0; j < M; j++) {
      const T yj = readlane(yi, j) / A[j * (j + 1) / 2 + j];
      if (l == j) yi = yj;
      else if (row && l > j) yi -= A[l * (l + 1) / 2 + j] * yj;
    }
    for (int j = M - 1; j >= 0; j--) {
      const T xj = readlane(yi, j) / A[j * (j + 1) / 2 + j];
      if (l == j) yi = xj;
      else if (l < j) yi -= A[j * (j + 1) / 2 + l] * xj;
    }
    if (row) y[l] = yi;
    wsync();
    // delta = J' y, its largest entry limited to max_step
    T smax = 0;
    for (int d = l; d < nv; d += 64) {
      T s = 0;
      for (int i = 0; i < M; i++) s += J[i * nv + d] * y[i];
      delta[d] = s;
      const T as = fabs(s);
      smax = as > smax ? as : smax;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const T t = __shfl_xor(smax, sh);
      smax = t > smax ? t : smax;
    }
    if (smax > a.max_step) {
      const T f = a.max_step / smax;
      for (int d = l; d < nv; d += 64) delta[d] *= f;
    }
    for (int k = l; k < nq; k += 64) qprev[k] = e.qpos[k];
    wsync();
    integrate_pos(m, e.qpos, delta, (T)1);
    if (a.dof_mask) {
      // what a masked dof owns keeps its bits (x + 0 may turn -0 into +0; mj_integratePos
      // renormalises a quaternion it does not rotate)
      for (int j = l; j < m.njnt; j += 64) {
        const int t = m.jnt_type[j], qa = m.jnt_qposadr[j], da = m.jnt_dofadr[j];
        if (t == JHINGE || t == JSLIDE) {
          if (!a.dof_mask[da]) e.qpos[qa] = qprev[qa];
        } else {
          const int ro = t == JFREE ? 3 : 0;
          if (t == JFREE)
            for (int c = 0; c < 3; c++)
              if (!a.dof_mask[da + c]) e.qpos[qa + c] = qprev[qa + c];
          if (!a.dof_mask[da + ro] && !a.dof_mask[da + ro + 1] && !a.dof_mask[da + ro + 2])
            for (int c = 0; c < 4; c++) e.qpos[qa + ro + c] = qprev[qa + ro + c];
        }
      }
      wsync();
    }
    if (a.clamp) ik_clamp(m, e.qpos, a.dof_mask);
    it++;
  }
  for (int k = l; k < nq; k += 64) a.qpos[(size_t)env * nq + k] = e.qpos[k];
  if (l == 0) {
    if (a.residual) a.residual[env] = r;
    if (a.iters) a.iters[env] = it;
    if (a.status) a.status[env] = status;
  }
}

// ------------------------------------------------------------------------- host side
template <typename T>
int ik_lds(const DevModel<T>& M, int P, int rows) {
  return ik_lds_reals(M.nq, M.nv, M.nu, M.nbody, M.njnt, M.nM, P, rows) * (int)sizeof(T);
}

template <typename T>
int configure(const DevModel<T>& M) {
  // the largest problem that fits: a call with more points or rows than the limit admits is refused
  int bytes = ik_lds(M, MGX_IK_MAX_POINT, MGX_IK_MAX_ROW);
  if (bytes > MGX_IK_LDS_LIMIT) bytes = MGX_IK_LDS_LIMIT;
  return mgx_set_lds(k_ik<T>, bytes);
}

template <typename T>
int launch_ik(DevModel<T> M, const mgx_state* s, int P, const int32_t* body, const int32_t* kind, const void* pos,
              const void* quat, const mgx_ik_io* io, int n_env, const uint8_t* mask, hipStream_t st) {
  IkArgs<T> a;
  a.body = (const int*)body; a.kind = (const int*)kind; a.pos = (const T*)pos; a.quat = (const T*)quat;
  a.target_pos = (const T*)io->target_pos; a.target_quat = (const T*)io->target_quat;
  a.qpos_init = (const T*)io->qpos_init; a.dof_mask = io->dof_mask;
  a.qpos = (T*)io->qpos; a.residual = (T*)io->residual; a.iters = io->iters; a.status = io->status;
  int rows = 0;
  for (int p = 0; p < MGX_IK_MAX_POINT; p++) {
    const bool in = p < P;
    a.pos_weight[p] = in ? (T)io->pos_weight[p] : (T)0;
    a.rot_weight[p] = in ? (T)io->rot_weight[p] : (T)0;
    a.row_pos[p] = a.row_rot[p] = -1;
    if (in && io->pos_weight[p] > 0) { a.row_pos[p] = (signed char)rows; rows += 3; }
    if (in && io->rot_weight[p] > 0) { a.row_rot[p] = (signed char)rows; rows += 3; }
  }
  a.damping2 = (T)io->damping * (T)io->damping; a.max_step = (T)io->max_step; a.tol = (T)io->tol;
  a.P = P; a.m = rows; a.max_iter = io->max_iter; a.clamp = (io->flags & MGX_IK_CLAMP_LIMITS) ? 1 : 0;
  const int bytes = ik_lds(M, P, rows);
  if (bytes > MGX_IK_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the inverse-kinematics kernel's LDS");
  M.L.late_geom = 1;
  hipLaunchKernelGGL(k_ik<T>, dim3(n_env), dim3(64), bytes, st, M, (const T*)s->qpos, a, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

}  // namespace

namespace mgx {
// dynamic-LDS attribute of k_ik (called by mgx_model_create); a model past the LDS limit still
// loads, and is refused by the call
int ik_kernels_configure(const mgx_model* m) {
  return m->precision == MGX_F32 ? configure(m->mf) : configure(m->md);
}
}  // namespace mgx

extern "C" {

int mgx_ik(const mgx_model* m, const mgx_state* s, int n_point, const int32_t* body, const int32_t* kind,
           const void* pos, const void* quat, const mgx_ik_io* io, int n_env, const uint8_t* env_mask, void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  if (n_point < 1 || n_point > MGX_IK_MAX_POINT || !body || !kind)
    return host_fail(MGX_E_ARG, "mgx_ik needs 1 <= n_point <= MGX_IK_MAX_POINT, body and kind");
  if (!io->qpos || !io->target_pos) return host_fail(MGX_E_ARG, "mgx_ik needs qpos and target_pos");
  if (!(io->damping > 0) || !(io->max_step > 0) || !(io->tol >= 0) || io->max_iter < 0)
    return host_fail(MGX_E_ARG, "mgx_ik needs damping > 0, max_step > 0, tol >= 0 and max_iter >= 0");
  if (io->flags & ~MGX_IK_CLAMP_LIMITS) return host_fail(MGX_E_ARG, "unknown mgx_ik flag bits");
  bool any = false, rot = false;
  for (int p = 0; p < n_point; p++) {
    const double wp = io->pos_weight[p], wr = io->rot_weight[p];
    if (!(wp >= 0) || !(wr >= 0) || !std::isfinite(wp) || !std::isfinite(wr))
      return host_fail(MGX_E_ARG, "mgx_ik weights must be finite and >= 0");
    any = any || wp > 0 || wr > 0;
    rot = rot || wr > 0;
  }
  if (!any) return host_fail(MGX_E_ARG, "mgx_ik: every weight is 0 (no row)");
  if (rot && !io->target_quat) return host_fail(MGX_E_ARG, "mgx_ik: a rot_weight > 0 needs target_quat");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (n_env == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32)
    return launch_ik<float>(m->mf, s, n_point, body, kind, pos, quat, io, n_env, env_mask, st);
  return launch_ik<double>(m->md, s, n_point, body, kind, pos, quat, io, n_env, env_mask, st);
}

}  // extern "C"
