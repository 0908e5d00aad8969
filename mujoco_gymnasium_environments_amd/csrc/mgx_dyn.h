// mgx_dyn.h — buffer views and LDS sizes of mgx_jac / mgx_dynamics (include/mgx.h "Jacobians, mass
// matrix, inverse dynamics and energy"), and the device code mgx_ik.hip shares with
// them: the slim Env binding, a point's world position and a column of its Jacobians.
#pragma once
#include "../../include/mgx.h"
#include "mgx_common.h"
#include "mgx_physics.h"

namespace mgx {

// Caller buffers of one mgx_dynamics call, typed (mgx_dyn_io).
template <typename T>
struct DynBuf {
  const T *qacc, *qfrc_constraint;
  T *M, *bias, *passive, *actuator, *external, *inverse, *energy;
};

#define MGX_JAC_CHUNK 64  // points whose world position k_jac stages in LDS at a time (one per lane)

// reals of LDS one env binds (dyn_bind, mgx_dyn.hip, takes them in this order): qpos, the arrays
// kinematics / com_crb write (body frames 51 nbody, joint axes and anchors, cdof, qM, qMH) and, with
// `vel`, what velocity_bodies and the per-dof forces add: qvel, ctrl, act_force, xfrc_applied, cvel,
// cfrc, cdof_dot, qacc and one [nv] vector of products
__host__ __device__ inline int dyn_lds_reals(int nq, int nv, int nu, int nb, int nj, int nM, int vel) {
  int n = nq + 51 * nb + 6 * nj + 6 * nv + 2 * nM;
  if (vel) n += nv + 2 * nu + 18 * nb + 6 * nv + 2 * nv;
  return n;
}
// k_jac: the position stages and MGX_JAC_CHUNK staged points (x, y, z, 1 / subtree mass)
__host__ __device__ inline int jac_lds_reals(int nq, int nv, int nu, int nb, int nj, int nM) {
  return dyn_lds_reals(nq, nv, nu, nb, nj, nM, 0) + 4 * MGX_JAC_CHUNK;
}

// the slim binding of k_jac / k_dynamics / k_ik; returns the reals taken (dyn_lds_reals)
template <typename T>
__device__ __forceinline__ int dyn_bind(const DevModel<T>& m, Env<T>& e, T* R, bool vel) {
  const int nb = m.nbody, nj = m.njnt, nv = m.nv;
  int o = 0;
  auto take = [&](int n) { T* r = R + o; o += n; return r; };
  e.qpos = take(m.nq);
  e.xpos = take(3 * nb); e.xquat = take(4 * nb); e.xmat = take(9 * nb); e.xipos = take(3 * nb);
  e.ximat = take(9 * nb); e.subtree_com = take(3 * nb); e.cinert = take(10 * nb); e.crb = take(10 * nb);
  e.xaxis = take(3 * nj); e.xanchor = take(3 * nj); e.cdof = take(6 * nv);
  e.qLD = take(m.nM); e.qMH = take(m.nM);  // com_crb leaves qM in qLD (nothing factors it here)
  if (vel) {
    e.qvel = take(nv); e.ctrl = take(m.nu); e.act_force = take(m.nu); e.xfrc = take(6 * nb);
    e.cvel = take(6 * nb); e.cfrc = take(6 * nb); e.cdof_dot = take(6 * nv);
  }
  return o;
}

// The world point x of one mgx_jac entry (body b, kind k, table position lp) after kinematics and
// com_crb, and w = 1 / subtree mass for MGX_JAC_SUBTREECOM (0 otherwise, and for a massless
// subtree). A body out of range gives zeros.
template <typename T>
__device__ __forceinline__ void jac_point(const DevModel<T>& m, const Env<T>& e, int b, int k, const T* lp, T* x, T& w) {
  x[0] = x[1] = x[2] = 0;
  w = 0;
  if ((unsigned)b >= (unsigned)m.nbody) return;
  if (k == MGX_JAC_WORLD) {
    x[0] = lp[0]; x[1] = lp[1]; x[2] = lp[2];
  } else if (k == MGX_JAC_LOCAL) {
    mulmatvec3(x, e.xmat + 9 * b, lp);
    for (int c = 0; c < 3; c++) x[c] += e.xpos[3 * b + c];
  } else if (k == MGX_JAC_BODYCOM) {
    for (int c = 0; c < 3; c++) x[c] = e.xipos[3 * b + c];
  } else if (k == MGX_JAC_SUBTREECOM) {
    for (int c = 0; c < 3; c++) x[c] = e.subtree_com[3 * b + c];
    T ms = 0;
    const int end = m.body_subtree_end[b];
    for (int i = b; i < end; i++) ms += m.body_mass[i];
    // a massless subtree: com_crb put its com at xipos[b]; the body-com Jacobian goes with it
    w = ms < minval<T>() ? (T)0 : (T)1 / ms;
  }
}

// Column d of that entry's Jacobians (jp translational, jr rotational) at the world point px
template <typename T>
__device__ __forceinline__ void jac_column(const DevModel<T>& m, const Env<T>& e, int b, int k, const T* px, T w, int d,
                                           T* jp, T* jr) {
  const bool ok = (unsigned)b < (unsigned)m.nbody && (unsigned)k <= (unsigned)MGX_JAC_SUBTREECOM;
  jp[0] = jp[1] = jp[2] = 0;
  jr[0] = jr[1] = jr[2] = 0;
  const T* cd = e.cdof + 6 * d;
  if (ok && k == MGX_JAC_SUBTREECOM && w > 0) {
    // mass-weighted body-com Jacobians of the DFS-contiguous subtree, in body order
    const int end = m.body_subtree_end[b];
    for (int j = b; j < end; j++) {
      if (!body_has_dof(m, j, d)) continue;
      const T* com = e.subtree_com + 3 * m.body_rootid[j];
      const T off[3] = {e.xipos[3 * j] - com[0], e.xipos[3 * j + 1] - com[1], e.xipos[3 * j + 2] - com[2]};
      T t[3];
      cross3(t, cd, off);
      const T mj = m.body_mass[j];
      for (int c = 0; c < 3; c++) jp[c] += mj * (cd[3 + c] + t[c]);
    }
    for (int c = 0; c < 3; c++) jp[c] *= w;
  } else if (ok && body_has_dof(m, b, d)) {
    const T* com = e.subtree_com + 3 * m.body_rootid[b];
    const T off[3] = {px[0] - com[0], px[1] - com[1], px[2] - com[2]};
    T t[3];
    cross3(t, cd, off);
    for (int c = 0; c < 3; c++) jp[c] = cd[3 + c] + t[c];
    if (k != MGX_JAC_SUBTREECOM)
      for (int c = 0; c < 3; c++) jr[c] = cd[c];
  }
}

}  // namespace mgx
