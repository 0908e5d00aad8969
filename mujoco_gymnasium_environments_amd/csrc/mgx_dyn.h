// mgx_dyn.h — buffer views and LDS sizes of mgx_jac / mgx_dynamics (include/mgx.h "Jacobians, mass
// matrix, inverse dynamics and energy").
#pragma once
#include "../../include/mgx.h"
#include "mgx_common.h"

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

}  // namespace mgx
