// mgx_ik.h — arguments and LDS size of mgx_ik (include/mgx.h "inverse kinematics").
#pragma once
#include "../../include/mgx.h"
#include "mgx_dyn.h"

namespace mgx {

// One mgx_ik call, typed: the shared point tables, the caller's buffers (mgx_ik_io) and the host
// fields in the model's real type. row_pos / row_rot: the first of a point's three position /
// orientation rows in e and J, -1 when its weight is 0.
template <typename T>
struct IkArgs {
  const int *body, *kind;
  const T *pos, *quat;
  const T *target_pos, *target_quat, *qpos_init;
  const uint8_t* dof_mask;
  T* qpos;
  T* residual;
  int *iters, *status;
  T pos_weight[MGX_IK_MAX_POINT], rot_weight[MGX_IK_MAX_POINT];
  T damping2, max_step, tol;  // damping2 = lambda^2
  int P, m, max_iter, clamp;
  signed char row_pos[MGX_IK_MAX_POINT], row_rot[MGX_IK_MAX_POINT];
};

// reals per point kept in LDS: the world point and 1 / subtree mass [4], the target position [3],
// the normalised target quaternion [4], the body-frame orientation offset [4], and its weights and
// first rows [4] (IkArgs' arrays, indexed there by constants only)
#define MGX_IK_POINT_REALS 19

// reals of LDS one env takes (k_ik binds them in this order): the position stages of k_jac
// (dyn_lds_reals without velocities), q before the update [nq], J [m][nv], e [m], the packed lower
// triangle of A [m (m + 1) / 2], y [m], delta [nv] and the points
__host__ __device__ inline int ik_lds_reals(int nq, int nv, int nu, int nb, int nj, int nM, int P, int m) {
  return dyn_lds_reals(nq, nv, nu, nb, nj, nM, 0) + nq + m * nv + m + m * (m + 1) / 2 + m + nv +
         MGX_IK_POINT_REALS * P;
}

}  // namespace mgx
