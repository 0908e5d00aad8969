// mgx_manifold.h — the state tangent x = (dq [nv], qvel [nv]): which array entry, or which
// quaternion and axis, row r lives in, and the difference of two states in it (MuJoCo's
// mj_differentiatePos [ext]). One definition for mgx_transition_fd's k_fd_diff, mgx_state_diff and
// the feedback law of mgx_rollout_feedback (include/mgx.h).
#pragma once
#include "mgx_common.h"

namespace mgx {

// Component `axis` of mj_differentiatePos for one quaternion: the rotation vector of conj(qb) o qa,
// angle 2 atan2(|v|, w) wrapped to (-pi, pi]; a zero vector gives 0.
// Evaluated in double whatever T is: conj(qb) o qa cancels to a vector of size |A| eps, and in
// float the product's rounding (6e-8 of components near 1) would be 1e-4 of that at eps = 2^-10.
__device__ __forceinline__ double tangent_rotvec(const double* qa, const double* qb, int axis) {
  const double cb[4] = {qb[0], -qb[1], -qb[2], -qb[3]};
  double d[4];
  mulquat(d, cb, qa);
  const double n = sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  if (n == 0) return 0;
  double ang = 2.0 * atan2(n, d[0]);
  if (ang > 3.14159265358979323846) ang -= 6.28318530717958647692;
  const double x = axis == 0 ? d[1] : (axis == 1 ? d[2] : d[3]);
  return x / n * ang;
}

// Row r of the state tangent: where it lives in a state's arrays.
struct TangentRow {
  int qi;          // >= 0: qpos[qi] (hinge, slide, free translation) or, with vel, qvel[qi]
  int quat, axis;  // quat >= 0: component `axis` of the quaternion at qpos[quat .. quat + 4)
  int vel;
};

// The map dof -> (qpos entry | quaternion, axis) for r < nv, qvel[r - nv] for nv <= r < 2 nv;
// any other r gives the scalar row qpos[0] (callers mask it).
template <typename T>
__device__ __forceinline__ TangentRow tangent_row(const DevModel<T>& m, int r) {
  TangentRow R{0, -1, 0, 0};
  const int nv = m.nv;
  if (r < 0) return R;
  if (r < nv) {
    const int j = m.dof_jntid[r], t = m.jnt_type[j], a = m.jnt_qposadr[j], k = r - m.jnt_dofadr[j];
    if (t == JFREE && k >= 3) { R.quat = a + 3; R.axis = k - 3; }
    else if (t == JBALL) { R.quat = a; R.axis = k; }
    else R.qi = a + k;
  } else if (r < 2 * nv) {
    R.vel = 1; R.qi = r - nv;
  }
  return R;
}

// x[r] of state a (qpos qa, qvel va) minus that of state b, in the tangent space.
// SAME_IS_ZERO: a quaternion row of q_a == q_b or q_a == -q_b (component-wise) is exactly 0, decided
// before the product, whose fused multiply-adds otherwise leave a rounding residue of some 1e-17.
// mgx_state_diff and the feedback law promise that zero (a rollout that sits on its nominal gets
// its nominal control bit for bit); k_fd_diff keeps the plain product, and so its bits.
template <bool SAME_IS_ZERO, typename T>
__device__ __forceinline__ T tangent_delta(const TangentRow& R, const T* qa, const T* va, const T* qb, const T* vb) {
  if (R.vel) return va[R.qi] - vb[R.qi];
  if (R.quat < 0) return qa[R.qi] - qb[R.qi];
  const T* a = qa + R.quat;
  const T* b = qb + R.quat;
  if (SAME_IS_ZERO) {
    if (a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]) return 0;
    if (a[0] == -b[0] && a[1] == -b[1] && a[2] == -b[2] && a[3] == -b[3]) return 0;
  }
  const double da[4] = {(double)a[0], (double)a[1], (double)a[2], (double)a[3]};
  const double db[4] = {(double)b[0], (double)b[1], (double)b[2], (double)b[3]};
  return (T)tangent_rotvec(da, db, R.axis);
}

}  // namespace mgx
