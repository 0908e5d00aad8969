// mgx_dyn.hip — Jacobians, dense mass matrix, force vectors, inverse dynamics and energy
// (include/mgx.h "Jacobians, mass matrix, inverse dynamics and energy").
//
// Two kernels, one wave per env, over a slim Env binding (as k_sensor): kinematics / com_crb /
// velocity_bodies of mgx_physics.h from the current qpos and qvel, unchanged, then
//   k_jac<T>       the points' world positions, one lane per point, staged in LDS; then per point
//                  lane = dof (strided by 64), each row stored coalesced along nv.
//   k_dynamics<T>  the dense M row by row from the tree-sparse qM (each element written once,
//                  coalesced), the per-dof force terms of dof_force_applied one by one, M x by a
//                  gather over the dof's ancestors and DFS-contiguous descendants, the energies by
//                  lane 0.
// Every sum runs in a fixed order on one lane, so results are bit-reproducible and independent of
// the batch size; no atomics. Lanes stride over bodies and dofs: nothing is limited to 64.
#include <hip/hip_runtime.h>

#include <string>

#include "mgx_internal.h"
#include "mgx_physics.h"
#include "mgx_dyn.h"

using namespace mgx;

#define MGX_DYN_LDS_LIMIT (160 * 1024)

namespace {

// ------------------------------------------------------------------------- Jacobians
template <typename T>
__global__ void __launch_bounds__(64) k_jac(DevModel<T> m, const T* gqpos, int P, const int* body, const int* kind,
                                            const T* pos, int pos_per_env, T* jacp, T* jacr, T* point,
                                            const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the rows stay untouched
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* R = reinterpret_cast<T*>(smem);
  const int nv = m.nv, l = lane_id();
  Env<T> e;
  T* pt = R + dyn_bind(m, e, R, false);  // [MGX_JAC_CHUNK][4]: the point, 1 / subtree mass
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = gqpos[(size_t)env * m.nq + k];
  wsync();
  kinematics(m, e);  // m.L.late_geom == 1 (set by the launcher): no geom poses
  com_crb(m, e);
  for (int p0 = 0; p0 < P; p0 += MGX_JAC_CHUNK) {
    wsync();  // the previous chunk's points have been read
    const int p = p0 + l;
    if (p < P) {
      const int b = body[p], k = kind[p];
      T x[3], w, lp[3] = {0, 0, 0};
      if (pos) {
        const T* q = pos + ((pos_per_env ? (size_t)env * P : (size_t)0) + p) * 3;
        lp[0] = q[0]; lp[1] = q[1]; lp[2] = q[2];
      }
      jac_point(m, e, b, k, lp, x, w);
      for (int c = 0; c < 3; c++) pt[4 * l + c] = x[c];
      pt[4 * l + 3] = w;
      if (point)
        for (int c = 0; c < 3; c++) point[((size_t)env * P + p) * 3 + c] = x[c];
    }
    wsync();
    const int np = P - p0 < MGX_JAC_CHUNK ? P - p0 : MGX_JAC_CHUNK;
    for (int i = 0; i < np; i++) {
      const int b = body[p0 + i], k = kind[p0 + i];
      const T px[3] = {pt[4 * i], pt[4 * i + 1], pt[4 * i + 2]}, w = pt[4 * i + 3];
      const size_t at = ((size_t)env * P + p0 + i) * 3 * nv;
      for (int d = l; d < nv; d += 64) {
        T jp[3], jr[3];
        jac_column(m, e, b, k, px, w, d, jp, jr);
        if (jacp)
          for (int c = 0; c < 3; c++) jacp[at + (size_t)c * nv + d] = jp[c];
        if (jacr)
          for (int c = 0; c < 3; c++) jacr[at + (size_t)c * nv + d] = jr[c];
      }
    }
  }
}

// ------------------------------------------------------------------------- dynamics
// (M x)[d] from the tree-sparse qM (dof_Madr layout: row d holds M[d][d], M[d][parent], ...): the
// dof's own row, then its descendants d + 1 .. (DFS-contiguous: the dofs that follow while their
// chain is longer than d's), whose row holds M[i][d] at chainlen[i] - chainlen[d]
template <typename T>
__device__ __forceinline__ T mul_M(const DevModel<T>& m, const T* qM, const T* x, int d) {
  T s = 0;
  const int adr = m.dof_Madr[d], cl = m.dof_chainlen[d];
  int j = d;
  for (int t = 0; j >= 0; t++, j = m.dof_parentid[j]) s += qM[adr + t] * x[j];
  for (int i = d + 1; i < m.nv; i++) {
    const int t = m.dof_chainlen[i] - cl;
    if (t <= 0) break;
    s += qM[m.dof_Madr[i] + t] * x[i];
  }
  return s;
}

template <typename T>
__global__ void __launch_bounds__(64) k_dynamics(DevModel<T> m, const T* gqpos, const T* gqvel, const T* gctrl,
                                                 const T* gqfrc, const T* gxfrc, DynBuf<T> io,
                                                 const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the rows stay untouched
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* R = reinterpret_cast<T*>(smem);
  const int nb = m.nbody, nv = m.nv, l = lane_id();
  Env<T> e;
  T* qacc = R + dyn_bind(m, e, R, true);
  T* prod = qacc + nv;
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = gqpos[(size_t)env * m.nq + k];
  for (int k = l; k < nv; k += 64) e.qvel[k] = gqvel[(size_t)env * nv + k];
  for (int k = l; k < m.nu; k += 64) e.ctrl[k] = gctrl[(size_t)env * m.nu + k];
  for (int k = l; k < 6 * nb; k += 64) e.xfrc[k] = gxfrc[(size_t)env * 6 * nb + k];
  if (io.qacc)
    for (int k = l; k < nv; k += 64) qacc[k] = io.qacc[(size_t)env * nv + k];
  wsync();
  kinematics(m, e);  // m.L.late_geom == 1 (set by the launcher): no geom poses
  com_crb(m, e);
  const T* qM = e.qLD;
  if (io.M) {
    // mj_fullM: row r, lane = column; (r, c) is nonzero when one dof is an ancestor of the other
    T* M = io.M + (size_t)env * nv * nv;
    for (int r = 0; r < nv; r++) {
      const int ar = m.dof_Madr[r], cr = m.dof_chainlen[r];
      for (int c = l; c < nv; c += 64) {
        const int t = cr - m.dof_chainlen[c];
        T v = 0;
        if (c <= r) {
          if (t >= 0 && m.dof_anc[r * MGX_MAX_DEPTH + t] == c) v = qM[ar + t];
        } else if (t < 0 && m.dof_anc[c * MGX_MAX_DEPTH - t] == r) {
          v = qM[m.dof_Madr[c] - t];
        }
        M[(size_t)r * nv + c] = v;
      }
    }
  }
  // bias, actuator forces: the velocity stage (RNE subtree sums land in crb storage; qM is built)
  const bool need_vel = io.bias || io.actuator || io.inverse;
  if (need_vel) velocity_bodies(m, e);
  for (int d = l; d < nv; d += 64) {
    const size_t at = (size_t)env * nv + d;
    const int b = m.dof_bodyid[d], j = m.dof_jntid[d];
    const T* cd = e.cdof + 6 * d;
    // the terms of dof_force_applied (mgx_physics.h), one by one
    const T bias = need_vel ? dot6(cd, e.crb + 10 * b) : (T)0;
    T passive = -m.dof_damping[d] * e.qvel[d];
    const T st = m.jnt_stiffness[j];
    if (st != 0) {
      const int t = m.jnt_type[j], a = m.jnt_qposadr[j], k = d - m.jnt_dofadr[j];
      if (t == JHINGE || t == JSLIDE) passive -= st * (e.qpos[a] - m.qpos_spring[a]);
      else if (t == JFREE && k < 3) passive -= st * (e.qpos[a + k] - m.qpos_spring[a + k]);
    }
    if (io.bias) io.bias[at] = bias;
    if (io.passive) io.passive[at] = passive;
    if (io.actuator) {
      T act = 0;
      for (int u = 0; u < m.nu; u++)
        if (m.jnt_dofadr[m.actuator_trnid[u]] == d) act += m.actuator_gear[u] * e.act_force[u];
      io.actuator[at] = act;
    }
    if (io.external) {
      // qfrc_applied + J(xipos)' xfrc_applied over the bodies whose chain holds this dof
      T xf = 0;
      for (int i = 1; i < nb; i++) {
        const T* f = e.xfrc + 6 * i;
        if (f[0] == 0 && f[1] == 0 && f[2] == 0 && f[3] == 0 && f[4] == 0 && f[5] == 0) continue;
        if (!body_has_dof(m, i, d)) continue;
        const T* com = e.subtree_com + 3 * m.body_rootid[i];
        const T off[3] = {e.xipos[3 * i] - com[0], e.xipos[3 * i + 1] - com[1], e.xipos[3 * i + 2] - com[2]};
        T t[3];
        cross3(t, cd, off);
        xf += (cd[3] + t[0]) * f[0] + (cd[4] + t[1]) * f[1] + (cd[5] + t[2]) * f[2] + cd[0] * f[3] + cd[1] * f[4] +
              cd[2] * f[5];
      }
      io.external[at] = gqfrc[at] + xf;
    }
    if (io.inverse) {
      const T fc = io.qfrc_constraint ? io.qfrc_constraint[at] : (T)0;
      io.inverse[at] = mul_M(m, qM, qacc, d) + bias - passive - fc;
    }
    if (io.energy) prod[d] = e.qvel[d] * mul_M(m, qM, e.qvel, d);
  }
  if (!io.energy) return;
  wsync();
  if (l == 0) {
    // mj_energyPos / mj_energyVel: gravity and springs; v' M v / 2, summed in dof order
    T pot = 0, kin = 0;
    for (int b = 1; b < nb; b++) pot -= m.body_mass[b] * dot3(m.gravity, e.xipos + 3 * b);
    for (int j = 0; j < m.njnt; j++) {
      const T st = m.jnt_stiffness[j];
      if (st == 0) continue;
      const int t = m.jnt_type[j], a = m.jnt_qposadr[j];
      if (t == JHINGE || t == JSLIDE) {
        const T dq = e.qpos[a] - m.qpos_spring[a];
        pot += (T)0.5 * st * dq * dq;
      } else if (t == JFREE) {
        for (int k = 0; k < 3; k++) {
          const T dq = e.qpos[a + k] - m.qpos_spring[a + k];
          pot += (T)0.5 * st * dq * dq;
        }
      }
    }
    for (int d = 0; d < nv; d++) kin += prod[d];
    io.energy[2 * (size_t)env] = pot;
    io.energy[2 * (size_t)env + 1] = (T)0.5 * kin;
  }
}

// ------------------------------------------------------------------------- host side
template <typename T>
int model_lds(const DevModel<T>& M, bool jac) {
  const int reals = jac ? jac_lds_reals(M.nq, M.nv, M.nu, M.nbody, M.njnt, M.nM)
                        : dyn_lds_reals(M.nq, M.nv, M.nu, M.nbody, M.njnt, M.nM, 1);
  return reals * (int)sizeof(T);
}

template <typename T>
int configure(const DevModel<T>& M) {
  const int bj = model_lds(M, true), bd = model_lds(M, false);
  int rc = MGX_OK;
  if (bj <= MGX_DYN_LDS_LIMIT) rc = mgx_set_lds(k_jac<T>, bj);
  if (rc == MGX_OK && bd <= MGX_DYN_LDS_LIMIT) rc = mgx_set_lds(k_dynamics<T>, bd);
  return rc;
}

template <typename T>
int launch_jac(DevModel<T> M, const mgx_state* s, int P, const int32_t* body, const int32_t* kind, const void* pos,
               int pos_per_env, void* jacp, void* jacr, void* point, int n_env, const uint8_t* mask, hipStream_t st) {
  const int bytes = model_lds(M, true);
  if (bytes > MGX_DYN_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the Jacobian kernel's LDS");
  M.L.late_geom = 1;
  hipLaunchKernelGGL(k_jac<T>, dim3(n_env), dim3(64), bytes, st, M, (const T*)s->qpos, P, (const int*)body,
                     (const int*)kind, (const T*)pos, pos_per_env, (T*)jacp, (T*)jacr, (T*)point, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

template <typename T>
int launch_dynamics(DevModel<T> M, const mgx_state* s, const mgx_dyn_io* io, int n_env, const uint8_t* mask,
                    hipStream_t st) {
  const int bytes = model_lds(M, false);
  if (bytes > MGX_DYN_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the dynamics kernel's LDS");
  M.L.late_geom = 1;
  const DynBuf<T> b{(const T*)io->qacc, (const T*)io->qfrc_constraint, (T*)io->M, (T*)io->qfrc_bias,
                    (T*)io->qfrc_passive, (T*)io->qfrc_actuator, (T*)io->qfrc_external, (T*)io->qfrc_inverse,
                    (T*)io->energy};
  hipLaunchKernelGGL(k_dynamics<T>, dim3(n_env), dim3(64), bytes, st, M, (const T*)s->qpos, (const T*)s->qvel,
                     (const T*)s->ctrl, (const T*)s->qfrc_applied, (const T*)s->xfrc_applied, b, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

}  // namespace

namespace mgx {
// dynamic-LDS attributes of k_jac / k_dynamics (called by mgx_model_create); a model past the LDS
// limit still loads, and is refused by the calls
int dyn_kernels_configure(const mgx_model* m) {
  return m->precision == MGX_F32 ? configure(m->mf) : configure(m->md);
}
}  // namespace mgx

extern "C" {

int mgx_jac(const mgx_model* m, const mgx_state* s, int n_point, const int32_t* body, const int32_t* kind,
            const void* pos, int pos_per_env, void* jacp, void* jacr, void* point, int n_env,
            const uint8_t* env_mask, void* stream) {
  if (!m || n_env < 0) return host_fail(MGX_E_ARG, "null model or n_env < 0");
  if (n_point < 1 || !body || !kind) return host_fail(MGX_E_ARG, "mgx_jac needs n_point >= 1, body and kind");
  if (pos_per_env != 0 && pos_per_env != 1) return host_fail(MGX_E_ARG, "pos_per_env is 0 or 1");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (n_env == 0 || (!jacp && !jacr && !point)) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32)
    return launch_jac<float>(m->mf, s, n_point, body, kind, pos, pos_per_env, jacp, jacr, point, n_env, env_mask, st);
  return launch_jac<double>(m->md, s, n_point, body, kind, pos, pos_per_env, jacp, jacr, point, n_env, env_mask, st);
}

int mgx_dynamics(const mgx_model* m, const mgx_state* s, const mgx_dyn_io* io, int n_env, const uint8_t* env_mask,
                 void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  if (io->qfrc_inverse && !io->qacc) return host_fail(MGX_E_ARG, "qfrc_inverse needs qacc");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (n_env == 0 || (!io->M && !io->qfrc_bias && !io->qfrc_passive && !io->qfrc_actuator && !io->qfrc_external &&
                     !io->qfrc_inverse && !io->energy))
    return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return launch_dynamics<float>(m->mf, s, io, n_env, env_mask, st);
  return launch_dynamics<double>(m->md, s, io, n_env, env_mask, st);
}

}  // extern "C"
