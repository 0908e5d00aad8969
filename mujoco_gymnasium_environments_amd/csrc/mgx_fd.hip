// mgx_fd.hip — finite-difference transition derivatives (MuJoCo's mjd_transitionFD [ext]) and
// their C-ABI: mgx_transition_fd_bytes, mgx_transition_fd (include/mgx.h).
//
// One env's linearisation is C = 1 + K (centred: 1 + 2 K) independent mj_steps, K = 2 nv + nu: the
// nominal one and one per perturbed coordinate. A pass materialises them as virtual envs in the
// caller's workspace and steps them with mgx_step itself, so the derivative is that of the step
// the user runs:
//   k_fd_expand  one wave per virtual env: copies the env's state rows (coalesced), the lane that
//                owns the perturbed coordinate perturbs it, and records the signed step taken;
//   mgx_step     on the workspace's mgx_state, nsub substeps, no frames;
//   k_fd_diff    one workgroup per env: differences in the tangent space and transposes
//                (virtual env = column, dof = row) through an LDS tile into row-major A and B.
// mgx_sensor_fd_bytes, mgx_sensor_fd are the other half of mjd_transitionFD, the
// sensor derivatives C and D: the same k_fd_expand, then no step but
//   mgx_forward  on the virtual envs, where an acceleration-stage sensor needs it;
//   mgx_sensor   into one staging row per virtual env;
//   k_sens_diff  one workgroup per env and column tile: plain differences of the staging rows, transposed
//                (virtual env = column, sensordata entry = row) through the same LDS tile.
// No atomics anywhere: results are bit-reproducible.
#include "mgx_internal.h"
#include "mgx_fd.h"
#include "mgx_manifold.h"
#include "mgx_sensor.h"

using namespace mgx;

namespace {

// ------------------------------------------------------------------ expand
// Virtual env v of the pass: env e0 + v / C, copy c = v % C. c = 0 is the nominal state, c = 1 + k
// perturbs column k by +eps and (centred) c = 1 + K + k by -eps. Columns: k < nv the position
// tangent (mj_integratePos along dof k), nv <= k < 2 nv qvel, 2 nv + u ctrl[u].
template <typename T>
__global__ void __launch_bounds__(64) k_fd_expand(DevModel<T> m, mgx_state s, FdBuf<T> w, int e0, int C, int K,
                                                  int centered, T eps, const uint8_t* mask) {
  const int v = blockIdx.x, l = threadIdx.x;
  const int env = e0 + v / C, c = v % C;
  if (mask) {
    const bool on = mask[env] != 0;
    if (l == 0) w.vmask[v] = on ? 1 : 0;
    if (!on) return;
  }
  const int nq = m.nq, nv = m.nv, nu = m.nu, nx = 6 * m.nbody;
  const T* sctrl = (const T*)s.ctrl + (size_t)env * nu;
  T h = 0;             // the signed step this virtual env takes
  int qa = -1;         // scalar qpos entry that takes it
  int quat = -1, axis = 0;  // or: the quaternion at qpos[quat .. quat + 4) turns about its local axis
  int dv = -1, du = -1;     // or: a qvel / ctrl entry
  if (c > 0) {
    const int col = (c - 1) % K;
    h = (c - 1) / K ? -eps : eps;
    if (col < nv) {
      const TangentRow R = tangent_row(m, col);
      if (R.quat >= 0) { quat = R.quat; axis = R.axis; }
      else qa = R.qi;
    } else if (col < 2 * nv) {
      dv = col - nv;
    } else {
      du = col - 2 * nv;
      // a perturbation that would leave the range of a limited actuator is not taken: forward mode
      // falls back to -eps, then to no step; centred mode drops the side that leaves
      if (m.actuator_ctrllimited[du]) {
        const T lo = m.actuator_ctrlrange[2 * du], hi = m.actuator_ctrlrange[2 * du + 1];
        const T cn = clampv(sctrl[du], lo, hi);
        const bool up = cn + eps <= hi, dn = cn - eps >= lo;
        if (centered) { if (h > 0 ? !up : !dn) h = 0; }
        else h = up ? eps : (dn ? -eps : (T)0);
      }
    }
  }
  const T* sq = (const T*)s.qpos + (size_t)env * nq;
  T* dq = w.qpos + (size_t)v * nq;
  for (int k = l; k < nq; k += 64) {
    if (quat >= 0 && k >= quat && k < quat + 4) continue;  // lane 0 writes the turned quaternion below
    T x = sq[k];
    if (k == qa) x += h;
    dq[k] = x;
  }
  if (quat >= 0 && l == 0) {
    // in double whatever T is: a handful of flops on one lane, and the step actually taken then
    // misses eps only by the final rounding of the four components to T
    const double q[4] = {(double)sq[quat], (double)sq[quat + 1], (double)sq[quat + 2], (double)sq[quat + 3]};
    const double hh = 0.5 * (double)h, sn = sin(hh);
    const double tw[4] = {cos(hh), axis == 0 ? sn : 0.0, axis == 1 ? sn : 0.0, axis == 2 ? sn : 0.0};
    double r[4];
    mulquat(r, q, tw);
    normalize4(r);
    dq[quat] = (T)r[0]; dq[quat + 1] = (T)r[1]; dq[quat + 2] = (T)r[2]; dq[quat + 3] = (T)r[3];
  }
  const T* sv = (const T*)s.qvel + (size_t)env * nv;
  const T* sa = (const T*)s.qacc_warmstart + (size_t)env * nv;
  const T* sf = (const T*)s.qfrc_applied + (size_t)env * nv;
  for (int k = l; k < nv; k += 64) {
    T x = sv[k];
    if (k == dv) x += h;
    w.qvel[(size_t)v * nv + k] = x;
    w.qacc[(size_t)v * nv + k] = sa[k];
    w.qfrc[(size_t)v * nv + k] = sf[k];
  }
  // the nominal ctrl is the value the step uses: clamped where the actuator is limited
  for (int k = l; k < nu; k += 64) {
    T x = sctrl[k];
    if (m.actuator_ctrllimited[k]) x = clampv(x, m.actuator_ctrlrange[2 * k], m.actuator_ctrlrange[2 * k + 1]);
    if (k == du) x += h;
    w.ctrl[(size_t)v * nu + k] = x;
  }
  const T* sx = (const T*)s.xfrc_applied + (size_t)env * nx;
  for (int k = l; k < nx; k += 64) w.xfrc[(size_t)v * nx + k] = sx[k];
  if (l == 0) {
    w.time[v] = ((const T*)s.time)[env];
    w.warning[v] = 0;
    w.overflow[v] = 0;
    w.step[v] = h;
  }
}

// ------------------------------------------------------------------ difference
// x'[r] of virtual env va minus that of vb, in the tangent space (mgx_manifold.h: the rotation
// vector of a quaternion row in double whatever T is)
template <typename T>
__device__ __forceinline__ T fd_delta(const FdBuf<T>& w, int nq, int nv, const TangentRow& R, size_t va, size_t vb) {
  return tangent_delta<false>(R, w.qpos + va * nq, w.qvel + va * nv, w.qpos + vb * nq, w.qvel + vb * nv);
}

// One workgroup of 4 waves per env. The output's contiguous index is the column (a virtual env),
// the input's the row (a dof of one virtual env): tiles of MGX_FD_TILE columns x MGX_FD_TILE rows
// are read with lane = row (coalesced along dofs), transposed through LDS (row pitch padded by one
// real against bank conflicts) and stored with lane = column (coalesced along A's / B's rows).
template <typename T>
__global__ void __launch_bounds__(256) k_fd_diff(DevModel<T> m, FdBuf<T> w, int e0, int C, int K, int centered, T eps,
                                                 const uint8_t* mask) {
  __shared__ T tile[MGX_FD_TILE * (MGX_FD_TILE + 1)];
  __shared__ int red[256];
  const int env = e0 + blockIdx.x;
  if (mask && !mask[env]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = m.nq, nv = m.nv, nu = m.nu, nx2 = 2 * nv;
  const size_t base = (size_t)blockIdx.x * C;
  const T eps2 = (T)2 * eps;
  if (w.A || w.B) {
    for (int r0 = 0; r0 < nx2; r0 += MGX_FD_TILE) {
      const int r = r0 + lane;
      const TangentRow R = tangent_row(m, r);
      for (int c0 = 0; c0 < K; c0 += MGX_FD_TILE) {
        if (!w.A && c0 + MGX_FD_TILE <= nx2) continue;  // a tile of A only (uniform over the workgroup)
        if (!w.B && c0 >= nx2) continue;                // a tile of B only
        __syncthreads();
        for (int cc = wave; cc < MGX_FD_TILE; cc += 4) {
          const int c = c0 + cc;
          T val = 0;
          if (r < nx2 && c < K) {
            const size_t vp = base + 1 + c;
            const T hp = w.step[vp];
            if (!centered) {
              if (hp != 0) val = fd_delta(w, nq, nv, R, vp, base) / hp;
            } else {
              const size_t vm = vp + K;
              const T hm = w.step[vm];
              if (hp != 0 && hm != 0) val = fd_delta(w, nq, nv, R, vp, vm) / eps2;
              else if (hp != 0) val = fd_delta(w, nq, nv, R, vp, base) / hp;
              else if (hm != 0) val = fd_delta(w, nq, nv, R, vm, base) / hm;
            }
          }
          tile[lane * (MGX_FD_TILE + 1) + cc] = val;
        }
        __syncthreads();
        for (int rr = wave; rr < MGX_FD_TILE; rr += 4) {
          const int ro = r0 + rr, c = c0 + lane;
          if (ro < nx2 && c < K) {
            const T val = tile[rr * (MGX_FD_TILE + 1) + lane];
            if (c < nx2) { if (w.A) w.A[((size_t)env * nx2 + ro) * nx2 + c] = val; }
            else if (w.B) w.B[((size_t)env * nx2 + ro) * nu + (c - nx2)] = val;
          }
        }
      }
    }
  }
  // bad-state resets of the env's C steps: integer sums, so the tree's order does not matter
  if (w.out_warning) {
    int sum = 0;
    for (int i = tid; i < C; i += 256) sum += w.warning[base + i];
    red[tid] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) w.out_warning[env] = red[0];
  }
  if (w.next_qpos) for (int k = tid; k < nq; k += 256) w.next_qpos[(size_t)env * nq + k] = w.qpos[base * nq + k];
  if (w.next_qvel) for (int k = tid; k < nv; k += 256) w.next_qvel[(size_t)env * nv + k] = w.qvel[base * nv + k];
}

// ------------------------------------------------------------------ sensor difference
// One workgroup of 4 waves per env and column tile (blockIdx.y; a pass is some tens of envs, so the
// column tiles are what fills the device), the transposing tile of k_fd_diff: the input's contiguous
// index is the sensordata entry of one virtual env, the output's the column (a virtual env). Tiles
// of MGX_FD_TILE columns x MGX_FD_TILE rows are read with lane = sensordata row (coalesced along
// the staging row), go through LDS (row pitch padded by one real) and are stored with lane = column
// (coalesced along C's / D's rows); the workgroup loops over the row tiles. Rows are plain
// differences: a framequat's four components included. Every virtual env of a selected env holds a
// state (the nominal one where no step was taken), so its staging row is read before the step
// decides what to do with it: the loads of a tile do not wait for one another. The nominal row goes
// to `sensordata` (column tile 0).
template <typename T>
__global__ void __launch_bounds__(256) k_sens_diff(SensFdBuf<T> w, int e0, int C, int K, int centered, T eps,
                                                   const uint8_t* mask) {
  __shared__ T tile[MGX_FD_TILE * (MGX_FD_TILE + 1)];
  const int env = e0 + blockIdx.x;
  if (mask && !mask[env]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ns = w.ns, nu = w.nu, nx2 = 2 * w.nv;
  const size_t base = (size_t)blockIdx.x * C;
  const T eps2 = (T)2 * eps;
  const int c0 = blockIdx.y * MGX_FD_TILE;
  // a tile of C only, or of D only, whose output is not wanted (uniform over the workgroup)
  const bool skip = (!w.C && c0 + MGX_FD_TILE <= nx2) || (!w.D && c0 >= nx2);
  if ((w.C || w.D) && !skip) {
    for (int r0 = 0; r0 < ns; r0 += MGX_FD_TILE) {
      const int r = r0 + lane;
      const T s0 = r < ns ? w.sens[base * ns + r] : (T)0;  // the nominal row's entry
      __syncthreads();
      for (int cc = wave; cc < MGX_FD_TILE; cc += 4) {
        const int c = c0 + cc;
        T val = 0;
        if (r < ns && c < K) {
          const size_t vp = base + 1 + c;
          const T hp = w.step[vp], sp = w.sens[vp * ns + r];
          if (!centered) {
            if (hp != 0) val = (sp - s0) / hp;
          } else {
            const size_t vm = vp + K;
            const T hm = w.step[vm], sm = w.sens[vm * ns + r];
            if (hp != 0 && hm != 0) val = (sp - sm) / eps2;
            else if (hp != 0) val = (sp - s0) / hp;
            else if (hm != 0) val = (sm - s0) / hm;
          }
        }
        tile[lane * (MGX_FD_TILE + 1) + cc] = val;
      }
      __syncthreads();
      for (int rr = wave; rr < MGX_FD_TILE; rr += 4) {
        const int ro = r0 + rr, c = c0 + lane;
        if (ro < ns && c < K) {
          const T val = tile[rr * (MGX_FD_TILE + 1) + lane];
          if (c < nx2) { if (w.C) w.C[((size_t)env * ns + ro) * nx2 + c] = val; }
          else if (w.D) w.D[((size_t)env * ns + ro) * nu + (c - nx2)] = val;
        }
      }
    }
  }
  if (w.sensordata && blockIdx.y == 0)
    for (int k = tid; k < ns; k += 256) w.sensordata[(size_t)env * ns + k] = w.sens[base * ns + k];
}

struct FdDims { int nq, nv, nu, nbody, real_bytes; size_t scratch; };

int fd_dims(const mgx_model* m, FdDims* d) {
  mgx_model_info info;
  const int rc = mgx_model_get_info(m, &info);
  if (rc) return rc;
  *d = FdDims{info.nq, info.nv, info.nu, info.nbody, m->precision == MGX_F32 ? 4 : 8, (size_t)info.scratch_bytes_per_env};
  return MGX_OK;
}

template <typename T>
int run_fd(const mgx_model* m, const DevModel<T>& M, const FdDims& d, const mgx_state* s, const mgx_fd_io* io, int n_env,
           const uint8_t* mask, hipStream_t st) {
  const int K = 2 * d.nv + d.nu, centered = io->flags & MGX_FD_CENTERED ? 1 : 0, C = 1 + (centered ? 2 : 1) * K;
  const FdLayout o = fd_layout(d.nq, d.nv, d.nu, d.nbody, d.real_bytes, d.scratch, io->slots);
  char* ws = (char*)io->workspace;
  FdBuf<T> w{(T*)(ws + o.qpos), (T*)(ws + o.qvel), (T*)(ws + o.qacc), (T*)(ws + o.ctrl), (T*)(ws + o.qfrc),
             (T*)(ws + o.xfrc), (T*)(ws + o.time), (T*)(ws + o.step), (int32_t*)(ws + o.warning),
             (int32_t*)(ws + o.overflow), (uint8_t*)(ws + o.vmask), (T*)io->A, (T*)io->B, (T*)io->next_qpos,
             (T*)io->next_qvel, io->warning};
  mgx_state vs{};
  vs.qpos = w.qpos; vs.qvel = w.qvel; vs.qacc_warmstart = w.qacc; vs.ctrl = w.ctrl; vs.qfrc_applied = w.qfrc;
  vs.xfrc_applied = w.xfrc; vs.time = w.time; vs.warning = w.warning; vs.overflow = w.overflow;
  vs.scratch = d.scratch ? ws + o.scratch : nullptr;
  const int per = io->slots / C;  // envs per pass
  const T eps = (T)io->eps;
  for (int e0 = 0; e0 < n_env; e0 += per) {
    const int cnt = n_env - e0 < per ? n_env - e0 : per;
    hipLaunchKernelGGL(k_fd_expand<T>, dim3(cnt * C), dim3(64), 0, st, M, *s, w, e0, C, K, centered, eps, mask);
    MGX_HIPCHK(hipGetLastError());
    // the library's own step, exactly as a caller of mgx_step gets it; virtual envs of deselected
    // envs hold no state and are masked out
    const int rc = mgx_step(m, &vs, nullptr, cnt * C, io->nsub, mask ? w.vmask : nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fd_diff<T>, dim3(cnt), dim3(256), 0, st, M, w, e0, C, K, centered, eps, mask);
    MGX_HIPCHK(hipGetLastError());
  }
  return MGX_OK;
}

struct SensFdDims { FdDims d; int max_ncon, nsd; };

// Dimensions, and what mgx_forward / mgx_sensor would refuse, before anything is launched
int sens_fd_dims(const mgx_model* m, SensFdDims* sd) {
  int rc = fd_dims(m, &sd->d);
  if (rc) return rc;
  if (!m->sensor) return host_fail(MGX_E_ARG, "mgx_sensor_configure has not been called for this model");
  if (m->sensor->unsupported) return host_fail(MGX_E_UNSUPPORTED, m->sensor->why);
  mgx_model_info info;
  rc = mgx_model_get_info(m, &info);
  if (rc) return rc;
  sd->max_ncon = info.max_ncon;
  sd->nsd = m->sensor->nsensordata;
  if (sd->nsd > 0 && m->sensor->need_acc) {
    if (m->wide) return host_fail(MGX_E_UNSUPPORTED, std::string("mgx_forward: ") + MGX_WIDE_MSG);
    if ((m->precision == MGX_F32 ? m->mf.cone : m->md.cone) != 0)
      return host_fail(MGX_E_UNSUPPORTED, "mgx_forward decodes pyramidal cones only");
  }
  return MGX_OK;
}

SensFdLayout sens_layout_of(const SensFdDims& sd, int slots) {
  const FdDims& d = sd.d;
  return sens_fd_layout(d.nq, d.nv, d.nu, d.nbody, d.real_bytes, d.scratch, sd.max_ncon, sd.nsd, slots);
}

template <typename T>
int run_sensor_fd(const mgx_model* m, const DevModel<T>& M, const SensFdDims& sd, const mgx_state* s,
                  const mgx_sensor_fd_io* io, int n_env, const uint8_t* mask, hipStream_t st) {
  const FdDims& d = sd.d;
  // the ctrl columns are the last ones: without D the expand kernel stops before them
  const int K = 2 * d.nv + (io->D ? d.nu : 0), centered = io->flags & MGX_FD_CENTERED ? 1 : 0, C = 1 + (centered ? 2 : 1) * K;
  const SensFdLayout L = sens_layout_of(sd, io->slots);
  const FdLayout& o = L.fd;
  char* ws = (char*)io->workspace;
  FdBuf<T> w{(T*)(ws + o.qpos), (T*)(ws + o.qvel), (T*)(ws + o.qacc), (T*)(ws + o.ctrl), (T*)(ws + o.qfrc),
             (T*)(ws + o.xfrc), (T*)(ws + o.time), (T*)(ws + o.step), (int32_t*)(ws + o.warning),
             (int32_t*)(ws + o.overflow), (uint8_t*)(ws + o.vmask), nullptr, nullptr, nullptr, nullptr, nullptr};
  mgx_state vs{};
  vs.qpos = w.qpos; vs.qvel = w.qvel; vs.qacc_warmstart = w.qacc; vs.ctrl = w.ctrl; vs.qfrc_applied = w.qfrc;
  vs.xfrc_applied = w.xfrc; vs.time = w.time; vs.warning = w.warning; vs.overflow = w.overflow;
  vs.scratch = d.scratch ? ws + o.scratch : nullptr;
  mgx_forward_out fo{};
  fo.qacc = ws + L.f_qacc; fo.qfrc_constraint = ws + L.f_qfrc; fo.ncon = (int32_t*)(ws + L.f_ncon);
  fo.con_geom = (int32_t*)(ws + L.f_geom); fo.con_dist = ws + L.f_dist; fo.con_pos = ws + L.f_pos;
  fo.con_frame = ws + L.f_frame; fo.con_force = ws + L.f_force;
  const bool need_fwd = m->sensor->need_acc;
  SensFdBuf<T> b{(const T*)(ws + L.sens), w.step, (T*)io->C, (T*)io->D, (T*)io->sensordata, sd.nsd, d.nv, d.nu};
  const int per = io->slots / C;  // envs per pass
  const T eps = (T)io->eps;
  for (int e0 = 0; e0 < n_env; e0 += per) {
    const int cnt = n_env - e0 < per ? n_env - e0 : per;
    hipLaunchKernelGGL(k_fd_expand<T>, dim3(cnt * C), dim3(64), 0, st, M, *s, w, e0, C, K, centered, eps, mask);
    MGX_HIPCHK(hipGetLastError());
    // the library's own forward pass and sensor kernel, exactly as a caller of mgx_forward and
    // mgx_sensor gets them; virtual envs of deselected envs hold no state and are masked out
    const uint8_t* vmask = mask ? w.vmask : nullptr;
    int rc;
    if (need_fwd) {
      rc = mgx_forward(m, &vs, &fo, cnt * C, vmask, st);
      if (rc) return rc;
    }
    rc = mgx_sensor(m, &vs, need_fwd ? &fo : nullptr, ws + L.sens, cnt * C, vmask, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sens_diff<T>, dim3(cnt, K > 0 ? (K + MGX_FD_TILE - 1) / MGX_FD_TILE : 1), dim3(256), 0, st, b, e0, C, K, centered,
                       eps, mask);
    MGX_HIPCHK(hipGetLastError());
  }
  return MGX_OK;
}

}  // namespace

extern "C" {

int64_t mgx_sensor_fd_bytes(const mgx_model* m, int slots) {
  if (!m || slots < 1) return host_fail(MGX_E_ARG, "null model or slots < 1");
  SensFdDims sd;
  const int rc = sens_fd_dims(m, &sd);
  if (rc) return rc;
  return (int64_t)sens_layout_of(sd, slots).bytes;
}

int mgx_sensor_fd(const mgx_model* m, const mgx_state* s, const mgx_sensor_fd_io* io, int n_env, const uint8_t* env_mask,
                  void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (io->flags & ~MGX_FD_CENTERED) return host_fail(MGX_E_ARG, "unknown mgx_sensor_fd_io.flags bits");
  if (!(io->eps > 0)) return host_fail(MGX_E_ARG, "eps must be > 0");
  SensFdDims sd;
  rc = sens_fd_dims(m, &sd);
  if (rc) return rc;
  if (sd.nsd == 0) return MGX_OK;  // a model without sensors: nothing to launch
  const FdDims& d = sd.d;
  const int K = 2 * d.nv + (io->D ? d.nu : 0), C = 1 + (io->flags & MGX_FD_CENTERED ? 2 : 1) * K;
  if (io->slots < C)
    return host_fail(MGX_E_ARG, "slots below the virtual envs of one env (1 + K, centred 1 + 2 K; K = 2 nv + nu, without D 2 nv)");
  if (!io->workspace || io->workspace_bytes < sens_layout_of(sd, io->slots).bytes)
    return host_fail(MGX_E_ARG, "workspace smaller than mgx_sensor_fd_bytes");
  if (n_env == 0 || (!io->C && !io->D && !io->sensordata)) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return run_sensor_fd<float>(m, m->mf, sd, s, io, n_env, env_mask, st);
  return run_sensor_fd<double>(m, m->md, sd, s, io, n_env, env_mask, st);
}

int64_t mgx_transition_fd_bytes(const mgx_model* m, int slots) {
  if (!m || slots < 1) return host_fail(MGX_E_ARG, "null model or slots < 1");
  FdDims d;
  const int rc = fd_dims(m, &d);
  if (rc) return rc;
  return (int64_t)fd_layout(d.nq, d.nv, d.nu, d.nbody, d.real_bytes, d.scratch, slots).bytes;
}

int mgx_transition_fd(const mgx_model* m, const mgx_state* s, const mgx_fd_io* io, int n_env, const uint8_t* env_mask,
                      void* stream) {
  if (!m || !io || n_env < 0) return host_fail(MGX_E_ARG, "null argument or n_env < 0");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (io->flags & ~MGX_FD_CENTERED) return host_fail(MGX_E_ARG, "unknown mgx_fd_io.flags bits");
  if (!(io->eps > 0)) return host_fail(MGX_E_ARG, "eps must be > 0");
  if (io->nsub < 1) return host_fail(MGX_E_ARG, "nsub must be >= 1");
  FdDims d;
  rc = fd_dims(m, &d);
  if (rc) return rc;
  const int K = 2 * d.nv + d.nu, C = 1 + (io->flags & MGX_FD_CENTERED ? 2 : 1) * K;
  if (io->slots < C) return host_fail(MGX_E_ARG, "slots below the virtual envs of one env (1 + K, centred 1 + 2 K; K = 2 nv + nu)");
  if (!io->workspace || io->workspace_bytes < fd_layout(d.nq, d.nv, d.nu, d.nbody, d.real_bytes, d.scratch, io->slots).bytes)
    return host_fail(MGX_E_ARG, "workspace smaller than mgx_transition_fd_bytes");
  if (n_env == 0 || (!io->A && !io->B && !io->next_qpos && !io->next_qvel && !io->warning)) return MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) return run_fd<float>(m, m->mf, d, s, io, n_env, env_mask, st);
  return run_fd<double>(m, m->md, d, s, io, n_env, env_mask, st);
}

}  // extern "C"
