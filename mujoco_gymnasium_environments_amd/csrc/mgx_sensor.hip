// mgx_sensor.hip — mj_forward outputs, contact forces and sensors (include/mgx.h "sensors,
// mj_forward and contact forces").
//
// Two kinds of kernel, one wave per env:
//   k_forward<T, GB, NT>  load_state and the stages of forward() (mgx_physics.h) over the step
//                         kernels' LDS layout and scratch, in k_debug_forward's order: the contact
//                         list goes out right after collision (later stages overlay it in some
//                         layouts), qacc / qfrc_constraint and the decoded contact wrenches after
//                         the solve. Nothing is written to mgx_state.
//   k_sensor<T>           a slim Env binding: kinematics / com_crb / velocity_bodies from the
//                         current qpos and qvel, then MuJoCo's mj_rnePostConstraint [ext] from the
//                         forward outputs (cacc by chain walk, cfrc_ext as a gather over the
//                         contact list with lane = body, cfrc_int as a subtree sum), then lane =
//                         sensor, the row staged in LDS and stored coalesced.
// Every sum runs in a fixed order on one lane, so results are bit-reproducible; no atomics.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "mgx_internal.h"
#include "mgx_physics.h"
#include "mgx_ray.h"
#include "mgx_sensor.h"

using namespace mgx;

#define MGX_SENSOR_LDS_LIMIT (64 * 1024)

namespace {

// MJCF sensor elements; the code of a type is its index (mgx_sensor_type_name). The first
// MGX_SENS_NTYPE are the ones k_sensor computes, in the order of the MGX_SENS_* codes.
const char* const kSensorNames[] = {
    "jointpos", "jointvel", "framepos", "framequat", "framelinvel", "frameangvel", "gyro", "velocimeter",
    "magnetometer", "accelerometer", "force", "torque", "touch",
    "rangefinder", "camprojection", "tendonpos", "tendonvel", "actuatorpos", "actuatorvel", "actuatorfrc",
    "jointactuatorfrc", "tendonactuatorfrc", "ballquat", "ballangvel", "jointlimitpos", "jointlimitvel",
    "jointlimitfrc", "tendonlimitpos", "tendonlimitvel", "tendonlimitfrc", "framexaxis", "frameyaxis", "framezaxis",
    "framelinacc", "frameangacc", "subtreecom", "subtreelinvel", "subtreeangmom", "insidesite", "distance", "normal",
    "fromto", "contact", "e_potential", "e_kinetic", "clock", "tactile", "plugin", "user"};
const int kSensorNameCount = (int)(sizeof(kSensorNames) / sizeof(kSensorNames[0]));
const int kSensorDim[MGX_SENS_NTYPE] = {1, 1, 3, 4, 3, 3, 3, 3, 3, 3, 3, 3, 1};

// ------------------------------------------------------------------------- forward
template <typename T, bool GB, bool NT>
__global__ void __launch_bounds__(64) k_forward(DevModel<T> m, mgx_state s, FwdBuf<T> o, int n_env,
                                                const uint8_t* mask) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int env = blockIdx.x;
  if (env >= n_env) return;
  if (mask && !mask[env]) return;
  Env<T> e;
  env_bind<T, GB>(m, e, smem, GB ? (T*)s.scratch + (size_t)env * m.L.gB_stride : nullptr);
  load_state(m, e, (T*)s.qpos, (T*)s.qvel, (T*)s.qacc_warmstart, (T*)s.ctrl, (T*)s.qfrc_applied,
             (T*)s.xfrc_applied, (T*)s.time, env);
  const int l = lane_id(), C = m.L.max_ncon;
  kinematics(m, e);
  com_crb(m, e);
  e.diaginv = factor_ld(m, e, e.qLD);
  velocity(m, e);
  e.qacc_smooth = solve_M(m, e, e.qLD, e.diaginv, e.qfrc_smooth);
  collision(m, e);
  // the contact list before make_constraint: with rows in global scratch its points and frames
  // overlay phase-A arrays or share LDS with the Newton Hessian (make_layout)
  for (int c = l; c < C; c += 64) {
    const bool on = c < e.ncon;
    const size_t at = (size_t)env * C + c;
    if (o.con_geom) {
      o.con_geom[2 * at] = on ? e.con_geom[2 * c] : -1;
      o.con_geom[2 * at + 1] = on ? e.con_geom[2 * c + 1] : -1;
    }
    if (o.con_dist) o.con_dist[at] = on ? e.con_dist[c] : (T)0;
    if (o.con_pos)
      for (int k = 0; k < 3; k++) o.con_pos[3 * at + k] = on ? e.con_pos[3 * c + k] : (T)0;
    if (o.con_frame)
      for (int k = 0; k < 9; k++) o.con_frame[9 * at + k] = on ? e.con_frame[9 * c + k] : (T)0;
  }
  if (l == 0 && o.ncon) o.ncon[env] = e.ncon;
  wsync();
  make_constraint(m, e);
  if (l < m.nv) e.vec0[l] = sqrt(e.diaginv);
  wsync();
  transform_rows(m, e);
  if constexpr (NT) newton(m, e);
  else pgs(m, e);
  wsync();
  if (l < m.nv) {
    if (o.qacc) o.qacc[(size_t)env * m.nv + l] = e.qacc;
    if (o.qfrc_constraint) o.qfrc_constraint[(size_t)env * m.nv + l] = e.qfrc_constraint;
  }
  if (!o.con_force) return;
  // mj_contactForce: limit rows come first, then each contact's rows in contact order; the rows
  // end at the first contact that did not fit (contact_rows_share)
  int nlim = 0;
  for (int rb = 0; rb < e.nefc; rb += 64) {
    const int r = rb + l;
    nlim += popc64(ballot(r < e.nefc && e.efc_type[r] == C_LIMIT_JOINT));
  }
  int row0 = nlim;
  for (int cb = 0; cb < C; cb += 64) {
    const int c = cb + l;
    int nr = 0, dim = 0, p = 0;
    if (c < e.ncon) {
      p = e.con_pair[c];
      dim = m.pair_condim[p];
      nr = dim == 1 ? 1 : 2 * (dim - 1);
    }
    int bt;
    const int r0 = row0 + wave_excl_scan(nr, &bt);
    T f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0;
    if (nr > 0 && r0 + nr <= e.nefc && e.efc_id[r0] == c && e.efc_type[r0] != C_LIMIT_JOINT) {
      if (dim == 1) {
        f0 = e.efc[8 * r0 + 1];
      } else {
        const T* mu = m.pair_friction + 5 * p;
#define MGX_EDGE(K, F)                                                 \
  if (K < dim) {                                                       \
    const T a = e.efc[8 * (r0 + 2 * (K - 1)) + 1], b = e.efc[8 * (r0 + 2 * (K - 1) + 1) + 1]; \
    f0 += a;                                                           \
    f0 += b;                                                           \
    F = (a - b) * mu[K - 1];                                           \
  }
        MGX_EDGE(1, f1) MGX_EDGE(2, f2) MGX_EDGE(3, f3) MGX_EDGE(4, f4) MGX_EDGE(5, f5)
#undef MGX_EDGE
      }
    }
    if (c < C) {
      T* dst = o.con_force + 6 * ((size_t)env * C + c);
      dst[0] = f0; dst[1] = f1; dst[2] = f2; dst[3] = f3; dst[4] = f4; dst[5] = f5;
    }
    row0 += bt;
  }
}

// ------------------------------------------------------------------------- sensors
// world position of a body, xbody or geom object of a frame sensor; returns its body (sites read
// the frames staged in LDS)
template <typename T>
__device__ __forceinline__ int obj_pos(const DevModel<T>& m, const Env<T>& e, int ot, int id, T* p) {
  if (ot == MGX_OBJ_BODY) {
    for (int k = 0; k < 3; k++) p[k] = e.xipos[3 * id + k];
    return id;
  }
  if (ot == MGX_OBJ_XBODY) {
    for (int k = 0; k < 3; k++) p[k] = e.xpos[3 * id + k];
    return id;
  }
  const int b = m.geom_bodyid[id];
  mulmatvec3(p, e.xmat + 9 * b, m.geom_pos + 3 * id);
  for (int k = 0; k < 3; k++) p[k] += e.xpos[3 * b + k];
  return b;
}
// world orientation of a body, xbody or geom object
template <typename T>
__device__ __forceinline__ void obj_quat(const DevModel<T>& m, const Env<T>& e, int ot, int id, T* q) {
  if (ot == MGX_OBJ_XBODY) {
    for (int k = 0; k < 4; k++) q[k] = e.xquat[4 * id + k];
  } else if (ot == MGX_OBJ_BODY) {
    mulquat(q, e.xquat + 4 * id, m.body_iquat + 4 * id);
  } else {
    mulquat(q, e.xquat + 4 * m.geom_bodyid[id], m.geom_quat + 4 * id);
  }
}

template <typename T>
__global__ void __launch_bounds__(64) k_sensor(DevModel<T> m, SensorTab<T> t, const T* gqpos, const T* gqvel,
                                               const T* gctrl, const T* gxfrc, FwdBuf<T> f, T* out,
                                               const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // the row stays untouched
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* R = reinterpret_cast<T*>(smem);
  const int nb = m.nbody, nj = m.njnt, nv = m.nv, l = lane_id(), C = m.L.max_ncon;
  Env<T> e;  // slim binding: only what kinematics / com_crb / velocity_bodies read or write
  int o = 0;
  auto take = [&](int n) { T* r = R + o; o += n; return r; };
  e.qpos = take(m.nq); e.qvel = take(nv); e.ctrl = take(m.nu); e.act_force = take(m.nu);
  e.xpos = take(3 * nb); e.xquat = take(4 * nb); e.xmat = take(9 * nb); e.xipos = take(3 * nb);
  e.ximat = take(9 * nb); e.subtree_com = take(3 * nb); e.cinert = take(10 * nb); e.crb = take(10 * nb);
  e.cvel = take(6 * nb); e.cfrc = take(6 * nb); e.xaxis = take(3 * nj); e.xanchor = take(3 * nj);
  e.cdof = take(6 * nv); e.cdof_dot = take(6 * nv); e.qLD = take(m.nM); e.qMH = take(m.nM);
  T* qacc = take(nv);
  T* cacc = take(6 * nb);
  T* cext = take(6 * nb);
  T* cint = take(6 * nb);
  T* sd = take(t.nsensordata);
  T* site_xpos = take(3 * t.nsite);
  T* site_xquat = take(4 * t.nsite);
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = gqpos[(size_t)env * m.nq + k];
  for (int k = l; k < nv; k += 64) e.qvel[k] = gqvel[(size_t)env * nv + k];
  for (int k = l; k < m.nu; k += 64) e.ctrl[k] = gctrl[(size_t)env * m.nu + k];
  if (t.need_acc)
    for (int k = l; k < nv; k += 64) qacc[k] = f.qacc[(size_t)env * nv + k];
  wsync();
  if (t.need_kin) {
    kinematics(m, e);  // m.L.late_geom == 1 (set by the launcher): no geom poses
    // site frames: the body frame composed with site_pos / site_quat (lane = site)
    for (int s = l; s < t.nsite; s += 64) {
      const int b = t.site_bodyid[s];
      T sp[3], sq[4];
      mulmatvec3(sp, e.xmat + 9 * b, t.site_pos + 3 * s);
      mulquat(sq, e.xquat + 4 * b, t.site_quat + 4 * s);
      for (int k = 0; k < 3; k++) site_xpos[3 * s + k] = sp[k] + e.xpos[3 * b + k];
      for (int k = 0; k < 4; k++) site_xquat[4 * s + k] = sq[k];
    }
    wsync();
  }
  if (t.need_vel) {
    com_crb(m, e);
    velocity_bodies(m, e);
  }
  if (t.need_acc) {
    // ---- mj_rnePostConstraint [ext]
    int ncon = f.ncon[env];
    ncon = ncon < 0 ? 0 : (ncon > C ? C : ncon);
    const int* cg = f.con_geom + 2 * (size_t)env * C;
    const T* cpos = f.con_pos + 3 * (size_t)env * C;
    const T* cfr = f.con_frame + 9 * (size_t)env * C;
    const T* cfo = f.con_force + 6 * (size_t)env * C;
    for (int b = l; b < nb; b += 64) {
      // cacc: the chain walk of velocity_bodies, with the qacc terms
      T a[6] = {0, 0, 0, -m.gravity[0], -m.gravity[1], -m.gravity[2]};
      const int depth = m.body_depth[b];
      for (int c = 0; c < depth; c++) {
        const int i = m.body_chain[b * MGX_MAX_DEPTH + c];
        const int bda = m.body_dofadr[i], nd = m.body_dofnum[i];
        for (int j = 0; j < nd; j++)
          for (int k = 0; k < 6; k++) a[k] += e.cdof_dot[6 * (bda + j) + k] * e.qvel[bda + j];
        for (int j = 0; j < nd; j++)
          for (int k = 0; k < 6; k++) a[k] += e.cdof[6 * (bda + j) + k] * qacc[bda + j];
      }
      for (int k = 0; k < 6; k++) cacc[6 * b + k] = a[k];
      // the body's own cinert cacc + cvel x* (cinert cvel)
      T fb[6], tmp[6], tmp1[6];
      mulinertvec(fb, e.cinert + 10 * b, a);
      mulinertvec(tmp, e.cinert + 10 * b, e.cvel + 6 * b);
      crossforce(tmp1, e.cvel + 6 * b, tmp);
      for (int k = 0; k < 6; k++) e.cfrc[6 * b + k] = fb[k] + tmp1[k];
      // cfrc_ext (torque, force) about subtree_com[root]: xfrc_applied, then the contacts of
      // this body in contact order (a gather: one lane sums one body)
      const T* com = e.subtree_com + 3 * m.body_rootid[b];
      T x[6] = {0, 0, 0, 0, 0, 0};
      if (b > 0) {
        const T* xf = gxfrc + ((size_t)env * nb + b) * 6;  // (force, torque) at xipos
        if (xf[0] != 0 || xf[1] != 0 || xf[2] != 0 || xf[3] != 0 || xf[4] != 0 || xf[5] != 0) {
          const T dif[3] = {com[0] - e.xipos[3 * b], com[1] - e.xipos[3 * b + 1], com[2] - e.xipos[3 * b + 2]};
          T cr[3];
          cross3(cr, dif, xf);
          for (int k = 0; k < 3; k++) { x[k] = xf[3 + k] - cr[k]; x[3 + k] = xf[k]; }
        }
      }
      for (int c = 0; c < ncon; c++) {
        const int g1 = cg[2 * c], g2 = cg[2 * c + 1];
        if ((unsigned)g1 >= (unsigned)m.ngeom || (unsigned)g2 >= (unsigned)m.ngeom) continue;
        const int b1 = m.geom_bodyid[g1], b2 = m.geom_bodyid[g2];
        if (b1 != b && b2 != b) continue;
        T wf[3], wt[3], cr[3];
        mulmatTvec3(wf, cfr + 9 * c, cfo + 6 * c);
        mulmatTvec3(wt, cfr + 9 * c, cfo + 6 * c + 3);
        const T dif[3] = {com[0] - cpos[3 * c], com[1] - cpos[3 * c + 1], com[2] - cpos[3 * c + 2]};
        cross3(cr, dif, wf);
        const T sg = (b2 == b ? (T)1 : (T)0) - (b1 == b ? (T)1 : (T)0);
        for (int k = 0; k < 3; k++) { x[k] += sg * (wt[k] - cr[k]); x[3 + k] += sg * wf[k]; }
      }
      for (int k = 0; k < 6; k++) cext[6 * b + k] = x[k];
    }
    wsync();
    // cfrc_int: the DFS-contiguous subtree sum
    for (int b = l; b < nb; b += 64) {
      T acc[6] = {0, 0, 0, 0, 0, 0};
      const int end = m.body_subtree_end[b];
      for (int i = b; i < end; i++)
        for (int k = 0; k < 6; k++) acc[k] += e.cfrc[6 * i + k] - cext[6 * i + k];
      for (int k = 0; k < 6; k++) cint[6 * b + k] = acc[k];
    }
    wsync();
  }
  // ---- lane = sensor
  for (int si = l; si < t.nsensor; si += 64) {
    const int type = t.type[si], ot = t.objtype[si], id = t.objid[si], adr = t.adr[si];
    T v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (type == MGX_SENS_JOINTPOS) {
      v0 = e.qpos[m.jnt_qposadr[id]];
    } else if (type == MGX_SENS_JOINTVEL) {
      v0 = e.qvel[m.jnt_dofadr[id]];
    } else if (type == MGX_SENS_FRAMEQUAT) {
      T q[4];
      if (ot == MGX_OBJ_SITE) { for (int k = 0; k < 4; k++) q[k] = site_xquat[4 * id + k]; }
      else obj_quat(m, e, ot, id, q);
      v0 = q[0]; v1 = q[1]; v2 = q[2]; v3 = q[3];
    } else {
      T p[3], r[3], w[3], v[3], res[3] = {0, 0, 0};
      int b;
      if (ot == MGX_OBJ_SITE) {
        b = t.site_bodyid[id];
        for (int k = 0; k < 3; k++) p[k] = site_xpos[3 * id + k];
      } else {
        b = obj_pos(m, e, ot, id, p);
      }
      const T* com = e.subtree_com + 3 * m.body_rootid[b];
      for (int k = 0; k < 3; k++) r[k] = p[k] - com[k];
      if (type == MGX_SENS_FRAMEPOS) {
        for (int k = 0; k < 3; k++) res[k] = p[k];
      } else if (type == MGX_SENS_FRAMEANGVEL) {
        for (int k = 0; k < 3; k++) res[k] = e.cvel[6 * b + k];
      } else if (type == MGX_SENS_FRAMELINVEL) {
        cross3(v, e.cvel + 6 * b, r);
        for (int k = 0; k < 3; k++) res[k] = e.cvel[6 * b + 3 + k] + v[k];
      } else {
        // site sensors: everything in the site frame
        T Rs[9];
        quat2mat(Rs, site_xquat + 4 * id);
        if (type == MGX_SENS_MAGNETOMETER) {
          const T mag[3] = {t.magnetic0, t.magnetic1, t.magnetic2};
          mulmatTvec3(res, Rs, mag);
        } else if (type == MGX_SENS_GYRO) {
          mulmatTvec3(res, Rs, e.cvel + 6 * b);
        } else if (type == MGX_SENS_VELOCIMETER || type == MGX_SENS_ACCELEROMETER) {
          T wl[3], vl[3];
          cross3(v, e.cvel + 6 * b, r);
          for (int k = 0; k < 3; k++) v[k] += e.cvel[6 * b + 3 + k];
          mulmatTvec3(vl, Rs, v);
          if (type == MGX_SENS_VELOCIMETER) {
            for (int k = 0; k < 3; k++) res[k] = vl[k];
          } else {
            // mj_objectAcceleration, local: Rs'(cacc_lin + alpha x r) + w_local x v_local
            T a[3], al[3], cr[3];
            cross3(a, cacc + 6 * b, r);
            for (int k = 0; k < 3; k++) a[k] += cacc[6 * b + 3 + k];
            mulmatTvec3(al, Rs, a);
            mulmatTvec3(wl, Rs, e.cvel + 6 * b);
            cross3(cr, wl, vl);
            for (int k = 0; k < 3; k++) res[k] = al[k] + cr[k];
          }
        } else if (type == MGX_SENS_FORCE) {
          mulmatTvec3(res, Rs, cint + 6 * b + 3);
        } else if (type == MGX_SENS_TORQUE) {
          T cr[3];
          cross3(cr, r, cint + 6 * b + 3);
          for (int k = 0; k < 3; k++) w[k] = cint[6 * b + k] - cr[k];
          mulmatTvec3(res, Rs, w);
        } else if (type == MGX_SENS_TOUCH) {
          // mj_sensorAcc's rule: a contact of the site's body counts when the ray from its point
          // along its normal (towards the body) meets the site's shape
          int ncon = f.ncon[env];
          ncon = ncon < 0 ? 0 : (ncon > C ? C : ncon);
          const int* cg = f.con_geom + 2 * (size_t)env * C;
          const T* cpos = f.con_pos + 3 * (size_t)env * C;
          const T* cfr = f.con_frame + 9 * (size_t)env * C;
          const T* cfo = f.con_force + 6 * (size_t)env * C;
          const int st = t.site_type[id];
          T sum = 0;
          for (int c = 0; c < ncon; c++) {
            const int g1 = cg[2 * c], g2 = cg[2 * c + 1];
            if ((unsigned)g1 >= (unsigned)m.ngeom || (unsigned)g2 >= (unsigned)m.ngeom) continue;
            const int b1 = m.geom_bodyid[g1], b2 = m.geom_bodyid[g2];
            if (b1 != b && b2 != b) continue;
            const T fn = cfo[6 * c];
            if (!(fn > 0)) continue;
            const T sg = b2 == b ? (T)-1 : (T)1;
            const T d[3] = {cpos[3 * c] - p[0], cpos[3 * c + 1] - p[1], cpos[3 * c + 2] - p[2]};
            const T n[3] = {sg * cfr[9 * c], sg * cfr[9 * c + 1], sg * cfr[9 * c + 2]};
            T lp[3], lv[3];
            mulmatTvec3(lp, Rs, d);
            mulmatTvec3(lv, Rs, n);
            if (ray_geom(st, t.site_size + 3 * id, lp, lv) < ray_inf<T>()) sum += fn;
          }
          res[0] = sum;
        }
      }
      v0 = res[0]; v1 = res[1]; v2 = res[2];
    }
    const T cut = t.cutoff[si];
    if (cut > 0 && type != MGX_SENS_FRAMEQUAT) {
      const T lo = type == MGX_SENS_TOUCH ? (T)0 : -cut;
      v0 = clampv(v0, lo, cut); v1 = clampv(v1, lo, cut); v2 = clampv(v2, lo, cut);
    }
    const int dim = t.dim[si];
    sd[adr] = v0;
    if (dim > 1) { sd[adr + 1] = v1; sd[adr + 2] = v2; }
    if (dim > 3) sd[adr + 3] = v3;
  }
  wsync();
  for (int k = l; k < t.nsensordata; k += 64) out[(size_t)env * t.nsensordata + k] = sd[k];
}

// ------------------------------------------------------------------------- host side
template <typename T, bool GB>
void launch_forward_v(const mgx_model* m, const DevModel<T>& M, const mgx_state* s, const FwdBuf<T>& o, int n_env,
                      const uint8_t* mask, hipStream_t st) {
  if (M.solver == 2)
    hipLaunchKernelGGL((k_forward<T, GB, true>), dim3(n_env), dim3(64), m->L.bytes, st, M, *s, o, n_env, mask);
  else
    hipLaunchKernelGGL((k_forward<T, GB, false>), dim3(n_env), dim3(64), m->L.bytes, st, M, *s, o, n_env, mask);
}

template <typename T>
FwdBuf<T> fwd_buf(const mgx_forward_out* o) {
  return FwdBuf<T>{(T*)o->qacc, (T*)o->qfrc_constraint, o->ncon, o->con_geom,
                   (T*)o->con_dist, (T*)o->con_pos, (T*)o->con_frame, (T*)o->con_force};
}

template <typename T>
int set_forward_lds(int bytes) {
  return mgx_set_lds(k_forward<T, false, false>, bytes) | mgx_set_lds(k_forward<T, false, true>, bytes) |
         mgx_set_lds(k_forward<T, true, false>, bytes) | mgx_set_lds(k_forward<T, true, true>, bytes);
}

template <typename T>
void upload_tabs(std::vector<char>& host, const mgx_sensor_desc* d, SensorTab<T>& t,
                 std::vector<std::pair<size_t, const void**>>& fix) {
  auto add = [&](const void* src, size_t bytes, const void** slot) {
    size_t off = (host.size() + 15) / 16 * 16;
    host.resize(off + (bytes ? bytes : 16));
    if (bytes) memcpy(host.data() + off, src, bytes);
    fix.push_back({off, slot});
  };
  auto reals = [&](const double* src, size_t n, const T** slot) {
    std::vector<T> v(n ? n : 1, (T)0);
    for (size_t i = 0; i < n; i++) v[i] = (T)src[i];
    add(v.data(), v.size() * sizeof(T), (const void**)slot);
  };
  const size_t ns = d->nsite, nn = d->nsensor;
  add(d->site_bodyid, 4 * ns, (const void**)&t.site_bodyid);
  add(d->site_type, 4 * ns, (const void**)&t.site_type);
  reals(d->site_pos, 3 * ns, &t.site_pos); reals(d->site_quat, 4 * ns, &t.site_quat);
  reals(d->site_size, 3 * ns, &t.site_size);
  add(d->sensor_type, 4 * nn, (const void**)&t.type);
  add(d->sensor_objtype, 4 * nn, (const void**)&t.objtype);
  add(d->sensor_objid, 4 * nn, (const void**)&t.objid);
  add(d->sensor_dim, 4 * nn, (const void**)&t.dim);
  add(d->sensor_adr, 4 * nn, (const void**)&t.adr);
  reals(d->sensor_cutoff, nn, &t.cutoff);
  t.magnetic0 = (T)d->magnetic[0]; t.magnetic1 = (T)d->magnetic[1]; t.magnetic2 = (T)d->magnetic[2];
}

int sensor_ready(const mgx_model* m) {
  if (!m) return host_fail(MGX_E_ARG, "null model");
  if (!m->sensor) return host_fail(MGX_E_ARG, "mgx_sensor_configure has not been called for this model");
  if (m->sensor->unsupported) return host_fail(MGX_E_UNSUPPORTED, m->sensor->why);
  return MGX_OK;
}

const char* obj_name(int ot) {
  static const char* const n[] = {"body", "xbody", "joint", "geom", "site"};
  return ot >= 0 && ot < 5 ? n[ot] : "other";
}

}  // namespace

namespace mgx {
void sensor_release(mgx_model* m) {
  if (!m || !m->sensor) return;
  if (m->sensor->dbuf) (void)hipFree(m->sensor->dbuf);
  delete m->sensor;
  m->sensor = nullptr;
}

// dynamic-LDS attributes of the forward kernels (called by mgx_model_create)
int forward_kernels_configure(const mgx_model* m) {
  if (m->wide) return MGX_OK;
  return m->precision == MGX_F32 ? set_forward_lds<float>(m->L.bytes) : set_forward_lds<double>(m->L.bytes);
}
}  // namespace mgx

extern "C" {

const char* mgx_sensor_type_name(int code) { return code >= 0 && code < kSensorNameCount ? kSensorNames[code] : nullptr; }

int mgx_sensor_configure(mgx_model* m, const mgx_sensor_desc* d) {
  if (!m || !d) return host_fail(MGX_E_ARG, "null argument");
  const bool f32 = m->precision == MGX_F32;
  const int nb = f32 ? m->mf.nbody : m->md.nbody, nj = f32 ? m->mf.njnt : m->md.njnt;
  const int ng = f32 ? m->mf.ngeom : m->md.ngeom, nq = f32 ? m->mf.nq : m->md.nq, nv = f32 ? m->mf.nv : m->md.nv;
  const int nu = f32 ? m->mf.nu : m->md.nu, nM = f32 ? m->mf.nM : m->md.nM;
  if (d->nsite < 0 || d->nsensor < 0 || d->nsensordata < 0) return host_fail(MGX_E_ARG, "negative count");
  if (d->nsite > 0 && (!d->site_bodyid || !d->site_type || !d->site_pos || !d->site_quat || !d->site_size))
    return host_fail(MGX_E_ARG, "null site table");
  if (d->nsensor > 0 && (!d->sensor_type || !d->sensor_objtype || !d->sensor_objid || !d->sensor_reftype ||
                         !d->sensor_dim || !d->sensor_adr || !d->sensor_cutoff))
    return host_fail(MGX_E_ARG, "null sensor table");
  for (int i = 0; i < d->nsite; i++)
    if (d->site_bodyid[i] < 0 || d->site_bodyid[i] >= nb) return host_fail(MGX_E_ARG, "site_bodyid out of range");
  sensor_release(m);
  SensorState* ss = new SensorState();
  m->sensor = ss;
  auto refuse = [&](const std::string& why) {
    ss->unsupported = true;
    ss->why = why;
    return sensor_ready(m);
  };
  auto bad = [&](const char* why) {
    sensor_release(m);
    return host_fail(MGX_E_ARG, why);
  };
  // joint types (the model keeps its tables on the device only)
  MGX_HIPCHK(hipSetDevice(m->device));
  std::vector<int> jt(nj > 0 ? nj : 1, 0);
  if (nj > 0 && d->nsensor > 0)
    MGX_HIPCHK(hipMemcpy(jt.data(), f32 ? m->mf.jnt_type : m->md.jnt_type, 4 * (size_t)nj, hipMemcpyDeviceToHost));
  int adr = 0;
  bool kin = false, vel = false, acc = false;
  for (int i = 0; i < d->nsensor; i++) {
    const int type = d->sensor_type[i], ot = d->sensor_objtype[i], id = d->sensor_objid[i];
    const char* name = mgx_sensor_type_name(type);
    if (type < 0 || !name) return bad("sensor_type is not a code of mgx_sensor_type_name");
    if (type >= MGX_SENS_NTYPE) return refuse(std::string("sensor type '") + name + "' is not supported");
    if (d->sensor_reftype[i] >= 0)
      return refuse(std::string("sensor type '") + name + "' with a reftype / refname frame is not supported");
    if (d->sensor_dim[i] != kSensorDim[type] || d->sensor_adr[i] != adr) return bad("sensor_dim / sensor_adr mismatch");
    adr += d->sensor_dim[i];
    if (type == MGX_SENS_JOINTPOS || type == MGX_SENS_JOINTVEL) {
      if (ot != MGX_OBJ_JOINT || id < 0 || id >= nj) return bad("jointpos / jointvel: joint id out of range");
      if (jt[id] != JHINGE && jt[id] != JSLIDE) return bad("jointpos / jointvel need a hinge or slide joint");
    } else if (type >= MGX_SENS_FRAMEPOS && type <= MGX_SENS_FRAMEANGVEL) {
      const int n = ot == MGX_OBJ_BODY || ot == MGX_OBJ_XBODY ? nb : ot == MGX_OBJ_GEOM ? ng : ot == MGX_OBJ_SITE ? d->nsite : -1;
      if (n < 0)
        return refuse(std::string("sensor type '") + name + "' on a " + obj_name(ot) + " object is not supported");
      if (id < 0 || id >= n) return bad("frame sensor: object id out of range");
      kin = true;
      vel = vel || type >= MGX_SENS_FRAMELINVEL;
    } else {
      if (ot != MGX_OBJ_SITE || id < 0 || id >= d->nsite) return bad("site sensor: site id out of range");
      kin = true;
      vel = vel || type != MGX_SENS_MAGNETOMETER;
      acc = acc || type >= MGX_SENS_ACCELEROMETER;
      if (type == MGX_SENS_TOUCH) {
        const int st = d->site_type[id];
        if (st != GSPHERE && st != GCAPSULE && st != GCYLINDER && st != GBOX)
          return refuse("sensor type 'touch' on an ellipsoid site is not supported");
      }
    }
  }
  if (adr != d->nsensordata) return bad("nsensordata differs from the sum of sensor_dim");
  if (d->nsensordata > 0 && m->wide) return refuse(std::string("sensors: ") + MGX_WIDE_MSG);
  ss->nsensordata = d->nsensordata;
  ss->need_acc = acc;
  ss->lds_bytes = sensor_lds_reals(nq, nv, nu, nb, nj, nM, d->nsensordata, d->nsite) * (f32 ? 4 : 8);
  if (d->nsensordata == 0) return MGX_OK;
  if (ss->lds_bytes > MGX_SENSOR_LDS_LIMIT) {
    sensor_release(m);
    return host_fail(MGX_E_CAPACITY, "model too large for the sensor kernel's LDS");
  }
  std::vector<char> host;
  std::vector<std::pair<size_t, const void**>> fix;
  if (f32) upload_tabs<float>(host, d, ss->tf, fix);
  else upload_tabs<double>(host, d, ss->td, fix);
  hipError_t err = hipMalloc(&ss->dbuf, host.size());
  if (err == hipSuccess) err = hipMemcpy(ss->dbuf, host.data(), host.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    sensor_release(m);
    return host_fail(MGX_E_HIP, std::string("mgx_sensor_configure: ") + hipGetErrorString(err));
  }
  for (auto& fx : fix) *fx.second = (char*)ss->dbuf + fx.first;
  // stages: velocity needs com (and so kinematics); acceleration needs both
  auto fill = [&](auto& t) {
    t.nsite = d->nsite; t.nsensor = d->nsensor; t.nsensordata = d->nsensordata;
    t.need_acc = acc; t.need_vel = vel || acc; t.need_kin = kin || vel || acc;
  };
  if (f32) fill(ss->tf);
  else fill(ss->td);
  return MGX_OK;
}

int mgx_forward(const mgx_model* m, const mgx_state* s, const mgx_forward_out* out, int n_env, const uint8_t* env_mask,
                void* stream) {
  if (!m || !out || n_env < 0) return host_fail(MGX_E_ARG, "bad argument");
  if (m->wide) return host_fail(MGX_E_UNSUPPORTED, std::string("mgx_forward: ") + MGX_WIDE_MSG);
  if ((m->precision == MGX_F32 ? m->mf.cone : m->md.cone) != 0)
    return host_fail(MGX_E_UNSUPPORTED, "mgx_forward decodes pyramidal cones only");
  int rc = host_check_state(s);
  if (rc) return rc;
  if (n_env == 0) return MGX_OK;
  rc = host_check_scratch(m, s);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) {
    if (m->L.gB) launch_forward_v<float, true>(m, m->mf, s, fwd_buf<float>(out), n_env, env_mask, st);
    else launch_forward_v<float, false>(m, m->mf, s, fwd_buf<float>(out), n_env, env_mask, st);
  } else {
    if (m->L.gB) launch_forward_v<double, true>(m, m->md, s, fwd_buf<double>(out), n_env, env_mask, st);
    else launch_forward_v<double, false>(m, m->md, s, fwd_buf<double>(out), n_env, env_mask, st);
  }
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

int mgx_sensor(const mgx_model* m, const mgx_state* s, const mgx_forward_out* fwd, void* sensordata, int n_env,
               const uint8_t* env_mask, void* stream) {
  int rc = sensor_ready(m);
  if (rc != MGX_OK) return rc;
  const SensorState& ss = *m->sensor;
  if (ss.nsensordata == 0 || n_env == 0) return MGX_OK;
  if (n_env < 0 || !sensordata) return host_fail(MGX_E_ARG, "null sensordata or n_env < 0");
  rc = host_check_state(s);
  if (rc) return rc;
  mgx_forward_out none{};
  if (ss.need_acc) {
    if (!fwd || !fwd->qacc || !fwd->ncon || !fwd->con_geom || !fwd->con_pos || !fwd->con_frame || !fwd->con_force)
      return host_fail(MGX_E_ARG, "this model's sensors need mgx_forward's qacc, ncon, con_geom, con_pos, con_frame "
                                  "and con_force");
  } else {
    fwd = &none;  // never read
  }
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) {
    DevModel<float> M = m->mf;
    M.L.late_geom = 1;
    hipLaunchKernelGGL(k_sensor<float>, dim3(n_env), dim3(64), ss.lds_bytes, st, M, ss.tf, (const float*)s->qpos,
                       (const float*)s->qvel, (const float*)s->ctrl, (const float*)s->xfrc_applied,
                       fwd_buf<float>(fwd), (float*)sensordata, env_mask);
  } else {
    DevModel<double> M = m->md;
    M.L.late_geom = 1;
    hipLaunchKernelGGL(k_sensor<double>, dim3(n_env), dim3(64), ss.lds_bytes, st, M, ss.td, (const double*)s->qpos,
                       (const double*)s->qvel, (const double*)s->ctrl, (const double*)s->xfrc_applied,
                       fwd_buf<double>(fwd), (double*)sensordata, env_mask);
  }
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

}  // extern "C"
