// mgx_ray.h — ray against one primitive geom and against an env's scene (MuJoCo's mj_ray /
// mju_rayGeom semantics [ext], restated in include/mgx.h and DESIGN.md "Ray casting").
//
// A ray is p + x v with x >= 0; v is not normalised, x is in units of |v|. Everything runs in
// the geom frame: lp = R'(p - pos), lv = R'v. The answer for one geom is the smallest x >= 0 over
// the pieces of its surface (side, caps, faces), each accepted only inside its own extent, so a
// ray that starts inside a closed geom finds its exit surface. Arithmetic is in the model's real
// type T.
#pragma once
#include "../../include/mgx.h"
#include "mgx_common.h"
#include "mgx_internal.h"
#include "mgx_physics.h"

namespace mgx {

// Device tables of mgx_ray_configure (reals in the model's type), one allocation.
template <typename T>
struct RayCams {
  int ncam;
  const int *bodyid, *mode;                         // [ncam]
  const T *pos, *quat, *pos0, *poscom0, *mat0;      // [ncam][3|4|3|3|9]
};

// Host side of the model's ray tables (mgx_model.ray).
struct RayState {
  bool unsupported = false;  // the model holds an hfield, mesh or ellipsoid geom
  int ngeom = 0, ncam = 0;
  void* dbuf = nullptr;      // enable flags, then the camera tables
  const uint8_t* enable = nullptr;  // device [ngeom]: 0 = eliminated by default
  struct RenderState* render = nullptr;  // mgx_render_configure (mgx_render.h); freed with the ray tables
  RayCams<float> cf;
  RayCams<double> cd;
  int cam_mode[MGX_RAY_MAX_CAM];
  double cam_fovy[MGX_RAY_MAX_CAM];
};

// One env's scene, in reals: geom_xpos [3 ngeom], geom_xmat [9 ngeom], then per camera its world
// position [3] and orientation [9].
__host__ __device__ inline int ray_scene_reals(int ngeom, int ncam) { return 12 * ngeom + 12 * ncam; }
__host__ __device__ inline int ray_scene_cam(int ngeom, int cam) { return 12 * ngeom + 12 * cam; }

// Staged geom record in LDS (RAY_REC reals): pos [3], mat [9], size [3], rbound [1].
#define MGX_RAY_REC 16
#define MGX_RAY_TILE 256                  // rays (pixels) per workgroup, one per lane
#define MGX_RAY_LDS_LIMIT (64 * 1024)     // LDS of one workgroup of a ray or render kernel

// mgx_ray.hip: MGX_OK when the model's ray tables are configured and its geoms supported
int ray_ready(const mgx_model* m);
// mgx_render.hip: frees the render tables that hang off the ray tables
void render_release(RayState* rs);

// The workgroup's staging of its env's geoms: coalesced reads of the scene's positions and
// matrices and of the size table into rec, and the geom type, or -1 when the geom is not enabled,
// into typ. The caller's barrier follows.
template <typename T>
__device__ __forceinline__ void ray_stage_geoms(T* rec, int* typ, int ngeom, const int* geom_type,
                                                const int* geom_bodyid, const T* geom_size, const T* geom_rbound,
                                                const uint8_t* enable0, const uint8_t* enable1, int bodyexclude,
                                                const T* sc, int tid) {
  for (int k = tid; k < 3 * ngeom; k += MGX_RAY_TILE) {
    const int g = k / 3, j = k - 3 * g;
    rec[MGX_RAY_REC * g + j] = sc[k];
    rec[MGX_RAY_REC * g + 12 + j] = geom_size[k];
  }
  for (int k = tid; k < 9 * ngeom; k += MGX_RAY_TILE) {
    const int g = k / 9, j = k - 9 * g;
    rec[MGX_RAY_REC * g + 3 + j] = sc[3 * ngeom + k];
  }
  for (int g = tid; g < ngeom; g += MGX_RAY_TILE) {
    rec[MGX_RAY_REC * g + 15] = geom_rbound[g];
    const bool on = enable0[g] && (!enable1 || enable1[g]) && geom_bodyid[g] != bodyexclude;
    typ[g] = on ? geom_type[g] : -1;
  }
}

template <typename T> __device__ __forceinline__ T ray_inf() { return (T)__builtin_huge_val(); }

// roots of a x^2 + 2 b x + c = 0, x0 <= x1 (mju ray_quad's guards: a and the discriminant above
// mjMINVAL, so a tangent ray misses)
template <typename T>
__device__ __forceinline__ bool ray_quad(T a, T b, T c, T& x0, T& x1) {
  if (a < minval<T>()) return false;
  T det = b * b - a * c;
  if (det < minval<T>()) return false;
  det = sqrt(det);
  x0 = (-b - det) / a;
  x1 = (-b + det) / a;
  return true;
}
template <typename T>
__device__ __forceinline__ void ray_take(T& best, T x, bool ok) {
  if (ok && x >= 0 && x < best) best = x;
}

// The surface piece whose root won, for callers that shade the hit (mgx_render.h): 0 = plane,
// sphere, or the side of a capsule / cylinder; 1 / 2 = the -z / +z cap; box faces 2 i + (s > 0).
// Ties keep the first piece in the order the pieces are tried. NoPiece records nothing, so the
// distances are those of the same arithmetic either way.
struct NoPiece {
  __device__ __forceinline__ void won(int) {}
};
struct WonPiece {
  int piece = 0;
  __device__ __forceinline__ void won(int k) { piece = k; }
};
template <typename T, typename P>
__device__ __forceinline__ void ray_take(T& best, T x, bool ok, P& rec, int piece) {
  if (ok && x >= 0 && x < best) { best = x; rec.won(piece); }
}

// side of the z-axis cylinder of radius r, |z| <= h (capsule and cylinder)
template <typename T, typename P>
__device__ __forceinline__ void ray_side(T& best, const T* lp, const T* lv, T r, T h, P& rec) {
  T x0, x1;
  if (ray_quad(lv[0] * lv[0] + lv[1] * lv[1], lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - r * r, x0,
               x1)) {
    ray_take(best, x0, fabs(lp[2] + x0 * lv[2]) <= h, rec, 0);
    ray_take(best, x1, fabs(lp[2] + x1 * lv[2]) <= h, rec, 0);
  }
}

// ray against one geom in its frame; returns the hit distance or +inf. `type` is wave-uniform in
// the scene walk, so this switch does not diverge; only hit / miss does.
template <typename T, typename P>
__device__ __forceinline__ T ray_geom(int type, const T* sz, const T* lp, const T* lv, P& rec) {
  T best = ray_inf<T>();
  T x0, x1;
  switch (type) {
    case GPLANE: {
      if (lv[2] < -minval<T>()) {  // front side only
        T x = -lp[2] / lv[2];
        T px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
        ray_take(best, x, (sz[0] <= 0 || fabs(px) <= sz[0]) && (sz[1] <= 0 || fabs(py) <= sz[1]), rec, 0);
      }
      break;
    }
    case GSPHERE: {
      if (ray_quad(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - sz[0] * sz[0], x0, x1)) {
        ray_take(best, x0, true, rec, 0);
        ray_take(best, x1, true, rec, 0);
      }
      break;
    }
    case GCAPSULE: {
      const T r = sz[0], h = sz[1];
      ray_side(best, lp, lv, r, h, rec);
      const T a = dot3(lv, lv);
#pragma unroll
      for (int s = -1; s <= 1; s += 2) {  // cap spheres at z = s h, accepted where s z >= h
        T dz = lp[2] - s * h;
        if (ray_quad(a, lv[0] * lp[0] + lv[1] * lp[1] + lv[2] * dz, lp[0] * lp[0] + lp[1] * lp[1] + dz * dz - r * r, x0,
                     x1)) {
          ray_take(best, x0, s * (lp[2] + x0 * lv[2]) >= h, rec, s < 0 ? 1 : 2);
          ray_take(best, x1, s * (lp[2] + x1 * lv[2]) >= h, rec, s < 0 ? 1 : 2);
        }
      }
      break;
    }
    case GCYLINDER: {
      const T r = sz[0], h = sz[1];
      ray_side(best, lp, lv, r, h, rec);
      if (fabs(lv[2]) > minval<T>()) {
#pragma unroll
        for (int s = -1; s <= 1; s += 2) {  // flat caps at z = s h, accepted inside the disc
          T x = (s * h - lp[2]) / lv[2];
          T px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
          ray_take(best, x, px * px + py * py <= r * r, rec, s < 0 ? 1 : 2);
        }
      }
      break;
    }
    case GBOX: {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        if (fabs(lv[i]) > minval<T>()) {
#pragma unroll
          for (int s = -1; s <= 1; s += 2) {  // face i = s size[i], accepted inside the other two extents
            T x = (s * sz[i] - lp[i]) / lv[i];
            ray_take(best, x, fabs(lp[j] + x * lv[j]) <= sz[j] && fabs(lp[k] + x * lv[k]) <= sz[k], rec,
                     2 * i + (s > 0));
          }
        }
      }
      break;
    }
    default: break;
  }
  return best;
}
template <typename T>
__device__ __forceinline__ T ray_geom(int type, const T* sz, const T* lp, const T* lv) {
  NoPiece none;
  return ray_geom(type, sz, lp, lv, none);
}

// Nearest hit over the staged geoms. rec: MGX_RAY_REC reals per geom, typ: the geom type or -1
// when the geom is not enabled. Every lane walks the same g, so typ[g] and rec reads are
// same-address LDS broadcasts. The bounding-sphere test only skips geoms the ray cannot touch
// (slack well above the rounding of its own terms), so it changes no result; planes have no
// bounding sphere. Ties keep the lower geom id. ray_scene_visit is the walk itself: visit(g, type,
// record, lp, lv) sees every enabled geom the ray can touch, with the ray in that geom's frame, and
// returns false to end the walk for the lanes it says so to (a shadow walk decides that on a ballot).
template <typename T, typename Visit>
__device__ __forceinline__ void ray_scene_visit(const T* rec, const int* typ, int ngeom, const T* p, const T* v,
                                                Visit&& visit) {
  const T eps = sizeof(T) == 4 ? (T)1.2e-7 : (T)2.3e-16;
  const T vv = dot3(v, v);
  for (int g = 0; g < ngeom; g++) {
    const int t = typ[g];
    if (t < 0) continue;
    const T* r = rec + MGX_RAY_REC * g;
    const T d[3] = {p[0] - r[0], p[1] - r[1], p[2] - r[2]};
    if (t != GPLANE) {
      const T dd = dot3(d, d), b = -dot3(d, v), rb = r[15];
      const T lim = rb * rb * (T)1.001 + (T)64 * eps * dd;
      // outside the sphere and heading away, or the line passes it by
      if (dd > lim && (b < 0 || dd * vv - b * b > lim * vv)) continue;
    }
    T lp[3], lv[3];
    mulmatTvec3(lp, r + 3, d);
    mulmatTvec3(lv, r + 3, v);
    if (!visit(g, t, r, lp, lv)) break;
  }
}
template <typename T>
__device__ __forceinline__ void ray_scene_walk(const T* rec, const int* typ, int ngeom, const T* p, const T* v, T& dist,
                                               int& geomid) {
  T best = ray_inf<T>();
  int id = -1;
  ray_scene_visit(rec, typ, ngeom, p, v, [&](int g, int t, const T* r, const T* lp, const T* lv) {
    const T x = ray_geom(t, r + 12, lp, lv);
    if (x < best) { best = x; id = g; }
    return true;
  });
  dist = best;
  geomid = id;
}

// The ray of pixel `ray` (row-major from the top-left) of a height x width image: p the camera
// position, v = R_cam ((2 (c + 1/2) / W - 1) t W / H, (1 - 2 (r + 1/2) / H) t, -1). cp: the camera's
// pose in the scene (position [3], orientation [9]).
template <typename T>
__device__ __forceinline__ void ray_camera_pixel(const T* cp, int height, int width, T t, int ray, T* p, T* v) {
  const int r = ray / width, c = ray - r * width;
  const T vc[3] = {((T)2 * ((T)c + (T)0.5) / (T)width - (T)1) * t * (T)width / (T)height,
                   ((T)1 - (T)2 * ((T)r + (T)0.5) / (T)height) * t, (T)-1};
  for (int k = 0; k < 3; k++) p[k] = cp[k];
  mulmatvec3(v, cp + 3, vc);
}

// reals of LDS the scene kernels bind (the arrays kinematics touches; geom poses go to the scene)
__host__ __device__ inline int scene_lds_reals(int nq, int nbody, int njnt) { return nq + 28 * nbody + 6 * njnt; }

// One env's ray scene, by one wave: kinematics() / geom_poses() from gqpos through a slim Env
// binding in R (scene_lds_reals reals of LDS), geom poses written straight into sc, then lane c
// writes camera c's world pose. e is left bound, with the body frames of this qpos, for a caller
// that places more in them (the lights of mgx_render_scene).
template <typename T>
__device__ __forceinline__ void ray_scene_env(const DevModel<T>& m, const RayCams<T>& rc, const T* gqpos, T* sc, T* R,
                                              Env<T>& e) {
  const int nb = m.nbody, nj = m.njnt, ng = m.ngeom, l = lane_id();
  int o = 0;
  e.qpos = R + o; o += m.nq;
  e.xpos = R + o; o += 3 * nb;
  e.xquat = R + o; o += 4 * nb;
  e.xmat = R + o; o += 9 * nb;
  e.xipos = R + o; o += 3 * nb;
  e.ximat = R + o; o += 9 * nb;
  e.xaxis = R + o; o += 3 * nj;
  e.xanchor = R + o;
  e.geom_xpos = sc;
  e.geom_xmat = sc + 3 * ng;
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = gqpos[k];
  wsync();
  kinematics(m, e);  // m.L.late_geom == 0 (set by the launcher): geom poses included
  for (int c = l; c < rc.ncam; c += 64) {
    const int b = rc.bodyid[c], mode = rc.mode[c];
    T* out = sc + ray_scene_cam(ng, c);
    if (mode == MGX_CAM_FIXED) {
      T p[3], q[4];
      mulmatvec3(p, e.xmat + 9 * b, rc.pos + 3 * c);
      for (int k = 0; k < 3; k++) out[k] = p[k] + e.xpos[3 * b + k];
      mulquat(q, e.xquat + 4 * b, rc.quat + 4 * c);
      quat2mat(out + 3, q);
    } else {
      T base[3] = {e.xpos[3 * b], e.xpos[3 * b + 1], e.xpos[3 * b + 2]};
      const T* off = rc.pos0 + 3 * c;
      if (mode == MGX_CAM_TRACKCOM) {
        // mj_comPos for this one body: the mass-weighted xipos over its DFS-contiguous subtree
        T s0 = 0, s1 = 0, s2 = 0, ms = 0;
        const int end = m.body_subtree_end[b];
        for (int i = b; i < end; i++) {
          T mi = m.body_mass[i];
          s0 += e.xipos[3 * i] * mi; s1 += e.xipos[3 * i + 1] * mi; s2 += e.xipos[3 * i + 2] * mi;
          ms += mi;
        }
        if (ms < minval<T>()) { s0 = e.xipos[3 * b]; s1 = e.xipos[3 * b + 1]; s2 = e.xipos[3 * b + 2]; }
        else { T inv = (T)1 / ms; s0 *= inv; s1 *= inv; s2 *= inv; }
        base[0] = s0; base[1] = s1; base[2] = s2;
        off = rc.poscom0 + 3 * c;
      }
      for (int k = 0; k < 3; k++) out[k] = base[k] + off[k];
      for (int k = 0; k < 9; k++) out[3 + k] = rc.mat0[9 * c + k];
    }
  }
}

}  // namespace mgx
