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

// side of the z-axis cylinder of radius r, |z| <= h (capsule and cylinder)
template <typename T>
__device__ __forceinline__ void ray_side(T& best, const T* lp, const T* lv, T r, T h) {
  T x0, x1;
  if (ray_quad(lv[0] * lv[0] + lv[1] * lv[1], lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - r * r, x0,
               x1)) {
    ray_take(best, x0, fabs(lp[2] + x0 * lv[2]) <= h);
    ray_take(best, x1, fabs(lp[2] + x1 * lv[2]) <= h);
  }
}

// ray against one geom in its frame; returns the hit distance or +inf. `type` is wave-uniform in
// the scene walk, so this switch does not diverge; only hit / miss does.
template <typename T>
__device__ __forceinline__ T ray_geom(int type, const T* sz, const T* lp, const T* lv) {
  T best = ray_inf<T>();
  T x0, x1;
  switch (type) {
    case GPLANE: {
      if (lv[2] < -minval<T>()) {  // front side only
        T x = -lp[2] / lv[2];
        T px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
        ray_take(best, x, (sz[0] <= 0 || fabs(px) <= sz[0]) && (sz[1] <= 0 || fabs(py) <= sz[1]));
      }
      break;
    }
    case GSPHERE: {
      if (ray_quad(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - sz[0] * sz[0], x0, x1)) {
        ray_take(best, x0, true);
        ray_take(best, x1, true);
      }
      break;
    }
    case GCAPSULE: {
      const T r = sz[0], h = sz[1];
      ray_side(best, lp, lv, r, h);
      const T a = dot3(lv, lv);
#pragma unroll
      for (int s = -1; s <= 1; s += 2) {  // cap spheres at z = s h, accepted where s z >= h
        T dz = lp[2] - s * h;
        if (ray_quad(a, lv[0] * lp[0] + lv[1] * lp[1] + lv[2] * dz, lp[0] * lp[0] + lp[1] * lp[1] + dz * dz - r * r, x0,
                     x1)) {
          ray_take(best, x0, s * (lp[2] + x0 * lv[2]) >= h);
          ray_take(best, x1, s * (lp[2] + x1 * lv[2]) >= h);
        }
      }
      break;
    }
    case GCYLINDER: {
      const T r = sz[0], h = sz[1];
      ray_side(best, lp, lv, r, h);
      if (fabs(lv[2]) > minval<T>()) {
#pragma unroll
        for (int s = -1; s <= 1; s += 2) {  // flat caps at z = s h, accepted inside the disc
          T x = (s * h - lp[2]) / lv[2];
          T px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
          ray_take(best, x, px * px + py * py <= r * r);
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
            ray_take(best, x, fabs(lp[j] + x * lv[j]) <= sz[j] && fabs(lp[k] + x * lv[k]) <= sz[k]);
          }
        }
      }
      break;
    }
    default: break;
  }
  return best;
}

// Nearest hit over the staged geoms. rec: MGX_RAY_REC reals per geom, typ: the geom type or -1
// when the geom is not enabled. Every lane walks the same g, so typ[g] and rec reads are
// same-address LDS broadcasts. The bounding-sphere test only skips geoms the ray cannot touch
// (slack well above the rounding of its own terms), so it changes no result; planes have no
// bounding sphere. Ties keep the lower geom id.
template <typename T>
__device__ __forceinline__ void ray_scene_walk(const T* rec, const int* typ, int ngeom, const T* p, const T* v, T& dist,
                                               int& geomid) {
  const T eps = sizeof(T) == 4 ? (T)1.2e-7 : (T)2.3e-16;
  const T vv = dot3(v, v);
  T best = ray_inf<T>();
  int id = -1;
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
    const T x = ray_geom(t, r + 12, lp, lv);
    if (x < best) { best = x; id = g; }
  }
  dist = best;
  geomid = id;
}

}  // namespace mgx
