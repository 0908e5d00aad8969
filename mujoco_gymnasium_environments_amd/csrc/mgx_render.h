// mgx_render.h — shading of a camera pixel on top of the ray walk of mgx_ray.h (include/mgx.h "RGB
// camera images" states the model). Intersections stay in the model's real type T;
// everything from the hit point on is float32.
#pragma once
#include "mgx_ray.h"

namespace mgx {

// Per-geom appearance record, resolved once by mgx_render_configure (floats):
//   c0 [3]  rgb * tex (checker: rgb * rgb1)      c1 [3]  the same (checker: rgb * rgb2)
//   alpha, emission, k_s, 128 s, L0, L1 (checker cell edges; L0 = 0: no checker)
#define MGX_RENDER_APP 12
// Per-light constants (floats): ambient [3] unused by the kernel (summed on the host), diffuse [3],
// specular [3], attenuation [3], cos(cutoff) (-2: no cone), exponent, flags (1 directional,
// 2 casts shadows, 4 active) as a float, pad.
#define MGX_RENDER_LREC 16
#define MGX_LIGHT_DIRECTIONAL 1
#define MGX_LIGHT_SHADOW 2
#define MGX_LIGHT_ACTIVE 4

// What the kernel needs besides the per-geom and per-light tables; passed by value.
struct RenderConst {
  float ambient[3];                  // sum of the active lights' and the headlight's ambient terms
  float head_diffuse[3], head_specular[3];
  int head_active;
  int sky;                           // MGX_BUILTIN_* of the skybox texture (NONE: black)
  float sky1[3], sky2[3];
};

// Host side of the model's render tables (RayState.render).
struct RenderState {
  int ngeom = 0, nlight = 0;
  void* dbuf = nullptr;              // appearance records, light constants, then the light frames
  const float* app = nullptr;        // device [ngeom][MGX_RENDER_APP]
  const float* lrec = nullptr;       // device [nlight][MGX_RENDER_LREC]
  const int* light_bodyid = nullptr; // device [nlight]
  const void* light_frame = nullptr; // device [nlight][6] reals: pos, dir in the body frame
  RenderConst rc;
};

// One env's render scene, in reals: the ray scene, then per light its world position [3] and
// direction [3].
__host__ __device__ inline int render_scene_reals(int ngeom, int ncam, int nlight) {
  return ray_scene_reals(ngeom, ncam) + 6 * nlight;
}
__host__ __device__ inline int render_scene_light(int ngeom, int ncam, int l) {
  return ray_scene_reals(ngeom, ncam) + 6 * l;
}

// LDS of one k_render workgroup: geom records and light frames (reals), appearance and light
// constants (floats), the type tables of the camera / layer walks and of the shadow walks.
__host__ __device__ inline int render_lds_bytes(int ngeom, int nlight, int rb) {
  return (MGX_RAY_REC * ngeom + 6 * nlight) * rb + 4 * (MGX_RENDER_APP * ngeom + MGX_RENDER_LREC * nlight) +
         8 * ngeom;
}

__device__ __forceinline__ float dot3f(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void normalize3f(float* a) {
  const float s = 1.0f / fmaxf(sqrtf(dot3f(a, a)), 1e-30f);
  a[0] *= s; a[1] *= s; a[2] *= s;
}

// Nearest hit with the winning geom's surface piece; `skip` (-1: none) is left out. The same walk
// and the same arithmetic as ray_scene_walk, so dist / geomid with skip = -1 are its results.
template <typename T>
__device__ __forceinline__ void render_walk(const T* rec, const int* typ, int ngeom, const T* p, const T* v, int skip,
                                            T& dist, int& geomid, int& piece) {
  T best = ray_inf<T>();
  int id = -1, pc = 0;
  ray_scene_visit(rec, typ, ngeom, p, v, [&](int g, int t, const T* r, const T* lp, const T* lv) {
    WonPiece w;
    const T x = ray_geom(t, r + 12, lp, lv, w);
    if (x < best && g != skip) { best = x; id = g; pc = w.piece; }
    return true;
  });
  dist = best;
  geomid = id;
  piece = pc;
}

// Is anything on the ray p + x v within x < limit? The walk ends early only when every lane of the
// wave that is still in it has found its occluder.
template <typename T>
__device__ __forceinline__ bool render_occluded(const T* rec, const int* typ, int ngeom, const T* p, const T* v,
                                                T limit) {
  bool hit = false;
  ray_scene_visit(rec, typ, ngeom, p, v, [&](int, int t, const T* r, const T* lp, const T* lv) {
    if (!hit) hit = ray_geom(t, r + 12, lp, lv) < limit;
    return !__all(hit);
  });
  return hit;
}

// Outward unit normal of piece `piece` of a geom of type t at the geom-frame hit point hp, rotated
// to world by the geom's matrix R (row-major [9]).
template <typename T>
__device__ __forceinline__ void render_normal(int t, int piece, const T* sz, const T* hp, const T* R, float* n) {
  float nl[3] = {0.f, 0.f, 1.f};
  if (t == GSPHERE) {
    nl[0] = (float)hp[0]; nl[1] = (float)hp[1]; nl[2] = (float)hp[2];
  } else if (t == GCAPSULE) {
    nl[0] = (float)hp[0]; nl[1] = (float)hp[1];
    nl[2] = piece == 0 ? 0.f : (float)(piece == 1 ? hp[2] + sz[1] : hp[2] - sz[1]);
  } else if (t == GCYLINDER) {
    nl[0] = piece == 0 ? (float)hp[0] : 0.f;
    nl[1] = piece == 0 ? (float)hp[1] : 0.f;
    nl[2] = piece == 0 ? 0.f : (piece == 1 ? -1.f : 1.f);
  } else if (t == GBOX) {
    const int ax = piece >> 1;
    const float s = (piece & 1) ? 1.f : -1.f;
    nl[0] = ax == 0 ? s : 0.f; nl[1] = ax == 1 ? s : 0.f; nl[2] = ax == 2 ? s : 0.f;
  }
  normalize3f(nl);
  for (int k = 0; k < 3; k++) n[k] = (float)R[3 * k] * nl[0] + (float)R[3 * k + 1] * nl[1] + (float)R[3 * k + 2] * nl[2];
}

// c diffuse max(0, n.L) + k_s specular max(0, n.H)^shin [n.L > 0], scaled by w, added to C
__device__ __forceinline__ void render_blinn_phong(float* C, const float* c, const float* n, const float* L,
                                                   const float* dhat, const float* diffuse, const float* specular,
                                                   float ks, float shin, float w) {
  const float ndl = dot3f(n, L);
  if (!(ndl > 0.f)) return;
  float H[3] = {L[0] - dhat[0], L[1] - dhat[1], L[2] - dhat[2]};
  normalize3f(H);
  const float sp = ks * powf(fmaxf(dot3f(n, H), 0.f), shin);
  for (int k = 0; k < 3; k++) C[k] += w * (c[k] * diffuse[k] * ndl + sp * specular[k]);
}

// The colour of the surface point P of geom g (piece, geom-frame hit point hp): emission, ambient
// and every light's Blinn-Phong term behind its shadow ray. The loop over lights is uniform.
template <typename T>
__device__ __forceinline__ void render_shade(const T* rec, const int* typ_shadow, int ngeom, const float* app,
                                             const float* lrec, const T* lightw, int nlight, const RenderConst& rc,
                                             int g, int gtype, int piece, const T* hp, const T* P, const T* v,
                                             const float* dhat, const float* headL, float cam_dist, float* C) {
  const T* r = rec + MGX_RAY_REC * g;
  const float* a = app + MGX_RENDER_APP * g;
  float n[3];
  render_normal(gtype, piece, r + 12, hp, r + 3, n);
  if (n[0] * (float)v[0] + n[1] * (float)v[1] + n[2] * (float)v[2] > 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  float c[3] = {a[0], a[1], a[2]};
  if (a[10] > 0.f) {  // checker on a plane: the cell parity of the plane-local hit point
    const T cu = floor(hp[0] / (T)a[10]), cw = floor(hp[1] / (T)a[11]);
    const T par = cu + cw;
    if (par - (T)2 * floor(par * (T)0.5) != (T)0) { c[0] = a[3]; c[1] = a[4]; c[2] = a[5]; }
  }
  const float emission = a[7], ks = a[8], shin = a[9];
  for (int k = 0; k < 3; k++) C[k] = c[k] * (emission + rc.ambient[k]);
  if (rc.head_active) render_blinn_phong(C, c, n, headL, dhat, rc.head_diffuse, rc.head_specular, ks, shin, 1.f);
  const float eps = 1e-4f * fmaxf(1.f, cam_dist);
  T O[3];
  for (int k = 0; k < 3; k++) O[k] = P[k] + (T)(eps * n[k]);
  for (int l = 0; l < nlight; l++) {
    const float* lr = lrec + MGX_RENDER_LREC * l;
    const int flags = (int)lr[14];
    if (!(flags & MGX_LIGHT_ACTIVE)) continue;  // uniform
    const T* lw = lightw + 6 * l;
    T Lt[3], limit = ray_inf<T>();
    float w = 1.f;
    if (flags & MGX_LIGHT_DIRECTIONAL) {
      for (int k = 0; k < 3; k++) Lt[k] = -lw[3 + k];
    } else {
      for (int k = 0; k < 3; k++) Lt[k] = lw[k] - P[k];
      const T len = sqrt(dot3(Lt, Lt));
      const T inv = (T)1 / (len > minval<T>() ? len : minval<T>());
      for (int k = 0; k < 3; k++) Lt[k] *= inv;
      limit = len;
      const float lf = (float)len;
      w = 1.f / (lr[9] + lr[10] * lf + lr[11] * lf * lf);
      if (lr[12] > -1.5f) {  // a cone
        const float ct = -((float)Lt[0] * (float)lw[3] + (float)Lt[1] * (float)lw[4] + (float)Lt[2] * (float)lw[5]);
        w = ct < lr[12] ? 0.f : w * powf(fmaxf(ct, 0.f), lr[13]);
      }
    }
    const float L[3] = {(float)Lt[0], (float)Lt[1], (float)Lt[2]};
    if ((flags & MGX_LIGHT_SHADOW) && w > 0.f && dot3f(n, L) > 0.f) {
      if (render_occluded(rec, typ_shadow, ngeom, O, Lt, limit)) w = 0.f;
    }
    if (w > 0.f) render_blinn_phong(C, c, n, L, dhat, lr + 3, lr + 6, ks, shin, w);
  }
}

}  // namespace mgx
