// mgx_render.hip — batched RGB camera images (include/mgx.h "RGB camera images").
//
// Two kernels:
//   k_render_scene  one wave per env: the ray scene by ray_scene_env (mgx_ray.h, the code of
//                   k_ray_scene), then lane l writes light l's world position and direction from
//                   the body frames that left behind.
//   k_render        grid (env, pixel tiles of 256), one pixel per lane. The workgroup stages its
//                   env's geoms (ray_stage_geoms), the per-geom appearance records, the light
//                   constants and the env's light frames into LDS once. The camera walk, the
//                   layer walks and the shadow walks all go through ray_scene_visit, every lane on
//                   the same geom index; the loops over layers and lights are uniform.
// No call allocates or synchronises (mgx_render_configure excepted: it is a *_configure).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mgx_internal.h"
#include "mgx_physics.h"
#include "mgx_render.h"

using namespace mgx;

namespace {

template <typename T>
__global__ void __launch_bounds__(64) k_render_scene(DevModel<T> m, RayCams<T> rc, int nlight, const int* light_bodyid,
                                                     const T* light_frame, const T* gqpos, T* scene,
                                                     const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  extern __shared__ __align__(16) char smem[];
  T* sc = scene + (size_t)env * render_scene_reals(m.ngeom, rc.ncam, nlight);
  Env<T> e;
  ray_scene_env(m, rc, gqpos + (size_t)env * m.nq, sc, reinterpret_cast<T*>(smem), e);
  for (int l = lane_id(); l < nlight; l += 64) {
    const int b = light_bodyid[l];
    T* out = sc + render_scene_light(m.ngeom, rc.ncam, l);
    T p[3], d[3];
    mulmatvec3(p, e.xmat + 9 * b, light_frame + 6 * l);
    mulmatvec3(d, e.xmat + 9 * b, light_frame + 6 * l + 3);
    for (int k = 0; k < 3; k++) { out[k] = p[k] + e.xpos[3 * b + k]; out[3 + k] = d[k]; }
  }
}

template <typename T>
struct RenderArgs {
  int ngeom, nlight, bodyexclude;
  const int *geom_type, *geom_bodyid;
  const T *geom_size, *geom_rbound;
  const uint8_t *enable0, *enable1;
  const float *app, *lrec;
  const T* scene;
  int scene_reals, cam_off, light_off, height, width;
  T t;  // tan(fovy / 2)
  uint8_t* rgb8;
  float *rgbf, *depth;
  int* seg;
  const uint8_t* mask;
  RenderConst rc;
};

template <typename T>
__global__ void __launch_bounds__(MGX_RAY_TILE) k_render(RenderArgs<T> a) {
  const int env = blockIdx.x;
  if (a.mask && !a.mask[env]) return;  // uniform over the workgroup: the outputs stay untouched
  extern __shared__ __align__(16) char smem[];
  const int ng = a.ngeom, nl = a.nlight, tid = threadIdx.x;
  T* rec = reinterpret_cast<T*>(smem);
  T* lightw = rec + MGX_RAY_REC * ng;
  float* app = reinterpret_cast<float*>(lightw + 6 * nl);
  float* lrec = app + MGX_RENDER_APP * ng;
  int* typ = reinterpret_cast<int*>(lrec + MGX_RENDER_LREC * nl);
  int* typ_shadow = typ + ng;
  const T* sc = a.scene + (size_t)env * a.scene_reals;
  ray_stage_geoms(rec, typ, ng, a.geom_type, a.geom_bodyid, a.geom_size, a.geom_rbound, a.enable0, a.enable1,
                  a.bodyexclude, sc, tid);
  for (int k = tid; k < MGX_RENDER_APP * ng; k += MGX_RAY_TILE) app[k] = a.app[k];
  for (int k = tid; k < MGX_RENDER_LREC * nl; k += MGX_RAY_TILE) lrec[k] = a.lrec[k];
  for (int k = tid; k < 6 * nl; k += MGX_RAY_TILE) lightw[k] = sc[a.light_off + k];
  __syncthreads();
  // shadow casters: the enabled geoms of alpha exactly 1
  for (int g = tid; g < ng; g += MGX_RAY_TILE) typ_shadow[g] = app[MGX_RENDER_APP * g + 6] == 1.f ? typ[g] : -1;
  __syncthreads();
  const int n_pix = a.height * a.width;
  const int pix = blockIdx.y * MGX_RAY_TILE + tid;
  if (pix >= n_pix) return;  // tail tile (no barrier follows)
  const size_t at = (size_t)env * n_pix + pix;
  const T* cp = sc + a.cam_off;
  T p[3], v[3];
  ray_camera_pixel(cp, a.height, a.width, a.t, pix, p, v);
  const T vinv = (T)1 / sqrt(dot3(v, v));
  const float dhat[3] = {(float)(v[0] * vinv), (float)(v[1] * vinv), (float)(v[2] * vinv)};
  const float headL[3] = {(float)cp[5], (float)cp[8], (float)cp[11]};  // the camera's +Z axis
  float out[3] = {0.f, 0.f, 0.f}, weight = 1.f;
  T o[3] = {p[0], p[1], p[2]};
  int skip = -1;
  bool live = true;
#pragma unroll 1
  for (int layer = 0; layer < MGX_RENDER_MAX_LAYERS; layer++) {
    if (live) {
      T x;
      int id, piece;
      render_walk(rec, typ, ng, o, v, skip, x, id, piece);
      if (layer == 0) {
        if (a.depth) a.depth[at] = id < 0 ? __builtin_huge_valf() : (float)x;
        if (a.seg) a.seg[at] = id;
      }
      if (id < 0) {
        float bg[3] = {0.f, 0.f, 0.f};
        if (a.rc.sky == MGX_BUILTIN_GRADIENT) {
          const float f = 0.5f + 0.5f * dhat[2];
          for (int k = 0; k < 3; k++) bg[k] = a.rc.sky2[k] + (a.rc.sky1[k] - a.rc.sky2[k]) * f;
        } else if (a.rc.sky == MGX_BUILTIN_FLAT) {
          for (int k = 0; k < 3; k++) bg[k] = a.rc.sky1[k];
        }
        for (int k = 0; k < 3; k++) out[k] += weight * bg[k];
        live = false;
      } else {
        const T* r = rec + MGX_RAY_REC * id;
        T P[3], d[3], hp[3], lv[3];
        for (int k = 0; k < 3; k++) { P[k] = o[k] + x * v[k]; d[k] = o[k] - r[k]; }
        mulmatTvec3(hp, r + 3, d);
        mulmatTvec3(lv, r + 3, v);
        for (int k = 0; k < 3; k++) hp[k] += x * lv[k];
        const T dc[3] = {P[0] - p[0], P[1] - p[1], P[2] - p[2]};
        float C[3];
        render_shade(rec, typ_shadow, ng, app, lrec, lightw, nl, a.rc, id, typ[id], piece, hp, P, v, dhat, headL,
                     (float)sqrt(dot3(dc, dc)), C);
        const float alpha = layer == MGX_RENDER_MAX_LAYERS - 1 ? 1.f : app[MGX_RENDER_APP * id + 6];
        for (int k = 0; k < 3; k++) out[k] += weight * alpha * C[k];
        weight *= 1.f - alpha;
        if (alpha >= 1.f) live = false;
        for (int k = 0; k < 3; k++) o[k] = P[k];
        skip = id;
      }
    }
    if (!__any(live)) break;  // the wave leaves only when none of its lanes has a layer left
  }
  float q[3];
  for (int k = 0; k < 3; k++) q[k] = fminf(fmaxf(out[k], 0.f), 1.f);
  if (a.rgbf) for (int k = 0; k < 3; k++) a.rgbf[3 * at + k] = q[k];
  if (a.rgb8) for (int k = 0; k < 3; k++) a.rgb8[3 * at + k] = (uint8_t)(q[k] * 255.f + 0.5f);
}

template <typename T>
int launch_render(const mgx_model* m, const DevModel<T>& M, const void* scene, int cam, int height, int width,
                  const uint8_t* geom_enable, int bodyexclude, uint8_t* rgb8, float* rgbf, float* depth, int32_t* seg,
                  int n_env, const uint8_t* mask, hipStream_t st) {
  const RayState& ray = *m->ray;
  const RenderState& rs = *ray.render;
  RenderArgs<T> a;
  a.ngeom = M.ngeom; a.nlight = rs.nlight; a.bodyexclude = bodyexclude;
  a.geom_type = M.geom_type; a.geom_bodyid = M.geom_bodyid; a.geom_size = M.geom_size; a.geom_rbound = M.geom_rbound;
  a.enable0 = ray.enable; a.enable1 = geom_enable;
  a.app = rs.app; a.lrec = rs.lrec;
  a.scene = (const T*)scene;
  a.scene_reals = render_scene_reals(M.ngeom, ray.ncam, rs.nlight);
  a.cam_off = ray_scene_cam(M.ngeom, cam);
  a.light_off = render_scene_light(M.ngeom, ray.ncam, 0);
  a.height = height; a.width = width;
  a.t = (T)std::tan(ray.cam_fovy[cam] * (M_PI / 180.0) * 0.5);
  a.rgb8 = rgb8; a.rgbf = rgbf; a.depth = depth; a.seg = seg; a.mask = mask;
  a.rc = rs.rc;
  const int tiles = (height * width + MGX_RAY_TILE - 1) / MGX_RAY_TILE;
  hipLaunchKernelGGL(k_render<T>, dim3(n_env, tiles), dim3(MGX_RAY_TILE), render_lds_bytes(M.ngeom, rs.nlight, sizeof(T)),
                     st, a);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

int render_ready(const mgx_model* m) {
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  if (!m->ray->render) return host_fail(MGX_E_ARG, "mgx_render_configure has not been called for this model");
  return MGX_OK;
}

}  // namespace

namespace mgx {
void render_release(RayState* rs) {
  if (!rs || !rs->render) return;
  if (rs->render->dbuf) (void)hipFree(rs->render->dbuf);
  delete rs->render;
  rs->render = nullptr;
}
}  // namespace mgx

extern "C" {

int mgx_render_configure(mgx_model* m, const mgx_render_desc* d) {
  if (!m || !d) return host_fail(MGX_E_ARG, "null argument");
  if (!m->ray) return host_fail(MGX_E_ARG, "mgx_render_configure needs a prior mgx_ray_configure");
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  const bool f32 = m->precision == MGX_F32;
  const int ng = m->ray->ngeom, nb = f32 ? m->mf.nbody : m->md.nbody;
  if (d->ngeom != ng) return host_fail(MGX_E_ARG, "mgx_render_desc.ngeom differs from the model's");
  if (d->nmat < 0 || d->ntex < 0 || d->nlight < 0) return host_fail(MGX_E_ARG, "negative table size");
  if (d->nlight > MGX_RENDER_MAX_LIGHT) return host_fail(MGX_E_CAPACITY, "more than MGX_RENDER_MAX_LIGHT lights");
  if (ng > 0 && (!d->geom_rgba || !d->geom_matid)) return host_fail(MGX_E_ARG, "null geom table");
  if (d->nmat > 0 && (!d->mat_emission || !d->mat_specular || !d->mat_shininess || !d->mat_texid || !d->mat_texrepeat ||
                      !d->mat_texuniform))
    return host_fail(MGX_E_ARG, "null material table");
  if (d->ntex > 0 && (!d->tex_type || !d->tex_builtin || !d->tex_file || !d->tex_rgb1 || !d->tex_rgb2))
    return host_fail(MGX_E_ARG, "null texture table");
  if (d->nlight > 0 && (!d->light_bodyid || !d->light_mode || !d->light_directional || !d->light_castshadow ||
                        !d->light_active || !d->light_pos || !d->light_dir || !d->light_ambient || !d->light_diffuse ||
                        !d->light_specular || !d->light_attenuation || !d->light_cutoff || !d->light_exponent))
    return host_fail(MGX_E_ARG, "null light table");
  if (d->skybox_tex < -1 || d->skybox_tex >= d->ntex) return host_fail(MGX_E_ARG, "skybox_tex out of range");
  for (int l = 0; l < d->nlight; l++) {
    if (d->light_mode[l] != MGX_CAM_FIXED)
      return host_fail(MGX_E_UNSUPPORTED, "light " + std::to_string(l) + ": only lights of mode fixed are supported");
    if (d->light_bodyid[l] < 0 || d->light_bodyid[l] >= nb) return host_fail(MGX_E_ARG, "light_bodyid out of range");
  }
  for (int g = 0; g < ng; g++) {
    const int mt = d->geom_matid[g];
    if (mt >= d->nmat) return host_fail(MGX_E_ARG, "geom_matid out of range");
    if (mt < 0) continue;
    const int tx = d->mat_texid[mt];
    if (tx >= d->ntex) return host_fail(MGX_E_ARG, "mat_texid out of range");
    if (tx >= 0 && d->tex_file[tx])
      return host_fail(MGX_E_UNSUPPORTED, "geom " + std::to_string(g) + " uses a material whose texture " +
                                              std::to_string(tx) + " comes from a file: only builtin textures render");
  }
  if (render_lds_bytes(ng, d->nlight, f32 ? 4 : 8) > MGX_RAY_LDS_LIMIT)
    return host_fail(MGX_E_CAPACITY, "too many geoms for the render kernel's LDS scene");
  MGX_HIPCHK(hipSetDevice(m->device));
  // plane sizes for the checker's cell edges (the model keeps its tables on the device only)
  std::vector<int> gt(ng > 0 ? ng : 1, 0);
  std::vector<double> gs(3 * (size_t)(ng > 0 ? ng : 1), 0.0);
  if (ng > 0) {
    MGX_HIPCHK(hipMemcpy(gt.data(), f32 ? m->mf.geom_type : m->md.geom_type, 4 * (size_t)ng, hipMemcpyDeviceToHost));
    if (f32) {
      std::vector<float> tmp(3 * (size_t)ng);
      MGX_HIPCHK(hipMemcpy(tmp.data(), m->mf.geom_size, 12 * (size_t)ng, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < tmp.size(); i++) gs[i] = tmp[i];
    } else {
      MGX_HIPCHK(hipMemcpy(gs.data(), m->md.geom_size, 24 * (size_t)ng, hipMemcpyDeviceToHost));
    }
  }
  render_release(m->ray);
  RenderState* rs = new RenderState();
  m->ray->render = rs;
  rs->ngeom = ng;
  rs->nlight = d->nlight;
  const int nl = d->nlight;
  std::vector<float> app((size_t)MGX_RENDER_APP * (ng > 0 ? ng : 1), 0.f);
  for (int g = 0; g < ng; g++) {
    float* a = app.data() + (size_t)MGX_RENDER_APP * g;
    const double* rgba = d->geom_rgba + 4 * (size_t)g;
    const int mt = d->geom_matid[g], tx = mt >= 0 ? d->mat_texid[mt] : -1;
    double t0[3] = {1, 1, 1}, t1[3] = {1, 1, 1}, L[2] = {0, 0};
    if (tx >= 0 && d->tex_builtin[tx] != MGX_BUILTIN_NONE) {
      const double *c1 = d->tex_rgb1 + 3 * (size_t)tx, *c2 = d->tex_rgb2 + 3 * (size_t)tx;
      const int bi = d->tex_builtin[tx];
      if (bi == MGX_BUILTIN_FLAT) {
        for (int k = 0; k < 3; k++) t0[k] = t1[k] = c1[k];
      } else if (bi == MGX_BUILTIN_CHECKER && gt[g] == GPLANE) {
        for (int k = 0; k < 3; k++) { t0[k] = c1[k]; t1[k] = c2[k]; }
        for (int k = 0; k < 2; k++) {
          const double rep = d->mat_texrepeat[2 * (size_t)mt + k], sz = gs[3 * (size_t)g + k];
          L[k] = (sz > 0 && !d->mat_texuniform[mt]) ? sz / rep : 1.0 / (2.0 * rep);
        }
      } else {
        for (int k = 0; k < 3; k++) t0[k] = t1[k] = 0.5 * (c1[k] + c2[k]);
      }
    }
    for (int k = 0; k < 3; k++) { a[k] = (float)(rgba[k] * t0[k]); a[3 + k] = (float)(rgba[k] * t1[k]); }
    a[6] = (float)rgba[3];
    a[7] = mt >= 0 ? (float)d->mat_emission[mt] : 0.f;
    a[8] = mt >= 0 ? (float)d->mat_specular[mt] : 0.5f;
    a[9] = (float)(128.0 * (mt >= 0 ? d->mat_shininess[mt] : 0.5));
    a[10] = (float)L[0];
    a[11] = (float)L[1];
  }
  RenderConst& c = rs->rc;
  memset(&c, 0, sizeof(c));
  c.head_active = d->headlight_active != 0;
  for (int k = 0; k < 3; k++) {
    c.ambient[k] = c.head_active ? (float)d->headlight_ambient[k] : 0.f;
    c.head_diffuse[k] = (float)d->headlight_diffuse[k];
    c.head_specular[k] = (float)d->headlight_specular[k];
  }
  std::vector<float> lrec((size_t)MGX_RENDER_LREC * (nl > 0 ? nl : 1), 0.f);
  std::vector<double> frame(6 * (size_t)(nl > 0 ? nl : 1), 0.0);
  for (int l = 0; l < nl; l++) {
    float* r = lrec.data() + (size_t)MGX_RENDER_LREC * l;
    for (int k = 0; k < 3; k++) {
      r[k] = (float)d->light_ambient[3 * l + k];
      r[3 + k] = (float)d->light_diffuse[3 * l + k];
      r[6 + k] = (float)d->light_specular[3 * l + k];
      r[9 + k] = (float)d->light_attenuation[3 * l + k];
      frame[6 * l + k] = d->light_pos[3 * l + k];
      frame[6 * l + 3 + k] = d->light_dir[3 * l + k];
      if (d->light_active[l]) c.ambient[k] += r[k];
    }
    r[12] = d->light_cutoff[l] >= 180.0 ? -2.f : (float)std::cos(d->light_cutoff[l] * (M_PI / 180.0));
    r[13] = (float)d->light_exponent[l];
    r[14] = (float)((d->light_directional[l] ? MGX_LIGHT_DIRECTIONAL : 0) | (d->light_castshadow[l] ? MGX_LIGHT_SHADOW : 0) |
                    (d->light_active[l] ? MGX_LIGHT_ACTIVE : 0));
  }
  c.sky = MGX_BUILTIN_NONE;
  if (d->skybox_tex >= 0) {
    c.sky = d->tex_builtin[d->skybox_tex];
    for (int k = 0; k < 3; k++) {
      c.sky1[k] = (float)d->tex_rgb1[3 * d->skybox_tex + k];
      c.sky2[k] = (float)d->tex_rgb2[3 * d->skybox_tex + k];
    }
  }
  // one allocation: appearance, light constants, light body ids, light frames (reals)
  const size_t rb = f32 ? 4 : 8;
  const size_t o_app = 0, o_lrec = o_app + app.size() * 4, o_body = o_lrec + lrec.size() * 4;
  const size_t o_frame = (o_body + 4 * (size_t)(nl > 0 ? nl : 1) + 15) / 16 * 16;
  std::vector<char> host(o_frame + frame.size() * rb, 0);
  memcpy(host.data() + o_app, app.data(), app.size() * 4);
  memcpy(host.data() + o_lrec, lrec.data(), lrec.size() * 4);
  if (nl > 0) memcpy(host.data() + o_body, d->light_bodyid, 4 * (size_t)nl);
  for (size_t i = 0; i < frame.size(); i++) {
    if (f32) reinterpret_cast<float*>(host.data() + o_frame)[i] = (float)frame[i];
    else reinterpret_cast<double*>(host.data() + o_frame)[i] = frame[i];
  }
  hipError_t err = hipMalloc(&rs->dbuf, host.size());
  if (err == hipSuccess) err = hipMemcpy(rs->dbuf, host.data(), host.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    render_release(m->ray);
    return host_fail(MGX_E_HIP, std::string("mgx_render_configure: ") + hipGetErrorString(err));
  }
  char* base = (char*)rs->dbuf;
  rs->app = (const float*)(base + o_app);
  rs->lrec = (const float*)(base + o_lrec);
  rs->light_bodyid = (const int*)(base + o_body);
  rs->light_frame = base + o_frame;
  return MGX_OK;
}

int64_t mgx_render_scene_bytes(const mgx_model* m, int n_env) {
  int rc = render_ready(m);
  if (rc != MGX_OK) return rc;
  if (n_env <= 0) return host_fail(MGX_E_ARG, "n_env must be > 0");
  return (int64_t)n_env * render_scene_reals(m->ray->ngeom, m->ray->ncam, m->ray->render->nlight) *
         (m->precision == MGX_F32 ? 4 : 8);
}

int mgx_render_scene(const mgx_model* m, const mgx_state* s, void* scene, uint64_t bytes, int n_env,
                     const uint8_t* env_mask, void* stream) {
  int rc = render_ready(m);
  if (rc != MGX_OK) return rc;
  if (!s || !s->qpos || !scene || n_env <= 0) return host_fail(MGX_E_ARG, "null state / scene or n_env <= 0");
  if (bytes < (uint64_t)mgx_render_scene_bytes(m, n_env)) return host_fail(MGX_E_ARG, "scene buffer too small");
  hipStream_t st = (hipStream_t)stream;
  const RenderState& rs = *m->ray->render;
  if (m->precision == MGX_F32) {
    DevModel<float> M = m->mf;
    M.L.late_geom = 0;
    const int lds = scene_lds_reals(M.nq, M.nbody, M.njnt) * 4;
    if (lds > MGX_RAY_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the scene kernel's LDS");
    hipLaunchKernelGGL(k_render_scene<float>, dim3(n_env), dim3(64), lds, st, M, m->ray->cf, rs.nlight, rs.light_bodyid,
                       (const float*)rs.light_frame, (const float*)s->qpos, (float*)scene, env_mask);
  } else {
    DevModel<double> M = m->md;
    M.L.late_geom = 0;
    const int lds = scene_lds_reals(M.nq, M.nbody, M.njnt) * 8;
    if (lds > MGX_RAY_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the scene kernel's LDS");
    hipLaunchKernelGGL(k_render_scene<double>, dim3(n_env), dim3(64), lds, st, M, m->ray->cd, rs.nlight, rs.light_bodyid,
                       (const double*)rs.light_frame, (const double*)s->qpos, (double*)scene, env_mask);
  }
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

int mgx_render_camera(const mgx_model* m, const void* scene, int cam, int height, int width, const uint8_t* geom_enable,
                      int bodyexclude, uint8_t* rgb8, float* rgbf, float* depth, int32_t* seg, int n_env,
                      const uint8_t* env_mask, void* stream) {
  int rc = render_ready(m);
  if (rc != MGX_OK) return rc;
  if (!scene) return host_fail(MGX_E_ARG, "null scene");
  if (!rgb8 && !rgbf && !depth && !seg) return host_fail(MGX_E_ARG, "none of rgb8, rgbf, depth and seg given");
  if (cam < 0 || cam >= m->ray->ncam) return host_fail(MGX_E_ARG, "camera index out of range");
  if (n_env <= 0 || height <= 0 || width <= 0 || (int64_t)height * width > (int64_t)65535 * MGX_RAY_TILE)
    return host_fail(MGX_E_ARG, "n_env, height and width must be > 0 (at most 65535 * 256 pixels)");
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32)
    return launch_render<float>(m, m->mf, scene, cam, height, width, geom_enable, bodyexclude, rgb8, rgbf, depth, seg,
                                n_env, env_mask, st);
  return launch_render<double>(m, m->md, scene, cam, height, width, geom_enable, bodyexclude, rgb8, rgbf, depth, seg,
                               n_env, env_mask, st);
}

}  // extern "C"
