// mgx_ray.hip — batched ray casting and depth cameras (include/mgx.h "ray casting").
//
// Two kinds of kernel:
//   k_ray_scene  one wave per env: kinematics() / geom_poses() of mgx_physics.h from the current
//                qpos, geom world poses written straight into the caller's scene buffer, then the
//                world pose of every camera (for trackcom cameras the subtree COM of its body).
//   k_ray<Gen>   grid (env, ray tiles of 256), one ray per lane. The workgroup stages its env's
//                scene and the geom constants into LDS once, then every lane walks the geoms in
//                the same order (ray_scene_walk, mgx_ray.h). Gen makes the ray and stores the
//                result: RayList reads caller rays, RayCamera makes a pixel's ray in registers.
// No call allocates or synchronises (mgx_ray_configure excepted: it is a *_configure).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mgx_internal.h"
#include "mgx_physics.h"
#include "mgx_ray.h"

using namespace mgx;

namespace {

// ------------------------------------------------------------------------- scene
template <typename T>
__global__ void __launch_bounds__(64) k_ray_scene(DevModel<T> m, RayCams<T> rc, const T* gqpos, T* scene,
                                                  const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  extern __shared__ __align__(16) char smem[];
  Env<T> e;  // slim binding: only what kinematics() and geom_poses() read or write
  ray_scene_env(m, rc, gqpos + (size_t)env * m.nq, scene + (size_t)env * ray_scene_reals(m.ngeom, rc.ncam),
                reinterpret_cast<T*>(smem), e);
}

// ------------------------------------------------------------------------- rays
// caller rays: pnt / vec [N][n_ray][3], dist [N][n_ray] (-1 for a miss), geomid [N][n_ray]
template <typename T>
struct RayList {
  const T *pnt, *vec;
  T* dist;
  int* geomid;
  __device__ __forceinline__ void make(const T*, size_t at, int, T* p, T* v) const {
    for (int k = 0; k < 3; k++) { p[k] = pnt[3 * at + k]; v[k] = vec[3 * at + k]; }
  }
  __device__ __forceinline__ void store(size_t at, T x, int id) const {
    dist[at] = id < 0 ? (T)-1 : x;
    geomid[at] = id;
  }
};

// camera pixels: the ray of pixel (r, c) is made in registers from the camera pose in the scene
template <typename T>
struct RayCamera {
  int cam_off, height, width;  // cam_off: the camera's pose in one env's scene (reals)
  T t;                         // tan(fovy / 2)
  float* depth;                // [N][H][W], +inf for a miss (nullable)
  int* seg;                    // [N][H][W] (nullable)
  __device__ __forceinline__ void make(const T* sc, size_t, int ray, T* p, T* v) const {
    ray_camera_pixel(sc + cam_off, height, width, t, ray, p, v);
  }
  __device__ __forceinline__ void store(size_t at, T x, int id) const {
    if (depth) depth[at] = id < 0 ? __builtin_huge_valf() : (float)x;
    if (seg) seg[at] = id;
  }
};

template <typename T, typename Gen>
__global__ void __launch_bounds__(MGX_RAY_TILE) k_ray(int ngeom, const int* geom_type, const int* geom_bodyid,
                                                      const T* geom_size, const T* geom_rbound,
                                                      const uint8_t* enable0, const uint8_t* enable1, int bodyexclude,
                                                      const T* scene, int scene_reals, Gen gen, int n_ray,
                                                      const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;  // uniform over the workgroup: the outputs stay untouched
  extern __shared__ __align__(16) char smem[];
  T* rec = reinterpret_cast<T*>(smem);
  int* typ = reinterpret_cast<int*>(rec + MGX_RAY_REC * ngeom);
  const T* sc = scene + (size_t)env * scene_reals;
  const int tid = threadIdx.x;
  ray_stage_geoms(rec, typ, ngeom, geom_type, geom_bodyid, geom_size, geom_rbound, enable0, enable1, bodyexclude, sc,
                  tid);
  __syncthreads();
  const int ray = blockIdx.y * MGX_RAY_TILE + tid;
  if (ray >= n_ray) return;  // tail tile (no barrier follows)
  const size_t at = (size_t)env * n_ray + ray;
  T p[3], v[3], x;
  int id;
  gen.make(sc, at, ray, p, v);
  ray_scene_walk(rec, typ, ngeom, p, v, x, id);
  gen.store(at, x, id);
}

int ray_lds_bytes(int ngeom, int rb) { return MGX_RAY_REC * ngeom * rb + 4 * ngeom; }

}  // namespace

namespace mgx {
int ray_ready(const mgx_model* m) {
  if (!m) return host_fail(MGX_E_ARG, "null model");
  if (!m->ray) return host_fail(MGX_E_ARG, "mgx_ray_configure has not been called for this model");
  if (m->ray->unsupported)
    return host_fail(MGX_E_UNSUPPORTED, "ray casting supports plane, sphere, capsule, cylinder and box geoms only");
  return MGX_OK;
}
}  // namespace mgx

namespace {

template <typename T, typename Gen>
int launch_rays(const mgx_model* m, const DevModel<T>& M, const void* scene, const Gen& gen, int n_ray,
                const uint8_t* geom_enable, int bodyexclude, int n_env, const uint8_t* mask, hipStream_t st) {
  const RayState& rs = *m->ray;
  const int tiles = (n_ray + MGX_RAY_TILE - 1) / MGX_RAY_TILE;
  if (tiles > 65535) return host_fail(MGX_E_CAPACITY, "more than 65535 * 256 rays per env");
  hipLaunchKernelGGL((k_ray<T, Gen>), dim3(n_env, tiles), dim3(MGX_RAY_TILE), ray_lds_bytes(M.ngeom, sizeof(T)), st,
                     M.ngeom, M.geom_type, M.geom_bodyid, M.geom_size, M.geom_rbound, rs.enable, geom_enable,
                     bodyexclude, (const T*)scene, ray_scene_reals(M.ngeom, rs.ncam), gen, n_ray, mask);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

template <typename T>
void upload_cams(std::vector<char>& host, const mgx_ray_desc* d, RayCams<T>& rc,
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
  const size_t nc = d->ncam;
  rc.ncam = d->ncam;
  add(d->cam_bodyid, 4 * nc, (const void**)&rc.bodyid);
  add(d->cam_mode, 4 * nc, (const void**)&rc.mode);
  reals(d->cam_pos, 3 * nc, &rc.pos); reals(d->cam_quat, 4 * nc, &rc.quat);
  reals(d->cam_pos0, 3 * nc, &rc.pos0); reals(d->cam_poscom0, 3 * nc, &rc.poscom0);
  reals(d->cam_mat0, 9 * nc, &rc.mat0);
}

}  // namespace

namespace mgx {
void ray_release(mgx_model* m) {
  if (!m || !m->ray) return;
  render_release(m->ray);
  if (m->ray->dbuf) (void)hipFree(m->ray->dbuf);
  delete m->ray;
  m->ray = nullptr;
}
}  // namespace mgx

extern "C" {

int mgx_ray_configure(mgx_model* m, const mgx_ray_desc* d) {
  if (!m || !d) return host_fail(MGX_E_ARG, "null argument");
  const bool f32 = m->precision == MGX_F32;
  const int ng = f32 ? m->mf.ngeom : m->md.ngeom, nb = f32 ? m->mf.nbody : m->md.nbody;
  if (d->ngeom != ng) return host_fail(MGX_E_ARG, "mgx_ray_desc.ngeom differs from the model's");
  if (d->ncam < 0 || d->ncam > MGX_RAY_MAX_CAM) return host_fail(MGX_E_CAPACITY, "more than MGX_RAY_MAX_CAM cameras");
  if (!d->geom_enable && ng > 0) return host_fail(MGX_E_ARG, "null geom_enable");
  if (d->ncam > 0 && (!d->cam_bodyid || !d->cam_mode || !d->cam_pos || !d->cam_quat || !d->cam_fovy || !d->cam_pos0 ||
                      !d->cam_poscom0 || !d->cam_mat0))
    return host_fail(MGX_E_ARG, "null camera table");
  ray_release(m);
  RayState* rs = new RayState();
  m->ray = rs;
  rs->ngeom = ng;
  // geom types the ray kernels know (the model keeps its tables on the device only)
  MGX_HIPCHK(hipSetDevice(m->device));
  std::vector<int> gt(ng > 0 ? ng : 1, 0);
  if (ng > 0)
    MGX_HIPCHK(hipMemcpy(gt.data(), f32 ? m->mf.geom_type : m->md.geom_type, 4 * (size_t)ng, hipMemcpyDeviceToHost));
  for (int g = 0; g < ng; g++) {
    const int t = gt[g];
    if (t != GPLANE && t != GSPHERE && t != GCAPSULE && t != GCYLINDER && t != GBOX) {
      rs->unsupported = true;
      return ray_ready(m);
    }
  }
  if (ray_lds_bytes(ng, f32 ? 4 : 8) > MGX_RAY_LDS_LIMIT) {
    ray_release(m);
    return host_fail(MGX_E_CAPACITY, "too many geoms for the ray kernels' LDS scene");
  }
  for (int c = 0; c < d->ncam; c++) {
    const int mode = d->cam_mode[c];
    if (mode != MGX_CAM_FIXED && mode != MGX_CAM_TRACK && mode != MGX_CAM_TRACKCOM) {
      ray_release(m);
      return host_fail(MGX_E_UNSUPPORTED, "camera modes targetbody / targetbodycom are not supported");
    }
    if (d->cam_bodyid[c] < 0 || d->cam_bodyid[c] >= nb) {
      ray_release(m);
      return host_fail(MGX_E_ARG, "cam_bodyid out of range");
    }
    if (!(d->cam_fovy[c] > 0 && d->cam_fovy[c] < 180)) {
      ray_release(m);
      return host_fail(MGX_E_ARG, "cam_fovy must be in (0, 180) degrees");
    }
    rs->cam_mode[c] = mode;
    rs->cam_fovy[c] = d->cam_fovy[c];
  }
  rs->ncam = d->ncam;
  std::vector<char> host((size_t)(ng > 0 ? ng : 1), 0);
  if (ng > 0) memcpy(host.data(), d->geom_enable, ng);
  std::vector<std::pair<size_t, const void**>> fix;
  if (f32) upload_cams<float>(host, d, rs->cf, fix);
  else upload_cams<double>(host, d, rs->cd, fix);
  hipError_t err = hipMalloc(&rs->dbuf, host.size());
  if (err == hipSuccess) err = hipMemcpy(rs->dbuf, host.data(), host.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    ray_release(m);
    return host_fail(MGX_E_HIP, std::string("mgx_ray_configure: ") + hipGetErrorString(err));
  }
  rs->enable = (const uint8_t*)rs->dbuf;
  for (auto& f : fix) *f.second = (char*)rs->dbuf + f.first;
  return MGX_OK;
}

int64_t mgx_ray_scene_bytes(const mgx_model* m, int n_env) {
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  if (n_env <= 0) return host_fail(MGX_E_ARG, "n_env must be > 0");
  return (int64_t)n_env * ray_scene_reals(m->ray->ngeom, m->ray->ncam) * (m->precision == MGX_F32 ? 4 : 8);
}

int mgx_ray_scene(const mgx_model* m, const mgx_state* s, void* scene, uint64_t bytes, int n_env,
                  const uint8_t* env_mask, void* stream) {
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  if (!s || !s->qpos || !scene || n_env <= 0) return host_fail(MGX_E_ARG, "null state / scene or n_env <= 0");
  if (bytes < (uint64_t)mgx_ray_scene_bytes(m, n_env)) return host_fail(MGX_E_ARG, "scene buffer too small");
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) {
    DevModel<float> M = m->mf;
    M.L.late_geom = 0;
    const int lds = scene_lds_reals(M.nq, M.nbody, M.njnt) * 4;
    if (lds > MGX_RAY_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the ray scene kernel's LDS");
    hipLaunchKernelGGL(k_ray_scene<float>, dim3(n_env), dim3(64), lds, st, M, m->ray->cf, (const float*)s->qpos,
                       (float*)scene, env_mask);
  } else {
    DevModel<double> M = m->md;
    M.L.late_geom = 0;
    const int lds = scene_lds_reals(M.nq, M.nbody, M.njnt) * 8;
    if (lds > MGX_RAY_LDS_LIMIT) return host_fail(MGX_E_CAPACITY, "model too large for the ray scene kernel's LDS");
    hipLaunchKernelGGL(k_ray_scene<double>, dim3(n_env), dim3(64), lds, st, M, m->ray->cd, (const double*)s->qpos,
                       (double*)scene, env_mask);
  }
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

int mgx_ray_cast(const mgx_model* m, const void* scene, const void* pnt, const void* vec, int n_ray,
                 const uint8_t* geom_enable, int bodyexclude, void* dist, int32_t* geomid, int n_env,
                 const uint8_t* env_mask, void* stream) {
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  if (!scene || !pnt || !vec || !dist || !geomid) return host_fail(MGX_E_ARG, "null buffer");
  if (n_env <= 0 || n_ray <= 0) return host_fail(MGX_E_ARG, "n_env and n_ray must be > 0");
  hipStream_t st = (hipStream_t)stream;
  if (m->precision == MGX_F32) {
    RayList<float> gen{(const float*)pnt, (const float*)vec, (float*)dist, geomid};
    return launch_rays<float>(m, m->mf, scene, gen, n_ray, geom_enable, bodyexclude, n_env, env_mask, st);
  }
  RayList<double> gen{(const double*)pnt, (const double*)vec, (double*)dist, geomid};
  return launch_rays<double>(m, m->md, scene, gen, n_ray, geom_enable, bodyexclude, n_env, env_mask, st);
}

int mgx_ray_camera(const mgx_model* m, const void* scene, int cam, int height, int width, const uint8_t* geom_enable,
                   int bodyexclude, float* depth, int32_t* seg, int n_env, const uint8_t* env_mask, void* stream) {
  int rc = ray_ready(m);
  if (rc != MGX_OK) return rc;
  if (!scene || (!depth && !seg)) return host_fail(MGX_E_ARG, "null scene, or neither depth nor seg given");
  if (cam < 0 || cam >= m->ray->ncam) return host_fail(MGX_E_ARG, "camera index out of range");
  if (n_env <= 0 || height <= 0 || width <= 0 || (int64_t)height * width > (int64_t)65535 * MGX_RAY_TILE)
    return host_fail(MGX_E_ARG, "n_env, height and width must be > 0 (at most 65535 * 256 pixels)");
  hipStream_t st = (hipStream_t)stream;
  const double t = std::tan(m->ray->cam_fovy[cam] * (M_PI / 180.0) * 0.5);
  const int off = ray_scene_cam(m->ray->ngeom, cam);
  if (m->precision == MGX_F32) {
    RayCamera<float> gen{off, height, width, (float)t, depth, seg};
    return launch_rays<float>(m, m->mf, scene, gen, height * width, geom_enable, bodyexclude, n_env, env_mask, st);
  }
  RayCamera<double> gen{off, height, width, t, depth, seg};
  return launch_rays<double>(m, m->md, scene, gen, height * width, geom_enable, bodyexclude, n_env, env_mask, st);
}

}  // extern "C"
