// mgx_internal.h — host-side definitions shared by the translation units of libmgx.so
// (mgx_api.hip: the model; mgx_staged_host.hip: what the staged tasks' hosts share; mgx_soccer.hip:
// humanoid_soccer; mgx_step.hip: generic step; mgx_parkour.hip: quadruped_parkour; mgx_bipedal.hip:
// bipedal_rescue; mgx_dancing.hip: humanoid_dancing; mgx_task_host.h: the checks and the kernel
// dispatch the task entries share).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/mgx.h"
#include "mgx_bipedal.h"
#include "mgx_construction.h"
#include "mgx_dancing.h"
#include "mgx_martial.h"
#include "mgx_parkour.h"
#include "mgx_staged.h"
#include "mgx_bank.h"

namespace mgx {
// A/B and test hooks (MGX_* environment variables). Read once per model, in mgx_model_create, and
// kept with the model, so a launch never depends on the environment at call time. None of them
// changes a result: each selects another schedule of the same arithmetic (tests/test_gpu_capacity.py
// checks the ones that move slots between launches bit for bit). MGX_PGS_LPS (solver lanes per
// slot) is read once per process (pgs_lanes): the solver kernels' LDS limits are set from it.
struct Hooks {
  int pgs_lds_rows = 0;  // MGX_PGS_LDS_ROWS: the soccer main solver launch's LDS rows (0: model default)
  int rk_lds_rows = 0;   // MGX_RK_LDS_ROWS: the RK4 main solver launch's LDS rows (0: 256)
  int pgs_single = 0;    // MGX_PGS_SINGLE: one main launch over every slot, scalars from the pipe
  int pgs_lds_b = 0;     // MGX_PGS_LDS_B: the main launch copies B into an LDS arena
  int pgs_arena = 0;     // MGX_PGS_ARENA: that arena's bytes (0: MGX_PGS_ARENA_F32 / _F64)
  int pgs_lds_pad = 0;   // MGX_PGS_LDS_PAD: pad the main solver launch's LDS (occupancy probe)
  int pgs_wide_lds = 1;  // MGX_PGS_WIDE_LDS: the wide launch copies its slot's B into LDS
  int pgs_spw = 0;       // MGX_PGS_SPW: slots per solver wave (debug)
  int pgs_wpc = 4;       // MGX_PGS_WPC: main solver launch's waves per CU its LDS rows are sized for
  int pgs_prio_rows = 0; // MGX_PGS_PRIO_ROWS: rows above which a main-launch solver wave raises its priority
  int pgs_split_blocks = -1;  // MGX_PGS_SPLIT_BLOCKS: blocks from which a main-launch slot is solved row-split,
                              // one slot per wave (-1: the pipeline's default; 0: off; 1: every slot)
  int tight_bp = -1;    // MGX_TIGHT_BROADPHASE: box prefilters in the broadphase (-1: by the pair count)
  int side_stream = 1;   // MGX_SIDE_STREAM: the wide solver launch on a side stream
  int bank_stream = 0;   // MGX_BANK_STREAM: the soccer reset banks' pipeline on a low-priority stream beside the
                         // live step (0: off, one stream; 1: bank finisher before the live one; 2: after it;
                         // -1, not set: the compiled default MGX_BANK_STREAM; in fp32 only with the tail finisher)
  int tail_finish = -1;  // MGX_TAIL_FINISH: soccer: the row-split (heavy) slots' solver waves on a side stream and
                         // the light envs finished beside them (soccer_step_staged; 0: off; 1: on;
                         // -1, not set: the compiled default MGX_TAIL_FINISH beside the bank stream, off without it)
  int tail_factor = 1;   // MGX_TAIL_FACTOR: with the tail finisher, the row builder factorises qMH for the heavy
                         // slots (1), for no slot (0), for every slot (2: test hook)
  int gcon = 1;          // MGX_GCON: the row builder's contact points in the pipe (0: in LDS)
  int rows_lds = 0;      // MGX_ROWS_LDS: pad the row builder's LDS (occupancy probe)
  int chain_records = 3; // MGX_CHAIN_RECORDS: the staged row builders' chain walks (Layout.chain_rec): 1 the joint
                         // pre-pass of kinematics, 2 the packed chain records, 3 both, 0 neither
};
Hooks read_hooks();
struct RayState;  // ray casting tables (mgx_ray.h), owned by the model once mgx_ray_configure ran
struct SensorState;  // site and sensor tables (mgx_sensor.h), owned by the model once mgx_sensor_configure ran
}  // namespace mgx

struct mgx_model {
  mgx::Hooks hooks;
  int precision;
  int device;
  void* dbuf = nullptr;
  size_t dbytes = 0;
  mgx::DevModel<float> mf, mfs, mff;   // monolithic / staged row builder / staged finisher layouts
  mgx::DevModel<double> md, mds, mdf;
  mgx::Layout L, Ls, Lf;
  bool soccer_ok = false;
  mgx::SoccerIds<float> sf;
  mgx::SoccerIds<double> sd;
  bool parkour_ok = false;
  mgx::ParkourIds<float> pkf;
  mgx::ParkourIds<double> pkd;
  bool martial_ok = false;
  mgx::MartialIds ma;
  bool bipedal_ok = false;
  mgx::BipedalIds bp;
  bool dancing_ok = false;
  mgx::DancingIds dn;
  bool assembly_ok = false;
  mgx_assembly_ids as;
  bool construction_ok = false;
  mgx::ConstructionIds cn;
  int npair;
  bool wide = false;       // nv > 64: only the wide kernels (mgx_wide.h) run this model
  bool staged_ok = false;  // the staged soccer pipeline supports this model's capacities
  bool staged_rk_ok = false;  // the staged RK4 pipeline (bipedal) supports this model
  mgx::RayState* ray = nullptr;  // mgx_ray_configure (mgx_ray.hip); freed by ray_release
  mgx::SensorState* sensor = nullptr;  // mgx_sensor_configure (mgx_sensor.hip); freed by sensor_release
};

namespace mgx {
// Debug dump of one forward pass (stage outputs): offsets into one env's record
// (mgx_debug_forward / mgx_debug_layout; the wide kernels write the same layout)
struct DbgOff {
  int xpos, xquat, xipos, subtree_com, cinert, cdof, qM, qLD, geom_xpos, geom_xmat, ncon, con_dist, con_pos,
      con_frame, con_geom, nefc, efc_type, efc_id, efc_pos, efc_margin, efc_R, efc_aref, Bmat, cvel, cdof_dot,
      qfrc_smooth, qacc_smooth, efc_force, qacc, qfrc_constraint, niter, total;
};
inline DbgOff dbg_offsets(int nb, int nv, int nM, int ng, int C, int E) {
  DbgOff o;
  int p = 0;
  auto take = [&](int n) { int r = p; p += n; return r; };
  o.xpos = take(3 * nb); o.xquat = take(4 * nb); o.xipos = take(3 * nb); o.subtree_com = take(3 * nb);
  o.cinert = take(10 * nb); o.cdof = take(6 * nv); o.qM = take(nM); o.qLD = take(nM);
  o.geom_xpos = take(3 * ng); o.geom_xmat = take(9 * ng); o.ncon = take(1); o.con_dist = take(C);
  o.con_pos = take(3 * C); o.con_frame = take(9 * C); o.con_geom = take(2 * C); o.nefc = take(1);
  o.efc_type = take(E); o.efc_id = take(E); o.efc_pos = take(E); o.efc_margin = take(E); o.efc_R = take(E);
  o.efc_aref = take(E); o.Bmat = take(E * nv); o.cvel = take(6 * nb); o.cdof_dot = take(6 * nv);
  o.qfrc_smooth = take(nv); o.qacc_smooth = take(nv); o.efc_force = take(E); o.qacc = take(nv);
  o.qfrc_constraint = take(nv); o.niter = take(1); o.total = p;
  return o;
}
// the wide (nv > 64) physics kernels (mgx_construction.hip)
int wide_step(const mgx_model* m, const mgx_state* s, const mgx_frames& fr, int n_env, int nsub, const uint8_t* mask,
              hipStream_t st);
int wide_debug(const mgx_model* m, const mgx_state* s, int n_env, void* dbg, const DbgOff& o, hipStream_t st);
int wide_kernels_configure(const mgx_model* m);
// records the message returned by mgx_last_error() and returns `code`
int host_fail(int code, const std::string& msg);
int host_check_state(const mgx_state* s);
// a model whose constraint rows live in per-env global scratch (Layout.gB) needs mgx_state.scratch
int host_check_scratch(const mgx_model* m, const mgx_state* s);
// dynamic-LDS attributes of the generic step kernels (mgx_step.hip)
int step_kernels_configure(const mgx_model* m);
// ... of the soccer kernels and, for a staged model, of the staged pipeline's (mgx_soccer.hip)
int soccer_kernels_configure(const mgx_model* m);
// the staged solver S2 (mgx_pgs.hip)
template <typename T>
void launch_pgs(const Pipe& P, int slots, int lds, hipStream_t st, int maxit, T tol, T scale, int big, const Hooks& h,
                int part = 0);
// bytes: the solver kernels' dynamic-LDS limit; wide: the LDS-B instantiations' (the wide launch)
int pgs_configure_lds(int precision, int bytes, int wide);
// S1 / S3 and the one-wave settle (mgx_pgs.hip, the staged TU)
template <typename T>
void launch_soccer_rows(const DevModel<T>& Ms, const SoccerIds<T>& ids, const mgx_state& s, const mgx_soccer_env& ev,
                        const float* action, int n_env, const uint8_t* mask, const Pipe& P, int banks, int slots, int lds,
                        hipStream_t st, int slot0 = 0);
template <typename T>
void launch_soccer_bank_finish(const DevModel<T>& Mf, const SoccerIds<T>& ids, int n_env, const Pipe& P, int lists,
                               int lds, hipStream_t st);
template <typename T>
void launch_soccer_finish(const DevModel<T>& Mf, const SoccerIds<T>& ids, const mgx_state& s, const mgx_soccer_env& ev,
                          const float* action, float* obs, double* reward, uint8_t* terminated, uint8_t* truncated,
                          float* final_obs, int autoreset, uint64_t seed, int env_offset, int n_env, const uint8_t* mask,
                          const Pipe& P, int banks, int lds, hipStream_t st, bool bank_too = true, int tier = 0);
template <typename T>
void launch_soccer_settle(const DevModel<T>& Ms, const DevModel<T>& Mf, const SoccerIds<T>& ids, const mgx_state& s,
                          const mgx_soccer_env& ev, const T* draws, float* obs, uint64_t seed, int env_offset, int n_env,
                          const uint8_t* mask, const Pipe& P, int mode, int grid, int lds, hipStream_t st, int maxit, T tol,
                          T scale);
int staged_kernels_configure(int precision, int ls, int lf, int settle);
// staged-step workspace layout (mgx_staged_host.hip) and the LDS of one solver wave holding `rows` rows
// per slot with `lps` lanes per slot and `tw` table words per block
// split_default: the pipeline's row-split threshold in blocks when MGX_PGS_SPLIT_BLOCKS is not set
// (Pipe.split_blocks; 0: off)
size_t make_staged_pipe(const mgx_model* m, void* ws, int n_env, int banks, Pipe* P, bool rk, int nobs,
                        int split_default = 0);
// sqg: row scalars in the pipe, only the forces in LDS (the RK4 pipeline; soccer at full capacity)
// twl: block-table words per block in LDS (mgx_twl: 8 for the 8-dof group layout, 4 dof-granular)
int staged_pgs_lds_bytes(const mgx_model* m, int rows, int lps, int sqg, int twl);
// LDS of the soccer wide launch's one-slot waves with B in LDS, 0 when B stays in global memory
int wide_arena_bytes(const mgx_model* m);
// LDS of a one-wave settle: the row builder's layout, then one solver wave with maxE rows per slot,
// then the finisher's layout, in turn
int staged_settle_lds(const mgx_model* m, const Pipe& P, int lps, int sqg, int twl);
// the solver's cost scale, 1 / (meaninertia * nv)
template <typename T>
T staged_scale(const DevModel<T>& M) {
  return (T)1 / (M.meaninertia * (T)(M.nv > 1 ? M.nv : 1));
}
// waves of a settle kernel's fixup launch (grid-stride over the finisher's list; exits at once when
// the list is empty)
inline int fixup_grid(int n_env) { return n_env < 256 ? n_env : 256; }
// f(std::integral_constant<int, E>) for the solver's register entries per lane E = epl in 1 .. 4
template <typename F>
void dispatch_epl(int epl, F&& f) {
  switch (epl) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
// A side stream and two events per caller stream (created once, kept for the process): a solver
// launch runs beside the main one. nullptr if the runtime refuses (then both run in order).
struct SideStream {
  hipStream_t s;
  hipEvent_t rows, big;
};
SideStream* side_stream(hipStream_t st);
// The cache behind such streams: one X (a stream and its events) per (caller stream, device), made
// by create(X&) on first use and kept for the process; nullptr is cached when create refuses.
template <typename X, typename Create>
X* stream_cache(hipStream_t st, Create create) {
  static std::mutex mu;
  static std::map<std::pair<hipStream_t, int>, X*> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find({st, dev});
  if (it != cache.end()) return it->second;
  X* x = new X{};
  if (!create(*x)) { delete x; x = nullptr; }
  return cache[{st, dev}] = x;
}
// What a staged task's workspace entries differ in: its name in the messages, the model check and
// its refusal (init_checks: mgx_<task>_workspace_init makes that check too), its make_staged_pipe
// parameters and its checkAcc template kernels, indexed by Layout.gB
struct StagedTask {
  const char* name;
  bool (*ok)(const mgx_model*);
  const char* refusal;
  bool init_checks;
  bool rk;
  int nobs, split_default;
  void (*template_f32[2])(DevModel<float>, Pipe);
  void (*template_f64[2])(DevModel<double>, Pipe);
};
size_t task_pipe(const StagedTask& t, const mgx_model* m, void* ws, int n_env, int banks, Pipe* P);
// the pipe of a step / reset call over the env's workspace, refused when that is too small
int task_pipe_checked(const StagedTask& t, const mgx_model* m, void* ws, uint64_t ws_bytes, int n_env, int banks, Pipe* P,
                      size_t* need = nullptr);
// a staged step / reset call's refusals: the model check, then the env's bank count
int staged_check(const StagedTask& t, const mgx_model* m, int banks);
int64_t staged_workspace_bytes(const StagedTask& t, const mgx_model* m, int n_env, int banks);
int staged_workspace_init(const StagedTask& t, const mgx_model* m, void* workspace, uint64_t bytes, int n_env, int banks,
                          hipStream_t st);
// the staged RK4 bipedal step (mgx_rk_staged.hip)
int bipedal_staged_configure(const mgx_model* m);
int bipedal_step_staged(const mgx_model* m, const mgx_state* s, const mgx_bipedal_env* e, const float* action, float* obs,
                        double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                        uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st);
int bipedal_reset_staged(const mgx_model* m, const mgx_state* s, const mgx_bipedal_env* e, const void* draws,
                         float* obs, uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st);
int64_t bipedal_workspace_bytes(const mgx_model* m, int n_env, int banks);
int bipedal_workspace_init(const mgx_model* m, void* workspace, uint64_t bytes, int n_env, int banks, hipStream_t st);
// the staged quadruped_parkour step (mgx_pk_staged.hip)
bool parkour_staged_ok(const mgx_model* m);
int parkour_staged_configure(const mgx_model* m);
int parkour_step_staged(const mgx_model* m, const mgx_state* s, const mgx_parkour_env* e, const float* action, float* obs,
                        double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                        uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st);
int parkour_reset_staged(const mgx_model* m, const mgx_state* s, const mgx_parkour_env* e, const void* draws,
                         float* obs, uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st);
int64_t parkour_workspace_bytes(const mgx_model* m, int n_env, int banks);
int parkour_workspace_init(const mgx_model* m, void* workspace, uint64_t bytes, int n_env, int banks, hipStream_t st);
int pgs_lanes();
// ray casting (mgx_ray.hip): frees the model's ray tables (mgx_model_destroy)
void ray_release(mgx_model* m);
// sensors and mj_forward (mgx_sensor.hip): frees the model's sensor tables (mgx_model_destroy); the
// dynamic-LDS attributes of the forward kernels (mgx_model_create)
void sensor_release(mgx_model* m);
int forward_kernels_configure(const mgx_model* m);
// Jacobians and dynamics (mgx_dyn.hip): the dynamic-LDS attributes of its kernels (mgx_model_create)
int dyn_kernels_configure(const mgx_model* m);
// inverse kinematics (mgx_ik.hip): the dynamic-LDS attribute of its kernel (mgx_model_create)
int ik_kernels_configure(const mgx_model* m);
}  // namespace mgx

#define MGX_WIDE_MSG "nv > 64: this model runs on the wide (two dofs per lane) kernels only"

#define MGX_HIPCHK(x)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (x);                                                                                \
    if (_e != hipSuccess) return mgx::host_fail(MGX_E_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

template <typename KernelT>
int mgx_set_lds(KernelT k, int bytes) {
  if (bytes > 64 * 1024) MGX_HIPCHK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return MGX_OK;
}
