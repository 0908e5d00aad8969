// mgx_pk_staged.hip — the staged quadruped_parkour step (BASELINE configs[1]).
//
// The monolithic parkour kernel (mgx_parkour.hip) runs one env step per wave: clip, ten serial
// mj_step's of 1 ms (parkour_env.py:367-368, each with its own 50-sweep PGS), obstacle motors,
// observation / reward / termination. Here each physics substep k = 0..9 is the staged soccer
// pipeline's three kernels over the same workspace layout (mgx_staged.h):
//
//   R(k)  k_pk_rows     wave per slot: the state -> checkPos / checkVel -> forward up to the
//                       constraint rows (stage_rows); k = 0 also the action clip -> ctrl[:16]
//   S(k)  k_pgs_groups  the lane-group PGS (16 lanes per slot, four slots per wave, heaviest first)
//   F(k)  k_pk_finish   wave per slot: qacc, checkAcc, Euler -> the state; k = 9 the task logic
//                       (parkour_env.py:371-394: obstacle motors, obs, reward, termination) and
//                       the same-step autoreset
//
// Reset banks: a parkour reset is mj_resetData + the start pose + two obstacle draws + ten settle
// mj_step's (parkour_env.py:314-354). A bank record advances one settle step per substep launch
// as an extra slot, so a bank restarted at the end of env step t is ready at the end of step t+1
// (its tenth settle step runs in substep 9's bank finisher, before the live finisher that may
// install it): one bank per env covers every autoreset. reset() and a reset whose bank is not ready
// run k_pk_settle, the same stages in one wave, in this translation unit (one set of flags), so a
// reset has one arithmetic whatever the bank count.
// the staged row builders' chain walks (mgx_physics.h chain_rec): pre-pass and packed records compiled in
#define MGX_CHAIN_RECORDS 1
#include "mgx_internal.h"

using namespace mgx;

namespace mgx {

constexpr int PK_LPS = 16;  // solver lanes per slot
constexpr int PK_OBS = 95;  // parkour_env.py:396-468
// slots of at least this many 4-row blocks are solved row-split, one per wave (Pipe.split_blocks;
// 40 / 56 / 72 measured alike against chains of up to 85 blocks)
constexpr int PK_SPLIT_BLOCKS = 56;
enum { PK_SUBSTEPS = 10 };  // frame_skip (parkour_env.py:367-368)

// ---------------------------------------------------------------- banks
// What parkour plugs into the bank layer (mgx_bank.h): a reset is mj_resetData, the start pose and
// two obstacle draws, ten Euler settle steps, then the observation (parkour_env.py:314-354).
template <typename T>
struct ParkourBank {
  typedef ParkourIds<T> Ids;
  typedef mgx_parkour_env EnvT;
  struct Draws { T d0, d1; };  // the obstacle draws, by value (reset_env clears the LDS they came from)
  static constexpr int OBS = PK_OBS, DRAWS = 2;
  static constexpr bool STG = false, STEP_COUNTS = false;
  static constexpr int FIX_CTR = 5;  // k_pgs_groups clears [0] at every launch, ten times per env step
  __device__ static int fix_entry(int env) { return env; }
  __device__ static int fix_env(int entry) { return entry; }
  __device__ __forceinline__ static Draws draws(Env<T>& e, const Ids&, const T* host, uint64_t seed, uint32_t genv,
                                                uint32_t episode) {
    if (host) return Draws{host[0], host[1]};
    parkour_philox_draws(seed, genv, episode, e.vec1);
    wsync();
    const Draws d{e.vec1[0], e.vec1[1]};
    wsync();
    return d;
  }
  // parkour_reset_body's prologue
  __device__ __forceinline__ static void pose(const DevModel<T>& m, Env<T>& e, const Ids& ids, const Pipe&, int, Draws d) {
    reset_env(m, e);
    if (lane_id() == 0) {
      e.qpos[0] = (T)2.0; e.qpos[1] = (T)0.0; e.qpos[2] = (T)0.6;
      e.qpos[3] = (T)1; e.qpos[4] = 0; e.qpos[5] = 0; e.qpos[6] = 0;
      e.qpos[ids.platform_qpos] = d.d0;
      e.qpos[ids.pendulum_qpos] = d.d1;
    }
    wsync();
  }
  // parkour_reset_body's epilogue: the reset observation from the last settle step's frames and
  // contacts (the finisher's Env)
  __device__ __forceinline__ static void finalize(const DevModel<T>& m, Env<T>& e, const Ids& ids, const Pipe& P, int bi) {
    const int fm = parkour_foot_mask(e, ids);
    parkour_obs(m, e, ids, fm, P.at<float>(P.o_bobs) + (size_t)bi * PK_OBS);
    wsync();
  }
  __device__ __forceinline__ static void track_reset(const DevModel<T>&, const Pipe&, EnvT ev, int env, int) {
    T* lp = (T*)ev.last_position + 3 * (size_t)env;
    if (lane_id() == 0) {
      lp[0] = (T)2.0; lp[1] = (T)0.0; lp[2] = (T)0.6;
      ((T*)ev.max_progress)[env] = 0;
      ev.episode_reward[env] = 0.0;
      ev.er_kind[env] = 0;
      ev.reached[env] = 0; ev.fall_count[env] = 0; ev.stuck[env] = 0; ev.step[env] = 0;
    }
  }
  template <int EPL, int LPS>
  __device__ __forceinline__ static void settle_step(const DevModel<T>& Ms, const DevModel<T>& Mf, const Ids& ids,
                                                     mgx_state, EnvT, const Pipe& P, char* smem, Env<T>& f, int env,
                                                     int bi, int slot, int maxit, T tol, T scale, bool last) {
    euler_settle_step<ParkourBank, T, EPL, LPS>(Ms, Mf, ids, P, smem, f, bi, slot, maxit, tol, scale, last);
  }
};

// ---------------------------------------------------------------- kernels
// R(k): live slot b < n_env (the env's state; k = 0: the action clip), or bank record b - n_env
// (its settle step bk, while 0 <= bk < 10)
template <typename T>
__global__ void __launch_bounds__(64) k_pk_rows(DevModel<T> m, ParkourIds<T> ids, mgx_state s, const float* action,
                                                int action_f64, int n_env, const uint8_t* mask, Pipe P, int banks,
                                                int sub) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  Env<T> e;
  if (b < n_env) {
    if (mask && !mask[b]) return;
    env_bind(m, e, smem);
    bind_carry_tail(m, e, P, b);
    load_state(m, e, (T*)s.qpos, (T*)s.qvel, (T*)s.qacc_warmstart, (T*)s.ctrl, (T*)s.qfrc_applied, (T*)s.xfrc_applied,
               (T*)s.time, b);
    if (sub == 0) parkour_pre(m, e, ids, ActRow(action, action_f64, b, ids.n_leg));
  } else {
    const int bi = b - n_env;
    if (!banks || bi >= n_env * P.R) return;
    const int k = P.at<int>(P.o_bk)[bi];
    if (k < 0 || k >= 10) return;
    env_bind(m, e, smem);
    bind_carry_tail(m, e, P, b);
    bank_load_state(m, e, P, bi);
  }
  int warn = 0;  // mj_checkPos / mj_checkVel
  if (any_bad(e.qpos, m.nq)) { reset_env(m, e); warn++; }
  if (any_bad(e.qvel, m.nv)) { reset_env(m, e); warn++; }
  stage_rows(m, e, P, b, warn);
}

// F(k), bank part: record bi's settle step (one wave per record), launched before the live part so
// that a record completing its tenth step in substep 9 is ready for this step's resets
template <typename T>
__global__ void __launch_bounds__(64) k_pk_bank_finish(DevModel<T> m, ParkourIds<T> ids, int n_env, Pipe P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bi = blockIdx.x;
  if (bi >= n_env * P.R) return;
  int k = P.at<int>(P.o_bk)[bi];
  if (k < 0 || k >= 10) return;
  Env<T> e;
  env_bind(m, e, smem);
  const int slot = n_env + bi;
  int warn = load_carry(m, e, P, slot);
  if (!finish_physics(m, e, P, slot)) {
    load_template(m, e, P);
    warn++;
  }
  bank_store_state(m, e, P, bi, warn);
  k++;
  if (k == 10) ParkourBank<T>::finalize(m, e, ids, P, bi);
  if (lane_id() == 0) P.at<int>(P.o_bk)[bi] = k;
}

// F(k), live part: the env's substep; after substep 9 the task logic and the autoreset. The
// overflow flag of the env step is the OR over its substeps (o_pko), counted once.
template <typename T>
__global__ void __launch_bounds__(64) k_pk_finish(DevModel<T> m, ParkourIds<T> ids, mgx_state s, mgx_parkour_env ev,
                                                  const float* action, float* obs, double* reward, uint8_t* terminated,
                                                  uint8_t* truncated, float* final_obs, int autoreset, uint64_t seed,
                                                  int env_offset, int n_env, const uint8_t* mask, Pipe P, int banks,
                                                  int sub) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int env = blockIdx.x;
  if (env >= n_env) return;
  const int l = lane_id();
  if (env == 0 && l == 0) {  // this substep's solver lists are consumed
    P.ctr()[3] = P.ctr()[1];
    P.ctr()[4] = P.ctr()[2];
    P.ctr()[1] = 0;
    P.ctr()[2] = 0;
    if (sub == 0) P.ctr()[5] = 0;  // the env step's fixup list
  }
  if (env == 0)
    for (int b = l; b < P.nbk; b += 64) P.at<int>(P.o_hist)[b] = 0;
  Env<T> e;
  env_bind(m, e, smem);
  if (mask && !mask[env]) return;
  int warn = load_carry(m, e, P, env);
  if (!finish_physics(m, e, P, env)) {
    load_template(m, e, P);
    warn++;
  }
  int* ovf = P.at<int>(P.o_rkw) + env;  // the env step's overflow flag (o_rkw: per-slot ints)
  const bool over = (sub > 0 && *ovf != 0) || e.overflow != 0;
  if (l == 0 && s.warning) s.warning[env] += warn;
  if (sub < PK_SUBSTEPS - 1) {
    store_state(m, e, (T*)s.qpos, (T*)s.qvel, (T*)s.qacc_warmstart, (T*)s.ctrl, (T*)s.qfrc_applied,
                (T*)s.xfrc_applied, (T*)s.time, env);
    if (l == 0) *ovf = over ? 1 : 0;
    return;
  }
  if (l == 0 && s.overflow && over) s.overflow[env] += 1;
  const bool done =
      parkour_post(m, e, ids, ActRow(action, ev.action_f64, env, ids.n_leg), ev, env, obs, reward, terminated, truncated);
  if (ev.rollout && l == 0) {
    T* ro = (T*)ev.rollout + 4 * (size_t)env;
    ro[0] += (T)reward[env];
    ro[1] += (T)terminated[env];
    ro[2] += (T)truncated[env];
    ro[3] += (T)1;
  }
  store_state(m, e, (T*)s.qpos, (T*)s.qvel, (T*)s.qacc_warmstart, (T*)s.ctrl, (T*)s.qfrc_applied, (T*)s.xfrc_applied,
              (T*)s.time, env);
  if (!(done && autoreset)) return;
  if (final_obs)
    for (int i = l; i < PK_OBS; i += 64) final_obs[(size_t)env * PK_OBS + i] = obs[(size_t)env * PK_OBS + i];
  __threadfence();
  wsync();
  bank_install_or_list<ParkourBank<T>>(m, e, ids, P, s, ev, obs, seed, env_offset, banks, env);
}

// reset() of a staged batch and the step's resets whose bank was not ready: the bank layer's settle
// (mgx_bank.h) over this translation unit's stages
template <typename T, int EPL>
__global__ void __launch_bounds__(64) k_pk_settle(DevModel<T> Ms, DevModel<T> Mf, ParkourIds<T> ids, mgx_state s,
                                                  mgx_parkour_env ev, const T* draws, float* obs, uint64_t seed,
                                                  int env_offset, int n_env, const uint8_t* mask, Pipe P, int mode,
                                                  int maxit, T tol, T scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bank_settle<ParkourBank<T>, T, EPL, PK_LPS>(Ms, Mf, ids, s, ev, draws, obs, seed, env_offset, n_env, mask, P, mode,
                                              maxit, tol, scale, smem);
}

// mj_checkAcc's outcome: mj_step from mj_resetData (monolithic layout; rows in the pipe's template
// scratch when the model keeps its rows in global memory), into the template arrays
template <typename T, bool GB>
__global__ void __launch_bounds__(64) k_pk_template(DevModel<T> m, Pipe P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Env<T> e;
  env_bind<T, GB>(m, e, smem, GB ? P.at<T>(P.o_tscr) : nullptr);
  reset_env(m, e);
  forward(m, e);
  e.qacc_ws = e.qacc;
  euler(m, e);
  template_store(m, e, P);
}

}  // namespace mgx

// ------------------------------------------------------------------------- host side
namespace {

// register entries per solver lane of the parkour model (16 lanes per slot: two 8-dof groups per
// entry): nv 33..48 -> 3
template <typename T>
int pk_epl(const DevModel<T>& M) {
  return ((M.nv + 7) / 8 + 1) / 2;
}

int pk_settle_lds(const mgx_model* m, const Pipe& P) { return staged_settle_lds(m, P, PK_LPS, 0, 8); }

const StagedTask kParkourStaged = {"parkour", parkour_staged_ok, "staged parkour step: model outside the staged pipeline",
                                   true, false, PK_OBS, PK_SPLIT_BLOCKS,
                                   {k_pk_template<float, false>, k_pk_template<float, true>},
                                   {k_pk_template<double, false>, k_pk_template<double, true>}};

template <typename T>
int step_staged(const mgx_model* m, const DevModel<T>& M, const DevModel<T>& Ms, const DevModel<T>& Mf,
                const ParkourIds<T>& ids, const mgx_state* s, const mgx_parkour_env* e, const float* action,
                float* obs, double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st) {
  Pipe P;
  const int banks = autoreset ? e->banks : 0;
  if (int rc = task_pipe_checked(kParkourStaged, m, e->workspace, e->workspace_bytes, n_env, e->banks, &P)) return rc;
  // parkour_staged_ok: every slot is solved by the main launch (a slot over capE rows, e.g. the
  // qpos0 pile-up after a bad-state reset, in its heaviest-first list: row-split, one slot per wave,
  // Pipe.split_blocks; with MGX_PGS_SPLIT_BLOCKS=0 its scalars read from the pipe, Pipe.hmain)
  const int slots = n_env * (1 + banks);
  const T scale = staged_scale(M);
  // Pipe.split_blocks: a row-split wave's one slot of maxE rows
  const int mlds = std::max({staged_pgs_lds_bytes(m, P.capE, PK_LPS, 0, 8),
                            P.hmain ? staged_pgs_lds_bytes(m, P.maxE, PK_LPS, 1, 8) : 0,
                            P.split_blocks ? staged_pgs_lds_bytes(m, P.maxE, 64, 0, 8) : 0});
  const int spw = 64 / PK_LPS, grid = (slots + spw - 1) / spw;
  for (int k = 0; k < PK_SUBSTEPS; k++) {
    hipLaunchKernelGGL(k_pk_rows<T>, dim3(slots), dim3(64), m->Ls.bytes, st, Ms, ids, *s, action, e->action_f64, n_env,
                       mask, P, banks, k);
    dispatch_epl(pk_epl(M), [&](auto epl) {
      hipLaunchKernelGGL((k_pgs_groups<T, decltype(epl)::value, PK_LPS, false>), dim3(grid), dim3(64), mlds, st, P,
                         M.iterations, M.tolerance, scale, spw, 0, 0);
    });
    if (banks && P.R > 0)
      hipLaunchKernelGGL(k_pk_bank_finish<T>, dim3(n_env * P.R), dim3(64), m->Lf.bytes, st, Mf, ids, n_env, P);
    hipLaunchKernelGGL(k_pk_finish<T>, dim3(n_env), dim3(64), m->Lf.bytes, st, Mf, ids, *s, *e, action, obs, reward,
                       terminated, truncated, final_obs, autoreset, seed, env_offset, n_env, mask, P, banks, k);
  }
  dispatch_epl(pk_epl(M), [&](auto epl) {
    hipLaunchKernelGGL((k_pk_settle<T, decltype(epl)::value>), dim3(fixup_grid(n_env)), dim3(64), pk_settle_lds(m, P), st,
                       Ms, Mf, ids, *s, *e, (const T*)nullptr, obs, seed, env_offset, n_env, (const uint8_t*)nullptr, P,
                       (int)SETTLE_FIXUP, M.iterations, M.tolerance, scale);
  });
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

template <typename T>
int reset_staged(const mgx_model* m, const DevModel<T>& M, const DevModel<T>& Ms, const DevModel<T>& Mf,
                 const ParkourIds<T>& ids, const mgx_state* s, const mgx_parkour_env* e, const T* draws, float* obs,
                 uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st) {
  Pipe P;
  if (int rc = task_pipe_checked(kParkourStaged, m, e->workspace, e->workspace_bytes, n_env, e->banks, &P)) return rc;
  const T scale = staged_scale(M);
  dispatch_epl(pk_epl(M), [&](auto epl) {
    hipLaunchKernelGGL((k_pk_settle<T, decltype(epl)::value>), dim3(n_env), dim3(64), pk_settle_lds(m, P), st, Ms, Mf, ids,
                       *s, *e, draws, obs, seed, env_offset, n_env, mask, P, (int)SETTLE_RESET, M.iterations, M.tolerance,
                       scale);
  });
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

template <typename T>
int configure_t(const mgx_model* m) {
  Pipe P;
  task_pipe(kParkourStaged, m, nullptr, 1, 1, &P);
  const int pl = staged_pgs_lds_bytes(m, P.maxE, PK_LPS, 0, 8);
  if (pl > 160 * 1024) return host_fail(MGX_E_CAPACITY, "staged parkour solver LDS exceeds 160 KiB");
  int rc = mgx_set_lds(k_pk_rows<T>, m->Ls.bytes) | mgx_set_lds(k_pk_finish<T>, m->Lf.bytes) |
           mgx_set_lds(k_pk_bank_finish<T>, m->Lf.bytes) | mgx_set_lds(k_pk_template<T, true>, m->L.bytes) |
           mgx_set_lds(k_pk_template<T, false>, m->L.bytes);
  const int sl = pk_settle_lds(m, P);
#define MGX_PK_SET(E) rc |= mgx_set_lds(k_pk_settle<T, E>, sl) | mgx_set_lds(k_pgs_groups<T, E, PK_LPS, false>, pl);
  MGX_PK_SET(1) MGX_PK_SET(2) MGX_PK_SET(3) MGX_PK_SET(4)
#undef MGX_PK_SET
  return rc;
}

}  // namespace

namespace mgx {
// The staged parkour step runs the main solver launch only (no wide launch beside it): a model
// (with its hooks) whose pipe would need one is refused here, and the env falls back to the
// monolithic step (envs/parkour.py), which holds the same capacity.
bool parkour_staged_ok(const mgx_model* m) {
  const int nv = m->precision == MGX_F32 ? m->mf.nv : m->md.nv;
  if (!m->staged_ok || nv > 64 || pgs_lanes() != PK_LPS || m->hooks.pgs_lds_b) return false;
  Pipe P;
  task_pipe(kParkourStaged, m, nullptr, 1, 1, &P);
  return !P.sqg && (P.maxE <= P.capE || P.hmain || P.split_blocks);
}

int parkour_staged_configure(const mgx_model* m) {
  if (!parkour_staged_ok(m)) return MGX_OK;
  return m->precision == MGX_F32 ? configure_t<float>(m) : configure_t<double>(m);
}

int parkour_step_staged(const mgx_model* m, const mgx_state* s, const mgx_parkour_env* e, const float* action, float* obs,
                        double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                        uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st) {
  if (int rc = staged_check(kParkourStaged, m, e->banks)) return rc;
  if (m->precision == MGX_F32)
    return step_staged<float>(m, m->mf, m->mfs, m->mff, m->pkf, s, e, action, obs, reward, terminated, truncated,
                              final_obs, autoreset, seed, env_offset, n_env, mask, st);
  return step_staged<double>(m, m->md, m->mds, m->mdf, m->pkd, s, e, action, obs, reward, terminated, truncated,
                             final_obs, autoreset, seed, env_offset, n_env, mask, st);
}

int parkour_reset_staged(const mgx_model* m, const mgx_state* s, const mgx_parkour_env* e, const void* draws,
                         float* obs, uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st) {
  if (int rc = staged_check(kParkourStaged, m, e->banks)) return rc;
  if (m->precision == MGX_F32)
    return reset_staged<float>(m, m->mf, m->mfs, m->mff, m->pkf, s, e, (const float*)draws, obs, seed, env_offset,
                               n_env, mask, st);
  return reset_staged<double>(m, m->md, m->mds, m->mdf, m->pkd, s, e, (const double*)draws, obs, seed, env_offset,
                              n_env, mask, st);
}

int64_t parkour_workspace_bytes(const mgx_model* m, int n_env, int banks) {
  return staged_workspace_bytes(kParkourStaged, m, n_env, banks);
}

int parkour_workspace_init(const mgx_model* m, void* workspace, uint64_t bytes, int n_env, int banks, hipStream_t st) {
  return staged_workspace_init(kParkourStaged, m, workspace, bytes, n_env, banks, st);
}
}  // namespace mgx
