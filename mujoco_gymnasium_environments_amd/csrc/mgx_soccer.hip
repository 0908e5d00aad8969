// mgx_soccer.hip — humanoid_soccer: the kernels of the monolithic step (one wave per env), the
// host side of the staged step (its kernels: mgx_pgs.hip) and the mgx_soccer_* C-ABI (include/mgx.h).
#include "mgx_task_host.h"

using namespace mgx;

MGX_PROF_SETTER(mgx_prof_set_buffer)

// ------------------------------------------------------------------------- kernels
// soccer reset body shared by the explicit-reset and autoreset paths: draws (36 values in
// reference order, from the host or from Philox) -> randomised qpos, 10 settle mj_steps, obs.
template <typename T>
__device__ __forceinline__ int soccer_reset_body(const DevModel<T>& m, Env<T>& e, const SoccerIds<T>& ids, const T* draws, T* wind,
                                 T* prev_ball, T* prev_robot, T* stats, int* step, uint8_t* goal, float* obs) {
  soccer_apply_reset(m, e, ids, draws, wind);
  int warn = 0;
  for (int k = 0; k < 10; k++) warn += mj_step_env(m, e);  // soccer_env.py:378-379
  soccer_obs(m, e, ids, 0, obs);
  wsync();
  int l = lane_id();
  if (l < 3) { prev_ball[l] = e.xpos[3 * ids.ball + l]; prev_robot[l] = e.xpos[3 * ids.torso + l]; }
  if (l < 5) stats[l] = 0;
  if (l == 0) { *step = 0; *goal = 0; }
  return warn;
}

// Philox-drawn reset of `env` for its current episode counter, then the counter advances;
// with banks, the bank of the consumed episode restarts for episode + R. Writes the state.
template <typename T>
__device__ __forceinline__ void soccer_reset_philox(const DevModel<T>& m, Env<T>& e, const SoccerIds<T>& ids, mgx_state s,
                                                    mgx_soccer_env ev, float* obs, uint64_t seed, int env_offset, int env,
                                                    const Pipe* P) {
  int l = lane_id();
  int E = ev.episode[env];
  soccer_philox_draws(seed, (uint32_t)(env_offset + env), (uint32_t)E, ids.n_noise, e.vec1);
  wsync();
  int warn = soccer_reset_body(m, e, ids, e.vec1, (T*)ev.wind + 3 * (size_t)env, (T*)ev.prev_ball_pos + 3 * (size_t)env,
                               (T*)ev.prev_robot_pos + 3 * (size_t)env, (T*)ev.stats + 5 * (size_t)env, ev.step + env,
                               ev.goal_scored + env, obs + (size_t)env * 80);
  store_state(m, e, (T*)s.qpos, (T*)s.qvel, (T*)s.qacc_warmstart, (T*)s.ctrl, (T*)s.qfrc_applied, (T*)s.xfrc_applied,
              (T*)s.time, env);
  if (l == 0) {
    if (s.warning) s.warning[env] += warn;
    if (s.overflow && e.overflow) s.overflow[env] += 1;
    ev.episode[env] = E + 1;
  }
  wsync();
  if (P) bank_init<SoccerBank<T>>(m, e, ids, *P, env, env * P->R + E % P->R, E + P->R, seed, env_offset);
}

// One full soccer step of `env` in one wave (pre, mj_step, post, same-step autoreset).
template <typename T>
__device__ __forceinline__ void soccer_step_mono(const DevModel<T>& m, Env<T>& e, const SoccerIds<T>& ids, mgx_state s,
                                                 mgx_soccer_env ev, const float* action, float* obs, double* reward,
                                                 uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                                                 uint64_t seed, int env_offset, int env, const Pipe* P) {
  T* qpos = (T*)s.qpos; T* qvel = (T*)s.qvel; T* qacc = (T*)s.qacc_warmstart; T* ctrl = (T*)s.ctrl;
  T* qfrc = (T*)s.qfrc_applied; T* xfrc = (T*)s.xfrc_applied; T* tm = (T*)s.time;
  load_state(m, e, qpos, qvel, qacc, ctrl, qfrc, xfrc, tm, env);
  T* prev_ball = (T*)ev.prev_ball_pos + 3 * (size_t)env;
  float* o = obs + (size_t)env * 80;
  int l = lane_id();
  const SoccerAct a(action, ev.action_f64, env, m.nu);
  soccer_pre(m, e, ids, a, prev_ball, (T*)ev.wind + 3 * (size_t)env);
  int warn = mj_step_env(m, e);
  bool done = soccer_post(m, e, ids, a, ev.step + env, ev.goal_scored + env, prev_ball,
                          (T*)ev.prev_robot_pos + 3 * (size_t)env, (T*)ev.stats + 5 * (size_t)env, o, reward + env,
                          terminated + env, truncated + env, ev.flags ? ev.flags + 2 * (size_t)env : nullptr);
  if (ev.rollout && l == 0) {
    double* ro = (double*)ev.rollout + 8 * (size_t)env;
    const double ne = e.nefc, it = e.niter;
    ro[0] += reward[env];
    ro[1] += terminated[env];
    ro[2] += truncated[env];
    ro[3] += 1.0;
    ro[4] += ne;
    ro[5] += it;
    ro[6] += ne * ne;
    ro[7] += it * ne * ne;
  }
  store_state(m, e, qpos, qvel, qacc, ctrl, qfrc, xfrc, tm, env);
  if (l == 0 && s.warning) s.warning[env] += warn;
  if (l == 0 && s.overflow && e.overflow) s.overflow[env] += 1;
  if (done && autoreset) {
    if (final_obs)
      for (int i = l; i < 80; i += 64) final_obs[(size_t)env * 80 + i] = o[i];
    __threadfence();
    wsync();
    if (!(P && bank_install<SoccerBank<T>>(m, e, ids, *P, s, ev, obs, seed, env_offset, env)))
      soccer_reset_philox(m, e, ids, s, ev, obs, seed, env_offset, env, P);
  }
}

// soccer, monolithic (one wave per env): MODE 0 = step (+ optional same-step autoreset), MODE 1 =
// reset. A staged batch (workspace) resets through k_soccer_settle instead (mgx_staged.h).
template <typename T, int MODE>
__global__ void __launch_bounds__(64) k_soccer(DevModel<T> m, SoccerIds<T> ids, mgx_state s, mgx_soccer_env ev,
                                               const float* action, const T* draws, float* obs, double* reward,
                                               uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                               int autoreset, uint64_t seed, int env_offset, int n_env,
                                               const uint8_t* mask, Pipe pipe, int use_pipe) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int env = blockIdx.x;
  if (env >= n_env) return;
  if (mask && !mask[env]) return;
  Env<T> e;
  env_bind(m, e, smem);
  const Pipe* P = use_pipe ? &pipe : nullptr;
  if (MODE == 0) {
    soccer_step_mono(m, e, ids, s, ev, action, obs, reward, terminated, truncated, final_obs, autoreset, seed,
                     env_offset, env, P);
    return;
  }
  if (!draws) {
    soccer_reset_philox(m, e, ids, s, ev, obs, seed, env_offset, env, nullptr);
    return;
  }
  T* qpos = (T*)s.qpos; T* qvel = (T*)s.qvel; T* qacc = (T*)s.qacc_warmstart; T* ctrl = (T*)s.ctrl;
  T* qfrc = (T*)s.qfrc_applied; T* xfrc = (T*)s.xfrc_applied; T* tm = (T*)s.time;
  load_state(m, e, qpos, qvel, qacc, ctrl, qfrc, xfrc, tm, env);
  int warn = soccer_reset_body(m, e, ids, draws + (size_t)env * 36, (T*)ev.wind + 3 * (size_t)env,
                               (T*)ev.prev_ball_pos + 3 * (size_t)env, (T*)ev.prev_robot_pos + 3 * (size_t)env,
                               (T*)ev.stats + 5 * (size_t)env, ev.step + env, ev.goal_scored + env,
                               obs + (size_t)env * 80);
  if (ev.episode && lane_id() == 0) ev.episode[env] += 1;
  store_state(m, e, qpos, qvel, qacc, ctrl, qfrc, xfrc, tm, env);
  if (lane_id() == 0 && s.warning) s.warning[env] += warn;
  if (lane_id() == 0 && s.overflow && e.overflow) s.overflow[env] += 1;
}

// mj_step from mj_resetData'd state (the checkAcc template, see load_template)
template <typename T>
__global__ void __launch_bounds__(64) k_soccer_template(DevModel<T> m, Pipe P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Env<T> e;
  env_bind(m, e, smem);
  reset_env(m, e);
  forward(m, e);
  e.qacc_ws = e.qacc;
  euler(m, e);
  template_store(m, e, P);
}

// Env-logic-only test hook: frames/contacts come from the caller (golden vectors generated
// from the reference's own Python), no physics is run.
template <typename T>
__global__ void __launch_bounds__(64) k_soccer_logic(DevModel<T> m, SoccerIds<T> ids, mgx_soccer_logic_io io,
                                                     int n_env) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int env = blockIdx.x;
  if (env >= n_env) return;
  Env<T> e;
  env_bind(m, e, smem);
  int l = lane_id();
  const T* qpos = (const T*)io.qpos + (size_t)env * m.nq;
  const T* qvel = (const T*)io.qvel + (size_t)env * m.nv;
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = qpos[k];
  for (int k = l; k < m.nv; k += 64) e.qvel[k] = qvel[k];
  for (int k = l; k < 3 * m.nbody; k += 64) {
    e.xpos[k] = ((const T*)io.xpos)[(size_t)env * 3 * m.nbody + k];
    e.subtree_com[k] = ((const T*)io.subtree_com)[(size_t)env * 3 * m.nbody + k];
  }
  for (int k = l; k < 4 * m.nbody; k += 64) e.xquat[k] = ((const T*)io.xquat)[(size_t)env * 4 * m.nbody + k];
  for (int k = l; k < 6 * m.nbody; k += 64) e.xfrc[k] = ((T*)io.xfrc_applied)[(size_t)env * 6 * m.nbody + k];
  e.qfrc_applied = l < m.nv ? ((T*)io.qfrc_applied)[(size_t)env * m.nv + l] : (T)0;
  int nc = io.ncon[env];
  e.ncon = nc;
  for (int c = l; c < nc; c += 64) {
    e.con_geom[2 * c] = io.con_geom[((size_t)env * io.max_contacts + c) * 2];
    e.con_geom[2 * c + 1] = io.con_geom[((size_t)env * io.max_contacts + c) * 2 + 1];
    e.con_dist[c] = ((const T*)io.con_dist)[(size_t)env * io.max_contacts + c];
    e.con_mu[c] = ((const T*)io.con_mu)[(size_t)env * io.max_contacts + c];
  }
  wsync();
  const T* stale = (const T*)io.xpos + (size_t)env * 3 * m.nbody + 3 * ids.ball;
  const SoccerAct a(io.action, 0, env, m.nu);
  soccer_pre(m, e, ids, a, stale, (const T*)io.wind + 3 * (size_t)env);
  soccer_post(m, e, ids, a, io.step + env, io.goal_scored + env, (T*)io.prev_ball_pos + 3 * (size_t)env,
              (T*)io.prev_robot_pos + 3 * (size_t)env, (T*)io.stats + 5 * (size_t)env, io.obs + (size_t)env * 80,
              io.reward + env, io.terminated + env, io.truncated + env, io.flags + 2 * (size_t)env);
  wsync();
  if (l < m.nv) ((T*)io.qfrc_applied)[(size_t)env * m.nv + l] = e.qfrc_applied;
  for (int k = l; k < 6 * m.nbody; k += 64) ((T*)io.xfrc_applied)[(size_t)env * 6 * m.nbody + k] = e.xfrc[k];
}

namespace {
// every buffer the soccer kernels dereference unguarded (flags, rollout and episode are optional)
bool soccer_env_ok(const mgx_soccer_env* e) {
  return e->prev_ball_pos && e->prev_robot_pos && e->wind && e->step && e->goal_scored && e->stats;
}

constexpr Task<mgx_soccer_env> kTask{"soccer", "soccer", &mgx_model::soccer_ok, soccer_env_ok, false};
// rows in LDS only (mgx_soccer_configure refuses the others): one kernel per MODE, named in both row placements
template <typename T>
constexpr auto kKernels = task_kernels(k_soccer<T, 0>, k_soccer<T, 0>, k_soccer<T, 1>, k_soccer<T, 1>, k_soccer_logic<T>);

}  // namespace

// ------------------------------------------------------------------------- host side
static int pgs_lds_bytes(const mgx_model* m, int rows, int sqg = 0) {
  return staged_pgs_lds_bytes(m, rows, pgs_lanes(), sqg, mgx_twl(false));
}

// The bank pipeline's stream (MGX_BANK_STREAM) and its events per caller stream, created once and
// kept for the process: the lowest stream priority the device offers, so the live step's waves are
// dispatched first. nullptr if the runtime refuses (then the step runs on one stream).
struct BankStream {
  hipStream_t s;
  hipEvent_t entry, rows, live, done;
};
static BankStream* bank_stream(hipStream_t st) {
  return stream_cache<BankStream>(st, [](BankStream& x) {
    int least = 0, greatest = 0;
    const bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
                    hipStreamCreateWithPriority(&x.s, hipStreamNonBlocking, least) == hipSuccess &&
                    hipEventCreateWithFlags(&x.entry, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&x.rows, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&x.live, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&x.done, hipEventDisableTiming) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
  });
}
// The bank view of a pipe: the bank slots' own solver-list state (Pipe, mgx_staged.h); no bank
// wave raises its priority
static Pipe bank_view(const Pipe& P) {
  Pipe B = P;
  B.o_ctr = P.o_ctr2; B.o_hist = P.o_hist2; B.o_blist = P.o_blist2; B.o_k2list = P.o_k2list2; B.o_k2big = P.o_k2big2;
  B.S = P.N * (P.R > 0 ? P.R : 1);
  B.prio_rows = P.maxE;
  B.qmh_pre = 0;  // bank records end no step
  return B;
}
// soccer's workspace_init has never refused a model outside the staged pipeline (init_checks)
static const StagedTask kSoccerStaged = {"soccer", [](const mgx_model* m) { return m->staged_ok; },
                                         "staged step: model exceeds the staged solver's capacity", false, false, 80,
                                         MGX_PGS_SPLIT_BLOCKS,
                                         {k_soccer_template<float>, k_soccer_template<float>},
                                         {k_soccer_template<double>, k_soccer_template<double>}};
static int settle_lds_bytes(const mgx_model* m, const Pipe& P) {
  return staged_settle_lds(m, P, pgs_lanes(), 0, mgx_twl(false));
}

// mgx_model_create: every model gets the soccer kernels' dynamic-LDS attributes (so workspace_init
// runs without mgx_soccer_configure), a staged model the staged pipeline's as well
int mgx::soccer_kernels_configure(const mgx_model* m) {
  const int rc = task_configure_lds(m, kKernels<float>, kKernels<double>) |
                 (m->precision == MGX_F32 ? mgx_set_lds(k_soccer_template<float>, m->L.bytes)
                                          : mgx_set_lds(k_soccer_template<double>, m->L.bytes));
  if (rc != MGX_OK || !m->staged_ok) return rc;
  const int sl = std::max({pgs_lds_bytes(m, m->Ls.max_nefc), m->Ls.bytes, m->Lf.bytes});  // settle_lds_bytes
  if (int r = staged_kernels_configure(m->precision, m->Ls.bytes, m->Lf.bytes, sl)) return r;
  int pl = pgs_lds_bytes(m, m->Ls.max_nefc);  // the global-B launch's
  if (pl < 96 * 1024) pl = 96 * 1024;  // the arena (MGX_PGS_ARENA tuning up to 96 KiB)
  if (pl > 160 * 1024) return host_fail(MGX_E_CAPACITY, "solver LDS exceeds 160 KiB: lower MGX_MAX_NEFC");
  return pgs_configure_lds(m->precision, pl, wide_arena_bytes(m) + 64);
}

// What one staged soccer step runs beside its rows -> PGS -> finish -> fixup, decided from the
// model's hooks and the pipe, whose per-step fields (qmh_pre, prio_rows) it sets.
struct SoccerPlan {
  bool one;          // every slot fits the main launch (the default capacity): no wide launch at all
  int bmode;         // the bank pipeline's mode, 0 without it
  BankStream* bs;    // the bank pipeline's stream (MGX_BANK_STREAM), or null
  SideStream *tail, *side;  // the tail finisher's side stream (MGX_TAIL_FINISH) and the wide launch's, or null
  int rlds, mlds, wgrid, wlds;  // LDS of a row-builder wave and a main-launch solver wave; the wide launch
};
static SoccerPlan soccer_step_plan(const mgx_model* m, Pipe& P, int banks, hipStream_t st) {
  const Hooks& H = m->hooks;
  SoccerPlan p{};
  // occupancy probe: MGX_ROWS_LDS pads the row builder's LDS (fewer waves per CU; up to 64 KiB)
  p.rlds = H.rows_lds > m->Ls.bytes && H.rows_lds <= 64 * 1024 ? H.rows_lds : m->Ls.bytes;
  p.one = !H.pgs_lds_b && (P.maxE <= P.capE || P.hmain || P.split_blocks);
  // both companions need the one-launch solver and the side stream, the tail finisher also split waves
  const bool beside = p.one && H.side_stream && !H.pgs_single;
  const bool tail_on = beside && P.split_blocks > 0 && (H.tail_finish >= 0 ? H.tail_finish : MGX_TAIL_FINISH);
  // MGX_BANK_STREAM not set: on in fp64; in fp32 on with the tail finisher only (alone it measured
  // 2% slower there, with the tail finisher 6% faster than one stream)
  p.bmode = banks > 0 && beside
                ? (H.bank_stream >= 0 ? H.bank_stream : m->precision == MGX_F32 && !tail_on ? 0 : MGX_BANK_STREAM) : 0;
  p.bs = p.bmode ? bank_stream(st) : nullptr;
  if (!p.bs) p.bmode = 0;
  // Without the bank stream the bank slots share the one solver list: the bank finisher then
  // follows V, before tier B; that layout measured 10% slower than the one launch (fp32), so it
  // runs only when MGX_TAIL_FINISH=1 asks for it.
  p.tail = tail_on && (p.bs || H.tail_finish == 1) ? side_stream(st) : nullptr;
  // tier B's waves are the step's last: the row builder takes euler()'s qMH factorisation off them
  if (p.tail) P.qmh_pre = H.tail_factor;
  // with the bank waves beside them, all the row-split waves (the launch's long chains) take
  // their SIMD first; MGX_PGS_PRIO_ROWS sets the threshold for A/B runs
  if (p.bs && !H.pgs_prio_rows && P.split_blocks) P.prio_rows = 4 * P.split_blocks - 1;
  p.mlds = H.pgs_lds_b ? P.arena : pgs_lds_bytes(m, P.capE, P.sqg);
  if (P.hmain) p.mlds = std::max(p.mlds, pgs_lds_bytes(m, P.maxE, 1));  // the heavy slots' SQG layout
  // a split wave's one slot of up to maxE rows (larger only under the MGX_PGS_LDS_ROWS test hook)
  if (P.split_blocks) p.mlds = std::max(p.mlds, staged_pgs_lds_bytes(m, P.maxE, 64, 0, mgx_twl(false)));
  // occupancy probe: MGX_PGS_LDS_PAD pads the main solver launch's LDS (fewer waves per CU)
  if (H.pgs_lds_pad > p.mlds && H.pgs_lds_pad <= 96 * 1024) p.mlds = H.pgs_lds_pad;
  // slots over the main launch's LDS rows (MuJoCo has no cap: the rows are kept, not dropped): the
  // wide launch, a small grid-stride global-B launch with maxE rows of LDS per slot, which exits at
  // once when the list is empty. It runs on a side stream beside the main launch (a slot of ~300
  // rows is one wave's 50-sweep chain, which would otherwise trail the main launch). With the
  // LDS-arena main launch (MGX_PGS_LDS_B) it also takes the waves that did not fit their arena, so
  // it follows the main launch there.
  p.side = !p.one && !H.pgs_lds_b && H.side_stream ? side_stream(st) : nullptr;
  p.wgrid = 64 / pgs_lanes() * MGX_PGS_WIDE_GRID, p.wlds = pgs_lds_bytes(m, P.maxE);
  return p;
}

// The staged soccer step (plan: soccer_step_plan), one sequence on the caller's stream with two
// optional companions. The bank pipeline (bs): the bank slots are not needed by this step and their
// chains are short, while the live envs' longest chain sets the solver launch's length and leaves
// most of the GPU idle at its end. So the bank slots' rows -> PGS -> bank finisher run on their own
// lowest-priority stream, over the bank view of the pipe, beside the live launches:
//
//   caller:  E  rows(live) -> PGS(live) ---------> [1: wait D] finish -> fixup -> L  [2: wait D]
//   bank:    wait E  rows(bank) -> R -> PGS(bank) -> [2: wait L] bank finish -> D
//
// E orders the bank stream behind the previous call's bank_install and reset(). Mode 1: a bank
// completing its tenth step is ready for this step's resets, as on one stream. Mode 2: the bank
// finisher follows the live finisher and the fixup (both restart bank records, which the bank
// finisher must not be writing meanwhile; it then skips the restarted records, o_bstg), so a bank
// is ready one step later and only the bank finisher is left on the live path; the live finisher
// waits for R, because the bank row builder reads the records it restarts. Either way the call
// returns with the caller's stream behind all bank work (the workspace is the caller's). Readiness
// depends on step counts only, and a reset is the same bits whether its bank was ready or not, so
// no mode changes a result. The tail finisher (tail): the solver launch is as long as its heaviest
// slot's chain, and an env's finish needs only that env's solver result. So the heavy (row-split)
// slots' waves go to a side stream behind event H, and the finisher runs in two tiers:
//
//   caller:  E  rows(live) H -> PGS(bulk) -> finish A ------> [wait V, 1: D, 2: R] finish B -> fixup -> L
//   side:    wait H  PGS(heavy) -> V
//   bank:    wait E  rows(bank) -> R -> PGS(bank) -> [2: wait L] bank finish -> D
//
// Tier A finishes the light envs beside the heavy chains. It restarts no bank record and leaves
// the solver lists alone (the heavy launch reads them): an env that ended its episode is put on
// the deferred list, so tier A is ordered against nothing but the bulk launch. Tier B finishes the
// heavy envs, installs the deferred resets and clears the lists; it sits where the one finisher
// sat (behind D or R), so bank records are restarted exactly where they were. Each env's finish is
// the same code on the same inputs in either tier. The wide launch (plan.one false) excludes both.
template <typename T>
static int soccer_step_staged(const mgx_model* m, const DevModel<T>& M, const DevModel<T>& Ms, const DevModel<T>& Mf,
                              const SoccerIds<T>& ids, const mgx_state* s, const mgx_soccer_env* e, const float* action,
                              float* obs, double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                              int autoreset, uint64_t seed, int env_offset, int n_env, const uint8_t* mask,
                              hipStream_t st) {
  Pipe P;
  if (int rc = task_pipe_checked(kSoccerStaged, m, e->workspace, e->workspace_bytes, n_env, e->banks, &P)) return rc;
  const int banks = autoreset ? e->banks : 0;
  const SoccerPlan plan = soccer_step_plan(m, P, banks, st);
  BankStream* const bs = plan.bs;
  SideStream *const tail = plan.tail, *const side = plan.side;
  const Pipe B = bank_view(P);
  const int live = bs ? n_env : n_env * (1 + banks), nbank = n_env * P.R, bmode = plan.bmode, mlds = plan.mlds;
  const T scale = staged_scale(M);
  auto pgs = [&](const Pipe& Q, int n, int lds, hipStream_t q, int big, int part) {
    launch_pgs<T>(Q, n, lds, q, M.iterations, M.tolerance, scale, big, m->hooks, part);
  };
  auto finish = [&](bool bank_too, int tier) {
    launch_soccer_finish<T>(Mf, ids, *s, *e, action, obs, reward, terminated, truncated, final_obs, autoreset, seed,
                            env_offset, n_env, mask, P, banks, m->Lf.bytes, st, bank_too, tier);
  };
  if (bs) MGX_HIPCHK(hipEventRecord(bs->entry, st));
  launch_soccer_rows<T>(Ms, ids, *s, *e, action, n_env, mask, P, bs ? 0 : banks, live, plan.rlds, st);
  if (tail) {  // the heavy slots (without the bank stream: of either kind, on the one solver list)
    MGX_HIPCHK(hipEventRecord(tail->rows, st));
    MGX_HIPCHK(hipStreamWaitEvent(tail->s, tail->rows, 0));
    pgs(P, live, mlds, tail->s, 0, 1);
    MGX_HIPCHK(hipEventRecord(tail->big, tail->s));
  }
  if (bs) {
    MGX_HIPCHK(hipStreamWaitEvent(bs->s, bs->entry, 0));
    launch_soccer_rows<T>(Ms, ids, *s, *e, action, n_env, nullptr, B, banks, nbank, plan.rlds, bs->s, n_env);
    if (bmode == 2) MGX_HIPCHK(hipEventRecord(bs->rows, bs->s));
    pgs(B, nbank, mlds, bs->s, 0, 0);
    if (bmode == 1) {
      launch_soccer_bank_finish<T>(Mf, ids, n_env, B, 1, m->Lf.bytes, bs->s);
      MGX_HIPCHK(hipEventRecord(bs->done, bs->s));
    }
  }
  if (side) {  // the wide launch beside the main one
    MGX_HIPCHK(hipEventRecord(side->rows, st));
    MGX_HIPCHK(hipStreamWaitEvent(side->s, side->rows, 0));
    pgs(P, plan.wgrid, plan.wlds, side->s, 1, 0);
    MGX_HIPCHK(hipEventRecord(side->big, side->s));
  }
  pgs(P, live, mlds, st, 0, tail ? 2 : 0);
  if (side) MGX_HIPCHK(hipStreamWaitEvent(st, side->big, 0));
  else if (!plan.one) pgs(P, plan.wgrid, plan.wlds, st, 1, 0);  // ... or after it
  if (tail) {
    finish(false, 1);  // tier A
    MGX_HIPCHK(hipStreamWaitEvent(st, tail->big, 0));
  }
  if (bs) MGX_HIPCHK(hipStreamWaitEvent(st, bmode == 1 ? bs->done : bs->rows, 0));
  finish(!bs, tail ? 2 : 0);
  // the fixup: resets whose bank was not ready, one wave each; exits at once when the list is empty
  launch_soccer_settle<T>(Ms, Mf, ids, *s, *e, (const T*)nullptr, obs, seed, env_offset, n_env, nullptr, P, SETTLE_FIXUP,
                          fixup_grid(n_env), settle_lds_bytes(m, P), st, M.iterations, M.tolerance, scale);
  if (bmode == 2) {
    MGX_HIPCHK(hipEventRecord(bs->live, st));
    MGX_HIPCHK(hipStreamWaitEvent(bs->s, bs->live, 0));
    launch_soccer_bank_finish<T>(Mf, ids, n_env, B, 1, m->Lf.bytes, bs->s);
    MGX_HIPCHK(hipEventRecord(bs->done, bs->s));
    MGX_HIPCHK(hipStreamWaitEvent(st, bs->done, 0));
  }
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

// reset() of a staged batch: every env's reset (and, with Philox draws, its R banks) settled by
// the pipeline's stages in one wave (k_soccer_settle), so the staged batch has one arithmetic for
// every reset, whatever the bank count
template <typename T>
static int soccer_reset_staged(const mgx_model* m, const DevModel<T>& M, const DevModel<T>& Ms, const DevModel<T>& Mf,
                               const SoccerIds<T>& ids, const mgx_state* s, const mgx_soccer_env* e, const T* draws,
                               float* obs, uint64_t seed, int env_offset, int n_env, const uint8_t* mask, hipStream_t st) {
  Pipe P;
  if (int rc = task_pipe_checked(kSoccerStaged, m, e->workspace, e->workspace_bytes, n_env, e->banks, &P)) return rc;
  const T scale = staged_scale(M);
  launch_soccer_settle<T>(Ms, Mf, ids, *s, *e, draws, obs, seed, env_offset, n_env, mask, P, SETTLE_RESET, n_env,
                          settle_lds_bytes(m, P), st, M.iterations, M.tolerance, scale);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

template <typename T>
static void fill_ids(SoccerIds<T>& o, const mgx_soccer_ids* ids) {
  o.torso = ids->torso; o.ball = ids->ball; o.goalkeeper = ids->goalkeeper; o.ball_geom = ids->ball_geom;
  o.right_foot = ids->right_foot; o.left_foot = ids->left_foot; o.field_geom = ids->field_geom;
  o.ball_qposadr = ids->ball_qposadr; o.ball_dofadr = ids->ball_dofadr; o.gk_qposadr = ids->gk_qposadr;
  o.gk_qfrc_index = ids->gk_dofadr; o.max_episode_steps = ids->max_episode_steps;
  for (int i = 0; i < 25; i++) {
    o.obs_qposadr[i] = ids->obs_jnt_qposadr[i];
    o.obs_dofadr[i] = ids->obs_jnt_dofadr[i];
    o.obs_lo[i] = (T)ids->obs_jnt_range[2 * i];
    o.obs_hi[i] = (T)ids->obs_jnt_range[2 * i + 1];
  }
  o.robot_mask_lo = ids->robot_geom_mask_lo;
  o.robot_mask_hi = ids->robot_geom_mask_hi;
}

extern "C" {

int mgx_soccer_configure(mgx_model* m, const mgx_soccer_ids* ids) {
  if (!m || !ids) return host_fail(MGX_E_ARG, "null argument");
  if (m->wide) return host_fail(MGX_E_UNSUPPORTED, MGX_WIDE_MSG);
  if (m->L.gB || (m->precision == MGX_F32 ? m->mf.integrator : m->md.integrator) != 0)
    return host_fail(MGX_E_UNSUPPORTED, "the soccer kernels need an Euler model whose rows fit LDS");
  if ((m->precision == MGX_F32 ? m->mf.solver : m->md.solver) != 0)
    return host_fail(MGX_E_UNSUPPORTED, "the soccer kernels solve with PGS (soccer_env.py:150-151)");
  if (ids->max_episode_steps <= 0) return host_fail(MGX_E_ARG, "max_episode_steps must be > 0");
  if (m->precision == MGX_F32) fill_ids(m->sf, ids);
  else fill_ids(m->sd, ids);
  m->soccer_ok = true;
  return MGX_OK;
}

// Reset-specific tables (noise joints) ride in the same ids struct; set via this helper.
int mgx_soccer_configure_reset(mgx_model* m, int root_qposadr, int n_noise, const int32_t* noise_qposadr,
                               const double* noise_range) {
  if (!m || n_noise < 0 || n_noise > 29 || (n_noise && (!noise_qposadr || !noise_range)))
    return host_fail(MGX_E_ARG, "bad reset table");
  auto fill = [&](auto& o) {
    o.root_qposadr = root_qposadr;
    o.n_noise = n_noise;
    for (int i = 0; i < n_noise; i++) {
      o.noise_qposadr[i] = noise_qposadr[i];
      o.noise_lo[i] = noise_range[2 * i];
      o.noise_hi[i] = noise_range[2 * i + 1];
    }
  };
  if (m->precision == MGX_F32) fill(m->sf); else fill(m->sd);
  return MGX_OK;
}

int mgx_soccer_step(const mgx_model* m, const mgx_state* s, const mgx_soccer_env* e, const float* action, float* obs,
                    double* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset,
                    uint64_t seed, int env_offset, int n_env, const uint8_t* mask, void* stream) {
  if (int rc = task_check_step(kTask, m, s, e, action && obs && reward && terminated && truncated, autoreset, n_env))
    return rc < 0 ? rc : MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (e->workspace) {
    if (int rc = staged_check(kSoccerStaged, m, e->banks)) return rc;
    if (m->precision == MGX_F32)
      return soccer_step_staged<float>(m, m->mf, m->mfs, m->mff, m->sf, s, e, action, obs, reward, terminated,
                                       truncated, final_obs, autoreset, seed, env_offset, n_env, mask, st);
    return soccer_step_staged<double>(m, m->md, m->mds, m->mdf, m->sd, s, e, action, obs, reward, terminated, truncated,
                                      final_obs, autoreset, seed, env_offset, n_env, mask, st);
  }
  return task_launch(m, s, kKernels<float>, kKernels<double>, m->sf, m->sd, 0, n_env, st, *e, action, RealPtr{nullptr},
                     obs, reward, terminated, truncated, final_obs, autoreset, seed, env_offset, n_env, mask, Pipe{}, 0);
}

int mgx_soccer_reset(const mgx_model* m, const mgx_state* s, const mgx_soccer_env* e, const void* draws, float* obs,
                     uint64_t seed, int env_offset, int n_env, const uint8_t* mask, void* stream) {
  if (int rc = task_check_reset(kTask, m, s, e, obs, !draws, n_env)) return rc < 0 ? rc : MGX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (e->workspace) {
    if (int rc = staged_check(kSoccerStaged, m, e->banks)) return rc;
    if (m->precision == MGX_F32)
      return soccer_reset_staged<float>(m, m->mf, m->mfs, m->mff, m->sf, s, e, (const float*)draws, obs, seed,
                                        env_offset, n_env, mask, st);
    return soccer_reset_staged<double>(m, m->md, m->mds, m->mdf, m->sd, s, e, (const double*)draws, obs, seed,
                                       env_offset, n_env, mask, st);
  }
  return task_launch(m, s, kKernels<float>, kKernels<double>, m->sf, m->sd, 1, n_env, st, *e, nullptr, RealPtr{draws},
                     obs, nullptr, nullptr, nullptr, nullptr, 0, seed, env_offset, n_env, mask, Pipe{}, 0);
}

int64_t mgx_soccer_workspace_bytes(const mgx_model* m, int n_env, int banks) {
  return staged_workspace_bytes(kSoccerStaged, m, n_env, banks);
}

int mgx_soccer_workspace_layout(const mgx_model* m, int n_env, int banks, int64_t* out, int n_out) {
  if (!m || !out || n_env <= 0 || banks < 0 || banks > 16 || n_out < 10) return host_fail(MGX_E_ARG, "bad argument");
  if (!m->staged_ok) return host_fail(MGX_E_UNSUPPORTED, "staged step: model exceeds the staged solver's capacity");
  Pipe P;
  task_pipe(kSoccerStaged, m, nullptr, n_env, banks, &P);
  // [11], [12]: the bank view's counter block and arrival list (MGX_BANK_STREAM); [13], [14]: the
  // deferred-reset list and the row-split threshold in blocks (MGX_TAIL_FINISH)
  const int64_t v[15] = {(int64_t)P.o_ctr, (int64_t)P.o_ne, (int64_t)P.o_k2list, (int64_t)P.o_blk, (int64_t)P.o_B,
                         P.bcap, P.maxE, P.capE, P.S, m->precision == MGX_F32 ? 4 : 8, (int64_t)P.o_k2big,
                         (int64_t)P.o_ctr2, (int64_t)P.o_k2list2, (int64_t)P.o_defer, P.split_blocks};
  for (int i = 0; i < (n_out < 15 ? n_out : 15); i++) out[i] = v[i];
  return MGX_OK;
}

int mgx_soccer_workspace_init(const mgx_model* m, void* workspace, uint64_t bytes, int n_env, int banks, void* stream) {
  return staged_workspace_init(kSoccerStaged, m, workspace, bytes, n_env, banks, (hipStream_t)stream);
}

int mgx_soccer_logic_test(const mgx_model* m, const mgx_soccer_logic_io* io, int n_env, void* stream) {
  if (!m || !io) return host_fail(MGX_E_ARG, "null argument");
  if (!m->soccer_ok) return host_fail(MGX_E_ARG, "mgx_soccer_configure not called");
  if (io->max_contacts > m->L.max_ncon) return host_fail(MGX_E_CAPACITY, "max_contacts exceeds the contact capacity");
  if (n_env <= 0) return MGX_OK;
  return task_launch_logic(m, kKernels<float>, kKernels<double>, m->sf, m->sd, n_env, (hipStream_t)stream, *io, n_env);
}

}  // extern "C"
