// mgx_bank.h — the reset banks and the one-wave settle of the staged tasks (soccer, parkour,
// bipedal), written once.
//
// Same-step autoreset without a serial 10-step settle on the critical path: a reset depends only on
// (seed, global env, episode), so each env keeps R "banks" — the post-settle states of its next R
// episodes — which the task's pipeline advances as extra slots. An env that ends its episode
// installs its ready bank, and that bank restarts for episode + R; a bank that is not ready, and
// reset(), go through the settle kernel: the pipeline's own stages in one wave, compiled in the
// task's translation unit with the task's flags, so a reset has one arithmetic whatever the bank
// count.
//
// A task plugs in with a policy struct B (SoccerBank in mgx_staged.h, ParkourBank in
// mgx_pk_staged.hip, BipedalBank in mgx_rk_staged.hip), compile-time only:
//   Ids, EnvT            the task's ids and mgx_*_env types
//   OBS, DRAWS           floats of an observation, host draws per reset
//   STG                  the records' "rows staged" flags (Pipe.o_bstg) are maintained
//   FIX_CTR, fix_entry, fix_env   the fixup list's counter in Pipe::ctr and its entry encoding
//   draws(e, ids, host, seed, genv, episode) -> Draws   host draws or Philox, as pose() takes them
//   pose(m, e, ids, P, bi, d)     mj_resetData'd data with the reset's randomised pose in e.qpos
//   finalize(m, e, ids, P, bi)    the settled record's observation and prev snapshots
//   track_reset(m, P, ev, env, bi)  the task's tracking reset when a record becomes live
//   settle_step<EPL, LPS>(...)    one settle mj_step of a record in one wave; the tenth (`last`)
//                                 finalizes the record
//   STEP_COUNTS                   settle_step advances the record's settle counter itself (bipedal's
//                                 stage finisher); otherwise settle_reset sets it to 10 at the end
#pragma once
#include "mgx_staged.h"

namespace mgx {

enum { SETTLE_RESET = 0, SETTLE_FIXUP = 1 };

template <typename T>
__device__ __forceinline__ void copy_g(T* dst, const T* src, int n) {
  for (int k = lane_id(); k < n; k += 64) dst[k] = src[k];
}

// record bi restarts for `episode` from the draws d: the pose, zero velocities / warmstart / time,
// settle counter 0. Clobbers the Env's state arrays.
template <typename B, typename T>
__device__ __forceinline__ void bank_restart(const DevModel<T>& m, Env<T>& e, const typename B::Ids& ids, const Pipe& P,
                                             int bi, int episode, uint64_t seed, typename B::Draws d) {
  const int l = lane_id();
  B::pose(m, e, ids, P, bi, d);
  copy_g(P.at<T>(P.o_bq) + (size_t)bi * m.nq, e.qpos, m.nq);
  if (l < m.nv) {
    P.at<T>(P.o_bv)[(size_t)bi * m.nv + l] = 0;
    P.at<T>(P.o_ba)[(size_t)bi * m.nv + l] = 0;
  }
  if (l == 0) {
    P.at<T>(P.o_btime)[bi] = 0;
    P.at<int>(P.o_bwarn)[bi] = 0;
    P.at<int>(P.o_bep)[bi] = episode;
    P.at<uint64_t>(P.o_bseed)[bi] = seed;
    P.at<int>(P.o_bk)[bi] = 0;
    if constexpr (B::STG) P.at<int>(P.o_bstg)[bi] = 0;  // rows staged for the record's earlier state are void
  }
  wsync();
}
// host: the env's host draws (reset(draws=)), or nullptr for Philox keyed by (seed, global env, episode)
template <typename B, typename T>
__device__ __forceinline__ void bank_init(const DevModel<T>& m, Env<T>& e, const typename B::Ids& ids, const Pipe& P,
                                          int env, int bi, int episode, uint64_t seed, int env_offset,
                                          const T* host = nullptr) {
  const typename B::Draws d = B::draws(e, ids, host, seed, (uint32_t)(env_offset + env), (uint32_t)episode);
  bank_restart<B>(m, e, ids, P, bi, episode, seed, d);
}

template <typename T>
__device__ __forceinline__ void bank_store_state(const DevModel<T>& m, Env<T>& e, const Pipe& P, int bi, int warn) {
  wsync();
  int l = lane_id();
  copy_g(P.at<T>(P.o_bq) + (size_t)bi * m.nq, e.qpos, m.nq);
  if (l < m.nv) {
    P.at<T>(P.o_bv)[(size_t)bi * m.nv + l] = e.qvel[l];
    P.at<T>(P.o_ba)[(size_t)bi * m.nv + l] = e.qacc_ws;
  }
  if (l == 0) {
    P.at<T>(P.o_btime)[bi] = e.time;
    P.at<int>(P.o_bwarn)[bi] += warn;
  }
}

// load bank state as an mj_resetData'd MjData (zero controls and applied forces)
template <typename T>
__device__ __forceinline__ void bank_load_state(const DevModel<T>& m, Env<T>& e, const Pipe& P, int bi) {
  int l = lane_id();
  const T* q = P.at<T>(P.o_bq) + (size_t)bi * m.nq;
  for (int k = l; k < m.nq; k += 64) e.qpos[k] = q[k];
  for (int k = l; k < m.nv; k += 64) e.qvel[k] = P.at<T>(P.o_bv)[(size_t)bi * m.nv + k];
  for (int k = l; k < m.nu; k += 64) e.ctrl[k] = 0;
  for (int k = l; k < 6 * m.nbody; k += 64) e.xfrc[k] = 0;
  e.qacc_ws = l < m.nv ? P.at<T>(P.o_ba)[(size_t)bi * m.nv + l] : (T)0;
  e.qfrc_applied = 0;
  e.time = P.at<T>(P.o_btime)[bi];
  wsync();
}

// the settled reset of bank record bi becomes env's live state for episode E: state, zero controls
// and applied forces, obs, the task's tracking reset; episode E + 1
template <typename B, typename T>
__device__ __forceinline__ void bank_copy_live(const DevModel<T>& m, const Pipe& P, mgx_state s, typename B::EnvT ev,
                                               float* obs, int env, int bi, int E) {
  const int l = lane_id();
  copy_g((T*)s.qpos + (size_t)env * m.nq, P.at<T>(P.o_bq) + (size_t)bi * m.nq, m.nq);
  copy_g((T*)s.qvel + (size_t)env * m.nv, P.at<T>(P.o_bv) + (size_t)bi * m.nv, m.nv);
  copy_g((T*)s.qacc_warmstart + (size_t)env * m.nv, P.at<T>(P.o_ba) + (size_t)bi * m.nv, m.nv);
  for (int k = l; k < m.nv; k += 64) ((T*)s.qfrc_applied)[(size_t)env * m.nv + k] = 0;
  for (int k = l; k < m.nu; k += 64) ((T*)s.ctrl)[(size_t)env * m.nu + k] = 0;
  for (int k = l; k < 6 * m.nbody; k += 64) ((T*)s.xfrc_applied)[(size_t)env * 6 * m.nbody + k] = 0;
  copy_g(obs + (size_t)env * B::OBS, P.at<float>(P.o_bobs) + (size_t)bi * B::OBS, B::OBS);
  B::track_reset(m, P, ev, env, bi);
  if (l == 0) {
    ((T*)s.time)[env] = P.at<T>(P.o_btime)[bi];
    if (s.warning) s.warning[env] += P.at<int>(P.o_bwarn)[bi];
    if (ev.episode) ev.episode[env] = E + 1;
  }
  wsync();
}

// Install the ready bank of env `env` into its live state and restart the bank for episode + R.
// Returns false if there is no bank or it is not ready (the caller falls back).
template <typename B, typename T>
__device__ __forceinline__ bool bank_install(const DevModel<T>& m, Env<T>& e, const typename B::Ids& ids, const Pipe& P,
                                             mgx_state s, typename B::EnvT ev, float* obs, uint64_t seed, int env_offset,
                                             int env) {
  if (P.R <= 0) return false;
  const int E = ev.episode[env];
  const int bi = env * P.R + E % P.R;
  const bool ready = P.at<int>(P.o_bk)[bi] == 10 && P.at<int>(P.o_bep)[bi] == E && P.at<uint64_t>(P.o_bseed)[bi] == seed;
  if (!ready) return false;
  bank_copy_live<B>(m, P, s, ev, obs, env, bi, E);
  bank_init<B>(m, e, ids, P, env, bi, E + P.R, seed, env_offset);
  return true;
}
// the same-step autoreset of a finisher: the env's ready bank (banks: the step runs with its banks),
// else the env goes on the fixup list, which the settle kernel works off behind the finisher
template <typename B, typename T>
__device__ __forceinline__ void bank_install_or_list(const DevModel<T>& m, Env<T>& e, const typename B::Ids& ids,
                                                     const Pipe& P, mgx_state s, typename B::EnvT ev, float* obs,
                                                     uint64_t seed, int env_offset, bool banks, int env) {
  const bool ok = banks && bank_install<B>(m, e, ids, P, s, ev, obs, seed, env_offset, env);
  if (!ok && lane_id() == 0) P.at<int>(P.o_fix)[atomicAdd(P.ctr() + B::FIX_CTR, 1)] = B::fix_entry(env);
}

// ------------------------------------------------------------------ one-wave settle
// One Euler settle step of bank record bi in one wave, through pipe slot `slot`: the pipeline's own
// stages in sequence — stage_rows, the PGS of the one slot (pgs_group, lane group 0 of the wave),
// the finisher's finish_physics / checkAcc template / bank store. A reset settled here is
// bit-identical to one settled as extra slots of the pipeline launches, so the fallback for a bank
// that is not ready (and reset()) produces exactly what a ready bank would have: the bank count is
// a performance knob only. Returns with the finisher's Env (layout Mf) in `smem`.
template <typename B, typename T, int EPL, int LPS>
__device__ __forceinline__ void euler_settle_step(const DevModel<T>& Ms, const DevModel<T>& Mf,
                                                  const typename B::Ids& ids, const Pipe& P, char* smem, Env<T>& f,
                                                  int bi, int slot, int maxit, T tol, T scale, bool last) {
  {
    Env<T> e;
    env_bind(Ms, e, smem);
    bind_carry_tail(Ms, e, P, slot);
    bank_load_state(Ms, e, P, bi);
    int warn = 0;  // mj_checkPos / mj_checkVel
    if (any_bad(e.qpos, Ms.nq)) { reset_env(Ms, e); warn++; }
    if (any_bad(e.qvel, Ms.nv)) { reset_env(Ms, e); warn++; }
    stage_rows(Ms, e, P, slot, warn, false);
  }
  __threadfence();
  __syncthreads();
  pgs_group<T, EPL, LPS, false>(P, smem, threadIdx.x < LPS ? slot : -1, P.maxE, maxit, tol, scale, 64 / LPS);
  __threadfence();
  __syncthreads();
  env_bind(Mf, f, smem);
  int warn = load_carry(Mf, f, P, slot);
  if (!finish_physics(Mf, f, P, slot)) {
    load_template(Mf, f, P);
    warn++;
  }
  bank_store_state(Mf, f, P, bi, warn);
  if (last) B::finalize(Mf, f, ids, P, bi);
  __threadfence();
  __syncthreads();
}

// Restart record bi for `episode` (host draws or nullptr for Philox) and settle it: ten mj_steps
// from the randomised pose, after which the record is finalized with counter 10. Its pipe slot is
// the env's live slot.
template <typename B, typename T, int EPL, int LPS>
__device__ __forceinline__ void settle_reset(const DevModel<T>& Ms, const DevModel<T>& Mf, const typename B::Ids& ids,
                                             mgx_state s, typename B::EnvT ev, const Pipe& P, char* smem, int env, int bi,
                                             int episode, const T* host, uint64_t seed, int env_offset, int maxit, T tol,
                                             T scale) {
  {
    Env<T> e;
    env_bind(Ms, e, smem);
    bind_carry_tail(Ms, e, P, env);
    bank_init<B>(Ms, e, ids, P, env, bi, episode, seed, env_offset, host);
  }
  __threadfence();
  __syncthreads();
  Env<T> f;
  for (int t = 0; t < 10; t++)
    B::template settle_step<EPL, LPS>(Ms, Mf, ids, s, ev, P, smem, f, env, bi, env, maxit, tol, scale, t == 9);
  if constexpr (!B::STEP_COUNTS) {
    if (lane_id() == 0) P.at<int>(P.o_bk)[bi] = 10;
    __threadfence();
    __syncthreads();
  }
}

// The settle kernels' body. reset() of a staged batch (SETTLE_RESET: one workgroup per env; with
// Philox draws and banks it also prefills the env's R banks) and the step's fallback for banks that
// were not ready (SETTLE_FIXUP: grid-stride over the finisher's list). Every reset goes through
// settle_reset, the pipeline's arithmetic.
template <typename B, typename T, int EPL, int LPS>
__device__ __forceinline__ void bank_settle(const DevModel<T>& Ms, const DevModel<T>& Mf, const typename B::Ids& ids,
                                            mgx_state s, typename B::EnvT ev, const T* draws, float* obs, uint64_t seed,
                                            int env_offset, int n_env, const uint8_t* mask, const Pipe& P, int mode,
                                            int maxit, T tol, T scale, char* smem) {
  const int cnt = mode == SETTLE_FIXUP ? P.ctr()[B::FIX_CTR] : n_env;
  for (int i = blockIdx.x; i < cnt; i += gridDim.x) {
    const int env = mode == SETTLE_FIXUP ? B::fix_env(P.at<int>(P.o_fix)[i]) : i;
    if (mode == SETTLE_RESET && mask && !mask[env]) continue;
    const int E = ev.episode ? ev.episode[env] : 0;
    const int bi = P.R > 0 ? env * P.R + E % P.R : env;  // R = 0: one scratch record per env
    const T* d = draws ? draws + (size_t)env * B::DRAWS : nullptr;
    settle_reset<B, T, EPL, LPS>(Ms, Mf, ids, s, ev, P, smem, env, bi, E, d, seed, env_offset, maxit, tol, scale);
    bank_copy_live<B>(Mf, P, s, ev, obs, env, bi, E);
    if (P.R > 0 && mode == SETTLE_FIXUP) {
      // as bank_install: the consumed bank restarts for episode E + R (the pipeline settles it)
      Env<T> e;
      env_bind(Ms, e, smem);
      bind_carry_tail(Ms, e, P, env);
      bank_init<B>(Ms, e, ids, P, env, bi, E + P.R, seed, env_offset);
    } else if (P.R > 0 && !draws) {
      // reset(): prefill the banks of episodes E + 1 .. E + R, so the first R terminations never wait
      for (int k = 1; k <= P.R; k++)
        settle_reset<B, T, EPL, LPS>(Ms, Mf, ids, s, ev, P, smem, env, env * P.R + (E + k) % P.R, E + k,
                                     (const T*)nullptr, seed, env_offset, maxit, tol, scale);
    } else if (lane_id() == 0) {
      P.at<int>(P.o_bk)[bi] = -1;  // a scratch record (R = 0, or host draws): nothing to settle
    }
    __threadfence();
    __syncthreads();
  }
}

// The template kernels' tail: mj_step's outcome from mj_resetData'd data (in e) into the arrays
// load_template reads
template <typename T>
__device__ __forceinline__ void template_store(const DevModel<T>& m, Env<T>& e, const Pipe& P) {
  const int l = lane_id();
  for (int k = l; k < m.nq; k += 64) P.at<T>(P.o_tq)[k] = e.qpos[k];
  for (int k = l; k < m.nv; k += 64) P.at<T>(P.o_tv)[k] = e.qvel[k];
  if (l < m.nv) P.at<T>(P.o_ta)[l] = e.qacc_ws;
  for (int k = l; k < 3 * m.nbody; k += 64) { P.at<T>(P.o_tx)[k] = e.xpos[k]; P.at<T>(P.o_tsc)[k] = e.subtree_com[k]; }
  for (int k = l; k < 4 * m.nbody; k += 64) P.at<T>(P.o_txq)[k] = e.xquat[k];
  const int nc = e.ncon < P.maxC ? e.ncon : P.maxC;
  for (int k = l; k < nc; k += 64) {
    P.at<int>(P.o_tcg)[2 * k] = e.con_geom[2 * k];
    P.at<int>(P.o_tcg)[2 * k + 1] = e.con_geom[2 * k + 1];
    P.at<T>(P.o_tcd)[k] = e.con_dist[k];
    P.at<T>(P.o_tcm)[k] = e.con_mu[k];
  }
  if (l == 0) { P.at<int>(P.o_tn)[0] = nc; P.at<T>(P.o_tt)[0] = e.time; }
}

}  // namespace mgx
