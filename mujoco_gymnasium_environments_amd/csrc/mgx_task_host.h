// mgx_task_host.h — the host path the seven tasks' C-ABI entries share (mgx_soccer.hip;
// mgx_parkour.hip, mgx_bipedal.hip, mgx_dancing.hip, mgx_martial.hip, mgx_assembly.hip,
// mgx_construction.hip): what a step / reset / logic-test call is refused for, in one order and with
// one set of messages, and the precision x rows-in-scratch choice of the kernel to launch, made from
// the table of instantiations the kernels' LDS attributes were set from. Host code only: a task
// keeps its kernels, its configure checks and its *_env_ok.
#pragma once
#include "mgx_internal.h"

namespace mgx {

// What a task brings to the shared checks.
template <typename EnvT>
struct Task {
  const char* name;             // "mgx_<name>_configure not called"
  const char* label;            // "null <label> env buffer"
  bool mgx_model::*configured;  // set by mgx_<name>_configure
  bool (*env_ok)(const EnvT*);  // every env buffer the kernels dereference unguarded is there
  bool episode_guarded;         // the kernels guard the episode counter: autoreset runs without one
};

// a passed check with no env to run: the entry returns MGX_OK without launching
constexpr int kNoEnvs = 1;

// null arguments, configured, env buffers (the head of every entry; all of a logic test's)
template <typename EnvT>
int task_check(const Task<EnvT>& t, const mgx_model* m, const EnvT* e, bool args, bool step = false) {
  if (!m || !e || !args) return host_fail(MGX_E_ARG, "null argument");
  if (step && e->action_f64 != 0 && e->action_f64 != 1)
    return host_fail(MGX_E_ARG, "action_f64 must be 0 (float32) or 1 (float64)");
  if (!(m->*t.configured)) return host_fail(MGX_E_ARG, std::string("mgx_") + t.name + "_configure not called");
  if (!t.env_ok(e)) return host_fail(MGX_E_ARG, std::string("null ") + t.label + " env buffer");
  return MGX_OK;
}

// mgx_<task>_step: `args` = every pointer argument of the entry is there. MGX_OK: launch; kNoEnvs:
// return MGX_OK; < 0: refused. The caller's staged branch (e->workspace) comes after it.
template <typename EnvT>
int task_check_step(const Task<EnvT>& t, const mgx_model* m, const mgx_state* s, const EnvT* e, bool args,
                    int autoreset, int n_env) {
  if (int rc = task_check(t, m, e, args, true)) return rc;
  if (autoreset && !t.episode_guarded && !e->episode)
    return host_fail(MGX_E_ARG, "autoreset needs the episode counter buffer");
  if (int rc = host_check_state(s)) return rc;
  return n_env <= 0 ? kNoEnvs : MGX_OK;
}

// mgx_<task>_reset: `device_draws` = the reset draws come from Philox keyed by the episode counter
template <typename EnvT>
int task_check_reset(const Task<EnvT>& t, const mgx_model* m, const mgx_state* s, const EnvT* e, bool args,
                     bool device_draws, int n_env) {
  if (int rc = task_check(t, m, e, args)) return rc;
  if (device_draws && !e->episode) return host_fail(MGX_E_ARG, "device draws need the episode counter buffer");
  if (int rc = host_check_state(s)) return rc;
  return n_env <= 0 ? kNoEnvs : MGX_OK;
}

// One task's kernel instantiations for one real type: the monolithic kernel by [MODE: 0 step,
// 1 reset][rows in LDS, rows in scratch] with MODE's block size, and the logic-test kernel. A task
// whose kernel has one row placement (soccer: LDS; construction: scratch) names it in both slots.
template <typename Fn, typename LogicFn>
struct TaskKernels {
  Fn mono[2][2];
  int threads[2];
  LogicFn logic;
};
template <typename Fn, typename LogicFn>
constexpr TaskKernels<Fn, LogicFn> task_kernels(Fn step_lds, Fn step_gb, Fn reset_lds, Fn reset_gb, LogicFn logic,
                                                int step_threads = 64, int reset_threads = 64) {
  return {{{step_lds, step_gb}, {reset_lds, reset_gb}}, {step_threads, reset_threads}, logic};
}

// a caller's `const void*` array of reals, converted to the launched kernel's `const T*` parameter
struct RealPtr {
  const void* p;
  template <typename T>
  operator const T*() const { return static_cast<const T*>(p); }
};

// the dynamic-LDS attribute of every kernel of the table that task_launch / task_launch_logic pick from
template <typename KF, typename KD>
int task_configure_lds(const mgx_model* m, const KF& kf, const KD& kd) {
  auto all = [&](const auto& k) {
    int rc = mgx_set_lds(k.logic, m->L.bytes);
    for (int mode = 0; mode < 2; mode++)
      for (int gb = 0; gb < 2; gb++) rc |= mgx_set_lds(k.mono[mode][gb], m->L.bytes);
    return rc;
  };
  return m->precision == MGX_F32 ? all(kf) : all(kd);
}

// The monolithic launch of `mode` for the model's precision and row placement: kernel(DevModel,
// ids, state, a...). The scratch test is the last refusal of the monolithic path.
template <typename KF, typename KD, typename IdsF, typename IdsD, typename... A>
int task_launch(const mgx_model* m, const mgx_state* s, const KF& kf, const KD& kd, const IdsF& idsf, const IdsD& idsd,
                int mode, int n_env, hipStream_t st, const A&... a) {
  if (int rc = host_check_scratch(m, s)) return rc;
  const int gb = m->L.gB ? 1 : 0;
  if (m->precision == MGX_F32)
    hipLaunchKernelGGL(kf.mono[mode][gb], dim3(n_env), dim3(kf.threads[mode]), m->L.bytes, st, m->mf, idsf, *s, a...);
  else
    hipLaunchKernelGGL(kd.mono[mode][gb], dim3(n_env), dim3(kd.threads[mode]), m->L.bytes, st, m->md, idsd, *s, a...);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

// the logic-test launch: kernel(DevModel, ids, a...), one wave per env
template <typename KF, typename KD, typename IdsF, typename IdsD, typename... A>
int task_launch_logic(const mgx_model* m, const KF& kf, const KD& kd, const IdsF& idsf, const IdsD& idsd, int n_env,
                      hipStream_t st, const A&... a) {
  if (m->precision == MGX_F32)
    hipLaunchKernelGGL(kf.logic, dim3(n_env), dim3(64), m->L.bytes, st, m->mf, idsf, a...);
  else
    hipLaunchKernelGGL(kd.logic, dim3(n_env), dim3(64), m->L.bytes, st, m->md, idsd, a...);
  MGX_HIPCHK(hipGetLastError());
  return MGX_OK;
}

}  // namespace mgx
