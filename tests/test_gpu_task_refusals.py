"""GPU: what every task's step entry refuses before it launches anything, pinned per task.

The seven mgx_<task>_step entries share one host path (csrc/mgx_task_host.h). Each refusal below
returns MGX_E_ARG with the exact message in mgx_last_error() and launches nothing: an action_f64
other than 0 / 1, autoreset without the episode counter buffer (robotic_arm_assembly takes it: its
kernel guards the counter) and a null obs. A model that was never configured for the task is
refused by name, and steps as any other once it is configured. Soccer's step refuses a struct
without one of the buffers its kernels read unguarded, as the other six tasks' always did.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = {
    "soccer": "SoccerVectorEnv",
    "parkour": "ParkourVectorEnv",
    "bipedal": "BipedalVectorEnv",
    "dancing": "DancingVectorEnv",
    "martial": "MartialArtsVectorEnv",
    "assembly": "AssemblyVectorEnv",
    "construction": "ConstructionVectorEnv",
}


def _make(task):
    import importlib
    mod = importlib.import_module("mujoco_gymnasium_environments_amd.envs." + task)
    return getattr(mod, TASKS[task])(2, precision="f64", autoreset=False)


def _actions(env):
    return torch.zeros(env.num_envs, env.action_space.shape[0], dtype=torch.float32, device=env.device)


def _step(task, env, act, handle=None, state=None, st=None, obs="own", autoreset=0):
    """mgx_<task>_step on the env's buffers, with one argument swapped; (return code, message)"""
    from mujoco_gymnasium_environments_amd.batch import _ptr, stream_handle
    from mujoco_gymnasium_environments_amd.native import lib
    keys = () if task == "assembly" else (env.seed_value, env.env_offset)
    rc = getattr(lib(), f"mgx_{task}_step")(
        handle or env.native.handle, C.byref(state or env.batch.state), C.byref(st if st is not None else env._env),
        _ptr(act), _ptr(env.obs) if obs == "own" else obs, _ptr(env.reward), _ptr(env.terminated),
        _ptr(env.truncated), _ptr(env.final_obs), autoreset, *keys, env.num_envs, None, stream_handle())
    return rc, lib().mgx_last_error().decode()


def _copy(st):
    return type(st).from_buffer_copy(st)


@pytest.mark.parametrize("task", list(TASKS))
def test_step_refusals(task):
    from mujoco_gymnasium_environments_amd import cabi
    env = _make(task)
    act = _actions(env)
    before = env.obs.clone()

    st = _copy(env._env)
    st.action_f64 = 2
    assert _step(task, env, act, st=st) == (cabi.MGX_E_ARG, "action_f64 must be 0 (float32) or 1 (float64)")

    if task != "assembly":  # its kernel guards the counter (mgx_assembly.hip), so it takes autoreset without one
        st = _copy(env._env)
        st.episode = None
        assert _step(task, env, act, st=st, autoreset=1) == (cabi.MGX_E_ARG,
                                                             "autoreset needs the episode counter buffer")

    assert _step(task, env, act, obs=None) == (cabi.MGX_E_ARG, "null argument")

    torch.cuda.synchronize()
    assert torch.equal(env.obs, before)  # nothing was launched


def test_soccer_step_needs_its_env_buffers():
    """the soccer kernels read wind, the previous positions, the step counter, the goal flag and the
    stats unguarded, so the shared path refuses a struct without one, as every other task's does"""
    from mujoco_gymnasium_environments_amd import cabi
    env = _make("soccer")
    act = _actions(env)
    for field in ("wind", "prev_ball_pos", "prev_robot_pos", "step", "goal_scored", "stats"):
        st = _copy(env._env)
        setattr(st, field, None)
        assert _step("soccer", env, act, st=st) == (cabi.MGX_E_ARG, "null soccer env buffer"), field
    env.reset(seed=0)
    for field in ("flags", "rollout"):  # optional: the kernels guard them
        st = _copy(env._env)
        setattr(st, field, None)
        assert _step("soccer", env, act, st=st)[0] == 0, field
    torch.cuda.synchronize()


@pytest.mark.parametrize("task", ["martial", "dancing"])  # one Euler task, one RK4 task
def test_unconfigured_model_is_refused_then_steps(task):
    from mujoco_gymnasium_environments_amd import cabi
    from mujoco_gymnasium_environments_amd.batch import PhysicsBatch, _ptr, stream_handle
    from mujoco_gymnasium_environments_amd.native import check, lib
    env, ref = _make(task), _make(task)
    act = _actions(env)
    fresh = PhysicsBatch(env.model, env.num_envs, precision="f64")  # its model: created, never configured
    h, s = fresh.native.handle, fresh.state
    assert _step(task, env, act, handle=h, state=s) == (cabi.MGX_E_ARG, f"mgx_{task}_configure not called")

    ids = env.tables.ids_struct()
    check(getattr(lib(), f"mgx_{task}_configure")(h, C.byref(ids)), "configure")
    check(getattr(lib(), f"mgx_{task}_reset")(h, C.byref(s), C.byref(env._env), None, _ptr(env.obs), 5, 0,
                                              env.num_envs, None, stream_handle()), "reset")
    rc, msg = _step(task, env, act, handle=h, state=s)
    assert rc == 0, msg
    ref.reset(seed=5)
    ref.step(act)
    torch.cuda.synchronize()
    assert torch.equal(env.obs, ref.obs) and torch.equal(env.reward, ref.reward)
    assert torch.equal(fresh.qpos, ref.batch.qpos)
