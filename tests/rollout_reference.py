"""numpy reference for mgx_rollout (TEST INFRASTRUCTURE ONLY): MuJoCo's mujoco.rollout [ext] as
include/mgx.h restates it — written against that text, not the HIP code.

``rollout`` loops a simulator's own step over K control sequences from one env's state and applies
the header's rules: the state vector [time, qpos, qvel], the zero-order hold of ``hold`` recorded
steps per knot, ``nsub`` substeps per recorded step, and stop-and-pad on divergence (a recorded step
that raises the simulator's ``warning`` count ends the rollout: n_done = t and rows t .. T-1 repeat
what that step left behind). The simulator is anything with numpy views ``time``, ``qpos``, ``qvel``,
``qacc_warmstart``, ``ctrl``, ``warning`` and a ``step(n)``: the CPU oracle (``oracle_sim``) or a
scripted stand-in (tests/test_rollout_cpu.py), which pins the divergence rule without physics.
"""
import numpy as np

from tests.helpers import STATE_FIELDS


def oracle_sim(packed, state):
    """A fresh RefSim holding ``state`` (a dict of tests.helpers.STATE_FIELDS) at time 0."""
    from tests.helpers import oracle_at
    sim = oracle_at(packed, state)
    sim.time[0] = 0.0
    sim.warning[0] = 0
    return sim


def n_knots(nstep, hold):
    return -(-nstep // hold)


def rollout(new_sim, nq, nv, nu, nstep, n_roll=None, ctrl=None, initial_state=None, initial_warmstart=None, nsub=1,
            hold=1):
    """(state [K, T, 1 + nq + nv], n_done [K], warned [K, T] bool) of one env. ``new_sim()`` returns
    a simulator holding the env's state; ctrl [K, ceil(T / hold), nu] or None (the env's ctrl held);
    initial_state [K, nstate] / initial_warmstart [K, nv] or None (the env's own). ``warned[k, t]``:
    recorded step t of rollout k raised the warning count (always False after n_done)."""
    K = n_roll
    for x in (ctrl, initial_state, initial_warmstart):
        if x is not None:
            assert K is None or K == len(x)
            K = len(x)
    K = 1 if K is None else K
    if ctrl is not None:
        assert np.shape(ctrl) == (K, n_knots(nstep, hold), nu), np.shape(ctrl)
    state = np.zeros((K, nstep, 1 + nq + nv))
    n_done = np.full(K, nstep, dtype=np.int32)
    warned = np.zeros((K, nstep), dtype=bool)
    for k in range(K):
        sim = new_sim()
        if initial_state is not None:
            x = np.asarray(initial_state[k], dtype=np.float64)
            sim.time[0], sim.qpos[:nq], sim.qvel[:nv] = x[0], x[1:1 + nq], x[1 + nq:]
        if initial_warmstart is not None:
            sim.qacc_warmstart[:nv] = initial_warmstart[k]
        for t in range(nstep):
            if ctrl is not None:
                sim.ctrl[:nu] = ctrl[k][t // hold]
            before = int(sim.warning[0])
            sim.step(nsub)
            row = np.concatenate([[float(sim.time[0])], sim.qpos[:nq], sim.qvel[:nv]])
            if int(sim.warning[0]) > before:
                warned[k, t] = True
                n_done[k] = t
                state[k, t:] = row
                break
            state[k, t] = row
    return state, n_done, warned


def oracle_rollout(model, packed, env_state, nstep, **kw):
    """``rollout`` of the CPU oracle in float64 from one tests.helpers state dict."""
    assert set(STATE_FIELDS) <= set(env_state)
    return rollout(lambda: oracle_sim(packed, env_state), model.nq, model.nv, model.nu, nstep, **kw)
