"""numpy reference for mgx_sensor_fd (TEST INFRASTRUCTURE ONLY): the sensor derivatives C and D of
MuJoCo's mjd_transitionFD [ext] as include/mgx.h restates them — written against that text, not
the HIP code.

The virtual envs are those of tests/fd_reference.py (``virtual_states``: the nominal state, then one
per perturbed column, centred mode +eps then -eps, under the control-limit rule); without D the
ctrl columns are dropped, so K = 2 nv. ``difference`` turns their sensordata rows into (C, D) with
the centred and one-sided rules of ``fd_reference.difference``; rows are plain differences.
``oracle_sensor_fd`` evaluates the rows on the CPU oracle in float64 (RefSim.forward() and
tests/sensor_reference.sensordata); the GPU tests evaluate them with ``PhysicsBatch.sensordata()``
instead (the hand-built composition the library call replaces). tests/test_sensor_fd_cpu.py pins
this file by known answers.
"""
import numpy as np

from tests import fd_reference as fr
from tests import sensor_reference as sr
from tests.helpers import STATE_FIELDS


def virtual_states(model, state, eps, centered, with_d=True, dtype=np.float64):
    """(states [C], steps [C - 1]) of fd_reference.virtual_states; without D only the 2 nv state
    columns (K = 2 nv: the ctrl columns are the last ones of each side)."""
    states, steps = fr.virtual_states(model, state, eps, centered, dtype)
    if with_d or model.nu == 0:
        return states, steps
    K, nx2 = 2 * model.nv + model.nu, 2 * model.nv
    keep = [i for i in range(len(steps)) if i % K < nx2]
    return [states[0]] + [states[1 + i] for i in keep], [steps[i] for i in keep]


def difference(model, sens, steps, eps, centered, with_d=True, dtype=np.float64):
    """(C [ns, 2nv], D [ns, nu] or None) in ``dtype`` from the virtual envs' sensordata rows sens
    [C, ns] (an array of ``dtype``): every entry is (s_a - s_b) / step in ``dtype``. Centred columns
    with both sides taken divide their difference by 2 eps; one side taken is that one-sided
    difference against the nominal row; no side taken is 0."""
    nx2 = 2 * model.nv
    K = nx2 + (model.nu if with_d else 0)
    sens = np.asarray(sens, dtype=dtype)
    M = np.zeros((sens.shape[1], K), dtype=dtype)
    two_eps = dtype(2) * dtype(eps)
    for k in range(K):
        hp = dtype(steps[k][1])
        if not centered:
            if hp != 0:
                M[:, k] = (sens[1 + k] - sens[0]) / hp
            continue
        hm = dtype(steps[K + k][1])
        if hp != 0 and hm != 0:
            M[:, k] = (sens[1 + k] - sens[1 + K + k]) / two_eps
        elif hp != 0:
            M[:, k] = (sens[1 + k] - sens[0]) / hp
        elif hm != 0:
            M[:, k] = (sens[1 + K + k] - sens[0]) / hm
    return M[:, :nx2].copy(), (M[:, nx2:].copy() if with_d else None)


def oracle_rows(model, packed, states):
    """float64 [len(states), ns]: the oracle's sensordata at each state (forward(), nothing stepped)."""
    from oracle.mjref import RefSim
    sim = RefSim(packed)
    rows = []
    for s in states:
        for f in STATE_FIELDS:
            sim.field(f)[:] = s[f]
        sim.forward()
        rows.append(sr.sensordata(model, sr.fields(sim)))
    return np.stack(rows) if rows else np.zeros((0, int(model.nsensordata)))


def oracle_sensor_fd(model, packed, state, eps=1e-6, centered=False, with_d=True):
    """(C, D, sensordata) of the CPU oracle in float64."""
    states, steps = virtual_states(model, state, eps, centered, with_d)
    rows = oracle_rows(model, packed, states)
    C, D = difference(model, rows, steps, eps, centered, with_d)
    return C, D, rows[0]
