"""GPU tests of the fused step whose forces kernel is also the first predictDensity + correctPressure: outside slab
mode `k_forces<true, true>` forms every neighbour's iteration-0 predicted position from the (x, v) it gathers and sums
k_predict_density's terms over the same 32 slots, boundary particles included; the separate iteration-0 launch is gone.

Everything is compared with the oracle bit for bit, on scenes whose oracle output is first asserted to hold the rows the fusion can
get wrong: liquid rows with a boundary neighbour (its `v` is a wall normal and must not move it), boundary rows with a liquid
neighbour (the rows the forces kernel used to leave at once), rows short of 32 neighbours (empty slots), velocities of -0.0, and
particles whose corrected pressure is positive (so that a wrong rho* of a neighbour shows in the pressure force). No tolerance
appears anywhere."""
import functools
import sys

import numpy as np
import pytest

import scenes
import sphmi
import test_wide_rows_host as W
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

gpu = pytest.mark.gpu  # (the premises need no GPU)

BOX = dict(box_in_h=(8, 8, 8), lattice=(12, 10, 12), origin_in_r0=(1, 1, 1))
LATTICE_SCENES = {"A resting lattice": {}, "B compressed and jittered": dict(spacing_in_r0=0.85, jitter_in_r0=0.2)}
ENOUGH_ROWS = 300


@functools.lru_cache(maxsize=None)
def lattice_scene(name, iterations=3):
    sc = scenes.liquid_box(**BOX, **LATTICE_SCENES[name])
    sc["cfg"].maxIteration = iterations
    nl = sc["numOfLiquidP"]
    v = sc["velocity"]
    v[0:nl:7, 0] = np.float32(-0.0)  # predict_position's `v + dt * 0` makes them +0.0
    v[0:nl:11, 1] = np.float32(-0.0)
    v[0:nl:13, 2] = np.float32(-1e-3)
    return sc


@functools.lru_cache(maxsize=None)
def oracle_states(name, iterations):
    """The oracle's canonical arrays after steps 1 and 3 of a lattice scene."""
    sc = lattice_scene(name, iterations)
    N = sc["cfg"].particleCount
    ora = scenes.oracle_for(sc)
    out = {}
    for step in (1, 2, 3):
        ora.step()
        if step != 2:
            out[step] = canon_ora(ora, N)
    ora.close()
    return sc, out


def row_kinds(canon, N):
    """Per sorted particle of the step that left `canon`: type, and its neighbour row's count, boundary and liquid members."""
    order = canon["particleIndex"].reshape(-1, 2)[:, 1].astype(np.int64)
    kind = canon["position"][:, 3].astype(np.int32)[order]  # (sortedPosition's .w is not the type in the reference's layout)
    ids = canon["neighborIds"].reshape(N, 32)
    nk = np.where(ids >= 0, kind[np.clip(ids, 0, N - 1)], 0)
    return kind, (ids >= 0).sum(1), (nk == sphmi.BOUNDARY_PARTICLE).any(1), (nk == sphmi.LIQUID_PARTICLE).any(1)


def test_premises_hold_on_the_oracles_output():
    """Seen (scene A / scene B, after one step): 2,792 particles, 1,352 of them boundary; liquid rows with a boundary neighbour
    640 / 641, boundary rows with a liquid neighbour 419 / 375, liquid rows short of 32 neighbours 847 / 1,006; particles with
    p > 0: 288 / 1,156 liquid and 0 / 69 boundary."""
    for name in LATTICE_SCENES:
        sc, states = oracle_states(name, 3)
        N = sc["cfg"].particleCount
        canon = states[1]
        kind, count, has_bnd, has_liq = row_kinds(canon, N)
        liquid, boundary = kind == sphmi.LIQUID_PARTICLE, kind == sphmi.BOUNDARY_PARTICLE
        seen = dict(liquid_with_boundary=int((liquid & has_bnd).sum()), boundary_with_liquid=int((boundary & has_liq).sum()),
                    liquid_short=int((liquid & (count < 32)).sum()), liquid_p=int((canon["pressure"][liquid] > 0).sum()),
                    boundary_p=int((canon["pressure"][boundary] > 0).sum()))
        print(name, N, int(boundary.sum()), seen)
        for k in ("position", "velocity", "rho", "pressure", "acceleration"):
            assert np.isfinite(canon[k]).all(), (name, k)
        v = sc["velocity"][:sc["numOfLiquidP"]]
        assert np.signbit(v[0::7, 0]).all() and (v[0::7, 0] == 0).all() and (v[0::13, 2] < 0).all()
        assert min(seen["liquid_with_boundary"], seen["boundary_with_liquid"], seen["liquid_short"]) >= ENOUGH_ROWS, (name, seen)
        if name.startswith("B"):
            assert seen["liquid_p"] >= 500 and seen["boundary_p"] >= 30, (name, seen)


@gpu
@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("name", list(LATTICE_SCENES))
def test_fused_step_equals_the_oracle(name, iterations):
    sc, states = oracle_states(name, iterations)
    N = sc["cfg"].particleCount
    hip = scenes.hip_for(sc)
    hip.set_stage_timing(True)
    for step in (1, 2, 3):
        hip.step(step - 1)
        if step == 2:
            continue
        where = "%s, maxIteration=%d, after %d steps" % (name, iterations, step)
        got, want = canon_hip(hip, N), states[step]
        if iterations == 1:  # rho* and p are what the forces kernel itself wrote: the boundary rows by themselves, so that a failure names them
            boundary = row_kinds(want, N)[0] == sphmi.BOUNDARY_PARTICLE
            for what, g, w in (("rho*", got["rho"][N:], want["rho"][N:]), ("pressure", got["pressure"], want["pressure"])):
                assert scenes.bits_equal(g[boundary], w[boundary]), "%s: %s of the boundary rows: %s" % (
                    where, what, scenes.diff_report(g[boundary], w[boundary]))
        assert_same(got, want, where, FUSED_SKIP)
    t = hip.stage_times()
    # (the stage counts stay one forces and maxIteration predict_density per step: the one inside the forces kernel is counted too)
    assert t["forces"][1] == 3 and t["predict_density"][1] == 3 * iterations, t
    hip.close()


@gpu
def test_fused_and_staged_steps_leave_the_same_predicted_state():
    """Scene B: the fused step against the 18 stage entry points (k_forces<false, false>, k_predict_positions, three separate
    predictDensity + correctPressure): rho*, pressure, predicted positions and both accelerations."""
    sc = lattice_scene("B compressed and jittered")
    N = sc["cfg"].particleCount
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(2):
        a.step(it)
        scenes.staged_step(b, it)
        got, want = canon_hip(a, N), canon_hip(b, N)
        for k in ("rho", "pressure", "predictedPosition", "acceleration", "position", "velocity"):
            assert scenes.bits_equal(got[k], want[k]), "step %d, %s: %s" % (it, k, scenes.diff_report(got[k], want[k]))
    a.close(), b.close()


@gpu
@pytest.mark.parametrize("state", ["blob0", "blob1"])
def test_rows_without_a_16_bit_copy(state):
    """Scene C: scenes.elastic_hard_box(blob=True), whose crowded blob is served by findNeighbors' exact walk (rows with 32-bit ids
    only): the fused kernel's wideRow path feeds the density half too."""
    c = W.case(state)
    assert len(c.wide) >= 100
    hip = scenes.hip_for(c.sc)
    for it in range(int(state[4:]) + 1):
        hip.step(it)
        hip.updateMuscleActivityData(scenes.hard_muscle_signal(it))
    assert_same(canon_hip(hip, c.N), c.canon, state, FUSED_SKIP)
    hip.close()


@gpu
def test_elastic_sheet_with_muscles():
    """Scene D: every particle kind, springs, a muscle row and membranes; k_elastic runs between the fused kernel and the
    pressure force and touches neither the predicted positions nor (rho*, p)."""
    sc = scenes.elastic_sheet_box()
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc)
    for it in range(3):
        hip.step(it)
        ora.step()
        sig = sphmi.muscle_signal(it)
        hip.updateMuscleActivityData(sig)
        ora.update_muscles(sig)
    assert_same(canon_hip(hip, N), canon_ora(ora, N), "elastic sheet, 3 steps", FUSED_SKIP)
    assert np.abs(canon_ora(ora, N)["acceleration"]).max() > 0
    hip.close(), ora.close()


@gpu
def test_slab_mode_keeps_the_separate_first_predict_density(tmp_path):
    """The gate: in slab mode the forces launch covers the owned layers only and the first predictDensity stays a launch of its
    own. Two slab ranks on the two-slab box against the single-domain solver, which takes the fused kernel."""
    import test_slab as TS
    sys.path.insert(0, TS.HERE)
    import slab_worker
    steps = 3
    results = TS.run_ranks("hip", 2, tmp_path, steps=steps)
    sc = slab_worker.scene()
    hip = scenes.hip_for(sc)
    for it in range(steps):
        hip.step(it)
    TS.check_union(results, sc, hip.read_position_buffer(), hip.read_velocity_buffer())
    hip.close()
