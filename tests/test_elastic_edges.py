"""GPU tests of the elastic and membrane kernels (sph_elastic.hip) on the inputs of scenes.elastic_hard_box: full 32-spring rows,
muscle ids at and beyond the guard, a zero-length spring, full 7-entry membrane lists on a tilted sheet, abandoned particles, odd
and even queue lengths, a queue longer than one sweep of the membrane kernel's grid, and queued rows without a 16-bit copy.
Everything is compared bit for bit with the oracle, which tests/test_elastic_edges_host.py pins to the reference's own kernels on
these very inputs; the conditions that make the comparisons meaningful are asserted there from the oracle alone."""
import numpy as np
import pytest

import scenes
import sphmi
import test_elastic_edges_host as H
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

pytestmark = pytest.mark.gpu


def queue_counter(hip):
    return int(hip.buffer("debugCounters")[5])  # what k_membrane_collect counted in the last membrane stage


def run_against_oracle(sc, steps, staged, where):
    """`steps` steps of both; the steps in `staged` stage by stage with a comparison after every stage, the others fused; muscles
    updated after every step on both sides; every buffer compared after every step, and the length of the membrane queue with the
    number of liquid particles that have an elastic neighbour in the oracle's buffers. Returns the GPU's buffers after each step."""
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc, threads=8)
    out = []
    for it in range(steps):
        if it in staged:
            for k, st in enumerate(scenes.STAGE_SEQUENCE):
                m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
                m(it) if st == "integrate" else m()
                ora.run(st)
                skip = ("sortedPosition",) if st in ("hashParticles", "sort") else ()  # (see test_stage_by_stage_matches_oracle)
                if k < scenes.STAGE_SEQUENCE.index("indexx"):
                    skip += FUSED_SKIP
                assert_same(canon_hip(hip, N), canon_ora(ora, N), "%s step %d stage %d %s" % (where, it, k, st), skip)
        else:
            hip.step(it)
            ora.step()
        sig = scenes.hard_muscle_signal(it)
        hip.updateMuscleActivityData(sig)
        ora.update_muscles(sig)
        got, want = canon_hip(hip, N), canon_ora(ora, N)
        assert_same(got, want, "%s after step %d" % (where, it), () if it in staged else FUSED_SKIP)
        if sc["particle_membranes"] is not None:
            assert queue_counter(hip) == len(scenes.membrane_queue(want, N)), (where, it)
        out.append(got)
    hip.close()
    ora.close()
    return out


@pytest.mark.parametrize("mask", [0xffff, 0xffffffff])
def test_hard_scene_stage_by_stage(mask):
    """Steps 0 and 3 stage by stage, 1 and 2 fused: k_elastic with a row of 32 live springs and muscle ids 100 (signal entry 99 is
    zero after even steps and 0.4 after odd ones) and 101 (beyond the guard); k_membranes with full lists, a tilted sheet, abandoned
    particles and queue lengths of both parities."""
    sc = scenes.elastic_hard_box(mask=mask)
    states = run_against_oracle(sc, H.STEPS_ON_GPU, (0, 3), "hard scene, mask %x" % mask)
    # (the abandoned set comes from the 16-bit oracle; for the wide mask that rests on
    # test_elastic_edges_host.test_wide_mode_equals_reference_mode_on_the_hard_scene, and the scratch is indexed by original id)
    gone, _, _ = H.abandoned_particles()
    assert not states[0]["membraneScratch"][gone].any()


def test_twin_without_degenerate_triangles_moves_the_abandoned_particles():
    """The same scene without the degenerate triangles: the particles the first scene abandons get their displacement here, so the
    abandon path costs exactly that and nothing else (everything else is compared with the oracle in both scenes)."""
    sc = scenes.elastic_hard_box(degenerate=False)
    states = run_against_oracle(sc, H.STEPS_ON_GPU, (0, 3), "twin")
    gone, _, _ = H.abandoned_particles()
    assert len(gone) >= 10 and (states[0]["membraneScratch"][gone] != 0).any(1).all()


def test_offset_form():
    """File-mode particle order (elasticOffset = numOfBoundaryP) with the full spring rows and the muscle ids of the hard scene."""
    sc = scenes.elastic_hard_box(offset=True)
    states = run_against_oracle(sc, 5, (), "offset form")
    assert np.abs(states[-1]["acceleration"]).max() > 0


def test_zero_length_spring():
    """Two sheet particles at one position, joined by a spring: k_elastic's `r != 0` skip. Staged up to computeElasticForces (beyond it
    the reference divides by r = 0); the buffers of test_coincident_particles_neighbour_search, and the acceleration."""
    sc = scenes.elastic_hard_box(zero_spring=True)
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc)
    for st in H.UP_TO_ELASTIC:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        ora.run(st)
    got, want = canon_hip(hip, N), canon_ora(ora, N)
    for k in ("particleIndex", "gridCellIndexFixedUp", "neighborIds", "neighborDist", "rho", "acceleration"):
        assert scenes.bits_equal(got[k], want[k]), (k, scenes.diff_report(got[k], want[k]))
    assert np.isfinite(want["acceleration"]).all() and (want["neighborDist"] == 0.0).sum() >= 2


def test_large_sheet_queue_takes_a_second_sweep():
    """90 x 90 sheet, N = 145 k: more than 2048 blocks x 8 half-waves = 16,384 queued particles, so the grid-stride loop of
    k_membranes goes round again. Two fused steps, every buffer."""
    sc, want = H.oracle_states((("large", True),), 2)
    N = sc["cfg"].particleCount
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
        hip.updateMuscleActivityData(scenes.hard_muscle_signal(it))
        assert_same(canon_hip(hip, N), want[it], "large form after step %d" % it, FUSED_SKIP)
        queued = queue_counter(hip)
        assert queued == len(scenes.membrane_queue(want[it], N)) and queued > 2048 * 8, queued
    hip.close()


def test_queued_rows_without_a_sixteen_bit_copy():
    """blob=True, two FUSED steps (the oracle stays finite for two; the staged shortcut was not needed): a dense blob around the
    sheet overflows findNeighbors' compaction lists, such particles take its exact walk, which leaves their rows without a 16-bit
    copy (fn_exact_walk writes SPH_N16_WIDE), and k_membranes reads them through nbr_decode's 32-bit branch.
    The counters. debugCounters[0] and [1] count the particles sent to the exact walk (a cell not staged / a list overflowed).
    debugCounters[2], which the issue behind this test named, counts something else: rows of the FAST path whose offsets do not fit
    16 bits, which takes more than 16,384 particles between a particle and a neighbour in sorted order and cannot happen in a box
    of this size; it is 0 here (printed; test_sixteen_bit_offsets_overflow_next_to_the_membrane covers that counter).
    Asserted instead, per step: at least as many particles took the exact walk as have more than 96 others within h in the
    oracle's buffers (each of a particle's two lanes lists 48 candidates, so one list must overflow:
    scenes.crowded_particles); tests/test_elastic_edges_host.py asserts that at least 50 of THOSE are in the membrane queue at
    every step (seen: 158 and 84), so k_membranes certainly reads rows without a 16-bit copy. Which row is wide cannot be read back."""
    sc = scenes.elastic_hard_box(blob=True)
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc, threads=8)
    before = 0
    for it in range(2):
        hip.step(it)
        ora.step()
        sig = scenes.hard_muscle_signal(it)
        hip.updateMuscleActivityData(sig)
        ora.update_muscles(sig)
        want = canon_ora(ora, N)
        assert_same(canon_hip(hip, N), want, "blob after step %d" % it, FUSED_SKIP)
        assert queue_counter(hip) == len(scenes.membrane_queue(want, N))
        c = hip.buffer("debugCounters")
        walked, before = int(c[0]) + int(c[1]) - before, int(c[0]) + int(c[1])
        crowded = len(scenes.crowded_particles(want, sc["cfg"].h))
        print("blob step %d: debugCounters[0..3] = %s, exact walks this step %d, crowded %d, queue %d"
              % (it, c[:4].tolist(), walked, crowded, queue_counter(hip)))
        assert walked >= crowded >= 50, (it, walked, crowded)
    hip.close()


def test_sixteen_bit_offsets_overflow_next_to_the_membrane():
    """bar=True, one fused step: rows of findNeighbors' FAST path whose offsets do not fit 16 bits (debugCounters[2]) among the
    particles k_membranes serves. tests/test_elastic_edges_host.py derives from the oracle the rows that are certainly of that kind
    unless the particle lost a cell from the staging, which debugCounters[0] counts (an overflowing list, the other way to the
    exact walk, is excluded: those rows have at most 48 candidates). So the counter is at least their number less
    debugCounters[0], and at least (queued ones) - debugCounters[0] of the rows k_membranes decodes are of that kind; both must
    be positive."""
    sc, want, wide, queued = H.bar_state()
    N = sc["cfg"].particleCount
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.updateMuscleActivityData(scenes.hard_muscle_signal(0))
    assert_same(canon_hip(hip, N), want, "bar form after step 0", FUSED_SKIP)
    c = hip.buffer("debugCounters")
    print("bar: debugCounters[0..3] = %s, queue %d, certainly wide %d, of them queued %d"
          % (c[:4].tolist(), queue_counter(hip), len(wide), len(queued)))
    assert queue_counter(hip) == len(scenes.membrane_queue(want, N))
    assert int(c[2]) >= len(wide) - int(c[0]) > 0 and len(queued) - int(c[0]) > 0, c[:4].tolist()
    hip.close()


def test_staged_and_fused_solvers_agree_on_the_hard_scene():
    sc = scenes.elastic_hard_box()
    args = (sc["cfg"], sc["position"], sc["velocity"], sc["elastic"], sc["membranes"], sc["particle_membranes"])
    a = sphmi.owPhysicsFluidSimulator(*args, fused=True, muscles=True)
    b = sphmi.owPhysicsFluidSimulator(*args, fused=False, muscles=True)
    for it in range(6):
        a.simulationStep(); b.simulationStep()
    assert scenes.bits_equal(a.getPosition_cpp(), b.getPosition_cpp())
    assert scenes.bits_equal(a.ocl_solver.read_velocity_buffer(), b.ocl_solver.read_velocity_buffer())
    assert scenes.bits_equal(a.getDensity_cpp(), b.getDensity_cpp())
    assert scenes.bits_equal(a.getParticleIndex_cpp(), b.getParticleIndex_cpp())
