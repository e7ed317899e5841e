"""CPU tests for the elastic / membrane edge cases (scenes.elastic_hard_box): the oracle against the reference's own
kernels on inputs that reach the branches no committed scene reaches — live where oracle/_ref/libsphref.so exists, and always
against the digests of those kernels' buffers (tests/golden/ref_elastic_digests.json, made by make_ref_elastic_digests.py) — and
the conditions, asserted from the oracle's buffers alone, that make the GPU tests of tests/test_elastic_edges.py meaningful.
(The reference prints one line per abandoned particle from inside its membrane kernel: expected noise in a live run.)"""
import functools
import json
import os

import numpy as np
import pytest

import scenes
from test_oracle import LIVE_BUFFERS, _ref_available, buffer_digest, ref_solver

EDGE_DIGESTS = os.path.join(scenes.GOLDEN, "ref_elastic_digests.json")
UP_TO_ELASTIC = scenes.STAGE_SEQUENCE[:scenes.STAGE_SEQUENCE.index("computeElasticForces") + 1]
# name -> (builder arguments, steps, stages of one step, record after every stage?, update the muscles after a step?)
EDGE_SCENES = {
    "hard16": (dict(), 3, scenes.STAGE_SEQUENCE, True, True),
    # elastic matter without membrane lists: the membrane stage is left out on both sides (test_oracle.live_scene)
    "hard_offset": (dict(offset=True), 3, [s for s in scenes.STAGE_SEQUENCE if s != "computeInteractionWithMembranes"], True, True),
    # beyond computeElasticForces the reference divides by r = 0
    "zero_spring": (dict(zero_spring=True), 1, UP_TO_ELASTIC, True, False),
    "large": (dict(large=True), 2, scenes.STAGE_SEQUENCE, False, True),
}
STEPS_ON_GPU = 4  # steps the GPU tests take on the small scenes (6 where the staged and the fused solver are compared)


def edge_run(name, run, update_muscles, on_record):
    """Drives a solver through the scene's plan with run(stage, iteration) and update_muscles(signal); on_record(k, label, it) at
    every recorded point. Returns the number of recorded points."""
    _, steps, stages, every_stage, muscles = EDGE_SCENES[name]
    k = 0
    for it in range(steps):
        for st in stages:
            run(st, it)
            if every_stage:
                on_record(k, st, it)
                k += 1
        if muscles:
            update_muscles(scenes.hard_muscle_signal(it))
        if not every_stage:
            on_record(k, "step", it)
            k += 1
    return k


@pytest.mark.parametrize("name", list(EDGE_SCENES))
def test_oracle_against_reference_kernels_on_edge_inputs(name):
    sc = scenes.elastic_hard_box(**EDGE_SCENES[name][0])
    recorded = json.load(open(EDGE_DIGESTS))[name]
    assert scenes.sha(sc["position"])[:16] == recorded["input"]["position"], "scene builder drifted from the recorded input"
    assert scenes.sha(sc["elastic"])[:16] == recorded["input"]["elastic"]
    rows = recorded["rows"]
    T = scenes.oracle_for(sc, threads=8)
    S = ref_solver(sc, threads=8) if _ref_available() else None

    def check(k, label, it):
        assert rows[k]["stage"] == label, (k, rows[k]["stage"], label)
        for b in LIVE_BUFFERS:  # every word of every buffer, including the dead .w lanes
            assert buffer_digest(T.buffer(b)) == rows[k]["digests"][b], (name, it, label, b)

    def check_live(k, label, it):
        for b in LIVE_BUFFERS:
            assert buffer_digest(S.buffer(b)) == rows[k]["digests"][b], (name, it, label, b, "reference drifted from its digests")

    assert edge_run(name, lambda st, it: T.run(st), T.update_muscles, check) == len(rows)
    if S is not None:
        assert edge_run(name, S.run, S.update_muscles, check_live) == len(rows)
    if name == "zero_spring":
        el = sc["elastic"].reshape(-1, 32, 4)
        assert np.array_equal(sc["position"][0, :3], sc["position"][1, :3]) and 1 in el[0, :, 0].astype(int)
        assert np.isfinite(T.buffer("acceleration")).all()


@functools.lru_cache(maxsize=None)
def oracle_states(key, steps):
    """(scene, the oracle's canonical buffers after each of `steps` steps) of elastic_hard_box(**dict(key)). The membrane scratch
    among them is what computeInteractionWithMembranes left: the finalize stage reads it and does not write it."""
    sc = scenes.elastic_hard_box(**dict(key))
    N = sc["cfg"].particleCount
    T = scenes.oracle_for(sc, threads=8)
    out = []
    for it in range(steps):
        T.step()
        T.update_muscles(scenes.hard_muscle_signal(it))
        out.append(scenes.canonical(T.buffer, N))
    return sc, out


def small(**kw):
    return oracle_states(tuple(sorted(kw.items())), STEPS_ON_GPU)


def test_spring_rows_membrane_lists_and_muscle_ids_reach_their_edges():
    for kw in (dict(), dict(large=True)):
        sc = scenes.elastic_hard_box(**kw)
        el = sc["elastic"].reshape(-1, 32, 4)
        live = el[:, :, 0] >= 0
        assert int(live.all(1).sum()) >= 1, "no spring row has 32 live entries"
        assert int((sc["particle_membranes"] >= 0).all(1).sum()) >= 20, "fewer than 20 membrane lists have 7 live entries"
        ids = set(el[:, :, 2][live].astype(np.int32).tolist())
        assert {100, 101} <= ids and sc["cfg"].muscleCount == 100
        # the block has no membranes, every list entry names a triangle, the degenerate ones come first in their lists
        S, pml, mem = sc["sheetCount"], sc["particle_membranes"], sc["membranes"]
        assert (pml[S:] == -1).all() and pml.max() < len(mem)
        deg = np.flatnonzero(mem[:, 0] == mem[:, 1])
        assert len(deg) >= (2 if not kw else 10) and all(pml[mem[t, 0], 0] == t for t in deg)


def abandoned_particles():
    """(orig ids abandoned at step 0, sorted cell key per orig id, moved mask per orig id) of the small 16-bit scene."""
    (sc, hard), (_, twin) = small(), small(degenerate=False)
    N = sc["cfg"].particleCount
    liquid = sc["position"][:, 3].astype(np.int32) == 1
    moved = (hard[0]["membraneScratch"] != 0).any(1)
    moved_twin = (twin[0]["membraneScratch"] != 0).any(1)
    pi = hard[0]["particleIndex"].reshape(-1, 2)
    cell = np.empty(N, np.int64)
    cell[pi[:, 1]] = pi[:, 0]
    return np.flatnonzero(liquid & ~moved & moved_twin), cell, moved


def test_abandoned_particles_exist_and_share_cells_with_moving_ones():
    """The scratch is cleared and written once per step and nothing else moves between the two scenes before the membrane
    stage of step 0, so scratch (= the second half of the position buffer after the step) differs only through the abandon path."""
    gone, cell, moved = abandoned_particles()
    assert len(gone) >= 10, len(gone)
    cells = set(cell[gone].tolist())
    assert len(cells) >= 3, cells
    with_movers = [c for c in cells if (moved & (cell == c)).any()]
    assert len(with_movers) >= 3, (cells, with_movers)


def test_queue_sizes_are_odd_and_even_and_exceed_one_sweep():
    sc, states = small()
    N = sc["cfg"].particleCount
    sizes = [len(scenes.membrane_queue(c, N)) for c in states]
    assert {s % 2 for s in sizes} == {0, 1}, sizes  # the odd one leaves the second half of the last wave without a particle
    big, bstates = oracle_states((("large", True),), 2)
    bsizes = [len(scenes.membrane_queue(c, big["cfg"].particleCount)) for c in bstates]
    assert min(bsizes) > 2048 * 8, bsizes  # more than one sweep of the membrane kernel's grid
    assert all(np.isfinite(c["position"]).all() and np.isfinite(c["velocity"]).all() for c in bstates)


def test_wide_mode_equals_reference_mode_on_the_hard_scene():
    """Nothing aliases in this box and the reference has no wide mode: the transitive argument of test_oracle.py."""
    (_, a), (_, b) = small(), small(mask=0xffffffff)
    for it in range(STEPS_ON_GPU):
        for k in a[it]:
            assert scenes.bits_equal(a[it][k], b[it][k]), (it, k)


@pytest.mark.parametrize("kw,steps", [(dict(), 6), (dict(degenerate=False), STEPS_ON_GPU), (dict(mask=0xffffffff), STEPS_ON_GPU),
                                      (dict(offset=True), 5), (dict(blob=True), 2)])
def test_positions_stay_finite_for_the_steps_the_gpu_tests_run(kw, steps):
    sc, states = oracle_states(tuple(sorted(kw.items())), steps)
    for it, c in enumerate(states):
        assert np.isfinite(c["position"]).all() and np.isfinite(c["velocity"]).all(), (kw, it)
    if kw.get("blob"):
        N, E, L, B = sc["cfg"].particleCount, sc["numOfElasticP"], sc["numOfLiquidP"], sc["blobCount"]
        for c in states:
            queue = scenes.membrane_queue(c, N)
            src = c["particleIndex"].reshape(-1, 2)[queue, 1]
            assert int(((src >= E + L - B) & (src < E + L)).sum()) >= 50  # blob particles are in the membrane queue
            # ... and at least 50 queued particles are certain to be served by findNeighbors' exact walk (no 16-bit row)
            assert len(np.intersect1d(queue, scenes.crowded_particles(c, sc["cfg"].h))) >= 50


def bar_state():
    """(scene, the oracle's buffers after step 0, certainly-wide rows, those of them that are queued) of the bar=True form."""
    sc, (c,) = oracle_states((("bar", True),), 1)
    N = sc["cfg"].particleCount
    wide = scenes.certainly_wide_rows(c, sc["cfg"], N)
    return sc, c, wide, np.intersect1d(wide, scenes.membrane_queue(c, N))


def test_sixteen_bit_offsets_overflow_for_queued_rows_of_the_bar_form():
    """More than 16,384 particles of the bar lie between liquid next to the sheet and its neighbours one cell row up: the fast path of
    findNeighbors cannot encode such rows in 16 bits (debugCounters[2]). From the oracle alone: such rows exist, some belong to queued
    particles, and some of those are moved by the membrane stage, so a wrong 32-bit read in k_membranes would show in the scratch."""
    sc, c, wide, queued = bar_state()
    assert np.isfinite(c["position"]).all() and np.isfinite(c["velocity"]).all()
    assert sc["barCount"] > 16384 + 3000
    src = c["particleIndex"].reshape(-1, 2)[queued, 1]
    moved = int((c["membraneScratch"][src] != 0).any(1).sum())
    assert len(wide) >= len(queued) >= moved >= 1, (len(wide), len(queued), moved)
