"""The overlapped step: sph_step() launches findNeighbors chunk by chunk of the sorted particles and runs the
density pass and the forces kernel's record pack of a chunk on a second stream under the findNeighbors launch of the next.
Every particle is computed from the same inputs by the same code whichever launch serves it, so results must not depend on the
chunk count: every test forces a chunk count on a small scene (owHIPSolver.set_step_chunks; automatically the path starts at
millions of particles) and asserts bit equality with the oracle, with the serial step (chunk count 1), or both."""
import numpy as np
import pytest

import bench
import scenes
import sphmi
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

BLOCK = 256     # SPH_CHUNK_ALIGN (include/sphmi_chunks.h)
FN_TILE = 128   # particles per findNeighbors workgroup (FN_PART, csrc/sph_neighbors.hip)
STEPS = 5


def _tiny_long():
    box, lattice, mask = bench.WORKLOADS["tiny_long"]  # 30 cell layers
    return scenes.liquid_box(box, lattice, mask=mask)


PARITY_SCENES = {"tiny_long": _tiny_long, "tiny": scenes.SCENES["tiny"]}
_reference = {}


def reference(name):
    """Canonical buffers after steps 1 and STEPS of the oracle and of the serial step (chunk count 1): computed once per scene,
    shared by the tests below and never changed."""
    if name not in _reference:
        sc = PARITY_SCENES[name]()
        N = sc["cfg"].particleCount
        hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc, threads=8)
        hip.set_step_chunks(1)
        out = {}
        for it in range(STEPS):
            hip.step(it)
            ora.step()
            if it in (0, STEPS - 1):
                out[it] = (canon_ora(ora, N), canon_hip(hip, N))
        ora.close()
        hip.close()
        _reference[name] = out
    return _reference[name]


def edges_of(n, chunks):
    return [int(e) for e in sphmi.step_chunk_edges(n, chunks)]


# ---------------------------------------------------------------------------------------------- partition (no GPU)
@pytest.mark.parametrize("chunks", [1, 2, 3, 8, 1000])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 16507704])
def test_chunk_partition(n, chunks):
    e = edges_of(n, chunks)
    assert len(e) == chunks + 1 and e[0] == 0 and e[-1] == n            # covers [0, n) ...
    assert all(b >= a for a, b in zip(e, e[1:]))                         # ... exactly once, no chunk negative
    assert sum(b - a for a, b in zip(e, e[1:])) == n
    assert all(x % BLOCK == 0 and x <= n for x in e[1:-1])               # inner edges are multiples of 256
    blocks = [(b - a + BLOCK - 1) // BLOCK for a, b in zip(e, e[1:])]
    assert max(blocks) - min(blocks) <= 1                                # dealt as evenly as whole blocks allow


def test_chunk_partition_rejects_bad_arguments():
    for n, chunks in ((-1, 2), (10, 0), (10, -3)):
        with pytest.raises(sphmi.SphError):
            sphmi.step_chunk_edges(n, chunks)


# ---------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 3, 7])
@pytest.mark.parametrize("name", list(PARITY_SCENES))
def test_chunked_steps_equal_the_oracle_and_the_serial_step(name, chunks):
    """Five fused steps with a forced chunk count: every buffer parity is judged on (positions, velocities, densities, neighbour
    ids and distances, pressures, accelerations, search structures) equals the oracle's and the serial step's, bit for bit."""
    sc = PARITY_SCENES[name]()
    N = sc["cfg"].particleCount
    assert N % (BLOCK * chunks) != 0
    e = edges_of(N, chunks)
    assert all(b > a for a, b in zip(e, e[1:])), "every chunk holds particles here"
    want = reference(name)
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(chunks)
    for it in range(STEPS):
        hip.step(it)
        if it in want:
            got = canon_hip(hip, N)
            assert_same(got, want[it][0], "%s, %d chunks, step %d, against the oracle" % (name, chunks, it), FUSED_SKIP)
            assert_same(got, want[it][1], "%s, %d chunks, step %d, against the serial step" % (name, chunks, it), FUSED_SKIP)
    hip.close()


# ---------------------------------------------------------------------------------------------- edge cases
def _against_oracle(sc, chunks, steps, where, threads=8):
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc, threads=threads)
    hip.set_step_chunks(chunks)
    hip.reset_stage_times()
    for it in range(steps):
        hip.step(it)
        ora.step()
    got, want = canon_hip(hip, N), canon_ora(ora, N)
    assert_same(got, want, where, FUSED_SKIP)
    ora.close()
    return hip, got


@pytest.mark.gpu
def test_more_chunks_than_blocks():
    sc = scenes.SCENES["tiny"]()
    N = sc["cfg"].particleCount
    e = edges_of(N, 16)
    assert (N + BLOCK - 1) // BLOCK < 16 and any(b == a for a, b in zip(e, e[1:])), "some chunks must be empty"
    _against_oracle(sc, 16, 3, "16 chunks of %d particles" % N)[0].close()


@pytest.mark.gpu
def test_last_chunk_shorter_than_one_search_tile():
    sc = scenes.liquid_box((6.0, 5.0, 7.0), (7, 5, 3))
    N = sc["cfg"].particleCount
    e = edges_of(N, 4)
    assert 0 < e[4] - e[3] < FN_TILE and e[3] > e[2] > e[1] > 0
    _against_oracle(sc, 4, 3, "last chunk of %d particles" % (e[4] - e[3]))[0].close()


@pytest.mark.gpu
def test_exact_walks_on_both_sides_of_a_chunk_edge():
    """~700 particles per cell: compaction lists overflow, so particles are served by the exact walk and their rows have no
    16-bit copy (the density, pack and forces launches read them through the 32-bit ids) — on both sides of the chunk edge."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (18, 18, 18), spacing_in_r0=0.45, origin_in_r0=(4.0, 4.0, 4.0))
    N = sc["cfg"].particleCount
    edge = edges_of(N, 2)[1]
    hip, got = _against_oracle(sc, 2, 2, "overcrowded cells, 2 chunks")
    c = hip.buffer("debugCounters")
    assert c[1] > 0 or c[2] > 0
    crowded = scenes.crowded_particles(got, sc["cfg"].h)  # (of the last step's search: certainly on the exact walk)
    assert (crowded < edge).sum() > 100 and (crowded >= edge).sum() > 100
    hip.close()


@pytest.mark.gpu
def test_worm_scene_with_muscles_equals_the_serial_step():
    """Elastic matter and membranes: the elastic and membrane kernels read rho and the neighbour rows behind the join."""
    solvers = []
    for chunks in (1, 3):
        hip = scenes.hip_for(scenes.worm_scene())
        hip.set_step_chunks(chunks)
        solvers.append(hip)
    N = solvers[0].N
    assert N % (BLOCK * 3) != 0
    for it in range(3):
        for hip in solvers:
            hip.step(it)
            hip.updateMuscleActivityData(sphmi.muscle_signal(it))
    assert_same(canon_hip(solvers[1], N), canon_hip(solvers[0], N), "worm, 3 chunks against the serial step", FUSED_SKIP)
    assert np.abs(canon_hip(solvers[0], N)["acceleration"]).max() > 0
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 3])
def test_predict_correct_iteration_counts(iterations):
    sc = scenes.SCENES["tiny_compressed"]()
    sc["cfg"].maxIteration = iterations
    assert sc["cfg"].particleCount % (BLOCK * 3) != 0
    hip, got = _against_oracle(sc, 3, 3, "maxIteration=%d, 3 chunks" % iterations)
    assert got["pressure"].max() > 0
    hip.close()


# ---------------------------------------------------------------------------------------------- state changes between steps
@pytest.mark.gpu
def test_stage_timing_switched_between_steps():
    """With stage timing on the step takes the serial path (its stages stay separately timed); switching it between steps
    alternates the two paths on one solver."""
    sc = PARITY_SCENES["tiny"]()
    N = sc["cfg"].particleCount
    want = reference("tiny")
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(3)
    timed = 0
    for it in range(STEPS):
        hip.set_stage_timing(it % 2 == 1)
        timed += it % 2
        hip.step(it)
        if it in want:
            assert_same(canon_hip(hip, N), want[it][0], "timing toggled, step %d" % it, FUSED_SKIP)
    t = hip.stage_times()
    M = sc["cfg"].maxIteration
    assert timed == 2
    assert t["find_neighbors"][1] == timed and t["density"][1] == timed and t["forces"][1] == timed
    assert t["predict_density"][1] == M * timed and t["pressure_force"][1] == M * timed
    assert all(ms >= 0 for ms, _ in t.values())
    hip.close()


@pytest.mark.gpu
def test_async_position_read_back_after_every_step():
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = reference("tiny_long")
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(3)
    bufs = [np.empty((N, 4), np.float32), np.empty((N, 4), np.float32)]
    for it in range(STEPS):
        hip.step(it)
        hip.read_position_buffer_async(bufs[it & 1])  # (waits for the copy of step it - 1 first)
        if it - 1 in want:
            assert scenes.bits_equal(bufs[(it - 1) & 1], want[it - 1][0]["position"]), "step %d" % (it - 1)
    hip.wait_position_buffer()
    assert scenes.bits_equal(bufs[(STEPS - 1) & 1], want[STEPS - 1][0]["position"])
    hip.close()


@pytest.mark.gpu
def test_removal_and_emission_between_steps():
    """N changes between steps, and with it the chunk edges: twin solvers, chunked and serial, through the same edits."""
    solvers = []
    for chunks in (1, 3):
        hip = scenes.hip_for(PARITY_SCENES["tiny_long"]())
        hip.set_step_chunks(chunks)
        solvers.append(hip)
    r0 = float(PARITY_SCENES["tiny_long"]()["cfg"].r0)
    counts = []
    for hip in solvers:
        ns = [hip.N]
        hip.step(0)
        z = hip.read_position_buffer()[:, 2]
        zc = float(np.median(z))
        assert hip.remove_region((-np.inf, -np.inf, -np.inf, np.inf, np.inf, zc), types=(1,)) > 0
        ns.append(hip.N)
        hip.step(1)
        hip.step(2)
        # a small block of new liquid in the space the removal emptied
        assert hip.emit_lattice((6 * r0, 6 * r0, 6 * r0), (r0, r0, r0), (5, 4, 7)) == 140
        ns.append(hip.N)
        hip.step(3)
        hip.step(4)
        counts.append(ns)
    assert counts[0] == counts[1]
    e = [edges_of(n, 3) for n in counts[1]]
    assert e[0] != e[1] and e[1] != e[2], "the edits must move the chunk edges"
    N = solvers[0].N
    assert_same(canon_hip(solvers[1], N), canon_hip(solvers[0], N), "edits between steps, 3 chunks against the serial step", FUSED_SKIP)
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
def test_closing_a_solver_right_after_a_step():
    sc = PARITY_SCENES["tiny"]()
    N = sc["cfg"].particleCount
    for _ in range(3):
        hip = scenes.hip_for(sc)
        hip.set_step_chunks(7)
        hip.step(0)
        hip.close()  # launches of both streams are still in flight
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(7)
    hip.step(0)
    assert_same(canon_hip(hip, N), reference("tiny")[0][0], "a solver created after the closed ones", FUSED_SKIP)
    hip.close()


@pytest.mark.gpu
def test_chunk_count_is_checked():
    hip = scenes.hip_for(PARITY_SCENES["tiny"]())
    for bad in (-1, 17):
        with pytest.raises(sphmi.SphError):
            hip.set_step_chunks(bad)
    hip.set_step_chunks(0)
    hip.close()
