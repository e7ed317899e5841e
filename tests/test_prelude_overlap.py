"""The prelude under the first search chunks on the GPU. Where the search runs in chunks, the velocity half of the
gather (sortedVelocity, particleIndexBack) and the band records of the chunks from the third on are written beside
the first search launches; if the halo check fails, the deferred records are scattered in front of the search instead. Every
particle's values come from the same expressions and inputs as in the serial step, so every test asserts bit equality with the
oracle (or the serial step), and the band arrays equal the numpy restatement (band_ref.py). Each premise — the check passes or
fails, the deferred range is not empty — is asserted first from the oracle's cell table."""
import numpy as np
import pytest

import band_cases
import band_ref
import scenes
import sphmi
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora
from test_search_bands import _oracle as muscle_oracle, bands_built
from test_search_bands_edges import assert_device_bands
from test_step_pipeline import DBG_PIPED, DBG_SERIAL, PARITY_SCENES, edges_of, halo_check, oracle_states

pytestmark = pytest.mark.gpu

STEPS = 3


def premise(name, chunks):
    """What the halo check says on each of the STEPS steps, from the oracle's cell tables (CPU)."""
    cfg = PARITY_SCENES[name]()["cfg"]
    return [halo_check(c, cfg, chunks) for c in oracle_states(name)[:STEPS]]


def deferred_range(n, chunks):
    e = edges_of(n, chunks)
    return e[sphmi.step_band_defer_first(chunks)], n


def solver(sc, chunks, depth, mode=0):
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    hip.set_search_bands(mode)
    return hip


def run(name, chunks, depth, mode, bands_allowed=True):
    """STEPS steps: every canonical buffer equals the oracle's after each, the band arrays the restatement. Returns the counters."""
    sc = PARITY_SCENES[name]()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states(name)
    hip = solver(sc, chunks, depth, mode)
    where = "%s, %d chunks, depth %d, bands mode %d" % (name, chunks, depth, mode)
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == (mode == 0 and bands_allowed)
        assert_same(canon_hip(hip, N), want[it], "%s, step %d" % (where, it), FUSED_SKIP)
        if mode == 0 and bands_allowed:
            assert_device_bands(hip, cfg, N, "%s, step %d" % (where, it))
    c = hip.buffer("debugCounters").astype(np.int64)
    hip.close()
    return c


def passing_counts():
    """The chunk counts 4 .. 8 of tiny_long on which the check passes on every step and the deferred range holds particles."""
    N = PARITY_SCENES["tiny_long"]()["cfg"].particleCount
    out = [c for c in range(4, 9) if all(premise("tiny_long", c)) and deferred_range(N, c)[0] < N]
    assert len(out) >= 2, out
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("depth", [0, 1])
def test_deferred_scatter_beside_the_first_search_chunks(depth, mode):
    """The check passes: the records of the chunks from the third on are scattered beside the first search launch. With bands the check runs
    at depth 0 too (the deferred scatter goes by its tables); without them only the velocity half moves."""
    assert band_ref.grid_allows_bands(PARITY_SCENES["tiny_long"]()["cfg"])
    for chunks in passing_counts():
        c = run("tiny_long", chunks, depth, mode)
        checked = depth > 0 or mode == 0
        assert c[DBG_PIPED] == (STEPS if checked else 0) and c[DBG_SERIAL] == 0, (chunks, c[9:11])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("chunks", [7, 16])
def test_failed_check_scatters_everything_in_front_of_the_search(chunks, depth, mode):
    """tiny: chunks thinner than a cell layer, the check fails on every step and the scatter by the serial table serves the
    deferred range; 16 chunks over 11 blocks leave some chunks empty."""
    sc = PARITY_SCENES["tiny"]()
    N = sc["cfg"].particleCount
    assert band_ref.grid_allows_bands(sc["cfg"])
    assert not any(premise("tiny", chunks)), "the check must fail on every step"
    assert deferred_range(N, chunks)[0] < N
    c = run("tiny", chunks, depth, mode)
    checked = depth > 0 or mode == 0
    assert c[DBG_SERIAL] == (STEPS if checked else 0) and c[DBG_PIPED] == 0, c[9:11]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("chunks", [2, 3])
def test_nothing_is_deferred_with_three_chunks_or_fewer(chunks, mode):
    assert sphmi.step_band_defer_first(chunks) == chunks
    c = run("tiny_long", chunks, 0, mode)
    assert c[DBG_PIPED] == 0 and c[DBG_SERIAL] == 0, "no check at depth 0 where nothing is deferred"
    c = run("tiny_long", chunks, 1, mode)
    assert c[DBG_PIPED] == STEPS


@pytest.mark.parametrize("depth", [0, 1])
def test_thin_column_with_an_empty_chunk_and_a_short_last_chunk(depth):
    """Sixteen chunks of at most one block, one empty, the last of 48 particles: the deferred scatter and k_sort_post_vel end in a
    wave of 48 lanes, and a search launch is one block."""
    sc = PARITY_SCENES["thin"]()
    N = sc["cfg"].particleCount
    e = edges_of(N, 16)
    assert sum(b == a for a, b in zip(e, e[1:])) == 1 and 0 < e[16] - e[15] < 64
    assert band_ref.grid_allows_bands(sc["cfg"]) and deferred_range(N, 16)[0] < N
    assert all(premise("thin", 16))
    c = run("thin", 16, depth, 0)
    assert c[DBG_PIPED] == STEPS and c[DBG_SERIAL] == 0


def test_counted_box_in_four_chunks():
    """131 073 particles: 513 blocks in four chunks, the deferred range crosses a block edge of the band scan (1024 waves) and ends
    in a wave with one live lane."""
    n = 131073
    sc = band_cases.counted_box(n)
    cfg = sc["cfg"]
    lo, hi = deferred_range(n, 4)
    assert 0 < lo < hi == n and lo // 64 // band_cases.BAND_SUPER < (n - 1) // 64 // band_cases.BAND_SUPER and n % 64 == 1
    ora = scenes.oracle_for(sc, threads=8)
    want = []
    for _ in range(STEPS):
        ora.step()
        want.append(canon_ora(ora, n))
    ora.close()
    passed = sum(sphmi.step_halo_check(w["particleIndex"].reshape(-1, 2)[:, 0].astype(np.uint32), w["gridCellIndexFixedUp"].astype(np.uint32),
                                       edges_of(n, 4), cfg.gridCellsX, cfg.gridCellsY) for w in want)
    for depth in (0, 1):
        hip = solver(sc, 4, depth)
        for it in range(STEPS):
            hip.step(it)
            assert bands_built(hip)
            where = "counted box %d, 4 chunks, depth %d, step %d" % (n, depth, it)
            assert_same(canon_hip(hip, n), want[it], where, FUSED_SKIP)
            assert_device_bands(hip, cfg, n, where)
        c = hip.buffer("debugCounters")
        assert c[DBG_PIPED] == passed and c[DBG_SERIAL] == STEPS - passed
        hip.close()


def test_worm_with_muscles_in_four_chunks():
    """k_sort_post (no compacted keys), no bands (16-bit ids alias), elastic matter: k_elastic and the membrane kernels read
    particleIndexBack behind the join."""
    sc = scenes.worm_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert not band_ref.grid_allows_bands(cfg) and cfg.numOfElasticP > 0
    assert edges_of(N, 4)[3] < N
    want = muscle_oracle("worm")
    for depth in (0, 1):
        hip = solver(sc, 4, depth)
        for it in range(STEPS):
            hip.updateMuscleActivityData(scenes.hard_muscle_signal(it)[:cfg.muscleCount])
            hip.step(it)
            assert not bands_built(hip)
            assert_same(canon_hip(hip, N), want[it], "worm, 4 chunks, depth %d, step %d" % (depth, it), FUSED_SKIP)
        hip.close()
    assert np.abs(want[STEPS - 1]["acceleration"]).max() > 0


def test_stage_timing_toggled_between_steps():
    """With stage timing on the step is the serial sequence (the full gather, the whole scatter in the prelude); the two paths
    alternate on one solver."""
    chunks = passing_counts()[0]
    sc = PARITY_SCENES["tiny_long"]()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states("tiny_long")
    hip = solver(sc, chunks, 1)
    hip.reset_stage_times()
    for it in range(STEPS):
        hip.set_stage_timing(it % 2 == 1)
        hip.step(it)
        assert_same(canon_hip(hip, N), want[it], "timing toggled, step %d" % it, FUSED_SKIP)
        assert_device_bands(hip, cfg, N, "timing toggled, step %d" % it)
    t = hip.stage_times()
    assert t["sort_post"][1] == 1 and t["bands"][1] == 1 and t["find_neighbors"][1] == 1
    c = hip.buffer("debugCounters")
    assert c[DBG_PIPED] == STEPS - 1 and c[DBG_SERIAL] == 0
    hip.close()


def test_removal_and_emission_between_steps():
    """N changes between steps, and with it the edges, the deferred range and the tables: twin solvers through the same edits."""
    chunks = passing_counts()[-1]
    solvers = [solver(PARITY_SCENES["tiny_long"](), c, d) for c, d in ((1, -1), (chunks, 0), (chunks, 1))]
    cfg = PARITY_SCENES["tiny_long"]()["cfg"]
    r0 = float(cfg.r0)
    for hip in solvers:
        hip.step(0)
        z = hip.read_position_buffer()[:, 2]
        assert hip.remove_region((-np.inf, -np.inf, -np.inf, np.inf, np.inf, float(np.median(z))), types=(1,)) > 0
        hip.step(1)
        assert hip.emit_lattice((6 * r0, 6 * r0, 6 * r0), (r0, r0, r0), (5, 4, 7)) == 140
        hip.step(2)
    N = solvers[0].N
    assert N != cfg.particleCount and all(h.N == N for h in solvers)
    ref = canon_hip(solvers[0], N)
    for hip in solvers[1:]:
        assert_same(canon_hip(hip, N), ref, "edits between steps against the serial step", FUSED_SKIP)
        flags = hip.buffer("searchBandFlags")
        assert np.array_equal(flags, solvers[0].buffer("searchBandFlags"))
        assert scenes.bits_equal(hip.buffer("searchBands"), solvers[0].buffer("searchBands"))
        assert np.array_equal(hip.buffer("searchBandStart"), solvers[0].buffer("searchBandStart"))
    for hip in solvers:
        hip.close()


def test_async_position_read_back_after_every_step():
    chunks = passing_counts()[0]
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = oracle_states("tiny_long")
    hip = solver(sc, chunks, 1)
    bufs = [np.empty((N, 4), np.float32), np.empty((N, 4), np.float32)]
    for it in range(STEPS):
        hip.step(it)
        hip.read_position_buffer_async(bufs[it & 1])  # (waits for the copy of step it - 1 first)
        if it > 0:
            assert scenes.bits_equal(bufs[(it - 1) & 1], want[it - 1]["position"]), "step %d" % (it - 1)
    hip.wait_position_buffer()
    assert scenes.bits_equal(bufs[(STEPS - 1) & 1], want[STEPS - 1]["position"])
    hip.close()


def test_velocity_read_right_after_a_step():
    """read_velocity_buffer enqueues on the solver's stream behind the join, hence behind the integrate that read what
    k_sort_post_vel gathered."""
    chunks = passing_counts()[0]
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = oracle_states("tiny_long")
    for depth in (0, 1):
        hip = solver(sc, chunks, depth)
        for it in range(STEPS):
            hip.step(it)
            assert scenes.bits_equal(hip.read_velocity_buffer()[:N], want[it]["velocity"]), "depth %d, step %d" % (depth, it)
        hip.close()


def test_closing_a_solver_right_behind_a_step():
    chunks = passing_counts()[0]
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    for _ in range(3):
        hip = solver(sc, chunks, 1)
        hip.step(0)
        hip.close()  # k_sort_post_vel, the deferred scatter and the searches may still be in flight
    hip = solver(sc, chunks, 1)
    hip.step(0)
    assert_same(canon_hip(hip, N), oracle_states("tiny_long")[0], "a solver created after the closed ones", FUSED_SKIP)
    hip.close()
