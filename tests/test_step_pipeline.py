"""The pipelined step: where sph_step() runs the search in chunks, up to six of the kernels behind it (forces, then
predicted density and pressure force of every predict-correct iteration) follow it on the chunk stream chunk by chunk, each stage
one chunk behind the stage before it. A one-block kernel checks every step that the neighbours of chunk c lie in chunks
c - 1 .. c + 1 (the premise the stream order rests on) and lets the same stages run over all particles behind the search if not.
Every particle is computed by the same instructions from the same inputs either way, so every test asserts bit equality with the
oracle, with the serial step, or both; the launch order and the halo check are also tested on their own, without a GPU."""
import numpy as np
import pytest

import bench
import scenes
import sphmi
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

BLOCK = 256   # SPH_CHUNK_ALIGN (include/sphmi_chunks.h)
STEPS = 5
DBG_SERIAL, DBG_PIPED = 9, 10   # debugCounters: steps whose halo check failed / passed (csrc/sph_neighbors.hip, layout comment)


def _tiny_long():
    box, lattice, mask = bench.WORKLOADS["tiny_long"]  # 30 cell layers
    return scenes.liquid_box(box, lattice, mask=mask)


def _thin():
    """A thin column, 44 cell layers of 2 x 2 cells: 3632 particles are 15 blocks of 256, so 16 chunks leave one chunk empty, every
    other chunk one block (about three cell layers) and the last one 48 particles; the halo check still passes."""
    return scenes.liquid_box((3.0, 3.0, 88.0), (2, 2, 20), mask=0xffffffff)


PARITY_SCENES = {"tiny_long": _tiny_long, "tiny": scenes.SCENES["tiny"], "thin": _thin}
_oracle = {}


def edges_of(n, chunks):
    return [int(e) for e in sphmi.step_chunk_edges(n, chunks)]


def oracle_states(name, max_iteration=None):
    """Canonical buffers of the oracle after each of STEPS steps (CPU only): computed once per scene, shared, never changed."""
    key = (name, max_iteration)
    if key not in _oracle:
        sc = PARITY_SCENES[name]()
        if max_iteration is not None:
            sc["cfg"].maxIteration = max_iteration
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for _ in range(STEPS):
            ora.step()
            out.append(canon_ora(ora, N))
        ora.close()
        _oracle[key] = out
    return _oracle[key]


def search_tables(canon):
    """(sorted cell ids, cell table) of the search of the step that left `canon`."""
    return canon["particleIndex"].reshape(-1, 2)[:, 0].astype(np.uint32), canon["gridCellIndexFixedUp"].astype(np.uint32)


def halo_check(canon, cfg, chunks):
    keys, start = search_tables(canon)
    assert start.size == cfg.gridCellCount + 1
    return sphmi.step_halo_check(keys, start, edges_of(keys.size, chunks), cfg.gridCellsX, cfg.gridCellsY)


def chunk_window(n, chunks):
    """Per sorted particle: the first and one past the last sorted index of chunks c - 1 .. c + 1 of its own chunk c."""
    e = np.array(edges_of(n, chunks), np.int64)
    c = np.searchsorted(e[1:], np.arange(n), side="right")  # (empty chunks: the particle's chunk is the one that holds it)
    return e[np.maximum(c - 1, 0)], e[np.minimum(c + 2, chunks)]


def rows_stay_in_the_halo(canon, chunks):
    """Brute force over the neighbour rows: no particle has a neighbour outside chunks c - 1 .. c + 1."""
    n = canon["particleIndex"].size // 2
    ids = canon["neighborIds"].reshape(n, 32).astype(np.int64)
    below, above = chunk_window(n, chunks)
    return bool(((ids < 0) | ((ids >= below[:, None]) & (ids < above[:, None]))).all())


def cells_stay_in_the_halo(keys, start, edges, gx, gy):
    """Brute force over the 27 cells the search can look at from a particle's cell (ids wrapped and clamped as findNeighbors does):
    every particle in one of them lies in chunks c - 1 .. c + 1."""
    keys = np.asarray(keys, np.int64)
    start = np.asarray(start, np.int64)
    n, G, chunks = keys.size, start.size - 1, len(edges) - 1
    e = np.asarray(edges, np.int64)
    c = np.searchsorted(e[1:], np.arange(n), side="right")
    below, above = e[np.maximum(c - 1, 0)], e[np.minimum(c + 2, chunks)]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cell = keys + dx + dy * gx + dz * gx * gy
                cell = np.where(cell < 0, cell + G, cell)
                cell = np.where(cell >= G, cell - G, cell)
                cell = np.clip(cell, 0, G - 1)
                lo, hi = start[cell], start[cell + 1]
                if ((hi > lo) & ((lo < below) | (hi > above))).any():
                    return False
    return True


# ---------------------------------------------------------------------------------------------- the launch order (no GPU)
@pytest.mark.parametrize("chunks", range(1, 17))
def test_schedule_orders_every_dependency(chunks):
    for depth in range(7):
        for M in (1, 2, 3):
            for elastic in (False, True):
                D, items = sphmi.step_pipeline_schedule(chunks, depth, M, elastic)
                assert D == (min(depth, 1) if elastic else min(depth, 2 * M))
                where = "C=%d depth=%d M=%d elastic=%s" % (chunks, depth, M, elastic)
                at = {it: i for i, it in enumerate(items)}
                assert len(at) == len(items), where                                     # nothing twice ...
                assert set(at) == {(k, c) for k in range(D + 1) for c in range(chunks)}, where  # ... everything once
                for k in range(1, D + 1):
                    for c in range(chunks):
                        for cc in (c - 1, c, c + 1):  # (k = 1: stage 0 is density and pack)
                            if 0 <= cc < chunks:
                                assert at[(k, c)] > at[(k - 1, cc)], where
                        if c > 0:
                            assert at[(k, c)] > at[(k, c - 1)], where


def test_schedule_rejects_bad_arguments():
    for chunks, depth, M in ((0, 1, 3), (4, -1, 3), (4, 7, 3), (4, 1, -1)):
        with pytest.raises(sphmi.SphError):
            sphmi.step_pipeline_schedule(chunks, depth, M)


# ---------------------------------------------------------------------------------------------- the halo check (no GPU)
HALO_CASES = [("tiny_long", 2, True), ("tiny_long", 3, True), ("tiny", 7, False), ("tiny", 16, False), ("tiny_long", 16, True),
              ("thin", 16, True)]


@pytest.mark.parametrize("name,chunks,expect", HALO_CASES)
def test_halo_check_against_the_oracles_neighbour_rows(name, chunks, expect):
    """On every step of the scenes the GPU tests run: a check that passes implies that no row holds a neighbour outside chunks
    c - 1 .. c + 1 and that no cell the search can look at does; `expect` is the premise the GPU tests of that case rest on."""
    cfg = PARITY_SCENES[name]()["cfg"]
    for it, canon in enumerate(oracle_states(name)):
        ok = halo_check(canon, cfg, chunks)
        if expect is not None:
            assert ok == expect, "step %d" % it
        keys, start = search_tables(canon)
        cells = cells_stay_in_the_halo(keys, start, edges_of(keys.size, chunks), cfg.gridCellsX, cfg.gridCellsY)
        if ok:
            assert cells and rows_stay_in_the_halo(canon, chunks), "step %d: the check passed" % it
        if expect is False:
            assert not cells, "step %d: the scene is meant to break the premise, not only the check" % it


def _edge_scene():
    """1024 particles in a 4 x 4 x 80 grid (reach 21 cells), four chunks of 256. Chunks 2 and 3 hold one particle per cell from cell
    600 on, chunk 1 fills the 21 cells below cell 600, chunk 0 one particle per cell below those. The lowest cell chunk 2 can see
    (600 - 21) then starts exactly at edge 1, and the cell behind the highest one chunk 0 can see exactly at edge 2."""
    gx = gy = 4
    G = gx * gy * 80
    keys = np.empty(1024, np.int64)
    keys[512:] = 600 + np.arange(512)
    keys[256:512] = 579 + np.arange(256) * 21 // 256
    keys[:256] = 579 - 256 + np.arange(256)
    assert (np.diff(keys) >= 0).all()
    start = np.searchsorted(keys, np.arange(G + 1)).astype(np.uint32)
    return keys.astype(np.uint32), start, gx, gy


def test_halo_check_at_its_edge():
    """Chunk 2's lowest visible cell starts exactly at edge 1 (passes); one more particle of chunk 0 in that cell (fails, and the
    brute force agrees that a visible cell then reaches into chunk 0)."""
    edges = edges_of(1024, 4)
    keys, start, gx, gy = _edge_scene()
    reach = gx * gy + gx + 1
    assert start[int(keys[512]) - reach] == edges[1]
    assert sphmi.step_halo_check(keys, start, edges, gx, gy)
    assert cells_stay_in_the_halo(keys, start, edges, gx, gy)
    # the last particle of chunk 0 moves into the first cell of chunk 1: that cell now starts one index below edge 1
    moved = keys.copy()
    moved[255] = moved[256]
    start2 = np.searchsorted(moved, np.arange(start.size)).astype(np.uint32)
    start2[-1] = moved.size
    assert start2[int(moved[512]) - reach] == edges[1] - 1
    assert not sphmi.step_halo_check(moved, start2, edges, gx, gy)
    assert not cells_stay_in_the_halo(moved, start2, edges, gx, gy)


@pytest.mark.parametrize("seed", range(8))
def test_halo_check_is_never_permissive_on_random_tables(seed):
    """Random sorted cell ids over small grids, wrapped cells, empty chunks, keys outside the table: whenever the check passes,
    the brute force over the 27 cells agrees."""
    rng = np.random.default_rng(7000 + seed)
    passed = 0
    for _ in range(300):
        gx, gy, gz = (int(rng.integers(1, 5)) for _ in range(3))
        gz *= int(rng.integers(1, 40))
        G = gx * gy * gz
        n = int(rng.integers(1, 3000))
        chunks = int(rng.integers(1, 17))
        span = int(rng.integers(1, G + 1))
        keys = np.sort(rng.integers(0, span, n) + int(rng.integers(0, G - span + 1)))
        if rng.random() < 0.1:
            keys[-1] = G + int(rng.integers(0, 5))  # a key outside the table
        start = np.searchsorted(keys, np.arange(G + 1)).astype(np.uint32)
        start[G] = n
        edges = edges_of(n, chunks)
        ok = sphmi.step_halo_check(keys.astype(np.uint32), start, edges, gx, gy)
        if ok:
            passed += 1
            assert keys[-1] < G
            assert cells_stay_in_the_halo(keys, start, edges, gx, gy), (gx, gy, gz, n, chunks)
    assert passed > 20


def test_halo_check_rejects_bad_arguments():
    keys, start = np.zeros(4, np.uint32), np.array([0, 4], np.uint32)
    with pytest.raises(sphmi.SphError):
        sphmi.step_halo_check(keys, start, [0, 3], 1, 1)       # the edges do not end at n
    with pytest.raises(sphmi.SphError):
        sphmi.step_halo_check(keys, start, [0, 4], 0, 1)
    assert sphmi.step_halo_check(keys, start, [0, 4], 1, 1)     # one chunk sees everything


# ---------------------------------------------------------------------------------------------- on the GPU
_serial = {}


def serial_states(name, max_iteration=None):
    """Canonical buffers of the serial step (chunk count 1) after steps 1 and STEPS: once per scene, shared, never changed."""
    key = (name, max_iteration)
    if key not in _serial:
        sc = PARITY_SCENES[name]()
        if max_iteration is not None:
            sc["cfg"].maxIteration = max_iteration
        N = sc["cfg"].particleCount
        hip = scenes.hip_for(sc)
        hip.set_step_chunks(1)
        out = {}
        for it in range(STEPS):
            hip.step(it)
            if it in (0, STEPS - 1):
                out[it] = canon_hip(hip, N)
        hip.close()
        _serial[key] = out
    return _serial[key]


def piped_solver(sc, chunks, depth):
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    return hip


def run_against_references(name, chunks, depth, max_iteration=None):
    """STEPS steps at (chunks, depth): every canonical buffer equals the oracle's and the serial step's after steps 1 and STEPS.
    Returns the debug counters."""
    sc = PARITY_SCENES[name]()
    if max_iteration is not None:
        sc["cfg"].maxIteration = max_iteration
    N = sc["cfg"].particleCount
    ora, ser = oracle_states(name, max_iteration), serial_states(name, max_iteration)
    hip = piped_solver(sc, chunks, depth)
    where = "%s, %d chunks, depth %d" % (name, chunks, depth)
    for it in range(STEPS):
        hip.step(it)
        if it in ser:
            got = canon_hip(hip, N)
            assert_same(got, ora[it], "%s, step %d, against the oracle" % (where, it), FUSED_SKIP)
            assert_same(got, ser[it], "%s, step %d, against the serial step" % (where, it), FUSED_SKIP)
    counters = hip.buffer("debugCounters")
    hip.close()
    return counters


def premise(name, chunks, max_iteration=None):
    """What the halo check says on each of the STEPS steps, from the oracle's cell tables (CPU)."""
    cfg = PARITY_SCENES[name]()["cfg"]
    return [halo_check(c, cfg, chunks) for c in oracle_states(name, max_iteration)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("chunks", [2, 3])
def test_every_depth_on_chunks_wider_than_the_halo(chunks, depth):
    assert all(premise("tiny_long", chunks)), "the check must pass on every step"
    N = PARITY_SCENES["tiny_long"]()["cfg"].particleCount
    assert N % (BLOCK * chunks) != 0
    c = run_against_references("tiny_long", chunks, depth)
    assert c[DBG_PIPED] == STEPS and c[DBG_SERIAL] == 0


@pytest.mark.gpu
def test_chunks_thinner_than_a_cell_layer_take_the_serial_table():
    assert not any(premise("tiny", 7)), "the check must fail on every step"
    c = run_against_references("tiny", 7, 6)
    assert c[DBG_SERIAL] == STEPS and c[DBG_PIPED] == 0


@pytest.mark.gpu
def test_serial_table_over_more_blocks_than_the_grid_stride_launch_has():
    """The launches over all particles loop over the blocks of 256 particles with a grid of 2048 blocks (SPH_SERIAL_GRID,
    csrc/sph_pcisph.hip); only a scene of more than 2048 x 256 particles makes a block take a second turn. A flat slab, four cell
    layers high: sixteen chunks are a quarter of a layer each, so the check fails and all six stages take those launches."""
    sc = scenes.liquid_box((480.0, 26.0, 8.0), (1000, 42, 10), mask=0xffffffff)
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert (N + BLOCK - 1) // BLOCK > 2048
    ora = scenes.oracle_for(sc, threads=8)
    for st in ("hashParticles", "sort", "sortPostPass", "indexx", "indexPostPass"):  # (the oracle's cell table; no search)
        ora.run(st)
    keys = ora.buffer("particleIndex").reshape(-1, 2)[:, 0].astype(np.uint32)
    start = ora.buffer("gridCellIndexFixedUp").astype(np.uint32)
    ora.close()
    assert not sphmi.step_halo_check(keys, start, edges_of(N, 16), cfg.gridCellsX, cfg.gridCellsY)
    solvers = [piped_solver(sc, chunks, depth) for chunks, depth in ((1, -1), (16, 6))]
    for it in range(2):
        for hip in solvers:
            hip.step(it)
    for name in ("position", "velocity", "acceleration", "pressure", "rho", "sortedPosition"):
        assert scenes.bits_equal(solvers[1].buffer(name), solvers[0].buffer(name)), name
    c = solvers[1].buffer("debugCounters")
    assert c[DBG_SERIAL] == 2 and c[DBG_PIPED] == 0
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
def test_depth_zero_runs_no_check():
    c = run_against_references("tiny_long", 3, 0)
    assert c[DBG_SERIAL] == 0 and c[DBG_PIPED] == 0


@pytest.mark.gpu
def test_more_chunks_than_blocks_on_the_serial_table():
    N = PARITY_SCENES["tiny"]()["cfg"].particleCount
    e = edges_of(N, 16)
    assert (N + BLOCK - 1) // BLOCK < 16 and any(b == a for a, b in zip(e, e[1:])), "some chunks must be empty"
    assert not any(premise("tiny", 16))
    c = run_against_references("tiny", 16, 6)
    assert c[DBG_SERIAL] == STEPS and c[DBG_PIPED] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 6])
def test_an_empty_chunk_and_a_last_chunk_shorter_than_one_wave(depth):
    """Sixteen chunks of at most one block, chunk by chunk: an empty chunk, and 48 particles in the last one."""
    N = PARITY_SCENES["thin"]()["cfg"].particleCount
    e = edges_of(N, 16)
    assert sum(b == a for a, b in zip(e, e[1:])) == 1 and 0 < e[16] - e[15] < 64 and max(b - a for a, b in zip(e, e[1:])) == BLOCK
    assert all(premise("thin", 16)), "the check must pass on every step"
    c = run_against_references("thin", 16, depth)
    assert c[DBG_PIPED] == STEPS and c[DBG_SERIAL] == 0


@pytest.mark.gpu
def test_sixteen_chunks_chunk_by_chunk():
    assert all(premise("tiny_long", 16))
    c = run_against_references("tiny_long", 16, 6)
    assert c[DBG_PIPED] == STEPS and c[DBG_SERIAL] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2])
def test_depth_is_clamped_to_the_stages_the_step_has(iterations):
    assert sphmi.step_pipeline_schedule(3, 6, iterations)[0] == 2 * iterations
    assert all(premise("tiny_long", 3, iterations))
    c = run_against_references("tiny_long", 3, 6, max_iteration=iterations)
    assert c[DBG_PIPED] == STEPS and c[DBG_SERIAL] == 0


@pytest.mark.gpu
def test_worm_scene_with_muscles_equals_the_serial_step():
    """Elastic matter: depth 6 clamps to 1 (the forces kernel alone); k_elastic and the membrane kernels run behind the join."""
    assert sphmi.step_pipeline_schedule(3, 6, 3, True)[0] == 1
    solvers = [piped_solver(scenes.worm_scene(), chunks, depth) for chunks, depth in ((1, -1), (3, 6))]
    N = solvers[0].N
    for it in range(3):
        for hip in solvers:
            hip.step(it)
            hip.updateMuscleActivityData(sphmi.muscle_signal(it))
    assert_same(canon_hip(solvers[1], N), canon_hip(solvers[0], N), "worm, 3 chunks at depth 6 against the serial step", FUSED_SKIP)
    assert np.abs(canon_hip(solvers[0], N)["acceleration"]).max() > 0
    c = solvers[1].buffer("debugCounters")
    assert c[DBG_PIPED] + c[DBG_SERIAL] == 3
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
def test_exact_walks_on_both_sides_of_a_chunk_edge():
    """The overcrowded scene of test_step_overlap.py: rows without a 16-bit copy on both sides of the edge. Two chunks always pass
    the check (chunks c - 1 .. c + 1 are everything), so all six stages read those rows chunk by chunk."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (18, 18, 18), spacing_in_r0=0.45, origin_in_r0=(4.0, 4.0, 4.0))
    N = sc["cfg"].particleCount
    edge = edges_of(N, 2)[1]
    hip, ora = piped_solver(sc, 2, 6), scenes.oracle_for(sc, threads=8)
    for it in range(2):
        hip.step(it)
        ora.step()
    got = canon_hip(hip, N)
    assert_same(got, canon_ora(ora, N), "overcrowded cells, 2 chunks, depth 6", FUSED_SKIP)
    ora.close()
    c = hip.buffer("debugCounters")
    assert c[1] > 0 or c[2] > 0
    assert c[DBG_PIPED] == 2 and c[DBG_SERIAL] == 0
    crowded = scenes.crowded_particles(got, sc["cfg"].h)
    assert (crowded < edge).sum() > 100 and (crowded >= edge).sum() > 100
    hip.close()


@pytest.mark.gpu
def test_blob_scene_with_wide_rows_equals_the_serial_step():
    """scenes.elastic_hard_box(blob=True): a crowded blob around an elastic sheet (exact walks, rows with 32-bit ids only), two
    chunks, depth 6 clamped to 1 by the elastic matter."""
    solvers = [piped_solver(scenes.elastic_hard_box(blob=True), chunks, depth) for chunks, depth in ((1, -1), (2, 6))]
    N = solvers[0].N
    for it in range(2):
        for hip in solvers:
            hip.step(it)
    got = canon_hip(solvers[1], N)
    assert_same(got, canon_hip(solvers[0], N), "blob, 2 chunks at depth 6 against the serial step", FUSED_SKIP)
    c = solvers[1].buffer("debugCounters")
    assert c[0] + c[1] > 0 and c[DBG_PIPED] == 2
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
def test_stage_timing_switched_between_steps():
    """With stage timing on the step takes the serial path; switching it between steps alternates the two paths on one solver."""
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = oracle_states("tiny_long")
    hip = piped_solver(sc, 3, 6)
    timed = 0
    for it in range(STEPS):
        hip.set_stage_timing(it % 2 == 1)
        timed += it % 2
        hip.step(it)
        assert_same(canon_hip(hip, N), want[it], "timing toggled, step %d" % it, FUSED_SKIP)
    t = hip.stage_times()
    M = sc["cfg"].maxIteration
    assert timed == 2
    assert t["find_neighbors"][1] == timed and t["density"][1] == timed and t["forces"][1] == timed
    assert t["predict_density"][1] == M * timed and t["pressure_force"][1] == M * timed
    c = hip.buffer("debugCounters")
    assert c[DBG_PIPED] == STEPS - timed and c[DBG_SERIAL] == 0
    hip.close()


@pytest.mark.gpu
def test_async_position_read_back_after_every_step():
    """At depth 6 the kernel that writes the positions runs on the chunk stream: it must wait for the copy of the step before."""
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = oracle_states("tiny_long")
    hip = piped_solver(sc, 3, 6)
    bufs = [np.empty((N, 4), np.float32), np.empty((N, 4), np.float32)]
    for it in range(STEPS):
        hip.step(it)
        hip.read_position_buffer_async(bufs[it & 1])  # (waits for the copy of step it - 1 first)
        if it > 0:
            assert scenes.bits_equal(bufs[(it - 1) & 1], want[it - 1]["position"]), "step %d" % (it - 1)
    hip.wait_position_buffer()
    assert scenes.bits_equal(bufs[(STEPS - 1) & 1], want[STEPS - 1]["position"])
    assert scenes.bits_equal(hip.read_position_buffer(), bufs[(STEPS - 1) & 1])  # the blocking read
    hip.close()


@pytest.mark.gpu
def test_removal_and_emission_between_steps():
    """N changes between steps, and with it the chunk edges and the tables of the check: twin solvers through the same edits."""
    solvers = [piped_solver(PARITY_SCENES["tiny_long"](), chunks, depth) for chunks, depth in ((1, -1), (3, 6))]
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
        assert hip.emit_lattice((6 * r0, 6 * r0, 6 * r0), (r0, r0, r0), (5, 4, 7)) == 140
        ns.append(hip.N)
        hip.step(3)
        hip.step(4)
        counts.append(ns)
    assert counts[0] == counts[1]
    N = solvers[0].N
    assert_same(canon_hip(solvers[1], N), canon_hip(solvers[0], N), "edits between steps, depth 6 against the serial step", FUSED_SKIP)
    c = solvers[1].buffer("debugCounters")
    assert c[DBG_PIPED] + c[DBG_SERIAL] == 5 and c[DBG_PIPED] > 0
    for hip in solvers:
        hip.close()


@pytest.mark.gpu
def test_closing_a_solver_right_after_a_step():
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    for _ in range(3):
        hip = piped_solver(sc, 3, 6)
        hip.step(0)
        hip.close()  # launches of all three streams are still in flight
    hip = piped_solver(sc, 3, 6)
    hip.step(0)
    assert_same(canon_hip(hip, N), oracle_states("tiny_long")[0], "a solver created after the closed ones", FUSED_SKIP)
    hip.close()


@pytest.mark.gpu
def test_two_solvers_with_different_depths():
    sc = PARITY_SCENES["tiny_long"]()
    N = sc["cfg"].particleCount
    want = oracle_states("tiny_long")
    solvers = [piped_solver(sc, 3, 2), piped_solver(sc, 2, 5)]
    for it in range(STEPS):
        for hip in solvers:
            hip.step(it)
    for hip in solvers:
        assert_same(canon_hip(hip, N), want[STEPS - 1], "two solvers alive", FUSED_SKIP)
        assert hip.buffer("debugCounters")[DBG_PIPED] == STEPS
        hip.close()


@pytest.mark.gpu
def test_depth_is_checked():
    hip = scenes.hip_for(PARITY_SCENES["tiny"]())
    for bad in (-2, 7):
        with pytest.raises(sphmi.SphError):
            hip.set_step_pipeline(bad)
    hip.set_step_pipeline(-1)
    hip.close()
