"""The staging rounds of findNeighbors (csrc/sph_neighbors.hip): a workgroup copies the candidates of its nine runs into LDS in
rounds of 2048 (8 per thread), and every thread of a round loads without a branch — a slot past the end reads the last candidate
again and is not stored. What can go wrong is the end of the last round, so the scenes are chosen by the number of candidates per
workgroup, restated here from the oracle's sorted cell ids and cell table: fewer than three per thread, no multiple of 2048, more
than one round, more than the LDS holds (the workgroup then splits itself into batches, and may drop runs), a workgroup that ends
in a partial tile, runs clamped at both ends of the cell table. Results are the reference's, bit for bit, serial and in chunks."""
import numpy as np
import pytest

import bench
import scenes
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

TILE = 128        # FN_PART: sorted particles per workgroup
THREADS = 256     # FN_THREADS
ROUND = 8 * 256   # FN_STAGE_PER * FN_THREADS: candidates per staging round
CAND_CAP = 4096   # FN_CAND_CAP: staged candidates per workgroup
STEPS = 3


def _tiny_long():
    box, lattice, mask = bench.WORKLOADS["tiny_long"]  # 30 cell layers, wide cell ids
    return scenes.liquid_box(box, lattice, mask=mask)


def _dense():
    """~700 particles per cell: the nine runs of a tile exceed the LDS capacity, so the workgroup serves it in batches."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (18, 18, 18), spacing_in_r0=0.45, origin_in_r0=(4.0, 4.0, 4.0))


def _sparse():
    """Most cells hold one particle: workgroups with two or three candidates per thread."""
    return scenes.liquid_box((6.0, 5.0, 7.0), (3, 3, 3), spacing_in_r0=2.9)


def _tight():
    """`tiny` on a grid cut down to the four cell layers it occupies. The reference declares twice as many cells per axis as the
    box is long (it divides by h, not by the cell size 2h), so in a box scene no cell id comes near G and no run is clamped at the
    table's upper end; here the last layer's runs are, and its particles' upper cells wrap round to the first layer."""
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    cfg.gridCellsZ = 4
    cfg.gridCellCount = cfg.gridCellsX * cfg.gridCellsY * cfg.gridCellsZ
    return sc


SCENE = {"tiny": scenes.SCENES["tiny"], "tiny_long": _tiny_long, "dense": _dense, "sparse": _sparse, "tight": _tight}
_oracle = {}


def oracle_states(name):
    """Canonical buffers of the oracle after each of STEPS steps (CPU only): computed once per scene, shared, never changed."""
    if name not in _oracle:
        sc = SCENE[name]()
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for _ in range(STEPS):
            ora.step()
            out.append(canon_ora(ora, N))
        ora.close()
        _oracle[name] = out
    return _oracle[name]


def staged_totals(canon, cfg):
    """Per workgroup (128 sorted particles): the candidates it stages when it serves its tile whole — the nine runs of the cells
    cLo - 1 .. cHi + 1 of the 3 x 3 rows around its own x-row, table reads clamped to [0, G] — and the unclamped cells of the run
    ends, int64[tiles, 9, 2]."""
    keys = canon["particleIndex"].reshape(-1, 2)[:, 0].astype(np.int64)
    start = canon["gridCellIndexFixedUp"].astype(np.int64)
    G, gx, gy = start.size - 1, cfg.gridCellsX, cfg.gridCellsY
    assert G == cfg.gridCellCount
    first = np.arange(0, keys.size, TILE)
    cLo, cHi = keys[first], keys[np.minimum(first + TILE, keys.size) - 1]
    shift = np.array([(r % 3 - 1) * gx + (r // 3 - 1) * gx * gy for r in range(9)], np.int64)
    cells = np.stack([cLo[:, None] - 1 + shift[None, :], cHi[:, None] + 2 + shift[None, :]], 2)
    ends = start[np.clip(cells, 0, G)]
    return np.maximum(ends[:, :, 1] - ends[:, :, 0], 0).sum(1), cells


def test_scenes_hold_the_cases_of_the_last_round():
    seen = {}
    for name in SCENE:
        cfg = SCENE[name]()["cfg"]
        total, cells = staged_totals(oracle_states(name)[0], cfg)
        seen[name] = total
        print("%s: N %d, candidates per workgroup %d .. %d, %d workgroups above the LDS capacity"
              % (name, cfg.particleCount, total.min(), total.max(), int((total > CAND_CAP).sum())))
        assert (cells[:, :, 0] < 0).any(), name + ": no run is clamped at cell < 0"
    # one round in which the later loads of every thread lie past the end; the last workgroup's tile is partial
    assert (seen["sparse"] < 3 * THREADS).any() and SCENE["sparse"]()["cfg"].particleCount % TILE != 0
    assert ((seen["tiny"] > ROUND) & (seen["tiny"] <= CAND_CAP) & (seen["tiny"] % ROUND != 0)).any()   # two rounds, the second partial
    assert ((seen["tiny"] < ROUND) & (seen["tiny"] % THREADS != 0)).any()                              # one partial round
    assert (seen["dense"] > CAND_CAP).any()
    cfg = SCENE["tight"]()["cfg"]
    _, cells = staged_totals(oracle_states("tight")[0], cfg)
    assert (cells[:, :, 1] > cfg.gridCellCount).any() and (cells[:, :, 0] > cfg.gridCellCount - 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,chunks", [(n, 1) for n in SCENE] + [("tiny_long", 2), ("tiny_long", 16), ("dense", 2), ("tight", 2)])
def test_rows_equal_the_oracle(name, chunks):
    """Every buffer, the neighbour rows among them (ids decoded from the 16-bit rows and their bases, or the 32-bit rows where a row
    is marked wide; distances), equals the oracle's after steps 1 and 3 — serial, and with the search launched in chunks on two
    streams with the forces kernel behind it. debugCounters[3] (candidate runs dropped) stays 0 where no workgroup exceeds the LDS
    capacity; [0] + [1] (particles handed to the exact walk) is at least the number of particles with more than 96 others within h."""
    sc = SCENE[name]()
    N = sc["cfg"].particleCount
    want = oracle_states(name)
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(1 if chunks > 1 else -1)
    hip.reset_stage_times()
    seen = {}
    for it in range(STEPS):
        hip.step(it)
        if it in (0, STEPS - 1):
            assert_same(canon_hip(hip, N), want[it], "%s, %d chunks, step %d" % (name, chunks, it), FUSED_SKIP)
            seen[it] = hip.buffer("debugCounters")[:4].astype(np.int64)
    print("%s, %d chunks: debugCounters[0..3] after steps 1 and 3: %s %s" % (name, chunks, seen[0].tolist(), seen[STEPS - 1].tolist()))
    if not any((staged_totals(w, sc["cfg"])[0] > CAND_CAP).any() for w in want):
        assert seen[STEPS - 1][3] == 0, "a candidate run was dropped although every workgroup fits the LDS capacity"
    crowded = scenes.crowded_particles(want[0], sc["cfg"].h).size
    walks = int(seen[0][0] + seen[0][1])
    assert walks >= crowded, "fewer exact walks (%d) than particles with more than 96 others within h (%d)" % (walks, crowded)
    if name == "dense":
        assert crowded > 0
    key = (name, "counters")
    if key in _oracle:  # the serial run of the scene came first: the counters do not depend on the launches
        assert np.array_equal(seen[STEPS - 1], _oracle[key]), (seen[STEPS - 1], _oracle[key])
    elif chunks == 1:
        _oracle[key] = seen[STEPS - 1]
    hip.close()
