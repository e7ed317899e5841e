"""What a slab solver computes on the way, on the GPU: its cell table wherever a kernel can read it, the neighbour
rows of every particle within the search depth, the density within the density depth, the owned state, and how many particles
take the exact walk — against the oracle on the same local particle set (tests/test_slab_structures_host.py asserts that this
equals the single domain). The scene (slab_ref.corner_scene) has liquid resting in the low corner of the box, whose walks reach
a cell that searchCell wraps to the other end of the table; several steps with a growing local count follow."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
import slab_ref as R
import sphmi
from sphmi import slab as S
from test_slab import HERE, check_union, free_port, run_ranks, single_domain_reference
from test_slab_structures_host import CORNER, CUTS2, DRIFT_DOWN, DRIFT_STEPS

pytestmark = pytest.mark.gpu

_cache = {}


def _scene():
    if "sc" not in _cache:
        _cache["sc"] = R.corner_scene()
    return _cache["sc"]


def slab_step(cuts, rank):
    """One step of a fresh HIP slab solver on a rank's local set of the corner scene, and of the oracle on the same set; every buffer
    the tests look at, computed once and left unchanged."""
    key = (tuple(cuts), rank)
    if key in _cache:
        return _cache[key]
    sc = _scene()
    slab, idx = R.rank_setup(sc, cuts, rank)
    cfg = R.corner_scene()["cfg"]  # (HipSlabBackend sets the particle count and capacity of the config it is given)
    pos0, vel0 = sc["position"][idx], sc["velocity"][idx]
    be = S.HipSlabBackend(cfg, pos0, vel0, idx, slab)
    be.step(0)
    sv = be.solver
    n = idx.size
    pi = sv.buffer("particleIndex")
    pos, vel, gid, owned = sv.slab_read()
    assert np.array_equal(gid, idx)
    hip = dict(table=sv.buffer("gridCellIndexFixedUp").astype(np.int64), dbg=sv.buffer("debugCounters"),
               rows=R.rows_by_global_id(sv.buffer("neighborMap"), pi, idx), rho=R.by_global_id(sv.buffer("rho")[:n], pi, idx),
               pos=pos, vel=vel, owned=owned.astype(bool))
    del be, sv
    o = R.oracle_step_on(sc, idx)
    opi = o.buffer("particleIndex")
    ora = dict(rows=R.rows_by_global_id(o.buffer("neighborMap"), opi, idx), rho=R.by_global_id(o.buffer("rho")[:n], opi, idx),
               pos=o.buffer("position").reshape(-1, 4)[:n].copy(), vel=o.buffer("velocity").reshape(-1, 4)[:n].copy())
    o.close()
    _cache[key] = dict(sc=sc, cfg=sc["cfg"], slab=slab, idx=idx, pos0=pos0, vel0=vel0, hip=hip, ora=ora)
    return _cache[key]


def _table_report(cells, got, want):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return "%d of %d table entries differ; first: cell %d holds %d, true %d" % (bad.size, cells.size, int(cells[i]), int(got[i]), int(want[i]))


@pytest.mark.parametrize("cuts,rank", [(CUTS2, 0), (CUTS2, 1), (R.CORNER_CUTS3, 1)])
def test_cell_table_is_true_wherever_a_kernel_reads_it(cuts, rank):
    """After a step, gridCellIndexFixedUp equals the true table (searchsorted of the sorted cell ids) at every entry a kernel can
    read: [c] and [c + 1] of each of the eight WRAPPED reference cells of every local particle within the search depth; the two
    ends; the first cell of every layer a ranged launch can start or end at; and the span the search stages its candidates from
    (the layers of those particles, one layer up and down, two cells beyond)."""
    r = slab_step(cuts, rank)
    cfg, slab, pos = r["cfg"], r["slab"], r["pos0"]
    G, lc, gz = cfg.gridCellCount, cfg.gridCellsX * cfg.gridCellsY, cfg.gridCellsZ
    truth = R.true_cell_table(pos, cfg)
    within = R.in_layers(pos, cfg, slab, R.SEARCH_DEPTH)
    _, wrapped = R.reference_cells(pos[within], cfg)
    walk = np.unique(wrapped)
    assert walk.min() >= 0 and walk.max() < G
    lay = S.particle_layers(pos[within], cfg)
    span = np.arange(max((int(lay.min()) - 1) * lc - 2, 0), min((int(lay.max()) + 2) * lc + 2, G) + 1)
    W = slab.ghostLayers
    ranged = np.arange(max(slab.layerLo - W, 0), min(slab.layerHi + W, gz) + 1) * lc
    cells = np.unique(np.concatenate([walk, walk + 1, [0, G], ranged, span]))
    if rank == 0:
        assert G - 1 in walk and G - 1 not in span  # the wrapped cell is read, and lies outside the contiguous span
    got, want = r["hip"]["table"][cells], truth[cells]
    assert np.array_equal(got, want), _table_report(cells, got, want)


@pytest.mark.parametrize("rank", [0, 1])
def test_rows_density_and_state_equal_the_oracle_on_the_local_set(rank):
    r = slab_step(CUTS2, rank)
    cfg, slab, pos0, hip, ora = r["cfg"], r["slab"], r["pos0"], r["hip"], r["ora"]
    sel = R.in_layers(pos0, cfg, slab, R.SEARCH_DEPTH)
    assert (pos0[sel, 3].astype(np.int32) == sphmi.BOUNDARY_PARTICLE).any()  # boundary rows are compared too
    diff = R.first_row_difference(hip["rows"], ora["rows"], sel, pos0, cfg)
    assert diff is None, diff
    sel = R.in_layers(pos0, cfg, slab, R.DENSITY_DEPTH)
    assert scenes.bits_equal(hip["rho"][sel], ora["rho"][sel]), \
        "rho of global id %d: %s" % (int(r["idx"][sel][np.flatnonzero(hip["rho"][sel].view(np.uint32) != ora["rho"][sel].view(np.uint32))[0]]),
                                     scenes.diff_report(hip["rho"][sel], ora["rho"][sel]))
    own = hip["owned"]
    assert np.array_equal(own, R.in_layers(pos0, cfg, slab, R.FORCES_DEPTH))
    assert scenes.bits_equal(hip["pos"][own], ora["pos"][own]), scenes.diff_report(hip["pos"][own], ora["pos"][own])
    assert scenes.bits_equal(hip["vel"][own], ora["vel"][own]), scenes.diff_report(hip["vel"][own], ora["vel"][own])


def test_no_exact_walk_because_of_a_stale_table_entry():
    """debugCounters[0] — particles handed to the exact walk because a non-empty cell of theirs was not staged — of the rank-0 slab
    solver after one step is at most that of a plain solver on the same local set, which computes the whole table and searches
    every particle. No candidate run was dropped in either ([3]), which would be another cause."""
    r = slab_step(CUTS2, 0)
    cfg = R.corner_scene()["cfg"]
    cfg.particleCount = int(r["idx"].size)
    plain = scenes.hip_for(dict(r["sc"], cfg=cfg, position=r["pos0"], velocity=r["vel0"]))
    plain.step(0)
    dbg = plain.buffer("debugCounters")
    print("exact walks for an unstaged cell: slab %d, plain %d" % (int(r["hip"]["dbg"][0]), int(dbg[0])))
    assert int(dbg[3]) == 0 and int(r["hip"]["dbg"][3]) == 0
    assert int(r["hip"]["dbg"][0]) <= int(dbg[0])


@pytest.mark.parametrize("env", [CORNER, DRIFT_DOWN], ids=["resting", "drifting_down"])
def test_corner_scene_two_ranks_equal_single_domain_gpu(tmp_path, env):
    """Five steps of two HIP ranks: the corner scene at rest, and the tall column drifting down, where rank 0's local count grows
    in every step (test_slab_structures_host.py asserts it), so every rebuild changes what the table's last entries must hold."""
    results = run_ranks("hip", 2, tmp_path, steps=DRIFT_STEPS, env=env)
    sc, pos_ref, vel_ref = single_domain_reference(steps=DRIFT_STEPS, env=env)
    check_union(results, sc, pos_ref, vel_ref)
    assert list(results[0]["cuts"]) == CUTS2
    if env is DRIFT_DOWN:
        assert (np.diff(results[0]["counts"]) > 0).sum() >= 2, results[0]["counts"]


def test_corner_scene_over_rccl_in_one_process(tmp_path):
    """The same scene through the asynchronous exchange (tests/rccl_pair_worker.py)."""
    steps = DRIFT_STEPS
    p = subprocess.run([sys.executable, os.path.join(HERE, "rccl_pair_worker.py"), "--steps", str(steps), "--port", str(free_port()),
                        "--out", str(tmp_path)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **CORNER))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    results = [np.load(os.path.join(tmp_path, "rank%d.npz" % k)) for k in range(2)]
    sc, pos_ref, vel_ref = single_domain_reference(steps=steps, env=CORNER)
    check_union(results, sc, pos_ref, vel_ref)
    assert all(bool(x["asynchronous"]) for x in results) and list(results[0]["cuts"]) == CUTS2
