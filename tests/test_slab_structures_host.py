"""What the GPU tests of tests/test_slab_structures.py rest on, asserted against the oracle alone (no GPU): the corner scene really
sends liquid walks into a wrapped cell that rank 0's cell table does not compute; one oracle step on a rank's LOCAL particle set gives
the single domain's neighbour rows (search depth) and densities (density depth), so the oracle on the local set is a valid
reference for a slab solver's structures; the drifting variant keeps such liquid in rank 0's range while its local count grows;
the slab exchange on this scene equals the single domain. And the frame-length rule of the asynchronous exchange:
both ends of a link post the agreed length even when it outgrows the sender's frame."""
import numpy as np
import pytest

import scenes
import slab_ref as R
import sphmi
from sphmi import slab as S
from test_slab import check_union, run_ranks, single_domain_reference

CUTS2 = [0, 8, 20]
CORNER = {"SPHMI_TEST_CORNER_SCENE": "1"}
# The tall column drifting down 0.17 cell layers per step: rank 0 (layers below 12 local) receives new liquid in every step
DRIFT_DOWN = {"SPHMI_TEST_CORNER_SCENE": "tall", "SPHMI_TEST_VZ": "-0.45"}
DRIFT_STEPS = 5


@pytest.fixture(scope="module")
def corner():
    """The corner scene and one single-domain oracle step on it: rows and density keyed by global id."""
    sc = R.corner_scene()
    n = sc["cfg"].particleCount
    o = scenes.oracle_for(sc, threads=4)
    o.step()
    gid = np.arange(n)
    rows = R.rows_by_global_id(o.buffer("neighborMap"), o.buffer("particleIndex"), gid)
    rho = R.by_global_id(o.buffer("rho"), o.buffer("particleIndex"), gid)
    o.close()
    return dict(sc=sc, rows=rows, rho=rho)


def liquid_walking_into_cell_minus_one(position, cfg):
    """bool[n]: liquid particles one of whose eight reference cells has the raw index -1 (searchCell turns it into G - 1)."""
    raw, wrapped = R.reference_cells(position, cfg)
    hit = raw == -1
    assert np.all(wrapped[hit] == cfg.gridCellCount - 1)
    return hit.any(1) & (position[:, 3].astype(np.int32) == 1)


def test_corner_scene_sends_liquid_walks_into_the_wrapped_cell(corner):
    sc = corner["sc"]
    cfg = sc["cfg"]
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    assert S.balanced_cuts(S.particle_layers(sc["position"], cfg), 2) == CUTS2
    m = liquid_walking_into_cell_minus_one(sc["position"], cfg)
    cells = R.cell_ids(sc["position"], cfg)[m]
    for c in (0, gx, gx * gy, gx * gy + gx):
        assert (cells == c).sum() >= 1, "no liquid particle of cell %d walks into raw cell -1" % c
    # every wrapped cell a walk of this scene reaches lies in the last layer of the table, and raw cells never reach G
    raw, wrapped = R.reference_cells(sc["position"], cfg)
    assert raw.max() < cfg.gridCellCount and wrapped[raw < 0].min() >= cfg.gridCellCount - (gx * gy + gx + 1)


def test_rank0_computes_its_table_short_of_the_wrapped_cell(corner):
    sc = corner["sc"]
    cfg = sc["cfg"]
    G = cfg.gridCellCount
    slab, idx = R.rank_setup(sc, CUTS2, 0)
    assert slab.layerHi + slab.ghostLayers + 3 < cfg.gridCellsZ  # cell G - 1 is outside the range rank 0 computes
    assert idx.size <= 1 << 20                                   # (a run longer than that is not walked at all)
    for pos in (sc["position"], sc["position"][idx]):
        t = R.true_cell_table(pos, cfg)
        assert t[G] - t[G - 1] == 0 and t[G] == pos.shape[0]     # the wrapped cell is empty: a true row has no entry from it
    # and rank 0 holds liquid that walks there
    assert liquid_walking_into_cell_minus_one(sc["position"][idx], cfg).sum() >= 4


@pytest.mark.parametrize("cuts,rank", [(CUTS2, 0), (CUTS2, 1), (R.CORNER_CUTS3, 1)])
def test_oracle_on_the_local_set_equals_the_single_domain(corner, cuts, rank):
    """Rows (global ids and distance bits) of EVERY local particle within the search depth, boundary particles included, and the
    density within the density depth: no difference between one oracle step on the local set and on the whole scene."""
    sc = corner["sc"]
    cfg = sc["cfg"]
    slab, idx = R.rank_setup(sc, cuts, rank)
    pos = sc["position"][idx]
    o = R.oracle_step_on(sc, idx)
    rows = R.rows_by_global_id(o.buffer("neighborMap"), o.buffer("particleIndex"), idx)
    rho = R.by_global_id(o.buffer("rho"), o.buffer("particleIndex"), idx)
    table = o.buffer("gridCellIndexFixedUp").astype(np.int64)
    o.close()
    assert np.array_equal(table, R.true_cell_table(pos, cfg))  # the numpy table is the oracle's
    want = tuple(a[idx] for a in corner["rows"])
    sel = R.in_layers(pos, cfg, slab, R.SEARCH_DEPTH)
    assert sel.sum() > 5000 and (pos[sel, 3].astype(np.int32) == sphmi.BOUNDARY_PARTICLE).any()
    diff = R.first_row_difference(rows, want, sel, pos, cfg)
    assert diff is None, diff
    sel = R.in_layers(pos, cfg, slab, R.DENSITY_DEPTH)
    assert sel.sum() > 2000
    assert scenes.bits_equal(rho[sel], corner["rho"][idx][sel]), scenes.diff_report(rho[sel], corner["rho"][idx][sel])


def test_stage_depths_are_those_of_the_fused_step():
    assert (R.stage_depth(5), R.stage_depth(1), R.stage_depth(0)) == (R.SEARCH_DEPTH, R.DENSITY_DEPTH, R.FORCES_DEPTH)


@pytest.mark.parametrize("world,env", [(2, {}), (3, {"SPHMI_TEST_CUTS": ",".join(map(str, R.CORNER_CUTS3))})])
def test_corner_scene_slab_runs_equal_single_domain_cpu(tmp_path, world, env):
    env = dict(CORNER, **env)
    results = run_ranks("oracle", world, tmp_path, steps=3, env=env)
    sc, pos_ref, vel_ref = single_domain_reference(steps=3, env=env)
    assert sc["cfg"].particleCount == 14192
    check_union(results, sc, pos_ref, vel_ref)
    assert len(results[0]["cuts"]) == world + 1


def test_drifting_corner_scene_grows_rank0_and_keeps_liquid_at_the_wrap_cpu(tmp_path):
    """The drift variant of the GPU test: at the start of EVERY step rank 0 holds liquid whose walk reaches raw cell -1, rank 0's
    local count grows from one step to the next (so a table entry written once with an earlier count would be wrong), the state
    stays finite and slower than a layer per step, and the two-rank run equals the single domain."""
    sc = R.corner_scene(tall=True)
    cfg = sc["cfg"]
    n = cfg.particleCount
    nl = sc["numOfLiquidP"]
    sc["velocity"][:nl, 2] = np.float32(DRIFT_DOWN["SPHMI_TEST_VZ"])
    slab, _ = R.rank_setup(sc, CUTS2, 0)
    o = scenes.oracle_for(sc, threads=4)
    pos = sc["position"]
    for step in range(DRIFT_STEPS):
        m = liquid_walking_into_cell_minus_one(pos, cfg) & R.in_layers(pos, cfg, slab, R.SEARCH_DEPTH)
        assert m.sum() >= 1, "step %d: no liquid at the wrap in rank 0's range" % step
        o.step()
        new = o.buffer("position").reshape(-1, 4)[:n].copy()
        assert np.isfinite(new).all()
        assert np.abs(new[:, 2] - pos[:, 2]).max() < 0.5 * cfg.hashGridCellSize
        pos = new
    o.close()
    results = run_ranks("oracle", 2, tmp_path, steps=DRIFT_STEPS, env=DRIFT_DOWN)
    ref_sc, pos_ref, vel_ref = single_domain_reference(steps=DRIFT_STEPS, env=DRIFT_DOWN)
    assert ref_sc["cfg"].particleCount == n and list(results[0]["cuts"]) == CUTS2
    check_union(results, ref_sc, pos_ref, vel_ref)
    counts = results[0]["counts"]
    assert (np.diff(counts) > 0).sum() >= 2, counts


FRAME_RECORDS = 2304


def test_agreed_length_beyond_the_senders_frame_cpu(tmp_path):
    """Asynchronous exchange with backend frames of 2,304 records: every message (about 2,100 records) fits its frame, but the length
    both ends agree on for the next step (message x 1.125 + 1,024 records) does not. The sender must still post that length — the
    receiver posts it without knowing the sender's frame — or the transfer never completes (120 s limit). Union == single domain."""
    steps = 4
    env = {"SPHMI_TEST_ASYNC": "1", "SPHMI_TEST_FRAME_RECORDS": str(FRAME_RECORDS)}
    results = run_ranks("oracle", 2, tmp_path, steps=steps, env=env, timeout=120)
    sc, pos_ref, vel_ref = single_domain_reference(steps=steps)
    check_union(results, sc, pos_ref, vel_ref)
    assert all(bool(r["asynchronous"]) for r in results)
    for r, link in zip(results, (1, 0)):  # rank 0 sends up, rank 1 down
        rec = r["message_words"][:, link] // int(r["record_words"])
        assert rec.size == steps and np.all(rec > 0) and np.all(rec <= FRAME_RECORDS)
        assert np.all(rec + rec // 8 + 1024 > FRAME_RECORDS), rec
        assert np.all(np.array([S.SlabDecomposition.next_bound(int(w), int(r["record_words"])) for w in r["message_words"][:, link]])
                      > FRAME_RECORDS * int(r["record_words"]))
    assert all(int(r["transfers"]) == steps + 1 for r in results)  # one framed transfer per step after the first exchange
    # the rule itself: what one end sends, transfer by transfer, is what the other end posted a receive for (gloo completes a
    # short send into a longer receive without complaint; RCCL does not)
    for a, b in ((0, 1), (1, 0)):
        sent = [w for kind, peer, w in results[a]["posted"].tolist() if kind == 0 and peer == b]
        expected = [w for kind, peer, w in results[b]["posted"].tolist() if kind == 1 and peer == a]
        assert len(sent) == steps + 1 and sent == expected, (a, b, sent, expected)
        assert max(sent) > 1 + FRAME_RECORDS * int(results[a]["record_words"])  # longer than the sender's own frame
