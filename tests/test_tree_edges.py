"""GPU tests of the fixed reduction tree at the chunk edge (sph_tree.h): exactly 1024 particles -- one chunk, no upper level -- and
exactly 1025 -- two chunks, the second holding one term, one upper level over two partials. Every call that reduces in the tree
and runs on a liquid scene is compared bit for bit with its numpy restatement: diagnostics, force_diagnostics, wall_diagnostics (a
body slot and WALL_ALL), field_diagnostics, each with 1 and 16 regions, gauges_accumulate with two gauges defined out of sixteen
(the other rows of its tree stay unwritten) and bodies_advance with one dynamic body (the rows of the other slots stay unwritten,
the count row holds one word). Every compared record has a non-zero count word; tests/test_tree_edges_host.py shows that on the
C oracle's state of the same scenes."""
import numpy as np
import pytest

import body_dyn_ref as bd
import diag_ref
import fields_ref as flr
import forces_ref as fr
import gauge_ref as gr
import scenes
import tree_edge_cases as tc
import wall_ref as wr

pytestmark = pytest.mark.gpu
f32 = np.float32


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def first_diff(got, want):
    d = np.argwhere(u64(got) != u64(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(u64(got), u64(want)), "%s: %s" % (what, first_diff(got, want))


@pytest.fixture(scope="module", params=tc.SIZES)
def edge(request):
    """The solver on the scene of exactly N particles after two steps, with the restated side computed once."""
    n = request.param
    sc = tc.scene(n)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    assert hip.N == n
    members = hip.body_define_region(tc.SLOT, tc.floor_half(cfg))
    assert members > 0
    hip.body_set_pose(tc.SLOT, tc.lift(cfg))
    gauges = tc.gauges(sc)
    for slot, g in gauges.items():
        hip.gauge_define(slot, **g)
    for it in range(2):
        hip.step(it)
    state = wr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    K, W = fr.constants(cfg), wr.constants(cfg)
    body_ids, ref_pos, _ = hip.body_read(tc.SLOT)
    bodies = {tc.SLOT: body_ids.copy()}
    walls = {s: wr.Wall(state, ids, dist, K, W, wr.wall_set(state, s, bodies)) for s in (tc.SLOT, wr.ALL)}
    forces = fr.Forces(state, ids, dist, K)
    yield dict(n=n, sc=sc, cfg=cfg, hip=hip, state=state, walls=walls, forces=forces, gauges=gauges, ref_pos=ref_pos.copy())
    hip.close()


@pytest.mark.parametrize("count", [1, 16])
def test_region_records(edge, count):
    hip, cfg, state, n = edge["hip"], edge["cfg"], edge["state"], edge["n"]
    rg = tc.regions(cfg, count)
    what = "N %d, %d regions" % (n, count)
    got = hip.diagnostics(rg, tc.TYPES)
    assert_bits(got, diag_ref.records(state, rg, tc.TYPES, cfg.rho0), what + ", diagnostics")
    assert (got[:, 0] > 0).all() and got[0, 0] == n
    got = hip.force_diagnostics(rg, tc.TYPES)
    assert_bits(got, fr.diag_records(state, edge["forces"].records, rg, tc.TYPES), what + ", force_diagnostics")
    assert (got[:, 0] > 0).all() and got[0, 0] == n and np.abs(got[0, 1:49]).max() > 0
    for slot in (tc.SLOT, wr.ALL):
        got = hip.wall_diagnostics(slot, rg, tc.TYPES)
        assert_bits(got, wr.diag_records(state, edge["walls"][slot].records, rg, tc.TYPES), what + ", wall_diagnostics of set %d" % slot)
        assert (got[:, 0] > 0).all() and got[0, 0] == n and got[0, 1] > 0 and got[0, 2] > 0  # in contact, and with a share of the set
    field = tc.field(n)
    if count == 1:
        hip.field_create(tc.FIELD_SLOT, field)
    got = hip.field_diagnostics(tc.FIELD_SLOT, rg, tc.TYPES)
    assert_bits(got, flr.diag_records(state, field[state["ids"]], rg, tc.TYPES), what + ", field_diagnostics")
    assert (got[:, 0] > 0).all() and got[0, 0] == n and 0 < got[0, 5] < n


def test_gauges_then_bodies(edge):
    """gauges_accumulate first (it reads where the step left the particles), bodies_advance last (it moves the members)."""
    hip, cfg, state, n = edge["hip"], edge["cfg"], edge["state"], edge["n"]
    rec = hip.gauges_accumulate()
    want = gr.records(gr.solver_state(hip), edge["gauges"])
    assert rec.shape == want.shape and np.array_equal(gr.zero_sign_blind(rec), gr.zero_sign_blind(want)), "N %d, gauges: %s" % (n, first_diff(rec, want))
    for slot in range(16):
        if slot in edge["gauges"]:
            assert rec[slot, 0] > 0 and rec[slot, 8] > 0, (n, slot)
        else:
            assert not rec[slot].any()
    # the body: the load is the restated wall record of its slot, the step is the restated integrator
    everything = np.array([diag_ref.EVERYTHING], np.float32)
    D = wr.diag_records(state, edge["walls"][tc.SLOT].records, everything, (1, 2, 3))[0]
    all_walls = wr.diag_records(state, edge["walls"][wr.ALL].records, everything, (1, 2, 3))[0]
    dyn = tc.dynamics(cfg, edge["ref_pos"])
    hip.body_set_dynamics(tc.SLOT, **dyn)
    rec = hip.bodies_advance()
    _, _, want = bd.advance(D, dyn, *bd.constants(cfg))
    got = rec[tc.SLOT, 4:28]  # (as numbers, the compare of tests/test_body_dynamics.py: the record's zeros carry no sign contract)
    assert ((got == want[4:28]) | (np.isnan(got) & np.isnan(want[4:28]))).all(), "N %d, bodies_advance: %r vs %r" % (n, got, want[4:28])
    assert rec[tc.SLOT, 0] == 0 and rec[tc.SLOT, 27] == D[2] > 0 and rec[tc.SLOT, 26] == D[1] == all_walls[1] > 0
    assert np.abs(rec[tc.SLOT, 20:23]).max() > 0  # a load
    for slot in range(rec.shape[0]):
        assert slot == tc.SLOT or (rec[slot, 0] == -1 and not rec[slot, 1:].any())
