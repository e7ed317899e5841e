"""CPU side of tests/test_tree_edges.py: on the C oracle's state of the same scenes (tests/tree_edge_cases.py: exactly 1024 and
1025 particles, the floor's half lifted, two steps), the numpy restatements give every record the GPU test compares a non-zero
count word and non-zero terms, so that test cannot pass on an empty answer."""
import numpy as np
import pytest

import body_dyn_ref as bd
import body_ref as br
import diag_ref
import fields_ref as flr
import forces_ref as fr
import gauge_ref as gr
import scenes
import tree_edge_cases as tc
import wall_ref as wr


def test_the_regions_tile_nothing_away():
    cfg = tc.scene(1024)["cfg"]
    assert tc.regions(cfg, 1).shape == (1, 6) and tc.regions(cfg, 16).shape == (16, 6)


@pytest.mark.parametrize("n", tc.SIZES)
def test_every_compared_record_counts_something(n):
    sc = tc.scene(n)
    cfg = sc["cfg"]
    assert cfg.particleCount == n == sc["position"].shape[0] and (n + 1023) // 1024 == (1 if n == 1024 else 2)
    members = br.region_members(sc["position"], tc.floor_half(cfg))
    assert members.size > 0
    pos, vel, _ = br.set_pose(cfg, sc["position"], sc["velocity"], br.define(sc["position"], sc["velocity"], members), tc.lift(cfg))
    ora = scenes.oracle_for(dict(sc, position=pos, velocity=vel))
    for _ in range(2):
        ora.step()
    state, ids, dist = wr.oracle_state(ora, n, cfg.gridCellCount)
    gstate = gr.oracle_state(ora, n)
    ora.close()
    K, W = fr.constants(cfg), wr.constants(cfg)
    field = tc.field(n)
    for count in (1, 16):
        rg = tc.regions(cfg, count)
        rec = diag_ref.records(state, rg, tc.TYPES, cfg.rho0)
        assert (rec[:, 0] > 0).all() and rec[0, 0] == n
        rec = fr.diag_records(state, fr.Forces(state, ids, dist, K).records, rg, tc.TYPES)
        assert (rec[:, 0] > 0).all() and np.abs(rec[0, 1:49]).max() > 0
        for slot in (tc.SLOT, wr.ALL):
            wall = wr.Wall(state, ids, dist, K, W, wr.wall_set(state, slot, {tc.SLOT: members}))
            rec = wr.diag_records(state, wall.records, rg, tc.TYPES)
            assert (rec[:, 0] > 0).all() and rec[0, 1] > 0 and rec[0, 2] > 0, (slot, rec[0, :3])
        rec = flr.diag_records(state, field[state["orig"]], rg, tc.TYPES)
        assert (rec[:, 0] > 0).all() and 0 < rec[0, 5] < n
    gauges = tc.gauges(sc)
    rec = gr.records(gstate, gauges)
    for slot in gauges:
        assert rec[slot, 0] > 0 and rec[slot, 8] > 0, (slot, rec[slot])
    wall = wr.Wall(state, ids, dist, K, W, wr.wall_set(state, tc.SLOT, {tc.SLOT: members}))
    D = wr.diag_records(state, wall.records, np.array([diag_ref.EVERYTHING], np.float32), (1, 2, 3))[0]
    ref_pos = br.define(sc["position"], sc["velocity"], members)[1]
    _, _, want = bd.advance(D, tc.dynamics(cfg, ref_pos), *bd.constants(cfg))
    assert D[1] > 0 and D[2] > 0 and np.abs(want[20:23]).max() > 0 and np.isfinite(want[4:28]).all()
