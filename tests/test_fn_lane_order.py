"""The lane pair of findNeighbors on the GPU (csrc/sph_neighbors.hip): lane A walks the cells 0 4 5 7 of the reference's order,
lane B the cells 1 2 3 6, and the rows come out in the reference's slot order A0 | B1 B2 B3 | A4 A5 | B6 | A7. On the scene that
test_fn_lane_order_host.py proves to exercise every piece start and the cut at 32 in every segment, and on the headline's lattice,
every canonical buffer — the neighbour ids and distances slot by slot among them — equals the oracle's bit for bit after steps
1-3, with the search bands on and off, serial, in chunks, and under stage timing; the exact-walk counters are the same with bands
on and off, so the rows came from the lane pair and not from the wave-per-particle walk."""
import numpy as np
import pytest

import scenes
from test_fn_lane_order_host import SCENE, STEPS, oracle_states
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip
from test_search_bands import bands_built

pytestmark = pytest.mark.gpu

# (bands mode, chunks, pipeline depth, stage timing)
CONFIG = {"bands": (0, 0, -1, False), "no_bands": (1, 0, -1, False), "serial": (0, 1, -1, False), "two_chunks": (0, 2, 1, False),
          "two_chunks_no_bands": (1, 2, 1, False), "stage_timing": (0, 0, -1, True)}
_counters = {}


@pytest.mark.parametrize("config", list(CONFIG))
@pytest.mark.parametrize("name", list(SCENE))
def test_rows_and_buffers_equal_the_oracle(name, config):
    mode, chunks, depth, timing = CONFIG[config]
    sc = SCENE[name]()
    N = sc["cfg"].particleCount
    want = oracle_states(name)
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    hip.set_stage_timing(timing)
    hip.reset_stage_times()
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        where = "%s, %s, step %d" % (name, config, it + 1)
        got = canon_hip(hip, N)
        ids, dist = got["neighborIds"].reshape(-1, 32), got["neighborDist"].reshape(-1, 32)
        wids, wdist = want[it]["neighborIds"].reshape(-1, 32), want[it]["neighborDist"].reshape(-1, 32)
        bad = np.argwhere(ids != wids)
        assert bad.size == 0, "%s: neighbour ids differ at (particle, slot) %s" % (where, bad[:6].tolist())
        bad = np.argwhere(dist.view(np.uint32) != wdist.view(np.uint32))
        assert bad.size == 0, "%s: neighbour distances differ at (particle, slot) %s" % (where, bad[:6].tolist())
        assert_same(got, want[it], where, FUSED_SKIP)
    c = hip.buffer("debugCounters")[:4].astype(np.int64)
    print("%s, %s: debugCounters[0..3] %s of %d particles x %d steps" % (name, config, c.tolist(), N, STEPS))
    _counters[name, config] = c
    hip.close()


@pytest.mark.parametrize("name", list(SCENE))
def test_exact_walk_counters_do_not_depend_on_the_bands(name):
    """(behind the cases above, whose counters it reads; run alone it steps the two configurations itself)"""
    for config in ("bands", "no_bands"):
        if (name, config) not in _counters:
            test_rows_and_buffers_equal_the_oracle(name, config)
    on, off = _counters[name, "bands"], _counters[name, "no_bands"]
    assert np.array_equal(on, off), (on.tolist(), off.tolist())
    N = SCENE[name]()["cfg"].particleCount
    assert on[0] + on[1] < N * STEPS // 2, "most rows came from the exact walk: %s" % on.tolist()
