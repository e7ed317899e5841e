"""The 256-particle tiles of findNeighbors' band instance on the GPU (csrc/sph_neighbors.hip): on the scenes that
test_fn_tile_host.py proves to hold tile ends of every kind, the lane-order rows in both halves of a tile, every rung of the batch
ladder, a batch wider than the cell-table window and exact walks that start from second halves, every canonical buffer — neighbour
ids and distances slot by slot among them — equals the oracle's bit for bit after steps 1-3, with the search bands on (256-particle
tiles) and off (128), serially and in 2 chunks at pipeline depth 1."""
import numpy as np
import pytest

import band_cases
import scenes
from test_fn_tile_host import COUNTED, SCENE, STEPS, oracle_states
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip
from test_search_bands import bands_built

pytestmark = pytest.mark.gpu

# (bands mode, chunks, pipeline depth)
CONFIG = {"bands": (0, 1, -1), "no_bands": (1, 1, -1), "bands_two_chunks": (0, 2, 1), "no_bands_two_chunks": (1, 2, 1)}
NAMES = ["counted%d" % n for n in COUNTED] + ["roomy", "jitter", "squeezed", "packed", "dense", "tight", "sparse", "stray"]
_counters = {}


def _rows_equal(got, want, where):
    ids, dist = got["neighborIds"].reshape(-1, 32), got["neighborDist"].reshape(-1, 32)
    wids, wdist = want["neighborIds"].reshape(-1, 32), want["neighborDist"].reshape(-1, 32)
    bad = np.argwhere(ids != wids)
    assert bad.size == 0, "%s: neighbour ids differ at (particle, slot) %s" % (where, bad[:6].tolist())
    bad = np.argwhere(dist.view(np.uint32) != wdist.view(np.uint32))
    assert bad.size == 0, "%s: neighbour distances differ at (particle, slot) %s" % (where, bad[:6].tolist())


def _run(name, config):
    mode, chunks, depth = CONFIG[config]
    sc = SCENE[name]()
    N = sc["cfg"].particleCount
    want = oracle_states(name)
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    hip.reset_stage_times()
    first = None
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        where = "%s, %s, step %d" % (name, config, it + 1)
        got = canon_hip(hip, N)
        _rows_equal(got, want[it], where)
        assert_same(got, want[it], where, FUSED_SKIP)
        if it == 0:
            first = hip.buffer("debugCounters")[:4].astype(np.int64)
    c = hip.buffer("debugCounters")[:4].astype(np.int64)
    print("%s, %s: debugCounters[0..3] %s after step 1, %s after %d steps" % (name, config, first.tolist(), c.tolist(), STEPS))
    _counters[name, config] = (first, c)
    hip.close()
    return first, c


@pytest.mark.parametrize("config", list(CONFIG))
@pytest.mark.parametrize("name", NAMES)
def test_rows_and_buffers_equal_the_oracle(name, config):
    first, c = _run(name, config)
    sc = SCENE[name]()
    if name == "stray" and CONFIG[config][0] == 0:  # the 34 moved particles fail the premise, in step 1 only (step 2 starts from the clamped positions)
        assert sc["moved"].size == 34 and first[0] == 34, first.tolist()
    if name in ("dense", "packed"):
        crowded = scenes.crowded_particles(oracle_states(name)[0], sc["cfg"].h).size
        assert crowded > 1000 and first[0] + first[1] >= crowded
    if name == "packed" and CONFIG[config][0] == 0:
        assert c[3] > 0, "the last rung of the ladder (dropped runs) was expected to be taken"
    if name in ("jitter", "roomy") or name.startswith("counted"):
        assert c[3] == 0 and c[0] + c[1] < sc["cfg"].particleCount * STEPS // 2, "most rows came from the exact walk: %s" % c.tolist()


@pytest.mark.parametrize("name", ["jitter", "counted%d" % COUNTED[2]])
def test_exact_walk_counters_do_not_depend_on_the_tile(name):
    """debugCounters[0..3] with bands (256-particle tiles) and without (128) are the same, as test_fn_lane_order.py asserts for its
    scenes: the rows came from the lane pair in both. (Behind the cases above, whose counters it reads; run alone it steps the two
    configurations itself.)"""
    for config in ("bands", "no_bands"):
        if (name, config) not in _counters:
            _run(name, config)
    on, off = _counters[name, "bands"], _counters[name, "no_bands"]
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[0], off[0]), (on, off)


def test_coincident_particles_in_both_halves():
    """Particles at identical positions: each other's first-bin neighbours at distance 0 (compared up to the density: beyond it
    the reference divides by r = 0), with the bands on and off."""
    sc = SCENE["coincident"]()
    N = sc["cfg"].particleCount
    want = oracle_states("coincident")[0]
    for mode in (0, 1):
        hip = scenes.hip_for(sc)
        hip.set_search_bands(mode)
        hip.step(0)
        assert bands_built(hip) == (mode == 0)
        got = canon_hip(hip, N)
        _rows_equal(got, want, "coincident, bands mode %d" % mode)
        for k in band_cases.SEARCH_BUFFERS:
            assert scenes.bits_equal(got[k], want[k]), (mode, k, scenes.diff_report(got[k], want[k]))
        assert scenes.bits_equal(got["rho"][:N], want["rho"][:N])
        hip.close()
