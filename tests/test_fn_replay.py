"""The replay behind findNeighbors' walk on the GPU (csrc/sph_neighbors.hip): sign-bit counting in the bisection and
in pass 1, ranks by popcount in the store walk. On the scenes that
test_fn_replay_host.py proves to hold lists of every length class, every kind of stop, accepted entries at list positions 32 and
above and coincident pairs in both halves of a tile: every canonical buffer — neighbour ids and distances slot by slot among them —
equals the oracle's bit for bit, bands on and off, serially and in two chunks; debugCounters[0..3] are what the kernel counted
before the replay was rewritten; rows without a 16-bit copy, of the exact walk and of the lane pair's second walk, equal the oracle.
(The short square root the issue behind this file also proposed did not pay and is not in the kernel, DESIGN.md 48: there is no
counter of its redone groups to assert on.)"""
import numpy as np
import pytest

import band_cases
import scenes
import test_elastic_edges_host as H
from test_fn_replay_host import NAMES, NO_COPY_SCENE, SCENE, oracle_states
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora
from test_search_bands import bands_built

pytestmark = pytest.mark.gpu

STEPS = 2
# (bands mode, chunks, pipeline depth)
CONFIG = {"bands": (0, 1, -1), "no_bands": (1, 1, -1), "bands_two_chunks": (0, 2, 1), "no_bands_two_chunks": (1, 2, 1)}
# debugCounters[0..3] after step 1 and after step 2, counted by the kernel as it was before this rewrite (the same for one and two
# chunks: the counters do not depend on the launch)
BEFORE = {
    ("dense", "bands"): [[0, 5832, 0, 0], [0, 10872, 0, 0]],
    ("dense", "no_bands"): [[3551, 2355, 0, 438], [5742, 5232, 0, 708]],
    ("tight", "bands"): [[632, 0, 0, 0], [1264, 0, 0, 0]],
    ("tight", "no_bands"): [[632, 0, 0, 0], [1264, 0, 0, 0]],
    ("sparse", "bands"): [[0, 0, 0, 0], [0, 0, 0, 0]],
    ("sparse", "no_bands"): [[0, 0, 0, 0], [0, 0, 0, 0]],
    ("squeezed", "bands"): [[0, 5067, 0, 0], [0, 8935, 0, 0]],
    ("squeezed", "no_bands"): [[878, 4207, 0, 113], [1901, 7080, 0, 240]],
    ("packed", "bands"): [[686, 6523, 0, 89], [1513, 12162, 0, 206]],
    ("packed", "no_bands"): [[2826, 4431, 0, 376], [5917, 7877, 0, 798]],
    ("coincident", "bands"): [[0, 0, 0, 0]],
    ("coincident", "no_bands"): [[0, 0, 0, 0]],
    ("stray", "bands"): [[34, 0, 0, 0], [34, 0, 0, 0]],
    ("stray", "no_bands"): [[0, 0, 0, 0], [0, 0, 0, 0]],
    ("jitter", "bands"): [[0, 29, 0, 0], [0, 51, 0, 0]],
    ("jitter", "no_bands"): [[0, 29, 0, 0], [0, 51, 0, 0]],
    ("lattice", "bands"): [[0, 0, 0, 0], [0, 0, 0, 0]],
    ("lattice", "no_bands"): [[0, 0, 0, 0], [0, 0, 0, 0]],
}


def _rows_equal(got, want, where):
    for k in ("neighborIds", "neighborDist"):
        g, w = got[k].reshape(-1, 32).view(np.uint32), want[k].reshape(-1, 32).view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: %s differs at (particle, slot) %s" % (where, k, bad[:6].tolist())


@pytest.mark.parametrize("config", list(CONFIG))
@pytest.mark.parametrize("name", [n for n in NAMES if n != "coincident"])
def test_rows_buffers_and_counters(name, config):
    mode, chunks, depth = CONFIG[config]
    sc = SCENE[name]()
    N = sc["cfg"].particleCount
    want = oracle_states(name)
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    hip.reset_stage_times()
    seen = []
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        where = "%s, %s, step %d" % (name, config, it + 1)
        got = canon_hip(hip, N)
        _rows_equal(got, want[it], where)
        assert_same(got, want[it], where, FUSED_SKIP)
        seen.append(hip.buffer("debugCounters").astype(np.int64))
    hip.close()
    print("%s, %s: debugCounters[0..3] %s after step 1, %s after step 2" % (name, config, seen[0][:4].tolist(), seen[1][:4].tolist()))
    assert [seen[0][:4].tolist(), seen[1][:4].tolist()] == BEFORE[name, "bands" if mode == 0 else "no_bands"]


@pytest.mark.parametrize("config", list(CONFIG))
def test_coincident_particles(config):
    """Particles at identical positions, in both halves of a tile: each other's first-bin neighbours at distance 0, equal d^2 on both
    sides of every threshold (compared up to the density: beyond it the reference divides by r = 0)."""
    mode, chunks, depth = CONFIG[config]
    sc = SCENE["coincident"]()
    N = sc["cfg"].particleCount
    want = oracle_states("coincident")[0]
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(depth)
    hip.reset_stage_times()
    hip.step(0)
    assert bands_built(hip) == (mode == 0)
    got = canon_hip(hip, N)
    _rows_equal(got, want, "coincident, %s" % config)
    for k in band_cases.SEARCH_BUFFERS:
        assert scenes.bits_equal(got[k], want[k]), (config, k, scenes.diff_report(got[k], want[k]))
    assert scenes.bits_equal(got["rho"][:N], want["rho"][:N])
    c = hip.buffer("debugCounters").astype(np.int64)
    hip.close()
    zero = int((want["neighborDist"].reshape(-1, 32)[:N] == 0.0).any(1).sum())
    print("coincident, %s: %d rows hold a distance of 0, debugCounters[0..3] = %s" % (config, zero, c[:4].tolist()))
    assert zero >= 10
    assert c[:4].tolist() == BEFORE["coincident", "bands" if mode == 0 else "no_bands"][0]


def test_rows_of_the_exact_walk_without_a_16_bit_copy():
    """~700 particles per cell: the lists overflow, the exact walk serves the particles and their rows have no 16-bit copy."""
    kw = dict(NO_COPY_SCENE)
    sc = scenes.liquid_box(kw.pop("box"), kw.pop("lattice"), **kw)
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc, threads=8)
    hip.reset_stage_times()
    hip.step(0)
    ora.step()
    got, want = canon_hip(hip, N), canon_ora(ora, N)
    ora.close()
    c = hip.buffer("debugCounters").astype(np.int64)
    hip.close()
    _rows_equal(got, want, "overcrowded cells")
    assert_same(got, want, "overcrowded cells", FUSED_SKIP)
    crowded = scenes.crowded_particles(got, sc["cfg"].h)
    assert c[1] > 0 and c[0] + c[1] >= crowded.size > 200, (c[:4].tolist(), crowded.size)


@pytest.mark.parametrize("mode", [0, 1])
def test_rows_of_the_lane_pair_without_a_16_bit_copy(mode):
    """The bar of scenes.elastic_hard_box: rows of the fast path whose offsets do not fit 16 bits — the store walk's second pass
    writes their 32-bit ids."""
    sc, canon, wide, _ = H.bar_state()
    N = sc["cfg"].particleCount
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.reset_stage_times()
    hip.step(0)
    got = canon_hip(hip, N)
    c = hip.buffer("debugCounters").astype(np.int64)
    hip.close()
    _rows_equal(got, canon, "bar, bands mode %d" % mode)
    assert_same(got, canon, "bar, bands mode %d" % mode, FUSED_SKIP)
    assert int(c[2]) >= len(wide) - int(c[0]) >= 150, c[:4].tolist()
