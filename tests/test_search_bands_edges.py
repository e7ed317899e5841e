"""The search bands on the GPU at the states where they can break (scenes: band_cases.py; what each scene holds is proven on
the CPU by test_search_bands_edges_host.py). Pairs across every y / z face and yz edge at the last separation the
reference accepts and ulps around it, lone candidates at the band radius to the ulp; particles outside the box, whose keys are not
their cells, with the bands on; particle counts at the block edges of the band scan, also with capacity above N; grids of three
cells along an axis, and of two, where the bands must stay off. Everywhere the device's flags, band arrays and start tables equal
the numpy restatement (band_ref.py), and the buffers equal the oracle's bit for bit, bands on and off."""
import numpy as np
import pytest

import band_cases
import band_ref
import scenes
from test_fn_staging import STEPS
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip
from test_search_bands import bands_built

pytestmark = pytest.mark.gpu


def assert_device_bands(hip, cfg, N, where):
    """Flags, the eight arrays, zeros behind each band's total and the start tables of the last step equal the restatement on the
    device's own sorted state. Returns the flags."""
    G = cfg.gridCellCount
    pos = hip.buffer("sortedPosition").reshape(-1, 4)[:N]
    keys = hip.buffer("particleIndex").reshape(-1, 2)[:, 0]
    cell_start = hip.buffer("gridCellIndexFixedUp")
    flags = hip.buffer("searchBandFlags")
    recs = hip.buffer("searchBands").reshape(8, N, 4)
    start = hip.buffer("searchBandStart").reshape(8, G + 1)
    want = band_ref.band_flags(pos, keys, cfg)
    assert flags.shape == want.shape
    assert np.array_equal(flags, want), "%s: flags differ at %s" % (where, np.nonzero(flags != want)[0][:8])
    want_start = band_ref.band_start(want, cell_start)
    assert np.array_equal(start, want_start), "%s: start tables differ at (band, cell) %s" % (where, np.argwhere(start != want_start)[:4])
    for s, w in enumerate(band_ref.band_arrays(pos, want)):
        assert int(start[s, G]) == w.shape[0], "%s: total of band %d" % (where, s)
        assert scenes.bits_equal(recs[s, :w.shape[0]], w), "%s: band %d" % (where, s)
        assert not recs[s, w.shape[0]:].any(), "%s: band %d is not zero behind its total" % (where, s)
    return flags


@pytest.mark.parametrize("mode", [0, 1])
def test_pairs_across_faces_and_edges(mode):
    """One fused step on the face scene: with a face distance that differed from the restatement's by one rounding the flags of the
    lone candidates would differ, with a band radius too small by 64 ulps a neighbour of every kind would be lost."""
    sc = band_cases.face_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = band_cases.oracle_states("face", 1)[0]
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.step(0)
    assert bands_built(hip) == (mode == 0)
    if mode == 0:
        flags = assert_device_bands(hip, cfg, N, "face scene")
        back = hip.buffer("particleIndexBack").astype(np.int64)
        for i, axis, side, what, bit, member, dist in sc["lone"]:
            if bit is not None:
                assert ((int(flags[back[i]]) >> bit) & 1) == int(member), (axis, side, what)
    assert_same(canon_hip(hip, N), want, "face scene, bands mode %d" % mode, FUSED_SKIP)
    hip.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_particles_outside_the_box(mode):
    """Keys that are not the cells the coordinates truncate to: such a candidate is in every band, such a visiting particle takes
    the exact walk. Step 2 starts from the clamped positions."""
    sc = band_cases.stray_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = band_cases.oracle_states("stray", 2)
    moved = sc["moved"]
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    for it in range(2):
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        if mode == 0:
            flags = assert_device_bands(hip, cfg, N, "stray scene, step %d" % it)
            orig = hip.buffer("particleIndex").reshape(-1, 2)[:, 1].astype(np.int64)
            every = sorted(orig[flags == 0xff].tolist())
            assert every == (moved.tolist() if it == 0 else []), every
            if it == 0:
                c = hip.buffer("debugCounters")[:4].astype(np.int64)
                print("stray scene: %d moved particles, debugCounters[0..3] %s" % (moved.size, c.tolist()))
                assert c[0] + c[1] >= moved.size, "fewer exact walks than particles that fail the premise"
        assert_same(canon_hip(hip, N), want[it], "stray scene, bands mode %d, step %d" % (mode, it), FUSED_SKIP)
    hip.close()


_counted = {}


def _counted_oracle(n, full_step=False):
    if (n, full_step) not in _counted:
        _counted[n, full_step] = band_cases.oracle_search(band_cases.counted_box(n), full_step)
    return _counted[n, full_step]


def _assert_rows_and_density(hip, want, N, where):
    got = canon_hip(hip, N)
    for k in band_cases.SEARCH_BUFFERS:
        assert scenes.bits_equal(got[k], want[k]), (where, k, scenes.diff_report(got[k], want[k]))
    assert scenes.bits_equal(got["rho"][:N], want["rho"][:N]), (where, "rho", scenes.diff_report(got["rho"][:N], want["rho"][:N]))


@pytest.mark.parametrize("n", band_cases.COUNTS)
def test_scan_across_blocks(n):
    """More than one block of 1024 waves in k_band_super / k_band_offsets: sums of the blocks in front, a band's total written by a
    block that owns no wave (n = 65 536, 131 072), a last wave with one live lane, a partial third block."""
    sc = band_cases.counted_box(n)
    cfg = sc["cfg"]
    assert cfg.particleCount == n
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert bands_built(hip)
    assert_device_bands(hip, cfg, n, "counted box %d" % n)
    _assert_rows_and_density(hip, _counted_oracle(n), n, "counted box %d" % n)
    hip.close()


def test_scan_across_blocks_in_chunks():
    n = 131073
    sc = band_cases.counted_box(n)
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(2)
    hip.set_step_pipeline(1)
    hip.step(0)
    assert bands_built(hip)
    assert_same(canon_hip(hip, n), _counted_oracle(n, True), "counted box %d, 2 chunks" % n, FUSED_SKIP)
    hip.close()


def test_capacity_above_the_particle_count():
    """bandCap is the stride of the eight arrays: with room for 4096 more particles it is not N."""
    n = 65537
    sc = band_cases.counted_box(n, n + 4096)
    cfg = sc["cfg"]
    assert cfg.capacity == n + 4096 and cfg.particleCount == n
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert bands_built(hip) and hip.N == n
    assert_device_bands(hip, cfg, n, "counted box %d with capacity %d" % (n, cfg.capacity))
    _assert_rows_and_density(hip, _counted_oracle(n), n, "counted box %d with capacity %d" % (n, cfg.capacity))
    hip.close()


@pytest.mark.parametrize("name", band_cases.GRID_NAMES)
def test_cut_grids(name):
    """Three cells along an axis: the smallest grid the proof admits, where the row offsets alias real cells — bands are built and
    change nothing. Two cells along an axis: the automatic mode must run without bands."""
    sc = band_cases.grid_scene(name)
    cfg = sc["cfg"]
    N = cfg.particleCount
    allowed = name[0] == "3"
    assert band_ref.grid_allows_bands(cfg) == allowed
    want = band_cases.oracle_states(name)
    hip = scenes.hip_for(sc)
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == allowed
        if allowed:
            assert_device_bands(hip, cfg, N, "%s, step %d" % (name, it))
        assert_same(canon_hip(hip, N), want[it], "%s, step %d" % (name, it), FUSED_SKIP)
    hip.close()
