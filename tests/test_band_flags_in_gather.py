"""The first stage of the search bands — flag bytes, per-wave ballots and counts — is written by the gather kernel of the fused
step (csrc/sph_sort.hip with sph_band_flags.h), not by a kernel of its own. What the device holds afterwards (searchBandFlags,
searchBands, searchBandStart) must equal the numpy restatement band_ref.py on the device's own sorted state, and the rows the oracle's.

Which gather a scene takes is decided by sphk_step_sort_bits: the compact-key gather (k_sort_post_rekey) where the cell ids are
wide AND the compacted keys take fewer radix passes than the declared grid's, the plain-key gather (k_sort_post) otherwise. The
test knows it from step_sort_passes(), the passes the step's sort takes, set against the passes of the declared key width:
  wide `tiny` box, 9 x 9 x 9 = 729 cells: 10 bits, 2 passes declared; 5 x 5 x 5 reachable cells, 7 bits, 1 pass -> compact-key gather;
  16-bit `tiny` box (the grid fits the mask, so bands apply): 16-bit ids never compact -> plain-key gather;
  counted boxes, wide, 41^3 cells: 17 bits, 2 passes of 9 bits declared; 21^3 reachable, 14 bits, 2 passes -> plain-key gather."""
import numpy as np
import pytest

import band_cases
import band_ref
import scenes
from test_fn_lane_order_host import jitter_scene
from test_fn_lane_order_host import oracle_states as lane_oracle
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip
from test_search_bands import bands_built

pytestmark = pytest.mark.gpu

_counted = {}


def declared_passes(cfg):
    """Radix passes for the declared key width (sph_sort_passes: 9-bit digits only where that saves a pass)."""
    bits = 16 if cfg.cellIdMask == 0xffff else max(int(cfg.gridCellCount - 1).bit_length(), 1)
    w = 9 if (bits + 8) // 9 < (bits + 7) // 8 else 8
    return (bits + w - 1) // w


def takes_compact_gather(hip, cfg):
    return cfg.cellIdMask == 0xffffffff and hip.step_sort_passes() < declared_passes(cfg)


def assert_device_bands(hip, cfg, N, where):
    """Flags, the eight arrays (zero behind each band's total) and the start tables equal the restatement on the device's own sorted state."""
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


def _assert_rows(hip, want, N, where):
    got = canon_hip(hip, N)
    for k in band_cases.SEARCH_BUFFERS:
        assert scenes.bits_equal(got[k], want[k]), (where, k, scenes.diff_report(got[k], want[k]))


def _counted_oracle(n):
    if n not in _counted:
        _counted[n] = band_cases.oracle_search(band_cases.counted_box(n))
    return _counted[n]


def test_compact_key_gather_writes_the_flags():
    """Wide ids, 2 792 = 43 x 64 + 40 particles: k_sort_post_rekey, a partial last wave."""
    sc = jitter_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = lane_oracle("jitter")
    hip = scenes.hip_for(sc)
    assert takes_compact_gather(hip, cfg) and N % 64 != 0
    for it in range(2):
        hip.step(it)
        assert bands_built(hip)
        assert_device_bands(hip, cfg, N, "wide tiny box, step %d" % (it + 1))
        assert_same(canon_hip(hip, N), want[it], "wide tiny box, step %d" % (it + 1), FUSED_SKIP)
    hip.close()


def test_plain_key_gather_writes_the_flags():
    """16-bit ids on a grid of 729 cells, which fits the mask: k_sort_post."""
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert cfg.cellIdMask == 0xffff and cfg.gridCellCount <= 0x10000 and band_ref.grid_allows_bands(cfg)
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc)
    assert not takes_compact_gather(hip, cfg)
    hip.step(0)
    ora.step()
    assert bands_built(hip)
    assert_device_bands(hip, cfg, N, "16-bit tiny box")
    assert_same(canon_hip(hip, N), scenes.canonical(ora.buffer, N), "16-bit tiny box", FUSED_SKIP)
    hip.close()
    ora.close()


@pytest.mark.parametrize("n,capacity", [(65537, 0), (131072, 0), (65537, 65537 + 4096)])
def test_last_wave_block_without_a_wave_and_spare_capacity(n, capacity):
    """65 537: the last wave has one live lane, and its 63 others must contribute zero to the ballots. 131 072 = 2048 waves: the
    band totals (entry `waves` of the offsets) are written by a scan block that owns no wave, which reads nothing the gather wrote.
    capacity > N: the arrays' stride is not N. (Wide ids, but no pass saved: the plain-key gather.)"""
    sc = band_cases.counted_box(n, capacity)
    cfg = sc["cfg"]
    assert cfg.particleCount == n and (capacity == 0 or cfg.capacity == capacity)
    hip = scenes.hip_for(sc)
    assert not takes_compact_gather(hip, cfg)
    hip.step(0)
    assert bands_built(hip) and hip.N == n
    where = "counted box %d, capacity %d" % (n, capacity)
    assert_device_bands(hip, cfg, n, where)
    _assert_rows(hip, _counted_oracle(n), n, where)
    hip.close()


def test_gather_stops_and_resumes_writing_flags():
    """Bands, then set_search_bands(1), then bands again: the step without bands runs the gather as it was (the flags of the first
    step stay unread), the third step's flags are those of its own sorted state."""
    sc = jitter_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = lane_oracle("jitter")
    hip = scenes.hip_for(sc)
    for it, mode in enumerate((0, 1, 0)):
        hip.set_search_bands(mode)
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        if mode == 0:
            assert_device_bands(hip, cfg, N, "toggled, step %d" % (it + 1))
        assert_same(canon_hip(hip, N), want[it], "toggled, step %d" % (it + 1), FUSED_SKIP)
    hip.close()
