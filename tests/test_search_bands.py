"""The search bands of the fused step on the GPU (csrc/sph_bands.hip, the BANDS instance of k_find_neighbors): the
device's flags, band arrays and start tables equal the numpy restatement (band_ref.py), and every canonical buffer equals the
oracle's bit for bit with the bands on and off — serial and in chunks, with exact walks, wrapped and clamped runs, a partial last
tile, elastic matter with muscles, an edit between steps, the switches toggled between steps. Where the superset proof does not
hold the automatic mode must run without bands."""
import numpy as np
import pytest

import band_ref
import edit_ref
import scenes
from test_fn_staging import SCENE as FN_SCENE, STEPS, oracle_states
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

pytestmark = pytest.mark.gpu

_extra = {}


def _scene(name):
    if name in FN_SCENE:
        return FN_SCENE[name]()
    if name == "compressed":  # the column at 0.85 r0
        return scenes.SCENES["tiny_compressed"]()
    if name == "worm":
        return scenes.worm_scene()
    if name == "sheet":  # elastic sheet with muscles and membranes in a box whose grid allows bands
        return scenes.SCENES["tiny_elastic"]()
    raise KeyError(name)


def _oracle(name):
    """Canonical oracle buffers after each of STEPS steps: test_fn_staging's where it has the scene, else computed once here."""
    if name in FN_SCENE:
        return oracle_states(name)
    if name not in _extra:
        sc = _scene(name)
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for it in range(STEPS):
            if sc["cfg"].muscleCount:
                ora.update_muscles(scenes.hard_muscle_signal(it)[:sc["cfg"].muscleCount])
            ora.step()
            out.append(canon_ora(ora, N))
        ora.close()
        _extra[name] = out
    return _extra[name]


def bands_built(hip):
    """Whether the last step built (and its search read) the bands."""
    try:
        hip.buffer("searchBandFlags")
        return True
    except Exception as e:  # SPH_ERR_ORDER: "the last step built no search bands"
        assert "no search bands" in str(e), e
        return False


def _device_bands(hip, N, G):
    flags = hip.buffer("searchBandFlags")
    recs = hip.buffer("searchBands").reshape(8, N, 4)
    start = hip.buffer("searchBandStart").reshape(8, G + 1)
    return flags, recs, start


@pytest.mark.parametrize("name", ["tiny", "tiny_long", "dense", "sparse", "tight", "compressed"])
def test_device_bands_equal_the_restatement(name):
    sc = _scene(name)
    cfg = sc["cfg"]
    N, G = cfg.particleCount, cfg.gridCellCount
    assert band_ref.grid_allows_bands(cfg)
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert bands_built(hip)
    pos = hip.buffer("sortedPosition").reshape(-1, 4)[:N]
    keys = hip.buffer("particleIndex").reshape(-1, 2)[:, 0]
    cell_start = hip.buffer("gridCellIndexFixedUp")
    flags, recs, start = _device_bands(hip, N, G)
    want = band_ref.band_flags(pos, keys, cfg)
    assert np.array_equal(flags, want), np.nonzero(flags != want)[0][:8]
    assert np.array_equal(start, band_ref.band_start(want, cell_start))
    per = []
    for s, w in enumerate(band_ref.band_arrays(pos, want)):
        assert int(start[s, G]) == w.shape[0]
        assert scenes.bits_equal(recs[s, :w.shape[0]], w), "band %d" % s
        assert not recs[s, w.shape[0]:].any()
        per.append(w.shape[0] / N)
    print("%s: Rb %.9g (filter radius %.9g), band entries per particle %s"
          % (name, band_ref.band_radius(cfg), np.sqrt(np.float64(band_ref.filter_r2(cfg.h))), ["%.3f" % p for p in per]))
    hip.close()


CASES = [(n, 1) for n in ("tiny", "tiny_long", "dense", "sparse", "tight", "compressed")] + \
        [("tiny_long", 2), ("tiny_long", 16), ("dense", 2), ("tight", 2)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,chunks", CASES)
def test_rows_and_buffers_equal_the_oracle(name, chunks, mode):
    """dense: overcrowded cells, every list overflows (exact walks, which read band rows from global memory), runs dropped;
    tight: wrapped and clamped runs; sparse: a last tile shorter than 128; chunks at pipeline depth 1."""
    sc = _scene(name)
    N = sc["cfg"].particleCount
    want = _oracle(name)
    hip = scenes.hip_for(sc)
    hip.set_search_bands(mode)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(1 if chunks > 1 else -1)
    hip.reset_stage_times()
    for it in range(STEPS):
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        assert_same(canon_hip(hip, N), want[it], "%s, %d chunks, bands mode %d, step %d" % (name, chunks, mode, it), FUSED_SKIP)
    c = hip.buffer("debugCounters")[:4].astype(np.int64)
    print("%s, %d chunks, mode %d: debugCounters[0..3] %s" % (name, chunks, mode, c.tolist()))
    if name == "dense":
        assert c[1] > 1000  # the list-overflow walks were exercised
    hip.close()


@pytest.mark.parametrize("name", ["worm", "sheet"])
def test_elastic_matter_with_muscles(name):
    """The worm (its 16-bit ids alias: the step must run without bands) and an elastic sheet in a grid that allows them."""
    sc = _scene(name)
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = _oracle(name)
    assert band_ref.grid_allows_bands(cfg) == (name == "sheet")
    hip = scenes.hip_for(sc)
    for it in range(STEPS):
        if cfg.muscleCount:
            hip.updateMuscleActivityData(scenes.hard_muscle_signal(it)[:cfg.muscleCount])
        hip.step(it)
        assert bands_built(hip) == (name == "sheet")
        assert_same(canon_hip(hip, N), want[it], "%s, step %d" % (name, it), FUSED_SKIP)
    hip.close()


def test_coincident_particles():
    """Particles at identical positions: each other's first-bin neighbours at distance 0 (compared up to the density: beyond it
    the reference divides by r = 0)."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), jitter_in_r0=0.03)
    pos = sc["position"].copy()
    pos[5:10, :3] = pos[200:205, :3]
    sc["position"] = pos
    N = sc["cfg"].particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc)
    hip.step(0)
    assert bands_built(hip)
    for st in scenes.STAGE_SEQUENCE[:scenes.STAGE_SEQUENCE.index("computeDensity") + 1]:
        ora.run(st)
    got, want = canon_hip(hip, N), canon_ora(ora, N)
    for k in ("particleIndex", "gridCellIndexFixedUp", "neighborIds", "neighborDist"):
        assert scenes.bits_equal(got[k], want[k]), (k, scenes.diff_report(got[k], want[k]))
    assert (want["neighborDist"].reshape(-1, 32) == 0.0).sum() >= 10
    hip.close()
    ora.close()


def test_switches_toggled_between_steps():
    """The mode and the stage timing change between steps: every step equals the oracle's, the band stage is timed exactly when
    bands were built under timing."""
    sc = _scene("tiny_long")
    N = sc["cfg"].particleCount
    want = _oracle("tiny_long")
    hip = scenes.hip_for(sc)
    hip.reset_stage_times()
    plan = [(0, True), (1, False), (0, False)]  # (bands mode, stage timing)
    for it, (mode, timing) in enumerate(plan):
        hip.set_search_bands(mode)
        hip.set_stage_timing(timing)
        hip.step(it)
        assert bands_built(hip) == (mode == 0)
        assert_same(canon_hip(hip, N), want[it], "toggled, step %d" % it, FUSED_SKIP)
    st = hip.stage_times()
    assert st["bands"][1] == 1 and st["bands"][0] > 0.0, st["bands"]
    assert st["find_neighbors"][1] == 1
    hip.close()


def test_edit_between_steps():
    """A removal and an emission between steps change N; the bands of the next step are built for the new set."""
    sc = _scene("tiny")
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    hip.step(0)
    removed = hip.remove_region((0.0, 0.0, 0.0, cfg.xmax, cfg.ymax, 0.5 * (cfg.zmin + cfg.zmax)), (1,))
    assert removed > 60
    r0 = cfg.r0
    added = hip.emit_lattice((0.4 * cfg.xmax, 0.4 * cfg.ymax, 0.3 * cfg.zmax), (r0, r0, r0), (5, 4, 3))
    assert added == 60
    pos, vel = hip.read_position_buffer().copy(), hip.read_velocity_buffer().copy()
    N = pos.shape[0]
    assert N == hip.N == cfg.particleCount - removed + added
    state = dict(sc, position=pos, velocity=vel, cfg=edit_ref.with_count(cfg, N))
    ora = scenes.oracle_for(state)
    hip.step(1)
    ora.step()
    assert bands_built(hip)
    assert_same(canon_hip(hip, N), canon_ora(ora, N), "after the edit", FUSED_SKIP)
    flags = hip.buffer("searchBandFlags")
    keys = hip.buffer("particleIndex").reshape(-1, 2)[:, 0]
    assert np.array_equal(flags, band_ref.band_flags(hip.buffer("sortedPosition").reshape(-1, 4)[:N], keys, state["cfg"]))
    hip.close()
    ora.close()


def test_close_behind_a_step():
    sc = _scene("tiny")
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.close()  # (the band build and the search may still be running)
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert bands_built(hip)
    hip.close()


def test_automatic_mode_runs_without_bands_where_the_proof_fails():
    """alias16: 150 000 declared cells under 16-bit ids — keys are not cell ids. The step must choose full lists, and equal the oracle."""
    sc = scenes.SCENES["alias16"]()
    cfg = sc["cfg"]
    assert not band_ref.grid_allows_bands(cfg)
    N = cfg.particleCount
    hip, ora = scenes.hip_for(sc), scenes.oracle_for(sc)
    hip.step(0)
    ora.step()
    assert not bands_built(hip)
    assert_same(canon_hip(hip, N), canon_ora(ora, N), "alias16", FUSED_SKIP)
    hip.close()
    ora.close()
