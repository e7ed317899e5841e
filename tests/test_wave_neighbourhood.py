"""Neighbourhood bytes in the predict-correct loop. A wave of the pressure-force kernel (K12) or of the predicted-density
kernel behind it (K10) decides at the top of the kernel, from one byte, whether any wave that could hold a neighbour of its particles
is flagged; the flagged waves store those bytes, by cells. Skipping is exact, so every case compares every canonical buffer with the
oracle bit for bit; the bytes are read back and compared with their restatement (wave_nb_ref), the decisions with what the bytes
imply, and both with the set the neighbour rows give (test_pressure_skip)."""
import numpy as np
import pytest

import scenes
import sphmi
import test_pressure_skip as tps
import wave_nb_ref as nb
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora
from test_step_pipeline import PARITY_SCENES
from test_wave_neighbourhood_host import small_oracle

pytestmark = pytest.mark.gpu
ALWAYS, GATED, OFF = 1, 0, 2


def grid(cfg):
    return cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellCount


def assert_bytes_and_decisions(hip, want, cfg, where):
    """Mode 1, after a step: both arrays of neighbourhood bytes equal their restatement; K12's decisions are those the bytes imply;
    no wave that the neighbour rows say must serve K12 in full skipped. Returns the share of waves with liquid that skipped."""
    N = cfg.particleCount
    keys, table = nb.search_tables(want)
    gx, gy, G = grid(cfg)
    liquid = nb.sorted_liquid(want)
    has_liquid, full, close, _ = tps._wave_sets(want, cfg)
    holds_p = nb.wave_any(want["pressure"][:N] != 0)
    assert np.array_equal(hip.buffer("pressureFlags") != 0, holds_p), where
    cells, closed, _ = nb.neighbourhood(keys, table, holds_p, gx, gy, G)
    assert not closed
    got = hip.buffer("pressureNeighbourhood") != 0
    assert np.array_equal(got, cells), "%s: pressure neighbourhood, %d waves differ" % (where, (got != cells).sum())
    if cfg.maxIteration >= 2:  # the waves the last K12 + predictPositions flagged: the keys of their non-boundary particles
        moved = hip.buffer("movedFlags") != 0
        assert not (moved & ~has_liquid).any()
        cells_x, closed, _ = nb.neighbourhood(keys, table, moved, gx, gy, G, active=liquid)
        got_x = hip.buffer("movedNeighbourhood") != 0
        assert not closed and np.array_equal(got_x, cells_x), "%s: moved neighbourhood, %d waves differ" % (where, (got_x != cells_x).sum())
        k10 = hip.buffer("predictDensitySkipped") != 0
        assert np.array_equal(k10, ~cells_x), where
    skipped = hip.buffer("pressureForceSkipped") != 0
    expect = np.where(has_liquid, ~(cells | nb.wave_any(close)), True)  # (a wave of boundary particles alone writes 1)
    assert np.array_equal(skipped, expect), "%s: %d decisions differ" % (where, (skipped != expect).sum())
    assert not (skipped & full).any(), "%s: a wave that must serve K12 in full skipped" % where
    return skipped[has_liquid].mean()


def test_mixed_column_always_consulting():
    sc = tps.mixed_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = tps.oracle_states("mixed", tps.MIXED_STEPS)
    hip = scenes.hip_for(sc)
    hip.set_wave_skip(ALWAYS)
    for it in range(1, 21):
        hip.step(it - 1)
        if it in tps.MIXED_STEPS:
            assert_same(canon_hip(hip, N), want[it], "mixed column, mode 1, step %d" % it, FUSED_SKIP)
            share = assert_bytes_and_decisions(hip, want[it], cfg, "step %d" % it)
            print("step %d: %.3f of the waves with liquid skipped K12" % (it, share))
            if it == 20:
                assert 0.2 <= share <= 0.8
    hip.close()


@pytest.mark.parametrize("mode", [GATED, OFF])
def test_mixed_column_other_modes(mode):
    sc = tps.mixed_scene()
    N = sc["cfg"].particleCount
    want = tps.oracle_states("mixed", tps.MIXED_STEPS)
    hip = scenes.hip_for(sc)
    hip.set_wave_skip(mode)
    before = hip.buffer("pressureForceSkipped").copy()
    for it in range(1, 21):
        hip.step(it - 1)
        if it in tps.MIXED_STEPS:
            assert_same(canon_hip(hip, N), want[it], "mixed column, mode %d, step %d" % (mode, it), FUSED_SKIP)
            if mode == GATED:
                tps.assert_k12_decisions(hip, want[it], sc["cfg"], "mode 0, step %d" % it)
    if mode == OFF:  # nothing wrote a decision
        assert np.array_equal(hip.buffer("pressureForceSkipped"), before)
    hip.close()


def test_compressed_column_nothing_skips():
    sc = tps.build("compressed")
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = tps.oracle_states("compressed", (1, 3))
    hip = scenes.hip_for(sc)
    hip.set_wave_skip(ALWAYS)
    for it in (1, 2, 3):
        hip.step(it - 1)
        if it in want:
            assert_same(canon_hip(hip, N), want[it], "0.85 r0, mode 1, step %d" % it, FUSED_SKIP)
            assert_bytes_and_decisions(hip, want[it], cfg, "0.85 r0, step %d" % it)
            has_liquid = tps.wave_sets(want[it], cfg)[0]
            assert not (hip.buffer("pressureForceSkipped")[has_liquid] != 0).any()
    hip.close()


_steps = {}


def oracle_steps(name, steps):
    """Canonical buffers after each of `steps` steps of a PARITY_SCENES / scenes.SCENES scene (CPU): once per scene, shared."""
    if name not in _steps:
        sc = (PARITY_SCENES.get(name) or scenes.SCENES[name])()
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for _ in range(steps):
            ora.step()
            out.append(canon_ora(ora, sc["cfg"].particleCount))
        ora.close()
        _steps[name] = out
    return _steps[name]


@pytest.mark.parametrize("name", ["alias16", "tiny_long"])
@pytest.mark.parametrize("chunks", [2, 16])
def test_chunked_search_depth_one(name, chunks):
    """The forces kernel marks chunk by chunk while the search still runs on the chunks behind; the marks cross chunk edges."""
    sc = (PARITY_SCENES.get(name) or scenes.SCENES[name])()
    cfg = sc["cfg"]
    want = oracle_steps(name, 3)
    hip = scenes.hip_for(sc)
    hip.set_step_chunks(chunks)
    hip.set_step_pipeline(1)
    hip.set_wave_skip(ALWAYS)
    for it in range(3):
        hip.step(it)
        assert_same(canon_hip(hip, cfg.particleCount), want[it], "%s, %d chunks, step %d" % (name, chunks, it + 1), FUSED_SKIP)
        assert_bytes_and_decisions(hip, want[it], cfg, "%s, %d chunks, step %d" % (name, chunks, it + 1))
    hip.close()


@pytest.mark.parametrize("name", ["tiny_compressed", "alias16"])
def test_waves_over_several_cells_and_boundary_only_waves(name):
    """tiny_compressed: flagged waves whose particles lie in four cells (a wave of 64 seldom holds more: a cell of the shell alone
    holds 16), so the marking walks several keys. alias16 is mostly boundary shell: waves of boundary particles alone, which K12
    leaves before its tail."""
    cfg, want = small_oracle(name)
    N = cfg.particleCount
    keys, _ = nb.search_tables(want)
    per_wave = np.array([np.unique(keys[w * 64:(w + 1) * 64]).size for w in range((N + 63) // 64)])
    if name == "tiny_compressed":
        assert per_wave[nb.wave_any(want["pressure"][:N] != 0)].max() >= 4
    else:
        assert (~nb.wave_any(nb.sorted_liquid(want))).sum() > 1000
    hip = scenes.hip_for(scenes.SCENES[name]())
    hip.set_wave_skip(ALWAYS)
    for it in range(2):
        hip.step(it)
    assert_same(canon_hip(hip, N), want, "%s, mode 1, step 2" % name, FUSED_SKIP)
    assert_bytes_and_decisions(hip, want, cfg, "%s, step 2" % name)
    hip.close()


def test_calling_rules():
    """The mode and stage timing switched between steps, the asynchronous read-back after every step, a removal and an emission
    between steps, closing right behind a step: the solver that went through all that ends where a plain one does."""
    sc = tps.mixed_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = tps.oracle_states("mixed", tps.MIXED_STEPS)[10]
    hip = scenes.hip_for(sc)
    out = np.empty((N, 4), np.float32)
    for it in range(10):
        hip.set_wave_skip((ALWAYS, GATED, OFF)[it % 3])
        hip.set_stage_timing(it % 4 == 1)
        hip.step(it)
        hip.read_position_buffer_async(out)
        hip.wait_position_buffer()
    assert_same(canon_hip(hip, N), want, "modes and stage timing switched between steps, step 10", FUSED_SKIP)
    assert scenes.bits_equal(out, want["position"])
    for bad in (-1, 3):
        with pytest.raises(sphmi.SphError):
            hip.set_wave_skip(bad)
    # a removal and an emission between steps: the particle count and the sorted order change under the per-wave arrays
    plain = scenes.hip_for(sc)
    plain.set_wave_skip(OFF)
    for it in range(10):
        plain.step(it)
    was = plain.read_position_buffer()
    is_liquid = was[:, 3].astype(np.int32) == 1
    inf = float("inf")
    box = (-inf, -inf, float(np.median(was[is_liquid, 2])), inf, inf, inf)  # the upper half of the liquid
    gone = np.flatnonzero(is_liquid & (was[:, 2] >= box[2]))[:500]
    assert gone.size == 500
    back = was[gone].copy()
    for h in (hip, plain):
        h.set_stage_timing(False)
        assert h.remove_region(box, types=(1,)) >= 500
        h.add_particles(back, np.zeros_like(back))
    assert hip.N == plain.N < N
    hip.set_wave_skip(ALWAYS)
    for it in range(10, 13):
        hip.step(it)
        plain.step(it)
    n = hip.N
    assert_same(canon_hip(hip, n), canon_hip(plain, n), "three steps behind a removal, mode 1 against mode 2", FUSED_SKIP)
    plain.close()
    hip.step(13)
    hip.close()  # right behind a step


def test_blown_up_state_closes_every_stage():
    """Coincident particles divide by r = 0 in the first step (sph_create refuses a NaN itself): the second step starts from NaN
    coordinates. It completes, its prelude closes the gate of every stage, so no wave with liquid skipped; nothing faults."""
    sc = tps.mixed_scene()
    cfg = sc["cfg"]
    pos = sc["position"].copy()
    pos[5:10, :3] = pos[200:205, :3]
    sc["position"] = pos
    hip = scenes.hip_for(sc)
    hip.set_wave_skip(ALWAYS)
    hip.step(0)
    hip.synchronize()  # the NaNs exist now, but nothing has hashed them yet
    assert np.isnan(hip.buffer("position").reshape(-1, 4)[:cfg.particleCount, :3]).any()
    hip.step(1)
    with pytest.raises(sphmi.SphError, match="not finite"):
        hip.synchronize()
    types = hip.buffer("position").reshape(-1, 4)[:cfg.particleCount, 3].astype(np.int32)
    order = hip.buffer("particleIndex").reshape(-1, 2)[:, 1].astype(np.int64)
    has_liquid = nb.wave_any(types[order] != nb.BOUNDARY)
    assert not (hip.buffer("pressureForceSkipped")[has_liquid] != 0).any()
    assert not (hip.buffer("predictDensitySkipped")[has_liquid] != 0).any()
    hip.close()
