"""GPU tests of field sampling (sph_sample_points / sph_sample_grid, include/sphmi.h): every record bit-identical to the numpy
float32 restatement of the contract (tests/sample_ref.py), the grid path bit-identical to the points path, sampling read-only
on the solver, and the calling rules."""
import os
import subprocess

import numpy as np
import pytest

import sample_ref
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

MASKS = [(1,), (1, 2), (1, 2, 3)]
SAMPLE_ORDER = -3  # SPH_ERR_ORDER
SAMPLE_INVALID = -1  # SPH_ERR_INVALID


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(bits(got), bits(want)):
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=-1))
        i = int(bad[0])
        raise AssertionError("%s: %d of %d records differ; first %d: %r vs %r" % (what, bad.size, got.shape[0], i, got[i], want[i]))


def query_points(sc, positions, rng, n_random=2000):
    """Every particle position, random points in the box, points just outside the box within h of the boundary shell,
    points far from everything and a NaN point."""
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    h = np.float32(cfg.h)
    inside = rng.uniform(lo, hi, (n_random, 3)).astype(np.float32)
    # just outside one face, within h of the shell
    out = rng.uniform(lo, hi, (600, 3)).astype(np.float32)
    axis = rng.integers(0, 3, 600)
    side = rng.integers(0, 2, 600)
    depth = rng.uniform(0.0, 0.95, 600).astype(np.float32) * h
    for k in range(600):
        a = axis[k]
        out[k, a] = lo[a] - depth[k] if side[k] == 0 else hi[a] + depth[k]
    far = np.array([[hi[0] + 10 * h, hi[1] + 10 * h, hi[2] + 10 * h], [lo[0] - 7 * h, lo[1], lo[2]]], np.float32)
    nan = np.array([[np.nan, lo[1], lo[2]]], np.float32)
    return np.concatenate([positions[:, :3], inside, out, far, nan]).astype(np.float32), far.shape[0], nan.shape[0]


def check_points(hip, sc, rng, masks=MASKS):
    state = sample_ref.solver_state(hip)
    pts, n_far, _ = query_points(sc, hip.read_position_buffer(), rng)
    for types in masks:
        got = hip.sample_points(pts, types)
        want = sample_ref.sample_reference(state, pts, types)
        assert_bits(got, want, "types %s" % (types,))
        # the far points and the NaN point give all-zero records with n == 0
        assert not bits(got[-(n_far + 1):]).any()
    return state, pts


@pytest.mark.parametrize("name", ["tiny", "tiny_compressed", "tiny_elastic", "config1"])
def test_sample_points_match_restatement(name):
    sc = scenes.config1() if name == "config1" else scenes.SCENES[name]()
    hip = scenes.hip_for(sc)
    rng = np.random.default_rng(11)
    hip.step(0)  # the first step's sorted state
    _, _ = check_points(hip, sc, rng)
    for it in range(1, 5):
        hip.step(it)
    state, pts = check_points(hip, sc, rng)
    got = hip.sample_points(pts, (1, 2, 3))
    assert got[:, 6].max() > 10, "the query points must hit particles"
    hip.close()


def test_sample_points_after_the_staged_path():
    """The sph_run_* stage sequence leaves the same sorted state to sample as the fused step."""
    sc = scenes.SCENES["tiny_elastic"]()
    hip = scenes.hip_for(sc)
    for st in scenes.STAGE_SEQUENCE:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(0) if st == "integrate" else m()
    check_points(hip, sc, np.random.default_rng(5), masks=[(1, 2, 3)])
    hip.close()


def _alias_points(sc, rng, z_lo):
    cfg = sc["cfg"]
    pos = sc["position"]
    liq = pos[pos[:, 3] == 1][:, :3]
    k = min(3000, liq.shape[0])
    pick = liq[rng.choice(liq.shape[0], k, replace=False)] + rng.normal(0, 1.0, (k, 3)).astype(np.float32)
    region = rng.uniform([cfg.xmin, cfg.ymin, z_lo], [cfg.xmax, cfg.ymax, cfg.zmax], (2000, 3))
    anywhere = rng.uniform([cfg.xmin, cfg.ymin, cfg.zmin], [cfg.xmax, cfg.ymax, cfg.zmax], (2000, 3))
    return np.concatenate([pick, region, anywhere]).astype(np.float32)


def test_aliased_cells_reference_mode():
    """alias16: liquid at z > 672 where raw cell ids exceed 16 bits, so runs of masked keys mix far-apart cells. The records equal
    the restatement (whose selected set is a brute-force search) bit for bit. The wide twin, after the same first step (same
    positions, different sorted order), selects the same number of particles at every point; its values agree to 1e-5 with the
    alias16 selection weighted by the wide run's own densities and pressures (the two modes' 32-neighbour lists, and so a few
    densities near the walls, differ)."""
    sc = scenes.SCENES["alias16"]()
    assert sc["cfg"].cellIdMask == 0xffff and sc["cfg"].gridCellCount > 65536
    rng = np.random.default_rng(2)
    pts = _alias_points(sc, rng, 672.0)
    hip = scenes.hip_for(sc)
    first = None
    for it in range(2):
        hip.step(it)
        state = sample_ref.solver_state(hip)
        assert (state["pos"][:, 2] > 672).any()
        got = hip.sample_points(pts, (1, 2, 3))
        assert_bits(got, sample_ref.sample_reference(state, pts, (1, 2, 3)), "alias16 step %d" % it)
        assert got[:, 6].max() > 10
        if first is None:
            first, first_state, first_orig = got, state, hip.read_particleIndex_buffer()[:, 1]
    hip.close()
    wide = scenes.hip_for(scenes.SCENES["wide"]())
    wide.step(0)
    wgot = wide.sample_points(pts, (1, 2, 3))
    wstate = sample_ref.solver_state(wide)
    worig = wide.read_particleIndex_buffer()[:, 1]
    wide.close()
    assert np.array_equal(wgot[:, 6], first[:, 6])
    rho_by_orig = np.empty_like(wstate["rho"])
    p_by_orig = np.empty_like(wstate["p"])
    rho_by_orig[worig] = wstate["rho"]
    p_by_orig[worig] = wstate["p"]
    mixed = dict(first_state, rho=rho_by_orig[first_orig], p=p_by_orig[first_orig])
    want = sample_ref.sample_reference(mixed, pts, (1, 2, 3))
    for col in range(7):
        scale = np.abs(want[:, col]).max()
        np.testing.assert_allclose(wgot[:, col], want[:, col], rtol=1e-5, atol=1e-5 * scale)


def test_aliased_cells_worm_scene():
    sc = scenes.worm_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)
    rng = np.random.default_rng(4)
    state = sample_ref.solver_state(hip)
    pos = hip.read_position_buffer()
    elastic = pos[(pos[:, 3] > 1.5) & (pos[:, 3] < 2.5)][:, :3]
    pts = np.concatenate([elastic[rng.choice(elastic.shape[0], min(3000, elastic.shape[0]), replace=False)],
                          _alias_points(sc, rng, 672.0)]).astype(np.float32)
    for types in MASKS:
        got = hip.sample_points(pts, types)
        assert_bits(got, sample_ref.sample_reference(state, pts, types), "worm %s" % (types,))
    hip.close()


def grid_vs_points(hip, origin, spacing, dims, types=(1, 2, 3)):
    g = hip.sample_grid(origin, spacing, dims, types)
    assert g.shape == (dims[2], dims[1], dims[0], 8)
    pts = sample_ref.grid_points(origin, spacing, dims).reshape(-1, 3)
    p = hip.sample_points(pts, types)
    assert_bits(g.reshape(-1, 8), p, "grid %s x %s" % (dims, spacing))
    return g, pts


def test_sample_grid_equals_points_config1():
    sc = scenes.config1()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    h = np.float32(cfg.h)
    # spacing h/2 (brick path) with dims not multiples of 4, over part of the box and past its edges
    grid_vs_points(hip, (-3.0, -2.0, 20.0), (h / 2, h / 2, h / 2), (47, 33, 30))
    grid_vs_points(hip, (cfg.xmax - 20, cfg.ymax - 10, -5.0), (h / 3, h / 2, 0.6 * h), (41, 27, 21), types=(1,))
    # spacing > 2h/3: one lane per point
    g, _ = grid_vs_points(hip, (0.0, 0.0, 0.0), (1.5 * h, 1.5 * h, 2 * h), (21, 15, 40))
    assert g[..., 6].max() > 5
    # brick path so far out that float coordinates no longer resolve h: bricks whose cell box exceeds the 64 cells of the
    # wave-uniform walk go lane by lane; nothing is within h, so every record is all +0
    far = ((2e7, 2e7, 2e7), (0.66 * h, 0.66 * h, 0.66 * h), (12, 12, 12))
    assert (sample_ref.brick_box_cells(*far, cfg.h, cfg.hashGridCellSizeInv) > 64).any()
    g, _ = grid_vs_points(hip, *far)
    assert not bits(g).any()
    hip.close()


def test_sample_grid_wide_million_box():
    sc = scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100), mask=0xffffffff)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    hip.step(0)
    h = np.float32(cfg.h)
    g, pts = grid_vs_points(hip, (cfg.xmin - 2, cfg.ymin - 2, cfg.zmin - 2), (h / 2, h / 2, h / 2), (102, 101, 103))
    assert g[..., 6].max() > 20
    state = sample_ref.solver_state(hip)
    rng = np.random.default_rng(9)
    sub = rng.choice(pts.shape[0], 10000, replace=False)
    assert_bits(g.reshape(-1, 8)[sub], sample_ref.sample_reference(state, pts[sub], (1, 2, 3)), "1M box subset")
    hip.close()


def test_sampling_is_read_only():
    """A solver that samples every step (with an asynchronous position read in between) ends bit-identical to an untouched twin."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    cfg = sc["cfg"]
    h = np.float32(cfg.h)
    buf = np.empty(4 * a.N, np.float32)
    rng = np.random.default_rng(1)
    for it in range(10):
        a.step(it)
        b.step(it)
        a.read_position_buffer_async(buf)
        a.sample_grid((0.0, 0.0, 0.0), (h / 2, h / 2, h / 2), (17, 17, 17))
        a.sample_points(rng.uniform(0, cfg.xmax, (500, 3)), (1, 2))
        a.wait_position_buffer()
    assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer()))
    assert np.array_equal(bits(a.read_velocity_buffer()), bits(b.read_velocity_buffer()))
    assert np.array_equal(bits(a.read_density_buffer()), bits(b.read_density_buffer()))
    a.close()
    b.close()


def _rc_points(hip, pts, count, mask):
    out = np.empty((max(count, 1), 8), np.float32)
    p = None if pts is None else np.ascontiguousarray(pts, np.float32)
    return hip._L.sph_sample_points(hip._h, None if p is None else p.ctypes.data, count, mask, out.ctypes.data)


def _rc_grid(hip, dims, mask):
    o = np.zeros(3, np.float32)
    sp = np.ones(3, np.float32)
    d = np.ascontiguousarray(dims, np.int32)
    out = np.empty(max(int(np.prod(np.maximum(d, 1))), 1) * 8, np.float32)
    return hip._L.sph_sample_grid(hip._h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, mask, out.ctypes.data)


def test_sampling_error_behaviour():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    twin = scenes.hip_for(sc)
    pts = np.zeros((4, 4), np.float32)
    assert _rc_points(hip, pts, 4, 0xE) == SAMPLE_ORDER  # before any step
    assert _rc_grid(hip, (4, 4, 4), 0xE) == SAMPLE_ORDER
    hip.step(0)
    twin.step(0)
    hip._runClearBuffers()
    hip._runHashParticles()  # a new step has begun: its density has not been computed
    assert _rc_points(hip, pts, 4, 0xE) == SAMPLE_ORDER
    assert _rc_grid(hip, (4, 4, 4), 0xE) == SAMPLE_ORDER
    for st in scenes.STAGE_SEQUENCE[2:]:  # finish that step through the staged path
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    twin.step(1)
    assert _rc_points(hip, pts, 4, 0xE) == 0
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_points(hip, pts, 4, mask) == SAMPLE_INVALID
        assert _rc_grid(hip, (4, 4, 4), mask) == SAMPLE_INVALID
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert _rc_grid(hip, dims, 0xE) == SAMPLE_INVALID
    assert _rc_points(hip, pts, -1, 0xE) == SAMPLE_INVALID
    assert _rc_points(hip, None, 3, 0xE) == SAMPLE_INVALID
    assert _rc_points(hip, None, 0, 0xE) == 0  # count == 0: nothing to do
    assert hip.sample_points(np.zeros((0, 3), np.float32)).shape == (0, 8)
    with pytest.raises(sphmi.SphError):
        hip.sample_points(pts, (0,))
    # the solver still steps correctly afterwards
    for it in range(2, 5):
        hip.step(it)
        twin.step(it)
    assert np.array_equal(bits(hip.read_position_buffer()), bits(twin.read_position_buffer()))
    hip.close()
    twin.close()


def test_sampling_a_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_points(hip, np.zeros((4, 4), np.float32), 4, 0xE) == SAMPLE_INVALID
    assert _rc_grid(hip, (4, 4, 4), 0xE) == SAMPLE_INVALID
    hip.close()


def test_cpp_driver_sample_grid(tmp_path):
    """sphmi_run --sample-grid: the files equal sample_grid of a Python solver on the same scene after the same steps."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    dims = (9, 7, 11)
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--quiet", "--sample-grid"]
                       + [str(d) for d in dims] + ["--sample-every", "2", "--sample-out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = scenes.SCENES["tiny"]()  # the same box: lattice spacing 0.93 r0 from 3 r0, reference-mode cell ids
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    spacing = (hi - lo) / np.float32(np.array(dims, np.float32) - np.float32(1))
    hip = scenes.hip_for(sc)
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want = hip.sample_grid(lo, spacing, dims)
            got = frames.read_fields(str(tmp_path / ("fields_%d.bin" % (it + 1))), dims)
            assert_bits(got.reshape(-1, 8), want.reshape(-1, 8), "fields_%d" % (it + 1))
            assert want[..., 6].max() > 5
    hip.close()
    assert sorted(os.listdir(tmp_path)) == ["fields_2.bin", "fields_4.bin"]
