"""GPU tests of gradient sampling and surface normals (sph_sample_gradient_points / sph_sample_gradient_grid /
sph_surface_normals, include/sphmi.h): every record bit-identical to the numpy float32 restatement (tests/gradient_ref.py),
words 0..7 bit-identical to sampling, the grid paths bit-identical to the points path, normals bit-identical to the restatement
at the mesh's vertices and close to the mesh's own face normals, read-only behaviour, the calling rules and the driver's files."""
import os
import subprocess

import numpy as np
import pytest

import gradient_ref
import sample_ref
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
MASKS = [(1,), (1, 2, 3)]
BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=-1))
        i = int(bad[0])
        words = np.flatnonzero(bits(got[i]) != bits(want[i]))
        raise AssertionError("%s: %d of %d records differ; first %d, words %s: %r vs %r"
                             % (what, bad.size, got.shape[0], i, words.tolist(), got[i][words], want[i][words]))


def query_points(sc, positions, rng, n_random=1500):
    """Particle positions, random points in the box and just past its faces, two far points and two non-finite points (last)."""
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    h = np.float32(cfg.h)
    inside = rng.uniform(lo - 0.9 * h, hi + 0.9 * h, (n_random, 3)).astype(np.float32)
    far = np.array([[hi[0] + 10 * h, hi[1] + 10 * h, hi[2] + 10 * h], [lo[0] - 7 * h, lo[1], lo[2]]], np.float32)
    bad = np.array([[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]]], np.float32)
    pick = positions[rng.choice(positions.shape[0], min(1500, positions.shape[0]), replace=False), :3]
    return np.concatenate([pick, inside, far, bad]).astype(np.float32)


def check_points(hip, sc, rng, masks=MASKS):
    state = sample_ref.solver_state(hip)
    pts = query_points(sc, hip.read_position_buffer(), rng)
    for types in masks:
        got = hip.sample_gradient_points(pts, types)
        assert_bits(got, gradient_ref.gradient_reference(state, pts, types), "types %s" % (types,))
        assert_bits(got[:, :8], hip.sample_points(pts, types), "words 0..7 vs sample_points")
        assert not bits(got[-2:]).any()  # non-finite points: all-zero records
        assert (got[-4:-2] == 0).all()  # far points: zero values
    return state, pts, got


@pytest.mark.parametrize("name", ["tiny", "tiny_compressed", "tiny_elastic", "config1"])
def test_gradient_points_match_restatement(name):
    sc = scenes.config1() if name == "config1" else scenes.SCENES[name]()
    hip = scenes.hip_for(sc)
    rng = np.random.default_rng(21)
    hip.step(0)
    check_points(hip, sc, rng)
    for it in range(1, 5):
        hip.step(it)
    state, pts, got = check_points(hip, sc, rng)
    assert got[:, 6].max() > 10
    assert np.abs(got[:, 14:23]).max() > 0 and np.abs(got[:, 26:31]).max() > 0
    if name == "tiny_compressed":  # a pressure-active state: grad p is not trivial
        assert np.abs(state["p"]).max() > 0
        assert np.abs(got[:, 23:26]).max() > 0
    hip.close()


def test_gradient_worm_scene_reference_mode():
    """Reference-mode cell ids with aliased masked keys (the worm scene reaches past 16 bits of cell id)."""
    sc = scenes.worm_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)
    rng = np.random.default_rng(4)
    state = sample_ref.solver_state(hip)
    pos = hip.read_position_buffer()
    cfg = sc["cfg"]
    elastic = pos[(pos[:, 3] > 1.5) & (pos[:, 3] < 2.5)][:, :3]
    liq = pos[pos[:, 3] == 1][:, :3]
    pts = np.concatenate([elastic[rng.choice(elastic.shape[0], min(2000, elastic.shape[0]), replace=False)],
                          liq[rng.choice(liq.shape[0], min(2000, liq.shape[0]), replace=False)] + rng.normal(0, 1.0, (min(2000, liq.shape[0]), 3)),
                          rng.uniform([cfg.xmin, cfg.ymin, 672.0], [cfg.xmax, cfg.ymax, cfg.zmax], (2000, 3))]).astype(np.float32)
    for types in ((1,), (2,), (1, 2, 3)):
        got = hip.sample_gradient_points(pts, types)
        assert_bits(got, gradient_ref.gradient_reference(state, pts, types), "worm %s" % (types,))
    hip.close()


def grid_vs_points(hip, origin, spacing, dims, types=(1, 2, 3)):
    g = hip.sample_gradient_grid(origin, spacing, dims, types)
    assert g.shape == (dims[2], dims[1], dims[0], 32)
    pts = sample_ref.grid_points(origin, spacing, dims).reshape(-1, 3)
    assert_bits(g.reshape(-1, 32), hip.sample_gradient_points(pts, types), "grid %s x %s vs points" % (dims, spacing))
    assert_bits(g.reshape(-1, 32)[:, :8], hip.sample_grid(origin, spacing, dims, types).reshape(-1, 8), "words 0..7 vs sample_grid")
    return g, pts


def test_gradient_grid_equals_points_config1():
    sc = scenes.config1()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    h = np.float32(cfg.h)
    state = sample_ref.solver_state(hip)
    # spacing h/2 (brick path) with dims not multiples of 4, over part of the box and past its edges
    g, pts = grid_vs_points(hip, (-3.0, -2.0, 20.0), (h / 2, h / 2, h / 2), (47, 33, 30))
    sub = np.random.default_rng(3).choice(pts.shape[0], 5000, replace=False)
    assert_bits(g.reshape(-1, 32)[sub], gradient_ref.gradient_reference(state, pts[sub], (1, 2, 3)), "brick grid vs restatement")
    grid_vs_points(hip, (cfg.xmax - 20, cfg.ymax - 10, -5.0), (h / 3, h / 2, 0.6 * h), (41, 27, 21), types=(1,))
    # spacing > 2h/3: one lane per point
    g, _ = grid_vs_points(hip, (0.0, 0.0, 0.0), (1.5 * h, 1.5 * h, 2 * h), (21, 15, 40))
    assert g[..., 6].max() > 5
    # a lattice with non-finite points: all-zero records
    g = hip.sample_gradient_grid((np.inf, 0.0, 0.0), (h / 2, h / 2, h / 2), (5, 6, 7))
    assert not bits(g).any()
    # brick path so far out that float coordinates no longer resolve h: bricks whose cell box exceeds the 64 cells of the
    # wave-uniform walk go lane by lane; nothing is within h, so n is 0 and every word is zero (words 8..13 are K * 0 = -0,
    # as on the points path)
    far = ((2e7, 2e7, 2e7), (0.66 * h, 0.66 * h, 0.66 * h), (12, 12, 12))
    assert (sample_ref.brick_box_cells(*far, cfg.h, cfg.hashGridCellSizeInv) > 64).any()
    g, _ = grid_vs_points(hip, *far)
    assert not g.any() and not bits(g[..., 6]).any()
    hip.close()


def test_gradient_grid_wide_million_box_several_chunks():
    """1 M particles, wide cell ids; the 1.06 M-point lattice's 128-B records fill the 64 MiB sampling scratch twice over, so the
    grid goes in three z-chunks."""
    sc = scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100), mask=0xffffffff)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    hip.step(0)
    h = np.float32(cfg.h)
    dims = (102, 101, 103)
    assert dims[0] * dims[1] * dims[2] * 128 > 2 * (64 << 20)
    g, pts = grid_vs_points(hip, (cfg.xmin - 2, cfg.ymin - 2, cfg.zmin - 2), (h / 2, h / 2, h / 2), dims)
    assert g[..., 6].max() > 20
    state = sample_ref.solver_state(hip)
    sub = np.random.default_rng(9).choice(pts.shape[0], 10000, replace=False)
    assert_bits(g.reshape(-1, 32)[sub], gradient_ref.gradient_reference(state, pts[sub], (1, 2, 3)), "1M box subset")
    hip.close()


def _read_all(hip):
    return {name: hip.buffer(name).copy() for name in BUFFERS}


def test_gradient_sampling_is_read_only():
    """Every exported buffer is unchanged by gradient sampling and normals, and a solver that uses them every step ends
    bit-identical to an untouched twin."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    cfg = sc["cfg"]
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    spacing = np.full(3, h / 2, np.float32)
    buf = np.empty(4 * a.N, np.float32)
    rng = np.random.default_rng(1)
    for it in range(8):
        a.step(it)
        b.step(it)
        before = _read_all(a)
        a.read_position_buffer_async(buf)
        a.sample_gradient_grid((0.0, 0.0, 0.0), (h / 2, h / 2, h / 2), (17, 17, 17))
        a.sample_gradient_points(rng.uniform(0, cfg.xmax, (500, 3)), (1, 2))
        a.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1, 2))
        a.surface_normals()
        a.wait_position_buffer()
        after = _read_all(a)
        for name in BUFFERS:
            assert np.array_equal(before[name].view(np.uint8), after[name].view(np.uint8)), name
    assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer()))
    assert np.array_equal(bits(a.read_velocity_buffer()), bits(b.read_velocity_buffer()))
    assert np.array_equal(bits(a.read_density_buffer()), bits(b.read_density_buffer()))
    a.close()
    b.close()


def _rc_points(hip, pts, count, mask):
    out = np.empty((max(count, 1), 32), np.float32)
    p = None if pts is None else np.ascontiguousarray(pts, np.float32)
    return hip._L.sph_sample_gradient_points(hip._h, None if p is None else p.ctypes.data, count, mask, out.ctypes.data)


def _rc_grid(hip, dims, mask, null_out=False):
    o = np.zeros(3, np.float32)
    sp = np.ones(3, np.float32)
    d = np.ascontiguousarray(dims, np.int32)
    out = np.empty(max(int(np.prod(np.maximum(d, 1))), 1) * 32, np.float32)
    return hip._L.sph_sample_gradient_grid(hip._h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, mask,
                                           None if null_out else out.ctypes.data)


def _rc_normals(hip, n=1):
    out = np.empty((max(n, 1), 3), np.float32)
    return hip._L.sph_surface_normals(hip._h, out.ctypes.data)


def _padded(cfg, over_h=0.5):
    h = np.float32(cfg.h)
    sp = h * np.float32(over_h)
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) + 1.5 * h
    return lo, np.array([sp, sp, sp], np.float32), [int(np.ceil((hi[a] - lo[a]) / sp)) + 1 for a in range(3)]


def test_gradient_error_behaviour():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    twin = scenes.hip_for(sc)
    pts = np.zeros((4, 4), np.float32)
    assert _rc_points(hip, pts, 4, 0xE) == ERR_ORDER  # before any step
    assert _rc_grid(hip, (4, 4, 4), 0xE) == ERR_ORDER
    assert _rc_normals(hip) == ERR_ORDER  # no mesh
    hip.step(0)
    twin.step(0)
    assert _rc_normals(hip) == ERR_ORDER  # still no mesh
    with pytest.raises(sphmi.SphError):
        hip.surface_normals()
    origin, spacing, dims = _padded(sc["cfg"])
    verts, _ = hip.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1,))
    assert verts.shape[0] > 0
    assert hip.surface_normals().shape == verts.shape
    assert hip._L.sph_surface_normals(hip._h, None) == ERR_INVALID  # vertices but no output
    hip._runClearBuffers()  # any stage since the extraction: the normals are refused ...
    assert _rc_normals(hip, verts.shape[0]) == ERR_ORDER
    assert hip._L.sph_read_surface(hip._h, None, None) == 0  # ... the mesh itself can still be read
    hip._runHashParticles()  # a new step has begun: its density has not been computed
    assert _rc_points(hip, pts, 4, 0xE) == ERR_ORDER
    assert _rc_grid(hip, (4, 4, 4), 0xE) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[2:]:  # finish that step through the staged path
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    twin.step(1)
    assert _rc_points(hip, pts, 4, 0xE) == 0
    assert _rc_normals(hip, verts.shape[0]) == ERR_ORDER
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_points(hip, pts, 4, mask) == ERR_INVALID
        assert _rc_grid(hip, (4, 4, 4), mask) == ERR_INVALID
    for d in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert _rc_grid(hip, d, 0xE) == ERR_INVALID
    assert _rc_grid(hip, (4, 4, 4), 0xE, null_out=True) == ERR_INVALID
    assert _rc_points(hip, pts, -1, 0xE) == ERR_INVALID
    assert _rc_points(hip, None, 3, 0xE) == ERR_INVALID
    assert _rc_points(hip, None, 0, 0xE) == 0  # count == 0: nothing to do
    assert hip.sample_gradient_points(np.zeros((0, 3), np.float32)).shape == (0, 32)
    # a fresh extraction allows normals again; a fused step refuses them
    verts, _ = hip.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1,))
    assert _rc_normals(hip, verts.shape[0]) == 0
    hip.step(2)
    twin.step(2)
    assert _rc_normals(hip, verts.shape[0]) == ERR_ORDER
    assert hip._L.sph_read_surface(hip._h, None, None) == 0
    # a failed extraction leaves no mesh: ORDER again
    o, sp, d = np.zeros(3, np.float32), np.ones(3, np.float32), np.full(3, 4, np.int32)
    c = np.zeros(2, np.int64)
    assert hip._L.sph_extract_surface(hip._h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, 0x2, 9, 0.5, c.ctypes.data) == ERR_INVALID
    assert _rc_normals(hip) == ERR_ORDER
    for it in range(3, 5):  # the solver still steps correctly afterwards
        hip.step(it)
        twin.step(it)
    assert np.array_equal(bits(hip.read_position_buffer()), bits(twin.read_position_buffer()))
    hip.close()
    twin.close()


def test_gradient_of_a_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_points(hip, np.zeros((4, 4), np.float32), 4, 0xE) == ERR_INVALID
    assert _rc_grid(hip, (4, 4, 4), 0xE) == ERR_INVALID
    assert _rc_normals(hip) == ERR_ORDER
    hip.close()


def face_normals_at_vertices(verts, tris):
    """Unit area-weighted sums of the normals (v1-v0)x(v2-v0) of the triangles around each vertex (float64)."""
    v = verts.astype(np.float64)
    fn = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])  # length = 2 x area
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, tris[:, k], fn)
    ln = np.linalg.norm(acc, axis=1)
    return acc / np.where(ln > 0, ln, 1)[:, None], ln > 0


def check_normals(hip, origin, spacing, dims, field, iso, types, min_agree=None):
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=iso, field=field, types=types)
    assert verts.shape[0] > 100
    normals = hip.surface_normals()
    word = frames.GRID_FIELDS.index(field)
    state = sample_ref.solver_state(hip)
    rec = gradient_ref.gradient_reference(state, verts, types)
    assert_bits(rec, hip.sample_gradient_points(verts, types), "gradient records at the vertices")
    assert_bits(normals, gradient_ref.normals_reference(rec, word), "normals %s" % field)
    if min_agree is not None:
        fn, ok = face_normals_at_vertices(verts, tris)
        unit = np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1) < 1e-6
        cos = (fn * normals).sum(1)
        frac = float(((cos > 0.9) & ok & unit).mean())
        print("%s: %.4f of %d vertex normals within 25.8 deg of the face normals" % (field, frac, verts.shape[0]))
        assert frac >= min_agree, frac
    return verts, normals


def test_normals_match_restatement_and_faces():
    """Bit-exact normals for the Shepard, density, velocity and pressure fields. On this small box (762 vertices, many of them on
    edges and corners of the liquid block) 93.3 % of the Shepard surface's vertex normals lie within 25.8 degrees (cos > 0.9) of
    the area-weighted normals of the triangles around them; the bound is 90 %."""
    sc = scenes.SCENES["tiny_compressed"]()
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    origin, spacing, dims = _padded(sc["cfg"])
    check_normals(hip, origin, spacing, dims, "shepard", 0.5, (1,), min_agree=0.90)
    check_normals(hip, origin, spacing, dims, "density", 500.0, (1,))
    g = hip.sample_grid(origin, spacing, dims, (1,))
    for field, word in (("vx", 2), ("pressure", 5)):
        inside = g[..., 1] > 0.5
        iso = float(np.median(g[..., word][inside]))
        check_normals(hip, origin, spacing, dims, field, iso, (1,))
    hip.close()


def test_normals_config1():
    """config #1 after 2 steps (about 6,000 vertices): 99.6 % of the vertex normals agree with the face normals to cos > 0.9;
    the bound is 98 %."""
    sc = scenes.config1()
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    origin, spacing, dims = _padded(sc["cfg"])
    check_normals(hip, origin, spacing, dims, "shepard", 0.5, (1, 2), min_agree=0.98)
    hip.close()


def test_cpp_driver_gradients_and_normals(tmp_path):
    """sphmi_run --sample-gradients / --surface-normals: the files equal sample_gradient_grid and the normals of a Python solver on
    the same scene after the same steps."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    dims = (9, 7, 11)
    sdims = (17, 15, 19)
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--sample-grid"]
                       + [str(d) for d in dims] + ["--sample-every", "2", "--sample-out", str(tmp_path), "--sample-gradients",
                                                   "--surface-grid"] + [str(d) for d in sdims]
                       + ["--surface-every", "2", "--surface-out", str(tmp_path), "--surface-normals"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "_sampleGradientGrid:" in r.stdout
    sc = scenes.SCENES["tiny"]()  # the same box
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    spacing = (hi - lo) / np.float32(np.array(dims, np.float32) - np.float32(1))
    sspacing = (hi - lo) / np.float32(np.array(sdims, np.float32) - np.float32(1))
    hip = scenes.hip_for(sc)
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want = hip.sample_gradient_grid(lo, spacing, dims)
            got = frames.read_gradients(str(tmp_path / ("gradients_%d.bin" % (it + 1))), dims)
            assert_bits(got.reshape(-1, 32), want.reshape(-1, 32), "gradients_%d" % (it + 1))
            assert np.abs(want[..., 26:29]).max() > 0
            want_v, want_t = hip.extract_surface(lo, sspacing, sdims, iso=0.5, field="shepard", types=(1, 2))
            want_n = hip.surface_normals()
            got_v, got_t, got_n = frames.read_ply(str(tmp_path / ("surface_%d.ply" % (it + 1))), with_normals=True)
            assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_t, want_t)
            assert got_n is not None and np.array_equal(bits(got_n), bits(want_n))
            assert want_t.shape[0] > 100
    hip.close()
    assert sorted(os.listdir(tmp_path)) == ["fields_2.bin", "fields_4.bin", "gradients_2.bin", "gradients_4.bin",
                                            "surface_2.ply", "surface_4.ply"]
    for args, msg in ((["--sample-gradients"], "--sample-gradients needs --sample-grid"),
                      (["--surface-normals"], "--surface-normals needs --surface-grid")):
        bad = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "1"] + args,
                             capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and msg in bad.stderr, bad.stderr
