"""GPU tests of isosurface extraction (sph_extract_surface / sph_read_surface, include/sphmi.h): every mesh bit-identical to the
numpy restatement of the contract (tests/surface_ref.py) applied to sample_grid's records for the same arguments (sample_grid
itself is pinned by test_sample.py), closed wherever the lattice is padded, read-only on the solver, the calling rules, and
the driver's PLY files."""
import os
import subprocess

import numpy as np
import pytest

import scenes
import sphmi
import surface_ref
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def padded_lattice(cfg, spacing_over_h, pad_over_h=1.5):
    """A lattice over the scene's box extended by pad_over_h * h on every side (more than h past every particle, so a field
    of liquid / elastic particles is 0 on its border)."""
    h = np.float32(cfg.h)
    sp = h * np.float32(spacing_over_h)
    pad = h * np.float32(pad_over_h)
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - pad
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) + pad
    dims = [int(np.ceil((hi[a] - lo[a]) / sp)) + 1 for a in range(3)]
    return lo, np.array([sp, sp, sp], np.float32), dims


def check_surface(hip, origin, spacing, dims, iso, field, types, closed=True, min_tris=1):
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=iso, field=field, types=types)
    word = frames.GRID_FIELDS.index(field) if isinstance(field, str) else int(field)
    g = hip.sample_grid(origin, spacing, dims, types)
    rv, rt = surface_ref.surface_reference(g[..., word], origin, spacing, iso)
    assert verts.shape == rv.shape and tris.shape == rt.shape, (verts.shape, rv.shape, tris.shape, rt.shape)
    if not np.array_equal(bits(verts), bits(rv)):
        bad = np.flatnonzero((bits(verts) != bits(rv)).any(axis=1))
        raise AssertionError("%d of %d vertices differ; first %d: %r vs %r" % (bad.size, rv.shape[0], bad[0], verts[bad[0]], rv[bad[0]]))
    if not np.array_equal(tris, rt):
        bad = np.flatnonzero((tris != rt).any(axis=1))
        raise AssertionError("%d of %d triangles differ; first %d: %r vs %r" % (bad.size, rt.shape[0], bad[0], tris[bad[0]], rt[bad[0]]))
    assert tris.shape[0] >= min_tris
    if closed:
        report = surface_ref.directed_edge_report(tris, verts.shape[0])
        assert report is None, report
    return verts, tris


@pytest.mark.parametrize("name", ["tiny", "tiny_elastic", "config1"])
def test_surface_matches_restatement(name):
    sc = scenes.config1() if name == "config1" else scenes.SCENES[name]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    origin, spacing, dims = padded_lattice(cfg, 0.5)
    verts, tris = check_surface(hip, origin, spacing, dims, 0.5, "shepard", (1,))
    assert surface_ref.signed_volume(verts, tris) > 0  # normals point out of the liquid
    check_surface(hip, origin, spacing, dims, np.float32(0.5) * np.float32(cfg.rho0), "density", (1,))
    # a coarser lattice, not padded on the low side: meshes still equal the restatement (open where they reach the border)
    check_surface(hip, (cfg.xmin + 2.0, cfg.ymin + 2.0, cfg.zmin + 2.0), spacing * np.float32(1.3), [d // 2 for d in dims], 0.5,
                  1, (1, 2, 3), closed=False)
    hip.close()


def test_surface_pressure_iso():
    """Outside the fluid the sampled pressure is 0, so a positive iso keeps the padded border outside."""
    sc = scenes.SCENES["tiny_compressed"]()
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    g = hip.sample_grid(origin, spacing, dims, (1,))
    pmax = float(g[..., 5].max())
    assert pmax > 0
    check_surface(hip, origin, spacing, dims, np.float32(0.25 * pmax), "pressure", (1,))
    hip.close()


def test_surface_worm_reference_mode():
    """The worm scene (reference-mode cell ids: aliased cells occur); liquid and elastic Shepard field on a padded h/2 lattice."""
    sc = scenes.worm_scene()
    assert sc["cfg"].cellIdMask == 0xffff
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    check_surface(hip, origin, spacing, dims, 0.5, "shepard", (1, 2), min_tris=1000)
    hip.close()


@pytest.fixture(scope="module")
def wide_cube():
    sc = scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100), mask=0xffffffff)
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.step(1)
    yield sc, hip
    hip.close()


def test_surface_wide_million_cube(wide_cube):
    sc, hip = wide_cube
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    verts, tris = check_surface(hip, origin, spacing, dims, 0.5, "shepard", (1,), min_tris=10000)
    assert surface_ref.euler_characteristic(verts, tris) % 2 == 0


def test_surface_across_sampling_chunks(wide_cube):
    """A lattice whose 32-B records exceed the 64 MiB sampling scratch at least three times: the field comes from several
    z-chunks, so chunk seams and vertex numbering across them are covered."""
    sc, hip = wide_cube
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.25)
    npts = dims[0] * dims[1] * dims[2]
    assert npts * 32 >= 3 * (64 << 20), npts
    check_surface(hip, origin, spacing, dims, 0.5, "shepard", (1,), min_tris=10000)


def test_surface_empty_mesh():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    hip.step(0)
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=1e30)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)
    counts = np.full(2, -7, np.int64)
    assert _rc_extract(hip, dims, 0x2, 1, 1e30, counts=counts) == 0
    assert counts.tolist() == [0, 0]
    assert hip._L.sph_read_surface(hip._h, None, None) == 0
    hip.close()


def test_surface_is_read_only():
    """A solver that extracts and reads a surface every step ends bit-identical to an untouched twin."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    buf = np.empty(4 * a.N, np.float32)
    n_tris = 0
    for it in range(8):
        a.step(it)
        b.step(it)
        a.read_position_buffer_async(buf)
        _, tris = a.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1, 2))
        n_tris += tris.shape[0]
        a.wait_position_buffer()
    assert n_tris > 0
    assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer()))
    assert np.array_equal(bits(a.read_velocity_buffer()), bits(b.read_velocity_buffer()))
    assert np.array_equal(bits(a.read_density_buffer()), bits(b.read_density_buffer()))
    a.close()
    b.close()


def _rc_extract(hip, dims, mask, field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), counts=None, null=None):
    o = np.ascontiguousarray(origin, np.float32)
    sp = np.ascontiguousarray(spacing, np.float32)
    d = np.ascontiguousarray(dims, np.int32)
    c = np.zeros(2, np.int64) if counts is None else counts
    args = [o.ctypes.data, sp.ctypes.data, d.ctypes.data, c.ctypes.data]
    if null is not None:
        args[null] = None
    return hip._L.sph_extract_surface(hip._h, args[0], args[1], args[2], mask, field, iso, args[3])


def test_surface_error_behaviour():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    twin = scenes.hip_for(sc)
    out_v = np.empty((8, 3), np.float32)
    assert hip._L.sph_read_surface(hip._h, out_v.ctypes.data, None) == ERR_ORDER  # before any extraction
    assert _rc_extract(hip, (4, 4, 4), 0x2, 1, 0.5) == ERR_ORDER  # before any step
    hip.step(0)
    twin.step(0)
    origin, spacing, dims = padded_lattice(sc["cfg"], 0.5)
    counts = np.zeros(2, np.int64)
    assert _rc_extract(hip, dims, 0x2, 1, 0.5, origin, spacing, counts) == 0 and counts[1] > 0
    assert hip._L.sph_read_surface(hip._h, None, None) == 0
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_extract(hip, (4, 4, 4), mask, 1, 0.5) == ERR_INVALID
    assert hip._L.sph_read_surface(hip._h, None, None) == ERR_ORDER  # a failed call leaves no mesh behind
    for field in (-1, 6, 7):
        assert _rc_extract(hip, (4, 4, 4), 0x2, field, 0.5) == ERR_INVALID
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert _rc_extract(hip, (4, 4, 4), 0x2, 1, iso) == ERR_INVALID
    for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -3, 4)):
        assert _rc_extract(hip, d, 0x2, 1, 0.5) == ERR_INVALID
    assert _rc_extract(hip, (2048, 2048, 512), 0x2, 1, 0.5) == ERR_INVALID  # 2^31 points
    assert _rc_extract(hip, (65536, 65536, 2), 0x2, 1, 0.5) == ERR_INVALID  # the product overflows 32 bits
    for null in range(4):
        assert _rc_extract(hip, (4, 4, 4), 0x2, 1, 0.5, null=null) == ERR_INVALID
    with pytest.raises(sphmi.SphError):
        hip.extract_surface(origin, spacing, dims, field="count")
    # a new step has begun: its density has not been computed
    hip._runClearBuffers()
    hip._runHashParticles()
    assert _rc_extract(hip, dims, 0x2, 1, 0.5, origin, spacing) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[2:]:  # finish that step through the staged path
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    twin.step(1)
    check_surface(hip, origin, spacing, dims, 0.5, 1, (1,))
    for it in range(2, 5):  # the solver still steps correctly afterwards
        hip.step(it)
        twin.step(it)
    assert np.array_equal(bits(hip.read_position_buffer()), bits(twin.read_position_buffer()))
    hip.close()
    twin.close()


def test_surface_of_a_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_extract(hip, (4, 4, 4), 0x2, 1, 0.5) == ERR_INVALID
    assert hip._L.sph_read_surface(hip._h, None, None) == ERR_ORDER
    hip.close()


def test_cpp_driver_surface(tmp_path):
    """sphmi_run --surface-grid: the PLY files equal extract_surface of a Python solver on the same scene after the same steps."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    dims = (17, 15, 19)
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--surface-grid"]
                       + [str(d) for d in dims] + ["--surface-every", "2", "--surface-out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "_extractSurface:" in r.stdout
    sc = scenes.SCENES["tiny"]()  # the same box
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    spacing = (hi - lo) / np.float32(np.array(dims, np.float32) - np.float32(1))
    hip = scenes.hip_for(sc)
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want_v, want_t = hip.extract_surface(lo, spacing, dims, iso=0.5, field="shepard", types=(1, 2))
            got_v, got_t = frames.read_ply(str(tmp_path / ("surface_%d.ply" % (it + 1))))
            assert np.array_equal(bits(got_v), bits(want_v))
            assert np.array_equal(got_t, want_t)
            assert want_t.shape[0] > 100
    hip.close()
    assert sorted(os.listdir(tmp_path)) == ["surface_2.ply", "surface_4.ply"]
    bad = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "1", "--surface-grid", "9", "9",
                          "9"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "go together" in bad.stderr
