"""GPU tests of the surface measures (sph_measure_surface / sph_read_shells, include/sphmi.h): shell numbers, table, boxes, counts
and exponents bit-equal to the numpy restatement (tests/shell_ref.py) run on the mesh sph_read_surface returns, on the scenes of
tests/shell_cases.py (tests/test_surface_shells_host.py shows on the CPU that each has something to compare); the empty mesh,
repeatability, the column sums, the measure's lifetime, the error table, read-only behaviour and the driver's CSV files."""
import os
import subprocess

import numpy as np
import pytest

import scenes
import shell_cases
import shell_ref
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
COUNT_KEYS = ("shells", "closed", "open_sides", "bad_triangles")
EXP_KEYS = ("kA", "kV", "kM")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stepped(sc, steps=shell_cases.STEPS):
    hip = scenes.hip_for(sc)
    for it in range(steps):
        hip.step(it)
    return hip


def extract(hip, field, types, iso, lattice):
    origin, spacing, dims = lattice
    if iso is None:
        g = hip.sample_grid(origin, spacing, dims, types)
        iso = shell_cases.iso_of(g[..., shell_cases.FIELD_WORD[field]], None)
    return hip.extract_surface(origin, spacing, dims, iso=iso, field=field, types=types)


def measured(hip):
    m = hip.measure_surface()
    vs, table, bb = hip.surface_shells()
    return m, vs, table, bb


def assert_equals_restatement(hip, verts, tris, lattice, where):
    m, vs, table, bb = measured(hip)
    ref = shell_ref.measure(verts, tris, *lattice)
    print(where, "V", verts.shape[0], "T", tris.shape[0], "device", m, "restatement", ref["counts"].tolist(), ref["exps"].tolist())
    assert [m[k] for k in COUNT_KEYS] == ref["counts"].tolist(), where
    assert [m[k] for k in EXP_KEYS] == ref["exps"].tolist(), where
    assert vs.dtype == np.int32 and np.array_equal(vs, ref["vertexShell"]), where
    assert table.dtype == np.int64 and table.shape == ref["table"].shape, where
    if not np.array_equal(table, ref["table"]):
        bad = np.argwhere(table != ref["table"])
        raise AssertionError("%s: %d table words differ; first at shell %d word %d: %d vs %d" % (
            where, bad.shape[0], bad[0, 0], bad[0, 1], table[bad[0, 0], bad[0, 1]], ref["table"][bad[0, 0], bad[0, 1]]))
    assert np.array_equal(bits(bb), bits(ref["bbox"])), where
    return m, vs, table, bb


@pytest.mark.parametrize("name", list(shell_cases.CASES))
def test_shells_equal_restatement(name):
    sc, field, types, iso, lattice = shell_cases.case(name)
    hip = stepped(sc)
    verts, tris = extract(hip, field, types, iso, lattice)
    assert tris.shape[0] > 0
    m, vs, table, bb = assert_equals_restatement(hip, verts, tris, lattice, name)
    # column sums
    assert int(table[:, 1].sum()) == verts.shape[0] and int(table[:, 2].sum()) == tris.shape[0]
    assert int(table[:, 3].sum()) == m["open_sides"] and int(table[:, 4].sum()) == m["bad_triangles"] == 0
    assert int((table[:, 3] == 0).sum()) == m["closed"]
    # repeatability: a second call returns identical bytes
    m2, vs2, table2, bb2 = measured(hip)
    assert m2 == m and vs2.tobytes() == vs.tobytes() and table2.tobytes() == table.tobytes() and bb2.tobytes() == bb.tobytes()
    hip.close()


def test_empty_mesh():
    sc = scenes.SCENES["tiny"]()
    hip = stepped(sc, 1)
    lattice = shell_cases.liquid_lattice(sc, 0.5)
    verts, tris = hip.extract_surface(*lattice, iso=1e30)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)
    m = hip.measure_surface()
    assert [m[k] for k in COUNT_KEYS] == [0, 0, 0, 0]
    ref = shell_ref.measure(verts, tris, *lattice)
    assert [m[k] for k in EXP_KEYS] == ref["exps"].tolist()
    vs, table, bb = hip.surface_shells()
    assert vs.shape == (0,) and table.shape == (0, 10) and bb.shape == (0, 6)
    assert hip._L.sph_read_shells(hip._h, None, None, None) == 0
    hip.close()


def test_lifetime():
    """Legal, with identical bytes, after further steps; dropped by a new extraction and by a failed one."""
    sc, field, types, iso, lattice = shell_cases.case("pieces")
    hip = stepped(sc)
    extract(hip, field, types, iso, lattice)
    m, vs, table, bb = measured(hip)
    hip.step(2)
    hip.step(3)
    vs2, table2, bb2 = hip.surface_shells()  # the reader alone
    assert vs2.tobytes() == vs.tobytes() and table2.tobytes() == table.tobytes() and bb2.tobytes() == bb.tobytes()
    m3, vs3, table3, bb3 = measured(hip)  # and a new measure of the same mesh
    assert m3 == m and vs3.tobytes() == vs.tobytes() and table3.tobytes() == table.tobytes() and bb3.tobytes() == bb.tobytes()
    verts, tris = extract(hip, field, types, iso, lattice)  # a new extraction drops the measure
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER
    assert_equals_restatement(hip, verts, tris, lattice, "after two more steps")
    counts = np.zeros(2, np.int64)
    o, sp, d = (np.ascontiguousarray(lattice[0], np.float32), np.ascontiguousarray(lattice[1], np.float32), np.ascontiguousarray(lattice[2], np.int32))
    assert hip._L.sph_extract_surface(hip._h, o.ctypes.data, sp.ctypes.data, d.ctypes.data, 0, 1, 0.5, counts.ctypes.data) == ERR_INVALID
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER  # a failed extraction drops it too
    c4, e3 = np.zeros(4, np.int64), np.zeros(3, np.int32)
    assert hip._L.sph_measure_surface(hip._h, c4.ctypes.data, e3.ctypes.data) == ERR_ORDER  # and leaves no mesh to measure
    hip.close()


def test_error_table():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    c4, e3 = np.full(4, -7, np.int64), np.zeros(3, np.int32)
    assert hip._L.sph_measure_surface(hip._h, c4.ctypes.data, e3.ctypes.data) == ERR_ORDER  # before any extraction
    assert c4.tolist() == [0, 0, 0, 0]
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER
    with pytest.raises(sphmi.SphError):
        hip.measure_surface()
    hip.step(0)
    lattice = shell_cases.liquid_lattice(sc, 0.5)
    verts, tris = hip.extract_surface(*lattice)
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER  # extracted, not measured
    assert hip._L.sph_measure_surface(hip._h, None, e3.ctypes.data) == ERR_INVALID
    assert hip._L.sph_measure_surface(hip._h, c4.ctypes.data, None) == ERR_INVALID
    assert hip._L.sph_measure_surface(hip._h, c4.ctypes.data, e3.ctypes.data) == 0 and c4[0] >= 1
    assert hip._L.sph_read_shells(hip._h, None, None, None) == 0
    assert hip._L.sph_measure_surface(hip._h, None, None) == ERR_INVALID
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER  # a failed measure leaves none behind
    # each pointer of the reader alone
    assert hip.measure_surface()["shells"] == c4[0]
    vs, table, bb = hip.surface_shells()
    one = np.empty_like(table)
    assert hip._L.sph_read_shells(hip._h, None, one.ctypes.data, None) == 0 and np.array_equal(one, table)
    one = np.empty_like(bb)
    assert hip._L.sph_read_shells(hip._h, None, None, one.ctypes.data) == 0 and np.array_equal(bits(one), bits(bb))
    one = np.empty_like(vs)
    assert hip._L.sph_read_shells(hip._h, one.ctypes.data, None, None) == 0 and np.array_equal(one, vs)
    assert hip._L.sph_measure_surface(None, c4.ctypes.data, e3.ctypes.data) == ERR_INVALID
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    c4, e3 = np.zeros(4, np.int64), np.zeros(3, np.int32)
    assert hip._L.sph_measure_surface(hip._h, c4.ctypes.data, e3.ctypes.data) == ERR_INVALID
    assert hip._L.sph_read_shells(hip._h, None, None, None) == ERR_ORDER
    hip.close()


def test_measure_is_read_only():
    """Positions, velocities and densities equal an untouched twin's; the mesh bytes, the normals, a labelling and a particle
    render are the same after the measure as before it."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    lattice = shell_cases.liquid_lattice(sc, 0.5)
    cfg = sc["cfg"]
    view = frames.render_view((cfg.xmin, cfg.ymin, cfg.zmin), (cfg.xmax, cfg.ymax, cfg.zmax), width=96, height=64)
    for it in range(4):
        a.step(it)
        b.step(it)
        verts, tris = a.extract_surface(*lattice, iso=0.5, field="shepard", types=(1, 2))
        normals = a.surface_normals()
        a.label_components()
        labels, rc, cbb = a.components()
        drawn = a.render(view)
        image = a.rendered()
        m = a.measure_surface()
        assert m["shells"] >= 1
        a.surface_shells()
        v2 = np.empty_like(verts)
        t2 = np.empty_like(tris)
        a._chk(a._L.sph_read_surface(a._h, v2.ctypes.data, t2.ctypes.data))
        assert v2.tobytes() == verts.tobytes() and t2.tobytes() == tris.tobytes()
        assert a.surface_normals().tobytes() == normals.tobytes()
        l2, rc2, cbb2 = a.components()
        assert l2.tobytes() == labels.tobytes() and rc2.tobytes() == rc.tobytes() and cbb2.tobytes() == cbb.tobytes()
        a.component_diagnostics([0])  # the labelling is still current
        again = a.rendered()  # the images of the render before the measure, then a fresh render of the same state
        assert drawn[1] > 0 and all(again[k].tobytes() == image[k].tobytes() for k in image)
        assert a.render(view) == drawn
        again = a.rendered()
        assert all(again[k].tobytes() == image[k].tobytes() for k in image)
    assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer()))
    assert np.array_equal(bits(a.read_velocity_buffer()), bits(b.read_velocity_buffer()))
    assert np.array_equal(bits(a.read_density_buffer()), bits(b.read_density_buffer()))
    a.close()
    b.close()


def test_cpp_driver_shells(tmp_path):
    """sphmi_run --surface-shells: the CSV files equal measure_surface / surface_shells of a Python solver on the same scene after
    the same steps, and frames.write_shells_csv writes the same bytes."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    dims = (17, 15, 19)
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--surface-grid"]
                       + [str(d) for d in dims] + ["--surface-every", "2", "--surface-out", str(tmp_path), "--surface-shells"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "_measureSurface:" in r.stdout
    sc = scenes.SCENES["tiny"]()  # the same box
    cfg = sc["cfg"]
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
    spacing = (hi - lo) / np.float32(np.array(dims, np.float32) - np.float32(1))
    hip = scenes.hip_for(sc)
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            hip.extract_surface(lo, spacing, dims, iso=0.5, field="shepard", types=(1, 2))
            m, vs, table, bb = measured(hip)
            path = str(tmp_path / ("shells_%d.csv" % (it + 1)))
            got_t, got_b, got_e = frames.read_shells(path)
            assert np.array_equal(got_t, table) and np.array_equal(bits(got_b), bits(bb))
            assert got_e.tolist() == [m[k] for k in EXP_KEYS]
            assert table.shape[0] >= 1 and int(table[:, 2].sum()) > 100
            mine = str(tmp_path / "python.csv")
            frames.write_shells_csv(mine, table, bb, got_e)
            with open(mine, "rb") as f, open(path, "rb") as g:
                assert f.read() == g.read()
            os.remove(mine)
    hip.close()
    assert sorted(os.listdir(tmp_path)) == ["shells_2.csv", "shells_4.csv", "surface_2.ply", "surface_4.ply"]
    bad = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "1", "--surface-shells"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--surface-shells needs --surface-grid" in bad.stderr
