"""CPU checks of isosurface extraction: the generated marching-cubes table (tools/gen_mc_table.py, csrc/sph_mc_table.h), the numpy
restatement of the contract (tests/surface_ref.py) on analytic and random lattices, and the PLY helpers of sphmi/frames.py.
No GPU needed."""
import os
import sys

import numpy as np

import surface_ref
from sphmi import frames

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table  # noqa: E402


def test_table_check_values():
    T = gen_mc_table.TABLE
    assert sum(len(t) for t in T) == 820
    assert max(len(t) for t in T) == gen_mc_table.MAX_TRIS == 5
    assert [c for c in range(256) if not T[c]] == [0, 255]
    assert max(len(cyc) for c in range(256) for cyc in gen_mc_table.cycles(c)) == 7
    # every crossed edge of a case is used, and only those
    for c in range(256):
        crossed = {e for e, (a, b) in enumerate(gen_mc_table.EDGES) if ((c >> a) ^ (c >> b)) & 1}
        assert {e for t in T[c] for e in t} == crossed
    # the single-corner case: one triangle around corner 0, normal away from it
    assert T[1] == [(0, 4, 8)]


def test_committed_header_equals_generator_output():
    with open(gen_mc_table.HEADER) as f:
        assert f.read() == gen_mc_table.render(), "run tools/gen_mc_table.py"


def _lattice(n=20):
    g = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return x - 9.5, y - 9.5, z - 9.5


def _mesh_checks(f, expect_v, expect_t, expect_chi, volume):
    verts, tris = surface_ref.surface_reference(f.astype(np.float32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0)
    assert (verts.shape[0], tris.shape[0]) == (expect_v, expect_t)
    assert surface_ref.directed_edge_report(tris, verts.shape[0]) is None
    assert surface_ref.euler_characteristic(verts, tris) == expect_chi
    vol = surface_ref.signed_volume(verts, tris)
    assert vol > 0 and abs(vol - volume) < 0.05 * volume


def test_sphere_check_values():
    x, y, z = _lattice()
    _mesh_checks(6.0 - np.sqrt(x * x + y * y + z * z), 672, 1340, 2, 4.0 / 3.0 * np.pi * 6.0 ** 3)


def test_torus_check_values():
    x, y, z = _lattice()
    f = 2.5 - np.sqrt((np.sqrt(x * x + y * y) - 6.0) ** 2 + z * z)
    _mesh_checks(f, 728, 1456, 0, 2.0 * np.pi ** 2 * 6.0 * 2.5 ** 2)


def _loop_reference(f, origin, spacing, iso):
    """The contract read literally, one cell and one edge at a time (tiny lattices only): checks the vectorised numbering."""
    f = np.asarray(f, np.float32)
    nz, ny, nx = f.shape
    iso = np.float32(iso)
    ins = f >= iso
    coord = [np.float32(origin[a]) + np.arange((nx, ny, nz)[a], dtype=np.float32) * np.float32(spacing[a]) for a in range(3)]
    ids, verts = {}, []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for a in range(3):
                    q = [i, j, k]
                    q[a] += 1
                    if q[0] >= nx or q[1] >= ny or q[2] >= nz or ins[k, j, i] == ins[q[2], q[1], q[0]]:
                        continue
                    f0, f1 = f[k, j, i], f[q[2], q[1], q[0]]
                    t = (iso - f0) / (f1 - f0)
                    p = [coord[0][i], coord[1][j], coord[2][k]]
                    x0, x1 = coord[a][(i, j, k)[a]], coord[a][q[a]]
                    p[a] = x0 + t * (x1 - x0)
                    ids[(i, j, k, a)] = len(verts)
                    verts.append(p)
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                case = sum(int(ins[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)]) << c for c in range(8))
                for t in gen_mc_table.TABLE[case]:
                    tri = []
                    for e in t:
                        dx, dy, dz = gen_mc_table.CORNERS[gen_mc_table.EDGES[e][0]]
                        tri.append(ids[(i + dx, j + dy, k + dz, e // 4)])
                    tris.append(tri)
    return np.array(verts, np.float32).reshape(-1, 3), np.array(tris, np.int32).reshape(-1, 3)


def _random_lattice(rng):
    dims = rng.integers(4, 8, 3)
    f = rng.uniform(-1.0, 1.0, (dims[2], dims[1], dims[0])).astype(np.float32)
    f[rng.random(f.shape) < 0.05] = 0.0  # on the iso value: t = 0, coincident vertices
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1.0, -1.0, -1.0, -1.0, -1.0, -1.0
    return f


def test_restatement_equals_the_contract_read_literally():
    rng = np.random.default_rng(3)
    for _ in range(40):
        f = _random_lattice(rng)
        f[rng.random(f.shape) < 0.1] = np.nan  # NaN: outside
        origin = rng.uniform(-5, 5, 3).astype(np.float32)
        spacing = rng.uniform(0.1, 2.0, 3).astype(np.float32)
        v, t = surface_ref.surface_reference(f, origin, spacing, 0.0)
        lv, lt = _loop_reference(f, origin, spacing, 0.0)
        assert np.array_equal(v.view(np.uint32), lv.view(np.uint32))
        assert np.array_equal(t, lt)


def _ambiguous_faces(case):
    """(face, diagonal) pairs of `case` whose face has four crossed edges."""
    out = []
    for fi, (ring, _) in enumerate(gen_mc_table.FACES):
        bits = [(case >> c) & 1 for c in ring]
        if bits in ([1, 0, 1, 0], [0, 1, 0, 1]):
            out.append((fi, bits[0]))
    return out


def test_random_lattices_give_closed_oriented_meshes():
    rng = np.random.default_rng(12)
    cases, ambiguous = set(), set()
    for n in range(3000):
        f = _random_lattice(rng)
        iso = 0.0
        verts, tris = surface_ref.surface_reference(f, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), iso)
        report = surface_ref.directed_edge_report(tris, verts.shape[0])
        assert report is None, "lattice %d: %s" % (n, report)
        ins = (f >= iso).astype(np.int64)
        nz, ny, nx = f.shape
        case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
        for c, (dx, dy, dz) in enumerate(gen_mc_table.CORNERS):
            case |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] << c
        cases.update(np.unique(case).tolist())
    for c in cases:
        ambiguous.update(_ambiguous_faces(c))
    assert len(cases) == 256
    assert ambiguous == {(fi, d) for fi in range(6) for d in (0, 1)}


def test_three_point_axes_and_empty_meshes():
    f = np.full((3, 3, 3), -1.0, np.float32)
    f[1, 1, 1] = 1.0
    verts, tris = surface_ref.surface_reference(f, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0)
    assert (verts.shape[0], tris.shape[0]) == (6, 8)  # an octahedron
    assert surface_ref.directed_edge_report(tris, 6) is None
    assert surface_ref.signed_volume(verts, tris) > 0
    verts, tris = surface_ref.surface_reference(f, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2.0)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)


def test_ply_round_trip(tmp_path):
    x, y, z = _lattice()
    verts, tris = surface_ref.surface_reference((6.0 - np.sqrt(x * x + y * y + z * z)).astype(np.float32), (1.5, -2.0, 0.25),
                                                (0.5, 0.5, 0.75), 0.0)
    path = str(tmp_path / "sphere.ply")
    assert frames.write_ply(path, verts, tris) == (verts.shape[0], tris.shape[0])
    v, t = frames.read_ply(path)
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(t, tris)
    with open(path, "rb") as f:
        head = f.read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % verts.shape[0])
    empty = str(tmp_path / "empty.ply")
    frames.write_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, t = frames.read_ply(empty)
    assert v.shape == (0, 3) and t.shape == (0, 3)
