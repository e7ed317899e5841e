"""CPU checks of gradient sampling: the numpy restatement of the contract (tests/gradient_ref.py) against float64 sums and
against the flows whose gradients are known, and the output helpers of sphmi/frames.py (PLY normals, gradient VTK and raw
files). No GPU needed."""
import json
import os

import numpy as np
import pytest

import gradient_ref
import sample_ref
from sphmi import frames

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constants.json")


def _constants():
    c = json.load(open(GOLDEN))
    fb = {k: float(np.array(v, np.uint32).view(np.float32)) for k, v in c["float_bits"].items()}
    return fb["h"], fb["r0"], fb["mass"], fb["rho0"], fb["simulationScale"], fb["mass"] * c["Wpoly6Coefficient"]


def lattice_state(n=16, velocity=None, pressure=None):
    """An n^3 particle lattice at spacing r0 with rho = rho0 everywhere (the box constants), velocities and pressures given as
    functions of the physical (simulation-scaled) position."""
    h, r0, mass, rho0, sim, mw = _constants()
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = (ijk * np.float32(r0)).astype(np.float32)
    x = pos.astype(np.float64) * sim
    N = pos.shape[0]
    vel = np.zeros((N, 3), np.float32) if velocity is None else velocity(x).astype(np.float32)
    p = np.zeros(N, np.float32) if pressure is None else pressure(x).astype(np.float32)
    state = dict(pos=pos, vel=vel, rho=np.full(N, rho0, np.float32), p=p, types=np.ones(N, np.float32),
                 keys=np.zeros(N, np.uint32), G=1, h=h, simScale=sim, massWpoly6=mw)
    return state, (n - 1) * np.float32(r0)


def interior_points(state, side, count=400, seed=1):
    """Random points more than h inside the lattice's faces."""
    h = state["h"]
    return np.random.default_rng(seed).uniform(h + 0.5, side - h - 0.5, (count, 3)).astype(np.float32)


def gradient_f64(state, points, types=(1, 2, 3)):
    """Words 8..30 of the contract from float64 all-pairs sums (for small clouds)."""
    pos = np.asarray(state["pos"], np.float64)
    tsel = np.isin(np.asarray(state["types"]).astype(np.int32), list(types))
    h, sim = float(np.float32(state["h"])), float(np.float32(state["simScale"]))
    hs2, K = (h * sim) ** 2, -6.0 * float(state["massWpoly6"]) * sim
    out = np.zeros((len(points), 32))
    for i, q in enumerate(np.asarray(points, np.float64)):
        d = q[:3] - pos
        r2 = (d ** 2).sum(1)
        s = tsel & (r2 < h * h)
        g = (hs2 - r2[s] * sim * sim) ** 2
        inv = 1.0 / np.asarray(state["rho"], np.float64)[s]
        v, qq = g * (hs2 - r2[s] * sim * sim) * inv, g * inv
        ds = d[s]
        out[i, 8:11] = K * (g[:, None] * ds).sum(0)
        C = (qq[:, None] * ds).sum(0)
        out[i, 11:14] = K * C
        if v.sum() != 0:
            A = np.concatenate([np.asarray(state["vel"], np.float64)[s], np.asarray(state["p"], np.float64)[s, None]], 1)
            mean = (v[:, None] * A).sum(0) / v.sum()
            G = K * (np.einsum("k,ki,kc->ic", qq, A, ds) - mean[:, None] * C[None, :])
            out[i, 14:23] = G[:3].reshape(-1)
            out[i, 23:26] = G[3]
            g3 = G[:3]
            out[i, 26:29] = (g3[2, 1] - g3[1, 2], g3[0, 2] - g3[2, 0], g3[1, 0] - g3[0, 1])
            out[i, 29] = np.trace(g3)
            out[i, 30] = -0.5 * (g3 * g3.T).sum()
    return out


def test_restatement_matches_float64_sums():
    """Random cloud, random velocities / pressures / densities: every gradient word within 1e-4 of the float64 sums relative to
    that word's largest magnitude (the float32 sums have 20-40 terms; cancellation in E - U*C is the loosest part)."""
    rng = np.random.default_rng(3)
    n = 3000
    h, r0, mass, rho0, sim, mw = _constants()
    state = dict(pos=rng.uniform(0, 20, (n, 3)).astype(np.float32), vel=rng.normal(0, 1e-3, (n, 3)).astype(np.float32),
                 rho=rng.uniform(900, 1100, n).astype(np.float32), p=rng.normal(0, 50, n).astype(np.float32),
                 types=rng.choice(np.array([1.0, 2.1, 3.0], np.float32), n), keys=np.zeros(n, np.uint32), G=1, h=h,
                 simScale=sim, massWpoly6=mw)
    pts = rng.uniform(1, 19, (200, 3)).astype(np.float32)
    for types in ((1,), (1, 2, 3)):
        got = gradient_ref.gradient_reference(state, pts, types)
        want = gradient_f64(state, pts, types)
        assert np.array_equal(got[:, :8], sample_ref.sample_reference(state, pts, types))
        for col in range(8, 31):
            scale = np.abs(want[:, col]).max()
            assert scale > 0, col
            np.testing.assert_allclose(got[:, col], want[:, col], rtol=0, atol=1e-4 * scale, err_msg="word %d" % col)
        assert not got[:, 31].any()


def test_restatement_edge_records():
    state, side = lattice_state(n=8)
    pts = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1e4, 1e4, 1e4], [-50.0, 3.0, 3.0]], np.float32)
    got = gradient_ref.gradient_reference(state, pts)
    assert not got[:2].view(np.uint32).any()  # non-finite: all +0
    assert (got[2:] == 0).all()  # far: zero values, -0 in words 8..13 (K*0, K < 0)
    assert np.signbit(got[2:, 8:14]).all() and not np.signbit(got[2:, :8]).any() and not np.signbit(got[2:, 14:]).any()


def test_rigid_rotation():
    """u = Omega x x: vorticity 2 Omega, divergence 0, Q = |Omega|^2. On a lattice at spacing r0 = h/2 the plain SPH gradient
    (not renormalised) underestimates by about the Shepard sum (0.83 here): the restatement gives 0.79..0.90 x 2 Omega per
    component and Q = 0.65..0.80 |Omega|^2 at random interior points, so the bounds are 0.75..0.95 and 0.6..0.85; the divergence
    stays below 1.1e-4 |Omega| (bound 1e-3)."""
    Om = np.array([20.0, -30.0, 40.0])
    state, side = lattice_state(velocity=lambda x: np.cross(Om, x))
    g = gradient_ref.gradient_reference(state, interior_points(state, side), (1,))
    ratio = g[:, 26:29] / (2 * Om)
    assert ratio.min() > 0.75 and ratio.max() < 0.95, (ratio.min(), ratio.max())
    assert np.abs(g[:, 29]).max() < 1e-3 * np.linalg.norm(Om)
    q = g[:, 30] / (Om @ Om)
    assert q.min() > 0.6 and q.max() < 0.85, (q.min(), q.max())
    # grad u is the rotation tensor's: its symmetric part is small (the restatement: below 0.037 max|Omega|; bound 0.06)
    G = g[:, 14:23].reshape(-1, 3, 3)
    sym = 0.5 * (G + G.transpose(0, 2, 1))
    assert np.abs(sym).max() < 0.06 * np.abs(Om).max()


def test_linear_pressure():
    """p = a . x: grad p is a constant 0.72..0.93 a per component on the r0 lattice (bounds 0.65..0.97); the velocity
    gradients are exactly 0 (u = 0)."""
    a = np.array([1e6, -2e6, 3e6])
    state, side = lattice_state(pressure=lambda x: x @ a)
    g = gradient_ref.gradient_reference(state, interior_points(state, side), (1,))
    ratio = g[:, 23:26] / a
    assert ratio.min() > 0.65 and ratio.max() < 0.97, (ratio.min(), ratio.max())
    assert not g[:, 14:23].any() and not g[:, 26:31].any()


def test_density_gradient_uniform_block():
    """Inside a uniform block grad rho is below 0.1 rho0 / (h * simScale) (the restatement: 0.07); at the top face it points
    down into the liquid and is several times larger than anywhere inside."""
    state, side = lattice_state()
    h, sim = state["h"], state["simScale"]
    scale = 1000.0 / (h * sim)
    inner = gradient_ref.gradient_reference(state, interior_points(state, side), (1,))
    assert np.linalg.norm(inner[:, 8:11], axis=1).max() < 0.1 * scale
    rng = np.random.default_rng(5)
    top = np.concatenate([rng.uniform(h + 0.5, side - h - 0.5, (200, 2)), np.full((200, 1), side + 0.3 * h)], 1).astype(np.float32)
    face = gradient_ref.gradient_reference(state, top, (1,))
    gr = face[:, 8:11]
    assert (gr[:, 2] < 0).all()
    cosine = -gr[:, 2] / np.linalg.norm(gr, axis=1)
    assert cosine.min() > 0.95
    assert np.linalg.norm(gr, axis=1).min() > 3 * np.linalg.norm(inner[:, 8:11], axis=1).max()


def test_normals_reference():
    rec = np.zeros((5, 32), np.float32)
    rec[0, 11:14] = (3.0, 0.0, -4.0)     # field 1
    rec[1, 11:14] = (0.0, 0.0, 0.0)      # zero gradient -> 0
    rec[2, 11:14] = (np.inf, 1.0, 0.0)   # not finite -> 0
    rec[3, 11:14] = (1e-30, 0.0, 0.0)    # squares underflow: len 0 -> 0
    rec[4, 11:14] = (0.0, -2.0, 0.0)
    n = gradient_ref.normals_reference(rec, 1)
    assert np.array_equal(n, np.array([[-0.6, 0.0, 0.8], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0.0, 1.0, 0.0]], np.float32))
    rec2 = np.zeros((1, 32), np.float32)
    rec2[0, 23:26] = (0.0, 5.0, 0.0)
    assert np.array_equal(gradient_ref.normals_reference(rec2, 5), np.array([[0.0, -1.0, 0.0]], np.float32))


def _mesh():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    n = -v + np.float32(0.25)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return v, t, n.astype(np.float32)


def test_ply_with_normals_round_trip(tmp_path):
    v, t, n = _mesh()
    path = str(tmp_path / "n.ply")
    assert frames.write_ply(path, v, t, normals=n) == (4, 4)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    assert "property float nx\nproperty float ny\nproperty float nz\n" in head
    rv, rt = frames.read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rt, t)
    rv, rt, rn = frames.read_ply(path, with_normals=True)
    assert np.array_equal(rv, v) and np.array_equal(rt, t) and np.array_equal(rn.view(np.uint32), n.view(np.uint32))
    plain = str(tmp_path / "p.ply")
    frames.write_ply(plain, v, t)
    assert frames.read_ply(plain, with_normals=True)[2] is None
    with pytest.raises(ValueError):
        frames.write_ply(str(tmp_path / "bad.ply"), v, t, normals=n[:3])


def test_default_ply_is_byte_identical(tmp_path):
    """Without normals write_ply writes exactly what it wrote before normals existed."""
    v, t, _ = _mesh()
    path = str(tmp_path / "a.ply")
    frames.write_ply(path, v, t)
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              b"element face 4\nproperty list uchar int vertex_indices\nend_header\n")
    faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in t)
    assert open(path, "rb").read() == header + v.astype("<f4").tobytes() + faces
    frames.write_ply(str(tmp_path / "b.ply"), v, t, normals=None)
    assert open(str(tmp_path / "b.ply"), "rb").read() == open(path, "rb").read()


def test_vtk_gradients_and_raw_file(tmp_path):
    rng = np.random.default_rng(2)
    rec = rng.normal(0, 1, (3, 4, 5, 32)).astype(np.float32)
    path = str(tmp_path / "g.vtk")
    assert frames.write_vtk_gradients(path, (1.0, 2.0, 3.0), (0.5, 0.5, 0.25), rec) == 60
    data = open(path, "rb").read()
    assert data.startswith(b"# vtk DataFile Version 3.0\nsphmi gradients\nBINARY\nDATASET STRUCTURED_POINTS\n"
                           b"DIMENSIONS 5 4 3\nORIGIN 1 2 3\nSPACING 0.5 0.5 0.25\nPOINT_DATA 60\nVECTORS vorticity float\n")
    at = data.index(b"VECTORS vorticity float\n") + len(b"VECTORS vorticity float\n")
    assert np.array_equal(np.frombuffer(data, ">f4", 180, at), rec[..., 26:29].reshape(-1))
    for name in (b"VECTORS density_gradient float\n", b"SCALARS divergence float 1\nLOOKUP_TABLE default\n",
                 b"SCALARS q_criterion float 1\nLOOKUP_TABLE default\n"):
        assert name in data
    at = data.index(b"SCALARS q_criterion float 1\nLOOKUP_TABLE default\n") + len(b"SCALARS q_criterion float 1\nLOOKUP_TABLE default\n")
    assert np.array_equal(np.frombuffer(data, ">f4", 60, at), rec[..., 30].reshape(-1))
    with pytest.raises(ValueError):
        frames.write_vtk_gradients(path, (0, 0, 0), (1, 1, 1), rec[..., :8])
    raw = str(tmp_path / "gradients_4.bin")
    rec.tofile(raw)
    assert np.array_equal(frames.read_gradients(raw, (5, 4, 3)), rec)


def test_gradient_field_names():
    F = frames.GRADIENT_FIELDS
    assert len(F) == gradient_ref.WORDS == 32 and len(set(F)) == 32
    assert F[:7] == frames.GRID_FIELDS
    assert (F.index("drho_dx"), F.index("dshepard_dx"), F.index("dvx_dx"), F.index("dvz_dz"), F.index("dp_dx")) == (8, 11, 14, 22, 23)
    assert (F.index("vorticity_x"), F.index("divergence"), F.index("q_criterion")) == (26, 29, 30)
