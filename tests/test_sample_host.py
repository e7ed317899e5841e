"""CPU checks of field sampling: the numpy restatement of the contract (tests/sample_ref.py) and the grid output helpers of
sphmi/frames.py. No GPU needed."""
import numpy as np
import pytest

import sample_ref
from sphmi import frames


def _cloud(seed=7, n=4000, L=20.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, L, (n, 3)).astype(np.float32)
    vel = rng.normal(0, 1, (n, 3)).astype(np.float32)
    rho = rng.uniform(900, 1100, n).astype(np.float32)
    p = rng.normal(0, 50, n).astype(np.float32)
    types = rng.choice(np.array([1.0, 2.1, 3.0], np.float32), n)
    h, sim = 3.34, 0.0037
    state = dict(pos=pos, vel=vel, rho=rho, p=p, types=types, keys=np.zeros(n, np.uint32), G=1, h=h, simScale=sim,
                 massWpoly6=3.25e-14 * 1.5e9)
    return state, rng


@pytest.mark.parametrize("types", [(1,), (1, 2), (1, 2, 3)])
def test_restatement_matches_float64_brute_force(types):
    state, rng = _cloud()
    pts = rng.uniform(-2, 22, (300, 3)).astype(np.float32)
    got = sample_ref.sample_reference(state, pts, types)
    want = sample_ref.brute_force_f64(state["pos"], state["vel"], state["rho"], state["p"], state["types"], pts,
                                      float(np.float32(state["h"])), float(np.float32(state["simScale"])),
                                      float(np.float32(state["massWpoly6"])), types)
    assert (got[:, 6] == want[:, 6]).mean() > 0.99  # counts: equal except for points within rounding of the radius
    assert got[:, 6].max() > 5
    for col in (0, 1, 2, 3, 4, 5):
        scale = np.abs(want[:, col]).max()
        np.testing.assert_allclose(got[:, col], want[:, col], rtol=1e-5, atol=1e-5 * scale)
    assert np.all(got[:, 7] == 0)


def test_restatement_edge_records():
    state, _ = _cloud(n=500)
    far = np.array([[1e4, 1e4, 1e4], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0]], np.float32)
    got = sample_ref.sample_reference(state, far)
    assert np.array_equal(got.view(np.uint32), np.zeros_like(got).view(np.uint32))


def test_restatement_excludes_keys_outside_the_cell_table():
    state, rng = _cloud(n=800)
    pts = rng.uniform(2, 18, (50, 3)).astype(np.float32)
    base = sample_ref.sample_reference(state, pts)
    state["keys"] = np.where(np.arange(800) % 2 == 0, 0, 5).astype(np.uint32)  # G = 1: odd particles are outside the table
    half = sample_ref.sample_reference(state, pts)
    assert (half[:, 6] < base[:, 6]).any() and (half[:, 6] <= base[:, 6]).all()


def test_grid_points_layout():
    g = sample_ref.grid_points((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (3, 2, 4))
    assert g.shape == (4, 2, 3, 3)
    assert g[3, 1, 2].tolist() == [np.float32(1.0) + np.float32(2) * np.float32(0.5), 2.25, 9.0]


def _parse_vtk(path):
    data = open(path, "rb").read()
    header = {}
    pos = 0
    lines = []
    for _ in range(8):
        end = data.index(b"\n", pos)
        lines.append(data[pos:end].decode())
        pos = end + 1
    assert lines[0] == "# vtk DataFile Version 3.0" and lines[2] == "BINARY" and lines[3] == "DATASET STRUCTURED_POINTS"
    header["dims"] = [int(v) for v in lines[4].split()[1:]]
    header["origin"] = [float(v) for v in lines[5].split()[1:]]
    header["spacing"] = [float(v) for v in lines[6].split()[1:]]
    n = int(lines[7].split()[1])
    arrays = {}
    while pos < len(data):
        end = data.index(b"\n", pos)
        line = data[pos:end].decode()
        pos = end + 1
        kind, name = line.split()[:2]
        comps = 1
        if kind == "SCALARS":
            end = data.index(b"\n", pos)
            assert data[pos:end] == b"LOOKUP_TABLE default"
            pos = end + 1
        else:
            assert kind == "VECTORS"
            comps = 3
        nbytes = 4 * n * comps
        arrays[name] = np.frombuffer(data[pos:pos + nbytes], ">f4").reshape(n, comps) if comps > 1 else np.frombuffer(
            data[pos:pos + nbytes], ">f4")
        pos += nbytes
        assert data[pos:pos + 1] == b"\n"
        pos += 1
    return header, n, arrays


def test_write_vtk_grid_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    g = rng.normal(0, 1, (5, 3, 4, 8)).astype(np.float32)
    path = str(tmp_path / "fields.vtk")
    n = frames.write_vtk_grid(path, (0.5, -1.25, 2.0), (0.1, 0.2, 0.3), g)
    assert n == 60
    header, npts, arrays = _parse_vtk(path)
    assert header["dims"] == [4, 3, 5]
    assert header["origin"] == [0.5, -1.25, 2.0]
    assert np.array_equal(np.float32(header["spacing"]), np.float32([0.1, 0.2, 0.3]))  # float32 values round-trip
    assert npts == 60
    assert sorted(arrays) == ["density", "pressure", "shepard", "velocity"]
    assert np.array_equal(arrays["density"].astype(np.float32), g[..., 0].ravel())
    assert np.array_equal(arrays["shepard"].astype(np.float32), g[..., 1].ravel())
    assert np.array_equal(arrays["pressure"].astype(np.float32), g[..., 5].ravel())
    assert np.array_equal(arrays["velocity"].astype(np.float32), g[..., 2:5].reshape(-1, 3))


def test_free_surface_height_on_a_half_filled_grid():
    nz, ny, nx = 11, 3, 4
    origin, spacing = (0.0, 0.0, 10.0), (1.0, 1.0, 0.5)
    g = np.zeros((nz, ny, nx, 8), np.float32)
    z = 10.0 + 0.5 * np.arange(nz)
    level = np.array([[12.1, 12.3, 12.6, 13.0], [11.2, 12.0, 13.7, 14.9], [10.0, 10.25, 15.3, 9.0]])  # surface per column
    # shepard falls linearly from 1 to 0 over two plane spacings around the level: exactly 0.5 at `level`, and the two planes
    # that bracket it are unclipped, so the linear interpolation between them is exact
    s = np.clip(0.5 + (level[None] - z[:, None, None]), 0.0, 1.0)
    s[0, 1, 1] = 0.7  # a lower crossing that is not the highest one must not matter
    s[1, 1, 1] = 0.2
    g[..., 1] = s
    got = frames.free_surface_height(g, origin, spacing)
    want = level.copy()
    want[2, 2] = 15.0  # top plane still >= 0.5: the top of the grid
    want[2, 3] = np.nan  # never reaches 0.5
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert np.isnan(got[2, 3])
