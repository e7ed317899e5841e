"""CPU checks of the diagnostics contract's numpy restatement (tests/diag_ref.py) on synthetic states: the fixed reduction tree
against math.fsum, flows whose sums are known, the selection and histogram edge rules, and the CSV helpers of sphmi/frames.py.
No GPU and no solver needed."""
import math

import numpy as np
import pytest

import diag_ref
from sphmi import frames

f32 = np.float32
RHO0 = f32(1000.0)


def make_state(pos, vel=None, rho=None, p=None, types=None, keys=None, G=1000):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n = pos.shape[0]
    return dict(pos=pos, vel=np.zeros((n, 3), np.float32) if vel is None else np.asarray(vel, np.float32).reshape(n, 3),
                rho=np.full(n, RHO0, np.float32) if rho is None else np.asarray(rho, np.float32),
                p=np.zeros(n, np.float32) if p is None else np.asarray(p, np.float32),
                types=np.ones(n, np.float32) if types is None else np.asarray(types, np.float32),
                keys=np.zeros(n, np.uint32) if keys is None else np.asarray(keys, np.uint32), G=G,
                ids=np.arange(n, dtype=np.int64)[::-1].copy())


def lattice(n=12, spacing=1.67):
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (ijk.astype(np.float32) * f32(spacing) + f32(3.0)).astype(np.float32)


# ---- the tree ----
@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 2813, 1000003])
def test_tree_sum_is_within_the_pairwise_bound_of_fsum(n):
    """|S - fsum| <= 30 * 2^-53 * sum|t|: three levels of ten rounds each, the standard pairwise-summation bound (derived, not
    measured). The terms are widened float32 values of mixed sign and magnitude, as the kernel's are."""
    rng = np.random.default_rng(n)
    t = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 4, n)).astype(np.float32).astype(np.float64)
    s = diag_ref.tree_sum(t)
    exact = math.fsum(t.tolist())
    err, bound = abs(s - exact), 30 * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
    print("n %d: |S - fsum| = %.3e, bound %.3e" % (n, err, bound))
    assert err <= bound
    for extra in (1, 1023, 1024, 5000):  # trailing zero terms never change the result
        assert diag_ref.tree_sum(np.concatenate([t, np.zeros(extra)])) == s


def test_tree_sum_shape():
    """The pairing is the contract's: a[i] + a[i + stride], stride 512 first; a different shape gives different bits here."""
    t = np.zeros(1024)
    t[0], t[512], t[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    # stride 512 adds t[512] to t[0] first (rounds away), later t[1] too: 1.0; a sequential sum gives the same, but pairing
    # (t[1] + t[512]) first would give 1 + 2^-52
    assert diag_ref.tree_sum(t) == 1.0
    t = np.zeros(1024)
    t[0], t[1], t[513] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert diag_ref.tree_sum(t) == 1.0 + 2.0 ** -52  # (t[1] + t[513]) meet at stride 512, then reach t[0] at stride 1
    assert diag_ref.tree_sum([]) == 0.0
    assert diag_ref.tree_sum(np.arange(3000.0)) == 2999 * 3000 / 2
    # two levels: chunk results are combined by the same tree
    big = np.ones(1024 * 1024 + 7)
    assert diag_ref.tree_sum(big) == big.size


# ---- known flows ----
def test_uniform_translation():
    pos = lattice()
    n = pos.shape[0]
    v = np.array([0.25, -1.5, 3.0], np.float32)  # exactly representable
    st = make_state(pos, vel=np.tile(v, (n, 1)))
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    assert r[0] == n
    assert np.array_equal(r[4:7], n * v.astype(np.float64))
    sx = r[1:4]
    assert np.allclose(sx, pos.astype(np.float64).sum(0), rtol=1e-15)
    assert np.allclose(r[7:10], np.cross(sx, v.astype(np.float64)), rtol=1e-5, atol=1e-3 * np.abs(sx).max())
    assert r[10] == n * float(f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
    assert r[20] == float(f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) and r[21] == 0 and r[22] == st["ids"][0]


def test_rigid_rotation_about_z_through_the_centroid():
    pos = lattice(11)
    c = pos.astype(np.float64).mean(0)
    omega = 0.75
    d = pos.astype(np.float64) - c
    vel = np.stack([-omega * d[:, 1], omega * d[:, 0], np.zeros(len(d))], 1).astype(np.float32)
    # angular momentum about the ORIGIN of a rotation about the centroid: sum x × v = omega * sum (dx² + dy²) for the z component
    # when sum v = 0
    st = make_state(pos, vel=vel)
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    scale = np.abs(vel).max() * len(d)
    assert abs(r[4]) < 1e-6 * scale and abs(r[5]) < 1e-6 * scale and r[6] == 0
    want = omega * (d[:, 0] ** 2 + d[:, 1] ** 2).sum()
    assert abs(r[9] - want) < 1e-5 * want
    assert abs(r[10] - omega ** 2 * (d[:, 0] ** 2 + d[:, 1] ** 2).sum()) < 1e-5 * r[10]


def test_lattice_at_rest_density():
    st = make_state(lattice(9))
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    n = st["pos"].shape[0]
    assert r[12] == 0.0 and r[16] == r[17] == float(RHO0) and r[11] == n * float(RHO0)
    assert r[10] == 0 and r[20] == 0 and r[21] == 0  # all at rest: the lowest index attains the maximum
    s = frames.diagnostics_summary(r, type("Cfg", (), dict(mass=0.5, rho0=float(RHO0))))
    assert s["n"] == n and s["mass"] == 0.5 * n and s["kinetic_energy"] == 0 and s["rms_density_error"] == 0
    assert s["max_density_error"] == 0 and s["mean_density"] == float(RHO0)
    assert np.allclose(s["centre_of_mass"], st["pos"].astype(np.float64).mean(0))
    assert s["bbox_min"] == tuple(st["pos"].min(0).astype(np.float64)) and s["bbox_max"] == tuple(st["pos"].max(0).astype(np.float64))


# ---- selection, extremes ----
def test_region_edges_types_and_keys():
    pos = np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1], [2.5, 1, 1], [2.5, 1, 1], [2.5, 1, 1]], np.float32)
    st = make_state(pos, types=[1, 1, 1, 2.1, 3, 1], keys=[0, 0, 0, 0, 0, 1000], G=1000)
    region = (1, 0, 0, 3, 2, 2)
    sel = diag_ref.selected(st, region, (1,))
    assert sel.tolist() == [True, True, False, False, False, False]  # on x0: in; on x1: out; key outside the table: out
    assert diag_ref.selected(st, region, (1, 2)).tolist() == [True, True, False, True, False, False]
    assert diag_ref.selected(st, region, (3,)).tolist() == [False, False, False, False, True, False]
    assert diag_ref.selected(st, (-np.inf, 0, -np.inf, np.inf, 2, np.inf), (1, 2, 3)).sum() == 5
    r = diag_ref.record(st, region, (1,), RHO0)
    assert r[0] == 2 and r[1] == 3 and r[23] == 1 and r[26] == 2


def test_empty_region_record():
    st = make_state(lattice(4))
    r = diag_ref.record(st, (100, 100, 100, 200, 200, 200), (1,), RHO0)
    want = np.zeros(32)
    want[21] = want[22] = -1
    assert np.array_equal(r, want) and not np.signbit(r[:21]).any()
    r = diag_ref.record(st, (5, 5, 5, 5, 9, 9), (1,), RHO0)  # x0 == x1
    assert np.array_equal(r, want)


def test_negative_zero_is_canonicalised():
    pos = np.array([[-0.0, 1, 2], [-0.0, 1, 2]], np.float32)
    st = make_state(pos, vel=[[-0.0, 0, 0]] * 2, p=[-0.0, -0.0])
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    for w in (18, 19, 20, 23, 26):
        assert r[w] == 0 and not np.signbit(r[w]), w
    assert not np.signbit(r[1]) and not np.signbit(r[4])  # the padding zeros are +0.0


def test_max_v2_takes_the_lowest_index():
    vel = np.zeros((3000, 3), np.float32)
    vel[[2500, 700, 1900], 0] = 2.0
    st = make_state(np.ones((3000, 3), np.float32), vel=vel)
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    assert r[20] == 4.0 and r[21] == 700 and r[22] == st["ids"][700]


# ---- histogram ----
def test_histogram_edges():
    lo, hi, bins = f32(0.0), f32(1.0), 10
    below = np.nextafter(lo, f32(-1))
    top = np.nextafter(hi, f32(0))
    h = diag_ref.histogram_of(np.array([below, lo, top, hi, 0.55], np.float32), lo, hi, bins)
    assert h[0] == 1 and h[1] == 1 and h[bins + 1] == 1  # q < lo; q == lo in bin 0; q == hi at-or-above
    assert h[bins] == 1 and h[6] == 1 and h.sum() == 5
    # the clamp: (q - lo) * scale rounds up to `bins` for the largest float below hi
    lo, hi, bins = f32(0.0), f32(3.0), 3
    q = np.nextafter(hi, f32(0))
    scale = f32(bins) / (hi - lo)
    assert int(f32((q - lo) * scale)) == 2
    # q - lo rounds up to hi - lo for a value just below hi, so the product is exactly `bins`: the clamp keeps it in the last bin
    lo, hi, q = f32(-1000.0), f32(0.0), f32(-1e-10)
    assert lo <= q < hi
    for bins in (1, 2, 10, 33, 100):
        assert int(f32(f32(q - lo) * (f32(bins) / (hi - lo)))) == bins
        h = diag_ref.histogram_of(np.array([q], np.float32), lo, hi, bins)
        assert h[bins] == 1 and h[bins + 1] == 0 and h.sum() == 1


def test_histogram_selection_and_neighbour_counts():
    pos = lattice(5)
    n = pos.shape[0]
    counts = (np.arange(n) % 33).astype(np.float32)
    st = make_state(pos, types=np.where(np.arange(n) % 2 == 0, 1.0, 3.0))
    h = diag_ref.histogram(st, "neighbors", 0, 33, 33, None, (1,), counts)
    assert h[0] == 0 and h[-1] == 0 and h.sum() == (n + 1) // 2
    assert np.array_equal(h[1:-1], np.bincount(counts[::2].astype(int), minlength=33))
    r = diag_ref.record(st, diag_ref.EVERYTHING, (1,), RHO0)
    assert h.sum() == r[0]


# ---- CSV ----
def test_csv_round_trip_is_bit_exact(tmp_path):
    rng = np.random.default_rng(5)
    rec = rng.standard_normal((4, 3, 32)) * 10.0 ** rng.uniform(-300, 300, (4, 3, 32))
    rec[0, 0, :6] = [0.0, -0.0, np.inf, -np.inf, 5e-324, 1.7976931348623157e308]
    rec[1, 2, 21:23] = -1
    steps = [10, 20, 30, 45]
    path = str(tmp_path / "d.csv")
    frames.write_diagnostics_csv(path, steps, rec)
    s, got = frames.read_diagnostics_csv(path)
    assert s.tolist() == steps and got.shape == rec.shape
    assert np.array_equal(got.view(np.uint64), rec.view(np.uint64))
    frames.write_diagnostics_csv(path, steps[:2], rec[:2, 0])  # [S, 32]: one region
    s, got = frames.read_diagnostics_csv(path)
    assert got.shape == (2, 1, 32) and np.array_equal(got[:, 0].view(np.uint64), rec[:2, 0].view(np.uint64))
    assert len(frames.DIAG_FIELDS) == 32 and frames.DIAG_FIELDS[22] == "max_v2_id"
