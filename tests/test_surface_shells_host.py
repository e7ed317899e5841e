"""CPU checks of the surface measures: the numpy restatement (tests/shell_ref.py) against closed forms, against the derived
quantisation bound, against the helpers of tests/surface_ref.py and against the directed-side definition of an open side; that
the scenes of tests/shell_cases.py give the device something to compare; and the summary / CSV helpers of sphmi/frames.py.
No GPU needed."""
import math
import os

import numpy as np
import pytest

import render_mesh_cases
import scenes
import shell_cases
import shell_ref
import sphmi
import surface_ref
from sphmi import frames

f32 = np.float32
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _l1(c, n=16):
    g = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.abs(x - f32(c[0])) + np.abs(y - f32(c[1])) + np.abs(z - f32(c[2]))


def _measure(f, origin=ZERO, spacing=ONE, iso=0.0):
    f = np.asarray(f, np.float32)
    dims = f.shape[::-1]
    v, t = surface_ref.surface_reference(f, origin, spacing, iso)
    return v, t, shell_ref.measure(v, t, origin, spacing, dims)


def _shell_terms(v, t, m, origin=ZERO):
    """Per shell: the double terms of its triangles [T_s, 5]."""
    terms = shell_ref.triangle_terms(v, t, origin)
    ts = m["vertexShell"][t[:, 0]]
    return [terms[ts == s] for s in range(m["table"].shape[0])]


def _assert_quantisation_bound(v, t, m, origin=ZERO):
    """|ldexp(sum, -k) - fsum(terms)| <= T_s * 2^(-k-1): every term is rounded once to a multiple of 2^-k, so it moves by at most
    half of that, and the integer sum adds no further error."""
    vals = shell_ref.values(m["table"], m["exps"])
    ks = [m["exps"][0], m["exps"][1], m["exps"][2], m["exps"][2], m["exps"][2]]
    for s, terms in enumerate(_shell_terms(v, t, m, origin)):
        Ts = terms.shape[0]
        assert Ts == m["table"][s, 2]
        for w in range(5):
            exact = math.fsum(terms[:, w].tolist())
            assert abs(vals[s, w] - exact) <= Ts * math.ldexp(1.0, -int(ks[w]) - 1), (s, w, vals[s, w], exact)


def _chi(table):
    return table[:, 1] - (3 * table[:, 2] + table[:, 3]) // 2 + table[:, 2]


# ---- closed forms: marching cubes is exact on a field that is linear in every cell, so an L1 ball centred on a lattice point
# ---- with a half-integer radius gives exact numbers
def test_octahedron_closed_form():
    v, t, m = _measure(f32(5.5) - _l1((8, 8, 8)))
    assert (v.shape[0], t.shape[0]) == (366, 728)
    assert m["counts"].tolist() == [1, 1, 0, 0]
    assert m["table"][0, :5].tolist() == [0, 366, 728, 0, 0]
    assert _chi(m["table"]).tolist() == [2]
    a2, d6 = shell_ref.values(m["table"], m["exps"])[0, :2]
    kA, kV = int(m["exps"][0]), int(m["exps"][1])
    # the d6 terms are exact in double (half-integer coordinates); each a2 term carries one rounding of sqrt (2^-53 relative)
    assert abs(d6 / 6 - 4 * 5.5 ** 3 / 3) <= 728 * math.ldexp(1.0, -kV - 1) / 6
    area = 4 * math.sqrt(3) * 5.5 ** 2
    assert abs(a2 / 2 - area) <= 728 * math.ldexp(1.0, -kA - 1) / 2 + area * math.ldexp(1.0, -52)
    assert np.array_equal(m["bbox"][0], np.array([2.5, 2.5, 2.5, 13.5, 13.5, 13.5], np.float32))
    s = frames.shell_summary(m["table"], m["exps"], ZERO)
    assert np.allclose(s["centroid"][0], (8, 8, 8), atol=1e-9) and s["genus"].tolist() == [0] and s["kind"].tolist() == [0]
    _assert_quantisation_bound(v, t, m)


def test_shell_with_cavity_and_a_second_drop():
    d = _l1((7, 7, 7))
    f = np.maximum(np.minimum(f32(6.5) - d, d - f32(2.5)), f32(1.5) - _l1((13, 13, 13)))
    v, t, m = _measure(f)
    tab = m["table"]
    assert m["counts"].tolist() == [3, 3, 0, 0]
    assert tab[:, 0].tolist() == [0, 84, 567]
    assert tab[:, 1].tolist() == [510, 78, 30]
    assert tab[:, 2].tolist() == [1016, 152, 56]
    assert _chi(tab).tolist() == [2, 2, 2]
    vol = shell_ref.values(tab, m["exps"])[:, 1] / 6
    kV = int(m["exps"][1])
    for s, exact in enumerate((4 * 6.5 ** 3 / 3, -4 * 2.5 ** 3 / 3, 4 * 1.5 ** 3 / 3)):
        assert abs(vol[s] - exact) <= tab[s, 2] * math.ldexp(1.0, -kV - 1) / 6, (s, vol[s], exact)
    assert vol[1] < 0  # the cavity
    summary = frames.shell_summary(tab, m["exps"], ZERO)
    assert [frames.SHELL_KINDS[k] for k in summary["kind"]] == ["drop", "cavity", "drop"]
    assert abs(summary["totals"]["volume"] - (4 * 6.5 ** 3 / 3 - 4 * 2.5 ** 3 / 3 + 4.5)) <= 1224 * math.ldexp(1.0, -kV - 1) / 6
    assert np.array_equal(m["vertexShell"][[0, 84, 567]], [0, 1, 2])
    _assert_quantisation_bound(v, t, m)


def test_octahedron_cut_by_the_lattice():
    v, t, m = _measure(f32(9.5) - _l1((8, 8, 8)))
    assert m["counts"].tolist() == [1, 0, 96, 0]
    assert m["table"][0, 3] == 96
    assert shell_ref.open_sides(t).shape[0] == 96 and int(shell_ref.open_vertices_by_sum(t, v.shape[0]).sum()) == 96
    assert frames.shell_summary(m["table"], m["exps"], ZERO)["kind"].tolist() == [2]
    _assert_quantisation_bound(v, t, m)


# ---- quantisation
def _random_lattice(rng, lo=4, hi=8, border=True):
    dims = rng.integers(lo, hi, 3)
    f = rng.uniform(-1.0, 1.0, (dims[2], dims[1], dims[0])).astype(np.float32)
    f[rng.random(f.shape) < 0.05] = 0.0  # on the iso value: t = 0, coincident vertices
    if border:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1.0, -1.0, -1.0, -1.0, -1.0, -1.0
    return f


def test_quantisation_bound_volume_and_euler_characteristic_on_random_lattices():
    rng = np.random.default_rng(7)
    u = math.ldexp(1.0, -53)
    for n in range(60):
        f = _random_lattice(rng, border=n % 2 == 0)
        origin = rng.uniform(-50, 50, 3).astype(np.float32)
        spacing = rng.uniform(0.05, 3.0, 3).astype(np.float32)
        v, t, m = _measure(f, origin, spacing)
        if t.shape[0] == 0:
            continue
        assert m["counts"][3] == 0
        _assert_quantisation_bound(v, t, m, origin)
        assert int(_chi(m["table"]).sum()) == surface_ref.euler_characteristic(v, t)
        assert int(m["table"][:, 1].sum()) == v.shape[0] and int(m["table"][:, 2].sum()) == t.shape[0]
        if m["counts"][2] == 0:
            # The whole-mesh volume against the helper on the shifted vertices. The helper forms v0 . (v1 x v2), the contract
            # p0 . ((p1 - p0) x (p2 - p0)): equal as real numbers, each evaluated with under 16 roundings of quantities bounded by
            # |p0| |p1| |p2| (component sums), and the helper adds its T terms in double: (T + 16) u sum |p0| |p1| |p2| covers both.
            p = v.astype(np.float64) - origin.astype(np.float64)
            mag = float((np.abs(p[t[:, 0]]).sum(1) * np.abs(p[t[:, 1]]).sum(1) * np.abs(p[t[:, 2]]).sum(1)).sum())
            kV = int(m["exps"][1])
            total = sum(int(x) for x in m["table"][:, 6])
            mine = math.ldexp(float(total), -kV) / 6
            T = t.shape[0]
            bound = T * math.ldexp(1.0, -kV - 1) / 6 + 2 * (T + 16) * u * mag / 6
            assert abs(mine - surface_ref.signed_volume(p, t)) <= bound, (n, mine, surface_ref.signed_volume(p, t), bound)


def test_no_partial_sum_reaches_2_62_at_the_bound():
    """Spacings just below a power of two (the largest cells an exponent allows), an extent just below one, the origin at a
    corner, and a field that alternates from point to point, so that every cell is crossed as often as a cell can be: the sum of
    the magnitudes of every column, an upper bound of every partial sum in any order, stays below 2^62."""
    n = 17
    g = np.indices((n, n, n)).sum(0)
    rng = np.random.default_rng(11)
    f = (np.where(g % 2 == 0, 1.0, -1.0) * rng.uniform(0.05, 1.0, g.shape)).astype(np.float32)
    spacing = np.full(3, np.nextafter(f32(2.0), f32(0.0)), np.float32)
    v, t = surface_ref.surface_reference(f, ZERO, spacing, 0.0)
    T = t.shape[0]
    assert T >= 4 * (n - 1) ** 3  # every cell is crossed: the alternating cases have four triangles each
    bT, kA, kV, kM = shell_ref.exponents(T, spacing, (n, n, n))
    assert (bT, kA, kV, kM) == (T.bit_length(), 60 - bT - 4, 59 - bT - 6 - 4, 58 - bT - 6 - 4)
    q, bad = shell_ref.quantise(shell_ref.triangle_terms(v, t, ZERO), (kA, kV, kM), bT)
    assert not bad.any()
    for w in range(5):
        assert sum(abs(int(x)) for x in q[:, w]) < 1 << 62
    # and the per-term bound the header derives
    assert int(np.abs(q).max()) < 1 << (62 - bT)


def test_bad_triangles_add_nothing():
    v, t, m = _measure(f32(5.5) - _l1((8, 8, 8)))
    v2 = v.copy()
    hit = int(t[5, 1])
    v2[hit, 0] = np.inf
    m2 = shell_ref.measure(v2, t, ZERO, ONE, (16, 16, 16))
    nbad = int((t == hit).any(1).sum())
    assert m2["counts"].tolist() == [1, 1, 0, nbad] and m2["table"][0, 4] == nbad
    keep = ~(t == hit).any(1)
    q, bad = shell_ref.quantise(shell_ref.triangle_terms(v, t, ZERO), m["exps"], 728 .bit_length())
    assert not bad.any()
    assert m2["table"][0, 5:].tolist() == [sum(int(x) for x in q[keep, w]) for w in range(5)]
    assert np.isinf(m2["bbox"][0, 3])


def test_exponents_and_empty_mesh():
    assert shell_ref.exponents(0, ONE, (16, 16, 16)) == (0, 60 - 4, 59 - 5 - 4, 58 - 5 - 4)  # frexp(1) = (0.5, 1), frexp(15) = (., 4)
    assert shell_ref.exponents(1, (0.5, 0.25, 0.5), (3, 3, 3))[0] == 1
    assert shell_ref.exponents(4, ONE, (2, 2, 2))[0] == 3 and shell_ref.exponents(3, ONE, (2, 2, 2))[0] == 2
    assert shell_ref.exponents(7, (-2.0, 1.0, 1.0), (5, 2, 2)) == shell_ref.exponents(7, (2.0, 1.0, 1.0), (5, 2, 2))
    m = shell_ref.measure(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), ZERO, ONE, (16, 16, 16))
    assert m["counts"].tolist() == [0, 0, 0, 0] and m["table"].shape == (0, 10) and m["bbox"].shape == (0, 6)
    assert m["exps"].tolist() == [56, 50, 49]


# ---- order independence
def test_permuting_the_triangles_changes_nothing():
    rng = np.random.default_rng(5)
    d = _l1((7, 7, 7))
    f = np.maximum(np.minimum(f32(6.5) - d, d - f32(2.5)), f32(1.5) - _l1((13, 13, 13)))
    for f in (f, _random_lattice(rng, 6, 9, border=False)):
        v, t, m = _measure(f)
        for _ in range(3):
            p = rng.permutation(t.shape[0])
            m2 = shell_ref.measure(v, t[p], ZERO, ONE, f.shape[::-1])
            assert np.array_equal(m2["table"], m["table"]) and np.array_equal(m2["vertexShell"], m["vertexShell"])
            assert np.array_equal(m2["bbox"].view(np.uint32), m["bbox"].view(np.uint32)) and np.array_equal(m2["counts"], m["counts"])


# ---- open sides: the vertex sums the kernel counts with against the definition
def test_open_sides_by_vertex_sums_equal_the_definition():
    rng = np.random.default_rng(21)
    total = 0
    for n in range(3000):
        f = _random_lattice(rng, 3, 7, border=False)
        if n % 3 == 0:
            f = (np.round(f * 2) / 2).astype(np.float32)  # many field values equal to iso
        v, t = surface_ref.surface_reference(f, ZERO, ONE, 0.0)
        if t.shape[0] == 0:
            continue
        starts = np.zeros(v.shape[0], np.int64)
        np.add.at(starts, shell_ref.open_sides(t), 1)
        assert np.array_equal(starts, shell_ref.open_vertices_by_sum(t, v.shape[0]).astype(np.int64)), n
        total += int(starts.sum())
    assert total > 100000


# ---- the GPU scenes have something to compare
@pytest.fixture(scope="module")
def case_meshes():
    out = {}
    for name in shell_cases.HOST_CASES:
        sc, field, types, iso, lattice = shell_cases.case(name)
        ora = scenes.oracle_for(sc)
        for _ in range(shell_cases.STEPS):
            ora.step()
        state = render_mesh_cases.oracle_state(ora, sc["cfg"])
        v, t, iso = shell_cases.reference_mesh(state, field, types, iso, lattice)
        out[name] = (sc, v, t, shell_ref.measure(v, t, *lattice), lattice)
    return out


def test_pieces_has_closed_shells_and_a_cavity(case_meshes):
    sc, v, t, m, lattice = case_meshes["pieces"]
    assert m["counts"][1] >= 3 and m["counts"][2] == 0
    vol = shell_ref.values(m["table"], m["exps"])[:, 1]
    assert (vol < 0).any() and (vol > 0).sum() >= 2


def test_spray_has_several_shells_to_a_wave(case_meshes):
    sc, v, t, m, lattice = case_meshes["spray"]
    liquid = sc["position"][:sc["numOfLiquidP"], :3].astype(np.float64)
    d = np.linalg.norm(liquid[:, None, :] - liquid[None, :, :], axis=2) + np.eye(liquid.shape[0]) * 1e9
    assert d.min() > 2 * float(sc["cfg"].h)
    assert m["counts"][0] >= 256 and np.median(m["table"][:, 2]) < 64
    # and some run of 256 consecutive triangles (one block of the table kernel at this size) holds more shells than the block
    # has rows in LDS (8), so the rows beyond them are exercised too
    ts = m["vertexShell"][t[:, 0]]
    assert max(np.unique(ts[b:b + 256]).size for b in range(0, t.shape[0], 256)) > 8


def test_tiny_is_one_large_shell(case_meshes):
    sc, v, t, m, lattice = case_meshes["tiny"]
    assert m["counts"].tolist()[:3] == [1, 1, 0]
    assert t.shape[0] > 4 * 256 and t.shape[0] % 64 != 0 and v.shape[0] % 64 != 0


def test_coarse_lattice_has_open_sides(case_meshes):
    sc, v, t, m, lattice = case_meshes["coarse"]
    assert m["counts"][2] > 0 and m["counts"][1] < m["counts"][0]
    assert m["counts"][2] == shell_ref.open_sides(t).shape[0]


# ---- the helpers around it
def test_shell_summary_and_csv_round_trip(tmp_path):
    d = _l1((7, 7, 7))
    f = np.maximum(np.minimum(f32(6.5) - d, d - f32(2.5)), f32(9.5) - _l1((15, 15, 15)))
    origin = (1.5, -2.0, 0.25)
    v, t, m = _measure(f, origin, (0.5, 0.5, 0.75))
    s = frames.shell_summary(m["table"], m["exps"], origin)
    assert s["closed"].tolist() == (m["table"][:, 3] == 0).tolist() and (~s["closed"]).any()
    assert np.array_equal(s["chi"], _chi(m["table"]))
    assert s["totals"]["triangles"] == t.shape[0] and s["totals"]["vertices"] == v.shape[0] and s["totals"]["open"] == m["counts"][2]
    vals = shell_ref.values(m["table"], m["exps"])
    assert np.array_equal(s["area"], vals[:, 0] / 2) and np.array_equal(s["volume"], vals[:, 1] / 6)
    big = 0  # the shell around (7, 7, 7): its area centroid is the ball's centre, in scene coordinates
    assert np.allclose(s["centroid"][big], np.array(origin) + 7 * np.array((0.5, 0.5, 0.75)), atol=1e-9)
    assert np.allclose(s["radius"], np.cbrt(3 * np.abs(s["volume"]) / (4 * np.pi)))
    path = str(tmp_path / "shells.csv")
    frames.write_shells_csv(path, m["table"], m["bbox"], m["exps"])
    table, bb, exps = frames.read_shells(path)
    assert table.dtype == np.int64 and np.array_equal(table, m["table"])
    assert bb.dtype == np.float32 and np.array_equal(bb.view(np.uint32), m["bbox"].view(np.uint32))
    assert exps.tolist() == m["exps"].tolist()
    empty = str(tmp_path / "empty.csv")
    frames.write_shells_csv(empty, np.zeros((0, 10), np.int64), np.zeros((0, 6), np.float32), (56, 50, 49))
    table, bb, exps = frames.read_shells(empty)
    assert table.shape == (0, 10) and bb.shape == (0, 6) and exps.tolist() == [56, 50, 49]
    with open(empty, "w") as g:
        g.write("step,region\n")
    with pytest.raises(ValueError):
        frames.read_shells(empty)


def test_entry_points_are_declared_and_exported():
    assert sphmi.SHELL_WORDS == shell_ref.WORDS == len(sphmi.SHELL_FIELDS) and sphmi.SHELL_FIELDS == shell_ref.FIELDS == frames.SHELL_FIELDS
    with open(os.path.join(scenes.ROOT, "include", "sphmi.h")) as f:
        txt = f.read()
    assert "#define SPH_SHELL_WORDS 10" in txt and "#define SPHMI_ABI_VERSION 2" in txt
    lib = sphmi.device_lib()
    for n in ("sph_measure_surface", "sph_read_shells"):
        assert n in sphmi.EXPORTED_SYMBOLS and ("int %s(" % n) in txt
        assert hasattr(lib, n)
    assert hasattr(sphmi.owHIPSolver, "measure_surface") and hasattr(sphmi.owHIPSolver, "surface_shells")
