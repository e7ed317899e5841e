"""The probe contract without a GPU (include/sphmi.h, sph_probes_*): the crossing rule of the numpy restatement (tests/probe_ref.py)
against literal numbers; the restatement and the helpers of sphmi/frames.py (level_columns, level_heights, probe_series) on a
synthetic cloud, against free_surface_height of the same lattice; the binding's structure and the wrappers' shape checks; and what
the line cases of the GPU tests (tests/probe_cases.py) claim, on the oracle's state."""
import ctypes

import numpy as np
import pytest

import probe_cases as pc
import probe_ref as pr
import sample_ref
import scenes
import sphmi
from sphmi import frames
from test_sample_host import _cloud

f32 = np.float32
NAN = np.nan


# ---------------------------------------------------------------------------------------------- the crossing rule
def test_one_crossing():
    status, K, t = pr.level_of([1.0, 0.75, 0.25, 0.0], 0.5)
    assert (status, K) == (pr.FOUND, 1) and t == f32(0.5)  # (0.5 - 0.75) / (0.25 - 0.75)


def test_several_crossings_the_far_one_wins():
    status, K, t = pr.level_of([1.0, 0.0, 1.0, 0.0, 0.875, 0.125, 0.0], 0.5)
    assert (status, K) == (pr.FOUND, 4) and t == f32(0.5)
    status, K, t = pr.level_of([1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], 0.25)
    assert (status, K) == (pr.FOUND, 2) and t == f32(0.75)


def test_value_equal_to_iso_is_inside_and_t_is_zero():
    status, K, t = pr.level_of([1.0, 0.5, 0.25], 0.5)
    assert (status, K) == (pr.FOUND, 1) and t == 0 and np.signbit(t)  # +0 / -0.25
    # ... and at K + 1 it is inside too: the crossing moves up
    status, K, t = pr.level_of([1.0, 0.5, 0.5, 0.25], 0.5)
    assert (status, K) == (pr.FOUND, 2)


def test_inside_at_the_far_end_is_submerged():
    assert pr.level_of([0.0, 1.0, 0.0, 0.5], 0.5) == (pr.SUBMERGED, 3, None)
    assert pr.level_of([0.0, 0.0], 0.0) == (pr.SUBMERGED, 1, None)
    assert pr.level_of([-1.0, -0.0], 0.0) == (pr.SUBMERGED, 1, None)  # -0 >= +0


def test_nothing_inside_is_dry():
    assert pr.level_of([0.25, 0.0, 0.125], 0.5) == (pr.DRY, -1, None)
    assert pr.level_of([0.0, 1.0], 0.5) == (pr.SUBMERGED, 1, None) and pr.level_of([0.0, 0.25], 0.5) == (pr.DRY, -1, None)


def test_nan_is_outside():
    assert pr.level_of([NAN, NAN, NAN], 0.5) == (pr.DRY, -1, None)
    assert pr.level_of([1.0, NAN], 0.5)[:2] == (pr.FOUND, 0) and np.isnan(pr.level_of([1.0, NAN], 0.5)[2])
    status, K, t = pr.level_of([1.0, NAN, 0.75, 0.25, NAN], 0.5)  # a NaN at the far end does not submerge the line
    assert (status, K) == (pr.FOUND, 2) and t == f32(0.5)
    status, K, t = pr.level_of([1.0, 0.75, NAN, 0.0], 0.5)  # the crossing into a NaN counts, with a NaN t
    assert (status, K) == (pr.FOUND, 1) and np.isnan(t)


def test_count_two():
    assert pr.level_of([1.0, 0.0], 0.5) == (pr.FOUND, 0, f32(0.5))
    assert pr.level_of([1.0, 1.0], 0.5) == (pr.SUBMERGED, 1, None)
    assert pr.level_of([0.0, 0.0], 0.5) == (pr.DRY, -1, None)


def test_record_words_of_the_three_outcomes():
    ln = pc.line((1.0, 2.0, 3.0), (0.0, 0.0, 0.5), 4)[0]
    r = pr.record_of(ln, np.array([1.0, 0.75, 0.25, 0.0], f32))
    assert r.tolist() == [1.0, 2.0, 3.75, 1.5, 0.0, 1.0, 0.75, 0.25]
    r = pr.record_of(ln, np.array([0.0, 0.0, 0.0, 2.0], f32))
    assert r.tolist() == [1.0, 2.0, 4.5, 3.0, 2.0, 3.0, 2.0, 0.0]
    r = pr.record_of(ln, np.array([0.0, 0.0, 0.0, 0.0], f32))
    assert r.tolist() == [1.0, 2.0, 3.0, 0.0, 1.0, -1.0, 0.0, 0.0]
    r = pr.record_of(ln, np.array([1.0, NAN, 0.0, 0.0], f32))
    assert np.isnan(r[:4]).all() and r[4:7].tolist() == [0.0, 0.0, 1.0] and np.isnan(r[7])


# ---------------------------------------------------------------------------------------------- the restatement on a cloud
LATTICE = ((-6.0, 2.0, 1.0), (1.0, 1.5, 0.5), (24, 6, 29))  # dyadic: float32 and float64 agree on every coordinate; top plane z = 15


@pytest.fixture(scope="module")
def cloud():
    """The cloud of test_sample_host with its upper half emptied where x < 12: a step in the level. The lattice starts outside the
    cloud in x (dry columns), ends at z = 15 inside the part that is still full (submerged columns) and crosses the cut elsewhere."""
    state, _ = _cloud()
    keep = ~((state["pos"][:, 2] > 10.0) & (state["pos"][:, 0] < 12.0))
    for k in ("pos", "vel", "rho", "p", "types", "keys"):
        state[k] = state[k][keep]
    o, s, d = LATTICE
    g = sample_ref.grid_points(o, s, d)
    grid = sample_ref.sample_reference(state, g.reshape(-1, 3), (1, 2, 3)).reshape(d[2], d[1], d[0], 8)
    iso = f32(0.5) * f32(np.median(grid[:10, :, 12:, 1]))
    lines = frames.level_columns(o, s, d, axis=2, field="shepard", iso=iso, types=(1, 2, 3))
    return state, g, grid, iso, lines, pr.level_records(state, lines)


def test_level_columns_are_the_lattice_columns(cloud):
    _, g, _, iso, lines, _ = cloud
    o, s, d = LATTICE
    assert lines.dtype == sphmi.PROBE_LINE_DTYPE == pr.LINE_DTYPE and lines.shape == (d[0] * d[1],)
    assert (lines["count"] == d[2]).all() and (lines["field"] == 1).all() and (lines["typeMask"] == 14).all() and (lines["iso"] == iso).all()
    for j, i in ((0, 0), (3, 17), (5, 23)):
        assert scenes.bits_equal(pr.line_points(lines[j * d[0] + i]), g[:, j, i])
    # the other axes: the far end is the lattice's last plane along the axis, the lower of the other two axes runs fastest
    lx = frames.level_columns(o, s, d, axis=0, field=5, iso=0.0, types=(1,))
    assert lx.shape == (d[1] * d[2],) and (lx["count"] == d[0]).all() and (lx["field"] == 5).all() and (lx["typeMask"] == 2).all()
    assert scenes.bits_equal(pr.line_points(lx[7 * d[1] + 2]), g[7, 2, :])
    ly = frames.level_columns(o, s, d, axis=1)
    assert scenes.bits_equal(pr.line_points(ly[9 * d[0] + 4]), g[9, :, 4]) and (ly["iso"] == f32(0.5)).all()
    with pytest.raises(ValueError):
        frames.level_columns(o, s, d, axis=3)


def test_records_are_the_rule_on_the_grid_sample(cloud):
    _, g, grid, iso, lines, rec = cloud
    o, s, d = LATTICE
    f = grid[..., 1]
    seen = set()
    for j in range(d[1]):
        for i in range(d[0]):
            r = rec[j * d[0] + i]
            status, K, t = pr.level_of(f[:, j, i], iso)
            seen.add(status)
            assert r[4] == status and r[5] == K
            if status == pr.FOUND:
                assert r[6] == f[K, j, i] and r[7] == f[K + 1, j, i] and r[3] == f32(K) + t
                assert r[0] == g[K, j, i, 0] and r[1] == g[K, j, i, 1]
                assert r[2] == g[K, j, i, 2] + t * (g[K + 1, j, i, 2] - g[K, j, i, 2])
    assert seen == {pr.FOUND, pr.DRY, pr.SUBMERGED}


def test_level_heights_against_free_surface_height(cloud):
    _, g, grid, iso, lines, rec = cloud
    o, s, d = LATTICE
    got = frames.level_heights(rec, axis=2).reshape(d[1], d[0])
    want = frames.free_surface_height(grid, o, s, threshold=float(iso))
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
    status = rec[:, 4].reshape(d[1], d[0])
    K = rec[:, 5].reshape(d[1], d[0]).astype(int)
    top = status == pr.SUBMERGED
    assert top.any() and np.array_equal(got[top], want[top]) and (got[top] == 15.0).all()
    found = status == pr.FOUND
    z0, z1 = g[:, 0, 0, 2][K[found]].astype(np.float64), g[:, 0, 0, 2][K[found] + 1].astype(np.float64)
    assert found.sum() > 20 and ((z0 <= want[found]) & (want[found] <= z1)).all() and ((z0 <= got[found]) & (got[found] <= z1)).all()
    assert np.abs(got[found] - want[found]).max() < 1e-4  # (float32 against float64 on heights up to 15: a sanity bound, not the contract)
    with pytest.raises(ValueError):
        frames.level_heights(rec[:, :7])


def test_probe_series(cloud):
    rec = cloud[5]
    hist = np.stack([rec, rec[::-1], rec])
    z = frames.probe_series(hist, "z")
    assert z.shape == (3, rec.shape[0]) and z.dtype == np.float32 and scenes.bits_equal(z[1], rec[::-1, 2])
    assert scenes.bits_equal(frames.probe_series(hist, 4), hist[:, :, 4]) and scenes.bits_equal(frames.probe_series(hist, "status"), hist[:, :, 4])
    assert scenes.bits_equal(frames.probe_series(hist, "pressure"), hist[:, :, 5])  # a point record's name
    assert frames.LEVEL_FIELDS == ("x", "y", "z", "index", "status", "k", "f_inside", "f_outside")
    for bad in (rec, hist[..., :7]):
        with pytest.raises(ValueError):
            frames.probe_series(bad, 0)
    with pytest.raises(ValueError):
        frames.probe_series(hist, "height")


def test_point_records_restate_sampling(cloud):
    state = cloud[0]
    pts = np.array([[5.0, 5.0, 5.0], [5.0, 5.0, 15.0], [NAN, 1.0, 1.0], [15.0, 5.0, 15.0]], f32)
    assert scenes.bits_equal(pr.point_records(state, pts, (1, 2)), sample_ref.sample_reference(state, pts, (1, 2)))


# ---------------------------------------------------------------------------------------------- the binding
def test_structure_and_symbols():
    assert ctypes.sizeof(sphmi.SphProbeLine) == 40 and sphmi.PROBE_LINE_DTYPE.itemsize == 40
    for name, _ in sphmi.SphProbeLine._fields_:
        assert getattr(sphmi.SphProbeLine, name).offset == sphmi.PROBE_LINE_DTYPE.fields[name][1]
    lib = sphmi.device_lib()
    txt = open(scenes.ROOT + "/include/sphmi.h").read()
    for n in ("sph_probes_set_points", "sph_probes_set_lines", "sph_probes_count", "sph_probes_record", "sph_probes_history",
              "sph_probes_read_history"):
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for name, value in (("SPH_PROBE_MAX_POINTS", sphmi.PROBE_MAX_POINTS), ("SPH_PROBE_MAX_LINES", sphmi.PROBE_MAX_LINES),
                        ("SPH_PROBE_LINE_MAX", sphmi.PROBE_LINE_MAX), ("SPH_PROBE_LEVEL_WORDS", sphmi.PROBE_LEVEL_WORDS),
                        ("SPH_PROBE_HISTORY_MAX", sphmi.PROBE_HISTORY_MAX), ("SPH_PROBE_FOUND", sphmi.PROBE_FOUND),
                        ("SPH_PROBE_DRY", sphmi.PROBE_DRY), ("SPH_PROBE_SUBMERGED", sphmi.PROBE_SUBMERGED)):
        assert "#define %s %d" % (name, value) in txt
    assert (pr.FOUND, pr.DRY, pr.SUBMERGED) == (sphmi.PROBE_FOUND, sphmi.PROBE_DRY, sphmi.PROBE_SUBMERGED)
    assert "#define SPHMI_ABI_VERSION 2" in txt  # entry points are appended; the version stays


def test_wrappers_refuse_bad_shapes():
    class NoSolver:  # the checks come before any library call
        _h = None
    for bad in (np.zeros((3, 2), f32), np.zeros((2, 3, 5), f32), np.zeros(7, f32)):
        with pytest.raises(sphmi.SphError):
            sphmi.owHIPSolver.probes_set_points(NoSolver(), bad)
    good = pc.line((0, 0, 0), (0, 0, 1), 4)
    for bad in (np.zeros((2, 10), f32), np.zeros(3, np.dtype([("origin", f32, 3), ("step", f32, 3)])), np.stack([good, good]), [1.5],
                [dict(origin=(0, 0), step=(0, 0, 1), count=4)], [dict(origin=(0, 0, 0), step=(0, 0, 1, 0), count=4)],
                [dict(origin=(0, 0, 0), step=(0, 0, 1), count=4, field="height")]):
        with pytest.raises(sphmi.SphError):
            sphmi.owHIPSolver.probes_set_lines(NoSolver(), bad)
    # what they accept comes out as the 40-byte records
    ln = sphmi.probe_lines([dict(origin=(1, 2, 3), step=(0, 0.5, 0), count=9, field="vy", iso=0.25, types=(1, 3))])
    want = pc.line((1, 2, 3), (0, 0.5, 0), 9, field=3, iso=0.25, mask=10)
    assert ln.tobytes() == want.tobytes()
    s = sphmi.SphProbeLine((1, 2, 3), (0, 0.5, 0), 9, 3, 0.25, 10)
    assert sphmi.probe_lines(s).tobytes() == want.tobytes() == bytes(s) and sphmi.probe_lines([s, s]).shape == (2,)
    assert sphmi.probe_lines(None).shape == (0,) and sphmi.probe_lines(want) is not None


# ---------------------------------------------------------------------------------------------- the GPU tests' cases
def test_line_cases_hold_what_they_claim():
    sc = pc.scene()
    state = pc.oracle_state(sc)
    cases = pc.build(sc["cfg"], state)
    lines = pc.all_lines(cases)
    fields = pr.line_fields(state, lines)
    rec = pr.level_records(state, lines, fields)
    pc.check_claims(cases, rec, fields)
    names = [n for n, _ in cases]
    assert names == ["counts", "sweep", "faces", "submerged", "dry", "t zero", "vy", "leaves up", "enters", "below zero", "masks"]
    # every line is one the library accepts
    assert (lines["count"] >= 2).all() and (lines["count"] <= sphmi.PROBE_LINE_MAX).all() and np.isfinite(lines["origin"]).all()
    # the sweep alone puts a crossing on every offset from the far end that a chunking by 64 (or by anything up to 130) can cut at
    s = pc.spans(cases)["sweep"]
    from_far_end = lines["count"][s] - 1 - rec[s, 5].astype(int)
    assert set(range(6, 136)) <= set(from_far_end.tolist())
