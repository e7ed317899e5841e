"""CPU tests of the time statistics on a lattice (include/sphmi.h, sph_stats_*): the restated fold and moments (tests/stats_ref.py)
against literal numbers, the claims of the shared cases (tests/stats_cases.py) on the oracle's states, frames.stats_summary, the
binding's record and the wrappers' shape checks. tests/test_stats.py compares the device with the same restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import probe_cases
import scenes
import sphmi
import stats_cases as sc_
import stats_ref as sr
from sphmi import frames

F = np.float32
INF, NAN = np.inf, np.nan


def rec(rho=0.0, v=(0.0, 0.0, 0.0), p=0.0, n=0.0):
    return np.array([[rho, 0.0, v[0], v[1], v[2], p, n, 0.0]], F)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_empty_values():
    a = sr.empty(3)
    want = [0, -1, -1] + [0] * 13 + [-INF, -1, -INF, -1, -INF, -1, INF, -1]
    assert a.shape == (3, 24) and all(np.array_equal(b64(row), b64(np.array(want, np.float64))) for row in a)
    assert not np.signbit(a[0, 0]) and not np.signbit(a[0, 3:16]).any()  # +0


def test_one_wet_call():
    r = rec(rho=1000.0, v=(0.5, -2.0, 0.25), p=-3.0, n=7.0)
    a = sr.fold(sr.empty(1), r, 4)[0]
    want = [1, 4, 4, 1000.0, 1e6, 0.5, -2.0, 0.25, 0.25, 4.0, 0.0625, -1.0, 0.125, -0.5, -3.0, 9.0, 1000.0, 4, 4.3125, 4, -3.0, 4, -3.0, 4]
    assert np.array_equal(b64(a), b64(np.array(want, np.float64))), a
    m = sr.moments(a[None], 5)[0]
    # n/C, rho/C, rho2/C - (rho/C)^2; the wet means; covariances of a single sample vanish; arrival 4, peak -3
    want_m = [0.2, 200.0, 2e5 - 4e4, 0.5, -2.0, 0.25, 0, 0, 0, 0, 0, 0, -3.0, 0.0, 4.0, -3.0]
    assert np.array_equal(m.view(np.uint32), np.array(want_m, F).view(np.uint32)), m


def test_dry_call_between_two_wet_ones():
    a = sr.empty(1)
    a = sr.fold(a, rec(rho=2.0, v=(1.0, 0.0, 0.0), p=5.0, n=1.0), 0)
    before = a.copy()
    a = sr.fold(a, rec(), 1)  # dry: all-zero record
    assert np.array_equal(b64(a), b64(before))
    a = sr.fold(a, rec(rho=4.0, v=(3.0, 0.0, 4.0), p=1.0, n=2.0), 2)[0]
    want = [2, 0, 2, 6.0, 20.0, 4.0, 0.0, 4.0, 10.0, 0.0, 16.0, 0.0, 12.0, 0.0, 6.0, 26.0, 4.0, 2, 25.0, 2, 5.0, 0, 1.0, 2]
    assert np.array_equal(b64(a), b64(np.array(want, np.float64))), a
    m = sr.moments(a[None], 3)[0]
    # wet 2 of 3; mean rho over all calls 2, variance 20/3 - 4; mean v (2, 0, 2); xx = 10/2 - 4 = 1, zz = 16/2 - 4 = 4, xz = 12/2 - 4 = 2
    want_m = [F(2.0 / 3.0), 2.0, F(20.0 / 3.0 - 4.0), 2.0, 0.0, 2.0, 1.0, 0.0, 4.0, 0.0, 2.0, 0.0, 3.0, 4.0, 0.0, 5.0]
    assert np.array_equal(m.view(np.uint32), np.array(want_m, F).view(np.uint32)), m


def test_tie_keeps_the_first_call():
    a = sr.empty(1)
    for c in range(3):
        a = sr.fold(a, rec(rho=2.0, v=(0.0, 1.0, 0.0), p=-1.0, n=1.0), c)
    assert tuple(a[0, [17, 19, 21, 23]]) == (0, 0, 0, 0) and tuple(a[0, [16, 18, 20, 22]]) == (2.0, 1.0, -1.0, -1.0)
    assert tuple(a[0, :3]) == (3, 0, 2)


def test_nan_word():
    """The compares ignore a NaN, the sums carry it."""
    a = sr.fold(sr.empty(1), rec(rho=1.0, v=(1.0, 1.0, 1.0), p=2.0, n=1.0), 0)
    a = sr.fold(a, rec(rho=3.0, v=(NAN, 1.0, 1.0), p=NAN, n=1.0), 1)[0]
    assert a[0] == 2 and a[2] == 1
    assert np.isnan(a[[5, 8, 11, 12, 14, 15]]).all() and not np.isnan(a[[3, 4, 6, 7, 9, 10, 13]]).any()
    assert tuple(a[16:24]) == (3.0, 1, 3.0, 0, 2.0, 0, 2.0, 0)
    # a NaN record first: the extremes stay empty until a number comes
    b = sr.fold(sr.empty(1), rec(rho=1.0, p=NAN, n=1.0), 0)[0]
    assert tuple(b[20:24]) == (-INF, -1, INF, -1)
    m = sr.moments(a[None], 2)[0]
    assert np.isnan(m[[3, 6, 9, 10, 12, 13]]).all() and m[14] == 0 and m[15] == 2.0


def test_moments_of_a_node_that_was_never_wet_and_of_no_call():
    m = sr.moments(sr.empty(2), 3)
    want = np.zeros(16, F)
    want[14] = -1
    assert np.array_equal(m.view(np.uint32), np.tile(want, (2, 1)).view(np.uint32))
    with pytest.raises(AssertionError):
        sr.moments(sr.empty(1), 0)
    with pytest.raises(ValueError):
        frames.stats_moments(sr.empty(1), 0)


@pytest.fixture(scope="module")
def oracle_records():
    """{lattice name: the records of the four calls} on oracle states; the edit is made by creating the oracle anew from the edited
    arrays."""
    sc = sc_.scene()
    lat = sc_.lattices(sc["cfg"])
    records = {k: [] for k in lat}
    done = 0
    for call, steps in enumerate(sc_.STEPS_BEFORE_CALL):
        if call == sc_.EDIT_BEFORE_CALL:
            ora = scenes.oracle_for(sc, threads=8)
            for _ in range(done):
                ora.step()
            N = sc["cfg"].particleCount
            pos, vel = ora.buffer("position").reshape(-1, 4)[:N].copy(), ora.buffer("velocity").reshape(-1, 4)[:N].copy()
            ora.close()
            sc, removed = sc_.edited_scene(sc, pos, vel)
            assert removed > 100
            done = 0
        done += steps
        state = probe_cases.oracle_state(sc, steps=done)
        for k, g in lat.items():
            records[k].append(sr.lattice_records(state, g))
    return records


@pytest.mark.parametrize("name", ["A", "B"])
def test_claims_on_the_oracle(oracle_records, name):
    sizes = sc_.check_claims(oracle_records[name])
    print(name, sizes)


def test_summary_against_the_restated_moments(oracle_records):
    acc, calls = sc_.fold_sequence(oracle_records["A"])[-1]
    m = sr.moments64(acc, calls)
    assert np.array_equal(b64(frames.stats_moments(acc, calls)), b64(m))
    s = frames.stats_summary(acc.reshape(9, 19, 17, 24), calls)
    flat = lambda v: np.ascontiguousarray(v).reshape(m.shape[0], -1)
    assert np.array_equal(b64(flat(s["wet_fraction"])[:, 0]), b64(m[:, 0]))
    assert np.array_equal(b64(flat(s["mean_velocity"])), b64(m[:, 3:6]))
    st = s["stress"].reshape(-1, 3, 3)
    for w, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        assert np.array_equal(b64(st[:, i, j]), b64(m[:, 6 + w])) and np.array_equal(b64(st[:, j, i]), b64(m[:, 6 + w]))
    assert np.array_equal(b64(flat(s["tke"])[:, 0]), b64(0.5 * ((m[:, 6] + m[:, 7]) + m[:, 8])))
    assert np.array_equal(b64(flat(s["mean_pressure"])[:, 0]), b64(m[:, 12]))
    assert np.array_equal(b64(flat(s["rms_pressure"])[:, 0]), b64(np.sqrt(np.maximum(m[:, 13], 0.0))))
    assert np.array_equal(b64(flat(s["arrival_call"])[:, 0]), b64(acc[:, 1]))
    assert np.array_equal(b64(flat(s["peak_pressure"])[:, 0]), b64(m[:, 15]))
    assert np.array_equal(b64(flat(s["peak_pressure_call"])[:, 0]), b64(acc[:, 21]))
    assert s["stress"].shape == (9, 19, 17, 3, 3) and (s["tke"][acc.reshape(9, 19, 17, 24)[..., 0] > 1] > 0).any()
    assert set(np.unique(s["arrival_call"])) >= {-1.0, 0.0, 2.0}


def test_vtk_and_file_round_trip(oracle_records, tmp_path):
    acc, calls = sc_.fold_sequence(oracle_records["B"])[-1]
    g = sc_.lattices(sc_.scene()["cfg"])["B"]
    nx, ny, nz = g["dims"]
    path = str(tmp_path / "stats.vtk")
    assert frames.write_vtk_stats(path, g["origin"], g["spacing"], acc.reshape(nz, ny, nx, 24), calls) == nx * ny * nz
    data = open(path, "rb").read()
    assert b"DIMENSIONS %d %d %d\n" % (nx, ny, nz) in data and b"VECTORS mean_velocity float" in data and b"SCALARS stress_xz float" in data
    at = data.index(b"SCALARS wet_fraction float 1\nLOOKUP_TABLE default\n") + len(b"SCALARS wet_fraction float 1\nLOOKUP_TABLE default\n")
    got = np.frombuffer(data[at:at + 4 * nx * ny * nz], ">f4")
    assert np.array_equal(got.astype(F), (acc[:, 0] / calls).astype(F))
    with pytest.raises(ValueError):
        frames.write_vtk_stats(path, g["origin"], g["spacing"], acc, calls)
    # the driver's file format
    rec = np.zeros(1, sphmi.STATS_LATTICE_DTYPE)
    rec["origin"], rec["spacing"], rec["dims"], rec["typeMask"] = g["origin"], g["spacing"], g["dims"], g["typeMask"]
    path = str(tmp_path / "stats.bin")
    with open(path, "wb") as f:
        f.write(b"sphmi stats calls %d from 1 every 2 nx %d ny %d nz %d\n" % (calls, nx, ny, nz))
        f.write(rec.tobytes())
        f.write(acc.tobytes())
    lat, a, c, first, every = frames.read_stats(path)
    assert (c, first, every) == (calls, 1, 2) and lat["dims"] == (nx, ny, nz) and lat["typeMask"] == g["typeMask"]
    assert np.array_equal(b64(a.reshape(-1, 24)), b64(acc)) and np.array_equal(lat["spacing"], g["spacing"])
    with open(path, "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(ValueError):
        frames.read_stats(path)


def test_binding_record_is_40_bytes():
    assert C.sizeof(sphmi.SphStatsLattice) == 40 and sphmi.STATS_LATTICE_DTYPE.itemsize == 40
    for (name, ctype), field in zip(sphmi.SphStatsLattice._fields_, sphmi.STATS_LATTICE_DTYPE.names):
        assert name == field and getattr(sphmi.SphStatsLattice, name).offset == sphmi.STATS_LATTICE_DTYPE.fields[field][1]
    g = sphmi.stats_lattice((1, 2, 3), (0.5, 0.25, 0.125), (4, 5, 6), types=(1, 3))
    s = sphmi.SphStatsLattice.from_buffer_copy(g.tobytes())
    assert tuple(s.origin) == (1, 2, 3) and tuple(s.spacing) == (0.5, 0.25, 0.125) and tuple(s.dims) == (4, 5, 6) and s.typeMask == 10
    assert len(sphmi.STATS_FIELDS) == sphmi.STATS_WORDS == sr.WORDS == 24
    assert len(sphmi.STATS_MOMENT_FIELDS) == sphmi.STATS_MOMENT_WORDS == sr.MOMENT_WORDS == 16
    assert len(set(sphmi.STATS_FIELDS)) == 24 and len(set(sphmi.STATS_MOMENT_FIELDS)) == 16
    assert sphmi.MAX_STATS == 4 and sphmi.STATS_BYTES_MAX == 1 << 31


def test_header_and_exports():
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    lib = sphmi.device_lib()
    for n in ("sph_stats_define", "sph_stats_get", "sph_stats_accumulate", "sph_stats_reset", "sph_stats_read", "sph_stats_read_moments"):
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for define in ("#define SPH_MAX_STATS 4", "#define SPH_STATS_WORDS 24", "#define SPH_STATS_MOMENT_WORDS 16", "#define SPHMI_ABI_VERSION 2"):
        assert define in txt, define
    assert lib.sph_abi_version() == 2


def test_wrapper_shape_checks():
    for bad in (dict(origin=(1, 2)), dict(spacing=(1, 2, 3, 4)), dict(dims=(4, 4)), dict(dims=(4.0, 4.0, 4.0)), dict(dims=(1 << 31, 1, 1))):
        args = dict(origin=(0, 0, 0), spacing=(1, 1, 1), dims=(4, 4, 4))
        args.update(bad)
        with pytest.raises(sphmi.SphError):
            sphmi.stats_lattice(**args)
    g = sphmi.stats_lattice(np.zeros((3, 1)), [1, 1, 1], np.array([2, 3, 4], np.int64), types=())
    assert g.shape == (1,) and tuple(g["dims"][0]) == (2, 3, 4) and g["typeMask"][0] == 0  # (the library judges mask and dims <= 0)
    with pytest.raises(ValueError):
        frames.stats_summary(np.zeros((5, 23)), 1)
