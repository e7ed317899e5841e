"""GPU tests of the flow diagnostics (sph_diagnostics / sph_histogram, include/sphmi.h): every record word and every bin
bit-identical to the numpy restatement (tests/diag_ref.py), independent of the other regions of a call, read-only behaviour, the
calling rules and the driver's CSV."""
import os
import subprocess

import numpy as np
import pytest

import diag_ref
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
MASKS = [(1,), (1, 2), (1, 2, 3)]
INF = np.inf
EMPTY = 12  # index of the empty region in make_regions()


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(u64(got), u64(want)):
        r, w = [int(x[0]) for x in np.nonzero(u64(got) != u64(want))]
        raise AssertionError("%s: %d words differ; first region %d word %d (%s): %r vs %r"
                             % (what, int((u64(got) != u64(want)).sum()), r, w, frames.DIAG_FIELDS[w], got[r, w], want[r, w]))


def make_regions(state, types):
    """16 regions from the bounding box of the selected particles: everything, the two halves along each axis, thin slabs, a
    centred box, an octant, one region with infinite bounds on two axes and (index EMPTY) one that holds nothing."""
    sel = diag_ref.selected(state, diag_ref.EVERYTHING, types)
    p = state["pos"][sel].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    mid, ext = (lo + hi) / 2, hi - lo
    big = [(-INF, -INF, -INF, INF, INF, INF)]
    for k in range(3):
        a, b = [-INF] * 6, [-INF] * 3 + [INF] * 3
        a[3], a[4], a[5] = INF, INF, INF
        a[3 + k] = mid[k]
        b[k] = mid[k]
        big += [tuple(a), tuple(b)]
    # thin slabs, an eighth of the extent, finite on every axis (the y one off-centre: tiny_elastic has no liquid at its sheet)
    for k, at in ((0, 0.5), (1, 0.3), (2, 0.5), (0, 0.2), (2, 0.8)):
        r = [lo[0] - 1, lo[1] - 1, lo[2] - 1, hi[0] + 1, hi[1] + 1, hi[2] + 1]
        r[k], r[3 + k] = lo[k] + at * ext[k] - ext[k] / 16, lo[k] + at * ext[k] + ext[k] / 16
        big.append(tuple(r))
    big.append((hi[0] + 100, hi[1] + 100, hi[2] + 100, hi[0] + 200, hi[1] + 200, hi[2] + 200))  # EMPTY
    big.append((-INF, -INF, lo[2] + 0.3 * ext[2], INF, INF, lo[2] + 0.6 * ext[2]))  # infinite on two axes
    big.append((lo[0], lo[1], lo[2], mid[0], mid[1], mid[2]))  # an octant
    big.append(tuple(mid - ext / 4) + tuple(mid + ext / 4))  # a centred box
    regions = np.array(big, np.float32)
    assert regions.shape == (16, 6) and EMPTY == 12
    return regions


def check_records(hip, masks=MASKS, what="", hollow=False):
    """Records of a 16-region call and of one-region calls against the restatement, for each mask; returns the state.
    hollow: the scene is a long boundary shell with a small body of liquid at one end, so the centred box (region 15) of the
    selections that include the boundary holds nothing."""
    state = diag_ref.state_with_ids(hip)
    rho0 = hip.cfg.rho0
    types_present = set(np.unique(state["types"].astype(np.int32)).tolist())
    for types in masks:
        if not types_present & set(types):
            continue
        regions = make_regions(state, types)
        want = diag_ref.records(state, regions, types, rho0)
        n_all = want[0, 0]
        assert n_all > 0
        for r in range(16):  # no case passes vacuously
            if r == EMPTY or (hollow and r == 15 and 3 in types):
                assert want[r, 0] == 0, (what, types, r)
            else:
                assert want[r, 0] > 0, (what, types, r)
                assert r == 0 or want[r, 0] < n_all, (what, types, r)
        got = hip.diagnostics(regions, types)
        assert_records(got, want, "%s types %s, 16 regions" % (what, types))
        for r in (0, 1, 7, EMPTY, 13):  # a record does not depend on the other regions of the call
            one = hip.diagnostics(regions[r:r + 1], types)
            assert_records(one, want[r:r + 1], "%s types %s, region %d alone" % (what, types, r))
        assert_records(hip.diagnostics(regions[[5, 0, EMPTY]], types), want[[5, 0, EMPTY]], "%s types %s, 3 regions" % (what, types))
    return state


HIST_CASES = [("density", 900.0, 1100.0, 64), ("density", 999.0, 1001.0, 4096), ("speed", 0.0, 2.0, 50), ("pressure", 0.0, 50.0, 33),
              ("pressure", -1.0, 1.0, 1), ("neighbors", 0.0, 33.0, 33), ("x", 0.0, 60.0, 100), ("y", 5.0, 25.0, 7), ("z", 0.0, 300.0, 1000)]


def check_histograms(hip, state, masks=MASKS, what=""):
    nbr = diag_ref.neighbor_counts(hip)
    types_present = set(np.unique(state["types"].astype(np.int32)).tolist())
    for types in masks:
        if not types_present & set(types):
            continue
        regions = make_regions(state, types)
        n_of = hip.diagnostics(regions, types)[:, 0]
        for region_index in (None, 2, 13, EMPTY):
            region = None if region_index is None else regions[region_index]
            n = n_of[0 if region_index is None else region_index]
            for field, lo, hi, bins in HIST_CASES:
                got = hip.histogram(field, lo, hi, bins, region, types)
                want = diag_ref.histogram(state, field, lo, hi, bins, region, types, nbr)
                assert got.dtype == np.uint32 and got.shape == (bins + 2,)
                assert np.array_equal(got, want), (what, types, region_index, field, np.flatnonzero(got != want)[:8])
                assert int(got.sum()) == int(n)  # every selected particle lands in exactly one counter
                assert np.array_equal(hip.histogram(diag_ref.FIELDS.index(field), lo, hi, bins, region, types), got)
        # the neighbour-count distribution against a direct count over the rows
        sel = diag_ref.selected(state, diag_ref.EVERYTHING, types)
        got = hip.histogram("neighbors", 0, 33, 33, None, types)
        assert got[0] == 0 and got[34] == 0
        assert np.array_equal(got[1:34], np.bincount(nbr[sel].astype(np.int64), minlength=33))
    return nbr


def _scene(name):
    return scenes.config1() if name == "config1" else scenes.SCENES[name]()


@pytest.mark.parametrize("name", ["tiny", "tiny_compressed", "tiny_jitter", "tiny_elastic", "config1", "alias16", "wide"])
def test_records_and_histograms_match_restatement(name):
    sc = _scene(name)
    hip = scenes.hip_for(sc)
    hip.step(0)
    hollow = name in ("alias16", "wide")
    state = check_records(hip, what=name + " step 0", hollow=hollow)
    check_histograms(hip, state, what=name + " step 0")
    for it in range(1, 5):
        hip.step(it)
    state = check_records(hip, what=name + " step 4", hollow=hollow)
    nbr = check_histograms(hip, state, what=name + " step 4")
    rec = hip.diagnostics()[0]  # the defaults: everything, types (1, 2)
    assert_records(rec[None], diag_ref.records(state, [diag_ref.EVERYTHING], (1, 2), hip.cfg.rho0), name + " defaults")
    assert rec[10] > 0 and rec[20] > 0 and rec[21] >= 0 and rec[22] >= 0  # the fluid moves after five steps
    assert nbr.max() > 10
    if name == "tiny_compressed":  # a pressure-active state
        assert rec[13] > 0 and rec[19] > 0 and rec[12] > 0
    s = frames.diagnostics_summary(rec, hip.cfg)
    assert s["n"] == int(rec[0]) and s["kinetic_energy"] > 0 and s["min_density"] <= s["mean_density"] <= s["max_density"]
    hip.close()


def test_staged_path_matches_restatement():
    """The sph_run_* path leaves the same kind of state as the fused step."""
    sc = scenes.SCENES["tiny_jitter"]()
    hip = scenes.hip_for(sc)
    hip.step(0)
    for st in scenes.STAGE_SEQUENCE:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    state = check_records(hip, what="staged")
    check_histograms(hip, state, masks=[(1, 2, 3)], what="staged")
    hip.close()


def test_three_tree_levels_on_more_than_a_million_particles():
    """More than 1024^2 particles: the third level of the reduction tree runs. The pressure-active 1.3 M box of the parity suite."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    assert sc["cfg"].particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    hip.step(0)
    check_records(hip, masks=[(1, 2, 3)], what="1.3M step 0")
    hip.step(1)
    hip.step(2)
    state = check_records(hip, what="1.3M step 2")
    assert diag_ref.selected(state, diag_ref.EVERYTHING, (1,)).sum() > 1024 * 1024  # three levels for the liquid alone, too
    check_histograms(hip, state, masks=[(1, 2, 3)], what="1.3M step 2")
    rec = hip.diagnostics()[0]
    assert rec[13] > 0 and rec[19] > 0
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_diagnostics_are_read_only():
    """Every exported buffer is unchanged by the calls, a solver that uses them every step ends bit-identical to an untouched twin,
    and a surface extracted before the calls still yields normals."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    cfg = sc["cfg"]
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    regions = np.array([diag_ref.EVERYTHING, (0, 0, 0, cfg.xmax / 2, INF, INF)], np.float32)
    for it in range(6):
        a.step(it)
        b.step(it)
        before = {n: a.buffer(n) for n in BUFFERS}
        verts, _ = a.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
        assert verts.shape[0] > 0
        a.diagnostics(regions, (1, 2, 3))
        a.histogram("neighbors", 0, 33, 33)
        a.histogram("density", 900, 1100, 4096, regions[1], (1,))
        normals = a.surface_normals()  # the mesh is still valid: the calls did not touch the state
        assert normals.shape == verts.shape and np.abs(normals).max() > 0
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    assert np.array_equal(a.buffer("neighborIds"), b.buffer("neighborIds"))
    a.close()
    b.close()


def _rc_diag(hip, regions, count, mask, null_regions=False, null_out=False):
    rg = np.ascontiguousarray(regions, np.float32)
    out = np.empty((max(count, 1), 32), np.float64)
    return hip._L.sph_diagnostics(hip._h, None if null_regions else rg.ctypes.data, count, mask, None if null_out else out.ctypes.data)


def _rc_hist(hip, field=0, lo=0.0, hi=1.0, bins=8, region=None, mask=0x6, null_out=False):
    out = np.empty(max(bins, 0) + 2, np.uint32)
    rg = None if region is None else np.ascontiguousarray(region, np.float32)
    return hip._L.sph_histogram(hip._h, field, lo, hi, bins, None if rg is None else rg.ctypes.data, mask,
                                None if null_out else out.ctypes.data)


def test_error_rules():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    every = np.array([diag_ref.EVERYTHING] * 17, np.float32)
    assert _rc_diag(hip, every, 1, 0x6) == ERR_ORDER  # a fresh solver
    assert _rc_hist(hip) == ERR_ORDER
    with pytest.raises(sphmi.SphError):
        hip.diagnostics()
    hip.step(0)
    assert _rc_diag(hip, every, 1, 0x6) == 0 and _rc_diag(hip, every, 16, 0xE) == 0 and _rc_hist(hip) == 0
    for st in scenes.STAGE_SEQUENCE[:7]:  # a new step has begun: its density and pressure-force stages have not run yet
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc_diag(hip, every, 1, 0x6) == ERR_ORDER and _rc_hist(hip) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    assert _rc_diag(hip, every, 1, 0x6) == 0 and _rc_hist(hip) == 0
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_diag(hip, every, 1, mask) == ERR_INVALID
        assert _rc_hist(hip, mask=mask) == ERR_INVALID
    for count in (0, -1, 17):
        assert _rc_diag(hip, every, count, 0x6) == ERR_INVALID
    assert _rc_diag(hip, every, 1, 0x6, null_regions=True) == ERR_INVALID
    assert _rc_diag(hip, every, 1, 0x6, null_out=True) == ERR_INVALID
    bad = every.copy()
    bad[2, 4] = np.nan
    assert _rc_diag(hip, bad, 2, 0x6) == 0  # the NaN is in a region the call does not use
    assert _rc_diag(hip, bad, 3, 0x6) == ERR_INVALID
    assert _rc_hist(hip, region=bad[2]) == ERR_INVALID
    assert _rc_hist(hip, region=every[0]) == 0
    assert _rc_hist(hip, null_out=True) == ERR_INVALID
    for bins in (0, -3, 4097):
        assert _rc_hist(hip, bins=bins) == ERR_INVALID
    assert _rc_hist(hip, bins=4096) == 0 and _rc_hist(hip, bins=1) == 0
    for field in (-1, 7):
        assert _rc_hist(hip, field=field) == ERR_INVALID
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf)):
        assert _rc_hist(hip, lo=lo, hi=hi) == ERR_INVALID
    with pytest.raises(sphmi.SphError):
        hip.histogram("vorticity", 0, 1, 4)
    with pytest.raises(sphmi.SphError):
        hip.diagnostics(np.zeros((17, 6), np.float32))
    assert b"sph_diagnostics" in hip._L.sph_last_error() or b"count" in hip._L.sph_last_error()
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_diag(hip, np.array([diag_ref.EVERYTHING], np.float32), 1, 0x6) == ERR_INVALID
    assert _rc_hist(hip) == ERR_INVALID
    hip.close()


def test_cpp_driver_diagnostics(tmp_path):
    """sphmi_run --diagnostics-every: the CSV's rows equal the Python call at the same steps; misuse exits with status 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    csv = str(tmp_path / "diag.csv")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    extra = [(0.0, 0.0, 0.0, 10.0, INF, INF), (-INF, 8.5, -INF, INF, 12.25, INF)]
    args = [exe] + box + ["--steps", "6", "--diagnostics-every", "2", "--diagnostics-out", csv]
    for r in extra:
        args += ["--diagnostics-region"] + [repr(float(x)) for x in r]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("_diagnostics: n ") == 3
    steps, got = frames.read_diagnostics_csv(csv)
    assert steps.tolist() == [2, 4, 6] and got.shape == (3, 3, 32)
    sc = scenes.SCENES["tiny"]()  # the same box
    hip = scenes.hip_for(sc)
    regions = np.array([diag_ref.EVERYTHING] + extra, np.float32)
    k = 0
    for it in range(6):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want = hip.diagnostics(regions, (1, 2))
            assert 0 < want[1, 0] < want[0, 0] and 0 < want[2, 0] < want[0, 0]
            assert_records(got[k], want, "csv rows of step %d" % (it + 1))
            k += 1
    hip.close()
    quiet = subprocess.run(args + ["--quiet"], capture_output=True, text=True, timeout=300)
    assert quiet.returncode == 0 and "_diagnostics" not in quiet.stdout
    for bad in (["--diagnostics-every", "2"], ["--diagnostics-out", csv], ["--diagnostics-every", "0", "--diagnostics-out", csv],
                ["--diagnostics-region", "0", "0", "0", "1", "1", "1"],
                ["--diagnostics-every", "1", "--diagnostics-out", csv, "--diagnostics-region", "0", "0", "0", "1", "1"],
                ["--diagnostics-every", "1", "--diagnostics-out", csv] + ["--diagnostics-region", "0", "0", "0", "1", "1", "1"] * 16):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
