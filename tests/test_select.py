"""GPU tests of particle selection, the surface measure and the compact read-back (sph_particle_measure / sph_select_particles /
sph_read_selection, include/sphmi.h): the measure, the selected indices, the original ids and the records bit-identical to the
numpy restatement (tests/select_ref.py), consistent with the existing analysis calls on the same state, read-only, the calling
and lifetime rules, and the driver's files. No tolerance appears anywhere: integer arrays are compared for equality, floats as
bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import diag_ref
import scenes
import select_ref as sr
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
MASKS = [(1,), (1, 2), (1, 2, 3)]
INF = np.inf
f32 = np.float32
SCENE_NAMES = ["tiny", "tiny_jitter", "tiny_compressed", "tiny_elastic", "worm", "alias16", "wide"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


class Snapshot:
    """The state, the rows and the restatement's per-particle quantities of the solver's last completed step."""

    def __init__(self, hip):
        self.state = diag_ref.state_with_ids(hip)
        self.rows = cr.neighbor_rows(hip)
        self.q = sr.Quantities(self.state, self.rows)


def check_measure(hip, snap, what):
    got = hip.particle_measure()
    assert got.dtype == np.float32 and got.shape == (hip.N,)
    bad = np.flatnonzero(u32(got) != u32(snap.q.m))
    assert bad.size == 0, "%s: measure differs at %d particles; first %d: %r vs %r" % (what, bad.size, bad[0], got[bad[0]], snap.q.m[bad[0]])
    assert ((got >= 0) & (got <= 1.0 + 1e-6)).all()


def check_selection(hip, snap, what, region=None, types=(1, 2), terms=(), component=None, labels=None):
    """One selection against the restatement; returns the number selected."""
    want = sr.select(snap.state, snap.q, region, types, terms, component, labels)
    n = hip.select(region, types, terms, component)
    tag = "%s region %r types %r terms %r component %r" % (what, region, types, terms, component)
    assert n == want.size, (tag, n, want.size)
    idx, ids, rec = hip.selection()
    assert idx.dtype == np.int32 and ids.dtype == np.uint32 and rec.dtype == np.float32
    assert idx.shape == (n,) and ids.shape == (n,) and rec.shape == (n, sphmi.SELECT_WORDS)
    assert np.array_equal(idx, want), (tag, np.flatnonzero(idx != want)[:8])
    assert (np.diff(idx) > 0).all()
    want_ids, want_rec = sr.records(snap.state, snap.q, want)
    assert np.array_equal(ids, want_ids), tag
    diff = u32(rec) != u32(want_rec)
    assert not diff.any(), "%s: %d record words differ; first record %d word %d: %r vs %r" % (
        (tag, int(diff.sum())) + tuple(int(x[0]) for x in np.nonzero(diff)) + (rec[diff][0], want_rec[diff][0]))
    return n


def quantile_bounds(values):
    """(lo, hi) float32 around the middle of the finite values; hi = +inf where the quartiles coincide."""
    v = np.sort(np.asarray(values, np.float32)[np.isfinite(values)])
    if v.size == 0:
        return f32(0), f32(INF)
    lo, hi = v[v.size // 4], v[(3 * v.size) // 4]
    return (lo, hi) if lo < hi else (lo, f32(INF))


def sweep(hip, what, cases, label_every=True):
    """Type sets x boxes, one term per field, conjunctions and a component filter on the solver's current state; appends
    (kind, types, n, n of the type set, N) to `cases`."""
    snap = Snapshot(hip)
    check_measure(hip, snap, what)
    st, q = snap.state, snap.q
    present = set(np.unique(st["types"].astype(np.int32)).tolist())
    N = hip.N
    for types in MASKS:
        if not present & set(types):
            continue
        everything = diag_ref.selected(st, diag_ref.EVERYTHING, types)
        total = int(everything.sum())
        p = st["pos"][everything]
        lo, hi = np.quantile(p, 0.3, axis=0).astype(np.float32), np.quantile(p, 0.7, axis=0).astype(np.float32)
        boxes = [None, tuple(lo) + tuple(hi), (lo[0], -INF, -INF, lo[0], INF, INF), (-INF, lo[1], -INF, INF, INF, hi[2])]
        for box in boxes:
            n = check_selection(hip, snap, what, box, types)
            cases.append(("box", types, n, total, N))
            if box is None:
                assert n == total
        for field in range(8):
            b = quantile_bounds(q.field(field)[everything])
            n = check_selection(hip, snap, what, None, types, [(field, b[0], b[1])])
            cases.append(("term%d" % field, types, n, total, N))
        bx, bs = quantile_bounds(q.field("x")[everything]), quantile_bounds(q.field("surface")[everything])
        n = check_selection(hip, snap, what, boxes[3], types, [("x", bx[0], INF), ("surface", -INF, bs[1] if np.isfinite(bs[1]) else 2.0)])
        cases.append(("two", types, n, total, N))
        four = [("density", -INF, INF), ("neighbors", 1, 33), ("z", -INF, hi[2]), ("surface", 0.0, 0.5)]
        n = check_selection(hip, snap, what, boxes[3], types, four)
        cases.append(("four", types, n, total, N))
    if 1 in present:
        nl = int(diag_ref.selected(st, diag_ref.EVERYTHING, (1,)).sum())
        n = check_selection(hip, snap, what, None, (1,), [("surface", 0.10, INF)])
        assert n == hip.select_surface()
        cases.append(("surface", (1,), n, nl, N))
    if label_every:
        types = (1, 2, 3) if 3 in present else (1, 2)
        n_sel, C = hip.label_components(1.5531, types)
        labels, rc, bbox = hip.components()
        for c in sorted({0, C // 2, C - 1, int(np.argmax(rc[:, 1]))}):
            n = check_selection(hip, snap, what, None, types, (), c, labels)
            assert n == rc[c, 1]
            cases.append(("component", types, n, n_sel, N))
        n = check_selection(hip, snap, what, None, (1, 2), [("surface", 0.05, INF)], int(np.argmax(rc[:, 1])), labels)
        cases.append(("component+term", types, n, n_sel, N))
    return snap


def check_sweep_conditions(name, cases):
    """No case passes vacuously."""
    assert any(0 < n < N // 2 for _, _, n, _, N in cases), name
    assert any(n == 0 for _, _, n, _, _ in cases), name
    assert any(n == total and total > 0 for kind, _, n, total, _ in cases if kind == "box"), name
    assert any(kind == "surface" and 0 < n < total for kind, _, n, total, _ in cases), name
    assert any(kind.startswith("term") and 0 < n < total for kind, _, n, total, _ in cases), name
    assert any(kind in ("two", "four") and n > 0 for kind, _, n, _, _ in cases), name


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_measure_and_selections_match_restatement(name):
    hip = scenes.hip_for(_scene(name))
    cases = []
    for it in range(5):
        hip.step(it)
        sweep(hip, "%s step %d" % (name, it), cases, label_every=it in (0, 4))
    check_sweep_conditions(name, cases)
    hip.close()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_staged_path_matches_restatement(name):
    """The sph_run_* path leaves the same kind of state and rows as the fused step."""
    hip = scenes.hip_for(_scene(name))
    cases = []
    for it in range(5):
        staged_step(hip, it)
        if it in (0, 4):
            sweep(hip, "%s staged step %d" % (name, it), cases, label_every=it == 4)
        else:
            check_measure(hip, Snapshot(hip), "%s staged step %d" % (name, it))
    check_sweep_conditions(name, cases)
    hip.close()


@pytest.mark.parametrize("name", ["tiny_jitter", "tiny_elastic"])
def test_consistent_with_the_other_analysis_calls(name):
    hip = scenes.hip_for(_scene(name))
    for it in range(4):
        hip.step(it)
    snap = Snapshot(hip)
    st = snap.state
    p = st["pos"]
    box = tuple(np.quantile(p, 0.2, axis=0).astype(np.float32)) + tuple(np.quantile(p, 0.8, axis=0).astype(np.float32))
    for types in MASKS:
        for region in (None, box):
            n = hip.select(region, types)
            assert n == int(hip.diagnostics(None if region is None else [region], types)[0, 0]) and n > 0
            for field in range(7):
                v = snap.q.field(field)[np.isfinite(snap.q.field(field))]
                lo, hi = f32(np.quantile(v, 0.2)), f32(np.quantile(v, 0.9))
                if not lo < hi:
                    hi = f32(lo + f32(1.0))
                hist = hip.histogram(field, lo, hi, 7, region, types)
                assert hip.select(region, types, [(field, lo, hi)]) == int(hist[1:-1].sum()), (types, region, field)
                assert hip.select(region, types, [(field, -INF, lo)]) == int(hist[0]), (types, region, field)
                assert hip.select(region, types, [(field, hi, INF)]) == int(hist[-1]), (types, region, field)
    # the records are the exported buffers at sortedIndex
    n = hip.select(box, (1, 2, 3), [("surface", 0.02, INF)])
    idx, ids, rec = hip.selection()
    assert 0 < n < hip.N
    sp = hip.buffer("sortedPosition").reshape(-1, 4)[:hip.N]
    sv = hip.buffer("sortedVelocity").reshape(-1, 4)
    pi = hip.read_particleIndex_buffer()
    assert np.array_equal(u32(rec[:, :3]), u32(sp[idx, :3])) and np.array_equal(u32(rec[:, 4:7]), u32(sv[idx, :3]))
    assert np.array_equal(u32(rec[:, 7]), u32(hip.buffer("rho")[:hip.N][idx])) and np.array_equal(u32(rec[:, 8]), u32(hip.buffer("pressure")[idx]))
    assert np.array_equal(u32(rec[:, 7]), u32(hip.read_density_buffer()[idx]))
    assert np.array_equal(ids, pi[idx, 1]) and np.array_equal(u32(rec[:, 3]), u32(hip.read_position_buffer()[ids, 3]))
    assert np.array_equal(rec[:, 9], (snap.rows[idx] >= 0).sum(1).astype(np.float32))
    assert np.array_equal(u32(rec[:, 10]), u32(hip.particle_measure()[idx])) and (u32(rec[:, 11]) == 0).all()
    # a component selection is the component table's row
    n_sel, C = hip.label_components(1.5364, (1, 2, 3))
    labels, rc, bbox = hip.components()
    assert C > 3
    order = np.argsort(-rc[:, 1].astype(np.int64), kind="stable")
    for c in (int(order[0]), int(order[1]), int(order[-1])):
        assert hip.select(None, (1, 2, 3), (), c) == rc[c, 1]
        idx, ids, rec = hip.selection()
        assert idx[0] == rc[c, 0] and np.array_equal(idx, np.flatnonzero(labels == c))
        got_box = np.concatenate([rec[:, :3].min(0), rec[:, :3].max(0)]) + f32(0.0)
        assert np.array_equal(u32(got_box), u32(bbox[c]))
    # ... intersected with the types of the selection, not of the labelling
    c = int(order[0])
    assert hip.select(None, (1,), (), c) == int(((labels == c) & (st["types"].astype(np.int32) == 1)).sum())
    hip.close()


def test_every_call_selects_the_same_particles_at_a_bound_on_a_particle():
    """diagnostics, force_diagnostics, histogram, select and selection count the same particles, the restatement's number, for
    boxes whose x bound is exactly the float32 x of a selected particle: as a lower bound it holds the particle, as an upper bound
    it does not, one float above as an upper bound it does again."""
    hip = scenes.hip_for(_scene("tiny_jitter"))
    for it in range(3):
        hip.step(it)
    snap = Snapshot(hip)
    st = snap.state
    for types in MASKS:
        sel = np.flatnonzero(diag_ref.selected(st, diag_ref.EVERYTHING, types))
        p = st["pos"][sel].astype(np.float32)
        j = int(sel[np.argsort(p[:, 0], kind="stable")[sel.size // 3]])  # a selected particle a third of the way along x
        x = f32(st["pos"][j, 0])
        up = np.nextafter(x, f32(INF))
        z0, z1 = f32(np.quantile(p[:, 2], 0.3)), f32(np.quantile(p[:, 2], 0.6))
        far = f32(p.max() + 100)
        regions = np.array([(-INF, -INF, -INF, INF, INF, INF),
                            (x, -INF, -INF, INF, INF, INF),    # the particle is inside
                            (-INF, -INF, -INF, x, INF, INF),   # ... outside
                            (-INF, -INF, -INF, up, INF, INF),  # ... inside again
                            (-INF, -INF, z0, INF, INF, z1),    # infinite on two axes
                            (far, far, far, far + 100, far + 100, far + 100)], np.float32)  # empty
        want = [sr.select(st, snap.q, tuple(r), types, (), None, None) for r in regions]
        n_diag = hip.diagnostics(regions, types)[:, 0]
        n_force = hip.force_diagnostics(regions, types)[:, 0]
        for r, region in enumerate(regions):
            arg = None if r == 0 else tuple(region)
            n_hist = int(hip.histogram("x", 0.0, 10.0, 16, arg, types).sum())
            n_sel = hip.select(arg, types)
            idx = hip.selection()[0]
            got = (int(n_diag[r]), int(n_force[r]), n_hist, n_sel, int(idx.size))
            print("types %r region %d: diagnostics, force_diagnostics, histogram, select, selection = %r; restatement %d"
                  % (types, r, got, want[r].size))
            assert got == (want[r].size,) * 5, (types, r, got, want[r].size)
            assert np.array_equal(idx, want[r]), (types, r)
            assert (j in idx.tolist()) == (r in (0, 1, 3)) or r == 4, (types, r, j)
        n = [w.size for w in want]
        assert n[0] == sel.size and n[1] + n[2] == n[0] and 0 < n[4] < n[0]  # no case passes vacuously
        assert n[3] - n[2] >= 1 and n[1] > 0 and n[2] > 0  # they differ by the particle on the bound
        assert n[5] == 0
    hip.close()


def test_more_than_a_million_particles():
    """More than 1024^2 particles (the pressure-active 1.3 M box of the parity suite): the scan runs over more than 4096 blocks.
    Selections of 0, 1, all and about half of the particles."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    assert sc["cfg"].particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    snap = Snapshot(hip)
    check_measure(hip, snap, "1.3M")
    assert (hip.N + 255) // 256 > 4096
    assert check_selection(hip, snap, "1.3M", None, (1, 2, 3)) == hip.N
    assert check_selection(hip, snap, "1.3M", None, (2,)) == 0
    assert check_selection(hip, snap, "1.3M", None, (1,), [("density", 1e9, INF)]) == 0
    liquid = np.flatnonzero(snap.state["types"].astype(np.int32) == 1)
    j = int(liquid[liquid.size // 3])
    x = snap.state["pos"][j]
    one = tuple(x) + tuple(np.nextafter(x, f32(INF)))
    assert check_selection(hip, snap, "1.3M", one, (1, 2, 3)) == 1
    assert hip.selection()[0].tolist() == [j]
    med = f32(np.median(snap.state["pos"][:, 0]))
    n = check_selection(hip, snap, "1.3M", None, (1, 2, 3), [("x", -INF, med)])
    assert hip.N // 3 < n < 2 * hip.N // 3
    n = check_selection(hip, snap, "1.3M", None, (1,), [("surface", 0.10, INF)])
    assert 0 < n < liquid.size // 4
    n = check_selection(hip, snap, "1.3M", None, (1,), [("neighbors", 32, 33), ("pressure", -INF, INF), ("z", med, INF), ("speed", -INF, INF)])
    assert n > 0
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_selection_is_read_only():
    """Every exported buffer, a mesh, a labelling and the following steps are unchanged by the three calls."""
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    for it in range(6):
        a.step(it)
        b.step(it)
        verts, _ = a.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
        normals = a.surface_normals()
        n_sel, C = a.label_components(1.5364, (1, 2, 3))
        comp = a.components()
        rec = a.component_diagnostics([0, C - 1])
        before = {n: a.buffer(n) for n in BUFFERS}
        a.particle_measure()
        assert a.select(None, (1, 2, 3), [("surface", 0.1, INF), ("neighbors", 0, 33)]) > 0
        first = a.selection()
        assert a.select(None, (1, 2), (), C - 1) >= 0
        a.selection()
        assert a.select_surface() > 0
        a.selection()
        assert a.select(None, (1, 2, 3), [("surface", 0.1, INF), ("neighbors", 0, 33)]) == first[0].size  # twice: the same arrays
        for x, y in zip(first, a.selection()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
        assert np.array_equal(a.surface_normals().view(np.uint32), normals.view(np.uint32))  # the mesh is still valid
        for x, y in zip(comp, a.components()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(a.component_diagnostics([0, C - 1]).view(np.uint64), rec.view(np.uint64))  # ... and the labelling
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    assert np.array_equal(a.buffer("neighborIds"), b.buffer("neighborIds"))
    a.close()
    b.close()


def _rc_select(hip, region=None, mask=0x6, terms=(), count=None, component=-1, null_count=False, null_terms=False):
    import ctypes as C
    arr = (sphmi.SphSelectTerm * max(len(terms), 1))()
    for k, (f, lo, hi) in enumerate(terms):
        arr[k].field, arr[k].lo, arr[k].hi = f, lo, hi
    rg = None if region is None else np.ascontiguousarray(region, np.float32)
    out = np.full(1, -7, np.int64)
    rc = hip._L.sph_select_particles(hip._h, None if rg is None else rg.ctypes.data, mask, None if null_terms else C.cast(arr, C.c_void_p),
                                     len(terms) if count is None else count, component, None if null_count else out.ctypes.data)
    return rc, int(out[0])


def _rc_read(hip, n=4096):
    idx = np.empty(max(n, 1), np.int32)
    ids = np.empty(max(n, 1), np.uint32)
    rec = np.empty((max(n, 1), 12), np.float32)
    return hip._L.sph_read_selection(hip._h, idx.ctypes.data, ids.ctypes.data, rec.ctypes.data)


def _rc_measure(hip, null=False):
    out = np.empty(hip.N, np.float32)
    return hip._L.sph_particle_measure(hip._h, None if null else out.ctypes.data)


def test_error_and_lifetime_rules():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    N = hip.N
    assert _rc_select(hip) == (ERR_ORDER, 0)  # a fresh solver
    assert _rc_read(hip) == ERR_ORDER and _rc_measure(hip) == ERR_ORDER
    with pytest.raises(sphmi.SphError):
        hip.select()
    with pytest.raises(sphmi.SphError):
        hip.selection()
    with pytest.raises(sphmi.SphError):
        hip.particle_measure()
    hip.step(0)
    assert _rc_read(hip) == ERR_ORDER  # stepped, but nothing selected yet
    assert _rc_measure(hip) == 0 and _rc_measure(hip, null=True) == ERR_INVALID
    assert _rc_select(hip) == (0, 1440) and _rc_read(hip) == 0
    assert hip._L.sph_read_selection(hip._h, None, None, None) == 0  # any pointer may be NULL
    assert _rc_select(hip, null_count=True)[0] == ERR_INVALID
    assert _rc_read(hip) == ERR_ORDER  # a failed selection leaves none behind
    for mask in (0, 1, 0x10, 0x80000002):  # a bad typeMask
        assert _rc_select(hip)[0] == 0
        assert _rc_select(hip, mask=mask) == (ERR_INVALID, 0) and _rc_read(hip) == ERR_ORDER
    assert _rc_select(hip, region=(0, 0, np.nan, 1, 1, 1)) == (ERR_INVALID, 0)  # a NaN region bound
    assert _rc_select(hip, region=(5, 5, 5, 1, 1, 1)) == (0, 0)  # an empty region is legal ...
    assert _rc_read(hip, 0) == 0 and hip.selection()[2].shape == (0, 12)  # ... and so is reading nothing
    assert _rc_select(hip, terms=[(0, 0.0, 1.0)] * 5) == (ERR_INVALID, 0)  # termCount outside 0..4
    assert _rc_select(hip, count=-1) == (ERR_INVALID, 0)
    assert _rc_select(hip, terms=[(0, 0.0, 1.0)], null_terms=True) == (ERR_INVALID, 0)  # null terms with termCount > 0
    assert _rc_select(hip, count=0, null_terms=True) == (0, 1440)
    assert _rc_select(hip, terms=[(0, 0.0, INF)] * 4)[0] == 0
    for field in (-1, 8):  # a field outside 0..7
        assert _rc_select(hip, terms=[(field, 0.0, 1.0)]) == (ERR_INVALID, 0)
    for lo, hi in ((np.nan, 1.0), (0.0, np.nan), (1.0, 1.0), (2.0, 1.0), (INF, INF)):  # a NaN bound or lo >= hi
        assert _rc_select(hip, terms=[(7, lo, hi)]) == (ERR_INVALID, 0)
    assert _rc_select(hip, terms=[(7, -INF, INF)]) == (0, 1440)
    assert _rc_select(hip, component=-2) == (ERR_INVALID, 0)  # component < -1
    assert _rc_select(hip, component=0) == (ERR_ORDER, 0)  # no labelling at all
    C = hip.label_components(1.5531, (1, 2, 3))[1]
    assert C > 16
    assert _rc_select(hip, mask=0xE, component=C) == (ERR_INVALID, 0) and _rc_select(hip, mask=0xE, component=C - 1)[0] == 0
    assert _rc_select(hip, mask=0x8) == (0, int(hip.diagnostics(None, (3,))[0, 0])) and N > 1440
    assert _rc_select(hip, mask=0x4) == (0, 0)  # no elastic particle in this scene: zero selected is legal
    # lifetime: the selection gathers from the live state
    assert _rc_select(hip, terms=[(7, 0.1, INF)]) == (0, 640) and _rc_read(hip) == 0
    hip.step(1)
    assert _rc_read(hip) == ERR_ORDER  # after a step
    assert _rc_select(hip, component=0) == (ERR_ORDER, 0)  # the labelling belongs to the previous state
    assert _rc_select(hip)[0] == 0 and _rc_read(hip) == 0
    hip._runClearBuffers()  # any stage call: a new step has begun
    assert _rc_read(hip) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[1:7]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc_select(hip) == (ERR_ORDER, 0) and _rc_measure(hip) == ERR_ORDER  # density and pressure force have not run yet
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(2) if st == "integrate" else m()
    assert _rc_select(hip) == (0, 1440) and _rc_read(hip) == 0 and _rc_measure(hip) == 0
    with pytest.raises(sphmi.SphError):
        hip.select(terms=[("nonsense", 0, 1)])
    with pytest.raises(sphmi.SphError):
        hip.select(terms=[("x", 0, 1)] * 5)
    assert b"sph_select_particles" in hip._L.sph_last_error()
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_select(hip) == (ERR_INVALID, 0)
    assert _rc_measure(hip) == ERR_INVALID and _rc_read(hip) == ERR_ORDER
    hip.close()


def test_cpp_driver_selection(tmp_path):
    """sphmi_run --select-*: the files equal the Python calls at the same steps; misuse exits with status 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    out = str(tmp_path)
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    runs = {
        "surface": (["--select-surface", "0.1"], dict(types=(1,), terms=[("surface", 0.1, INF)])),
        "terms": (["--select-types", "1", "3", "--select-region", "-inf", "0", "0", "inf", "9", "inf", "--select-term", "neighbors", "20", "33",
                   "--select-term", "6", "-inf", "12.5"],
                  dict(region=(-INF, 0, 0, INF, 9, INF), types=(1, 3), terms=[("neighbors", 20, 33), ("z", -INF, 12.5)])),
    }
    hip = scenes.hip_for(scenes.SCENES["tiny"]())  # the same box
    want = {}
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            for key, (_, kw) in runs.items():
                n = hip.select(**kw)
                want[key, it + 1] = (n,) + hip.selection()
    hip.close()
    for key, (flags, _) in runs.items():
        d = os.path.join(out, key)
        os.makedirs(d)
        r = subprocess.run([exe] + box + ["--steps", "4", "--select-every", "2", "--select-out", d] + flags, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(d)) == ["selection_2.bin", "selection_4.bin"]
        for step in (2, 4):
            n, idx, ids, rec = want[key, step]
            assert 0 < n < 1440 + 2000 and ("_select: selected %d of " % n) in r.stdout
            gi, gd, gr = frames.read_selection(os.path.join(d, "selection_%d.bin" % step))
            assert np.array_equal(gi, idx) and np.array_equal(gd, ids) and np.array_equal(u32(gr), u32(rec)), (key, step)
    d = os.path.join(out, "quiet")
    os.makedirs(d)
    r = subprocess.run([exe] + box + ["--steps", "1", "--select-every", "1", "--select-out", d, "--quiet"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "_select" not in r.stdout
    assert frames.read_selection(os.path.join(d, "selection_1.bin"))[0].size == 1440  # the default: all the liquid
    for bad in (["--select-every", "2"], ["--select-out", d], ["--select-every", "0", "--select-out", d], ["--select-surface", "0.1"],
                ["--select-types", "1"], ["--select-every", "1", "--select-out", d, "--select-types"],
                ["--select-every", "1", "--select-out", d, "--select-types", "4"],
                ["--select-every", "1", "--select-out", d, "--select-term", "vorticity", "0", "1"],
                ["--select-every", "1", "--select-out", d, "--select-term", "x", "2", "1"],
                ["--select-every", "1", "--select-out", d, "--select-term", "x", "nan", "1"],
                ["--select-every", "1", "--select-out", d, "--select-region", "0", "0", "nan", "1", "1", "1"],
                ["--select-every", "1", "--select-out", d] + ["--select-term", "x", "0", "1"] * 5):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
