"""GPU tests of the analysis kernels on neighbour rows that have no 16-bit copy: force_measure (both
instantiations) and force_diagnostics, field_diffuse with field_read and field_diagnostics, particle_measure and select_surface,
select with a term on the neighbour count, histogram of the neighbour count, render coloured by it, and label_components with
components and component_diagnostics, on four states in which findNeighbors certainly leaves such rows: the blob form of
scenes.elastic_hard_box after a fused step 0, after a fused step 1 and after a staged step 0 (rows of the exact walk), and the bar
form after a fused step 0 (rows of the fast path whose offsets do not fit 16 bits).

Per state: first the canonical buffers against the oracle's and the counters that say the wide paths were taken, then every call
against its numpy restatement, every word bit for bit, and once more on the certainly-wide rows alone. The restatements are
evaluated on the oracle's buffers (tests/test_wide_rows_host.py, which also asserts that each comparison here is sensitive to a
wrong read of exactly those rows); the first test of each state makes them the solver's. No tolerance appears anywhere."""
import types as _types

import numpy as np
import pytest

import components_ref as cr
import diag_ref
import fields_ref as flr
import forces_ref as fr
import scenes
import test_components as tc
import test_render as tr
import test_select as ts
import test_wide_rows_host as W
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip

pytestmark = pytest.mark.gpu

# GPU state -> (the host file's state, steps, staged?)
GPU_STATES = {"blob after fused step 0": ("blob0", 1, False), "blob after fused step 1": ("blob1", 2, False),
              "blob after staged step 0": ("blob0", 1, True), "bar after fused step 0": ("bar0", 1, False)}
NO_COPY = "certainly-wide rows (no 16-bit copy)"


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def first_diff64(got, want):
    d = np.argwhere(u64(got) != u64(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


@pytest.fixture(scope="module", params=list(GPU_STATES))
def live(request):
    """One solver per state, brought there the way the oracle's state was made (a muscle update after every step), with the
    counters before and after the last step."""
    name, steps, staged = GPU_STATES[request.param]
    c = W.case(name)
    hip = scenes.hip_for(c.sc)
    hip.field_create(1)
    before = np.zeros(8, np.int64)
    for it in range(steps):
        before = hip.buffer("debugCounters")[:8].astype(np.int64)
        if staged:
            scenes.staged_step(hip, it)
        else:
            hip.step(it)
        hip.updateMuscleActivityData(scenes.hard_muscle_signal(it))
    after = hip.buffer("debugCounters")[:8].astype(np.int64)
    want = W.evaluated(name)
    snap = _types.SimpleNamespace(state=c.state, q=want.q, rows=c.ids, counts=want.count, rho0=float(c.cfg.rho0),
                                  label=lambda types, link: (want.labels, want.rc, want.bbox))
    yield _types.SimpleNamespace(what=request.param, name=name, staged=staged, c=c, hip=hip, want=want, snap=snap, before=before, after=after)
    hip.close()


def assert_rows_equal(got, want, what, c, index=None, view=u32):
    """Whole arrays bit for bit (row r of both belongs to sorted particle index[r], default r), then the certainly-wide rows alone."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    index = np.arange(got.shape[0]) if index is None else np.asarray(index)
    bad = np.flatnonzero((view(got).reshape(got.shape[0], -1) != view(want).reshape(got.shape[0], -1)).any(1))
    at_wide = np.isin(index, c.wide)
    if bad.size:
        raise AssertionError("%s: %d rows differ, %d of them %s; first at sorted particle %d: %r vs %r" % (
            what, bad.size, int(at_wide[bad].sum()), NO_COPY, index[bad[0]], got[bad[0]], want[bad[0]]))
    assert at_wide.sum() >= W.ENOUGH, (what, int(at_wide.sum()))
    assert np.array_equal(view(got[at_wide]), view(want[at_wide])), "%s on the %s" % (what, NO_COPY)


def test_state_equals_the_oracles_and_the_wide_paths_were_taken(live):
    c, hip = live.c, live.hip
    assert_same(canon_hip(hip, c.N), c.canon, live.what, () if live.staged else FUSED_SKIP)
    before, after = live.before, live.after
    print("%s: debugCounters[0..3] = %s (before the step %s), certainly wide %d" % (live.what, after[:4].tolist(), before[:4].tolist(), len(c.wide)))
    if live.name.startswith("blob"):  # exact walks of this step: a cell not staged, or a list overflowed
        walked = int(after[0] + after[1] - before[0] - before[1])
        assert walked >= len(c.wide) >= 100, (walked, len(c.wide))
    else:  # fast-path rows whose offsets do not fit, unless the particle lost a staged cell
        assert int(after[2]) >= len(c.wide) - int(after[0]) >= 150, after[:4].tolist()


def test_force_measure_both_instantiations(live):
    c, hip, want = live.c, live.hip, live.want
    rec = hip.force_measure()
    assert rec.dtype == np.float32 and rec.shape == (c.N, 40)
    assert_rows_equal(rec, want.records, live.what + " force records", c)
    # the LIST instantiation on the box round the certainly-wide particles
    index = np.flatnonzero(c.in_box).astype(np.int32)
    assert hip.select(c.box, W.DIFFUSE_TYPES) == index.size
    assert np.array_equal(hip.selection()[0], index)
    got = hip.force_measure(selection=True)
    assert_rows_equal(got, want.records[index], live.what + " force records of the selection", c, index)
    assert np.abs(got[:, 0:9]).max() > 0 and (got[:, 27:30].sum(1) > 0).all()  # every selected particle used a slot


@pytest.mark.parametrize("count", [1, 16])
def test_force_diagnostics(live, count):
    c, hip = live.c, live.hip
    rg = W.regions_of(c.box, c.cfg, count)
    got = hip.force_diagnostics(rg, W.DIFFUSE_TYPES)
    want = fr.diag_records(c.state, live.want.records, rg, W.DIFFUSE_TYPES)
    assert got.dtype == np.float64 and got.shape == (count, 64)
    assert np.array_equal(u64(got), u64(want)), "%s totals of %d regions: %s" % (live.what, count, first_diff64(got, want))
    assert got[0, 0] == c.in_box.sum() and np.abs(got[0, 1:28]).max() > 0


@pytest.mark.parametrize("substeps", W.SUBSTEPS)
def test_field_diffuse_read_and_diagnostics(live, substeps):
    c, hip, want = live.c, live.hip, live.want
    orig = c.state["ids"]
    hip.field_write(1, c.dye)
    sigma = hip.field_diffuse(1, c.coefficient, substeps, W.DIFFUSE_TYPES)
    got = hip.field_read(1)
    assert u32([sigma])[0] == u32([want.sigma[substeps]])[0], (live.what, sigma, want.sigma[substeps])
    # (in sorted order, so that a row is a sorted particle's)
    assert_rows_equal(got[orig], want.diffused[substeps][orig], "%s dye after %d substeps" % (live.what, substeps), c)
    assert np.array_equal(u32(got), u32(want.diffused[substeps]))
    for count in (1, 16):
        rg = W.regions_of(c.box, c.cfg, count)
        rec = hip.field_diagnostics(1, rg, W.DIFFUSE_TYPES)
        want_rec = flr.diag_records(c.state, want.diffused[substeps][orig], rg, W.DIFFUSE_TYPES)
        assert np.array_equal(u64(rec), u64(want_rec)), "%s dye records of %d regions: %s" % (live.what, count, first_diff64(rec, want_rec))


def test_particle_measure_and_select_surface(live):
    c, hip, want = live.c, live.hip, live.want
    assert_rows_equal(hip.particle_measure(), want.measure, live.what + " measure", c)
    ts.check_measure(hip, live.snap, live.what)
    n = ts.check_selection(hip, live.snap, live.what, None, (1,), [("surface", 0.10, np.inf)])
    assert n == hip.select_surface() == want.surface.size
    assert np.array_equal(hip.selection()[0], want.surface)
    assert np.intersect1d(want.surface, c.wide).size >= 20 and np.setdiff1d(c.wide, want.surface).size >= 20  # on both sides


def test_select_by_neighbour_count(live):
    """A term on field 3 (sph_neighbor_count): the records carry the count (word 9) and the measure (word 10) of every selected
    particle, the certainly-wide ones among them."""
    c, hip, want = live.c, live.hip, live.want
    for terms in (W.COUNT_TERM, [("neighbors", 24.0, 33.0)], [("neighbors", 0.0, 24.0), ("surface", 0.0, 0.5)]):
        n = ts.check_selection(hip, live.snap, live.what, None, W.COUNT_TYPES, terms)
        assert n > 0
    n = ts.check_selection(hip, live.snap, live.what, None, W.COUNT_TYPES, W.COUNT_TERM)
    index, _, rec = hip.selection()
    assert n == want.by_count.size and np.isin(c.wide, index).all()
    assert_rows_equal(rec[:, 9:11], np.stack([want.count, want.measure], 1)[index], live.what + " count and measure of the selection", c, index)


def test_histogram_of_the_neighbour_count(live):
    c, hip, want = live.c, live.hip, live.want
    field, lo, hi, bins = W.HIST
    got = hip.histogram(field, lo, hi, bins, None, W.COUNT_TYPES)
    assert got.dtype == np.uint32 and np.array_equal(got, want.hist), (live.what, np.flatnonzero(got != want.hist)[:8])
    assert int(got.sum()) == c.N and got[0] == 0 and got[bins + 1] == 0
    # ... and of the box round the certainly-wide particles alone, where they are most of what is counted
    got = hip.histogram(field, lo, hi, bins, c.box, W.COUNT_TYPES)
    want_box = diag_ref.histogram(c.state, field, lo, hi, bins, c.box, W.COUNT_TYPES, want.count)
    assert np.array_equal(got, want_box), "%s in the box round the %s: bins %s" % (live.what, NO_COPY, np.flatnonzero(got != want_box)[:8])
    assert int(got.sum()) >= (c.kind[c.wide] != 3).sum() >= W.ENOUGH


def test_render_coloured_by_the_neighbour_count(live):
    c, hip = live.c, live.hip
    view = W.view_of(c)
    want = tr.check_render(hip, live.snap, view, live.what, c.view_region, W.COUNT_TYPES, False, None)
    got = hip.rendered()
    won = np.isin(want["index"], c.wide)
    assert np.intersect1d(np.unique(want["index"]), c.wide).size >= W.ENOUGH
    assert np.array_equal(got["rgba"][won], want["rgba"][won]), "%s: colours of the %s" % (live.what, NO_COPY)
    assert np.unique(want["rgba"][won].reshape(-1, 4), axis=0).shape[0] > 8  # many counts, many shades


def test_components_table_and_records(live):
    c, hip, want = live.c, live.hip, live.want
    link = W.LINK_RADIUS[live.name]
    n_sel, C, largest = tc.check_labelling(hip, live.snap, W.LABEL_TYPES, link, live.what)
    assert 1 < C < n_sel and largest > 100
    labels, rc, bbox = hip.components()
    assert_rows_equal(labels, want.labels, live.what + " labels", c, view=lambda a: a.view(np.uint32))
    tc.check_component_records(hip, live.snap, W.LABEL_TYPES, link, live.what)
    # the components the certainly-wide particles belong to
    ids = np.unique(want.labels[c.wide][want.labels[c.wide] >= 0])[:16]
    tc.assert_records(hip.component_diagnostics(ids), cr.component_records(c.state, want.labels, ids, c.cfg.rho0),
                      "%s components of the %s" % (live.what, NO_COPY))
