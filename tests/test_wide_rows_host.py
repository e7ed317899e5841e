"""CPU premises of tests/test_wide_rows.py: the analysis kernels on neighbour rows that have no 16-bit copy.

findNeighbors marks a row it cannot store as 16-bit offsets (SPH_N16_WIDE) and its readers then take the 32-bit row. The step's
kernels and k_membranes are pinned to the oracle on such rows (tests/test_elastic_edges.py); the analysis kernels carry their own
copies of the branch (FmRow::id_wide in sph_forces.hip and sph_fields.hip, the wide arm of sph_row_for_each_slot under
sph_select.hip, sph_components.hip and sph_selector.h, hist_neighbor_count in sph_diag.hip). Which row is wide cannot be read
back, so the tests work with lower bounds derived from the oracle's buffers alone, on two inputs of scenes.elastic_hard_box:

  blob  N = 5,283; after steps 0 and 1 the particles with more than 96 others within h (scenes.crowded_particles): one of their
        two 48-entry candidate lists must overflow, so they are served by the exact walk and their rows are wide;
  bar   N = 32,538; after step 0 the fast-path rows whose offsets cannot fit 16 bits (scenes.certainly_wide_rows), wide unless the
        particle lost a staged cell, which debugCounters[0] counts on the GPU.

This file asserts, from the oracle's buffers and the numpy restatements the analysis tests already compare against, that
 (1) those sets are large enough and the states finite, and
 (2) each call of the GPU file is SENSITIVE to them: the restatement evaluated on rows whose certainly-wide rows are corrupted
     (scenes.corrupt_rows: "empty", every id -1; "shift", every id >= 0 replaced by min(id + 1, N - 1)) differs from the true result
     at, or because of, at least 50 of the certainly-wide particles. A kernel that mis-read those rows in either way would
     therefore fail the bit-for-bit comparison of the GPU file.
The inputs of the calls (dye, coefficient, regions, terms, view, link radius) are fixed here and imported by the GPU file.

What cannot be met as stated, and what stands in its place:
  * A count of entries >= 0 does not change when every id >= 0 is replaced by another id >= 0. The neighbour count, and with it
    select's field-3 term, histogram(3) and render's field 3, are therefore insensitive to "shift" by construction; the test
    asserts exactly that (zero changes) next to the "empty" condition, and the "shift" kind of error is caught on the same rows
    by the measure, the force records, the diffusion and the labelling.
  * No check here is elastic-only: the certainly-wide sets hold 17, 8 and 6 elastic particles, fewer than the 20 such a check
    would need. The elastic particles take part in every check through types=(1, 2).
  * Under "shift" the labelling changes, and the (root, members) of the components of at least 50 certainly-wide particles with
    it, but few particles change sides (seen: 38, 7 and 2), at every link radius tried: an off-by-one neighbour is mostly a near
    particle of the same cell, and the partner's row often holds the edge. 50 particles changing sides is asserted for "empty".
  * hist_neighbor_count has its own decoder; a decoder that counted one entry of each group of four four times would go unnoticed
    on full rows (count 32 either way), so test_rows_with_a_partly_filled_group asserts that enough certainly-wide rows have a
    group whose first entry does not speak for the other three."""
import functools
import types as _types

import numpy as np
import pytest

import scenes  # (first: it puts the package on the path)
import components_ref as cr
import diag_ref
import fields_ref as flr
import forces_ref as fr
import render_ref as rr
import select_ref as sr
import test_elastic_edges_host as H
from sphmi import frames

f32 = np.float32
INF = np.inf
STATES = ("blob0", "blob1", "bar0")
KINDS = ("empty", "shift")
ENOUGH = 50

# ---- the inputs of the calls, shared with tests/test_wide_rows.py ---------------------------------------------------------------
DIFFUSE_TYPES = (1, 2)
SUBSTEPS = (1, 3)
COUNT_TYPES = (1, 2, 3)  # the bar's boundary rows show only in the neighbour count
COUNT_TERM = [("neighbors", 1.0, 33.0)]  # at least one neighbour: an emptied row leaves the selection
HIST = (3, 0.0, 33.0, 33)
# the labelling: liquid and elastic matter, linked below 0.5 r0 = 0.835 (the dense matter stands 0.45 r0 apart, the lattice 0.93 r0):
# only dense particles link, and the blob's interior links through its own rows alone, all of them wide
# ... on the bar the certainly-wide rows belong to the lattice beside it: 1.6 is just above its spacing 0.93 r0 = 1.5531, so a particle
# links to its six nearest, and a block of emptied rows falls apart where no partner's row holds the edge
LABEL_TYPES = (1, 2)
LINK_RADIUS = {"blob0": 0.835, "blob1": 0.835, "bar0": 1.6}
IMAGE = (64, 64)
# spheres small enough that the matter behind shows between them, and a slab through the middle of the certainly-wide particles
# as the region, which lays a cross-section of the dense interior open: (radius, slab thickness) in r0
SPLAT = {"blob0": (0.12, 1.0), "blob1": (0.12, 1.0), "bar0": (0.25, 2.0)}


class CanonAsOracle:
    """The canonical buffers of scenes.canonical behind the `buffer(name)` of an oracle solver, for the *_ref.oracle_state
    helpers (the states come from the cache of test_elastic_edges_host.oracle_states, which keeps no solver)."""

    def __init__(self, canon):
        self.c = canon

    def buffer(self, name):
        if name == "neighborMap":
            return np.stack([self.c["neighborIds"].astype(np.float32), self.c["neighborDist"]], 1).reshape(-1)
        return self.c[name]


def dye(n):
    """A field in ORIGINAL-id order that is no smooth function of anything: a multiplicative hash of the id, in [0, 1)."""
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)
    return ((k >> np.uint64(22)).astype(np.float32) / f32(1024)).astype(np.float32)


def regions_of(box, cfg, count):
    """`count` regions: the box round the certainly-wide particles first, then everything, an empty one, one outside the scene and
    slabs along x."""
    out = [tuple(box), diag_ref.EVERYTHING, (5, 5, 5, 5, 6, 6), (-9, -9, -9, -1, -1, -1)]
    k = 0
    while len(out) < count:
        lo = f32(cfg.xmax) * f32(k) / f32(12)
        out.append((lo, -INF, -INF, lo + f32(cfg.xmax) / f32(12), INF, INF))
        k += 1
    return np.array(out[:count], np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """One state from the oracle's buffers: scene, canonical buffers, the certainly-wide sorted ids, the restatements' state and
    rows, the box round the certainly-wide particles and the fixed inputs derived from it."""
    if name.startswith("blob"):
        sc, states = H.oracle_states((("blob", True),), 2)
        canon = states[int(name[4:])]
        wide = scenes.crowded_particles(canon, sc["cfg"].h)
    else:
        sc, canon, wide, _ = H.bar_state()
    cfg = sc["cfg"]
    N = cfg.particleCount
    ora = CanonAsOracle(canon)
    state, ids, dist = fr.oracle_state(ora, N, cfg.gridCellCount)
    state2, rows = cr.oracle_state(ora, cfg)
    assert np.array_equal(rows, ids)
    state["ids"] = state2["ids"]
    state["h"], state["simScale"] = float(cfg.h), float(cfg.simulationScale)
    kind = np.trunc(state["types"]).astype(np.int64)
    r0 = f32(cfg.r0)
    p = state["pos"][wide[kind[wide] != 3]]  # (the bar's certainly-wide boundary rows lie at the far end of the box)
    box = tuple((p.min(0) - r0).astype(np.float32)) + tuple((p.max(0) + r0).astype(np.float32))
    c = _types.SimpleNamespace(name=name, sc=sc, cfg=cfg, N=N, canon=canon, wide=wide, state=state, ids=ids, dist=dist, kind=kind,
                               box=box, r0=r0)
    c.in_box = diag_ref.selected(state, box, DIFFUSE_TYPES)
    # the dye and a coefficient at half the stability limit of the TRUE rows
    c.dye = dye(N)
    D = flr.Diffusion(state, ids, dist, flr.constants(cfg), DIFFUSE_TYPES)
    c.coefficient = f32(0.5 / float((D.sD.astype(np.float64) * D.W.astype(np.float64))[D.P].max()))
    # an oblique orthographic view of the box
    radius, slab = SPLAT[name]
    lo, hi = np.array(box[:3], np.float64), np.array(box[3:], np.float64)
    mid = 0.5 * (lo + hi)
    c.view_kw = dict(bbox_min=lo, bbox_max=hi, width=IMAGE[0], height=IMAGE[1], eye=mid + np.array([0.3, 0.25, -1.0]) * 40.0, target=mid,
                     up=(0.0, 1.0, 0.0), perspective=False, radius=radius * float(r0), colour="field", field=3, lo=0.0, hi=32.0)
    zc = f32(np.median(p[:, 2]))
    c.view_region = box[:2] + (f32(zc - f32(0.5 * slab) * r0),) + box[3:5] + (f32(zc + f32(0.5 * slab) * r0),)
    return c


def view_of(c):
    return frames.render_view(**c.view_kw)


# ---- the restatements of the calls on given rows ----------------------------------------------------------------------------------
def evaluate(c, ids):
    """Every result the GPU file compares, from the restatements, on the neighbour ids `ids` (the true ones or corrupted ones)."""
    cfg, st = c.cfg, c.state
    out = _types.SimpleNamespace()
    out.F = fr.Forces(st, ids, c.dist, fr.constants(cfg))
    out.records = out.F.records
    K = flr.constants(cfg)
    D = flr.Diffusion(st, ids, c.dist, K, DIFFUSE_TYPES)
    out.diffused, out.sigma = {}, {}
    for n in SUBSTEPS:
        out.diffused[n], out.sigma[n], _ = flr.diffuse(st, ids, c.dist, K, c.dye, c.coefficient, n, DIFFUSE_TYPES, D)
    out.q = sr.Quantities(st, ids)
    out.measure, out.count = out.q.m, out.q.count
    out.surface = sr.select(st, out.q, None, (1,), [("surface", 0.10, INF)])
    out.by_count = sr.select(st, out.q, None, COUNT_TYPES, COUNT_TERM)
    out.hist = diag_ref.histogram(st, HIST[0], HIST[1], HIST[2], HIST[3], None, COUNT_TYPES, out.count)
    out.image = rr.render(st, view_of(c), c.view_region, COUNT_TYPES, False, float(cfg.rho0), None, out.count)
    out.labels, out.rc, out.bbox = cr.label_state(st, ids, LABEL_TYPES, LINK_RADIUS[c.name])
    return out


@functools.lru_cache(maxsize=None)
def evaluated(name, kind=None):
    c = case(name)
    return evaluate(c, c.ids if kind is None else scenes.corrupt_rows(c.ids, c.wide, kind))


def bits_differ(a, b):
    """bool[n]: rows of a and b that differ in any bit."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    d = a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)
    return d.any(1)


def membership(labels, rc):
    """int64[N, 2]: (root, members) of every particle's component, (-1, 0) where not selected: what a relabelling cannot hide."""
    out = np.full((labels.shape[0], 2), -1, np.int64)
    out[:, 1] = 0
    sel = labels >= 0
    out[sel] = rc[labels[sel]]
    return out


def sensitivity(name, kind):
    """For each call: how many certainly-wide particles the corruption shows at."""
    c, true, bad = case(name), evaluated(name), evaluated(name, kind)
    w = c.wide
    orig = c.state["ids"][w]
    out = {"records": int(bits_differ(true.records[w], bad.records[w]).sum()),
           "records in the box": int((bits_differ(true.records[w], bad.records[w]) & c.in_box[w]).sum()),
           "measure": int(bits_differ(true.measure[w], bad.measure[w]).sum()),
           "count": int((true.count[w] != bad.count[w]).sum()),
           "surface": int(np.isin(w, np.setxor1d(true.surface, bad.surface)).sum()),
           "by_count": int(np.isin(w, np.setxor1d(true.by_count, bad.by_count)).sum()),
           "hist": int(np.abs(true.hist.astype(np.int64) - bad.hist.astype(np.int64)).sum() // 2),
           "labels": int((membership(true.labels, true.rc)[w] != membership(bad.labels, bad.rc)[w]).any(1).sum())}
    for n in SUBSTEPS:
        out["diffused %d" % n] = int(bits_differ(true.diffused[n][orig], bad.diffused[n][orig]).sum())
    # the image: certainly-wide particles that win a pixel in both and whose pixel colour differs
    a, b = true.image, bad.image
    same_winner = (a["index"] == b["index"]) & (a["index"] >= 0)
    changed = same_winner & (a["rgba"] != b["rgba"]).any(2)
    out["image"] = int(np.intersect1d(np.unique(a["index"][changed]), w).size)
    return out


def separated(a, b, which):
    """How many of the particles `which` are, in labelling b, outside the b-component that holds most of their a-component: the
    particles a change of the rows splits off (a -> b) or merges in (b -> a), whatever it does to the numbering and the sizes."""
    sel = (a >= 0) & (b >= 0)
    Cb = int(b.max()) + 1
    pair, n = np.unique(a[sel].astype(np.int64) * Cb + b[sel], return_counts=True)
    order = np.lexsort((-n, pair // Cb))  # by a-component, the largest share first
    first = np.concatenate([[True], np.diff((pair // Cb)[order]) != 0])
    best = np.full(int(a.max()) + 1, -1, np.int64)
    best[(pair // Cb)[order][first]] = (pair % Cb)[order][first]
    w = which[sel[which]]
    return int((b[w] != best[a[w]]).sum())


# ---- (1) counts and finiteness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STATES)
def test_enough_certainly_wide_rows_and_finite_states(name):
    """Seen: blob after step 0: 418 (401 liquid, 17 elastic); after step 1: 179 (171, 8); bar after step 0: 285 (247 liquid,
    6 elastic, 32 boundary)."""
    c = case(name)
    by_type = np.bincount(c.kind[c.wide], minlength=4)
    print("%s: certainly wide %d, liquid %d, elastic %d, boundary %d" % (name, len(c.wide), by_type[1], by_type[2], by_type[3]))
    if name.startswith("blob"):
        assert by_type[1] >= 100 and by_type[2] >= 5, by_type
    else:
        assert len(c.wide) >= 200 and by_type[1] >= 150, by_type
        assert by_type[3] >= 20  # the rows only the neighbour count can show
    for k in ("position", "velocity", "sortedPosition", "sortedVelocity", "rho", "pressure", "acceleration"):
        assert np.isfinite(c.canon[k]).all(), (name, k)
    assert np.isfinite(evaluated(name).records).all() and np.isfinite(evaluated(name).measure).all()
    # the selection of the LIST instantiation and the region of the totals hold at least 50 of them
    assert int(c.in_box[c.wide].sum()) >= ENOUGH


@pytest.mark.parametrize("name", STATES)
def test_rows_with_a_partly_filled_group(name):
    """At least 50 certainly-wide rows have a group of four slots whose first entry is valid while another is not, so that a
    decoder which counted the first entry of a group four times would give another count (seen: 308, 126 and 189 rows; 44, 27
    and 55 of the certainly-wide rows are full)."""
    c = case(name)
    valid = c.ids[c.wide].reshape(-1, 8, 4) >= 0
    wrong = 4 * valid[:, :, 0].sum(1) != valid.sum((1, 2))
    print("%s: rows with a partly filled group %d of %d; full rows %d" % (name, wrong.sum(), len(c.wide), int(valid.all((1, 2)).sum())))
    assert int(wrong.sum()) >= ENOUGH


# ---- (2) sensitivity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", STATES)
def test_every_call_is_sensitive_to_the_certainly_wide_rows(name, kind):
    """Certainly-wide particles at which each result changes (blob after step 0 / after step 1 / bar; `empty`, then `shift`):
  force records, all of them inside the box     418 / 179 / 253 (the bar's other 32 are boundary: all-zero records)   the same
  diffused dye after 1 and after 3 substeps     418 / 179 / 253                                                       the same
  free-surface measure                          418 / 179 / 285                                                       the same
  select_surface (in one selection, not both)   252 /  67 / 159                                                       228 / 55 / 73
  neighbour count, select's field-3 term, bins  418 / 179 / 285                                                       0 by construction
  image: winners whose colour changes           158 /  98 / 188                                                       0 by construction
  labelling: (root, members) changes            380 / 178 / 253                                                       380 / 178 / 253
  labelling: split off their component          374 / 176 / 107                                                       38 / 7 / 2"""
    c, s = case(name), sensitivity(name, kind)
    print(name, kind, s)
    moving = int((c.kind[c.wide] != 3).sum())
    # a boundary particle's force record is all zero and it takes no part in the diffusion: every OTHER certainly-wide particle shows
    assert s["records"] == s["records in the box"] == moving >= ENOUGH
    for n in SUBSTEPS:
        assert s["diffused %d" % n] == moving
    assert s["measure"] >= ENOUGH and s["surface"] >= ENOUGH and s["labels"] >= ENOUGH
    if kind == "empty":
        # ... and the boundary ones in the neighbour count, with types=(1, 2, 3)
        assert s["count"] == s["by_count"] == s["hist"] == len(c.wide)
        assert s["image"] >= ENOUGH
    else:
        assert s["count"] == s["by_count"] == s["hist"] == s["image"] == 0  # (see the module's docstring)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", STATES)
def test_the_totals_and_the_tables_change_too(name, kind):
    """What is reduced from the per-particle results changes with them: the force totals and the dye's record of the box round the
    certainly-wide particles, and the labelling with its component table."""
    c, true, bad = case(name), evaluated(name), evaluated(name, kind)
    rg = regions_of(c.box, c.cfg, 1)
    a, b = (fr.diag_records(c.state, x.records, rg, DIFFUSE_TYPES) for x in (true, bad))
    assert a[0, 0] == b[0, 0] == c.in_box.sum() and int((a.view(np.uint64) != b.view(np.uint64)).sum()) >= 20
    for n in SUBSTEPS:
        a, b = (flr.diag_records(c.state, x.diffused[n][c.state["ids"]], rg, DIFFUSE_TYPES) for x in (true, bad))
        assert (a[0, 1:3].view(np.uint64) != b[0, 1:3].view(np.uint64)).all()  # the sum and the sum of squares
    assert not scenes.bits_equal(true.rc, bad.rc) or not scenes.bits_equal(true.labels, bad.labels)
    # split off (true -> corrupted) or merged in (corrupted -> true)
    moved = separated(true.labels, bad.labels, c.wide) + separated(bad.labels, true.labels, c.wide)
    print("%s %s: components %d -> %d, certainly-wide particles split off or merged in: %d" % (name, kind, true.rc.shape[0], bad.rc.shape[0], moved))
    if kind == "empty":
        assert moved >= ENOUGH
    else:
        # an off-by-one neighbour is usually a near particle of the same cell and the partner's row often holds the edge: the
        # labelling changes (asserted above and, at 50 particles, through (root, members)) but few particles change sides
        assert moved >= 1


def test_the_dye_is_not_smooth_and_the_coefficient_is_stable():
    for name in STATES:
        c, true = case(name), evaluated(name)
        d = c.dye[c.state["ids"]]
        assert np.unique(d).size > 500 and (np.diff(d) > 0).sum() > c.N // 4 and (np.diff(d) < 0).sum() > c.N // 4  # it goes up and down
        assert 0 < true.sigma[1] <= 0.5 and u32(true.sigma[1]) == u32(true.sigma[3])
        assert not scenes.bits_equal(true.diffused[1], c.dye) and not scenes.bits_equal(true.diffused[3], true.diffused[1])


def u32(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)[0]
