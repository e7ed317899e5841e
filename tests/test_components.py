"""GPU tests of the connected-component labelling (sph_label_components / sph_read_components / sph_component_diagnostics,
include/sphmi.h): labels, table, counts and per-component records bit-identical to the numpy restatement
(tests/components_ref.py), independent of launch order, read-only behaviour, the calling and lifetime rules and the driver's CSV.
No tolerance appears anywhere: integer arrays are compared for equality, floats and doubles as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
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
# Link radii in scene units (r0 = 1.67, h = 3.34, lattice spacings 0.93 r0 = 1.5531 and 0.85 r0 = 1.4195): +inf, h, two radii above
# every nearest-neighbour distance, a run through the spread of tiny_jitter's nearest-neighbour distances (the cubic lattice's
# bond-percolation threshold lies inside it), the lattice spacings themselves (pairs at r2 == link2 up to rounding), and two radii
# below the smallest pair distance of the lattice scenes. Chosen on the CPU from the oracle's neighbour rows with the restatement;
# the conditions they were chosen for are asserted in check_sweep_conditions.
RADII = [INF, 3.34, 2.004, 1.67, 1.5865, 1.5531, 1.5364, 1.5197, 1.503, 1.4696, 1.4195, 0.835, 0.167]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(u64(got), u64(want)):
        r, w = [int(x[0]) for x in np.nonzero(u64(got) != u64(want))]
        raise AssertionError("%s: %d words differ; first record %d word %d (%s): %r vs %r"
                             % (what, int((u64(got) != u64(want)).sum()), r, w, frames.DIAG_FIELDS[w], got[r, w], want[r, w]))


class Snapshot:
    """The state, the rows and the undirected row graph of the solver's last completed step (for the restatement)."""

    def __init__(self, hip):
        self.state = diag_ref.state_with_ids(hip)
        self.rows = cr.neighbor_rows(hip)
        self.graph = cr.graph(self.rows, self.state["pos"])

    def label(self, types, link):
        return cr.label_state(self.state, self.rows, types, link, self.graph)


def check_labelling(hip, snap, types, link, what):
    """One labelling against the restatement; returns (n_selected, C, size of the largest component) of the restatement."""
    labels, rc, bbox = snap.label(types, link)
    n_sel, C = int((labels >= 0).sum()), rc.shape[0]
    got_counts = hip.label_components(link, types)
    print("%s types %s link %r: selected %d components %d (library %r)" % (what, types, link, n_sel, C, got_counts))
    assert got_counts == (n_sel, C), (what, types, link)
    got_labels, got_rc, got_bbox = hip.components()
    assert got_labels.dtype == np.int32 and got_rc.dtype == np.int32 and got_bbox.dtype == np.float32
    assert got_labels.shape == (hip.N,) and got_rc.shape == (C, 2) and got_bbox.shape == (C, 6)
    assert np.array_equal(got_labels, labels), (what, types, link, np.flatnonzero(got_labels != labels)[:8])
    assert np.array_equal(got_rc, rc), (what, types, link, np.flatnonzero((got_rc != rc).any(1))[:8])
    assert np.array_equal(u32(got_bbox), u32(bbox)), (what, types, link, np.flatnonzero((u32(got_bbox) != u32(bbox)).any(1))[:8])
    assert int(got_rc[:, 1].sum()) == n_sel
    return n_sel, C, int(rc[:, 1].max()) if C else 0


def sweep(hip, what, cases):
    """Every type set and radius on the solver's current state; appends (types, link, n_selected, C, largest) to `cases`."""
    snap = Snapshot(hip)
    present = set(np.unique(snap.state["types"].astype(np.int32)).tolist())
    for types in MASKS:
        if not present & set(types):
            continue
        for link in RADII:
            n_sel, C, largest = check_labelling(hip, snap, types, link, what)
            cases.append((types, link, n_sel, C, largest))
    return snap


def check_sweep_conditions(name, cases):
    """No case passes vacuously: the sweep holds a properly mixed case, a fully split one and (tiny_jitter) several stages of
    the percolation transition."""
    assert any(1 < C < n and 1 < largest < n for _, _, n, C, largest in cases), name
    assert any(C == n and n > 0 for _, _, n, C, _ in cases), name
    assert any(C < n and link == INF for _, link, n, C, _ in cases), name
    if name == "tiny_jitter":
        liquid = sorted({C for types, _, n, C, _ in cases if types == (1,) and 1 < C < n})
        assert len(liquid) >= 3, liquid
        assert any(1 < C < n and 1 < largest < n // 2 for types, _, n, C, largest in cases if types == (1,))  # past the threshold


def _scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter", "tiny_compressed", "tiny_elastic", "worm"])
def test_labels_and_table_match_restatement(name):
    hip = scenes.hip_for(_scene(name))
    cases = []
    for it in range(5):
        hip.step(it)
        sweep(hip, "%s step %d" % (name, it), cases)
    check_sweep_conditions(name, cases)
    hip.close()


def test_staged_path_matches_restatement():
    """The sph_run_* path leaves the same kind of state and rows as the fused step."""
    hip = scenes.hip_for(scenes.SCENES["tiny_jitter"]())
    hip.step(0)
    for st in scenes.STAGE_SEQUENCE:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    cases = []
    sweep(hip, "staged", cases)
    check_sweep_conditions("tiny_jitter", cases)
    hip.close()


def two_bodies_scene():
    """tiny's box with lattice planes 4 and 5 along x removed: a gap of three spacings (4.66 > h = 3.34) between a body of
    4 x 10 x 12 and one of 6 x 10 x 12 liquid particles."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12))
    nl = sc["numOfLiquidP"]
    pos, vel = sc["position"], sc["velocity"]
    xs = np.unique(pos[:nl, 0])
    assert xs.size == 12 and 3 * float(xs[1] - xs[0]) > float(sc["cfg"].h)
    keep = np.ones(pos.shape[0], bool)
    keep[:nl] = ~np.isin(pos[:nl, 0], xs[4:6])
    sc["position"], sc["velocity"] = np.ascontiguousarray(pos[keep]), np.ascontiguousarray(vel[keep])
    sc["cfg"].particleCount = int(keep.sum())
    sc["numOfLiquidP"] = nl - 240
    return sc


def test_two_separated_bodies():
    hip = scenes.hip_for(two_bodies_scene())
    for it in range(3):
        hip.step(it)
        snap = Snapshot(hip)
        assert hip.label_components(INF, (1,)) == (1200, 2)
        labels, rc, bbox = hip.components()
        assert sorted(rc[:, 1].tolist()) == [480, 720]
        assert bbox[np.argmin(rc[:, 1]), 3] < bbox[np.argmax(rc[:, 1]), 0]  # the small body lies wholly below the large one in x
        check_labelling(hip, snap, (1,), INF, "two bodies step %d" % it)
        check_labelling(hip, snap, (1, 2), 3.34, "two bodies step %d" % it)
        # with the walls selected, the shell joins the bodies or not as the restatement says
        n_sel, C, largest = check_labelling(hip, snap, (1, 2, 3), INF, "two bodies step %d" % it)
        assert n_sel == hip.N and 1 <= C <= 3
        want_labels = snap.label((1, 2, 3), INF)[0]
        liquid = snap.state["types"].astype(np.int32) == 1
        got_labels = hip.components()[0]
        assert np.unique(got_labels[liquid]).size == np.unique(want_labels[liquid]).size
    hip.close()


def check_component_records(hip, snap, types, link, what):
    labels, rc, bbox = snap.label(types, link)
    assert hip.label_components(link, types) == (int((labels >= 0).sum()), rc.shape[0])
    got_labels, got_rc, got_bbox = hip.components()
    C = rc.shape[0]
    order = np.lexsort((np.arange(C), -rc[:, 1].astype(np.int64)))[:16]  # the 16 largest, then by id
    want = cr.component_records(snap.state, labels, order, hip.cfg.rho0)
    got = hip.component_diagnostics(order)
    assert_records(got, want, "%s types %s link %r, %d largest" % (what, types, link, order.size))
    assert np.array_equal(got[:, 0], got_rc[order, 1].astype(np.float64))  # word 0 is the table's n
    assert np.array_equal(u32(got[:, 23:29].astype(np.float32)), u32(got_bbox[order]))  # words 23..28 are the table's bbox
    assert np.array_equal(got[:, 23:29], got_bbox[order].astype(np.float64))
    assert np.array_equal(got[:, 21] >= got_rc[order, 0], np.ones(order.size, bool))  # the fastest member is not before the root
    for r in (0, order.size - 1):  # a record does not depend on the other ids of the call
        assert_records(hip.component_diagnostics([order[r]]), want[r:r + 1], "%s component %d alone" % (what, order[r]))
    rep = [order[0], order[-1], order[0], order[0]]
    assert_records(hip.component_diagnostics(rep), want[[0, order.size - 1, 0, 0]], "%s repeated ids" % what)
    if C > 16:  # the smallest and the last component, too
        ids = [int(np.argmin(rc[:, 1])), C - 1]
        assert_records(hip.component_diagnostics(ids), cr.component_records(snap.state, labels, ids, hip.cfg.rho0), "%s small" % what)
    return C, int(rc[:, 1].max())


@pytest.mark.parametrize("name", ["tiny_jitter", "tiny_elastic", "tiny_compressed"])
def test_component_diagnostics_match_restatement(name):
    hip = scenes.hip_for(_scene(name))
    for it in range(5):
        hip.step(it)
    snap = Snapshot(hip)
    seen = []
    for types, link in (((1,), 1.5197), ((1, 2), 1.503), ((1, 2, 3), 1.5364), ((1, 2, 3), INF), ((1,), 0.167)):
        seen.append(check_component_records(hip, snap, types, link, name))
    assert any(C > 16 and largest > 1 for C, largest in seen)
    # one component: its record is the diagnostics record of everything with the same types, bit for bit
    assert hip.label_components(INF, (1,))[1] == 1
    assert_records(hip.component_diagnostics([0]), hip.diagnostics(None, (1,)), name + " single component")
    rec = hip.component_diagnostics([0])[0]
    assert rec[10] > 0 and rec[20] > 0 and rec[22] >= 0  # the fluid moves after five steps
    s = frames.diagnostics_summary(rec, hip.cfg)
    assert s["n"] == int(rec[0]) and s["kinetic_energy"] > 0
    hip.close()


def test_launch_independence_and_unrelated_calls():
    """Labelling twice, and labelling after unrelated read-only calls, gives identical arrays; a labelling survives those calls;
    a mesh extracted before still yields normals afterwards."""
    sc = scenes.SCENES["tiny_jitter"]()
    hip = scenes.hip_for(sc)
    cfg = sc["cfg"]
    for it in range(3):
        hip.step(it)
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    verts, _ = hip.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
    assert verts.shape[0] > 0
    for link in (1.5197, INF):
        counts = hip.label_components(link, (1, 2, 3))
        first = hip.components()
        rec = hip.component_diagnostics([0, counts[1] - 1])
        assert hip.label_components(link, (1, 2, 3)) == counts
        for a, b in zip(first, hip.components()):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        hip.diagnostics(None, (1,))
        hip.histogram("neighbors", 0, 33, 33)
        hip.sample_grid(origin, np.full(3, h, np.float32), [5, 4, 6])
        hip.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
        for a, b in zip(first, hip.components()):  # the labelling is still there ...
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert_records(hip.component_diagnostics([0, counts[1] - 1]), rec, "after unrelated calls")  # ... and still valid
        assert hip.label_components(link, (1, 2, 3)) == counts
        for a, b in zip(first, hip.components()):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        normals = hip.surface_normals()  # labelling does not invalidate the mesh
        assert normals.shape == verts.shape and np.abs(normals).max() > 0
    assert counts[1] == 2 and 1 < first[1][:, 1].max() < counts[0]
    hip.close()


def test_more_than_a_million_particles():
    """More than 1024^2 particles (the pressure-active 1.3 M box of the parity suite): the scan runs over more than 4096 blocks
    and the records' reduction tree has three levels."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    assert sc["cfg"].particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    snap = Snapshot(hip)
    n_sel, C, largest = check_labelling(hip, snap, (1, 2, 3), INF, "1.3M")
    assert n_sel == hip.N and 1 <= C < 16
    check_component_records(hip, snap, (1, 2, 3), INF, "1.3M")
    n_sel, C, largest = check_labelling(hip, snap, (1,), 1.4195, "1.3M")
    assert n_sel > 1024 * 1024 and 16 < C < n_sel and 1 < largest < n_sel
    check_component_records(hip, snap, (1,), 1.4195, "1.3M")
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_components_are_read_only():
    """Every exported buffer is unchanged by the three calls, and a solver that labels every step ends bit-identical to an
    untouched twin."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(6):
        a.step(it)
        b.step(it)
        before = {n: a.buffer(n) for n in BUFFERS}
        for link, types in ((INF, (1, 2)), (1.5364, (1, 2, 3))):
            n_sel, C = a.label_components(link, types)
            assert C >= 1
            a.components()
            a.component_diagnostics(list(range(min(C, 16))))
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    assert np.array_equal(a.buffer("neighborIds"), b.buffer("neighborIds"))
    a.close()
    b.close()


def _rc_label(hip, link=INF, mask=0x6, null_counts=False):
    counts = np.full(2, -7, np.int64)
    rc = hip._L.sph_label_components(hip._h, link, mask, None if null_counts else counts.ctypes.data)
    return rc, counts.tolist()


def _rc_read(hip):
    labels = np.empty(hip.N, np.int32)
    return hip._L.sph_read_components(hip._h, labels.ctypes.data, None, None)


def _rc_cdiag(hip, ids, count=None, null_ids=False, null_out=False):
    comp = np.ascontiguousarray(ids, np.int32)
    out = np.empty((max(comp.size, 1), 32), np.float64)
    return hip._L.sph_component_diagnostics(hip._h, None if null_ids else comp.ctypes.data, comp.size if count is None else count,
                                            None if null_out else out.ctypes.data)


def test_error_and_lifetime_rules():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    assert _rc_label(hip) == (ERR_ORDER, [0, 0])  # a fresh solver
    assert _rc_read(hip) == ERR_ORDER and _rc_cdiag(hip, [0]) == ERR_ORDER
    with pytest.raises(sphmi.SphError):
        hip.label_components()
    with pytest.raises(sphmi.SphError):
        hip.components()
    hip.step(0)
    assert _rc_read(hip) == ERR_ORDER and _rc_cdiag(hip, [0]) == ERR_ORDER  # stepped, but never labelled
    assert _rc_label(hip) == (0, [1440, 1])
    assert _rc_read(hip) == 0 and _rc_cdiag(hip, [0]) == 0
    # invalid arguments; a failed labelling leaves none behind
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_label(hip, mask=mask) == (ERR_INVALID, [0, 0])
        assert _rc_read(hip) == ERR_ORDER and _rc_cdiag(hip, [0]) == ERR_ORDER
        assert _rc_label(hip)[0] == 0
    for link in (0.0, -1.0, -INF, np.nan):
        assert _rc_label(hip, link=link) == (ERR_INVALID, [0, 0])
        assert _rc_read(hip) == ERR_ORDER
    assert _rc_label(hip, null_counts=True)[0] == ERR_INVALID
    assert _rc_label(hip, link=1e-30) == (0, [1440, 1440])  # any positive radius is legal
    assert _rc_label(hip, link=3e38, mask=0xE)[0] == 0  # (link2 overflows to +inf: every finite r2 is below it)
    assert _rc_label(hip, mask=0x4) == (0, [0, 0])  # no elastic particle in this scene: zero selected is legal
    labels, rc, bbox = hip.components()
    assert (labels == -1).all() and rc.shape == (0, 2) and bbox.shape == (0, 6)
    assert _rc_cdiag(hip, [0]) == ERR_INVALID  # no component 0
    assert _rc_label(hip, link=1.5531, mask=0xE)[0] == 0
    C = hip.label_components(1.5531, (1, 2, 3))[1]
    assert C > 16
    assert _rc_cdiag(hip, list(range(16))) == 0 and _rc_cdiag(hip, [C - 1]) == 0
    for ids in ([C], [-1], [0, C], [0, 1, -5]):
        assert _rc_cdiag(hip, ids) == ERR_INVALID
    for count in (0, -1, 17):
        assert _rc_cdiag(hip, list(range(17)), count=count) == ERR_INVALID
    assert _rc_cdiag(hip, [0], null_ids=True) == ERR_INVALID and _rc_cdiag(hip, [0], null_out=True) == ERR_INVALID
    with pytest.raises(sphmi.SphError):
        hip.component_diagnostics(list(range(17)))
    assert b"sph_component_diagnostics" in hip._L.sph_last_error()
    # lifetime: the arrays survive further steps, the records do not
    old = hip.components()
    hip.step(1)
    assert _rc_cdiag(hip, [0]) == ERR_ORDER
    for a, b in zip(old, hip.components()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert hip.label_components(1.5531, (1, 2, 3))[1] > 16 and _rc_cdiag(hip, [0]) == 0
    hip._runClearBuffers()  # any stage call: a new step has begun
    assert _rc_cdiag(hip, [0]) == ERR_ORDER and _rc_read(hip) == 0
    for st in scenes.STAGE_SEQUENCE[1:7]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc_label(hip) == (ERR_ORDER, [0, 0])  # the new step's density and pressure-force stages have not run yet
    assert _rc_read(hip) == ERR_ORDER  # ... and the failed call has dropped the old labelling
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(2) if st == "integrate" else m()
    assert _rc_label(hip)[0] == 0 and _rc_cdiag(hip, [0]) == 0
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_label(hip) == (ERR_INVALID, [0, 0])
    assert _rc_read(hip) == ERR_ORDER and _rc_cdiag(hip, [0]) == ERR_ORDER
    hip.close()


def test_labels_in_original_order():
    """frames.labels_in_original_order puts each particle's label beside it: the members of a component, looked up in the
    orig-order type column, have the selected types, and the per-component member counts are the table's."""
    sc = scenes.SCENES["tiny_elastic"]()
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    n_sel, C = hip.label_components(1.5364, (1, 2))
    labels, rc, _ = hip.components()
    orig = frames.labels_in_original_order(labels, hip.read_particleIndex_buffer())
    types = sc["position"][:, 3].astype(np.int32)
    assert np.array_equal(orig >= 0, (types == 1) | (types == 2)) and int((orig >= 0).sum()) == n_sel
    assert np.array_equal(np.bincount(orig[orig >= 0], minlength=C), rc[:, 1])
    s = frames.component_summary(rc, hip.components()[2], hip.cfg.mass)
    assert s["components"] == C and s["largest_n"] == rc[:, 1].max() and s["outside_largest"] == n_sel - s["largest_n"]
    hip.close()


def test_cpp_driver_components(tmp_path):
    """sphmi_run --components-every: the CSV's rows equal the Python calls at the same steps; misuse exits with status 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    csv = str(tmp_path / "components.csv")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    args = [exe] + box + ["--steps", "4", "--components-every", "2", "--components-out", csv, "--components-link", "1.5531",
                          "--components-types", "1", "2", "3", "--components-top", "5"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("_components: selected ") == 2
    steps, ids, rc, bbox, rec = frames.read_components_csv(csv)
    assert steps.tolist() == [2] * 5 + [4] * 5
    hip = scenes.hip_for(scenes.SCENES["tiny"]())  # the same box
    k = 0
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2:
            continue
        n_sel, C = hip.label_components(1.5531, (1, 2, 3))
        _, want_rc, want_bbox = hip.components()
        assert C > 5 and 1 < want_rc[:, 1].max() < n_sel
        order = np.lexsort((np.arange(C), -want_rc[:, 1].astype(np.int64)))[:5]
        assert ("_components: selected %d  components %d  largest %d  outside it %d" %
                (n_sel, C, want_rc[order[0], 1], n_sel - want_rc[order[0], 1])) in r.stdout
        assert ids[k:k + 5].tolist() == order.tolist()
        assert np.array_equal(rc[k:k + 5], want_rc[order])
        assert np.array_equal(u32(bbox[k:k + 5]), u32(want_bbox[order]))
        assert_records(rec[k:k + 5], hip.component_diagnostics(order), "csv rows of step %d" % (it + 1))
        k += 5
    hip.close()
    # the defaults: liquid + elastic, every row entry, up to 16 components
    dflt = subprocess.run([exe] + box + ["--steps", "1", "--components-every", "1", "--components-out", csv, "--quiet"],
                          capture_output=True, text=True, timeout=300)
    assert dflt.returncode == 0 and "_components" not in dflt.stdout
    steps, ids, rc, bbox, rec = frames.read_components_csv(csv)
    assert steps.tolist() == [1] and ids.tolist() == [0] and rc.tolist() == [[rc[0, 0], 1440]] and rec[0, 0] == 1440
    for bad in (["--components-every", "2"], ["--components-out", csv], ["--components-every", "0", "--components-out", csv],
                ["--components-link", "1.5"], ["--components-top", "3"], ["--components-types", "1"],
                ["--components-every", "1", "--components-out", csv, "--components-link", "0"],
                ["--components-every", "1", "--components-out", csv, "--components-link", "-2"],
                ["--components-every", "1", "--components-out", csv, "--components-top", "0"],
                ["--components-every", "1", "--components-out", csv, "--components-top", "17"],
                ["--components-every", "1", "--components-out", csv, "--components-types"],
                ["--components-every", "1", "--components-out", csv, "--components-types", "4"]):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
