"""GPU tests of the probes (sph_probes_set_points / sph_probes_set_lines / sph_probes_count / sph_probes_record / sph_probes_history /
sph_probes_read_history, include/sphmi.h): every word of every point and level record equal to the numpy restatement
(tests/probe_ref.py) and to sph_sample_points, on the line cases tests/test_probe_host.py proves to hold what they claim
(tests/probe_cases.py); independence of the lines' order and number; the tie to marching cubes' vertices; the ring; the life of the
definitions across steps, edits and pose changes; the calling rules. Floats are compared as bit patterns throughout."""
import re

import numpy as np
import pytest

import probe_cases as pc
import probe_ref as pr
import sample_cases
import sample_ref
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
NAN, INF = np.nan, np.inf


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), "%s: %s" % (what, scenes.diff_report(got, want))


def status_of(call):
    """The library's status of a wrapper call: 0, or the code in the SphError."""
    try:
        call()
    except sphmi.SphError as e:
        return int(re.search(r"\(status (-?\d+)\)", str(e)).group(1))
    return 0


def device_fields(hip, lines):
    """f_k of every line from a host loop over sph_sample_points: probe_ref.line_fields with the device's sampler."""
    out = []
    for ln in lines:
        rec = hip.sample_points(pr.line_points(ln), pr.mask_types(ln["typeMask"]))
        out.append(rec[:, int(ln["field"])].copy())
    return out


def points_of(sc, state):
    """Point probes: inside the liquid, outside it, in the air gap, at particles, outside the box, non-finite."""
    r0 = f32(sc["cfg"].r0)
    fixed = np.array([[7.1, 6.0, 7.3], [7.1, 9.9, 7.3], [7.1, 12.5, 7.3], [1.0, 1.0, 1.0], [-3.0, 5.0, 40.0], [0.0, 0.0, 0.0]], f32) * r0
    at = state["pos"][[0, 17, state["pos"].shape[0] // 2, -1]]
    odd = np.array([[NAN, 5.0, 5.0], [5.0, INF, 5.0], [5.0, 5.0, -INF], [NAN, NAN, NAN], [3.0e38, 5.0, 5.0]], f32)
    rng = np.random.default_rng(11)
    spread = rng.uniform(-1.0, 17.0, (300, 3)).astype(f32) * r0  # more than one block of the point kernel
    return np.concatenate([fixed, at, odd, spread]).astype(f32)


@pytest.fixture(scope="module")
def box():
    sc = pc.scene()
    hip = scenes.hip_for(sc)
    for it in range(pc.STEPS):
        hip.step(it)
    state = sample_ref.solver_state(hip)
    cases = pc.build(sc["cfg"], state)
    lines = pc.all_lines(cases)
    fields = pr.line_fields(state, lines)
    want = pr.level_records(state, lines, fields)
    pc.check_claims(cases, want, fields)  # (on this state too: the host test made them on the oracle's)
    yield dict(sc=sc, hip=hip, state=state, cases=cases, lines=lines, want=want)
    hip.close()


# ---------------------------------------------------------------------------------------------- every word, bit for bit
def test_level_records(box):
    hip, lines = box["hip"], box["lines"]
    hip.probes_set_points(None)
    hip.probes_set_lines(lines)
    assert hip.probes_count() == (0, lines.shape[0])
    pts, got = hip.probes_record()
    assert pts.shape == (0, 8)
    for name, s in pc.spans(box["cases"]).items():
        assert_bits(got[s], box["want"][s], "case %r against the restatement" % name)
    assert_bits(got, pr.level_records(None, lines, device_fields(hip, lines)), "against a host loop over sph_sample_points")
    assert set(got[:, 4].tolist()) == {0.0, 1.0, 2.0} and (got[:, 7][got[:, 4] != 0] == 0).all()
    # a second call on the same state gives the same records
    assert_bits(hip.probes_record()[1], got, "second call")


@pytest.mark.parametrize("types", [(1,), (3,), (1, 2, 3)])
def test_point_records(box, types):
    hip, state = box["hip"], box["state"]
    pts = points_of(box["sc"], state)
    hip.probes_set_lines(None)
    hip.probes_set_points(pts, types)
    assert hip.probes_count() == (pts.shape[0], 0)
    got, lev = hip.probes_record()
    assert lev.shape == (0, 8)
    assert_bits(got, hip.sample_points(pts, types), "against sph_sample_points")
    assert_bits(got, pr.point_records(state, pts, types), "against the restatement")
    if 1 in types:
        assert got[0, 6] > 10 and got[2, 6] == 0 and not got[10:15].any()
    if types == (1, 2, 3):
        assert (got[6:10, 6] >= 1).all()  # at a particle


def test_points_and_lines_in_one_call(box):
    hip, state, lines = box["hip"], box["state"], box["lines"]
    pts = points_of(box["sc"], state)
    hip.probes_set_points(pts, (1, 2, 3))
    hip.probes_set_lines(lines)
    gp, gl = hip.probes_record()
    assert_bits(gp, pr.point_records(state, pts, (1, 2, 3)), "points beside lines")
    assert_bits(gl, box["want"], "lines beside points")


@pytest.mark.parametrize("types", [(1,), (1, 2, 3)])
def test_ring_scene_edge_queries(types):
    """The queries at the support boundary to the ulp, across cell faces and at negative coordinates (tests/sample_cases.py)."""
    sc = sample_cases.ring_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)
    state = sample_ref.solver_state(hip)
    pts = sc["queries"][0]
    hip.probes_set_points(pts, types)
    got, _ = hip.probes_record()
    assert_bits(got, hip.sample_points(pts, types), "against sph_sample_points")
    assert_bits(got, pr.point_records(state, pts, types), "against the restatement")
    # ... and as two-point lines from each query to itself moved by h: f_K and f_{K+1} are samples at the queries
    h = f32(sc["cfg"].h)
    lines = np.concatenate([pc.line(p, (0.0, 0.0, h), 2, field=0, iso=f32(1e-30), mask=sphmi.type_mask(types)) for p in pts[:200]])
    hip.probes_set_lines(lines)
    assert_bits(hip.probes_record()[1], pr.level_records(state, lines), "two-point lines")
    hip.close()


# ---------------------------------------------------------------------------------------------- order and number of the lines
def test_order_independence(box):
    hip, lines, want = box["hip"], box["lines"], box["want"]
    hip.probes_set_points(None)
    perm = np.random.default_rng(3).permutation(lines.shape[0])
    hip.probes_set_lines(lines[perm])
    assert_bits(hip.probes_record()[1], want[perm], "shuffled")
    for i in range(lines.shape[0]):
        hip.probes_set_lines(lines[i:i + 1])
        assert_bits(hip.probes_record()[1], want[i:i + 1], "line %d alone" % i)


# ---------------------------------------------------------------------------------------------- marching cubes
def test_levels_are_marching_cubes_vertices(box):
    hip, sc = box["hip"], box["sc"]
    r0 = f32(sc["cfg"].r0)
    o, s, d = (f32(2.0) * r0, f32(2.0) * r0, f32(2.0) * r0), (r0, r0, f32(0.75) * r0), (12, 11, 17)
    verts, _ = hip.extract_surface(o, s, d, iso=0.5, field="shepard", types=(1,))
    lines = frames.level_columns(o, s, d, axis=2, field="shepard", iso=0.5, types=(1,))
    hip.probes_set_points(None)
    hip.probes_set_lines(lines)
    rec = hip.probes_record()[1]
    found = np.flatnonzero(rec[:, 4] == pr.FOUND)
    assert found.size > 40 and (rec[:, 4] == pr.DRY).any()
    vb = bits(verts)
    for i in found:
        col = lines["origin"][i]
        on = (vb[:, 0] == bits(col[0:1])[0]) & (vb[:, 1] == bits(col[1:2])[0])  # the z-edge vertices of this column (and none above them)
        assert on.any(), i
        top = verts[on][np.argmax(verts[on][:, 2])]
        assert np.array_equal(bits(rec[i, :3]), bits(top)), (i, rec[i], top)


# ---------------------------------------------------------------------------------------------- history
def _probed(sc, lines, pts):
    hip = scenes.hip_for(sc)
    hip.probes_set_points(pts, (1, 2, 3))
    hip.probes_set_lines(lines)
    return hip


def test_history(box):
    sc, lines = box["sc"], np.concatenate([l for n, l in box["cases"] if n in ("counts", "faces", "dry", "masks")])
    pts = points_of(sc, box["state"])[:40]
    a, b = _probed(sc, lines, pts), _probed(sc, lines, pts)
    assert status_of(lambda: a.probe_history(0, 1)) == ERR_ORDER  # no ring
    a.probes_history(3)
    blocking = []
    for it in range(5):
        a.step(it)
        b.step(it)
        assert a.probes_record(read=False) is None
        blocking.append(b.probes_record())
    hp, hl = a.probe_history(2, 3)
    assert hp.shape == (3, 40, 8) and hl.shape == (3, lines.shape[0], 8)
    for k in range(3):
        assert_bits(hp[k], blocking[2 + k][0], "points of call %d" % (2 + k))
        assert_bits(hl[k], blocking[2 + k][1], "levels of call %d" % (2 + k))
    assert not np.array_equal(bits(hl[0]), bits(hl[2]))  # the states differ
    assert_bits(a.probe_history(4, 1)[1][0], blocking[4][1], "the newest alone")
    assert_bits(frames.probe_series(hl, "y")[:, 0], np.array([blocking[k][1][0, 1] for k in (2, 3, 4)], f32), "a series")
    for first, count in ((1, 1), (1, 3), (2, 4), (5, 1), (-1, 1)):
        assert status_of(lambda: a.probe_history(first, count)) == ERR_INVALID, (first, count)
    calls = np.zeros(1, np.int64)
    assert a._L.sph_probes_read_history(a._h, 0, 0, None, None, calls.ctypes.data) == 0 and calls[0] == 5
    # a new set restarts the ring: call 4 is gone, call 5 is readable once made
    a.probes_set_points(pts[:7], (1,))
    assert status_of(lambda: a.probe_history(4, 1)) == ERR_INVALID
    a.probes_record(read=False)
    b.probes_set_points(pts[:7], (1,))
    want = b.probes_record()
    hp, hl = a.probe_history(5, 1)
    assert_bits(hp[0], want[0], "points after the new set")
    assert_bits(hl[0], want[1], "levels after the new set")
    assert status_of(lambda: a.probe_history(4, 2)) == ERR_INVALID
    # a new ring restarts it too; releasing it brings SPH_ERR_ORDER back
    a.probes_history(2)
    assert status_of(lambda: a.probe_history(5, 1)) == ERR_INVALID
    a.probes_history(0)
    assert status_of(lambda: a.probe_history(5, 1)) == ERR_ORDER
    a.close()
    b.close()


def test_history_byte_cap(box):
    hip = scenes.hip_for(box["sc"])
    rows_max = sphmi.PROBE_HISTORY_MAX
    assert status_of(lambda: hip.probes_history(rows_max + 1)) == ERR_INVALID and status_of(lambda: hip.probes_history(-1)) == ERR_INVALID
    per_row = sphmi.PROBE_HISTORY_BYTES // rows_max // 32  # records a row may hold at the largest ring: 512
    hip.probes_set_points(np.zeros((per_row + 1, 3), f32))
    assert status_of(lambda: hip.probes_history(rows_max)) == ERR_INVALID
    hip.probes_history(rows_max // 2)  # (513 records a row: 8192 rows fit)
    hip.probes_set_points(np.zeros((per_row, 3), f32))
    hip.probes_history(rows_max)  # exactly 1 << 28 bytes
    # a set that would push the existing ring over the cap is refused and nothing changes
    one = pc.line((0, 0, 0), (0, 0, 1), 2)
    assert status_of(lambda: hip.probes_set_lines(one)) == ERR_INVALID and hip.probes_count() == (per_row, 0)
    assert status_of(lambda: hip.probes_set_points(np.zeros((per_row + 1, 3), f32))) == ERR_INVALID and hip.probes_count() == (per_row, 0)
    hip.probes_history(0)
    hip.probes_set_lines(one)
    assert hip.probes_count() == (per_row, 1)
    hip.close()


# ---------------------------------------------------------------------------------------------- lifetime
def test_probes_outlive_steps_edits_and_poses(box):
    sc = box["sc"]
    r0 = float(sc["cfg"].r0)
    lines = np.concatenate([l for n, l in box["cases"] if n in ("counts", "faces", "masks")])
    pts = points_of(sc, box["state"])[:60]
    hip = _probed(sc, lines, pts)

    def check(what):
        gp, gl = hip.probes_record()
        assert_bits(gp, hip.sample_points(pts, (1, 2, 3)), what + ": points")
        assert_bits(gl, pr.level_records(None, lines, device_fields(hip, lines)), what + ": levels")
        return gl

    hip.step(0)
    first = check("step 0")
    for it in (1, 2, 3):
        hip.step(it)
    later = check("step 3")
    assert not np.array_equal(bits(first), bits(later))  # the records follow the state
    # an edit: sampling is out of order until the next step, and so is the record; then the probes are still there
    removed = hip.remove_region((6.0 * r0, 8.0 * r0, 6.0 * r0, 9.0 * r0, 12.0 * r0, 9.0 * r0), types=(1,))
    assert removed > 5
    assert status_of(lambda: hip.sample_points(pts)) == status_of(lambda: hip.probes_record()) == ERR_ORDER
    hip.step(4)
    assert hip.probes_count() == (60, lines.shape[0])
    dented = check("after remove_region and a step")
    assert not np.array_equal(bits(dented), bits(later))
    # a pose change of a body made of the lid: the probes stay, and the record is the sampler's before and after the next step
    lid = hip.body_define_region(0, (-INF, 15.0 * r0, -INF, INF, INF, INF))
    assert lid > 0
    hip.body_set_pose(0, np.array([[1, 0, 0, 0], [0, 1, 0, -0.25 * r0], [0, 0, 1, 0]], f32))
    assert status_of(lambda: hip.sample_points(pts)) == status_of(lambda: hip.probes_record())
    hip.step(5)
    assert hip.probes_count() == (60, lines.shape[0])
    check("after body_set_pose and a step")
    hip.close()


# ---------------------------------------------------------------------------------------------- the calling rules
def test_statuses_follow_sample_points(box):
    sc = box["sc"]
    pts = points_of(sc, box["state"])[:20]
    hip = scenes.hip_for(sc)
    assert status_of(lambda: hip.probes_record()) == ERR_ORDER and status_of(lambda: hip.probes_record(read=False)) == ERR_ORDER  # nothing set
    hip.step(0)
    assert status_of(lambda: hip.probes_record()) == ERR_ORDER  # ... whatever the state
    hip.close()
    hip = scenes.hip_for(sc)
    hip.probes_set_lines(pc.line((0, 0, 0), (0, 0, 1), 5))

    def both(what):
        want = status_of(lambda: hip.sample_points(pts))
        assert status_of(lambda: hip.probes_record()) == want and status_of(lambda: hip.probes_record(read=False)) == want, what
        return want

    assert both("before the first step") == ERR_ORDER
    calls = np.zeros(1, np.int64)
    hip.probes_history(2)
    assert hip._L.sph_probes_read_history(hip._h, 0, 0, None, None, calls.ctypes.data) == 0 and calls[0] == 0  # failed calls took no index
    hip.step(0)
    assert both("after a step") == 0
    hip._runClearBuffers()
    hip._runHashParticles()
    both("inside a stage-by-stage step")
    hip.close()
    hip = scenes.hip_for(sc)
    hip.probes_set_points(pts)
    scenes.staged_step(hip, 0)
    assert both("after a stage-by-stage step") == 0
    r0 = float(sc["cfg"].r0)
    assert hip.remove_region((6.0 * r0, 8.0 * r0, 6.0 * r0, 9.0 * r0, 12.0 * r0, 9.0 * r0), types=(1,)) > 0
    assert both("after an edit") == ERR_ORDER
    hip.step(1)
    assert both("after the edit's step") == 0
    hip.close()


def test_validation_is_all_or_nothing(box):
    sc, state = box["sc"], box["state"]
    hip = scenes.hip_for(sc)
    for it in range(pc.STEPS):
        hip.step(it)
    good = np.concatenate([l for n, l in box["cases"] if n in ("counts", "dry")])
    pts = points_of(sc, state)[:30]
    hip.probes_set_lines(good)
    hip.probes_set_points(pts, (1,))
    before = hip.probes_record()

    def bad_line(**change):
        ln = good.copy()
        for k, v in change.items():
            ln[k][3] = v
        return ln

    bad_sets = [bad_line(origin=(0.0, NAN, 0.0)), bad_line(origin=(INF, 0.0, 0.0)), bad_line(step=(0.0, 0.0, -INF)), bad_line(step=(NAN, 1.0, 1.0)),
                bad_line(iso=NAN), bad_line(iso=INF), bad_line(count=1), bad_line(count=0), bad_line(count=-5),
                bad_line(count=sphmi.PROBE_LINE_MAX + 1), bad_line(field=-1), bad_line(field=6), bad_line(typeMask=0), bad_line(typeMask=1),
                bad_line(typeMask=16), bad_line(typeMask=2 | 32), np.tile(good[:1], sphmi.PROBE_MAX_LINES + 1)]
    for k, ln in enumerate(bad_sets):
        assert status_of(lambda: hip.probes_set_lines(ln)) == ERR_INVALID, k
    L, h = hip._L, hip._h
    assert L.sph_probes_set_lines(h, None, 3) == ERR_INVALID and L.sph_probes_set_lines(h, good.ctypes.data, -1) == ERR_INVALID
    assert L.sph_probes_set_points(h, None, 3, 2) == ERR_INVALID and L.sph_probes_set_points(h, pts.ctypes.data, -1, 2) == ERR_INVALID
    for types in ((), (0,), (4,), (1, 5)):
        assert status_of(lambda: hip.probes_set_points(pts, types)) == ERR_INVALID, types
    assert status_of(lambda: hip.probes_set_points(np.zeros((sphmi.PROBE_MAX_POINTS + 1, 3), f32))) == ERR_INVALID
    assert L.sph_probes_count(h, None) == ERR_INVALID
    # the refused sets left the old ones recording
    assert hip.probes_count() == (30, good.shape[0])
    after = hip.probes_record()
    assert_bits(after[0], before[0], "points after the refusals")
    assert_bits(after[1], before[1], "levels after the refusals")
    # the largest sets are accepted: non-finite points too, lines of 1024 points
    hip.probes_set_points(np.full((sphmi.PROBE_MAX_POINTS, 3), NAN, f32))
    hip.probes_set_lines(None)
    assert hip.probes_count() == (sphmi.PROBE_MAX_POINTS, 0) and not hip.probes_record()[0].any()
    hip.probes_set_points(None)
    assert hip.probes_count() == (0, 0) and status_of(lambda: hip.probes_record()) == ERR_ORDER
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    L, h = hip._L, hip._h
    out, cnt, ln = np.zeros((4, 8), f32), np.zeros(2, np.int64), pc.line((0, 0, 0), (0, 0, 1), 2)
    rcs = [L.sph_probes_set_points(h, out.ctypes.data, 2, 2), L.sph_probes_set_points(h, None, 0, 2), L.sph_probes_set_lines(h, ln.ctypes.data, 1),
           L.sph_probes_count(h, cnt.ctypes.data), L.sph_probes_record(h, None, None), L.sph_probes_history(h, 4),
           L.sph_probes_read_history(h, 0, 1, out.ctypes.data, None, None)]
    assert rcs == [ERR_INVALID] * len(rcs), rcs
    assert b"slab" in L.sph_last_error()
    hip.close()


# ---------------------------------------------------------------------------------------------- the driver
def test_cpp_driver_probe_history(tmp_path):
    """sphmi_run --probe ... --level-line ... --level-grid ... --probe-every K --probe-out FILE writes the history a Python replay of
    its schedule reads from the ring."""
    import os
    import subprocess
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.SCENES["tiny"]()
    r0 = f32(sc["cfg"].r0)
    p = [f32(7.0) * r0, f32(6.0) * r0, f32(7.5) * r0]
    lo, st, n = [f32(7.25) * r0, f32(4.0) * r0, f32(6.5) * r0], [f32(0), f32(0.125) * r0, f32(0)], 80
    go, gs, gd = [f32(4.0) * r0, f32(5.0) * r0, f32(3.0) * r0], [f32(2.0) * r0, f32(1.5) * r0, f32(0.25) * r0], (3, 2, 70)
    num = lambda v: ["%.9g" % x for x in v]
    out = str(tmp_path / "probes.bin")
    args = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "7", "--quiet", "--probe"] + num(p) + ["--probe", "1", "2", "nan"] + \
           ["--level-line"] + num(lo) + num(st) + [str(n), "--level-grid"] + num(go) + num(gs) + [str(d) for d in gd] + \
           ["--probe-every", "2", "--probe-out", out]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "_probes: calls 3 points 2 lines 7" in r.stdout
    gp, gl, every = frames.read_probes(out)
    assert every == 2 and gp.shape == (3, 2, 8) and gl.shape == (3, 7, 8)
    hip = scenes.hip_for(sc)
    hip.probes_set_points([p, [1, 2, NAN]], (1, 2))
    hip.probes_set_lines(np.concatenate([pc.line(lo, st, n), frames.level_columns(go, gs, gd)]))
    hip.probes_history(3)
    for it in range(7):
        hip.step(it)
        if (it + 1) % 2 == 0:
            hip.probes_record(read=False)
    wp, wl = hip.probe_history(0, 3)
    hip.close()
    assert_bits(gp, wp, "the driver's points")
    assert_bits(gl, wl, "the driver's levels")
    assert (wl[:, :, 4] == pr.FOUND).any() and wp[:, 0, 6].min() > 5 and not wp[:, 1].any()
    for bad in (["--probe", "1", "2", "3"], ["--probe", "1", "2", "3", "--probe-every", "2"], ["--probe-every", "2", "--probe-out", out],
                ["--probe", "1", "2", "3", "--probe-every", "0", "--probe-out", out],
                ["--level-grid", "0", "0", "0", "1", "1", "1", "0", "2", "5", "--probe-every", "1", "--probe-out", out]):
        r = subprocess.run([exe, "--steps", "1"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip(), bad
