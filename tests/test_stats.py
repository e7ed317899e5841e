"""GPU tests of the time statistics on a lattice (sph_stats_define / sph_stats_get / sph_stats_accumulate / sph_stats_reset /
sph_stats_read / sph_stats_read_moments, include/sphmi.h): every accumulator word and every moment word equal, as bit patterns, to
the numpy restatement (tests/stats_ref.py) over the solver's state and to a host fold of the solver's own sph_sample_grid records, on
the cases tests/test_stats_host.py proves to hold what they claim (tests/stats_cases.py); lattice shapes on both routes; slots,
windows, reset, redefine and release; the edge states of the brick walk; the calling rules; the life of the numbers across steps,
edits and poses; the driver."""
import re

import numpy as np
import pytest

import sample_cases
import sample_ref
import scenes
import sphmi
import stats_cases as sc_
import stats_ref as sr
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
NAN, INF = np.nan, np.inf


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_acc(got, want, what):
    got, want = np.asarray(got).reshape(-1, 24), np.asarray(want).reshape(-1, 24)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = np.argwhere(b64(got) != b64(want))
    assert ne.size == 0, "%s: %d words differ; first at node %d word %d: %r vs %r" % (
        what, ne.shape[0], ne[0][0], ne[0][1], got[tuple(ne[0])], want[tuple(ne[0])])


def assert_mom(got, want, what):
    got, want = np.asarray(got).reshape(-1, 16), np.asarray(want).reshape(-1, 16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = np.argwhere(b32(got) != b32(want))
    assert ne.size == 0, "%s: %d words differ; first at node %d word %d: %r vs %r" % (
        what, ne.shape[0], ne[0][0], ne[0][1], got[tuple(ne[0])], want[tuple(ne[0])])


def status_of(call):
    """The library's status of a wrapper call: 0, or the code in the SphError."""
    try:
        call()
    except sphmi.SphError as e:
        return int(re.search(r"\(status (-?\d+)\)", str(e)).group(1))
    return 0


def types_of(mask):
    return tuple(t for t in (1, 2, 3) if mask >> t & 1)


def define(hip, slot, g):
    hip.stats_define(slot, g["origin"], g["spacing"], g["dims"], types_of(g["typeMask"]))


def grid_records(hip, g):
    """The solver's own sph_sample_grid records on the lattice, float32[nodes, 8]."""
    return hip.sample_grid(g["origin"], g["spacing"], g["dims"], types_of(g["typeMask"])).reshape(-1, 8)


def stepped(sc, steps):
    hip = scenes.hip_for(sc)
    for it in range(steps):
        hip.step(it)
    return hip


@pytest.fixture(scope="module")
def box():
    """A solver of the scene after two steps for the tests that need no history of their own; they leave slots 0..3 released."""
    sc = sc_.scene()
    hip = stepped(sc, 2)
    yield dict(sc=sc, hip=hip, lat=sc_.lattices(sc["cfg"]))
    hip.close()


# ---------------------------------------------------------------------------------------------- every word, bit for bit
def test_restatement():
    """A and B in two slots through the sequence; all 24 words and the 16 moment words after every call against the restatement over
    the solver's state and against a host fold of the solver's own sample_grid records."""
    sc = sc_.scene()
    cfg = sc["cfg"]
    lat = sc_.lattices(cfg)
    hip = scenes.hip_for(sc)
    for slot, name in enumerate("AB"):
        define(hip, slot, lat[name])
    ref = {k: sr.empty(np.prod(lat[k]["dims"])) for k in lat}
    own = {k: sr.empty(np.prod(lat[k]["dims"])) for k in lat}
    records = {k: [] for k in lat}
    it = 0
    for call, steps in enumerate(sc_.STEPS_BEFORE_CALL):
        if call == sc_.EDIT_BEFORE_CALL:
            assert hip.remove_region(sc_.edit_region(cfg), types=(1,)) > 100
            hip.add_particles(*sc_.added_block(cfg))
        for _ in range(steps):
            hip.step(it)
            it += 1
        hip.stats_accumulate()
        state = sample_ref.solver_state(hip)
        for slot, name in enumerate("AB"):
            g = lat[name]
            nx, ny, nz = g["dims"]
            rec = sr.lattice_records(state, g)
            records[name].append(rec)
            ref[name] = sr.fold(ref[name], rec, call)
            own[name] = sr.fold(own[name], grid_records(hip, g), call)
            got, calls = hip.stats(slot)
            assert got.shape == (nz, ny, nx, 24) and got.dtype == np.float64 and calls == call + 1
            assert_acc(got, ref[name], "%s after call %d against the restatement" % (name, call))
            assert_acc(got, own[name], "%s after call %d against the fold of sample_grid" % (name, call))
            mom, calls = hip.stats_moments(slot)
            assert mom.shape == (nz, ny, nx, 16) and mom.dtype == np.float32 and calls == call + 1
            assert_mom(mom, sr.moments(ref[name], call + 1), "%s moments after call %d" % (name, call))
            assert_mom(mom, frames.stats_moments(got, calls).astype(f32), "%s moments against frames.stats_moments" % name)
    hip.close()
    for name in "AB":
        print(name, sc_.check_claims(records[name]))  # (on these states too: the host test made them on the oracle's)


SHAPES = [(1, 1, 1), (4, 4, 4), (5, 3, 2), (64, 1, 1), (1, 1, 65)]


@pytest.mark.parametrize("route", ["bricks", "points"])
def test_shapes(box, route):
    hip, r0 = box["hip"], f32(box["sc"]["cfg"].r0)
    sp = f32(0.6) * r0 if route == "bricks" else f32(1.4) * r0
    wet_somewhere = 0
    for dims in SHAPES:
        # the lattice starts inside the liquid; the long ones run through it along x and z
        g = dict(origin=np.array([f32(3.1) * r0, f32(5.2) * r0, f32(3.3) * r0], f32) - (np.array(dims) > 8) * f32(2.0) * r0,
                 spacing=np.array([sp, sp, sp if dims[2] < 8 else f32(0.2) * r0 if route == "bricks" else sp], f32), dims=dims,
                 typeMask=2)
        define(hip, 2, g)
        got0, calls = hip.stats(2)
        assert calls == 0
        assert_acc(got0, sr.empty(np.prod(dims)), "%s empty" % (dims,))
        want = sr.empty(np.prod(dims))
        for c in range(2):
            hip.stats_accumulate(2)
            want = sr.fold(want, grid_records(hip, g), c)
        got, calls = hip.stats(2)
        assert calls == 2 and got.shape == (dims[2], dims[1], dims[0], 24)
        assert_acc(got, want, "%s %s" % (route, dims))
        assert_mom(hip.stats_moments(2)[0], sr.moments(want, 2), "%s %s moments" % (route, dims))
        wet_somewhere += int((got[..., 0] == 2).any())
        assert set(np.unique(got[..., 0])) <= {0.0, 2.0}
    assert wet_somewhere == len(SHAPES)
    hip.stats_release(2)


def test_no_host_wait():
    """Five accumulates over five steps with no read in between, then one read."""
    sc = sc_.scene()
    lat = sc_.lattices(sc["cfg"])
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    define(a, 0, lat["A"])
    want = sr.empty(np.prod(lat["A"]["dims"]))
    for it in range(5):
        a.step(it)
        b.step(it)
        a.stats_accumulate(0)
        want = sr.fold(want, grid_records(b, lat["A"]), it)
    got, calls = a.stats(0)
    assert calls == 5
    assert_acc(got, want, "five calls, one read")
    assert len(set(got[..., 19][got[..., 0] > 0].tolist())) >= 3  # the peak speed moved between the calls
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- slots
def test_slots(box):
    hip, lat, r0 = box["hip"], box["lat"], f32(box["sc"]["cfg"].r0)
    # three masks on one lattice that crosses the liquid, the air and the lid, and B: slot -1 against the slots one by one
    col = dict(origin=np.array([f32(6.9) * r0, f32(7.0) * r0, f32(7.1) * r0], f32), spacing=np.array([f32(0.5) * r0] * 3, f32), dims=(3, 21, 2))
    gs = [dict(col, typeMask=m) for m in (2, 8, 14)] + [lat["B"]]
    for slot, g in enumerate(gs):
        define(hip, slot, g)
    hip.stats_accumulate(-1)
    hip.stats_accumulate(-1)
    all_at_once = [hip.stats(slot) for slot in range(4)]
    hip.stats_reset(-1)
    assert [hip.stats_get(slot)[1] for slot in range(4)] == [0] * 4
    for slot in (2, 0, 3, 1):
        hip.stats_accumulate(slot)
        hip.stats_accumulate(slot)
    for slot, g in enumerate(gs):
        got, calls = hip.stats(slot)
        assert calls == 2 and all_at_once[slot][1] == 2
        assert_acc(got, all_at_once[slot][0], "slot %d: one by one against -1" % slot)
        rec = grid_records(hip, g)
        assert_acc(got, sr.fold(sr.fold(sr.empty(rec.shape[0]), rec, 0), rec, 1), "slot %d against the fold" % slot)
    liquid, boundary, both = (all_at_once[s][0][..., 0] for s in range(3))
    assert (liquid > 0).any() and (boundary > 0).any() and ((liquid > 0) != (boundary > 0)).any()
    assert np.array_equal(both > 0, (liquid > 0) | (boundary > 0)) and (both == 0).any()
    # stats_get
    g, calls = hip.stats_get(1)
    assert calls == 2 and g["dims"] == (3, 21, 2) and g["typeMask"] == 8 and np.array_equal(b32(g["spacing"]), b32(col["spacing"]))
    # reset of one slot leaves the others
    hip.stats_reset(1)
    assert_acc(hip.stats(1)[0], sr.empty(126), "reset slot")
    assert hip.stats_get(1)[1] == 0 and hip.stats_get(1)[0]["typeMask"] == 8
    for slot in (0, 2, 3):
        assert_acc(hip.stats(slot)[0], all_at_once[slot][0], "slot %d after the reset of slot 1" % slot)
        assert hip.stats_get(slot)[1] == 2
    assert status_of(lambda: hip.stats_moments(1)) == ERR_ORDER  # no call yet
    hip.stats_accumulate(1)
    assert hip.stats(1)[1] == 1 and tuple(np.unique(hip.stats(1)[0][..., 1])) == (-1.0, 0.0)  # the index starts again
    # windows against slices of the full read
    full, _ = hip.stats(3)
    mom, _ = hip.stats_moments(3)
    nodes = full.shape[0] * full.shape[1] * full.shape[2]
    for first, count in ((0, nodes), (0, 1), (nodes - 1, 1), (5, 37), (100, 0), (nodes, 0)):
        got, calls = hip.stats(3, first, count)
        assert got.shape == (count, 24) and calls == 2
        assert_acc(got, full.reshape(-1, 24)[first:first + count], "window %d + %d" % (first, count)) if count else None
        gm, _ = hip.stats_moments(3, first, count)
        assert gm.shape == (count, 16)
        assert_mom(gm, mom.reshape(-1, 16)[first:first + count], "moment window %d + %d" % (first, count)) if count else None
    for first, count in ((-1, 1), (0, nodes + 1), (nodes, 1), (nodes + 1, 0), (5, -1)):
        assert status_of(lambda: hip.stats(3, first, count)) == ERR_INVALID, (first, count)
        assert status_of(lambda: hip.stats_moments(3, first, count)) == ERR_INVALID, (first, count)
    big = np.zeros(24, np.float64)
    for first, count in ((1 << 62, 1 << 62), (1, (1 << 63) - 1), (-(1 << 63), 1)):  # (no sum of the two may wrap)
        assert hip._L.sph_stats_read(hip._h, 3, first, count, big.ctypes.data, None) == ERR_INVALID
        assert hip._L.sph_stats_read_moments(hip._h, 3, first, count, big.ctypes.data, None) == ERR_INVALID
    assert hip._L.sph_stats_read(hip._h, 3, 0, 1, None, None) == ERR_INVALID
    # redefine: empty again, with the new lattice; release: the slot is gone and its calls are 0
    define(hip, 3, lat["A"])
    got, calls = hip.stats(3)
    assert calls == 0 and got.shape == (9, 19, 17, 24)
    assert_acc(got, sr.empty(17 * 19 * 9), "redefined slot")
    hip.stats_accumulate(3)
    assert_acc(hip.stats(3)[0], sr.fold(sr.empty(17 * 19 * 9), grid_records(hip, lat["A"]), 0), "redefined slot, one call")
    hip.stats_release(3)
    assert hip.stats_get(3) == (None, 0)
    assert status_of(lambda: hip.stats_accumulate(3)) == ERR_ORDER and status_of(lambda: hip.stats_reset(3)) == ERR_ORDER
    assert hip._L.sph_stats_read(hip._h, 3, 0, 0, None, None) == ERR_ORDER
    hip.stats_accumulate(-1)  # the other three go on
    assert [hip.stats_get(slot)[1] for slot in range(4)] == [3, 2, 3, 0]
    for slot in range(3):
        hip.stats_release(slot)
    assert status_of(lambda: hip.stats_accumulate(-1)) == ERR_ORDER
    hip.stats_reset(-1)  # nothing defined: nothing to do


# ---------------------------------------------------------------------------------------------- the edge states of the walks
def test_per_lane_fallback_and_overflowing_lattice(box):
    hip, cfg = box["hip"], box["sc"]["cfg"]
    h, r0 = f32(cfg.h), f32(cfg.r0)
    # so far out that float coordinates no longer resolve h: bricks whose cell box exceeds 64 cells go lane by lane; all dry
    far = dict(origin=np.array([2e7] * 3, f32), spacing=np.array([f32(0.66) * h] * 3, f32), dims=(12, 12, 12), typeMask=14)
    assert (sample_ref.brick_box_cells(far["origin"], far["spacing"], far["dims"], cfg.h, cfg.hashGridCellSizeInv) > 64).any()
    # far points overflow: x = ox + (float)i * 3e37 is finite and far away for i < 12 and +inf from there on; the columns i = 0 lie in the
    # liquid. (A spacing that can overflow is above 2h/3: this is the point route. With finite origin and spacing <= 2h/3 no point of a
    # lattice can overflow.)
    over = dict(origin=np.array([f32(5.0) * r0, f32(5.0) * r0, f32(5.0) * r0], f32), spacing=np.array([f32(3e37), f32(0.5) * r0, f32(0.0)], f32),
                dims=(14, 5, 3), typeMask=2)
    with np.errstate(over="ignore"):
        finite = np.isfinite(sample_ref.grid_points(over["origin"], over["spacing"], over["dims"])).all(-1)
    assert finite[:, :, :12].all() and not finite[:, :, 12:].any()
    for name, g in (("far", far), ("overflow", over)):
        define(hip, 0, g)
        hip.stats_accumulate(0)
        hip.stats_accumulate(0)
        rec = grid_records(hip, g)
        got, _ = hip.stats(0)
        assert_acc(got, sr.fold(sr.fold(sr.empty(rec.shape[0]), rec, 0), rec, 1), name)
        wet = got[..., 0] > 0
        if name == "far":
            assert not wet.any()
            assert_acc(got, sr.empty(rec.shape[0]), "far: untouched")
        else:
            assert wet[:, :, 0].all() and not wet[:, :, 1:].any()
            assert_acc(got[:, :, 1:], sr.empty(3 * 5 * 13), "overflow: the dry nodes are untouched")
    hip.stats_release(0)


@pytest.mark.parametrize("types", [(1,), (1, 2, 3)])
def test_ring_scene_bricks(types):
    """The lattice calls of tests/sample_cases.py: queries at the support boundary to the ulp, across cell faces and at negative
    coordinates, as point (0, 0, 0) of small brick lattices. (Reference-mode scene: masked keys.)"""
    sc = sample_cases.ring_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)
    state = sample_ref.solver_state(hip)
    calls = sample_cases.brick_calls(sc, (5, 4, 3))[::61]  # (61 and the 3 calls of a query are coprime: every spacing pattern occurs)
    assert 20 <= len(calls) <= 60
    wet = 0
    for _, origin, spacing, dims in calls:
        g = dict(origin=np.asarray(origin, f32), spacing=np.asarray(spacing, f32), dims=dims, typeMask=sphmi.type_mask(types))
        define(hip, 1, g)
        hip.stats_accumulate(1)
        got, _ = hip.stats(1)
        rec = sr.lattice_records(state, g)
        assert_acc(got, sr.fold(sr.empty(rec.shape[0]), rec, 0), "brick call at %s" % (origin,))
        wet += int((got[..., 0] > 0).sum())
    assert wet > 0
    hip.close()


def test_aliased_cells():
    """Reference-mode cell ids beyond 16 bits: runs of masked keys mix far-apart cells (scene alias16)."""
    sc = scenes.SCENES["alias16"]()
    cfg = sc["cfg"]
    assert cfg.cellIdMask == 0xffff and cfg.gridCellCount > 65536
    hip = scenes.hip_for(sc)
    hip.step(0)
    state = sample_ref.solver_state(hip)
    liq = state["pos"][(state["types"].astype(int) == 1) & (state["pos"][:, 2] > 672)]
    assert liq.shape[0] > 0
    h = f32(cfg.h)
    o = (liq[liq.shape[0] // 2] - f32(1.0) * h).astype(f32)
    for name, sp, dims in (("bricks", f32(0.5) * h, (9, 6, 7)), ("points", f32(1.1) * h, (5, 4, 4))):
        g = dict(origin=o, spacing=np.array([sp, sp, sp], f32), dims=dims, typeMask=14)
        define(hip, 0, g)
        hip.stats_accumulate(0)
        got, _ = hip.stats(0)
        rec = sr.lattice_records(state, g)
        assert_acc(got, sr.fold(sr.empty(rec.shape[0]), rec, 0), "alias16 " + name)
        assert (got[..., 0] > 0).any()
    hip.close()


# ---------------------------------------------------------------------------------------------- the calling rules
def test_statuses_follow_sample_points():
    sc = sc_.scene()
    lat = sc_.lattices(sc["cfg"])
    r0 = float(sc["cfg"].r0)
    pts = np.zeros((3, 3), f32)
    hip = scenes.hip_for(sc)
    assert status_of(lambda: hip.stats_accumulate()) == ERR_ORDER and status_of(lambda: hip.stats_accumulate(2)) == ERR_ORDER  # nothing defined
    hip.step(0)
    assert status_of(lambda: hip.stats_accumulate()) == ERR_ORDER  # ... whatever the state
    for slot in (-2, 4, 99):
        assert status_of(lambda: hip.stats_accumulate(slot)) == ERR_INVALID and status_of(lambda: hip.stats_reset(slot)) == ERR_INVALID
    hip.close()
    hip = scenes.hip_for(sc)
    define(hip, 0, lat["B"])
    define(hip, 2, lat["A"])

    def both(what):
        want = status_of(lambda: hip.sample_points(pts))
        assert status_of(lambda: hip.stats_accumulate()) == want and status_of(lambda: hip.stats_accumulate(2)) == want, what
        return want

    assert both("before the first step") == ERR_ORDER
    assert hip.stats_get(0)[1] == 0 and hip.stats_get(2)[1] == 0  # failed calls took no index
    hip.step(0)
    assert both("after a step") == 0
    assert hip.stats_get(0)[1] == 1 and hip.stats_get(2)[1] == 2
    before = hip.stats(0)[0], hip.stats(2)[0]
    hip._runClearBuffers()
    hip._runHashParticles()
    inside = both("inside a stage-by-stage step")
    hip.close()
    hip = scenes.hip_for(sc)
    define(hip, 0, lat["B"])
    define(hip, 2, lat["A"])
    scenes.staged_step(hip, 0)
    assert both("after a stage-by-stage step") == 0
    assert inside in (0, ERR_ORDER)
    assert_acc(hip.stats(0)[0], before[0], "one call after a staged step against one call after a fused step")
    assert hip.remove_region((6.0 * r0, 8.0 * r0, 6.0 * r0, 9.0 * r0, 12.0 * r0, 9.0 * r0), types=(1,)) > 0
    kept = hip.stats(2)
    assert both("after an edit") == ERR_ORDER
    assert_acc(hip.stats(2)[0], kept[0], "a failed call changes nothing")
    assert hip.stats(2)[1] == kept[1] == 2
    hip.step(1)
    assert both("after the edit's step") == 0
    hip.close()


def test_validation(box):
    hip, lat = box["hip"], box["lat"]
    good = lat["B"]
    define(hip, 1, good)
    hip.stats_accumulate(1)
    before = hip.stats(1)

    def bad(**change):
        g = dict(good)
        g.update(change)
        return status_of(lambda: hip.stats_define(1, g["origin"], g["spacing"], g["dims"], g.get("types", (1,))))

    o, s = good["origin"], good["spacing"]
    for k in range(3):
        for v in (NAN, INF, -INF):
            oo, ss = o.copy(), s.copy()
            oo[k], ss[k] = v, v
            assert bad(origin=oo) == ERR_INVALID and bad(spacing=ss) == ERR_INVALID
        for v in (0, -1, -2 ** 31 + 1):
            d = list(good["dims"])
            d[k] = v
            assert bad(dims=d) == ERR_INVALID
    for types in ((), (0,), (4,), (1, 5), (0, 1)):
        assert bad(types=types) == ERR_INVALID, types
    for slot in (-1, 4, 1 << 20):
        assert status_of(lambda: hip.stats_define(slot, o, s, good["dims"])) == ERR_INVALID
        assert status_of(lambda: hip.stats_release(slot)) == ERR_INVALID
        assert status_of(lambda: hip.stats_get(slot)) == ERR_INVALID
        assert status_of(lambda: hip.stats(slot)) == ERR_INVALID and status_of(lambda: hip.stats_moments(slot)) == ERR_INVALID
    assert hip._L.sph_stats_read(hip._h, -1, 0, 0, None, None) == ERR_INVALID
    assert hip._L.sph_stats_read_moments(hip._h, 4, 0, 0, None, None) == ERR_INVALID
    # the byte cap: 2^31 bytes = 11184810 nodes and two thirds
    cap = sphmi.STATS_BYTES_MAX // (8 * sphmi.STATS_WORDS)
    for dims in ((cap + 1, 1, 1), (1, 1, cap + 1), (3344, 3345, 1), (224, 224, 224), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (65536, 65536, 1),
                 (2 ** 16, 2 ** 16, 2 ** 16), (2 ** 21, 2 ** 21, 2 ** 22)):
        assert bad(dims=dims) == ERR_INVALID, dims
    assert b"exceed" in hip._L.sph_last_error()
    # zero spacing and negative spacing are lattices like any other
    assert bad(spacing=np.array([0.0, -s[1], s[2]], f32)) == 0
    define(hip, 1, good)
    hip.stats_accumulate(1)
    # ... and every refusal above left the old slot as it was, still accumulating
    g, calls = hip.stats_get(1)
    assert calls == 1 and g["dims"] == good["dims"] and np.array_equal(b32(g["origin"]), b32(good["origin"]))
    assert_acc(hip.stats(1)[0], before[0], "the slot after the refusals")
    assert bad(dims=(cap + 1, 1, 1)) == ERR_INVALID and bad(origin=np.array([NAN, 0, 0], f32)) == ERR_INVALID
    hip.stats_accumulate(1)
    rec = grid_records(hip, good)
    assert hip.stats(1)[1] == 2
    assert_acc(hip.stats(1)[0], sr.fold(sr.fold(sr.empty(rec.shape[0]), rec, 0), rec, 1), "the old slot goes on")
    hip.stats_release(1)


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    L, h = hip._L, hip._h
    g = sphmi.stats_lattice((0, 0, 0), (1, 1, 1), (2, 2, 2))
    out, calls, has = np.zeros((8, 24), np.float64), np.zeros(1, np.int64), np.zeros(1, np.int32)
    assert status_of(lambda: hip.sample_points(np.zeros((1, 3), f32))) == ERR_INVALID
    rcs = [L.sph_stats_define(h, 0, g.ctypes.data), L.sph_stats_define(h, 0, None), L.sph_stats_get(h, 0, None, has.ctypes.data, None),
           L.sph_stats_accumulate(h, -1), L.sph_stats_accumulate(h, 0), L.sph_stats_reset(h, -1), L.sph_stats_read(h, 0, 0, 1, out.ctypes.data, None),
           L.sph_stats_read_moments(h, 0, 0, 1, out.ctypes.data, calls.ctypes.data)]
    assert rcs == [ERR_INVALID] * len(rcs), rcs
    assert b"slab" in L.sph_last_error()
    hip.close()


# ---------------------------------------------------------------------------------------------- lifetime
def test_untouched_by_the_rest():
    """Steps, remove_region, body_set_pose, selections and diagnostics between two accumulates leave the numbers alone."""
    sc = sc_.scene()
    cfg = sc["cfg"]
    r0 = float(cfg.r0)
    lat = sc_.lattices(cfg)
    hip = stepped(sc, 2)
    define(hip, 0, lat["A"])
    define(hip, 3, lat["B"])
    hip.stats_accumulate()
    rec0 = {s: grid_records(hip, lat[k]) for s, k in ((0, "A"), (3, "B"))}
    first = {s: hip.stats(s)[0] for s in (0, 3)}

    def same(what):
        for s in (0, 3):
            got, calls = hip.stats(s)
            assert calls == 1
            assert_acc(got, first[s], "slot %d after %s" % (s, what))

    hip.step(2)
    hip.step(3)
    same("two steps")
    hip.diagnostics()
    assert hip.select(types=(1,)) > 0
    hip.sample_grid(lat["A"]["origin"], lat["A"]["spacing"], lat["A"]["dims"])
    same("diagnostics, a selection and sample_grid")
    assert hip.remove_region((6.0 * r0, 8.0 * r0, 6.0 * r0, 9.0 * r0, 12.0 * r0, 9.0 * r0), types=(1,)) > 5
    same("remove_region")
    assert hip.body_define_region(0, (-INF, 15.0 * r0, -INF, INF, INF, INF)) > 0
    hip.body_set_pose(0, np.array([[1, 0, 0, 0], [0, 1, 0, -0.25 * r0], [0, 0, 1, 0]], f32))
    same("body_set_pose")
    hip.step(4)
    same("the step after the edits")
    # the next call folds the new state at call index 1, at the lattice's old place
    hip.stats_accumulate()
    for s, k in ((0, "A"), (3, "B")):
        got, calls = hip.stats(s)
        assert calls == 2
        rec1 = grid_records(hip, lat[k])
        assert_acc(got, sr.fold(sr.fold(sr.empty(rec1.shape[0]), rec0[s], 0), rec1, 1), "slot %d: the second call" % s)
        assert not np.array_equal(b32(rec0[s]), b32(rec1))
    hip.close()


# ---------------------------------------------------------------------------------------------- the driver
def test_cpp_driver_stats_file(tmp_path):
    """sphmi_run --stats-grid ... --stats-types --stats-from S --stats-every K --stats-out FILE writes the accumulators a Python replay
    of its schedule reads."""
    import os
    import subprocess
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.SCENES["tiny"]()
    r0 = f32(sc["cfg"].r0)
    o, s, d = [f32(3.5) * r0, f32(4.0) * r0, f32(3.0) * r0], [f32(0.75) * r0, f32(1.0) * r0, f32(1.0) * r0], (9, 14, 6)
    num = lambda v: ["%.9g" % x for x in v]
    out = str(tmp_path / "stats.bin")
    args = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "7", "--quiet", "--stats-grid"] + num(o) + num(s) + \
           [str(v) for v in d] + ["--stats-types", "1 2", "--stats-from", "1", "--stats-every", "2", "--stats-out", out]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "_stats: calls 3 nodes %d" % (9 * 14 * 6) in r.stdout
    lat, got, calls, first, every = frames.read_stats(out)
    assert (calls, first, every) == (3, 1, 2) and lat["dims"] == d and lat["typeMask"] == 6 and got.shape == (6, 14, 9, 24)
    hip = scenes.hip_for(sc)
    hip.stats_define(0, o, s, d, types=(1, 2))
    for it in range(7):
        hip.step(it)
        if it >= 1 and (it - 1) % 2 == 0:
            hip.stats_accumulate(0)
    want, wcalls = hip.stats(0)
    hip.close()
    assert wcalls == 3
    assert_acc(got, want, "the driver's accumulators")
    assert (got[..., 0] == 3).any() and (got[..., 0] == 0).any()
    for bad in (["--stats-grid"] + num(o) + num(s) + ["4", "4", "4"], ["--stats-out", out], ["--stats-every", "2", "--stats-out", out],
                ["--stats-grid"] + num(o) + num(s) + ["4", "4", "4", "--stats-every", "0", "--stats-out", out],
                ["--stats-grid"] + num(o) + num(s) + ["4", "4", "4", "--stats-from", "-1", "--stats-out", out]):
        r = subprocess.run([exe, "--steps", "1"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip(), bad
