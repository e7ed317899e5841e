"""GPU tests of the wall loads (sph_wall_measure / sph_wall_diagnostics, include/sphmi.h): every word of both calls bit-identical
to the numpy restatement (tests/wall_ref.py, which tests/test_wall_host.py ties to the oracle's integrate stage) for a body, a
second body, all walls and the walls of no body, on scenes whose floor was lifted into the liquid so that integrate's contact and
reflection branches run; the records' position and velocity against the read-back in every step mode; the selection variant; rows
that have no 16-bit copy; the calling rules; and the driver's line. No tolerance appears anywhere: integers are compared for
equality, floats as bit patterns."""
import os
import subprocess
import types as _types

import numpy as np
import pytest

import body_ref as br
import diag_ref
import forces_ref as fr
import scenes
import sphmi
import wall_cases
import wall_ref as wr
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
A, B = wall_cases.SLOT_A, wall_cases.SLOT_B
BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def first_diff(got, want, view):
    d = np.argwhere(view(got) != view(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def regions_of(cfg, count):
    """`count` regions: everything, halves and octants of the box, an empty one (x0 >= x1), one outside the scene, slabs in y
    (the lowest holds the contacts), an infinite half space."""
    mid = [f32(0.5) * f32(getattr(cfg, a + "max")) for a in "xyz"]
    inf = np.inf
    out = [diag_ref.EVERYTHING, (-inf, -inf, -inf, mid[0], inf, inf), (mid[0], -inf, -inf, inf, inf, inf),
           (0, 0, 0, mid[0], mid[1], mid[2]), (mid[0], mid[1], mid[2], mid[0], inf, inf), (-9, -9, -9, -1, -1, -1),
           (-inf, mid[1], -inf, inf, inf, inf), (-inf, -inf, mid[2], inf, inf, inf)]
    k = 0
    while len(out) < count:
        lo = f32(cfg.ymax) * f32(k) / f32(8)
        out.append((-inf, lo, -inf, inf, lo + f32(cfg.ymax) / f32(8), inf))
        k += 1
    return np.array(out[:count], np.float32)


def lifted_solver(name, setup=None, staged=False, release_b=False, stop_at_integrate=False):
    """(solver, bodies {slot: ids}, case): `name` of wall_cases.LIFTED stepped to the lift, the floor's halves defined as bodies A
    and B and lifted, B then released if asked, and one more step; tiny_elastic: 20 steps, the halves of the whole shell defined where
    they stand, one more step (stop_at_integrate: staged, and stopped behind its integrate stage)."""
    if name == "tiny_elastic":
        sc = scenes.SCENES[name]()
        case = dict(sc=sc, cfg=sc["cfg"], N=sc["cfg"].particleCount, steps=20, pose=frames.pose_identity())
    else:
        case = wall_cases.lifted(name)
        sc = case["sc"]
    hip = scenes.hip_for(sc)
    if setup:
        setup(hip)
    for it in range(case["steps"]):
        scenes.staged_step(hip, it) if staged else hip.step(it)
    if name == "tiny_elastic":
        pos, cfg = hip.read_position_buffer(), case["cfg"]
        mid, inf = f32(0.5) * f32(cfg.xmax), np.inf  # (the liquid stands clear of the floor: the bodies are the halves of the whole shell)
        ids = {A: br.region_members(pos, (-inf, -inf, -inf, mid, inf, inf)), B: br.region_members(pos, (mid, -inf, -inf, inf, inf, inf))}
    else:
        ids = {A: case["A"], B: case["B"]}
        assert scenes.bits_equal(hip.read_position_buffer(), case["pos"])  # the state the lift was worked out for
    for slot in (A, B):
        assert hip.body_define_ids(slot, ids[slot]) == ids[slot].size
        hip.body_set_pose(slot, case["pose"])
    if release_b:
        hip.body_release(B)
        del ids[B]
    if stop_at_integrate:
        for st in scenes.STAGE_SEQUENCE[:scenes.STAGE_SEQUENCE.index("integrate")]:
            getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        hip._run_pcisph_integrate(case["steps"])
    elif staged:
        scenes.staged_step(hip, case["steps"])
    else:
        hip.step(case["steps"])
    return hip, ids, case


def restatement(hip, bodies, slots):
    """The restatement on the solver's own exported state: (state, {slot: Wall})."""
    state = wr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    K, W = fr.constants(hip.cfg), wr.constants(hip.cfg)
    return state, {s: wr.Wall(state, ids, dist, K, W, wr.wall_set(state, s, bodies)) for s in slots}


LIVE = [("tiny", False), ("tiny_jitter", False), ("tiny_elastic", False), ("tiny", True), ("tiny_jitter", True)]


@pytest.fixture(scope="module", params=LIVE, ids=["%s%s" % (n, "-B-released" if r else "") for n, r in LIVE])
def live(request):
    name, released = request.param
    hip, bodies, case = lifted_solver(name, release_b=released)
    slots = [A, wr.ALL, wr.NO_BODY] + ([] if released else [B])
    state, walls = restatement(hip, bodies, slots)
    yield _types.SimpleNamespace(name=name, released=released, hip=hip, bodies=bodies, case=case, slots=slots, state=state, walls=walls)
    hip.close()


def test_records_match_restatement(live):
    hip = live.hip
    for slot in live.slots:
        rec = hip.wall_measure(slot)
        want = live.walls[slot].records
        assert rec.dtype == np.float32 and rec.shape == (hip.N, 32)
        assert np.array_equal(u32(rec), u32(want)), "%s set %d: %s" % (live.name, slot, first_diff(rec, want, u32))
    w = live.walls[wr.ALL]
    print("%s: %d in contact, %d reflected; set sizes %s" % (live.name, w.contact.sum(), w.reflected.sum(),
                                                              {s: int((live.walls[s].records[:, 9] > 0).sum()) for s in live.slots}))
    if live.name == "tiny_elastic":
        assert w.contact.sum() == 0 and np.abs(w.records[:, 10:19]).max() > 0
        assert (live.walls[A].records[:, 9] > 0).any() and (live.walls[B].records[:, 9] > 0).any()
        return
    # nothing passes vacuously: contacts, reflections, a particle that touches both bodies, and a no-body set that is touched
    assert w.contact.sum() >= 1 and w.reflected.sum() >= 1
    ra, rn = live.walls[A].records, live.walls[wr.NO_BODY].records
    assert (ra[:, 6] > 0).any() and (ra[:, 6] == 1).any() and ((ra[:, 6] > 0) & (ra[:, 6] < 1)).any()
    if live.released:
        assert (rn[:, 6] > 0).any() and np.abs(rn[:, 3:6]).max() > 0, "the released half of the floor is touched as no-body"
    else:
        rb = live.walls[B].records
        assert ((ra[:, 8] > 0) & (rb[:, 8] > 0)).sum() > 0 and not np.array_equal(u32(ra), u32(rb))


@pytest.mark.parametrize("count", [1, 16])
def test_totals_match_restatement(live, count):
    hip = live.hip
    rg = regions_of(hip.cfg, count)
    for slot in live.slots:
        for types in ((1, 2), (1, 2, 3)):
            got = hip.wall_diagnostics(slot, rg, types)
            assert got.dtype == np.float64 and got.shape == (count, 32)
            want = wr.diag_records(live.state, live.walls[slot].records, rg, types)
            assert np.array_equal(u64(got), u64(want)), "%s set %d, %d regions: %s" % (live.name, slot, count, first_diff(got, want, u64))
        assert got[0, 0] == hip.N and not got[:, 27:].any()
        if count >= 6:
            assert not got[4].any() and not got[5].any() and got[0, 1] == got[1, 1] + got[2, 1]
    if live.name != "tiny_elastic":
        assert hip.wall_diagnostics(wr.ALL, rg)[0, 1] == live.walls[wr.ALL].contact.sum() > 0


def test_all_walls_tie_to_the_force_decomposition_and_the_shares(live):
    hip = live.hip
    r = hip.wall_measure(sphmi.WALL_ALL)
    f = hip.force_measure()
    assert np.array_equal(u32(r[:, 10:19]), u32(f[:, 18:27])) and np.abs(r[:, 10:19]).max() > 0
    on = r[:, 26] != 0
    assert (r[on, 6] == 1).all() and not r[~on, 0:7].any() and np.array_equal(r[:, 7] > 0, r[:, 8] > 0)
    # a partition of the walls: slots and touching slots add up exactly, the step's own words do not depend on the set
    parts = [hip.wall_measure(s) for s in live.slots if s != wr.ALL]
    assert np.array_equal(sum(p[:, 9] for p in parts), r[:, 9]) and np.array_equal(sum(p[:, 8] for p in parts), r[:, 8])
    for p in parts:
        assert np.array_equal(u32(p[:, 19:28]), u32(r[:, 19:28]))


# ---------------------------------------------------------------------------------------------- the tie to the step, in every mode
def _chunks(n):
    return lambda hip: hip.set_step_chunks(n)


def _pipeline(depth):
    def setup(hip):
        hip.set_step_chunks(4)
        hip.set_step_pipeline(depth)
    return setup


def _skip(mode):
    return lambda hip: hip.set_wave_skip(mode)


MODES = {"fused": dict(), "staged": dict(staged=True), "chunks-2": dict(setup=_chunks(2)), "chunks-5": dict(setup=_chunks(5)),
         "chunks-16": dict(setup=_chunks(16))}
MODES.update({"pipeline-%d" % d: dict(setup=_pipeline(d)) for d in range(0, 7)})
MODES.update({"wave-skip-%d" % m: dict(setup=_skip(m)) for m in (0, 1, 2)})
_reference_records = {}


@pytest.mark.parametrize("mode", list(MODES))
def test_words_19_to_25_are_the_read_back(mode):
    """On the lifted tiny scene, per step mode: the record's position and velocity are sph_read_position / sph_read_velocity right
    after the step at the particle's original id, and the whole record is the one every other mode gives."""
    hip, bodies, case = lifted_solver("tiny", **MODES[mode])
    rec = hip.wall_measure(A)
    pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
    orig = hip.read_particleIndex_buffer()[:, 1].astype(np.int64)
    moving = pos[orig, 3].astype(np.int32) != 3
    assert moving.sum() == case["sc"]["numOfLiquidP"] and rec[:, 26].sum() >= 1 and rec[:, 27].sum() >= 1
    assert np.array_equal(u32(rec[moving, 19:22]), u32(pos[orig[moving], :3])), first_diff(rec[moving, 19:22], pos[orig[moving], :3], u32)
    assert np.array_equal(u32(rec[moving, 22:26]), u32(vel[orig[moving]])), first_diff(rec[moving, 22:26], vel[orig[moving]], u32)
    assert not rec[~moving].any()
    ref = _reference_records.setdefault("tiny", rec)
    assert np.array_equal(u32(rec), u32(ref)), "mode %s against mode %s" % (mode, list(MODES)[0])
    hip.close()


def test_words_19_to_25_at_the_integrate_stage_with_elastic_matter():
    hip, bodies, case = lifted_solver("tiny_elastic", staged=True, stop_at_integrate=True)
    N = hip.N
    rec = hip.wall_measure(sphmi.WALL_ALL)
    pos = hip.buffer("position").reshape(-1, 4)[:N]
    vel = hip.buffer("velocity").reshape(-1, 4)[:N]
    orig = hip.read_particleIndex_buffer()[:, 1].astype(np.int64)
    moving = pos[orig, 3].astype(np.int32) != 3
    assert (pos[orig, 3].astype(np.int32) == 2).any()
    assert np.array_equal(u32(rec[moving, 19:22]), u32(pos[orig[moving], :3])) and np.array_equal(u32(rec[moving, 22:26]), u32(vel[orig[moving]]))
    # the membrane stages then rewrite positions: the record is of the integrate stage, and stays what it was
    for st in scenes.STAGE_SEQUENCE[scenes.STAGE_SEQUENCE.index("integrate") + 1:]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert np.array_equal(u32(hip.wall_measure(sphmi.WALL_ALL)), u32(rec))
    hip.close()


# ---------------------------------------------------------------------------------------------- variants
def test_selection_variant(live):
    hip = live.hip
    full = hip.wall_measure(A)
    cfg = hip.cfg
    n = hip.select(region=(-np.inf, -np.inf, -np.inf, np.inf, f32(6) * f32(cfg.r0), np.inf), types=(1, 2))  # the layers above the floor
    idx = hip.selection()[0]
    got = hip.wall_measure(A, selection=True)
    assert 0 < n < hip.N and got.shape == (n, 32) and np.array_equal(u32(got), u32(full[idx]))
    if live.name != "tiny_elastic":
        assert got[:, 26].sum() == full[:, 26].sum() > 0
    n2 = hip.select(types=(1, 2), terms=[("surface", 0.05, np.inf)])  # not a contiguous run
    idx2 = hip.selection()[0]
    assert 0 < n2 < hip.N and np.array_equal(u32(hip.wall_measure(sphmi.WALL_NO_BODY, selection=True)), u32(hip.wall_measure(sphmi.WALL_NO_BODY)[idx2]))
    assert hip.select(region=(-9, -9, -9, -1, -1, -1)) == 0 and hip.wall_measure(A, selection=True).shape == (0, 32)


def test_rows_without_a_16_bit_copy():
    """A dense cube standing on the floor: its particles take findNeighbors' exact walk, whose rows exist in 32 bits only, and the
    bottom layers touch the floor in the first step. Both calls and both instantiations against the restatement, and once more on
    the certainly-wide rows that hold a wall alone."""
    sc = wall_cases.dense_on_floor()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    inf = np.inf
    na = hip.body_define_region(A, (-inf, -inf, -inf, f32(5) * f32(cfg.r0), f32(cfg.r0), inf))  # the cube stands on the body's edge
    assert na > 0
    hip.step(0)
    counters = hip.buffer("debugCounters")[:4].astype(np.int64)
    canon = scenes.canonical(hip.buffer, hip.N)
    crowded = np.zeros(hip.N, bool)
    crowded[scenes.crowded_particles(canon, cfg.h)] = True
    bodies = {A: hip.body_read(A)[0]}
    state, walls = restatement(hip, bodies, [A, wr.ALL, wr.NO_BODY])
    w = walls[wr.ALL]
    wide_wall = crowded & (w.records[:, 9] > 0)
    print("dense cube: %d crowded, %d of them with a wall in the row, %d in contact, %d reflected; debugCounters[0..3] = %s" % (
        crowded.sum(), wide_wall.sum(), (wide_wall & w.contact).sum(), (wide_wall & w.reflected).sum(), counters.tolist()))
    assert int(counters[0] + counters[1]) >= crowded.sum() and wide_wall.sum() >= 100
    assert (wide_wall & w.contact).sum() >= 10 and (wide_wall & w.reflected).sum() >= 10
    rg = regions_of(cfg, 3)
    for slot in (A, wr.ALL, wr.NO_BODY):
        rec = hip.wall_measure(slot)
        want = walls[slot].records
        assert np.array_equal(u32(rec), u32(want)), "set %d: %s" % (slot, first_diff(rec, want, u32))
        assert np.array_equal(u32(rec[wide_wall]), u32(want[wide_wall])) and (want[wide_wall, 9] > 0).any()
        got = hip.wall_diagnostics(slot, rg)
        assert np.array_equal(u64(got), u64(wr.diag_records(state, want, rg, (1, 2))))
    index = np.flatnonzero(wide_wall).astype(np.int32)
    assert hip.select(region=(-inf, -inf, -inf, inf, f32(4) * f32(cfg.r0), inf), types=(1,)) >= index.size
    idx = hip.selection()[0]
    assert np.isin(index, idx).all()
    assert np.array_equal(u32(hip.wall_measure(A, selection=True)), u32(walls[A].records[idx]))
    hip.close()


def test_a_pose_after_the_step_leaves_the_answer_unchanged(live):
    hip = live.hip
    rg = regions_of(hip.cfg, 3)
    before = (hip.wall_measure(A), hip.wall_diagnostics(A, rg), hip.wall_measure(sphmi.WALL_ALL), hip.wall_measure(sphmi.WALL_NO_BODY))
    pos0 = hip.read_position_buffer().copy()
    vel0 = hip.read_velocity_buffer().copy()
    move = hip.body_set_pose(A, frames.pose_compose(frames.pose_translate((0.0, 0.7 * float(hip.cfg.r0), 0.0)), live.case["pose"]))
    assert move > 0 and not np.array_equal(u32(hip.read_position_buffer()), u32(pos0))
    after = (hip.wall_measure(A), hip.wall_diagnostics(A, rg), hip.wall_measure(sphmi.WALL_ALL), hip.wall_measure(sphmi.WALL_NO_BODY))
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    hip.body_set_pose(A, live.case["pose"])  # back where the step left it, for the tests that follow
    assert np.array_equal(u32(hip.read_position_buffer()), u32(pos0)) and np.array_equal(u32(hip.read_velocity_buffer()), u32(vel0))


def test_calls_are_read_only():
    """Every exported buffer, a selection and the following steps are unchanged by the two calls."""
    a, bodies, case = lifted_solver("tiny_jitter")
    b, _, _ = lifted_solver("tiny_jitter")
    rg = regions_of(case["cfg"], 5)
    for it in range(case["steps"] + 1, case["steps"] + 4):
        assert a.select(None, (1, 2), [("surface", 0.05, np.inf)]) > 0
        sel = a.selection()
        before = {n: a.buffer(n) for n in BUFFERS}
        first = [a.wall_measure(s) for s in (A, B, sphmi.WALL_ALL, sphmi.WALL_NO_BODY)] + [a.wall_measure(A, selection=True), a.wall_diagnostics(B, rg)]
        again = [a.wall_measure(s) for s in (A, B, sphmi.WALL_ALL, sphmi.WALL_NO_BODY)] + [a.wall_measure(A, selection=True), a.wall_diagnostics(B, rg)]
        for x, y in zip(first, again):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
        for x, y in zip(sel, a.selection()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        a.step(it)
        b.step(it)
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- the calling rules
def _rc(hip, slot, from_selection=0, regions=None, count=1, mask=0x6, n=None):
    out = np.empty((max(hip.N if n is None else n, 1), 32), np.float32)
    rg = np.array([diag_ref.EVERYTHING] * max(count, 1), np.float32) if regions is None else np.ascontiguousarray(regions, np.float32)
    tot = np.empty((max(count, 1), 32), np.float64)
    L, h = hip._L, hip._h
    return (L.sph_wall_measure(h, slot, from_selection, out.ctypes.data), L.sph_wall_diagnostics(h, slot, rg.ctypes.data, count, mask, tot.ctypes.data))


def test_calling_rules():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    ALL, NONE = sphmi.WALL_ALL, sphmi.WALL_NO_BODY
    assert _rc(hip, ALL) == (ERR_ORDER, ERR_ORDER)  # before a step
    with pytest.raises(sphmi.SphError):
        hip.wall_measure(ALL)
    with pytest.raises(sphmi.SphError):
        hip.wall_diagnostics(ALL)
    hip.step(0)
    assert _rc(hip, ALL) == (0, 0) and _rc(hip, NONE) == (0, 0)
    L, h = hip._L, hip._h
    # a free slot; a slot out of range
    for slot in (0, A, 15):
        assert _rc(hip, slot) == (ERR_ORDER, ERR_ORDER)
    assert b"holds no body" in L.sph_last_error()
    for slot in (16, -3, 1 << 20):
        assert _rc(hip, slot) == (ERR_INVALID, ERR_INVALID)
    assert b"sph_wall_diagnostics" in L.sph_last_error()
    assert hip.body_define_region(A, (-np.inf, -np.inf, -np.inf, np.inf, f32(cfg.r0), np.inf)) > 0
    assert _rc(hip, A) == (0, 0) and _rc(hip, B) == (ERR_ORDER, ERR_ORDER)
    # the selection variant
    assert _rc(hip, A, from_selection=1)[0] == ERR_ORDER  # no selection yet
    n = hip.select(types=(2,))
    assert _rc(hip, A, from_selection=1, n=n)[0] == 0
    for bad in (2, -1):
        assert _rc(hip, A, from_selection=bad)[0] == ERR_INVALID
    assert b"sph_wall_measure" in L.sph_last_error()
    assert L.sph_wall_measure(h, A, 0, None) == ERR_INVALID
    tot = np.empty((1, 32), np.float64)
    rg = np.array([diag_ref.EVERYTHING], np.float32)
    assert L.sph_wall_diagnostics(h, A, None, 1, 0x6, tot.ctypes.data) == ERR_INVALID
    assert L.sph_wall_diagnostics(h, A, rg.ctypes.data, 1, 0x6, None) == ERR_INVALID
    for mask in (0, 1, 0x10, 0x16):
        assert _rc(hip, A, mask=mask)[1] == ERR_INVALID
    for count in (0, -1, 17):
        assert _rc(hip, A, count=count)[1] == ERR_INVALID
    nan = np.array([diag_ref.EVERYTHING], np.float32)
    nan[0, 4] = np.nan
    assert _rc(hip, A, regions=nan)[1] == ERR_INVALID
    with pytest.raises(sphmi.SphError):
        hip.wall_diagnostics(A, np.zeros((17, 6), np.float32))
    hip.step(1)  # a further step: the selection is of another state
    assert _rc(hip, A, from_selection=1, n=n)[0] == ERR_ORDER and _rc(hip, A) == (0, 0)
    # a half-done staged step: SPH_ERR_ORDER from its first stage until its integrate stage has run
    seq = scenes.STAGE_SEQUENCE
    k = seq.index("integrate")
    for i, st in enumerate(seq[:k]):
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        if i in (0, 1, 7, k - 1):
            assert _rc(hip, A) == (ERR_ORDER, ERR_ORDER), st
    assert b"before the stage" in L.sph_last_error()
    hip._run_pcisph_integrate(2)
    assert _rc(hip, A) == (0, 0)
    for st in seq[k + 1:]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        assert _rc(hip, A) == (0, 0), st
    # after an edit the sorted state is gone
    assert hip.remove_region((-np.inf, f32(0.5) * f32(cfg.ymax), -np.inf, np.inf, np.inf, np.inf), (1,)) > 0
    assert _rc(hip, A) == (ERR_ORDER, ERR_ORDER) and _rc(hip, ALL) == (ERR_ORDER, ERR_ORDER)
    hip.step(3)
    assert _rc(hip, A) == (0, 0)
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc(hip, sphmi.WALL_ALL) == (ERR_INVALID, ERR_INVALID)
    hip.close()


def test_three_tree_levels_and_several_pieces_on_more_than_a_million_particles():
    """More than 1024^2 particles: the third level of the tree runs and the records travel in several pieces (the piece loop is
    the one sph_force_measure runs, with this call's launch and record width). The 1.3 M box of test_forces.py with half of its
    floor, a body, lifted 2.4 r0 into the liquid before the first step."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    cfg = sc["cfg"]
    assert cfg.particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    inf = np.inf
    assert hip.body_define_region(A, (-inf, -inf, -inf, f32(0.5) * f32(cfg.xmax), f32(cfg.r0), inf)) > 0
    hip.body_set_pose(A, frames.pose_translate((0.0, 2.4 * float(f32(cfg.r0)), 0.0)))
    hip.step(0)
    state, walls = restatement(hip, {A: hip.body_read(A)[0]}, [A])
    want = walls[A].records
    rec = hip.wall_measure(A)
    assert np.array_equal(u32(rec), u32(want)), first_diff(rec, want, u32)
    rg = regions_of(cfg, 2)
    got = hip.wall_diagnostics(A, rg, (1, 2, 3))
    assert np.array_equal(u64(got), u64(wr.diag_records(state, want, rg, (1, 2, 3)))) and got[0, 0] == hip.N
    print("1.3 M: %d particles with a slot of the body, %d in contact, %d reflected" % ((want[:, 9] > 0).sum(), want[:, 26].sum(), want[:, 27].sum()))
    assert (want[:, 6] > 0).sum() > 1000 and want[:, 27].sum() > 0 and np.abs(want[:, 10:19]).max() > 0
    assert (want[:524288, 6] > 0).any() and (want[524288:, 6] > 0).any()  # on both sides of the first piece's end (64 MiB / 128 B)
    pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
    orig, moving = state["orig"], walls[A].moving
    assert np.array_equal(u32(rec[moving, 19:22]), u32(pos[orig[moving], :3])) and np.array_equal(u32(rec[moving, 22:26]), u32(vel[orig[moving]]))
    hip.close()


def test_cpp_driver_wall_load():
    """sphmi_run --wall-load-every prints, per defined body, the numbers of frames.wall_summary."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    r0 = float(f32(cfg.r0))
    # the lift of wall_cases: three steps, then the floor 2.4 r0 up at once; the line after the step that follows
    lift = "%.17g" % (2.4 * r0)
    args = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--quiet", "--body-region", "-inf", "-inf", "-inf", "inf",
            "%.9g" % r0, "inf", "--body-velocity", "0", lift, "0", "--body-from", "3", "--wall-load-every", "2"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("_wall: step")]
    assert len(lines) == 2 and lines[0].startswith("_wall: step 2 body 0 (members 256): contact n 0 ") and lines[1].startswith("_wall: step 4 body 0"), r.stdout
    hip = scenes.hip_for(sc)
    assert hip.body_define_region(0, (-np.inf, -np.inf, -np.inf, np.inf, f32(r0), np.inf)) == 256
    for it in range(4):
        if it >= 3:
            hip.body_set_pose(0, frames.pose_translate(np.array([0.0, float(lift), 0.0]) * float(it - 3 + 1)))
        hip.step(it)
    s = frames.wall_summary(hip.wall_diagnostics(0, types=(1,))[0], cfg.mass, cfg.timeStep)
    assert s["n_contact"] > 0 and s["n_reflected"] > 0 and s["contact_force"][1] > 0
    ln = lines[1]
    counts = ln.split("contact n")[1].split("contact force")[0].replace("shared", " ").replace("reflected", " ").split()
    assert [float(x) for x in counts] == [s["n_contact"], s["n_shared"], s["n_reflected"]]
    for key, label in (("contact_force", "contact force"), ("stage_force", "stage force"), ("body_load", "load on body"), ("body_torque", "torque on body")):
        got = [float(x) for x in ln.split(label)[1].split()[:3]]
        assert got == [float("%.9e" % x) for x in s[key]], (key, got, s[key])
    hip.close()
    # without a body: one line for all walls
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--wall-load-every", "2", "--quiet"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("_wall: step") == 2 and "body all (members 0)" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, "--steps", "1", "--wall-load-every", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip()
