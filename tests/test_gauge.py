"""GPU tests of the flow gauges (sph_gauge_define / sph_gauges_accumulate / sph_gauges_read / sph_gauges_history /
sph_gauge_crossings, include/sphmi.h): every word of the records, the totals, the history and the crossing list equal to the numpy
restatement (tests/gauge_ref.py) on the cases tests/test_gauge_host.py proves non-empty on the oracle; the exact conservation of
the particle count behind a plane against sph_diagnostics' own count; every step mode; liquid counts at the wave and chunk edges;
sparse and empty crossings; more than 2^20 particles; the ring; the call without a host wait; totals across edits; bodies moved
between the step and the call; the read-only rule; the calling rules; the driver's line. No tolerance appears anywhere: integers
are compared for equality, floats as bit patterns (the sign of a zero total, which the contract leaves open, aside)."""
import os
import subprocess

import numpy as np
import pytest

import gauge_cases as gc
import gauge_ref as gr
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
INF = np.inf
BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def zb(a):
    return gr.zero_sign_blind(a)


def first_diff(got, want):
    d = np.argwhere(zb(got) != zb(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def same(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(zb(got), zb(want))


def define(hip, gauges, slots=None):
    for slot in (gauges if slots is None else slots):
        hip.gauge_define(slot, **gauges[slot])


def solver(sc, extra=0):
    if extra:
        sc = dict(sc)
        cfg = type(sc["cfg"]).from_buffer_copy(sc["cfg"])
        cfg.capacity = cfg.particleCount + extra
        sc["cfg"] = cfg
    return scenes.hip_for(sc)


def lists_equal(got, want):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and x.dtype == y.dtype
               for x, y in zip(got, want))


# ---------------------------------------------------------------------------------------------- every word, bit for bit
SLOTS = {"16": tuple(range(16)), "1": gc.SINGLE, "spread": gc.SPREAD}


@pytest.mark.parametrize("config", list(SLOTS))
@pytest.mark.parametrize("name", list(gc.CASES))
def test_every_word_against_the_restatement(name, config):
    """Records, totals, history and crossing lists over the case's six steps, against the restatement on the ORACLE's states (the
    solver's positions are the oracle's bit for bit, which the last lines check too)."""
    c = gc.case(name)
    slots = SLOTS[config]
    hip = solver(c["sc"])
    define(hip, c["gauges"], slots)
    for slot in range(16):
        g = hip.gauge(slot)
        assert (g is not None) == (slot in slots)
        if g:
            want = c["gauges"][slot]
            assert all(np.array_equal(g[k], np.asarray(want[k], np.float32)) for k in ("origin", "u", "v"))
            assert g["plane"] == bool(want.get("plane")) and g["typeMask"] == sum(1 << t for t in c["types"]) and g["field"] is None
    hip.gauges_history(gc.STEPS)
    totals = gr.empty_totals()
    for k in range(gc.STEPS):
        hip.step(k)
        rec = hip.gauges_accumulate()
        want = np.zeros((16, 16))
        want[list(slots)] = c["records"][k][list(slots)]
        assert rec.dtype == np.float64 and same(rec, want), "%s step %d: %s" % (name, k, first_diff(rec, want))
        totals = gr.accumulate(totals, want, slots, k)
        for slot in slots if k in (1, 3) else slots[:1]:
            got = hip.gauge_crossings(slot)
            ref = gr.crossing_list(c["states"][k], c["gauges"][slot])
            assert lists_equal(got, ref), (name, k, slot, got[0].size, ref[0].size)
            assert got[0].size == want[slot, 0] + want[slot, 8]
            if name == "elastic" and slot == 1 and k == 1:  # elastic particles cross too
                assert (c["states"][k]["a"][got[0], 3].astype(np.int32) == 2).sum() >= 8
    tot, calls = hip.gauges()
    assert calls == gc.STEPS and same(tot, totals), first_diff(tot, totals)
    assert (tot[list(slots), 16] == gc.STEPS).all() and (tot[list(slots), 0] >= 8).all() and (tot[list(slots), 8] >= 8).all()
    hist = hip.gauge_history(0, gc.STEPS)
    for k in range(gc.STEPS):
        want = np.zeros((16, 16))
        want[list(slots)] = c["records"][k][list(slots)]
        assert same(hist[k], want)
    st = gr.solver_state(hip)
    assert scenes.bits_equal(st["pos"], c["states"][-1]["pos"]) and scenes.bits_equal(st["a"], c["states"][-1]["a"])
    hip.close()


def test_conservation_on_the_device():
    """Net crossings of the plane x = c over K steps == the change of sph_diagnostics' own count in the region x >= c. The
    diagnostics read the sorted state, one step behind: after step 1 they count the initial state, after step K + 1 the state K
    steps later."""
    c = gc.case("tiny_jitter")
    hip = solver(c["sc"])
    for slot, axis in ((0, 0), (1, 1), (2, 2)):
        hip.gauge_define(slot, **c["gauges"][slot])
    regions = []
    for slot, axis in ((0, 0), (1, 1), (2, 2)):
        rg = [-INF, -INF, -INF, INF, INF, INF]
        rg[axis] = float(c["gauges"][slot]["origin"][axis])
        regions.append(rg)
    hip.step(0)
    before = hip.diagnostics(regions, types=(1,))[:, 0].copy()
    K = 5
    for k in range(1, K + 1):
        hip.gauges_accumulate(read=False)
        hip.step(k)
    after = hip.diagnostics(regions, types=(1,))[:, 0]
    tot, calls = hip.gauges()
    assert calls == K
    for slot in range(3):
        assert tot[slot, 0] - tot[slot, 8] == after[slot] - before[slot], (slot, tot[slot, 0], tot[slot, 8], before[slot], after[slot])
        assert tot[slot, 0] >= 8 and tot[slot, 8] >= 8
    hip.close()


# ---------------------------------------------------------------------------------------------- step modes
def _chunks(n):
    return lambda hip: hip.set_step_chunks(n)


def _pipeline(depth):
    def setup(hip):
        hip.set_step_chunks(4)
        hip.set_step_pipeline(depth)
    return setup


def _skip(mode):
    return lambda hip: hip.set_wave_skip(mode)


MODES = {"staged": dict(staged=True), "chunks-2": dict(setup=_chunks(2)), "chunks-5": dict(setup=_chunks(5)), "chunks-16": dict(setup=_chunks(16))}
MODES.update({"pipeline-%d" % d: dict(setup=_pipeline(d)) for d in range(0, 7)})
MODES.update({"wave-skip-%d" % m: dict(setup=_skip(m)) for m in (0, 1, 2)})


@pytest.mark.parametrize("mode", list(MODES))
def test_the_record_does_not_depend_on_the_step_mode(mode):
    c = gc.case("tiny")
    hip = solver(c["sc"])
    if MODES[mode].get("setup"):
        MODES[mode]["setup"](hip)
    define(hip, c["gauges"])
    for k in range(3):
        scenes.staged_step(hip, k) if MODES[mode].get("staged") else hip.step(k)
        rec = hip.gauges_accumulate()
        assert same(rec, c["records"][k]), "%s step %d: %s" % (mode, k, first_diff(rec, c["records"][k]))
    hip.close()


def test_with_elastic_matter_the_positions_are_final_after_the_finalize_stage():
    c = gc.case("elastic")
    hip = solver(c["sc"])
    define(hip, c["gauges"])
    out = np.zeros((16, 16))
    n = np.zeros(1, np.int64)
    seq = scenes.STAGE_SEQUENCE
    for k in range(2):
        for st in seq[:seq.index("integrate")]:
            getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        hip._run_pcisph_integrate(k)
        assert hip._L.sph_gauges_accumulate(hip._h, out.ctypes.data) == ERR_ORDER and b"half done" in hip._L.sph_last_error()
        assert hip._L.sph_gauge_crossings(hip._h, 0, n.ctypes.data) == ERR_ORDER
        for st in seq[seq.index("integrate") + 1:]:
            getattr(hip, scenes.HIP_STAGE_METHOD[st])()
        rec = hip.gauges_accumulate()
        assert same(rec, c["records"][k]), first_diff(rec, c["records"][k])
    assert hip.gauges()[1] == 2
    hip.close()


# ---------------------------------------------------------------------------------------------- shapes
def _gauges_for(sc, types=(1,)):
    return gc.gauges_of(sc, types)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_liquid_counts_at_wave_and_chunk_edges(n):
    sc = gc.seeded(gc.liquid_only(n))
    assert (sc["position"][:, 3].astype(np.int32) == 1).sum() == n
    hip = solver(sc)
    gauges = _gauges_for(gc.liquid_only(1025))  # laid out on the whole column, whatever part of it exists
    define(hip, gauges)
    crossings = 0
    for k in range(3):
        hip.step(k)
        st = gr.solver_state(hip)
        want = gr.records(st, gauges)
        rec = hip.gauges_accumulate()
        assert same(rec, want), "n %d step %d: %s" % (n, k, first_diff(rec, want))
        crossings += int(want[:, 0].sum() + want[:, 8].sum())
        for slot in (0, 7):
            assert lists_equal(hip.gauge_crossings(slot), gr.crossing_list(st, gauges[slot]))
    assert crossings > 0 or n == 1
    hip.close()


def test_a_single_lane_and_no_lane():
    """At rest nothing crosses: every record word is +0.0, the list is empty, the call words stay -1. Then the one liquid particle
    that is the last lane of its wave, highest in the sorted order, is sent through a plane just behind it: one crossing, found
    by that lane alone."""
    sc = scenes.SCENES["tiny"]()
    hip = solver(sc)
    gauges = _gauges_for(sc)
    define(hip, gauges)
    hip.step(0)
    rec = hip.gauges_accumulate()
    assert not rec.view(np.uint64).any()
    tot, calls = hip.gauges()
    assert calls == 1 and (tot[:, 16] == 1).all() and (tot[:, 17:] == -1).all() and not tot[:, :16].any()
    got = hip.gauge_crossings(0)
    assert all(x.size == 0 for x in got) and got[3].shape == (0, 3)
    st = gr.solver_state(hip)
    liquid = st["a"][:, 3].astype(np.int32) == 1
    j = int(np.flatnonzero(liquid & (np.arange(hip.N) % 64 == 63))[-1])
    o = int(st["orig"][j])
    hip.close()
    # the same scene with that particle moving along +x, and a plane 0.05 r0 in front of it
    sc2 = dict(sc)
    vel = np.array(sc["velocity"], np.float32)
    vel[o, 0] = f32(0.25)
    sc2["velocity"] = vel
    r0 = f32(sc["cfg"].r0)
    plane = frames.gauge_plane((sc["position"][o, 0] + f32(0.05) * r0, 0, 0), (1, 0, 0))
    hip = solver(sc2)
    hip.gauge_define(9, **plane)
    hip.step(0)
    rec = hip.gauges_accumulate()
    st = gr.solver_state(hip)
    assert int(np.flatnonzero(st["orig"] == o)[0]) == j and j % 64 == 63
    want = gr.records(st, {9: plane})
    assert same(rec, want) and rec[9, 0] == 1 and rec[9, 8] == 0 and not rec[:9].any()
    idx, ids, way, tab = hip.gauge_crossings(9)
    assert idx.tolist() == [j] and ids.tolist() == [o] and way.tolist() == [1] and 0 < tab[0, 0] < 1
    tot, _ = hip.gauges()
    assert tot[9, 17] == 0 and tot[9, 18] == -1 and tot[9, 19] == 0
    hip.close()


def test_two_upper_tree_levels_on_more_than_a_million_particles():
    sc = gc.seeded(scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff))
    cfg = sc["cfg"]
    assert cfg.particleCount > 1024 * 1024
    hip = solver(sc)
    all16 = _gauges_for(sc)
    gauges = {s: all16[s] for s in (0, 4, 7, 14)}
    define(hip, gauges)
    hip.step(0)
    rec = hip.gauges_accumulate()
    st = gr.solver_state(hip)
    want = gr.records(st, gauges)
    assert same(rec, want), first_diff(rec, want)
    print("1.3 M: crossings per gauge", {s: (int(want[s, 0]), int(want[s, 8])) for s in gauges})
    # half of the 85 x 125 particles of the column in front of the plane move towards it; the others see at least the 8 the cases ask for
    assert want[0, 0] > 1000 and (want[[4, 7, 14], 0] >= 8).all() and (want[[7, 14], 8] >= 8).all()
    assert lists_equal(hip.gauge_crossings(7), gr.crossing_list(st, gauges[7]))
    got = hip.gauge_crossings(0)
    assert lists_equal(got, gr.crossing_list(st, gauges[0])) and got[0][0] < 1 << 19 and got[0][-1] > 1 << 20  # across the scan's blocks
    hip.close()


# ---------------------------------------------------------------------------------------------- ring, no wait
def test_the_ring_wraps():
    c = gc.case("tiny")
    hip = solver(c["sc"])
    define(hip, c["gauges"])
    hip.gauges_history(4)
    for k in range(6):
        hip.step(k)
        hip.gauges_accumulate(read=False)
    hist = hip.gauge_history(2, 4)  # rows 2, 3, 0, 1 of the ring: two runs
    for k in range(2, 6):
        assert same(hist[k - 2], c["records"][k]), k
    assert same(hip.gauge_history(5, 1)[0], c["records"][5]) and hip.gauge_history(3, 0).shape == (0, 16, 16)
    L, h = hip._L, hip._h
    out = np.zeros((6, 16, 16))
    calls = np.zeros(1, np.int64)
    for first, count in ((1, 1), (1, 5), (0, 1), (5, 2), (6, 1), (-1, 1)):
        assert L.sph_gauges_read_history(h, first, count, out.ctypes.data, calls.ctypes.data) == ERR_INVALID, (first, count)
        assert calls[0] == 6
    assert b"not all in the ring" in L.sph_last_error()
    assert L.sph_gauges_read_history(h, 2, -1, out.ctypes.data, None) == ERR_INVALID
    assert L.sph_gauges_read_history(h, 2, 1, None, None) == ERR_INVALID
    # a new ring starts empty: calls made before it are not in it
    hip.gauges_history(8)
    assert L.sph_gauges_read_history(h, 5, 1, out.ctypes.data, None) == ERR_INVALID
    hip.step(6)
    hip.gauges_accumulate(read=False)
    assert hip.gauge_history(6, 1).shape == (1, 16, 16) and hip.gauges()[1] == 7
    hip.gauges_history(0)
    assert L.sph_gauges_read_history(h, 6, 1, out.ctypes.data, None) == ERR_ORDER
    for rows in (-1, sphmi.GAUGE_HISTORY_MAX + 1):
        assert L.sph_gauges_history(h, rows) == ERR_INVALID
    hip.close()


def test_without_a_host_wait():
    c = gc.case("tiny_jitter")
    a, b = solver(c["sc"]), solver(c["sc"])
    for hip in (a, b):
        define(hip, c["gauges"])
        hip.gauges_history(4)
    for k in range(3):
        a.step(k)
        b.step(k)
        assert a.gauges_accumulate(read=False) is None
        rec = b.gauges_accumulate(read=True)
        assert same(a.gauge_history(k, 1)[0], rec) and same(rec, c["records"][k])
    assert same(a.gauges()[0], b.gauges()[0])
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- totals, edits, bodies
def test_totals_across_edits_and_reset_redefine_release():
    c = gc.case("tiny_jitter")
    cfg = c["cfg"]
    hip = solver(c["sc"], extra=600)
    gauges = c["gauges"]
    define(hip, gauges)
    totals = gr.empty_totals()
    out = np.zeros((16, 16))
    r0 = f32(cfg.r0)
    call = 0
    for k in range(5):
        if k == 2:
            assert hip.remove_region((-INF, -INF, -INF, float(gauges[0]["origin"][0]) - 4 * float(r0), INF, INF), (1,)) > 50
            assert hip._L.sph_gauges_accumulate(hip._h, out.ctypes.data) == ERR_ORDER  # removed particles are not crossings
        if k == 3:
            top = float(c["sc"]["position"][:c["sc"]["numOfLiquidP"], 1].max())  # above the liquid, aimed at the plane x = c
            o = (float(gauges[0]["origin"][0]) - 1.5 * float(r0), top + 1.5 * float(r0), float(gauges[2]["origin"][2]))
            assert hip.emit_lattice(o, (float(r0),) * 3, (2, 2, 6), velocity=(0.9, 0, 0)) == 24
            n = np.zeros(1, np.int64)
            assert hip._L.sph_gauge_crossings(hip._h, 0, n.ctypes.data) == ERR_ORDER
        hip.step(k)
        want = gr.records(gr.solver_state(hip), gauges)
        rec = hip.gauges_accumulate()
        assert same(rec, want), "step %d: %s" % (k, first_diff(rec, want))
        totals = gr.accumulate(totals, want, range(16), call)
        call += 1
        assert same(hip.gauges()[0], totals)
    assert totals[0, 0] > 0 and totals[0, 8] > 0
    # reset one, then all; a redefinition and a release clear their slot alone
    hip.gauges_reset(4)
    totals[4] = gr.empty_totals()[4]
    assert same(hip.gauges()[0], totals)
    hip.gauge_define(7, **gauges[8])
    totals[7] = gr.empty_totals()[7]
    hip.gauge_define(9)
    totals[9] = gr.empty_totals()[9]
    assert same(hip.gauges()[0], totals) and hip.gauge(9) is None and hip.gauge(7)["plane"]
    hip.gauge_define(9)  # releasing a free slot: a no-op
    hip.step(5)
    rec = hip.gauges_accumulate()
    st = gr.solver_state(hip)
    now = dict(gauges)
    now[7] = gauges[8]
    del now[9]
    want = gr.records(st, now)
    assert same(rec, want) and not rec[9].any() and same(rec[7], rec[8])
    totals = gr.accumulate(totals, want, now, call)
    assert same(hip.gauges()[0], totals) and totals[4, 16] == 1 and totals[0, 16] == 6 and hip.gauges()[1] == 6
    hip.gauges_reset()
    assert same(hip.gauges()[0], gr.empty_totals()) and hip.gauges()[1] == 6
    hip.close()


def test_bodies_moved_between_the_step_and_the_call_change_nothing():
    c = gc.case("tiny")
    cfg = c["cfg"]
    hip = solver(c["sc"])
    define(hip, c["gauges"])
    assert hip.body_define_region(3, (-INF, -INF, -INF, INF, f32(cfg.r0), INF)) > 0
    ref = hip.body_read(3)[1]
    com = ref[:, :3].astype(np.float64).mean(0)
    hip.body_set_dynamics(3, mass=1.0e3, com=com, position=com, velocity=(0.0, 0.02, 0.0), locks="xyzr")
    for k in range(2):
        hip.step(k)
        pos = hip.read_position_buffer().copy()
        adv = hip.bodies_advance()
        assert adv[3, 0] == 0 and adv[3, 3] > 0
        assert hip.body_define_region(5, (-INF, f32(cfg.ymax) - f32(cfg.r0), -INF, INF, INF, INF)) > 0
        assert hip.body_set_pose(5, frames.pose_translate((0.0, -0.3 * float(f32(cfg.r0)), 0.0))) > 0
        assert not np.array_equal(hip.read_position_buffer(), pos)
        rec = hip.gauges_accumulate()
        assert same(rec, gr.records(dict(gr.solver_state(hip), pos=pos), c["gauges"]))
        if k == 0:
            assert same(rec, c["records"][0])  # the first step has not seen a moved wall yet
        hip.body_set_pose(5, frames.pose_identity())
    hip.close()


def test_calls_are_read_only():
    """Exported buffers, selection, labelling, fields, mesh, body state and the following steps are unchanged by every call."""
    c = gc.case("tiny_jitter")
    a, b = solver(c["sc"]), solver(c["sc"])
    cfg = c["cfg"]
    define(a, c["gauges"])
    a.gauges_history(2)
    a.field_create(1, np.arange(a.N, dtype=np.float32))
    a.gauge_define(6, field=1, **{k: c["gauges"][6][k] for k in ("origin", "u", "v")})
    assert a.body_define_region(2, (-INF, -INF, -INF, INF, f32(cfg.r0), INF)) > 0
    lo = [f32(3) * f32(cfg.r0)] * 3
    for k in range(3):
        a.step(k)
        b.step(k)
        assert a.select(None, (1,), [("surface", 0.05, INF)]) > 0
        sel = a.selection()
        assert a.label_components()[1] >= 1
        labels = a.components()
        verts = a.extract_surface(lo, [f32(cfg.r0)] * 3, (10, 8, 12))[0]
        normals = a.surface_normals()
        assert verts.shape[0] > 0
        before = {n: a.buffer(n) for n in BUFFERS}
        field, body = a.field_read(1).copy(), a.body_read(2)
        first = a.gauges_accumulate()
        a.gauges_accumulate(read=False)
        lists = [a.gauge_crossings(s) for s in (0, 6, 7)]
        a.gauges(), a.gauge_history(2 * k, 2), a.gauges_reset(3), a.gauge(3)
        assert same(a.gauge_history(2 * k + 1, 1)[0], first)
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), a.buffer(n).view(np.uint8)), n
        for x, y in zip(sel, a.selection()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for x, y in zip(labels, a.components()):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        assert np.array_equal(field, a.field_read(1)) and lists_equal(body, a.body_read(2))
        assert np.array_equal(normals.view(np.uint32), a.surface_normals().view(np.uint32))  # the mesh is still current
        assert lists_equal(lists[0], a.gauge_crossings(0))
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    a.close()
    b.close()


def test_the_crossing_list_feeds_a_drain_and_goes_stale():
    c = gc.case("tiny")
    hip = solver(c["sc"])
    define(hip, c["gauges"], (0,))
    hip.step(0)
    idx, ids, way, tab = hip.gauge_crossings(0)
    assert lists_equal((idx, ids, way, tab), gr.crossing_list(c["states"][0], c["gauges"][0])) and ids.size >= 8
    n0 = hip.N
    pos = hip.read_position_buffer().copy()
    L, h = hip._L, hip._h
    assert hip.remove_ids(ids[way > 0]) == int((way > 0).sum()) and hip.N == n0 - int((way > 0).sum())
    keep = np.ones(n0, bool)
    keep[ids[way > 0]] = False
    assert scenes.bits_equal(hip.read_position_buffer(), pos[keep])
    assert L.sph_read_gauge_crossings(h, None, None, None, None) == ERR_ORDER and b"state has changed" in L.sph_last_error()
    hip.step(1)
    assert L.sph_read_gauge_crossings(h, None, None, None, None) == ERR_ORDER
    n = hip.gauge_crossings(0)[0].size
    assert L.sph_read_gauge_crossings(h, None, None, None, None) == 0
    hip.step(2)  # stale after the next step
    buf = np.zeros(max(n, 1), np.int32)
    assert L.sph_read_gauge_crossings(h, buf.ctypes.data, None, None, None) == ERR_ORDER
    hip.close()


def test_field_flux_of_a_painted_dye():
    c = gc.case("tiny_jitter")
    hip = solver(c["sc"])
    g = c["gauges"]
    x0 = float(g[0]["origin"][0])
    hip.field_create(2)
    assert hip.field_set_region(2, 2.5, (-INF, -INF, -INF, x0, INF, INF), (1,)) > 100  # the dye stands in front of the plane
    gauges = {0: dict(g[0], field=2), 4: dict(g[4], field=2), 8: g[8]}
    define(hip, gauges)
    assert hip.gauge(0)["field"] == 2 and hip.gauge(8)["field"] is None
    flux = 0.0
    for k in range(3):
        hip.step(k)
        rec = hip.gauges_accumulate()
        want = gr.records(gr.solver_state(hip, fields=(2,)), gauges)
        assert same(rec, want), first_diff(rec, want)
        assert not rec[8, [5, 13]].any()
        if k == 0:  # in the first step only dyed liquid goes forward, and nothing comes back
            assert rec[0, 5] == 2.5 * rec[0, 0] > 0 and rec[0, 8] == 0 and rec[4, 5] == 2.5 * rec[4, 0] > 0
        flux += frames.gauge_summary(rec[0], hip.cfg)["field_flux"]
    tot = hip.gauges()[0]
    assert flux == tot[0, 5] - tot[0, 13] > 0
    # a gauge whose field is gone refuses the call until it is redefined
    hip.field_release(2)
    out = np.zeros((16, 16))
    assert hip._L.sph_gauges_accumulate(hip._h, out.ctypes.data) == ERR_ORDER and b"released" in hip._L.sph_last_error()
    hip.gauge_define(0, **g[0])
    hip.gauge_define(4)
    assert hip.gauges_accumulate().shape == (16, 16)
    hip.close()


# ---------------------------------------------------------------------------------------------- the calling rules
def _gauge(origin=(1, 1, 1), u=(0, 1, 0), v=(0, 0, 1), mask=2, field=-1, flags=0):
    g = sphmi.SphGauge()
    g.origin, g.u, g.v = (f32(origin[0]), f32(origin[1]), f32(origin[2])), tuple(map(float, u)), tuple(map(float, v))
    g.typeMask, g.fieldSlot, g.flags = mask, field, flags
    return g


def test_calling_rules():
    import ctypes as C
    sc = scenes.SCENES["tiny_elastic"]()
    hip = solver(sc)
    L, h = hip._L, hip._h
    out, tot, n = np.zeros((16, 16)), np.zeros((16, 20)), np.zeros(1, np.int64)
    acc = lambda: L.sph_gauges_accumulate(h, out.ctypes.data)
    cross = lambda slot=0: L.sph_gauge_crossings(h, slot, n.ctypes.data)
    define_rc = lambda slot, g: L.sph_gauge_define(h, slot, C.byref(g) if g is not None else None)
    # definitions
    assert define_rc(0, _gauge()) == 0 and define_rc(15, _gauge(mask=6, flags=1)) == 0
    for bad in (_gauge(origin=(np.nan, 0, 0)), _gauge(u=(0, np.inf, 0)), _gauge(v=(0, 0, -np.inf)), _gauge(u=(0, 0, 2)), _gauge(u=(0, 0, 0)),
                _gauge(mask=0), _gauge(mask=8), _gauge(mask=3), _gauge(mask=0xE), _gauge(field=0), _gauge(field=4), _gauge(field=-2),
                _gauge(flags=2), _gauge(flags=3)):
        assert define_rc(1, bad) == ERR_INVALID
        assert hip.gauge(1) is None
    assert b"sph_gauge_define" in L.sph_last_error()
    assert define_rc(0, _gauge(mask=0)) == ERR_INVALID and hip.gauge(0)["typeMask"] == 2  # a refused definition leaves the slot as it was
    for slot in (-1, 16, 1 << 20):
        assert define_rc(slot, _gauge()) == ERR_INVALID and define_rc(slot, None) == ERR_INVALID and cross(slot) == ERR_INVALID
        assert L.sph_gauge_get(h, slot, None, n.ctypes.data) == ERR_INVALID and L.sph_gauges_reset(h, slot if slot != -1 else -2) == ERR_INVALID
    hip.field_create(0)
    assert define_rc(2, _gauge(field=0)) == 0 and define_rc(2, None) == 0 and define_rc(2, None) == 0
    assert L.sph_gauge_get(h, 0, None, None) == ERR_INVALID and L.sph_gauges_read(h, None, None) == ERR_INVALID
    assert L.sph_gauges_read(h, tot.ctypes.data, None) == 0 and (tot[:, 17:] == -1).all() and not tot[:, :17].any()
    # order: before a step; with no gauge; a free slot
    assert acc() == ERR_ORDER and cross() == ERR_ORDER and b"before the stage" in L.sph_last_error()
    assert L.sph_read_gauge_crossings(h, None, None, None, None) == ERR_ORDER
    hip.step(0)
    assert acc() == 0 and L.sph_gauges_accumulate(h, None) == 0 and cross() == 0 and cross(15) == 0
    assert cross(3) == ERR_ORDER and b"holds no gauge" in L.sph_last_error() and L.sph_gauge_crossings(h, 0, None) == ERR_INVALID
    assert L.sph_read_gauge_crossings(h, None, None, None, None) == 0
    assert define_rc(0, None) == 0 and define_rc(15, None) == 0
    assert acc() == ERR_ORDER and b"no gauge is defined" in L.sph_last_error()
    assert define_rc(0, _gauge()) == 0
    # a half-done staged step: SPH_ERR_ORDER from its first stage until its finalize stage has run (elastic matter)
    seq = scenes.STAGE_SEQUENCE
    for i, st in enumerate(seq):
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
        if i < len(seq) - 1 and (i in (0, 1, 7) or st in ("integrate", "clearMembraneBuffers", "computeInteractionWithMembranes")):
            assert acc() == ERR_ORDER and cross() == ERR_ORDER, st
    assert acc() == 0 and cross() == 0
    # after an edit until the next step
    assert hip.remove_region((-INF, f32(0.5) * f32(sc["cfg"].ymax), -INF, INF, INF, INF), (1,)) > 0
    assert acc() == ERR_ORDER and cross() == ERR_ORDER
    assert L.sph_gauges_read(h, tot.ctypes.data, n.ctypes.data) == 0 and n[0] == 3 and tot[0, 16] == 1  # totals survive the edit
    hip.step(2)
    assert acc() == 0
    with pytest.raises(sphmi.SphError):
        hip.gauge_define(16, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    with pytest.raises(sphmi.SphError):
        hip.gauge_define(1, (0, 0, 0), (1, 0, 0), (2, 0, 0))
    with pytest.raises(sphmi.SphError):
        hip.gauge_crossings(5)
    hip.close()


def test_slab_solver_is_invalid():
    import ctypes as C
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    L, h = hip._L, hip._h
    out, cnt = np.zeros((16, 20)), np.zeros(1, np.int64)
    g = _gauge()
    rcs = [L.sph_gauge_define(h, 0, C.byref(g)), L.sph_gauge_define(h, 0, None), L.sph_gauge_get(h, 0, None, cnt.ctypes.data),
           L.sph_gauges_accumulate(h, out.ctypes.data), L.sph_gauges_read(h, out.ctypes.data, None), L.sph_gauges_reset(h, -1),
           L.sph_gauges_history(h, 4), L.sph_gauges_read_history(h, 0, 1, out.ctypes.data, None), L.sph_gauge_crossings(h, 0, cnt.ctypes.data),
           L.sph_read_gauge_crossings(h, None, None, None, None)]
    assert rcs == [ERR_INVALID] * len(rcs), rcs
    assert b"slab" in L.sph_last_error()
    hip.close()


# ---------------------------------------------------------------------------------------------- the driver
def test_cpp_driver_gauge_line():
    """sphmi_run --gauge ... --gauge-every prints the totals a Python replay of its schedule reads: an emitter blows liquid through
    a plane and a rectangle in front of it."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    n, r0 = cfg.particleCount, f32(cfg.r0)
    liq = sc["position"][:sc["numOfLiquidP"], :3]
    # the emitter stands above the liquid and fires along +x; the plane cuts its jet half a spacing in front of the lattice. Every
    # number is a float first and printed with nine digits, which the driver reads back to the same float
    o = [f32(liq[:, 0].min()), f32(liq[:, 1].max() + f32(1.25) * r0), f32(liq[:, 2].min() + f32(2) * r0)]
    x = f32(o[0] + f32(1.5) * r0)
    ro = [x, f32(o[1] - f32(0.5) * r0), f32(o[2] - f32(0.5) * r0)]
    side = f32(f32(2) * r0)
    plane = "%.9g 0 0  0 1 0  0 0 1" % x
    rect = "%.9g %.9g %.9g  0 %.9g 0  0 0 %.9g" % (ro[0], ro[1], ro[2], side, side)
    args = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "6", "--quiet", "--capacity", str(n + 400), "--emit-lattice",
            "%.9g" % o[0], "%.9g" % o[1], "%.9g" % o[2], "2", "2", "4", "--emit-spacing", "%.9g" % r0, "--emit-velocity", "0.8", "0", "0",
            "--emit-every", "2", "--gauge", plane, "--gauge-plane", "--gauge", rect, "--gauge-every", "3"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("_gauge: step")]
    assert len(lines) == 4 and lines[0].startswith("_gauge: step 3 gauge 0 plus ") and lines[3].startswith("_gauge: step 6 gauge 1 plus "), r.stdout
    hip = solver(sc, extra=400)
    hip.gauge_define(0, (x, 0, 0), (0, 1, 0), (0, 0, 1), plane=True)
    hip.gauge_define(1, ro, (0, side, 0), (0, 0, side))
    want = []
    for it in range(6):
        if it % 2 == 0:
            assert hip.emit_lattice(o, (r0,) * 3, (2, 2, 4), velocity=(f32(0.8), 0, 0)) == 16
        hip.step(it)
        hip.gauges_accumulate(read=False)
        if (it + 1) % 3 == 0:
            want.append(hip.gauges()[0][:2].copy())
    assert want[1][0, 0] >= 8 and want[1][1, 0] >= 4 and want[1][0, 0] > want[1][1, 0]
    for ln, (step, g) in zip(lines, ((3, 0), (3, 1), (6, 0), (6, 1))):
        t = want[step // 3 - 1][g]
        w = ln.replace("_gauge: step", "").split()
        assert [int(w[0]), int(w[2])] == [step, g]
        first = t[17] if t[18] < 0 else t[18] if t[17] < 0 else min(t[17], t[18])
        assert [float(w[k]) for k in (4, 6, 8, 10, 12, 14)] == [t[0], t[8], t[0] - t[8], t[16], first, t[19]], ln
        mean = [float(v) for v in ln.split("mean velocity plus")[1].split()[:3]]
        assert mean == [float("%.9e" % (t[1 + a] / t[0] if t[0] > 0 else 0.0)) for a in range(3)], ln
    hip.close()
    for bad in (["--gauge", "1 2 3"], ["--gauge", plane], ["--gauge-every", "2"], ["--gauge-plane", "--gauge", plane, "--gauge-every", "1"],
                ["--gauge", plane, "--gauge-every", "0"]):
        r = subprocess.run([exe, "--steps", "1"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip(), bad
