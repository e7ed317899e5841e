"""The flow-gauge contract without a GPU (include/sphmi.h, sph_gauge_define / sph_gauges_accumulate / sph_gauge_crossings): the numpy
restatement (tests/gauge_ref.py) against literal numbers on hand-made segments, the dual basis, the exact conservation of the
particle count behind a plane over steps of the C oracle, rectangles that tile, the tree, and the Python helpers and binding. The
GPU tests (tests/test_gauge.py) compare the library with this restatement word for word, on the same cases."""
import ctypes
import types as _types

import numpy as np
import pytest

import diag_ref
import gauge_cases as gc
import gauge_ref as gr
import scenes
import sphmi
from sphmi import frames

f32, f64 = np.float32, np.float64
NAMES = list(gc.CASES)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- hand-made segments
RECT = dict(origin=(0, 0, 0), u=(0, 2, 0), v=(0, 0, 4))  # n = (8, 0, 0), nn = 64, A = (0, 1/2, 0), B = (0, 0, 1/4)
nan = np.nan
# a (x, y, z, type) -> b (x, y, z), velocity after the step
SEGMENTS = [
    ((-1, 1, 1, 1.1), (1, 1, 3), (1.0, 0.5, -0.25)),    # 0 through the middle: positive, t 1/2, alpha 1/2, beta 1/2
    ((0, 1, 1, 1.1), (-1, 1, 1), (2.0, 0.5, -0.25)),    # 1 starts ON the plane: the non-negative side, so a negative crossing, t 0
    ((-1, 1, 1, 1.1), (0, 1, 1), (4.0, 0.5, -0.25)),    # 2 ends exactly on it: positive, t 1
    ((-1, 1, 1, 1.1), (-1, 1.5, 2), (8.0, 0.5, -0.25)),  # 3 parallel, in front
    ((0, 1, 1, 1.1), (0, 1.5, 1), (16.0, 0.5, -0.25)),  # 4 parallel, in the plane
    ((-1, 0, 1, 1.1), (1, 0, 1), (32.0, 0.5, -0.25)),   # 5 alpha exactly 0: inside
    ((-1, 2, 1, 1.1), (1, 2, 1), (64.0, 0.5, -0.25)),   # 6 alpha exactly 1: outside the rectangle, counted by the plane
    ((nan, 1, 1, 1.1), (1, 1, 1), (128.0, 0.5, -0.25)),  # 7 a NaN at the start
    ((-1, 1, 1, 1.1), (1, nan, 1), (256.0, 0.5, -0.25)),  # 8 a NaN at the end (not in the normal's axis: s(b) is NaN all the same)
    ((-1, 1, 1, 3.0), (1, 1, 1), (512.0, 0.5, -0.25)),  # 9 a boundary particle
    ((1, 1, 2, 2.1), (-1, 1, 2), (1024.0, 0.5, -0.25)),  # 10 an elastic particle, the other way: counted only with type 2 in the mask
]


def hand_state(order=None):
    n = len(SEGMENTS)
    order = np.arange(n) if order is None else np.asarray(order)
    a = np.array([s[0] for s in SEGMENTS], np.float32)
    pos = np.array([tuple(s[1]) + (s[0][3],) for s in SEGMENTS], np.float32)
    vel = np.array([tuple(s[2]) + (0.0,) for s in SEGMENTS], np.float32)
    return dict(a=a[order], orig=order.astype(np.int64), pos=pos, vel=vel, fields={0: np.arange(n, dtype=np.float32) * f32(0.5)})


def test_derived_values_of_the_hand_made_gauge():
    D = gr.derive(RECT)
    assert D["n"].tolist() == [8.0, 0.0, 0.0] and D["nn"] == 64.0
    assert D["A"].tolist() == [0.0, 0.5, 0.0] and D["B"].tolist() == [0.0, 0.0, 0.25]


@pytest.mark.parametrize("order", [None, [10, 3, 0, 7, 1, 9, 2, 8, 5, 4, 6]])
def test_hand_made_segments_against_literal_numbers(order):
    st = hand_state(order)
    where = np.argsort(st["orig"])  # sorted index of segment k
    C = gr.Crossings(st, dict(RECT, types=(1,)))
    assert C.direction[where].tolist() == [1, -1, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert C.crossed[where].tolist() == [True, True, True, False, False, True, True, False, False, False, False]
    k = where[[0, 1, 2, 5, 6]]
    assert C.t[k].tolist() == [0.5, 0.0, 1.0, 0.5, 0.5]
    assert C.alpha[k].tolist() == [0.5, 0.5, 0.5, 0.0, 1.0] and C.beta[k].tolist() == [0.5, 0.25, 0.25, 0.25, 0.25]
    rec = gr.record(st, dict(RECT, types=(1,), field=0))
    #           n    vx    vy    vz     v2 = (vx*vx + 0.25) + 0.0625                 field (k/2)       alpha  beta
    assert rec[:8].tolist() == [3.0, 37.0, 1.5, -0.75, (1 + 16 + 1024) + 3 * 0.3125, 0.0 + 1.0 + 2.5, 1.0, 1.0]
    assert rec[8:].tolist() == [1.0, 2.0, 0.5, -0.25, 4.3125, 0.5, 0.5, 0.25]
    # the whole plane counts alpha == 1 too; type 2 in the mask adds the elastic particle, never the boundary particle
    rec = gr.record(st, dict(RECT, types=(1, 2), plane=True))
    assert rec[0] == 4.0 and rec[1] == 101.0 and rec[6] == 2.0 and rec[8] == 2.0 and rec[9] == 1026.0 and rec[13] == 0.0
    idx, ids, way, tab = gr.crossing_list(st, dict(RECT, types=(1, 2)))
    assert np.array_equal(idx, np.sort(where[[0, 1, 2, 5, 10]])) and np.array_equal(ids, st["orig"][idx])
    assert way[np.argsort(ids)].tolist() == [1, -1, 1, 1, -1] and tab.dtype == np.float32 and tab.shape == (5, 3)
    assert tab[np.argsort(ids)].tolist() == [[0.5, 0.5, 0.5], [0.0, 0.5, 0.25], [1.0, 0.5, 0.25], [0.5, 0.0, 0.25], [0.5, 0.5, 0.5]]
    # turned round (u and v swapped): positive and negative trade places, except ON the plane, which stays the non-negative side
    C = gr.Crossings(st, dict(origin=RECT["origin"], u=RECT["v"], v=RECT["u"], types=(1,)))
    assert C.direction[where].tolist() == [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0]  # 1: s(a) = -0.0 >= 0 and s(b) > 0; 2: s(b) = 0 is not < 0


def test_definitions_the_library_refuses():
    ok = dict(RECT, types=(1,))
    assert gr.valid(ok) and gr.valid(dict(ok, types=(1, 2))) and gr.valid(dict(ok, field=2), live_fields=(2,))
    assert not gr.valid(dict(ok, u=(0, 0, 8)))        # u parallel to v: nn == 0
    assert not gr.valid(dict(ok, u=(0, 0, 0)))
    assert not gr.valid(dict(ok, origin=(0, np.inf, 0))) and not gr.valid(dict(ok, v=(0, nan, 4)))
    assert gr.valid(dict(ok, u=(0, 3e38, 0), v=(0, 0, 3e38)))  # (finite floats cannot overflow nn in double)
    assert not gr.valid(dict(ok, types=())) and not gr.valid(dict(ok, types=(3,))) and not gr.valid(dict(ok, types=(0, 1)))
    assert not gr.valid(dict(ok, field=1)) and not gr.valid(dict(ok, field=1), live_fields=(0,))


# ---------------------------------------------------------------------------------------------- on the oracle
@pytest.mark.parametrize("name", NAMES)
def test_no_comparison_passes_on_empty_sums(name):
    """What the issue asks of every case: at least 8 crossings in each direction of each gauge, for a parallelogram at least 8
    counted and at least 8 rejected by the (alpha, beta) test; with elastic matter, crossings of type 2."""
    c = gc.case(name)
    k = gc.counts(c)
    print(name, k)
    assert set(k) == set(range(16))
    for slot, (plus, minus, counted, rejected, elastic) in k.items():
        assert plus >= 8 and minus >= 8, (slot, plus, minus)
        if c["gauges"][slot].get("plane"):
            assert rejected == 0
        else:
            assert counted >= 8 and rejected >= 8, (slot, counted, rejected)
    if name == "elastic":
        assert k[1][4] >= 1 and sum(v[4] for v in k.values()) >= 8
    for st in c["states"]:
        assert np.isfinite(st["pos"]).all() and np.isfinite(st["vel"]).all()
    # every record word of some step is non-zero for every gauge: counts, velocity sums, alpha and beta
    total = np.abs(np.sum(c["records"], axis=0))
    assert (total[:, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 15]] > 0).all() and not total[:, [5, 13]].any()
    u, v = (np.asarray(c["gauges"][7][x], f64) for x in "uv")
    assert (np.abs(u) > 0).all() and (np.abs(v) > 0).all() and abs(float(u @ v)) > 0.1 * np.sqrt((u @ u) * (v @ v))  # tilted, not orthogonal


@pytest.mark.parametrize("name", NAMES)
def test_the_sorted_position_is_where_the_particle_was(name):
    c = gc.case(name)
    before = c["pos0"]
    for st in c["states"]:
        assert scenes.bits_equal(st["a"], before[st["orig"]])
        before = st["pos"]


@pytest.mark.parametrize("name", NAMES)
def test_dual_basis(name):
    c = gc.case(name)
    eps = np.finfo(f64).eps
    for slot, g in c["gauges"].items():
        D = gr.derive(g)
        u, v = np.asarray(g["u"], f64), np.asarray(g["v"], f64)
        scale = lambda p, q: 8 * eps * np.sqrt((p @ p) * (q @ q))
        assert abs(D["A"] @ u - 1) <= 8 * eps and abs(D["B"] @ v - 1) <= 8 * eps, slot
        assert abs(D["A"] @ v) <= scale(D["A"], v) and abs(D["B"] @ u) <= scale(D["B"], u), slot
        assert abs(D["A"] @ D["n"]) <= scale(D["A"], D["n"]) and abs(D["B"] @ D["n"]) <= scale(D["B"], D["n"])


@pytest.mark.parametrize("name", NAMES)
def test_conservation_is_exact(name):
    """Net crossings of a plane over the steps == the change of the number of considered particles with s >= 0. An integer
    identity: it would not survive a crossing rule that is not half-open, or a particle counted on both sides."""
    c = gc.case(name)
    planes = [s for s, g in c["gauges"].items() if g.get("plane")]
    assert {0, 1, 2}.issubset(planes) and len(planes) >= 8  # an x, a y and a z plane among them, and tilted ones
    for slot in planes:
        g = c["gauges"][slot]
        net = sum(int(r[slot, 0]) - int(r[slot, 8]) for r in c["records"])
        before, after = gr.side_count(c["pos0"], g, c["types"]), gr.side_count(c["states"][-1]["pos"], g, c["types"])
        assert net == after - before, (slot, net, before, after)
        # and step by step
        prev = c["pos0"]
        for st, r in zip(c["states"], c["records"]):
            assert int(r[slot, 0]) - int(r[slot, 8]) == gr.side_count(st["pos"], g, c["types"]) - gr.side_count(prev, g, c["types"])
            prev = st["pos"]
    g0 = c["gauges"][0]
    x0 = float(g0["origin"][0])
    liquid = np.isin(c["pos0"][:, 3].astype(np.int32), c["types"])
    assert gr.side_count(c["pos0"], g0, c["types"]) == int((liquid & (c["pos0"][:, 0] >= f32(x0))).sum())  # s >= 0 is x >= c


@pytest.mark.parametrize("name", NAMES)
def test_rectangles_that_tile_add_up(name):
    c = gc.case(name)
    seen = 0
    for r in c["records"]:
        for w in (0, 8):
            assert r[5, w] + r[6, w] == r[4, w]
            seen += int(r[5, w] > 0) + int(r[6, w] > 0)
    assert seen >= 4
    # the plane they lie in counts every crossing they count, and more
    for st in c["states"]:
        d = [gr.Crossings(st, c["gauges"][s]).direction for s in (0, 4, 5, 6)]
        assert np.array_equal(d[1], d[2] + d[3]) and not (d[2] * d[3]).any()
        assert np.array_equal(d[1][d[1] != 0], d[0][d[1] != 0])


@pytest.mark.parametrize("name", NAMES)
def test_a_gauge_turned_round_trades_the_directions(name):
    c = gc.case(name)
    for r in c["records"]:
        assert np.array_equal(u64(r[3, 0:6]), u64(r[0, 8:14])) and np.array_equal(u64(r[3, 8:14]), u64(r[0, 0:6]))
        assert u64(r[3, 6]) == u64(r[0, 15]) and u64(r[3, 7]) == u64(r[0, 14])  # alpha and beta trade places with u and v


def test_tree_properties():
    c = gc.case("tiny_jitter")
    st, g = c["states"][2], c["gauges"][8]
    C = gr.Crossings(st, g)
    t = gr.terms(st, g, C)
    rec = gr.record(st, g, C)
    assert rec[0] == (C.direction == 1).sum() > 8 and rec[8] == (C.direction == -1).sum() > 8
    for w in (1, 4, 6, 9, 15):
        assert u64(rec[w]) == u64(diag_ref.tree_sum(t[w])) and rec[w] != 0
        assert abs(rec[w] - t[w].sum()) <= 1e-12 * np.abs(t[w]).sum()
    # more than one chunk: the state three times over is three chunks, and the tree adds their results
    big = dict(a=np.concatenate([st["a"]] * 3), orig=np.concatenate([st["orig"]] * 3), pos=st["pos"], vel=st["vel"], fields={})
    assert big["a"].shape[0] > 2 * 1024
    rb = gr.record(big, g)
    assert rb[0] == 3 * rec[0] and abs(rb[1] - 3 * rec[1]) <= 1e-12 * abs(rec[1])
    # totals: added once per call, the call words
    tot = gr.empty_totals()
    assert (tot[:, :17] == 0).all() and (tot[:, 17:] == -1).all()
    recs = c["records"]
    for call, r in enumerate(recs):
        tot = gr.accumulate(tot, r, range(16), call)
    assert tot[0, 16] == len(recs) and tot[0, 0] == sum(r[0, 0] for r in recs)
    assert tot[0, 17] == 0 and tot[0, 18] == 2 and tot[0, 19] == len(recs) - 1  # the first step moves everything one way


# ---------------------------------------------------------------------------------------------- helpers and binding
def test_definition_helpers():
    r = frames.gauge_rect((1, 2, 3), (2, 0, 0), 2.0, 4.0)
    assert set(r) == {"origin", "u", "v"} and all(r[k].dtype == np.float32 for k in r)
    assert np.cross(r["u"], r["v"]).tolist() == [8.0, 0.0, 0.0] and (r["origin"] + 0.5 * r["u"] + 0.5 * r["v"]).tolist() == [1.0, 2.0, 3.0]
    assert np.sqrt((r["u"] ** 2).sum()) == 2.0 and np.sqrt((r["v"] ** 2).sum()) == 4.0 and r["v"].tolist() == [0.0, 4.0, 0.0]
    t = frames.gauge_rect((0, 0, 0), (1, 1, 0), 1.0, 1.0, up=(0, 0, 1))
    n = np.cross(t["u"], t["v"])
    assert abs(n[0] - n[1]) < 1e-6 and n[0] > 0 and abs(n[2]) < 1e-6 and gr.valid(dict(t, types=(1,)))
    p = frames.gauge_plane((1, 2, 3), (0, 0, -5))
    assert p["plane"] is True and np.cross(p["u"], p["v"]).tolist() == [0.0, 0.0, -1.0] and p["origin"].tolist() == [1.0, 2.0, 3.0]
    for bad in (lambda: frames.gauge_rect((0, 0, 0), (0, 0, 0), 1, 1), lambda: frames.gauge_rect((0, 0, 0), (0, 1, 0), 1, 1),
                lambda: frames.gauge_rect((0, 0, 0), (1, 0, 0), 0, 1), lambda: frames.gauge_plane((0, 0, 0), (0, 0, 0))):
        with pytest.raises(ValueError):
            bad()


def test_gauge_summary():
    c = gc.case("tiny")
    cfg = c["cfg"]
    rec = c["records"][3][0]
    s = frames.gauge_summary(rec, cfg)
    assert s["plus"] == rec[0] and s["minus"] == rec[8] and s["net"] == rec[0] - rec[8] and s["gross"] == rec[0] + rec[8]
    vol = float(cfg.mass) / float(cfg.rho0)
    assert s["volume_rate"] == (rec[0] - rec[8]) * vol / float(cfg.timeStep)
    assert np.array_equal(s["mean_velocity_plus"], rec[1:4] / rec[0]) and s["mean_velocity_plus"][0] > 0 > s["mean_velocity_minus"][0]
    assert s["mean_v2_minus"] == rec[12] / rec[8] and np.array_equal(s["centroid_plus"], rec[6:8] / rec[0]) and s["field_flux"] == 0
    tot = gr.empty_totals()
    for call, r in enumerate(c["records"]):
        tot = gr.accumulate(tot, r, range(16), call)
    st = frames.gauge_summary(tot[0], cfg)
    assert st["net"] == tot[0, 0] - tot[0, 8] and st["volume_rate"] == st["net"] * vol / (len(c["records"]) * float(cfg.timeStep))
    assert frames.gauge_summary(tot[0], cfg, calls=2)["volume_rate"] == st["net"] * vol / (2 * float(cfg.timeStep))
    empty = frames.gauge_summary(np.zeros(16), cfg)
    assert empty["net"] == 0 and np.isnan(empty["mean_velocity_plus"]).all()
    with pytest.raises(ValueError):
        frames.gauge_summary(np.zeros(17), cfg)
    assert len(frames.GAUGE_FIELDS) == sphmi.GAUGE_WORDS == gr.WORDS and len(frames.GAUGE_TOTAL_FIELDS) == sphmi.GAUGE_TOTAL_WORDS == gr.TOTAL_WORDS
    assert len(set(frames.GAUGE_TOTAL_FIELDS)) == 20 and frames.GAUGE_FIELDS[0] == "plus_n" and frames.GAUGE_FIELDS[13] == "minus_sum_field"
    assert frames.GAUGE_TOTAL_FIELDS[16:] == ("calls", "first_plus_call", "first_minus_call", "last_call")


def test_binding_lists_the_gauge_calls_and_checks_its_arguments():
    lib = ctypes.CDLL(sphmi.LIB_PATH)
    txt = open(scenes.ROOT + "/include/sphmi.h").read()
    names = ("sph_gauge_define", "sph_gauge_get", "sph_gauges_accumulate", "sph_gauges_read", "sph_gauges_reset", "sph_gauges_history",
             "sph_gauges_read_history", "sph_gauge_crossings", "sph_read_gauge_crossings")
    for n in names:
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for m in ("gauge_define", "gauge", "gauges_accumulate", "gauges", "gauges_reset", "gauges_history", "gauge_history", "gauge_crossings"):
        assert callable(getattr(sphmi.owHIPSolver, m))
    for name, value in (("SPH_MAX_GAUGES", sphmi.MAX_GAUGES), ("SPH_GAUGE_WORDS", sphmi.GAUGE_WORDS), ("SPH_GAUGE_TOTAL_WORDS", sphmi.GAUGE_TOTAL_WORDS),
                        ("SPH_GAUGE_HISTORY_MAX", sphmi.GAUGE_HISTORY_MAX)):
        assert "#define %s %d\n" % (name, value) in txt
    assert "#define SPH_GAUGE_PLANE %du" % sphmi.GAUGE_PLANE in txt and "#define SPHMI_ABI_VERSION 2" in txt
    assert ctypes.sizeof(sphmi.SphGauge) == 48 and sphmi.SphGauge.typeMask.offset == 36 and sphmi.SphGauge.flags.offset == 44
    # the wrapper refuses what it cannot pass on, before it reaches the library
    fake = _types.SimpleNamespace()
    for kw in (dict(origin=(0, 0), u=(0, 1, 0), v=(0, 0, 1)), dict(origin=(0, 0, 0), u=(0, 1, 0, 0), v=(0, 0, 1)),
               dict(origin=(0, 0, 0), u=(0, 1, 0), v=None)):
        with pytest.raises((sphmi.SphError, TypeError, ValueError)):
            sphmi.owHIPSolver.gauge_define(fake, 0, **kw)
