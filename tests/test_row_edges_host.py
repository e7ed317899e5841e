"""CPU proof that the scenes of tests/row_cases.py hold the states they are meant to carry to the row-walk analysis kernels
(DESIGN.md 47), on the oracle's first step and with the numpy restatements of the contracts (forces_ref, fields_ref, select_ref,
components_ref, diag_ref): pair_scene's pairs are isolated from each other and from the shell, their stored distances lie on the
claimed side of closeRf and hs at every offset, a pair beyond hs is listed in one row only, rows are empty where claimed and one
key is not a cell; block_scene has positive pressures, full rows and slots on both sides of closeRf with its nudged pair at the
threshold; coincident_scene has r == 0 in its rows, and the NaN words of the restatements are the ones named here and no others.
The restatement's words 30..35 are tied to the oracle's own acceleration at all these states. No GPU needed."""
import numpy as np
import pytest

import components_ref as cr
import diag_ref
import fields_ref as flr
import forces_ref as fr
import row_cases as R
import select_ref as sr
from band_cases import F, INF
from test_fields import make_fields

SCENE_NAMES = list(R.SCENES)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pair():
    return (R.pair_scene(),) + R.oracle_step0("pair")


@pytest.fixture(scope="module")
def coincident():
    return (R.coincident_scene(),) + R.oracle_step0("coincident")


def test_pairs_are_isolated(pair):
    sc, state, ids, dist, _ = pair
    cfg = sc["cfg"]
    h = float(cfg.h)
    n = sc["numOfLiquidP"] + sc["walls"]
    p = sc["position"][:, :3].astype(np.float64)
    cluster = np.full(n, -1)
    for c, (_, _, _, _, ip, iq) in enumerate(sc["pairs"]):
        cluster[[ip, iq]] = c
    for c, i in enumerate(sc["lone"] + [sc["stray"], sc["control"]]):
        cluster[i] = len(sc["pairs"]) + c
    assert (cluster >= 0).all()
    d = np.sqrt(((p[:n, None] - p[None, :n]) ** 2).sum(-1))
    other = cluster[:, None] != cluster[None, :]
    assert d[other].min() > R.SEPARATION_IN_H * h
    shell = np.sqrt(((p[:n, None] - p[None, n:]) ** 2).sum(-1))
    assert shell.min() > 31.0 * h / 30.0
    vel = sc["velocity"][:sc["numOfLiquidP"], :3]
    assert (np.abs(vel) > 5e-4).all() and (np.abs(vel) < 5e-3).all() and np.unique(vel, axis=0).shape[0] == vel.shape[0]
    assert len(sc["pairs"]) == 22 and sum(w for _, _, _, w, _, _ in sc["pairs"]) == sc["walls"] == 7
    assert {d for _, _, d, _, _, _ in sc["pairs"]} == {0, 1, 2}


def test_pair_scene_holds_its_thresholds(pair):
    """On the oracle's rows: no shell neighbour, no third particle, accepted for the offsets <= 0 and refused for those > 0."""
    sc, state, ids, dist, _ = pair
    counts = R.assert_pair_states(sc, state, ids, dist)
    assert counts == R.expected_pair_counts()
    for kind in ("hs", "close"):
        assert all(counts[kind, o] >= 1 for o in R.OFFSETS)
    k = R.Constants(sc["cfg"])
    # the thresholds are reached to the ulp of the stored distance somewhere: the accepted and the refused distance are neighbours
    slots = {(kd, o, d): (sp, a) for kd, o, d, w, sp, sq, a, b in R.pair_slots(sc, state, ids, dist)}
    for kind in ("hs", "close"):
        inside, outside = (dist[slots[kind, o, 0]] for o in (0, 1))
        assert inside < k.limit[kind] <= outside, (kind, inside, outside)
        # (a step of Q's coordinate is 4 steps of the stored distance at hs, 17 at closeRf)
        assert abs(int(u32([outside])[0]) - int(u32([inside])[0])) <= (4 if kind == "hs" else 17), (kind, inside, outside)


def test_pair_restatements(pair):
    sc, state, ids, dist, acc = pair
    cfg = sc["cfg"]
    k = R.Constants(cfg)
    N = cfg.particleCount
    Fo = fr.Forces(state, ids, dist, k.K)
    rec = Fo.records
    moving = np.trunc(state["types"]) != 3
    # the restatement at these states is what the oracle's K7 and K12 computed
    assert np.array_equal(u32(rec[moving, 30:33]), u32(acc[:N][moving, :3])) and np.array_equal(u32(rec[moving, 33:36]), u32(acc[N:][moving, :3]))
    assert not np.isnan(rec).any()
    for kind, off, direction, wall, sp, sq, a, b in R.pair_slots(sc, state, ids, dist):
        word = 29 if wall else 27
        if kind == "hs":
            assert rec[sp, word] == (1 if off <= 0 else 0) and rec[sp, 27:30].sum() == rec[sp, word], (off, rec[sp, 27:30])
        if kind == "close":  # pressure is 0: only the close-range term exists
            assert state["p"][sp] == 0 and state["p"][sq] == 0
            assert (rec[sp, 33:36] != 0).any() == (off <= 0), (off, rec[sp, 33:36])
        if kind in ("far", "half"):
            assert not rec[sp, 33:36].any() and rec[sp, word] == (kind == "half")
    # the measure: 1.0 with a neighbour in the row beyond h (W == 0, n > 0), 1.0 with none
    q = sr.Quantities(state, ids)
    back = R.sorted_of(state)
    far = [(sp, sq, a, b) for kind, _, _, _, sp, sq, a, b in R.pair_slots(sc, state, ids, dist) if kind == "far"]
    for sp, sq, a, b in far:
        for i, slot in ((sp, a), (sq, b)):
            assert q.m[i] == 1.0 and q.count[i] == (slot >= 0)
    assert any(q.count[sq] == 1 for _, sq, _, _ in far)
    for i in sc["lone"] + [sc["stray"], sc["control"]]:
        assert q.m[back[i]] == 1.0 and q.count[back[i]] == 0
    liquid = np.trunc(state["types"]) == 1
    assert np.unique(q.m[liquid]).size > 8 and set(q.count[liquid].tolist()) == {0.0, 1.0}


def test_the_key_that_is_not_a_cell_is_selected_by_no_mask(pair):
    """The stray's z is the first float of cell layer 9, the control's the last float of layer 8: one float decides `key < G`."""
    sc, state, ids, dist, _ = pair
    cfg = sc["cfg"]
    back = R.sorted_of(state)
    stray, control = int(back[sc["stray"]]), int(back[sc["control"]])
    z = sc["position"][[sc["control"], sc["stray"]], 2]
    assert np.nextafter(z[0], INF) == z[1]
    assert state["keys"][stray] >= cfg.gridCellCount > state["keys"][control] and stray == cfg.particleCount - 1
    for types in R.MASKS + [(2,), (3,)]:
        sel = diag_ref.selected(state, diag_ref.EVERYTHING, types)
        assert not sel[stray] and sel[control] == (1 in types)
        assert not flr.participates(state, types)[stray] and flr.participates(state, types)[control] == (1 in types)
        assert cr.label_state(state, ids, types)[0][stray] == -1
        q = sr.Quantities(state, ids)
        assert stray not in sr.select(state, q, None, types) and (control in sr.select(state, q, None, types)) == (1 in types)


def test_extreme_field_overflows_where_claimed(pair):
    sc, state, ids, dist, _ = pair
    K = flr.constants(sc["cfg"])
    back = R.sorted_of(state)
    values, roles = R.extreme_field(sc, make_fields(state, 5)[0])
    for types in R.MASKS:
        D = flr.Diffusion(state, ids, dist, K, types)
        coefficient = R.power_coefficient(D, state, roles)
        one, sigma, _ = flr.diffuse(state, ids, dist, K, values, coefficient, 1, types, D)
        four = flr.diffuse(state, ids, dist, K, values, coefficient, 4, types, D)[0]
        assert sigma > 4 and np.isfinite(sigma)
        ip, iq = roles["power"]
        assert one[ip] == -np.inf and one[iq] == np.inf  # a * S overflowed in the first substep
        ip, iq = roles["overflow"]
        assert one[ip] == -np.inf and one[iq] == np.inf  # c_j - c_i overflowed
        ip, iq = roles["overflow wall"]
        assert (one[ip] == -np.inf) == (3 in types) and (one[ip] == R.FLT_MAX) == (3 not in types)
        assert not np.isnan(one).any()
        assert np.flatnonzero(np.isnan(four)).tolist() == R.field_nan_ids(sc, state, roles, types, 4) != []
        ip, iq = roles["minus zero"]
        assert u32(values[[ip]])[0] == 0x80000000 and u32(one[[ip]])[0] == 0
        ip, iq = roles["tiny"]
        assert 0 < values[iq] < R.TINY == values[ip]
    # no participant: the stability number is +0 and nothing moves
    D = flr.Diffusion(state, ids, dist, K, (2,))
    got, sigma, _ = flr.diffuse(state, ids, dist, K, values, F(1), 4, (2,), D)
    assert u32([sigma])[0] == 0 and np.array_equal(u32(got), u32(values))


@pytest.mark.parametrize("side", ["in", "out"])
def test_block_scene_holds_its_states(side):
    sc = R.block_scene(side)
    state, ids, dist, acc = R.oracle_step0("block_" + side)
    close, middle, full = R.assert_block_states(sc, side, state, ids, dist)
    assert close > 100 and middle > 1000 and full > 0, (close, middle, full)
    k = R.Constants(sc["cfg"])
    N = sc["cfg"].particleCount
    rec = fr.Forces(state, ids, dist, k.K).records
    moving = np.trunc(state["types"]) != 3
    assert np.array_equal(u32(rec[moving, 30:36]), u32(np.concatenate([acc[:N, :3], acc[N:, :3]], 1)[moving]))
    sp, sq, a, b, want = R.block_pair(sc, state, ids, dist)
    assert state["p"][sp] > 0 and state["p"][sq] > 0
    counts = sr.neighbor_counts(ids)
    assert 32 in counts[moving] and np.isfinite(rec).all()


def test_the_two_block_scenes_differ_in_the_branch_only():
    a, b = R.block_scene("in"), R.block_scene("out")
    differ = np.argwhere(u32(a["position"]) != u32(b["position"]))
    assert differ.tolist() == [[a["pair"][1], 0]]
    assert abs(int(u32(a["position"])[a["pair"][1], 0]) - int(u32(b["position"])[a["pair"][1], 0])) == 1


def test_coincident_scene_holds_its_states(coincident):
    sc, state, ids, dist, acc = coincident
    cfg = sc["cfg"]
    k = R.Constants(cfg)
    N = cfg.particleCount
    back = R.sorted_of(state)
    names = [name for name, _ in sc["clusters"]]
    assert names.count("pair") == 2 and names.count("wall pair") == 1 and names.count("triple") == 1
    for name, members in sc["clusters"]:
        for i in members:
            row = ids[back[i]]
            others = sorted(int(back[j]) for j in members if j != i)
            assert sorted(row[row >= 0].tolist()) == others, (name, i)
            if name in ("pair", "wall pair", "triple"):
                assert not dist[back[i]][row >= 0].any()  # r == 0
    assert np.isfinite(state["pos"]).all() and np.isfinite(state["rho"]).all() and np.isfinite(state["p"]).all()
    Fo = fr.Forces(state, ids, dist, k.K)
    rec = Fo.records
    nan = R.force_nan_words(sc, state)
    assert nan.sum() == (2 * 2 + 1 + 3) * 6 and np.array_equal(np.isnan(rec), nan)
    moving = np.trunc(state["types"]) != 3
    both = np.concatenate([acc[:N, :3], acc[N:, :3]], 1)
    assert R.same_bits_or_nan(rec[moving, 30:36], both[moving]).all() and np.array_equal(np.isnan(both[:, 3:]).all(1), nan[:, 33:36].all(1))
    # the region sums that a coincident particle reaches: its pressure words, aP, the torque and the power of those classes
    d = fr.diag_records(state, rec, [diag_ref.EVERYTHING, (-9, -9, -9, -1, -1, -1)], (1, 2, 3))
    want = sorted([1 + w for w in (6, 7, 8, 24, 25, 26)] + [31, 32, 33] + [34, 35, 36, 40, 41, 42] + [43, 45])
    assert np.flatnonzero(np.isnan(d[0])).tolist() == want and not d[1].any()
    # the measure of a coincident particle is 0 (B == 0, W != 0)
    q = sr.Quantities(state, ids)
    for name, members in sc["clusters"]:
        for i in members:
            assert q.m[back[i]] == {"pair": 0.0, "wall pair": 0.0, "triple": 0.0, "lone": 1.0}.get(name, q.m[back[i]])
    # diffusion: no difference of positions enters, the stored distance 0 is the largest weight
    D = flr.Diffusion(state, ids, dist, flr.constants(cfg), (1, 2, 3))
    assert np.isfinite(D.W).all() and D.used[back[sc["clusters"][0][1][0]]].sum() == 1


def test_a_histogram_bin_that_the_clamp_decides(pair):
    """With diag_ref.histogram_of's arithmetic: a coordinate of the scene, q < hi, whose (q - lo) * scale reaches `bins`."""
    sc, state, ids, dist, _ = pair
    back = R.sorted_of(state)
    for field in (4, 5, 6):
        v = diag_ref.field_values(state, field)[back[0]]
        lo, hi, bins, q = R.clamp_case([v])
        scale = F(bins) / F(hi - lo)
        assert q == v and lo <= q < hi and F(F(q - lo) * scale) >= bins
        h = diag_ref.histogram_of(np.array([q], F), lo, hi, bins)
        assert h[bins] == 1 and h.sum() == 1  # the last bin, not the overflow slot


def test_scenes_hold_the_counts_and_measures_they_claim(pair, coincident):
    for name, want_counts, want_m in (("pair", {0.0, 1.0}, {1.0}), ("coincident", {0.0, 1.0, 2.0}, {0.0, 1.0}), ("block_in", {32.0}, set())):
        state, ids, dist, _ = R.oracle_step0(name)
        q = sr.Quantities(state, ids)
        liquid = np.trunc(state["types"]) == 1
        assert set(q.count[liquid].tolist()) >= want_counts and set(q.m[liquid].tolist()) >= want_m, name
    sc, state, ids, dist, _ = pair  # every lone particle holds the clamp density exactly
    assert np.unique(u32(state["rho"][R.sorted_of(state)[sc["lone"]]])).size == 1


def test_a_pair_that_one_row_lists_is_one_component(pair):
    """The contract counts either end's row: labelled, under every mask that holds the liquid, with the same label."""
    sc, state, ids, dist, _ = pair
    g = cr.graph(ids, state["pos"])
    one_sided = [(sp, sq, w) for kd, o, d, w, sp, sq, a, b in R.pair_slots(sc, state, ids, dist) if kd == "far" and (a >= 0) != (b >= 0)]
    assert len(one_sided) == 2 and sorted(w for _, _, w in one_sided) == [False, True]
    for sp, sq, wall in one_sided:
        for types in R.MASKS:
            labels = cr.label_state(state, ids, types, np.inf, g)[0]
            assert labels[sp] >= 0 and (labels[sq] >= 0) == (not wall or 3 in types), (types, wall)
            if labels[sq] >= 0:
                assert labels[sp] == labels[sq]
            else:  # the wall end is not selected: the liquid end is a component of one
                assert (labels == labels[sp]).sum() == 1
