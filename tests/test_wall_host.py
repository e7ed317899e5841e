"""CPU tests of the wall-load contract's numpy restatement (tests/wall_ref.py): one hand-made neighbourhood against literal
numbers, the tie to the C oracle's integrate stage on scenes whose floor is lifted into the liquid (the committed scenes never
touch a wall in integrate's sense), the split of a contact between two bodies, the tie to the force decomposition, the totals'
tree and frames.wall_summary. Floats are compared as bit patterns; the one bound (the shares' sum) is derived where it stands."""
import ctypes
import functools

import numpy as np
import pytest

import diag_ref
import forces_ref as fr
import scenes
import sphmi
import wall_cases
import wall_ref as wr
from sphmi import frames

f32 = np.float32


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- one neighbourhood by hand
def _hand():
    """Nine particles in sorted order; original id = 8 - sorted index. dt = posTimeStep = r0 = 1, the box is [0, 100]^3.
    0 liquid: walls 2 (body A, d = 0.5) and 3 (body B, d = 0.625) in reach, wall 4 (body A) at d = 2, a liquid neighbour; moving down
    1 liquid: wall 5 (no body, d = 0.5 from x0 = (20, 1.5, 20)), moving up: contact without reflection
    2..5 boundary     6 liquid, empty row, velocity.w = 0.5     7 liquid, leaves the box in x     8 elastic, no wall in its row"""
    pos = np.array([[10, 1, 10], [20, 1, 20], [10, 0, 10], [10.625, 0.5, 10], [10, 0.5, 12], [20.5, 1.5, 20], [30, 30, 30], [99.5, 50, 50],
                    [40, 40, 40]], f32)
    types = np.array([1.1, 1.1, 3.1, 3.1, 3.1, 3.1, 1.1, 1.1, 2.1], f32)
    vel4 = np.array([[0, -0.5, 0, 0], [0, 0.5, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0.5], [2, 0, 0, 0],
                     [0, 0, 0, 0]], f32)
    N = pos.shape[0]
    ids = -np.ones((N, 32), np.int32)
    ids[0, [0, 1, 3, 4]] = [2, 3, 4, 1]  # slot 2 is empty
    ids[1, 5] = 5
    ids[8, 0] = 6
    dist = np.full((N, 32), 99.0, f32)  # stored distances beyond hs: K7 uses no slot
    state = dict(pos=pos, vel=vel4[:, :3].copy(), vel4=vel4, acc=np.zeros((2 * N, 4), f32), types=types, rho=np.full(N, 1000.0, f32),
                 rhoStar=np.full(N, 1000.0, f32), p=np.ones(N, f32), keys=np.zeros(N, np.uint32), G=1, orig=8 - np.arange(N))
    W = dict(dt=f32(1), posTimeStep=f32(1), r0=f32(1), lo=np.zeros(3, f32), hi=np.full(3, 100.0, f32), fold=True)
    bodies = {0: [8 - 2, 8 - 4], 5: [8 - 3]}  # A = sorted 2 and 4, B = sorted 3, by original id
    return state, ids, dist, W, bodies


def _hand_wall(slot):
    state, ids, dist, W, bodies = _hand()
    K = fr.constants(sphmi.default_config())
    return wr.Wall(state, ids, dist, K, W, wr.wall_set(state, slot, bodies)), state


def test_neighbourhood_by_hand():
    A, state = _hand_wall(0)
    B, _ = _hand_wall(5)
    ALL, _ = _hand_wall(wr.ALL)
    NONE, _ = _hand_wall(wr.NO_BODY)
    r = ALL.records
    # particle 0: n = 0.5 (0, 1, 0) + 0.375 (-1, 0, 0), |n| = 0.625, wsum = 0.875, wsum2 = 0.25 + 0.140625
    n, ln, wsum, wsum2 = (f32(-0.375), f32(0.5), f32(0)), f32(0.625), f32(0.875), f32(0.390625)
    sh = [f32(f32(f32(c / ln) * wsum2) / wsum) for c in n]
    assert u32(r[0, 0:3]).tolist() == u32(sh).tolist()
    assert np.allclose(r[0, 0:3], [-0.267857, 0.357143, 0.0], rtol=1e-6, atol=0)
    # x0 = (10, 0.5, 10); vn = 0.5 * -0.5 = -0.25 < 0: reflected
    u1 = [f32(f32(f32(0) - f32(n[0] * f32(-0.25))) * f32(0.99)), f32(f32(f32(-0.5) - f32(n[1] * f32(-0.25))) * f32(0.99)), f32(0)]
    assert u32(r[0, 22:25]).tolist() == u32(u1).tolist() and np.allclose(r[0, 22:25], [-0.0928125, -0.37125, 0.0], rtol=1e-6)
    assert u32(r[0, 3:6]).tolist() == u32([u1[0] - f32(0), u1[1] - f32(-0.5), f32(0)]).tolist()
    assert np.allclose(r[0, 3:6], [-0.0928125, 0.12875, 0.0], rtol=1e-6)
    assert u32(r[0, 19:22]).tolist() == u32([f32(10) + sh[0], f32(0.5) + sh[1], f32(10)]).tolist()
    assert r[0, 6:10].tolist() == [1.0, 0.875, 2.0, 3.0] and r[0, 26:28].tolist() == [1.0, 1.0] and not r[0, 28:].any()
    # the two bodies: A holds the slots of walls 2 (w 0.5) and 4 (beyond r0: w 0), B that of wall 3 (w 0.375)
    assert A.records[0, 6:10].tolist() == [float(f32(0.5) / f32(0.875)), 0.5, 1.0, 2.0]
    assert B.records[0, 6:10].tolist() == [float(f32(0.375) / f32(0.875)), 0.375, 1.0, 1.0]
    assert np.allclose([A.records[0, 6], B.records[0, 6]], [0.571428571, 0.428571429], rtol=1e-7)
    for X in (A, B):
        assert u32(X.records[0, 0:6]).tolist() == u32(np.concatenate([r[0, 0:3] * X.records[0, 6], r[0, 3:6] * X.records[0, 6]])).tolist()
        assert u32(X.records[:, 19:28]).tolist() == u32(r[:, 19:28]).tolist()  # the step's own words do not depend on the set
    assert not NONE.records[0, 0:19].any() and NONE.records[0, 26:28].tolist() == [1.0, 1.0]
    # particle 1: contact (d = 0.5, w = 0.5, sh = (0, 1, 0) * 0.25 / 0.5), vn = 0.5 * 0.5 > 0: not reflected; its wall is in no body
    assert r[1, 0:10].tolist() == [0, 0.5, 0, 0, 0, 0, 1.0, 0.5, 1.0, 1.0] and r[1, 19:28].tolist() == [20, 2, 20, 0, 0.5, 0, 0, 1.0, 0.0]
    assert u32(NONE.records[1]).tolist() == u32(r[1]).tolist() and not A.records[1, 0:19].any() and not B.records[1, 0:19].any()
    # boundary particles: all zero. The empty row: free flight, every lane of the velocity. The box clamp. An elastic particle.
    assert not r[2:6].any()
    assert r[6].tolist() == [0] * 19 + [31, 30, 30, 1, 0, 0, 0.5] + [0] * 6
    assert u32(r[7, 19]) == u32(f32(100) - f32(0.000001)) and r[7, 22] == 2.0 and r[7, 26] == 0
    assert r[8, 19:22].tolist() == [40, 40, 40] and not r[8, 0:19].any()
    assert ALL.contact.tolist() == [True, True] + [False] * 7 and ALL.reflected.tolist() == [True] + [False] * 8
    # K7 uses nothing (stored distances beyond hs); K12 is class 3 of the decomposition, and splits between the sets slot by slot
    F = fr.Forces(state, _hand()[1], _hand()[2], fr.constants(sphmi.default_config()))
    assert u32(r[:, 10:19]).tolist() == u32(F.records[:, 18:27]).tolist() and np.abs(r[0, 16:19]).max() > 0 and not r[:, 10:16].any()
    assert np.abs(A.records[0, 16:19]).max() > 0 and np.abs(B.records[0, 16:19]).max() > 0
    assert not np.array_equal(u32(A.records[0, 16:19]), u32(B.records[0, 16:19]))
    # the totals: counts and sums of the two contacts
    t = wr.diag_records(state, r, [diag_ref.EVERYTHING, (0, 0, 0, 15, 100, 100)], (1, 2))
    assert t[:, 0:4].tolist() == [[5, 2, 2, 1], [1, 1, 1, 1]] and t[0, 25] == 2 and t[0, 26] == 1.375 and not t[:, 27:].any()
    assert t[0, 5] == float(r[0, 1]) + float(r[1, 1])
    x, dv = state["pos"][0], r[0, 3:6]
    assert u64(t[1, 19:22]).tolist() == u64([f32(x[1] * dv[2]) - f32(x[2] * dv[1]), f32(x[2] * dv[0]) - f32(x[0] * dv[2]),
                                            f32(x[0] * dv[1]) - f32(x[1] * dv[0])]).tolist()
    ta = wr.diag_records(state, A.records, [diag_ref.EVERYTHING], (1, 2))
    assert ta[0, 0:4].tolist() == [5, 2, 1, 1]


# ---------------------------------------------------------------------------------------------- the tie to the oracle
@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle driven stage by stage through the step that follows the lift (tiny_elastic: through its 21st step): the state
    just before integrate, position and velocity right after it and after the whole step."""
    if name == "tiny_elastic":
        sc = scenes.SCENES[name]()
        cfg, A, B = sc["cfg"], None, None
        ora = scenes.oracle_for(sc)
        for _ in range(20):
            ora.step()
    else:
        case = wall_cases.lifted(name)
        sc, cfg, A, B = wall_cases.moved_scene(case), case["cfg"], case["A"], case["B"]
        ora = scenes.oracle_for(sc)
    N = cfg.particleCount
    seq = scenes.STAGE_SEQUENCE
    k = seq.index("integrate")
    for st in seq[:k]:
        ora.run(st)
    state, ids, dist = wr.oracle_state(ora, N, cfg.gridCellCount)
    ora.run("integrate")
    pos_i = ora.buffer("position").reshape(-1, 4)[:N].copy()
    vel_i = ora.buffer("velocity").reshape(-1, 4)[:N].copy()
    for st in seq[k + 1:]:
        ora.run(st)
    pos_f = ora.buffer("position").reshape(-1, 4)[:N].copy()
    vel_f = ora.buffer("velocity").reshape(-1, 4)[:N].copy()
    ora.close()
    K, W = fr.constants(cfg), wr.constants(cfg)
    bodies = {} if A is None else {wall_cases.SLOT_A: A, wall_cases.SLOT_B: B}
    walls = {s: wr.Wall(state, ids, dist, K, W, wr.wall_set(state, s, bodies)) for s in [wr.ALL, wr.NO_BODY] + sorted(bodies)}
    return dict(cfg=cfg, N=N, state=state, ids=ids, dist=dist, K=K, W=W, walls=walls, pos_i=pos_i, vel_i=vel_i, pos_f=pos_f,
                vel_f=vel_f, A=A, B=B)


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter", "tiny_elastic"])
def test_words_19_to_25_are_the_oracles_integrate(name):
    c = oracle_case(name)
    w = c["walls"][wr.ALL]
    moving, orig = w.moving, c["state"]["orig"]
    rec = w.records
    n_contact, n_reflected = int(w.contact.sum()), int(w.reflected.sum())
    print("%s: %d particles in contact, %d reflected" % (name, n_contact, n_reflected))
    if name == "tiny_elastic":
        assert n_contact == 0 and (np.trunc(c["state"]["types"]) == 2).any()  # the no-contact path beside elastic matter
        x_i = rec[:, 19:22]
    else:
        assert n_contact >= 1 and n_reflected >= 1
        # without elastic matter the record carries integrate's `+ 0.f` fold, which the reference applies in the membrane stages
        assert scenes.bits_equal(rec[moving, 19:22], c["pos_f"][orig[moving], :3])
        assert scenes.bits_equal(rec[moving, 22:26], c["vel_f"][orig[moving]])
        x_i = wr.Wall(c["state"], c["ids"], c["dist"], c["K"], dict(c["W"], fold=False), np.zeros(c["N"], bool)).records[:, 19:22]
    assert scenes.bits_equal(x_i[moving], c["pos_i"][orig[moving], :3]), scenes.diff_report(x_i[moving], c["pos_i"][orig[moving], :3])
    assert scenes.bits_equal(rec[moving, 22:26], c["vel_i"][orig[moving]])
    assert not rec[~moving].any()
    # the contact changed something: shift and velocity change are not zero where the flags say so
    assert (np.abs(rec[w.contact, 0:3]).max(1) > 0).all() and (np.abs(rec[w.reflected, 3:6]).max(1) > 0).all()
    assert not rec[~w.contact, 0:7].any()


@pytest.mark.parametrize("name,members", [("tiny", 128), ("tiny_jitter", 160)])
def test_a_floor_split_into_two_bodies(name, members):
    c = oracle_case(name)
    assert c["A"].size == members and c["B"].size == members
    wa, wb, wn, w = (c["walls"][s] for s in (wall_cases.SLOT_A, wall_cases.SLOT_B, wr.NO_BODY, wr.ALL))
    ra, rb, rn, r = wa.records, wb.records, wn.records, w.records
    contact = w.contact
    only = {k: contact & (x.records[:, 8] == w.touching) & (w.touching > 0) for k, x in (("A", wa), ("B", wb), ("none", wn))}
    one_set = only["A"] | only["B"] | only["none"]
    both = contact & (ra[:, 8] > 0) & (rb[:, 8] > 0)
    print("%s: %d particles touch one set only, %d touch both bodies" % (name, one_set.sum(), both.sum()))
    assert both.sum() > 0 and one_set.sum() > 0 and not (one_set & both).any()
    # one set only: the weights of the other sets are sums of +0, so wS has wsum's bits and the share is exactly 1
    for k, x in (("A", wa), ("B", wb), ("none", wn)):
        m = only[k]
        assert scenes.bits_equal(x.wS[m], w.wsum[m]) and (x.records[m, 6] == 1).all()
        assert scenes.bits_equal(x.records[m, 0:6], r[m, 0:6])
    # elsewhere: wA, wB, wNone and wsum are sequential float sums of at most 32 non-negative terms, each within 31 * 2^-24
    # relative of its exact value, and the three-term sum adds two more roundings: well inside 2^-18 * wsum
    total = (ra[:, 7].astype(np.float64) + rb[:, 7]) + rn[:, 7]
    err = np.abs(total - w.wsum.astype(np.float64))
    print("%s: largest |wA + wB + wNone - wsum| / wsum = %.3g" % (name, (err[contact] / w.wsum[contact]).max()))
    assert (err[contact] <= 2.0 ** -18 * w.wsum[contact]).all() and (total[~contact] == 0).all()
    # slots and touching slots partition exactly; the step's own words do not depend on the set
    assert np.array_equal(ra[:, 9] + rb[:, 9] + rn[:, 9], r[:, 9]) and np.array_equal(ra[:, 8] + rb[:, 8] + rn[:, 8], r[:, 8])
    assert np.array_equal(r[:, 8], w.touching.astype(np.float32))
    for x in (ra, rb, rn):
        assert scenes.bits_equal(x[:, 19:28], r[:, 19:28])
    # both bodies push up: the summed velocity change attributed to each is upwards
    assert ra[:, 4].sum() > 0 and rb[:, 4].sum() > 0


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter", "tiny_elastic"])
def test_all_walls_are_class_3_of_the_force_decomposition(name):
    c = oracle_case(name)
    r = c["walls"][wr.ALL].records
    F = fr.Forces(c["state"], c["ids"], c["dist"], c["K"])
    assert scenes.bits_equal(r[:, 10:19], F.records[:, 18:27]) and np.abs(r[:, 10:19]).max() > 0
    assert np.array_equal(r[:, 9] >= F.records[:, 29], np.ones(c["N"], bool))  # the slot count includes slots K7 does not use
    on = r[:, 26] != 0
    assert (r[on, 6] == 1).all() and scenes.bits_equal(r[:, 7], c["walls"][wr.ALL].wsum)


def test_totals_tree_properties():
    c = oracle_case("tiny")
    st, cfg = c["state"], c["cfg"]
    mid = f32(0.5) * f32(cfg.xmax)
    inf = np.inf
    rg = [diag_ref.EVERYTHING, (-inf, -inf, -inf, mid, inf, inf), (mid, -inf, -inf, inf, inf, inf), (5, 5, 5, 5, 9, 9), (-9, -9, -9, -1, -1, -1)]
    recs = {s: w.records for s, w in c["walls"].items()}
    t = {s: wr.diag_records(st, recs[s], rg, (1, 2)) for s in recs}
    ta = t[wr.ALL]
    w = c["walls"][wr.ALL]
    liquid = np.trunc(st["types"]) == 1
    assert ta[0, 0] == liquid.sum() and ta[0, 1] == w.contact.sum() == ta[0, 2] and ta[0, 3] == w.reflected.sum() and ta[0, 25] == ta[0, 1]
    assert not ta[3].any() and not ta[4].any() and not ta[:, 27:].any()
    # integer-valued words add up exactly over a partition of the box, and over the partition of the walls
    for word in (0, 1, 2, 3, 25):
        assert ta[0, word] == ta[1, word] + ta[2, word]
    assert t[wall_cases.SLOT_A][0, 1] == ta[0, 1]  # contact is the particle's, whatever the set
    assert t[wall_cases.SLOT_A][0, 2] + t[wall_cases.SLOT_B][0, 2] + t[wr.NO_BODY][0, 2] >= ta[0, 2]
    # the tree is not the sequential sum, and it is what the contract says: one chunk of 1024 at a time
    terms = np.where(diag_ref.selected(st, rg[0], (1, 2)), recs[wr.ALL][:, 4].astype(np.float64), 0.0)
    assert u64(ta[0, 8]) == u64(diag_ref.tree_sum(terms)) and ta[0, 8] > 0
    assert abs(ta[0, 8] - terms.sum()) <= 1e-12 * np.abs(terms).sum()
    # types: the boundary particles' records are zero, so selecting them adds to the count alone
    tb = wr.diag_records(st, recs[wr.ALL], rg[:1], (1, 2, 3))
    assert tb[0, 0] == c["N"] and np.array_equal(u64(tb[0, 1:4]), u64(ta[0, 1:4]))


def test_wall_summary():
    c = oracle_case("tiny")
    cfg = c["cfg"]
    rec = wr.diag_records(c["state"], c["walls"][wall_cases.SLOT_A].records, [diag_ref.EVERYTHING], (1, 2))[0]
    s = frames.wall_summary(rec, cfg.mass, cfg.timeStep)
    m, dt = float(cfg.mass), float(cfg.timeStep)
    assert s["n"] == rec[0] and s["n_contact"] == rec[1] and s["n_shared"] == rec[2] and s["n_reflected"] == rec[3]
    assert np.array_equal(s["contact_force"], m / dt * rec[7:10]) and s["contact_force"][1] > 0  # the lifted floor pushes up
    assert np.array_equal(s["viscous"], m * rec[10:13]) and np.array_equal(s["tension"], m * rec[13:16]) and np.array_equal(s["pressure"], m * rec[16:19])
    assert np.array_equal(s["stage_force"], (s["viscous"] + s["pressure"]) + s["tension"])
    assert np.array_equal(s["body_contact_load"], -s["contact_force"]) and np.array_equal(s["body_stage_load"], -s["stage_force"])
    assert np.array_equal(s["body_load"], -(s["contact_force"] + s["stage_force"]))
    assert np.array_equal(s["contact_torque"], m / dt * rec[19:22]) and np.array_equal(s["stage_torque"], m * rec[22:25])
    assert np.array_equal(s["body_torque"], -(s["contact_torque"] + s["stage_torque"]))
    assert np.array_equal(s["shift"], rec[4:7]) and s["share"] == rec[25] and s["w_set"] == rec[26]
    assert len(frames.WALL_FIELDS) == sphmi.WALL_WORDS == wr.WORDS and len(frames.WALL_DIAG_FIELDS) == sphmi.WALL_DIAG_WORDS == wr.DIAG_WORDS
    assert len(set(frames.WALL_FIELDS)) == 32 and len(set(frames.WALL_DIAG_FIELDS)) == 32
    assert frames.WALL_FIELDS[6] == "share" and frames.WALL_FIELDS[19] == "x" and frames.WALL_DIAG_FIELDS[7] == "sum_dv_x"


def test_binding_lists_the_wall_calls():
    lib = ctypes.CDLL(sphmi.LIB_PATH)
    txt = open(scenes.ROOT + "/include/sphmi.h").read()
    for n in ("sph_wall_measure", "sph_wall_diagnostics"):
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for m in ("wall_measure", "wall_diagnostics"):
        assert callable(getattr(sphmi.owHIPSolver, m))
    assert "#define SPH_WALL_WORDS %d" % sphmi.WALL_WORDS in txt and "#define SPH_WALL_DIAG_WORDS %d" % sphmi.WALL_DIAG_WORDS in txt
    assert "#define SPH_WALL_ALL (%d)" % sphmi.WALL_ALL in txt and "#define SPH_WALL_NO_BODY (%d)" % sphmi.WALL_NO_BODY in txt
    assert (wr.ALL, wr.NO_BODY) == (sphmi.WALL_ALL, sphmi.WALL_NO_BODY)
    assert "#define SPHMI_ABI_VERSION 2" in txt
