"""CPU tests of the particle-editing contract's numpy restatement (tests/edit_ref.py), of frames.track_ids, and of the premise the
feature rests on: between two steps the solver's state is exactly (position, velocity) in original-id order, so a solver made
from a read-back continues bit for bit like the one it was read from (checked on the C oracle). No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import edit_ref as er
import scenes
import sphmi
from sphmi import frames

f32 = np.float32
INF = np.inf


def _state(n, seed=1):
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 4), np.float32)
    pos[:, 3] = f32(1.0)
    vel = rng.random((n, 4), np.float32)
    return pos, vel


def test_remove_keeps_order_and_maps_ids():
    pos, vel = _state(10)
    marked = np.zeros(10, bool)
    marked[[0, 3, 4, 9]] = True
    p, v, m = er.remove(pos, vel, marked)
    assert scenes.bits_equal(p, pos[[1, 2, 5, 6, 7, 8]]) and scenes.bits_equal(v, vel[[1, 2, 5, 6, 7, 8]])
    assert m.dtype == np.int32 and m.tolist() == [-1, 0, 1, -1, -1, 2, 3, 4, 5, -1]
    # o - #marked below o
    for o in np.flatnonzero(~marked):
        assert m[o] == o - marked[:o].sum()
    # nothing marked: the identity; everything marked: refused
    p, v, m = er.remove(pos, vel, np.zeros(10, bool))
    assert scenes.bits_equal(p, pos) and m.tolist() == list(range(10))
    with pytest.raises(er.Refused):
        er.remove(pos, vel, np.ones(10, bool))


def test_region_marks_half_open_box_types_and_bounds():
    pos = np.array([[1, 1, 1, 1], [2, 1, 1, 1], [1, 2, 1, 1], [1, 1, 2, 1], [1.5, 1.5, 1.5, 3], [1.5, 1.5, 1.5, 2.1],
                    [np.nextafter(f32(2), f32(0)), 1, 1, 1], [1.5, 1.5, 1.5, 1.9]], f32)
    box = (1, 1, 1, 2, 2, 2)
    assert er.region_marks(pos, box, (1,)).tolist() == [True, False, False, False, False, False, True, True]  # lower in, upper out
    assert er.region_marks(pos, box, (3,)).tolist() == [False] * 4 + [True, False, False, False]
    assert er.region_marks(pos, box, (2,)).tolist() == [False] * 5 + [True, False, False]                      # (int)2.1 == 2
    assert er.region_marks(pos, box, (1, 2, 3)).sum() == 5
    assert er.region_marks(pos, None, (1,)).sum() == 6
    assert er.region_marks(pos, (-INF, -INF, -INF, INF, INF, INF), (1, 3)).sum() == 7
    assert er.region_marks(pos, (-INF, -INF, -INF, 1.5, INF, INF), (1,)).tolist() == [True, False, True, True, False, False, False, False]
    # the compare is a float32 compare: a bound between two floats rounds first
    edge = f32(1.0) + f32(2.0 ** -23)
    assert er.region_marks(np.array([[edge, 1, 1, 1]], f32), (1.0 + 2.0 ** -25, 0, 0, 2, 2, 2), (1,)).tolist() == [True]
    for k in range(6):
        b = [0, 0, 0, 1, 1, 1]
        b[k] = np.nan
        with pytest.raises(er.Refused):
            er.region_marks(pos, b, (1,))
    for bad in ((), (0,), (4,), (1, 5)):
        with pytest.raises(er.Refused):
            er.region_marks(pos, box, bad)


def test_id_marks_duplicates_and_range():
    assert er.id_marks(6, [4, 1, 4, 4, 1]).tolist() == [False, True, False, False, True, False]
    assert er.id_marks(6, []).sum() == 0
    for bad in ([6], [0, 7], [-1]):
        with pytest.raises(er.Refused):
            er.id_marks(6, bad)


def test_lattice_index_order_and_bit_patterns():
    o, s = (f32(0.1), f32(0.2), f32(0.3)), (f32(0.7), f32(0.011), f32(1.3))
    pos, vel = er.lattice(o, s, (3, 4, 2), velocity=(0.5, -1, 2), type_value=1.0)
    assert pos.shape == (24, 4) and pos.dtype == np.float32 and vel.shape == (24, 4)
    for iz in range(2):
        for iy in range(4):
            for ix in range(3):
                k = (iz * 4 + iy) * 3 + ix  # x fastest
                want = np.array([o[0] + f32(ix) * s[0], o[1] + f32(iy) * s[1], o[2] + f32(iz) * s[2], 1.0], f32)
                assert scenes.bits_equal(pos[k], want), k
    # one float multiply, one float add: not the double expression rounded once
    many, _ = er.lattice((f32(0.1),) * 3, (f32(0.01),) * 3, (1000, 1, 1))
    dbl = (np.float64(f32(0.1)) + np.arange(1000) * np.float64(f32(0.01))).astype(f32)
    two = f32(0.1) + (np.arange(1000).astype(f32) * f32(0.01))
    assert scenes.bits_equal(many[:, 0], two) and not scenes.bits_equal(many[:, 0], dbl)
    assert (vel == np.array([0.5, -1, 2, 0], f32)).all()
    assert er.lattice(o, s, (0, 4, 2))[0].shape == (0, 4)
    with pytest.raises(er.Refused):
        er.lattice(o, s, (3, -1, 2))


def test_append_validates_like_create():
    cfg = scenes.liquid_box_config((8.0, 8.0, 8.0), mask=0xffffffff)
    pos, vel = _state(5)
    ap, av = er.hand_made_particles(cfg, (f32(3) * f32(cfg.r0),) * 3)
    p, v = er.append(pos, vel, ap, av, cfg, capacity=12)
    assert scenes.bits_equal(p[:5], pos) and scenes.bits_equal(p[5:], ap) and scenes.bits_equal(v[5:], av)
    assert (ap[:, 3] == 3).sum() == 1
    with pytest.raises(er.Refused, match="capacity"):
        er.append(pos, vel, ap, av, cfg, capacity=11)
    for col, val, why in ((0, np.nan, "not finite"), (1, np.inf, "not finite"), (2, -1.0, "outside"), (3, 2.1, "type"), (3, 0.5, "type")):
        bad = ap.copy()
        bad[2, col] = val
        with pytest.raises(er.Refused, match="particle 2: " + why):
            er.append(pos, vel, bad, av, cfg)
    narrow = scenes.liquid_box_config((8.0, 8.0, 8.0))  # reference cell ids: out-of-box input aliases, as in sph_create
    bad = ap.copy()
    bad[2, 2] = -1.0
    er.append(pos, vel, bad, av, narrow)


@pytest.mark.parametrize("name", ["tiny_elastic", "elastic_offset_box"])
def test_elastic_range_refusal(name):
    sc = scenes.elastic_offset_box() if name == "elastic_offset_box" else scenes.SCENES[name]()
    cfg, pos, vel = sc["cfg"], sc["position"], sc["velocity"]
    N, E, off = cfg.particleCount, cfg.numOfElasticP, cfg.elasticOffset
    t = pos[:, 3].astype(np.int32)
    assert (t[off:off + E] == 2).all() and (t == 2).sum() == E
    # the liquid lies behind the elastic block in both orders: it can be drained
    liquid = er.region_marks(pos, None, (1,))
    assert liquid.any() and np.flatnonzero(liquid).min() >= off + E
    p, v, m = er.remove(pos, vel, liquid, E, off)
    assert p.shape[0] == N - liquid.sum() and (m[off:off + E] == np.arange(off, off + E)).all()  # the elastic ids did not shift
    # an elastic particle, and anything in front of the block, cannot go; the error names the lowest id
    for ids, first in (([off + 3, off + 1, N - 1], off + 1), ([off + E - 1], off + E - 1)):
        marked = er.id_marks(N, ids)
        assert er.elastic_range_check(marked, E, off) == first
        with pytest.raises(er.Refused, match="particle %d " % first):
            er.remove(pos, vel, marked, E, off)
    if off:  # file-mode order: the walls are stored in front of the elastic block
        walls = er.region_marks(pos, None, (3,))
        assert np.flatnonzero(walls).max() < off
        with pytest.raises(er.Refused, match="particle 0 "):
            er.remove(pos, vel, walls, E, off)
    else:    # generated order: the walls are stored last and can be opened (a gate)
        walls = er.region_marks(pos, None, (3,))
        assert er.remove(pos, vel, walls, E, off)[0].shape[0] == N - walls.sum()
    assert er.elastic_range_check(er.id_marks(N, [off + E]), E, off) is None
    assert er.elastic_range_check(er.id_marks(N, [0]), 0, 0) is None  # no elastic matter: no protected range


def test_track_ids_across_two_chained_edits():
    ids, nxt = frames.track_ids(np.arange(8))
    assert ids.tolist() == list(range(8)) and nxt == 8
    pos, vel = _state(8)
    # edit 1: remove 2 and 5, then add 3
    marked = er.id_marks(8, [2, 5])
    pos1, vel1, m1 = er.remove(pos, vel, marked)
    ap, av = _state(3, seed=2)
    pos1, vel1 = er.append(pos1, vel1, ap, av)
    ids1, nxt = frames.track_ids(ids, m1, added=3, next_id=nxt)
    assert ids1.tolist() == [0, 1, 3, 4, 6, 7, 8, 9, 10] and nxt == 11
    # edit 2: remove the last survivor of the original set, one of the new ones and particle 0; add 1
    marked = er.id_marks(9, [5, 7, 0])
    pos2, vel2, m2 = er.remove(pos1, vel1, marked)
    bp, bv = _state(1, seed=3)
    pos2, vel2 = er.append(pos2, vel2, bp, bv)
    ids2, nxt = frames.track_ids(ids1, m2, added=1, next_id=nxt)
    assert ids2.tolist() == [1, 3, 4, 6, 8, 10, 11] and nxt == 12  # 9 is gone and never given out again
    # the identities join the frames: every surviving original particle carries its own data
    first = {int(i): pos[i] for i in range(8)}
    for row, ident in enumerate(ids2):
        if ident < 8:
            assert scenes.bits_equal(pos2[row], first[int(ident)])
    assert scenes.bits_equal(pos2[ids2.tolist().index(8)], ap[0]) and scenes.bits_equal(pos2[-1], bp[0])
    # additions only, removal only, the default next id, a map of the wrong length
    assert frames.track_ids([4, 9], added=2)[0].tolist() == [4, 9, 10, 11]
    assert frames.track_ids([4, 9, 5], [1, -1, 0])[0].tolist() == [5, 4]
    assert frames.track_ids([], added=2) [0].tolist() == [0, 1]
    with pytest.raises(ValueError):
        frames.track_ids([1, 2, 3], [0, 1])


def test_binding_lists_the_editing_calls():
    names = ["sph_remove_region", "sph_remove_selection", "sph_remove_ids", "sph_add_particles", "sph_emit_lattice", "sph_read_edit_map"]
    lib = ctypes.CDLL(sphmi.LIB_PATH)
    txt = open(scenes.ROOT + "/include/sphmi.h").read()
    for n in names:
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for m in ("remove_region", "remove_selection", "remove_ids", "add_particles", "emit_lattice", "edit_map"):
        assert callable(getattr(sphmi.owHIPSolver, m))
    assert sphmi.ABI_VERSION == 2


def _oracle(sc, cfg, pos, vel):
    from oracle import oraclebind as O
    return O.OracleSolver(sphmi.config_dict(cfg), pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"], threads=4)


def _oracle_state(ora, n):
    return ora.buffer("position").reshape(-1, 4)[:n].copy(), ora.buffer("velocity").reshape(-1, 4)[:n].copy()


@pytest.mark.parametrize("name", ["tiny", "tiny_compressed", "tiny_elastic"])
def test_premise_state_between_steps_is_position_and_velocity(name):
    """k steps, read back, a fresh oracle from the read-back, m more steps on both: bit-identical. Then the restated drain and
    emit: an oracle made with the new count steps to a finite state."""
    K, M = 3, 3
    sc = scenes.SCENES[name]()
    cfg = sc["cfg"]
    N, E, off = cfg.particleCount, cfg.numOfElasticP, cfg.elasticOffset
    a = _oracle(sc, cfg, sc["position"], sc["velocity"])
    for _ in range(K):
        a.step()
    pos, vel = _oracle_state(a, N)
    b = _oracle(sc, cfg, pos, vel)
    for _ in range(M):
        a.step()
        b.step()
    for buf, n in (("position", 4 * N), ("velocity", 4 * N), ("rho", N)):
        assert scenes.bits_equal(a.buffer(buf)[:n], b.buffer(buf)[:n]), buf + ": " + scenes.diff_report(a.buffer(buf)[:n], b.buffer(buf)[:n])
    # the edit, restated: drain the middle of the liquid, clear a place, emit a block there, add seven particles
    r0 = f32(cfg.r0)
    marked = er.region_marks(pos, er.liquid_quantile_box(pos), (1,))
    assert 31 <= marked.sum() < (pos[:, 3].astype(np.int32) == 1).sum()
    p1, v1, m1 = er.remove(pos, vel, marked, E, off)
    sp = f32(0.93) * r0
    origin, place = er.clear_origin(p1, cfg, (6, 5, 4), sp, r0)
    p2, v2, _ = er.remove(p1, v1, er.region_marks(p1, place, (1,)), E, off)
    lp, lv = er.lattice(origin, (sp, sp, sp), (6, 5, 4))
    p3, v3 = er.append(p2, v2, lp, lv, cfg)
    assert p3.shape[0] == p2.shape[0] + 120
    c = _oracle(sc, er.with_count(cfg, p3.shape[0]), p3, v3)
    for _ in range(M):
        c.step()
    n3 = p3.shape[0]
    assert np.isfinite(c.buffer("position")[:4 * n3]).all() and np.isfinite(c.buffer("velocity")[:4 * n3]).all()
    assert np.isfinite(c.buffer("rho")[:n3]).all()
