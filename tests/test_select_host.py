"""CPU tests of the numpy restatement of the particle-selection contract (tests/select_ref.py) and of the selection helpers of
sphmi.frames: they pin the restatement the GPU tests compare the library with (tests/test_select.py), independently of the
library. No GPU."""
import numpy as np
import pytest

import components_ref as cr
import scenes
import select_ref as sr
import sphmi
from sphmi import frames

f32 = np.float32
INF = np.inf


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def block_3x3x3():
    """27 particles on integer coordinates 0..2, index = (x * 3 + y) * 3 + z; every row lists all the others in ascending
    order. With h = 2 and simScale = 1: hs2 = 4, ss2 = 1, t = 4 - r2, and every product and sum is a small integer."""
    pos = np.array([(x, y, z) for x in range(3) for y in range(3) for z in range(3)], np.float32)
    rows = np.full((27, 32), -1, np.int32)
    for i in range(27):
        rows[i, :26] = [j for j in range(27) if j != i]
    return pos, rows


def test_centre_of_a_full_block_is_exactly_zero():
    pos, rows = block_3x3x3()
    m = sr.measure(pos, rows, 2.0, 1.0)
    assert m[13] == 0.0 and u32(m[13:14])[0] == 0  # (1, 1, 1): +0 bits
    assert (m[np.arange(27) != 13] > 0).all()


def test_face_particle_is_the_rational_of_the_contract():
    """(0, 1, 1): the 8 neighbours in its own plane weigh 4 x 27 + 4 x 8 = 140, the 9 of the next plane 27 + 4 x 8 + 4 x 1 = 63
    with dx = 1, the 9 of the plane at dx = 2 lie at r2 >= 4 = h^2 (t <= 0: ignored). W = 203, B = (63, 0, 0)."""
    pos, rows = block_3x3x3()
    m = sr.measure(pos, rows, 2.0, 1.0)
    cx = f32(63) / f32(203)
    want = f32(np.sqrt(f32(cx * cx)) / f32(2))
    assert u32(m[4:5])[0] == u32([want])[0]
    assert abs(float(m[4]) - 63.0 / 406.0) < 2e-8
    assert sr.measure_scalar(pos, rows[4], 4, 2.0, 1.0) == m[4]


def test_no_neighbours_gives_one_and_entries_at_or_beyond_h_are_ignored():
    pos = np.array([(0, 0, 0), (2, 0, 0), (3, 0, 0), (0, 1, 0)], np.float32)
    rows = np.full((4, 32), -1, np.int32)
    m = sr.measure(pos, rows, 2.0, 1.0)
    assert (m == 1.0).all()
    rows[0, :2] = [1, 2]  # r == h exactly (t == 0) and r > h (t < 0): both ignored, W stays 0
    assert sr.measure(pos, rows, 2.0, 1.0)[0] == 1.0
    rows[0, 2] = 0  # the particle itself is skipped
    assert sr.measure(pos, rows, 2.0, 1.0)[0] == 1.0
    rows[0, 5] = 3  # one real neighbour at distance 1: the centroid is the neighbour, m = 1 / h
    assert sr.measure(pos, rows, 2.0, 1.0)[0] == 0.5
    rows[0, :3] = -1  # ... whatever else the row held
    assert sr.measure(pos, rows, 2.0, 1.0)[0] == 0.5


def test_the_restatement_follows_the_slots():
    """Float sums depend on their order: the vectorised restatement equals a plain loop over the slots for a row and for its
    reverse, bit for bit, and for some particle the two orders differ."""
    cfg = sphmi.default_config()
    h, ss = cfg.h, cfg.simulationScale
    rng = np.random.default_rng(17)
    pos = (rng.random((200, 3)) * 4.0).astype(np.float32)
    rows = np.full((200, 32), -1, np.int32)
    for i in range(200):
        d2 = ((pos - pos[i]) ** 2).sum(1)
        near = np.flatnonzero((d2 < float(h) ** 2 * 1.1) & (np.arange(200) != i))[:32]
        rows[i, :near.size] = near
    rev = rows[:, ::-1].copy()
    a, b = sr.measure(pos, rows, h, ss), sr.measure(pos, rev, h, ss)
    for i in range(200):
        assert u32([sr.measure_scalar(pos, rows[i], i, h, ss)])[0] == u32(a[i:i + 1])[0]
        assert u32([sr.measure_scalar(pos, rev[i], i, h, ss)])[0] == u32(b[i:i + 1])[0]
    assert (u32(a) != u32(b)).any()
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() < 1e-5  # the same quantity all the same
    assert ((a >= 0) & (a <= 1.0 + 1e-6)).all()


def test_underflow_regression_with_the_real_constants():
    """simulationScale is about 2e-6, so w is about 1e-31: the quotients must be taken before the squares. A face particle of a
    lattice at the usual spacing has m > 0.1, while sqrt(B.B) / (W h) underflows to 0."""
    cfg = sphmi.default_config()
    h, ss = f32(cfg.h), f32(cfg.simulationScale)
    sp = f32(0.93) * f32(cfg.r0)
    pos = (np.array([(x, y, z) for x in range(5) for y in range(5) for z in range(5)], np.float32) * sp).astype(np.float32)
    N = pos.shape[0]
    rows = np.full((N, 32), -1, np.int32)
    for i in range(N):
        d2 = ((pos.astype(np.float64) - pos[i]) ** 2).sum(1)
        near = np.flatnonzero((d2 < float(h) ** 2) & (np.arange(N) != i))
        rows[i, :min(near.size, 32)] = near[:32]
    m = sr.measure(pos, rows, h, ss)
    face = (0 * 5 + 2) * 5 + 2  # (0, 2, 2)
    centre = (2 * 5 + 2) * 5 + 2
    assert m[face] > 0.1 and m[centre] < 1e-6
    # the first version of the definition, on the face particle
    _, hs2, ss2 = sr.constants(h, ss)
    W = B = f32(0)
    for j in rows[face][rows[face] >= 0]:
        d = pos[j] - pos[face]
        t = hs2 - ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * ss2
        if t > 0:
            w = (t * t) * t
            W, B = W + w, B + w * d[0]
    assert 0 < W < 1e-28
    with np.errstate(under="ignore"):
        assert f32(B * B) == 0.0 and np.sqrt(f32(B * B)) / (W * h) == 0.0


LATTICE = {"tiny": 0.93, "tiny_jitter": 0.93, "tiny_compressed": 0.85}


@pytest.mark.parametrize("name", sorted(LATTICE))
def test_outer_layer_of_a_resting_lattice_is_above_the_threshold(name):
    """On the oracle's state after steps 0-2: every liquid particle of the outermost lattice layer (closer than half a lattice
    spacing to a face of the liquid's bounding box) has m >= 0.10, every liquid particle deeper than 2.5 spacings from all faces
    has m < 0.10, and both groups are non-empty. (Resting lattices: nothing here calibrates 0.10 for disordered liquid.)"""
    sc = scenes.SCENES[name]()
    cfg = sc["cfg"]
    ora = scenes.oracle_for(sc)
    spacing = float(f32(LATTICE[name]) * f32(cfg.r0))
    for step in range(3):
        ora.step()
        state, rows = cr.oracle_state(ora, cfg)
        m = sr.measure(state["pos"], rows, cfg.h, cfg.simulationScale)
        liquid = state["types"].astype(np.int32) == 1
        p = state["pos"][liquid].astype(np.float64)
        depth = np.minimum(p - p.min(0), p.max(0) - p).min(1)  # distance to the nearest face of the liquid's bounding box
        outer, deep = depth < 0.5 * spacing, depth > 2.5 * spacing
        ml = m[liquid]
        print("%s step %d: outer %d m in [%.3f, %.3f], deep %d m in [%.3f, %.3f], m >= 0.10: %d of %d" % (
            name, step, outer.sum(), ml[outer].min(), ml[outer].max(), deep.sum(), ml[deep].min(), ml[deep].max(),
            (ml >= f32(0.10)).sum(), ml.size))
        assert outer.sum() > 0 and deep.sum() > 0
        assert (ml[outer] >= f32(0.10)).all(), (name, step, float(ml[outer].min()))
        assert (ml[deep] < f32(0.10)).all(), (name, step, float(ml[deep].max()))
        assert ((m >= 0) & (m <= 1.0 + 1e-6)).all()


def synthetic_state(n=64):
    """Particles on a line x = 0 .. n-1 with every quantity a known function of the index."""
    i = np.arange(n)
    pos = np.zeros((n, 3), np.float32)
    pos[:, 0] = i
    pos[:, 1] = i % 4
    pos[:, 2] = -(i % 3)
    vel = np.zeros((n, 3), np.float32)
    vel[:, 0] = 3 * (i % 5)
    vel[:, 1] = 4 * (i % 5)  # speed = 5 * (i % 5)
    types = np.where(i % 8 == 7, f32(3.0), np.where(i % 8 == 3, f32(2.1), f32(1.0))).astype(np.float32)
    keys = np.where(i == 10, 99, 0).astype(np.int64)  # particle 10 lies outside the cell table
    state = dict(pos=pos, vel=vel, rho=(1000 + i).astype(np.float32), p=(i * 0.5).astype(np.float32), types=types, keys=keys, G=50,
                 ids=(n - 1 - i).astype(np.int64), h=2.0, simScale=1.0)
    rows = np.full((n, 32), -1, np.int32)
    for k in range(n):
        nb = [j for j in (k - 1, k + 1) if 0 <= j < n]
        rows[k, :len(nb)] = nb
    return state, rows


def test_selection_semantics():
    state, rows = synthetic_state()
    n = 64
    q = sr.Quantities(state, rows)
    i = np.arange(n)
    base = (i % 8 != 7) & (i != 10)  # types (1, 2), key inside the table
    assert np.array_equal(q.count, np.where((i == 0) | (i == n - 1), 1, 2).astype(np.float32))
    # the full and the empty selection
    full = sr.select(state, q)
    assert np.array_equal(full, np.flatnonzero(base)) and full.dtype == np.int32
    assert sr.select(state, q, types=(1, 2, 3)).size == n - 1
    assert sr.select(state, q, region=(5, -INF, -INF, 5, INF, INF)).size == 0
    assert sr.select(state, q, terms=[("density", 5000, INF)]).size == 0
    # half-open box: x0 <= x < x1
    got = sr.select(state, q, region=(4, -INF, -INF, 9, INF, INF))
    assert got.tolist() == [4, 5, 6, 8]
    assert sr.select(state, q, region=(4, 1, -INF, 9, 2, INF)).tolist() == [5]  # y = i % 4 in [1, 2)
    # half-open term bounds, +-inf bounds
    assert sr.select(state, q, terms=[("density", 1004, 1009)]).tolist() == [4, 5, 6, 8]
    assert sr.select(state, q, terms=[(0, -INF, 1002)]).tolist() == [0, 1]
    assert sr.select(state, q, terms=[("pressure", 30.0, INF)]).tolist() == [j for j in range(60, 64) if base[j]]
    assert np.array_equal(sr.select(state, q, terms=[("speed", -INF, INF)]), full)
    assert np.array_equal(sr.select(state, q, terms=[("speed", 10, 15)]), np.flatnonzero(base & (i % 5 == 2)))
    assert sr.select(state, q, terms=[("neighbors", 1, 2)]).tolist() == [0]  # (63 is a boundary particle)
    assert sr.select(state, q, types=(3,), terms=[("neighbors", 1, 2)]).tolist() == [63]
    assert np.array_equal(sr.select(state, q, terms=[("z", -1, 0)]), np.flatnonzero(base & (i % 3 == 1)))
    # several terms are a conjunction
    both = sr.select(state, q, terms=[("speed", 10, 15), ("z", -1, 0), ("x", 0, 40), ("density", 1000, 1030)])
    assert both.tolist() == [j for j in range(30) if base[j] and j % 5 == 2 and j % 3 == 1]
    assert both.size > 0
    with pytest.raises(ValueError):
        sr.select(state, q, terms=[("x", 0, 1)] * 5)
    with pytest.raises(ValueError):
        sr.select(state, q, terms=[("x", 1, 1)])
    with pytest.raises(ValueError):
        sr.select(state, q, terms=[("x", np.nan, 1)])
    # a NaN q fails the term, even with infinite bounds
    st = dict(state)
    st["rho"] = state["rho"].copy()
    st["rho"][[2, 20]] = np.nan
    qn = sr.Quantities(st, rows)
    got = sr.select(st, qn, terms=[("density", -INF, INF)])
    assert np.array_equal(got, np.flatnonzero(base & (i != 2) & (i != 20)))
    # the surface term: the ends of the line see one neighbour (m = 1 / h), the others a symmetric pair (m = 0)
    line = dict(state)
    line["pos"] = state["pos"] * np.array([1, 0, 0], np.float32)  # (y = z = 0: every neighbour at distance 1)
    ql = sr.Quantities(line, rows)
    assert ql.m[0] == 0.5 and ql.m[n - 1] == 0.5 and (ql.m[1:n - 1] == 0).all()
    assert sr.select(line, ql, types=(1, 2, 3), terms=[("surface", 0.1, INF)]).tolist() == [0, n - 1]
    assert sr.select(line, ql, terms=[(7, 0.1, INF)]).tolist() == [0]
    assert sr.select(line, ql, terms=[(7, 0.5, INF)]).tolist() == [0] and sr.select(line, ql, terms=[(7, 0.1, 0.5)]).size == 0
    # component filter
    labels = np.where(base, i // 16, -1).astype(np.int32)
    assert np.array_equal(sr.select(state, q, component=2, labels=labels), np.flatnonzero(base & (i // 16 == 2)))
    assert np.array_equal(sr.select(state, q, component=-1, labels=labels), full)
    assert sr.select(state, q, component=2, labels=labels, terms=[("x", 0, 33)]).tolist() == [32]
    # ascending order, orig ids, records
    for sel in (full, both, got):
        assert (np.diff(sel) > 0).all()
    ids, rec = sr.records(state, q, both)
    assert ids.dtype == np.uint32 and rec.dtype == np.float32 and rec.shape == (both.size, sr.WORDS)
    assert np.array_equal(ids, (n - 1 - both).astype(np.uint32))
    assert np.array_equal(rec[:, 0], both.astype(np.float32)) and np.array_equal(rec[:, 7], (1000 + both).astype(np.float32))
    assert np.array_equal(u32(rec[:, 3]), u32(state["types"][both]))  # the type's bit pattern (2.1 stays 2.1)
    assert np.array_equal(rec[:, 4:7], state["vel"][both]) and np.array_equal(rec[:, 8], state["p"][both])
    assert np.array_equal(rec[:, 9], q.count[both]) and np.array_equal(rec[:, 10], q.m[both]) and (rec[:, 11] == 0).all()
    ids, rec = sr.records(state, q, np.zeros(0, np.int32))
    assert ids.shape == (0,) and rec.shape == (0, sr.WORDS)


def test_field_names_agree_with_the_package():
    assert sr.FIELDS == sphmi.SELECT_FIELDS and sr.FIELDS.index("surface") == sr.SURFACE == 7
    assert sr.WORDS == sphmi.SELECT_WORDS == len(frames.SELECT_FIELDS) and sr.MAX_TERMS == sphmi.SELECT_MAX_TERMS
    for name in ("sph_particle_measure", "sph_select_particles", "sph_read_selection"):
        assert name in sphmi.EXPORTED_SYMBOLS


def test_frames_selection_round_trip(tmp_path):
    state, rows = synthetic_state()
    q = sr.Quantities(state, rows)
    idx = sr.select(state, q, terms=[("speed", 10, 15)])
    ids, rec = sr.records(state, q, idx)
    rec[0, 8] = np.float32(-0.0)
    path = str(tmp_path / "selection_3.bin")
    assert frames.write_selection(path, idx, ids, rec) == idx.size
    gi, gd, gr = frames.read_selection(path)
    assert gi.dtype == np.int32 and gd.dtype == np.uint32 and gr.dtype == np.float32
    assert np.array_equal(gi, idx) and np.array_equal(gd, ids) and np.array_equal(u32(gr), u32(rec))
    frames.write_selection(path, idx[:0], ids[:0], rec[:0])  # the empty selection
    gi, gd, gr = frames.read_selection(path)
    assert gi.shape == (0,) and gd.shape == (0,) and gr.shape == (0, 12)
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError):
        frames.read_selection(path)
    with pytest.raises(ValueError):
        frames.write_selection(path, idx, ids[:-1], rec)
    # npz
    npz = str(tmp_path / "frame.npz")
    frames.write_npz(npz, np.zeros((4, 4), np.float32), np.zeros(4, np.float32), step=3, selection=(idx, ids, rec))
    with np.load(npz) as z:
        assert np.array_equal(z["selection_index"], idx) and np.array_equal(z["selection_id"], ids)
        assert np.array_equal(u32(z["selection_records"]), u32(rec)) and int(z["step"]) == 3
    # vtk: header, point count and the big-endian payloads in order
    vtk = str(tmp_path / "selection.vtk")
    assert frames.write_vtk_selection(vtk, rec, ids) == idx.size
    data = open(vtk, "rb").read()
    n = idx.size
    assert data.startswith(b"# vtk DataFile Version 3.0\nsphmi selection\nBINARY\nDATASET POLYDATA\n")
    at = data.index(b"POINTS %d float\n" % n) + len(b"POINTS %d float\n" % n)
    assert np.array_equal(np.frombuffer(data, ">f4", 3 * n, at).reshape(n, 3), rec[:, :3])
    for name, col in (("type", 3), ("density", 7), ("pressure", 8), ("neighbors", 9), ("surface", 10)):
        tag = b"SCALARS %s float 1\nLOOKUP_TABLE default\n" % name.encode()
        at = data.index(tag) + len(tag)
        assert np.array_equal(np.frombuffer(data, ">f4", n, at).astype(np.float32).view(np.uint32), u32(rec[:, col])), name
    tag = b"SCALARS id int 1\nLOOKUP_TABLE default\n"
    assert np.array_equal(np.frombuffer(data, ">i4", n, data.index(tag) + len(tag)), ids.astype(np.int32))
    tag = b"VECTORS velocity float\n"
    assert np.array_equal(np.frombuffer(data, ">f4", 3 * n, data.index(tag) + len(tag)).reshape(n, 3), rec[:, 4:7])
    with pytest.raises(ValueError):
        frames.write_vtk_selection(vtk, rec, ids[:-1])
