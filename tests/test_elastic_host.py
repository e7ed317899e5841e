"""CPU tests of the elastic-matter restatement (tests/elastic_ref.py), the yardstick the GPU calls are held to
(tests/test_elastic.py): hand-made rows and triangles with exact answers, the tie to the oracle's elastic-force stage bit for
bit, the properties of the fixed tree, and the host-side helpers of sphmi.frames."""
import os

import numpy as np
import pytest

import elastic_ref as er
import scenes
import sphmi
from sphmi import frames

f32 = np.float32


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def table(rows):
    """A connection table from rows of (partner, L0, group) tuples; -1 terminated and padded like the generator's."""
    t = np.zeros((len(rows), 32, 4), np.float32)
    t[:, :, 0] = -1.0
    for i, row in enumerate(rows):
        for k, (j, L0, g) in enumerate(row):
            t[i, k] = (f32(j) + f32(0.1) if j >= 0 else f32(-1.0), L0, g, 0)
    return t


def hand_made():
    """Six elastic particles on integer coordinates (simulationScale 1, identity sort): every length is an integer."""
    pos = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 12], [0, 0, 0], [6, 8, 0], [1, 0, 0]], np.float32)
    rows = [
        [(1, 4.0, 1.5), (2, 8.0, 0.0), (3, 2.0, 1.9), (4, 0.0, 1.0)],  # r = 5, 12, 0 (r == 0), 10 with L0 == 0
        [],                                                            # ends at slot 0
        [(0, 16.0, 3.2), (-1, 0, 0), (1, 1.0, 1.0)],                   # group 3 > muscleCount -> 0; the slot behind the end is dead
        [((k % 5) + (1 if (k % 5) >= 3 else 0), 1.0, 2.0) for k in range(32)],  # a full row of 32, all in muscle 2 (signal <= 0)
        [(0, 8.0, 1.0)],                                               # r = 10
        [(0, 2.0, 1.0)],                                               # r = 1: compressed
    ]
    return pos, table(rows)


def test_hand_made_rows_have_exact_answers():
    pos, tab = hand_made()
    back = np.arange(6)
    signal = np.array([2.0, -1.0], np.float32)  # muscle 1 active, muscle 2 not
    c = er.Connections(pos, back, tab, 0, 1.0, 2, signal)
    assert not c.bad
    idx, rec, con = er.elastic_records(c)
    idx2, rec2, con2 = er.elastic_records_fast(c)
    assert np.array_equal(u32(rec), u32(rec2)) and np.array_equal(u32(con), u32(con2)) and np.array_equal(idx, idx2)
    assert idx.tolist() == list(range(6))
    # row 0: r = 5, 12, 0, 10; L0 = 4, 8, 2, 0 -> dr = 1, 4, -2, 10; e = 0.25, 0.5, -1, 0 (L0 == 0)
    assert con[0, :4].tolist() == [[5, 1], [12, 4], [0, -2], [10, 10]] and con[0, 4:].tolist() == [[-1, 0]] * 28
    assert rec[0, :6].tolist() == [4, 3, -1.0, 0.5, -0.25, 1 + 16 + 4 + 100]
    # spring: -(v/r)*dr*6e8 with v = x_0 - x_j: slot 0 (0.6, 0.8, 0)*1, slot 1 (0, 0, 1)*4, slot 2 none (r == 0), slot 3 (0.6, 0.8, 0)*10
    s0 = [f32(f32(f32(0.6) * f32(1)) * er.K_SPRING), f32(f32(f32(0.8) * f32(1)) * er.K_SPRING)]
    s3 = [f32(f32(f32(0.6) * f32(10)) * er.K_SPRING), f32(f32(f32(0.8) * f32(10)) * er.K_SPRING)]
    assert rec[0, 6] == f32(s0[0] + s3[0]) and rec[0, 7] == f32(s0[1] + s3[1]) and rec[0, 8] == f32(4) * er.K_SPRING
    # contraction: muscle 1, signal 2: slots 0 and 3 (slot 2 has r == 0): (0.6, 0.8, 0) * 2 * 800, twice
    c0 = [f32(f32(f32(0.6) * f32(2)) * er.K_MUSCLE), f32(f32(f32(0.8) * f32(2)) * er.K_MUSCLE)]
    assert rec[0, 9] == f32(c0[0] + c0[0]) and rec[0, 10] == f32(c0[1] + c0[1]) and rec[0, 11] == 0
    # row 1 ends at slot 0
    assert not rec[1].any() and con[1].tolist() == [[-1, 0]] * 32
    # row 2: one live slot, r = 12, L0 = 16, group 3 is above muscleCount; the slot behind the terminator is dead
    assert rec[2, :6].tolist() == [1, 0, -0.25, -0.25, -0.25, 16] and con[2, :3].tolist() == [[12, -4], [-1, 0], [-1, 0]]
    assert rec[2, 8] == f32(f32(-f32(1.0)) * f32(-4)) * er.K_SPRING and not rec[2, 9:].any()
    # row 3: a full row; muscle 2 has signal <= 0: no contraction term
    assert rec[3, 0] == 32 and rec[3, 1] == 32 and not rec[3, 9:].any() and (con[3, :, 0] >= 0).all()
    assert rec[5, :6].tolist() == [1, 1, -0.5, -0.5, -0.5, 1]
    # groups
    m = er.muscle_records(c, 2, signal)
    assert m.shape == (3, 16)
    assert m[:, 0].tolist() == [2, 5, 32] and m[:, 0].sum() == c.live.sum() == 39
    assert m[:, 1].tolist() == [0, 2, -1]
    # record 1: slots (5, 4), (0, 2), (10, 0), (10, 8), (1, 2) as (r, L0)
    assert m[1, 2:6].tolist() == [16, 26, 10, 1 + 4 + 100 + 4 + 1] and m[1, 6:9].tolist() == [0.25 - 1 + 0 + 0.25 - 0.5, -1, 0.25]
    assert m[1, 9] == float(f32(1) * er.K_SPRING) * 10 and m[1, 10] == 4 * 1600.0 and m[1, 14] == 1
    assert m[1, 11:14].tolist() == [0 + 0 + 0 + 6 + 1, 8, 0]
    assert m[0, 2:5].tolist() == [24, 24, 0] and m[0, 10] == 0 and m[0, 7:9].tolist() == [-0.25, 0.5]
    assert m[2, 10] == 0 and m[2, 0] == 32 and m[:, 15].tolist() == [0, 0, 0]
    # an id outside 0..N-1 is reported and not followed
    bad = tab.copy()
    bad[4, 0, 0] = 6.1
    assert er.Connections(pos, back, bad, 0, 1.0, 2, signal).bad


def test_a_record_does_not_depend_on_the_other_groups():
    pos, tab = hand_made()
    back = np.arange(6)
    signal = np.array([2.0, -1.0, 0.5, 0.0], np.float32)
    full = er.muscle_records(er.Connections(pos, back, tab, 0, 1.0, 4, signal), 4, signal)
    assert full[3, 0] == 1  # group 3 exists now: the connection leaves record 0
    two = er.muscle_records(er.Connections(pos, back, tab, 0, 1.0, 2, signal[:2]), 2, signal[:2])
    assert np.array_equal(full[1:3].view(np.uint64), two[1:3].view(np.uint64))
    assert full[0, 0] + full[3, 0] == two[0, 0] and full[:, 0].sum() == two[:, 0].sum() == 39


def test_hand_made_triangles():
    pos = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 2], [6, 0, 0], [1, 1, 1]], np.float32)
    back = np.array([5, 4, 3, 2, 1, 0])  # a real permutation: sorted index of original id o
    sp = pos[np.argsort(back)]  # sorted position s holds the original particle with back[o] == s
    assert np.array_equal(sp[back], pos)
    tris = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [0, 1, 4], [5, 5, 5]], np.int32)
    rec, totals = er.membrane_records(sp, back, tris)
    assert rec[:, 0].tolist() == [6, 6, 3, 0, 0]
    assert rec[0, 1:4].tolist() == [0, 0, 1] and rec[1, 1:4].tolist() == [0, 0, -1] and rec[2, 1:4].tolist() == [0, -1, 0]
    assert not rec[3, 1:4].any() and not rec[4, 1:4].any()  # degenerate: normal 0
    assert rec[0, 4:7].tolist() == [1, f32(4) / f32(3), 0] and rec[4, 4:7].tolist() == [1, 1, 1] and not rec[:, 7].any()
    assert totals.tolist() == [5, 15, 0, 6]


@pytest.mark.parametrize("name", ["tiny_elastic", "elastic_offset_box", "worm"])
@pytest.mark.parametrize("muscles", [False, True])
def test_force_terms_reproduce_the_oracles_elastic_stage(name, muscles):
    """r, dr and both force terms are the reference's arithmetic: added to the acceleration before the elastic-force stage, in
    slot order, they give the acceleration after it, bit for bit."""
    sc = scenes.worm_scene() if name == "worm" else (scenes.elastic_offset_box() if name == "elastic_offset_box" else scenes.SCENES[name]())
    cfg = sc["cfg"]
    ora = scenes.oracle_for(sc)
    N = cfg.particleCount
    signal = np.zeros(cfg.muscleCount, np.float32)
    steps = 1 if name == "worm" else 3
    for it in range(steps):
        if muscles:
            signal = sphmi.muscle_signal(60 + 40 * it, cfg.muscleCount)
            if name != "worm":
                signal[0] = f32(0.75)  # these scenes have one muscle
            ora.update_muscles(signal)
        if it < steps - 1:
            ora.step()
    upto = scenes.STAGE_SEQUENCE.index("computeForcesAndInitPressure")
    for st in scenes.STAGE_SEQUENCE[:upto + 1]:
        ora.run(st)
    before = ora.buffer("acceleration").reshape(-1, 4)[:N, :3].copy()
    sp = ora.buffer("sortedPosition").reshape(-1, 4)[:N]
    back = ora.buffer("particleIndexBack")[:N]
    ora.run("computeElasticForces")
    after = ora.buffer("acceleration").reshape(-1, 4)[:N, :3]
    c = er.Connections(sp, back, sc["elastic"], cfg.elasticOffset, cfg.simulationScale, cfg.muscleCount, signal)
    assert not c.bad and c.live.sum() > 0
    acc = before.copy()
    rows = c.owner
    for k in range(32):  # per slot: the spring term, then the contraction term (the stage's order)
        for has, term in ((c.has_s[:, k], c.s[:, k]), (c.has_c[:, k], c.c[:, k])):
            acc[rows[has]] = (acc[rows[has]] + term[has]).astype(np.float32)
    assert np.unique(rows).size == rows.size
    assert scenes.bits_equal(acc, after), scenes.diff_report(acc, after)
    assert not scenes.bits_equal(before, after)
    assert c.has_c.any() == muscles
    # the per-particle record's sums are the same terms, each as a sum of its own
    _, rec, _ = er.elastic_records_fast(c)
    if name != "worm":
        assert np.array_equal(u32(rec), u32(er.elastic_records(c)[1]))
    assert (rec[:, 0] == c.live.sum(1)).all()
    ora.close()


def test_worm_fixture_group_counts():
    """The counts of the worm fixture: 137,804 live connections, 127,436 in no muscle and 10,368 in the 96 muscles (108 each on
    average; the groups hold between 16 and 190), none in groups 97..100; muscleCount changes which records exist, not what a
    record holds."""
    sc = scenes.worm_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    pos = sc["position"]
    back = np.arange(N)  # the initial state, unsorted: positions in original order
    signal = sphmi.muscle_signal(100, cfg.muscleCount)
    assert (signal > 0).sum() > 3
    c = er.Connections(pos, back, sc["elastic"], 0, cfg.simulationScale, cfg.muscleCount, signal)
    assert cfg.numOfElasticP == 10143 and cfg.numOfMembranes == 11386 and int(c.live.sum()) == 137804
    m = er.muscle_records(c, cfg.muscleCount, signal)
    assert m.shape == (101, 16)
    assert m[0, 0] == 127436 and (m[1:97, 0] > 0).all() and m[1:97, 0].sum() == 96 * 108 and (m[97:, 0] == 0).all()
    assert m[:, 0].sum() == 137804 and m[1:97, 0].min() == 16 and m[1:97, 0].max() == 190
    assert not m[97:, 2:].any() and (m[1:97, 1] == signal[:96]).all()
    assert (m[1:97, 10] > 0).sum() == (signal[:96] > 0).sum() and (m[:, 14] == 0).all()
    # every spring is listed from both ends: the owning-end sum over n is the centroid of the spring midpoints
    g = 5
    sel = c.live & (c.m == g)
    rows, slots = np.nonzero(sel)
    partner = np.trunc(np.asarray(sc["elastic"], np.float32).reshape(-1, 32, 4)[rows, slots, 0]).astype(np.int64)
    mid = 0.5 * (pos[rows, :3].astype(np.float64) + pos[partner, :3].astype(np.float64))
    assert np.allclose(m[g, 11:14] / m[g, 0], mid.mean(0), rtol=1e-6)
    # with muscleCount 96 the same records; with 40 the groups above go to record 0
    c96 = er.Connections(pos, back, sc["elastic"], 0, cfg.simulationScale, 96, signal[:96])
    m96 = er.muscle_records(c96, 96, signal[:96], groups=[0, 1, 50, 96])
    for g in (0, 1, 50, 96):
        assert np.array_equal(m96[g].view(np.uint64), m[g].view(np.uint64))
    c40 = er.Connections(pos, back, sc["elastic"], 0, cfg.simulationScale, 40, signal[:40])
    m40 = er.muscle_records(c40, 40, signal[:40], groups=[0, 7, 40])
    assert np.array_equal(m40[7].view(np.uint64), m[7].view(np.uint64)) and np.array_equal(m40[40].view(np.uint64), m[40].view(np.uint64))
    assert m40[0, 0] == 127436 + m[41:97, 0].sum()
    # the membrane table: areas are positive and the tree's total is the exactly rounded sum here
    rec, totals = er.membrane_records(pos, back, sc["membranes"])
    assert totals[0] == 11386 and totals[2] > 0 and totals[3] >= totals[2]
    assert abs(totals[1] - rec[:, 0].astype(np.float64).sum()) <= 1e-9 * totals[1]


def test_frames_helpers(tmp_path):
    pos, tab = hand_made()
    signal = np.array([2.0, -1.0], np.float32)
    c = er.Connections(pos, np.arange(6), tab, 0, 1.0, 2, signal)
    m = er.muscle_records(c, 2, signal)
    s = frames.muscle_summary(m)
    assert s.shape == (3, len(frames.MUSCLE_SUMMARY_FIELDS)) and len(frames.MUSCLE_FIELDS) == 16 and len(frames.ELASTIC_FIELDS) == 12
    assert s[1].tolist() == [1, 5, 2, 26 / 5, 16 / 5, (0.25 - 1 + 0.25 - 0.5) / 5, -1, 0.25]
    assert frames.muscle_summary(np.zeros((1, 16)))[0].tolist() == [0] * 8
    path = os.path.join(str(tmp_path), "muscles.csv")
    assert frames.write_muscles_csv(path, m) == 3
    assert np.array_equal(frames.read_muscles_csv(path).view(np.uint64), s.view(np.uint64))
    idx, rec, _ = er.elastic_records(c)
    p4 = np.concatenate([pos, np.full((6, 1), 2.1, np.float32)], axis=1)
    vtk = os.path.join(str(tmp_path), "elastic.vtk")
    assert frames.write_vtk_elastic(vtk, p4, np.arange(6, dtype=np.uint32), rec) == 6
    data = open(vtk, "rb").read()
    assert data.startswith(b"# vtk DataFile") and b"VECTORS spring_acceleration float" in data and b"SCALARS max_strain float 1" in data
    with pytest.raises(ValueError):
        frames.write_vtk_elastic(vtk, p4, np.arange(5, dtype=np.uint32), rec)
