"""CPU tests of the kinematic-body contract's numpy restatement (tests/body_ref.py), of the pose helpers of sphmi.frames, and of
the premise the feature rests on: a wall moved in the read-back state reaches the liquid through the step as it is (checked on the
C oracle). No tolerance anywhere: floats are compared as bit patterns."""
import ctypes

import numpy as np
import pytest

import body_ref as br
import edit_ref as er
import scenes
import sphmi
from sphmi import frames

f32 = np.float32


def _cfg(wide=False):
    return scenes.liquid_box_config((8.0, 8.0, 8.0), mask=0xffffffff if wide else 0xffff)


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def test_pose_by_hand():
    # 90 degrees about z, then a shift: (x, y, z) -> (-y + 10, x + 20, z + 30); the normal turns and is not shifted
    pose = np.array([[0, -1, 0, 10], [1, 0, 0, 20], [0, 0, 1, 30]], f32)
    p, n = br.placed(pose, [[1, 2, 3, 3.0]], [[0, 1, 0, 0.5]])
    assert p.tolist() == [[8.0, 21.0, 33.0, 3.0]] and n.tolist() == [[-1.0, 0.0, 0.0, 0.5]]
    # the w words are copied bit for bit, whatever they hold
    odd = np.array([[1, 2, 3, 0]], f32)
    odd.view(np.uint32)[0, 3] = 0x7fc01234
    p, n = br.placed(pose, odd, odd)
    assert p.view(np.uint32)[0, 3] == n.view(np.uint32)[0, 3] == 0x7fc01234


def test_pose_keeps_the_sign_of_zero_as_the_float_expression_does():
    ident = frames.pose_identity()
    p, n = br.placed(ident, [[-0.0, -0.0, -0.0, 3.0]], [[-0.0, 0.0, -0.0, 0.0]])
    # x' = ((1 * -0 + 0 * -0) + 0 * -0) + 0 = ((-0 + -0) + -0) + +0 = +0: the translation's +0 wins; the normal has no such add
    assert _bits(p)[0, :3].tolist() == [0, 0, 0]
    # nx' = (1 * -0 + 0 * +0) + 0 * -0 = (-0 + +0) + -0 = +0; ny' = (0 * -0 + 1 * +0) + 0 * -0 = +0
    assert _bits(n)[0, :3].tolist() == [0, 0, 0]
    neg = np.array([[-1, 0, 0, -0.0], [0, -1, 0, -0.0], [0, 0, -1, -0.0]], f32)
    p, _ = br.placed(neg, [[0.0, 0.0, 0.0, 3.0]], [[0, 0, 0, 0]])
    # ((-1 * 0 + 0 * 0) + 0 * 0) + -0 = ((-0 + 0) + 0) + -0 = +0
    assert _bits(p)[0, :3].tolist() == [0, 0, 0]
    allneg = np.array([[-1, -1, -1, -0.0]] * 3, f32)
    p, _ = br.placed(allneg, [[0.0, 0.0, 0.0, 3.0]], [[0, 0, 0, 0]])
    assert _bits(p)[0, :3].tolist() == [0x80000000] * 3  # ((-0 + -0) + -0) + -0 = -0


def test_pose_follows_the_float32_expression_not_the_double_one():
    rng = np.random.default_rng(7)
    pose = frames.pose_compose(frames.pose_translate((0.3, -1.7, 2.9)), frames.pose_rotate((1, 2, 3), 0.7, (5.1, 3.3, 4.7)))
    ref = (rng.random((4096, 4)) * 20).astype(f32)
    nrm = rng.standard_normal((4096, 4)).astype(f32)
    p, n = br.placed(pose, ref, nrm)
    m = pose.astype(np.float64)
    dbl = (ref[:, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(f32)
    assert not scenes.bits_equal(p[:, :3], dbl) and np.abs(p[:, :3] - dbl).max() < 1e-5
    # spelled out for one member, operation by operation
    k = int(np.flatnonzero((_bits(p[:, :3]) != _bits(dbl)).any(1))[0])
    x, y, z = ref[k, :3]
    for r in range(3):
        want = f32(f32(f32(f32(pose[r, 0] * x) + f32(pose[r, 1] * y)) + f32(pose[r, 2] * z)) + pose[r, 3])
        assert _bits(want) == _bits(p[k, r])
        want_n = f32(f32(f32(pose[r, 0] * nrm[k, 0]) + f32(pose[r, 1] * nrm[k, 1])) + f32(pose[r, 2] * nrm[k, 2]))
        assert _bits(want_n) == _bits(n[k, r])
    assert scenes.bits_equal(p[:, 3], ref[:, 3]) and scenes.bits_equal(n[:, 3], nrm[:, 3])


def test_pose_helpers():
    assert frames.pose_identity().dtype == np.float32 and frames.pose_identity().tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    assert frames.pose_translate((1, 2, 3)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]]
    quarter = frames.pose_rotate((0, 0, 2), np.pi / 2)
    assert np.abs(quarter - np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]])).max() < 1e-7
    # about a point: the point stays where it is
    about = np.array([5.0, 3.0, 4.0])
    r = frames.pose_rotate((1, 1, 0), 1.1, about).astype(np.float64)
    assert np.abs(r[:, :3] @ about + r[:, 3] - about).max() < 1e-6
    assert np.abs(r[:, :3] @ r[:, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(r[:, :3]) - 1) < 1e-6
    # compose against the product of the homogeneous matrices (b first, then a), rounded once
    a, b = frames.pose_rotate((0.2, -1, 0.4), 2.3, (1, 2, 3)), frames.pose_compose(frames.pose_translate((4, 5, 6)), frames.pose_rotate((1, 0, 0), -0.4))

    def homogeneous(p):
        return np.vstack([np.asarray(p, np.float64), [0, 0, 0, 1]])
    want = (homogeneous(a) @ homogeneous(b))[:3].astype(f32)
    got = frames.pose_compose(a, b)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= 2e-6
    assert scenes.bits_equal(frames.pose_compose(frames.pose_identity(), b), b) and scenes.bits_equal(frames.pose_compose(b, frames.pose_identity()), b)
    # the schedules start at the reference placement
    assert scenes.bits_equal(frames.piston((0, 1, 0), 0.3, 40, 0), frames.pose_identity())
    assert scenes.bits_equal(frames.spin((0, 0, 1), (3, 4, 5), 0.05, 0), frames.pose_identity())
    assert scenes.bits_equal(frames.piston((0, 2, 0), 0.3, 40, 10), frames.pose_translate((0, 0.3, 0)))
    assert scenes.bits_equal(frames.spin((0, 0, 1), (3, 4, 5), 0.05, 7), frames.pose_rotate((0, 0, 1), 0.05 * 7, (3, 4, 5)))
    for bad in (lambda: frames.pose_rotate((0, 0, 0), 1.0), lambda: frames.piston((0, 0, 0), 1, 10, 1), lambda: frames.piston((0, 1, 0), 1, 0, 1)):
        with pytest.raises(ValueError):
            bad()


def _state():
    pos = np.array([[1, 1, 1, 3.0], [2, 1, 1, 1.0], [3, 1, 1, 3.0], [4, 1, 1, 3.5], [5, 1, 1, 2.1], [6, 1, 1, 3.0], [7, 1, 1, 3.0]], f32)
    vel = np.array([[0, 1, 0, 0], [9, 9, 9, 0], [1, 0, 0, 0], [0, 0, 1, 0], [8, 8, 8, 0], [0, -1, 0, 0], [-1, 0, 0, 0.25]], f32)
    return pos, vel


def test_definition_by_hand():
    pos, vel = _state()
    assert br.region_members(pos).tolist() == [0, 2, 3, 5, 6]  # (int)3.5 == 3
    assert br.region_members(pos, (3, 0, 0, 6, 2, 2)).tolist() == [2, 3]  # half open: x = 3 is in, x = 6 (id 5) is out
    ids, rp, rn = br.define(pos, vel, [5, 0, 3])
    assert ids.dtype == np.uint32 and ids.tolist() == [5, 0, 3] and scenes.bits_equal(rp, pos[[5, 0, 3]]) and scenes.bits_equal(rn, vel[[5, 0, 3]])
    assert br.id_offenders(pos, [5, 0, 3]) == (0, -1)
    assert br.id_offenders(pos, [5, 1, 3]) == (1, 1)            # liquid
    assert br.id_offenders(pos, [5, 0, 7]) == (1, 2)            # id >= N
    assert br.id_offenders(pos, [5, 0, 3, 0]) == (2, 1)         # every occurrence of a repeated id counts
    assert br.id_offenders(pos, [4, 0, 0, 0, 9]) == (5, 0)
    for bad in ([], [1], [0, 0], [7]):
        with pytest.raises(br.Refused):
            br.define(pos, vel, bad)
    with pytest.raises(br.Refused):
        br.region_members(pos, (0, 0, np.nan, 1, 1, 1))


def test_set_pose_validation_and_max_move_by_hand():
    pos, vel = _state()
    body = br.define(pos, vel, [6, 2, 0])
    cfg = _cfg(wide=True)
    r0 = f32(cfg.r0)
    shift = frames.pose_translate((0, 0.5, 0))
    p, v, move = br.set_pose(cfg, pos, vel, body, shift)
    assert p[[6, 2, 0], 1].tolist() == [1.5] * 3 and scenes.bits_equal(v, vel)
    assert scenes.bits_equal(p[[1, 3, 4, 5]], pos[[1, 3, 4, 5]])
    assert move.dtype == np.float32 and _bits(move) == _bits(np.sqrt(f32(0.25)) / r0)
    # applied to the REFERENCE placement: the same pose again moves nothing
    p2, v2, move2 = br.set_pose(cfg, p, v, body, shift)
    assert scenes.bits_equal(p2, p) and move2 == 0
    # wide cell ids: the box is [0, xmax]; members 0 (x = 7) and 1 (x = 3) leave it, member 2 (x = 1) stays
    out = frames.pose_translate((float(cfg.xmax) - 2.5, 0, 0))
    with pytest.raises(br.Refused) as ei:
        br.set_pose(cfg, pos, vel, body, out)
    assert (ei.value.offenders, ei.value.lowest_member) == (2, 0)
    assert br.pose_offenders(cfg, br.placed(out, body[1], body[2])[0]) == (2, 0)
    # reference cell ids: out-of-box positions alias, as in sph_create; only non-finite ones fail
    br.set_pose(_cfg(wide=False), pos, vel, body, out)
    huge = frames.pose_translate((3e38, 0, 0))
    huge[0, 0] = f32(3e38)
    with pytest.raises(br.Refused) as ei:
        br.set_pose(_cfg(wide=False), pos, vel, body, huge)
    assert ei.value.offenders == 3 and ei.value.lowest_member == 0
    for word in (np.nan, np.inf, -np.inf):
        bad = shift.copy()
        bad[1, 2] = word
        with pytest.raises(br.Refused):
            br.set_pose(cfg, pos, vel, body, bad)


def test_remap_by_hand():
    pos, vel = _state()
    body = br.define(pos, vel, [6, 2, 0, 5])
    _, _, m = er.remove(pos, vel, er.id_marks(7, [1, 2, 4]))
    assert m.tolist() == [0, -1, -1, 1, -1, 2, 3]
    ids, rp, rn = br.follow_removal(body, m)
    assert ids.tolist() == [3, 0, 2] and scenes.bits_equal(rp, pos[[6, 0, 5]]) and scenes.bits_equal(rn, vel[[6, 0, 5]])
    assert br.follow_removal(br.define(pos, vel, [2]), m) is None
    same = br.follow_removal(body, np.arange(7))
    assert same[0].tolist() == [6, 2, 0, 5] and scenes.bits_equal(same[1], body[1])


def test_binding_lists_the_body_calls():
    names = ["sph_body_define_ids", "sph_body_define_region", "sph_body_release", "sph_body_count", "sph_body_read", "sph_body_set_pose"]
    lib = ctypes.CDLL(sphmi.LIB_PATH)
    txt = open(scenes.ROOT + "/include/sphmi.h").read()
    for n in names:
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    for m in ("body_define_ids", "body_define_region", "body_release", "body_count", "body_read", "body_set_pose"):
        assert callable(getattr(sphmi.owHIPSolver, m))
    assert "#define SPH_MAX_BODIES %d" % sphmi.MAX_BODIES in txt


def test_premise_a_moved_wall_reaches_the_liquid():
    """tiny, 3 steps; then 3 times: lift the floor of the read-back by the restatement (1.2 r0 at once, 0.25 r0 more per step),
    create a new oracle from the arrays and step it once. After each such step at least one liquid particle differs bitwise from
    the run whose floor was left alone, and nothing but the body's rows was moved."""
    K, M = 3, 3
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    N, r0 = cfg.particleCount, f32(cfg.r0)
    still = scenes.oracle_for(sc)
    for _ in range(K):
        still.step()

    def state(o):
        return o.buffer("position").reshape(-1, 4)[:N].copy(), o.buffer("velocity").reshape(-1, 4)[:N].copy()
    pos, vel = state(still)
    liquid = pos[:, 3].astype(np.int32) == 1
    floor = (-np.inf, -np.inf, -np.inf, np.inf, r0, np.inf)  # the shell's bottom layer lies at y = 0.5 r0
    body = br.define(pos, vel, br.region_members(pos, floor))
    assert 0 < body[0].size < (~liquid).sum()
    from oracle import oraclebind as O
    for k in range(M):
        pose = frames.pose_translate((0.0, float(r0) * (1.2 + 0.25 * k), 0.0))
        moved_pos, moved_vel, move = br.set_pose(cfg, pos, vel, body, pose)
        others = np.ones(N, bool)
        others[body[0]] = False
        assert scenes.bits_equal(moved_pos[others], pos[others]) and scenes.bits_equal(moved_vel, vel) and move > 0
        moved = O.OracleSolver(sphmi.config_dict(cfg), moved_pos, moved_vel, threads=4)
        moved.step()
        still.step()
        pos, vel = state(moved)
        ref_pos, _ = state(still)
        assert np.isfinite(pos).all() and np.isfinite(vel).all()
        assert scenes.bits_equal(pos[body[0]], moved_pos[body[0]]), "the step moved a wall"
        differ = (_bits(pos[liquid]) != _bits(ref_pos[liquid])).any(1).sum()
        assert differ > 0, "step %d: the lifted floor did not reach the liquid" % k
        moved.close()
    still.close()
