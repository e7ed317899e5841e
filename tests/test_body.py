"""GPU tests of the kinematic bodies (sph_body_define_ids / sph_body_define_region / sph_body_release / sph_body_count /
sph_body_read / sph_body_set_pose, include/sphmi.h): definitions, poses and the tunnelling number equal to the numpy restatement
(tests/body_ref.py); a solver whose wall was moved in place continues bit for bit like a solver newly created from the restated
arrays and like the C oracle created from them; the analysis state survives a pose; member-count, block and scan edges; refusals
leave everything as it was; removals carry the bodies; the calling rules; the driver's flags. No tolerance appears anywhere:
integers are compared for equality, floats as bit patterns."""
import os
import re
import subprocess

import numpy as np
import pytest

import body_ref as br
import edit_ref as er
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import error_status as _status, staged_step

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_ORDER = -1, -3
f32 = np.float32
INF = np.inf
ROOM = 1024


def _hip(sc, cfg, pos, vel):
    return sphmi.owHIPSolver(cfg, pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"])


def read_state(hip):
    return hip.read_position_buffer(), hip.read_velocity_buffer()


def assert_state(hip, pos, vel, what):
    gp, gv = read_state(hip)
    assert scenes.bits_equal(gp, pos), "%s: position: %s" % (what, scenes.diff_report(gp, pos))
    assert scenes.bits_equal(gv, vel), "%s: velocity: %s" % (what, scenes.diff_report(gv, vel))


def assert_body(hip, slot, body, what):
    ids, rp, rn = hip.body_read(slot)
    assert hip.body_count(slot) == body[0].size == ids.size, what
    assert ids.dtype == np.uint32 and np.array_equal(ids, body[0]), what + ": ids"
    assert scenes.bits_equal(rp, body[1]) and scenes.bits_equal(rn, body[2]), what + ": reference rows"


def pose_and_check(hip, cfg, slot, body, pose, pos, vel, what):
    """One pose on the solver and on the restatement: the tunnelling number has equal bits, and so has the whole state."""
    pos, vel, want = br.set_pose(cfg, pos, vel, body, pose)
    got = hip.body_set_pose(slot, pose)
    assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), "%s: max_move %r, restated %r" % (what, got, want)
    assert_state(hip, pos, vel, what)
    return pos, vel


def general_poses(cfg):
    r0 = float(cfg.r0)
    mid = (0.5 * (cfg.xmin + cfg.xmax), 0.5 * (cfg.ymin + cfg.ymax), 0.5 * (cfg.zmin + cfg.zmax))
    return [("identity", frames.pose_identity()),
            ("translation", frames.pose_translate((0.3 * r0, -0.2 * r0, 0.45 * r0))),
            ("quarter turn", frames.pose_rotate((0, 0, 1), np.pi / 2, mid)),
            ("general", frames.pose_compose(frames.pose_translate((0.1 * r0, 0.2 * r0, -0.3 * r0)),
                                            frames.pose_rotate((0.3, -1.0, 0.5), 0.37, (mid[0] + 2 * r0, mid[1] - r0, mid[2] + 3 * r0))))]


def refused(hip, status, call, pos, vel, what):
    with pytest.raises(sphmi.SphError) as ei:
        call()
    assert _status(ei) == status, "%s: %s" % (what, ei.value)
    assert_state(hip, pos, vel, what + ": the state after the refusal")
    return ei.value


# ---------------------------------------------------------------------------------------------- poses against the restatement
@pytest.fixture(scope="module")
def tiny():
    """tiny after one step, with room to grow; tests that change the state put it back or make their own solver."""
    sc = scenes.SCENES["tiny"]()
    n = sc["cfg"].particleCount
    hip = sphmi.owHIPSolver(er.with_count(sc["cfg"], n, n + ROOM), sc["position"], sc["velocity"])
    hip.step(0)
    yield sc, hip
    hip.close()


@pytest.mark.parametrize("kind", ["region", "ids"])
def test_pose_equals_restatement(tiny, kind):
    sc, hip = tiny
    cfg = sc["cfg"]
    pos, vel = read_state(hip)
    r0 = f32(cfg.r0)
    if kind == "region":  # the wall at x = xmax
        box = (f32(cfg.xmax) - r0, -INF, -INF, INF, INF, INF)
        want = br.region_members(pos, box)
        assert hip.body_define_region(0, box) == want.size and 0 < want.size < (pos[:, 3].astype(np.int32) == 3).sum()
    else:  # a shuffled third of the shell
        shell = br.region_members(pos)
        want = np.random.default_rng(5).permutation(shell)[:shell.size // 3]
        assert not np.array_equal(want, np.sort(want))
        assert hip.body_define_ids(0, want) == want.size
    body = br.define(pos, vel, want)
    assert_body(hip, 0, body, kind)
    members = np.zeros(pos.shape[0], bool)
    members[body[0]] = True
    p, v = pos, vel
    for name, pose in general_poses(cfg):
        p, v = pose_and_check(hip, cfg, 0, body, pose, p, v, "%s, %s" % (kind, name))
        assert scenes.bits_equal(p[~members], pos[~members]) and scenes.bits_equal(v[~members], vel[~members])
        assert_body(hip, 0, body, "the reference placement after " + name)
    assert not scenes.bits_equal(v[members], vel[members])  # the normals turned
    p, v = pose_and_check(hip, cfg, 0, body, frames.pose_identity(), p, v, "back to the reference placement")
    assert np.array_equal(p, pos) and np.array_equal(v, vel)  # (as numbers: 1 * -0 + 0 * x is +0)
    hip.body_release(0)
    assert hip.body_count(0) == 0 and hip.body_read(0)[0].size == 0


# ---------------------------------------------------------------------------------------------- continuation
def _plate(pos, cfg, wide):
    """A 5 x 1 x 6 plate of boundary particles, normal -y, 1.5 r0 above the liquid's top: (origin, spacing, dims)."""
    r0 = f32(cfg.r0)
    liq = pos[pos[:, 3].astype(np.int32) == 1]
    lo = liq[:, :3].min(0)
    origin = (lo[0] + f32(2) * r0, liq[:, 1].max() + f32(1.5) * r0, lo[2] + f32(2) * r0)
    return origin, (r0, r0, r0), (5, 1, 6)


@pytest.mark.parametrize("name", ["tiny_jitter", "wide", "tiny_elastic"])
def test_continuation_equals_fresh_solver_and_oracle(name):
    """3 steps, a plate emitted above the liquid and made a body, then 4 times: a pose (a push of 0.25 r0 per step into the liquid;
    on `wide` a blade that turns by 0.1 rad per step about its middle), then one step on the moved solver (stage by stage for
    tiny_jitter), on a solver created with capacity 0 from the restated arrays and on the oracle created from them."""
    from oracle import oraclebind as O
    sc = scenes.SCENES[name]()
    cfg0 = sc["cfg"]
    n0, r0 = cfg0.particleCount, f32(cfg0.r0)
    hip = _hip(sc, er.with_count(cfg0, n0, n0 + ROOM), sc["position"], sc["velocity"])
    for it in range(3):
        hip.step(it)
    pos, vel = read_state(hip)
    origin, spacing, dims = _plate(pos, cfg0, name == "wide")
    lp, lv = er.lattice(origin, spacing, dims, velocity=(0.0, -1.0, 0.0), type_value=3.0)
    pos, vel = er.append(pos, vel, lp, lv, cfg0)
    assert hip.emit_lattice(origin, spacing, dims, velocity=(0.0, -1.0, 0.0), type_value=3.0) == 30
    N = pos.shape[0]
    plate = np.arange(N - 30, N, dtype=np.uint32)
    box = tuple(np.asarray(origin, f32) - f32(0.5) * r0) + tuple(lp[:, :3].max(0) + f32(0.5) * r0)
    assert hip.body_define_region(3, box) == 30
    body = br.define(pos, vel, plate)
    assert_body(hip, 3, body, "the plate")
    cfg = er.with_count(cfg0, N, 0)
    centre = lp[:, :3].astype(np.float64).mean(0)
    fresh = None
    for k in range(1, 5):
        if name == "wide":
            pose = frames.spin((0, 0, 1), centre, 0.1, k)
        else:
            pose = frames.pose_translate((0.0, -0.25 * float(r0) * k, 0.0))
        pos, vel = pose_and_check(hip, cfg0, 3, body, pose, pos, vel, "%s, pose %d" % (name, k))
        if fresh is not None:
            fresh.close()
        fresh = _hip(sc, cfg, pos, vel)
        ora = O.OracleSolver(sphmi.config_dict(cfg), pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"], threads=4)
        it = 2 + k
        staged_step(hip, it) if name == "tiny_jitter" else hip.step(it)
        fresh.step(it)
        ora.step()
        pos, vel = read_state(hip)
        for a, b, c, what in ((pos, fresh.read_position_buffer(), ora.buffer("position").reshape(-1, 4)[:N], "position"),
                              (vel, fresh.read_velocity_buffer(), ora.buffer("velocity").reshape(-1, 4)[:N], "velocity"),
                              (hip.read_density_buffer(), fresh.read_density_buffer(), ora.buffer("rho")[:N], "rho")):
            assert scenes.bits_equal(a, b), "%s step %d, %s, moved vs fresh: %s" % (name, k, what, scenes.diff_report(a, b))
            assert scenes.bits_equal(a, c), "%s step %d, %s, moved vs oracle: %s" % (name, k, what, scenes.diff_report(a, c))
        ora.close()
    assert np.isfinite(pos).all()
    # the analysis calls agree with the fresh solver's
    box = er.liquid_quantile_box(pos, 0.2, 0.8)
    regions = [(-INF,) * 3 + (INF,) * 3, tuple(box)]
    assert scenes.bits_equal(hip.diagnostics(regions, (1, 2, 3)), fresh.diagnostics(regions, (1, 2, 3)))
    n1, n2 = hip.select(box, (1,), (("density", 0.0, INF),)), fresh.select(box, (1,), (("density", 0.0, INF),))
    assert n1 == n2 and n1 > 0
    for a, b in zip(hip.selection(), fresh.selection()):
        assert scenes.bits_equal(a, b)
    hip.close(); fresh.close()


# ---------------------------------------------------------------------------------------------- the analysis state survives
def test_analysis_state_survives_a_pose():
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    pos, vel = read_state(hip)
    r0 = f32(cfg.r0)
    box = er.liquid_quantile_box(pos, 0.1, 0.9)
    assert hip.select(box, (1,), (("density", 0.0, INF),)) > 0
    sel = hip.selection()
    assert hip.label_components()[1] > 0
    comp = hip.components()
    values = np.random.default_rng(3).random(hip.N, np.float32)
    hip.field_create(1, values)
    assert hip.field_set_region(1, 2.5, box, (1,)) > 0
    dye = hip.field_read(1)
    diag = hip.diagnostics()
    hip.tracers_set([(8 * r0, 6 * r0, 8 * r0)])
    floor = (-INF, -INF, -INF, INF, r0, INF)
    body = br.define(pos, vel, br.region_members(pos, floor))
    assert hip.body_define_region(0, floor) == body[0].size
    pose_and_check(hip, cfg, 0, body, frames.pose_translate((0, 0.3 * float(r0), 0)), pos, vel, "the floor lifted")
    for a, b in zip(hip.selection(), sel):
        assert scenes.bits_equal(a, b)
    for a, b in zip(hip.components(), comp):
        assert scenes.bits_equal(a, b)
    assert scenes.bits_equal(hip.field_read(1), dye) and scenes.bits_equal(hip.diagnostics(), diag)
    assert hip.tracers()[0].shape[0] == 1
    assert hip.component_diagnostics([0]).shape[0] == 1 and hip.field_set_selection(1, 0.5) == sel[0].size
    hip.step(2)
    assert np.isfinite(hip.read_position_buffer()).all()
    hip.close()


# ---------------------------------------------------------------------------------------------- member counts, blocks, the scan
def test_member_count_edges(tiny):
    sc, hip = tiny
    cfg = sc["cfg"]
    pos, vel = read_state(hip)
    shell = br.region_members(pos)
    pose = general_poses(cfg)[3][1]
    for n in (1, 63, 64, 65, 255, 256, 257):
        for ids in (shell[7:7 + n], shell[7:7 + n][::-1]):
            assert hip.body_define_ids(5, ids) == n
            body = br.define(pos, vel, ids)
            assert_body(hip, 5, body, "%d members" % n)
            p, v = pose_and_check(hip, cfg, 5, body, pose, pos, vel, "%d members" % n)
            pos, vel = pose_and_check(hip, cfg, 5, body, frames.pose_identity(), p, v, "%d members, back" % n)
    hip.body_release(5)


@pytest.fixture(scope="module")
def wide():
    sc = scenes.SCENES["wide"]()
    hip = scenes.hip_for(sc)
    hip.step(0)
    yield sc, hip
    hip.close()


def test_whole_shell_is_one_body(wide):
    """102,408 members: 401 blocks of the pose kernels, the scan of the region definition over 410 blocks."""
    sc, hip = wide
    cfg = sc["cfg"]
    pos, vel = read_state(hip)
    shell = br.region_members(pos)
    assert shell.size > 4096
    r0 = float(cfg.r0)
    pose = frames.pose_translate((0.25 * r0, -0.125 * r0, 0.2 * r0))
    assert hip.body_define_region(1, None) == shell.size
    for ids, what in ((shell, "ascending"), (shell[::-1], "reversed")):
        if what == "reversed":
            assert hip.body_define_ids(1, ids) == shell.size
        body = br.define(pos, vel, ids)
        assert_body(hip, 1, body, what)
        p, v = pose_and_check(hip, cfg, 1, body, pose, pos, vel, "the whole shell, " + what)
        pos, vel = pose_and_check(hip, cfg, 1, body, frames.pose_identity(), p, v, "the whole shell back, " + what)
    hip.body_release(1)


# ---------------------------------------------------------------------------------------------- all or nothing
def test_pose_is_all_or_nothing(wide):
    sc, hip = wide
    cfg = sc["cfg"]
    pos, vel = read_state(hip)
    r0 = f32(cfg.r0)
    box = (f32(cfg.xmax) - f32(3) * r0, -INF, -INF, INF, INF, INF)  # the wall at x = xmax and the rows of the others next to it
    body = br.define(pos, vel, br.region_members(pos, box))
    assert hip.body_define_region(2, box) == body[0].size
    out = frames.pose_translate((float(r0), 0, 0))
    with pytest.raises(br.Refused) as want:
        br.set_pose(cfg, pos, vel, body, out)
    assert 0 < want.value.offenders < body[0].size
    e = refused(hip, ERR_INVALID, lambda: hip.body_set_pose(2, out), pos, vel, "partly out of the box")
    assert (e.offenders, e.lowest_member) == (want.value.offenders, want.value.lowest_member)
    assert "%d of %d members" % (e.offenders, body[0].size) in str(e) and "member %d;" % e.lowest_member in str(e)
    for k, word in ((0, np.nan), (7, np.inf), (11, -np.inf)):
        bad = frames.pose_identity().reshape(-1)
        bad[k] = word
        refused(hip, ERR_INVALID, lambda: hip.body_set_pose(2, bad), pos, vel, "pose word %d = %r" % (k, word))
    assert_body(hip, 2, body, "after the refusals")
    p, v = pose_and_check(hip, cfg, 2, body, frames.pose_translate((-0.25 * float(r0), 0, 0)), pos, vel, "still usable")
    pose_and_check(hip, cfg, 2, body, frames.pose_identity(), p, v, "back")
    hip.body_release(2)


# ---------------------------------------------------------------------------------------------- definition refusals
def test_definition_refusals_leave_the_slot_alone(tiny):
    sc, hip = tiny
    pos, vel = read_state(hip)
    N = pos.shape[0]
    shell = br.region_members(pos)
    liquid = int(np.flatnonzero(pos[:, 3].astype(np.int32) == 1)[3])
    keep = br.define(pos, vel, shell[10:40][::-1])
    assert hip.body_define_ids(2, keep[0]) == 30

    def entries(e):
        m = re.search(r"(\d+) of (\d+) entries .* the lowest is entry (\d+)", str(e))
        return int(m.group(1)), int(m.group(3))
    for ids, what in (([shell[0], liquid, shell[1]], "a liquid id"), ([shell[0], shell[1], N], "an id >= N"),
                      ([shell[4], shell[2], shell[4], shell[3]], "a duplicate"), ([N + 5, shell[2], liquid, shell[2]], "all three")):
        e = refused(hip, ERR_INVALID, lambda: hip.body_define_ids(2, ids), pos, vel, what)
        assert entries(e) == br.id_offenders(pos, ids), what
        assert_body(hip, 2, keep, what)
    refused(hip, ERR_INVALID, lambda: hip.body_define_ids(2, []), pos, vel, "count 0")
    refused(hip, ERR_INVALID, lambda: hip.body_define_ids(2, np.concatenate([shell, shell, shell[:N]])[:N + 1]), pos, vel, "count > N")
    nothing = (f32(8) * f32(sc["cfg"].r0),) * 3 + (f32(9) * f32(sc["cfg"].r0),) * 3  # in the liquid
    assert br.region_members(pos, nothing).size == 0
    refused(hip, ERR_INVALID, lambda: hip.body_define_region(2, nothing), pos, vel, "an empty region")
    refused(hip, ERR_INVALID, lambda: hip.body_define_region(2, (0, 0, np.nan, 1, 1, 1)), pos, vel, "a NaN bound")
    assert_body(hip, 2, keep, "after the refused definitions")
    for slot in (-1, sphmi.MAX_BODIES):
        for call in (lambda: hip.body_define_ids(slot, shell[:3]), lambda: hip.body_define_region(slot, None), lambda: hip.body_count(slot),
                     lambda: hip.body_read(slot), lambda: hip.body_release(slot), lambda: hip.body_set_pose(slot, frames.pose_identity())):
            refused(hip, ERR_INVALID, call, pos, vel, "slot %d" % slot)
    refused(hip, ERR_ORDER, lambda: hip.body_set_pose(9, frames.pose_identity()), pos, vel, "a free slot")
    assert_body(hip, 2, keep, "at the end")
    # a slot in use is redefined by a definition that succeeds
    assert hip.body_define_ids(2, shell[50:53]) == 3
    assert_body(hip, 2, br.define(pos, vel, shell[50:53]), "redefined")
    hip.body_release(2)


# ---------------------------------------------------------------------------------------------- edits carry the bodies
def test_edits_carry_the_bodies():
    sc = scenes.SCENES["tiny"]()
    cfg0 = sc["cfg"]
    n, r0 = cfg0.particleCount, f32(cfg0.r0)
    hip = sphmi.owHIPSolver(er.with_count(cfg0, n, n + ROOM), sc["position"], sc["velocity"])
    hip.step(0)
    pos, vel = read_state(hip)
    shell = br.region_members(pos)
    corner = (-INF, -INF, -INF, f32(6) * r0, INF, INF)  # liquid (the lowest ids) and wall particles with x < 6 r0
    gone = er.region_marks(pos, corner, (1, 3))
    assert 0 < (gone & (pos[:, 3].astype(np.int32) == 1)).sum() and 0 < gone[shell].sum() < shell.size
    mixed = np.random.default_rng(11).permutation(shell)[:700]
    assert 0 < gone[mixed].sum() < mixed.size
    doomed = shell[gone[shell]][:5]
    bodies = {0: br.define(pos, vel, mixed), 4: br.define(pos, vel, doomed), 15: br.define(pos, vel, shell[~gone[shell]][:257])}
    for slot, b in bodies.items():
        assert hip.body_define_ids(slot, b[0]) == b[0].size
    pos, vel, m = er.remove(pos, vel, gone)
    assert hip.remove_region(corner, (1, 3)) == gone.sum() and np.array_equal(hip.edit_map(), m)
    assert_state(hip, pos, vel, "the removal")
    assert m[shell[~gone[shell]]].min() < shell[~gone[shell]].min()  # every surviving id shifted
    bodies = {slot: br.follow_removal(b, m) for slot, b in bodies.items()}
    assert bodies[4] is None and hip.body_count(4) == 0 and hip.body_read(4)[0].size == 0
    for slot in (0, 15):
        assert_body(hip, slot, bodies[slot], "body %d through the edit map" % slot)
    assert bodies[0][0].size == mixed.size - gone[mixed].sum() and bodies[15][0].size == 257
    pose = general_poses(cfg0)[3][1]
    p, v = pose_and_check(hip, cfg0, 0, bodies[0], pose, pos, vel, "a pose on the new arrays")
    pos, vel = pose_and_check(hip, cfg0, 0, bodies[0], frames.pose_identity(), p, v, "back")
    # additions and an empty removal leave the bodies alone
    ap, av = er.hand_made_particles(cfg0, (f32(8) * r0, f32(13) * r0, f32(8) * r0))
    hip.add_particles(ap, av)
    assert hip.emit_lattice((f32(8) * r0, f32(12) * r0, f32(3) * r0), (r0, r0, r0), (2, 1, 2)) == 4
    assert hip.remove_ids([]) == 0 and hip.remove_region((0, 0, 0, 0, 0, 0), (1,)) == 0
    assert hip.remove_region(None, (1,), count_only=True) > 0
    for slot in (0, 15):
        assert_body(hip, slot, bodies[slot], "body %d after additions and an empty removal" % slot)
    hip.step(1)
    assert np.isfinite(hip.read_position_buffer()).all()
    hip.close()


# ---------------------------------------------------------------------------------------------- calling rules
def test_slab_solver_is_refused():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    n = sc["cfg"].particleCount
    hip = sphmi.owHIPSolver(sc["cfg"], sc["position"], sc["velocity"])
    lay = S.particle_layers(sc["position"], sc["cfg"])
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    pos, vel, _, _ = hip.slab_read()
    for call in (lambda: hip.body_define_region(0, None), lambda: hip.body_define_ids(0, [n - 1]), lambda: hip.body_count(0),
                 lambda: hip.body_read(0), lambda: hip.body_release(0), lambda: hip.body_set_pose(0, frames.pose_identity())):
        with pytest.raises(sphmi.SphError) as ei:
            call()
        assert _status(ei) == ERR_INVALID
        p, v, _, _ = hip.slab_read()
        assert scenes.bits_equal(p, pos) and scenes.bits_equal(v, vel)
    hip.close()


def test_refused_while_a_staged_step_is_half_done():
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    hip.step(0)
    pos, vel = read_state(hip)
    floor = (-INF, -INF, -INF, INF, f32(cfg.r0), INF)
    body = br.define(pos, vel, br.region_members(pos, floor))
    assert hip.body_define_region(0, floor) == body[0].size
    pose = frames.pose_translate((0, 0.2 * float(cfg.r0), 0))
    calls = (lambda: hip.body_set_pose(0, pose), lambda: hip.body_define_region(1, floor), lambda: hip.body_define_ids(1, body[0]),
             lambda: hip.body_release(0), lambda: hip.body_count(0), lambda: hip.body_read(0))
    for st in scenes.STAGE_SEQUENCE:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
        if st in ("hashParticles", "findNeighbors", "computePressureForceAcceleration"):
            for call in calls:
                with pytest.raises(sphmi.SphError) as ei:
                    call()
                assert _status(ei) == ERR_ORDER, st
        if st == "integrate":  # accepted from here on, also between the membrane stages of a solver without elastic matter
            pos, vel = read_state(hip)
            pos, vel = pose_and_check(hip, cfg, 0, body, pose, pos, vel, "after integrate")
    assert hip.body_count(0) == body[0].size and hip.body_count(1) == 0
    assert_state(hip, pos, vel, "after the step's last stage")
    hip.step(2)
    pose_and_check(hip, cfg, 0, body, frames.pose_identity(), *read_state(hip), "after a fused step")
    hip.close()


def test_pose_while_an_asynchronous_read_back_is_outstanding():
    """The reader gets the positions of before the pose; the state holds the pose."""
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    hip.step(0)
    pos, vel = read_state(hip)
    floor = (-INF, -INF, -INF, INF, f32(cfg.r0), INF)
    body = br.define(pos, vel, br.region_members(pos, floor))
    assert hip.body_define_region(0, floor) == body[0].size
    guard = 64
    raw = np.full((n + guard) * 4 + 3, f32(-7.0), f32)[3:]  # (odd offset: not page-aligned)
    out = raw[:4 * n]
    hip.read_position_buffer_async(out)
    pose = frames.pose_translate((0, 0.25 * float(cfg.r0), 0))
    want_p, want_v, want_move = br.set_pose(cfg, pos, vel, body, pose)
    assert np.float32(hip.body_set_pose(0, pose)).view(np.uint32) == np.float32(want_move).view(np.uint32)
    hip.wait_position_buffer()
    assert scenes.bits_equal(out.reshape(-1, 4), pos) and not scenes.bits_equal(pos, want_p)
    assert (raw[4 * n:] == f32(-7.0)).all(), "written past the requested bytes"
    assert_state(hip, want_p, want_v, "the pose")
    hip.step(1)
    assert np.isfinite(hip.read_position_buffer()).all()
    hip._L.sph_host_unregister(hip._h, out.ctypes.data)
    hip.close()


# ---------------------------------------------------------------------------------------------- driver
def test_driver_moves_a_wall(tmp_path):
    """sphmi_run --body-region --body-velocity --body-from --body-until: the `_body:` lines and the final positions equal the
    Python replay of the schedule."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12))
    cfg = sc["cfg"]
    r0 = f32(cfg.r0)
    floor = [-INF, -INF, -INF, INF, float(r0), INF]
    v = [0.0, 0.25 * float(r0), 0.01 * float(r0)]
    out = str(tmp_path / "final.bin")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    r = subprocess.run([exe] + box + ["--steps", "6", "--quiet", "--body-region"] + ["%.9g" % x for x in floor] + ["--body-velocity"] +
                       ["%.17g" % x for x in v] + ["--body-from", "1", "--body-until", "5", "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [re.match(r"_body: step (\d+) members (\d+) max_move (\S+)$", l).groups() for l in r.stdout.splitlines() if l.startswith("_body:")]
    hip = scenes.hip_for(sc)
    members = hip.body_define_region(0, [f32(x) for x in floor])
    want = []
    for step in range(6):
        if 1 <= step < 5:
            move = hip.body_set_pose(0, frames.pose_translate(np.array(v, np.float64) * float(step - 1 + 1)))
            want.append((str(step), str(members), "%.9g" % float(move)))
        hip.step(step)
    assert lines == want and len(want) == 4 and members > 0 and all(float(w[2]) > 0 for w in want)
    final = np.fromfile(out, f32).reshape(-1, 4)
    assert final.shape[0] == hip.N and scenes.bits_equal(final, hip.read_position_buffer())
    hip.close()
    # misuse exits with status 2 and a message
    for bad in (["--body-velocity", "0", "1", "0"], ["--body-from", "2"], ["--body-region", "0", "0", "nan", "1", "1", "1"],
                ["--body-region", "0", "0", "0", "1", "1", "1", "--body-velocity", "0", "inf", "0"],
                ["--body-region", "0", "0", "0", "1", "1", "1", "--body-spin", "0", "0", "0", "1", "1", "1", "0.1"]):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
