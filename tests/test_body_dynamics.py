"""GPU tests of the free bodies (sph_body_set_dynamics / sph_body_get_dynamics / sph_bodies_advance, include/sphmi.h): the loads of
an advance against sph_wall_diagnostics on the same state and against tests/wall_ref.py; every record word, the live state and the
placed particles against the restatement tests/body_dyn_ref.py; the device route against the host loop it replaces
(wall_diagnostics -> restatement -> body_set_pose) step after step, and against a fresh solver and the oracle created from the
moved arrays, in every step mode; rotation, locks, refusal, member counts, the tree on more than 2^20 particles, rows without a
16-bit copy, elastic matter, edits, the calling rules and the driver. Numbers are compared for equality (the sign of a zero total
is not part of the contract), particle arrays as bit patterns. No tolerance appears anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

import body_dyn_ref as bd
import body_ref as br
import diag_ref
import edit_ref as er
import forces_ref as fr
import scenes
import sphmi
import wall_cases
import wall_ref as wr
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER, ERR_INVALID = -3, -1
f32 = np.float32
INF = np.inf
A, B, C3 = wall_cases.SLOT_A, wall_cases.SLOT_B, 7
EVERYTHING = np.array([diag_ref.EVERYTHING], np.float32)
ALL_TYPES = (1, 2, 3)


def read_state(hip):
    return hip.read_position_buffer(), hip.read_velocity_buffer()


def assert_state(hip, pos, vel, what):
    gp, gv = read_state(hip)
    assert scenes.bits_equal(gp, pos), "%s: position: %s" % (what, scenes.diff_report(gp, pos))
    assert scenes.bits_equal(gv, vel), "%s: velocity: %s" % (what, scenes.diff_report(gv, vel))


def same_numbers(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def mass_state(cfg, ref_pos, pose=None, com_shift=(0, 0, 0), **kw):
    """A state for a body of equal point masses of cfg.mass at ref_pos (reference placement) standing at `pose` (a translation)."""
    m = ref_pos.shape[0] * float(f32(cfg.mass))
    com, _, jinv = frames.body_mass_properties(ref_pos, m)
    com = com + np.asarray(com_shift, np.float64)
    t = np.zeros(3) if pose is None else np.asarray(pose, np.float64).reshape(3, 4)[:, 3]
    kw.setdefault("gravity", (cfg.gravity_x, cfg.gravity_y, cfg.gravity_z))
    return bd.make_state(m, com=com, position=com + t, inertiaInv=jinv, **kw)


def set_dynamics(hip, slot, state):
    hip.body_set_dynamics(slot, **state)
    got = hip.body_dynamics(slot)
    for k, v in state.items():
        assert same_numbers(got[k], v), (slot, k, got[k], v)


def load_records(hip, slots):
    return {s: hip.wall_diagnostics(s, EVERYTHING, ALL_TYPES)[0] for s in slots}


class Bodies:
    """The restated side of a solver's dynamic bodies: {slot: body}, {slot: state}, {slot: advances}, and the arrays."""

    def __init__(self, hip, cfg):
        self.hip, self.cfg = hip, cfg
        self.body, self.state, self.advances = {}, {}, {}
        self.pos, self.vel = read_state(hip)

    def add(self, slot, state):
        ids, rp, rn = self.hip.body_read(slot)
        self.body[slot] = (ids.copy(), rp.copy(), rn.copy())
        self.state[slot], self.advances[slot] = state, 0
        set_dynamics(self.hip, slot, state)

    def advance_and_check(self, what):
        """One advance on the device against: sph_wall_diagnostics just before it, the restatement, the live state, the arrays."""
        hip = self.hip
        D = load_records(hip, self.state)
        rec = hip.bodies_advance()
        assert rec.shape == (sphmi.MAX_BODIES, 48) and rec.dtype == np.float64
        for slot in range(sphmi.MAX_BODIES):
            if slot not in self.state:
                assert rec[slot, 0] == -1 and not rec[slot, 1:].any(), (what, slot)
                continue
            self.state[slot], self.advances[slot], want, self.pos, self.vel = bd.advance_body(
                self.cfg, D[slot], self.state[slot], self.advances[slot], self.body[slot], self.pos, self.vel)
            bad = np.flatnonzero(~((rec[slot] == want) | (np.isnan(rec[slot]) & np.isnan(want))))
            assert bad.size == 0, "%s, slot %d: record words %s: %r vs restated %r" % (what, slot, bad.tolist(), rec[slot, bad], want[bad])
            assert rec[slot, 26] == D[slot][1] and rec[slot, 27] == D[slot][2]
            got = hip.body_dynamics(slot)
            for k, v in self.state[slot].items():
                assert same_numbers(got[k], v), "%s, slot %d: live %s %r vs %r" % (what, slot, k, got[k], v)
        assert_state(hip, self.pos, self.vel, what)
        return rec


def lifted_solver(name, setup=None, staged=False):
    """`name` of wall_cases.LIFTED stepped to the lift, the floor's halves defined as bodies A and B and lifted, one more step."""
    case = wall_cases.lifted(name)
    hip = scenes.hip_for(case["sc"])
    if setup:
        setup(hip)
    for it in range(case["steps"]):
        scenes.staged_step(hip, it) if staged else hip.step(it)
    for slot, ids in ((A, case["A"]), (B, case["B"])):
        assert hip.body_define_ids(slot, ids) == ids.size
        hip.body_set_pose(slot, case["pose"])
    scenes.staged_step(hip, case["steps"]) if staged else hip.step(case["steps"])
    return hip, case


def floor_states(case, **kw):
    cfg = case["cfg"]
    return {A: mass_state(cfg, case["pos"][case["A"].astype(np.int64)], case["pose"], gravity=(0, 0, 0), **kw),
            B: mass_state(cfg, case["pos"][case["B"].astype(np.int64)], case["pose"], **kw)}


def dynamic_floor(name, setup=None, staged=False, **kw):
    hip, case = lifted_solver(name, setup, staged)
    bodies = Bodies(hip, case["cfg"])
    for slot, st in floor_states(case, **kw).items():
        bodies.add(slot, st)
    return hip, case, bodies


# ---------------------------------------------------------------------------------------------- loads, state, placement
@pytest.mark.parametrize("name,third", [("tiny", False), ("tiny_jitter", False), ("tiny", True)])
def test_loads_state_and_placement(name, third):
    hip, case, bodies = dynamic_floor(name)
    cfg = case["cfg"]
    if third:  # a kinematic body on part of the shell: the wall at x = xmin above the floor
        assert hip.body_define_region(C3, (-INF, f32(2) * f32(cfg.r0), -INF, f32(cfg.r0), INF, INF)) > 0
    # the loads against the restatement of the wall loads on the solver's exported state
    state = wr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    K, W = fr.constants(cfg), wr.constants(cfg)
    members = {A: case["A"], B: case["B"]}
    D_ref = {}
    for slot in (A, B):
        wall = wr.Wall(state, ids, dist, K, W, wr.wall_set(state, slot, members))
        D_ref[slot] = wr.diag_records(state, wall.records, EVERYTHING, ALL_TYPES)[0]
    D_gpu = load_records(hip, (A, B))
    old = {s: dict(bodies.state[s]) for s in (A, B)}
    rec = bodies.advance_and_check("%s, first advance" % name)
    for slot in (A, B):
        assert same_numbers(D_gpu[slot], D_ref[slot])
        _, _, want = bd.advance(D_ref[slot], old[slot], *bd.constants(cfg))
        assert same_numbers(rec[slot, 20:28], want[20:28]), (slot, rec[slot, 20:28], want[20:28])
        assert rec[slot, 0] == 0 and rec[slot, 1] == members[slot].size and rec[slot, 2] == 1 and 0 < rec[slot, 3] < 0.25
        assert rec[slot, 21] < 0 and rec[slot, 12] < 0 and rec[slot, 27] > 0 and np.abs(rec[slot, 23:26]).max() > 0
    assert rec[A, 26] == rec[B, 26] > 0
    if third:
        assert rec[C3, 0] == -1 and hip.body_dynamics(C3) is None
    # a second advance on the same state: the load is the same (the walls are where the step saw them), the state moves on
    rec2 = bodies.advance_and_check("%s, second advance" % name)
    assert same_numbers(rec2[A, 20:23], rec[A, 20:23]) and same_numbers(rec2[A, 26:28], rec[A, 26:28])
    assert rec2[A, 2] == 2 and rec2[A, 12] < rec[A, 12] and not same_numbers(rec2[A, 23:26], rec[A, 23:26])  # (Tl is about the new X)
    hip.step(case["steps"] + 1)
    bodies.pos, bodies.vel = read_state(hip)
    bodies.advance_and_check("%s, after a further step" % name)
    hip.close()


def test_free_rotation():
    """The half floor with its centre of mass displaced, so that the load has a torque about it."""
    r0 = float(wall_cases.lifted("tiny_jitter")["cfg"].r0)
    hip, case, bodies = dynamic_floor("tiny_jitter", com_shift=(1.5 * r0, 0.0, -0.75 * r0), angularMomentum=(0.0, 1e-7, 0.0),
                                      orientation=(0.999, 0.01, -0.02, 0.03))
    vel0 = bodies.vel.copy()
    for k in range(3):
        rec = bodies.advance_and_check("free rotation, advance %d" % k)
        assert rec[A, 0] == 0 and np.abs(rec[A, 17:20]).min() > 0 and np.abs(rec[A, 14:17]).min() > 0
        hip.step(case["steps"] + 1 + k)
        bodies.pos, bodies.vel = read_state(hip)
    m = case["A"].astype(np.int64)
    assert not scenes.bits_equal(bodies.vel[m], vel0[m])  # the normals turned
    q = bodies.state[A]["orientation"]
    assert q != [0.999 / np.sqrt(0.999 ** 2 + 0.0014), 0, 0, 0] and abs(q[1]) + abs(q[2]) + abs(q[3]) > 0
    hip.close()


def test_locks():
    """Everything locked with a set velocity is a piston; the unlocked body beside it answers the liquid."""
    hip, case = lifted_solver("tiny")
    cfg = case["cfg"]
    _, hp, _ = bd.constants(cfg)
    bodies = Bodies(hip, cfg)
    st = floor_states(case)
    v = 0.05 * float(cfg.r0) / hp
    st[A] = dict(st[A], locks=15, velocity=[0.0, v, 0.0], spin=[0.0, 0.0, 0.0])
    bodies.add(A, st[A])
    bodies.add(B, st[B])
    y0 = st[A]["position"][1]
    for k in range(3):
        rec = bodies.advance_and_check("locks, advance %d" % k)
        assert rec[A, 11:14].tolist() == [0.0, v, 0.0] and not rec[A, 17:20].any() and rec[A, 21] < 0
        assert rec[B, 12] < 0 and np.abs(rec[B, 17:20]).max() > 0
        hip.step(case["steps"] + 1 + k)
        bodies.pos, bodies.vel = read_state(hip)
    y = y0
    for _ in range(3):
        y = y + hp * v
    assert bodies.state[A]["position"][1] == y and bodies.state[A]["orientation"] == [1.0, 0.0, 0.0, 0.0]
    hip.close()


# ---------------------------------------------------------------------------------------------- the host loop it replaces
def host_loop_advance(hip, cfg, bodies):
    """What sph_bodies_advance replaces: per body a blocking wall_diagnostics, the integrator on the host, a blocking pose."""
    D = load_records(hip, bodies.state)
    dt, hp, mp = bd.constants(cfg)
    for slot in sorted(bodies.state):
        new, pose, rec = bd.advance(D[slot], bodies.state[slot], dt, hp, mp)
        assert rec[0] == 0
        hip.body_set_pose(slot, pose)
        bodies.state[slot] = new


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter"])
def test_equals_the_host_loop_over_six_steps(name):
    from oracle import oraclebind as O
    dev, case, bodies_dev = dynamic_floor(name)
    host, _ = lifted_solver(name)
    cfg = case["cfg"]
    sc = case["sc"]
    bodies_host = Bodies(host, cfg)
    bodies_host.state = floor_states(case)
    for k in range(6):
        it = case["steps"] + 1 + k
        assert dev.bodies_advance(read=False) is None
        host_loop_advance(host, cfg, bodies_host)
        pos, vel = read_state(dev)
        assert_state(host, pos, vel, "%s, advance %d: device route vs host loop" % (name, k))
        fresh = ora = None
        if k < 2:  # the continuation property: a solver, and the oracle, created from the moved arrays
            fresh = sphmi.owHIPSolver(cfg, pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"])
            ora = O.OracleSolver(sphmi.config_dict(cfg), pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"], threads=4)
            fresh.step(it)
            ora.step()
        dev.step(it)
        host.step(it)
        pos, vel = read_state(dev)
        assert_state(host, pos, vel, "%s, step %d: device route vs host loop" % (name, k))
        if fresh is not None:
            assert_state(fresh, pos, vel, "%s, step %d: moved vs fresh" % (name, k))
            N = cfg.particleCount
            assert scenes.bits_equal(pos, ora.buffer("position").reshape(-1, 4)[:N]) and scenes.bits_equal(vel, ora.buffer("velocity").reshape(-1, 4)[:N])
            fresh.close()
            ora.close()
    for slot in (A, B):
        got = dev.body_dynamics(slot)
        for key, v in bodies_host.state[slot].items():
            assert same_numbers(got[key], v), (slot, key)
    assert bodies_host.state[A]["position"][1] < floor_states(case)[A]["position"][1]  # the floor sank
    assert np.isfinite(pos).all()
    dev.close()
    host.close()


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
_mode_reference = {}


@pytest.mark.parametrize("mode", list(MODES))
def test_every_step_mode(mode):
    """One advance and one step per mode: the record and the arrays against the restatement, and against the first mode's."""
    hip, case, bodies = dynamic_floor("tiny", **MODES[mode])
    rec = bodies.advance_and_check("mode %s" % mode)
    it = case["steps"] + 1
    scenes.staged_step(hip, it) if MODES[mode].get("staged") else hip.step(it)
    pos, vel = read_state(hip)
    ref = _mode_reference.setdefault("tiny", (rec, pos, vel))
    assert same_numbers(rec, ref[0]) and scenes.bits_equal(pos, ref[1]) and scenes.bits_equal(vel, ref[2]), "mode %s vs %s" % (mode, list(MODES)[0])
    hip.close()


# ---------------------------------------------------------------------------------------------- refusal, member counts
@pytest.fixture(scope="module")
def wide():
    sc = scenes.SCENES["wide"]()
    hip = scenes.hip_for(sc)
    hip.step(0)
    yield sc, hip
    hip.close()


def test_refused_pose_leaves_the_body_and_advances_the_other(wide):
    sc, hip = wide
    cfg = sc["cfg"]
    r0 = f32(cfg.r0)
    _, hp, _ = bd.constants(cfg)
    pos, vel = read_state(hip)
    box = (f32(cfg.xmax) - f32(3) * r0, -INF, -INF, INF, INF, INF)  # the wall at x = xmax and the rows of the others next to it
    other = (-INF, -INF, -INF, f32(cfg.xmin) + r0, INF, INF)          # the wall at x = xmin
    assert hip.body_define_region(2, box) > 0 and hip.body_define_region(9, other) > 0
    bodies = Bodies(hip, cfg)
    v = float(r0) / hp
    bodies.add(2, mass_state(cfg, bodies_ref(hip, 2), locks=15, velocity=[v, 0.0, 0.0]))
    bodies.add(9, mass_state(cfg, bodies_ref(hip, 9), locks=15, velocity=[0.25 * v, 0.0, 0.0]))
    before = dict(bodies.state[2])
    rec = bodies.advance_and_check("refusal")
    with pytest.raises(br.Refused) as want:
        br.set_pose(cfg, pos, vel, bodies.body[2], frames.pose_translate((float(r0), 0, 0)))
    assert rec[2, 0] == 1 and rec[2, 2] == 0 and rec[2, 3] == 0
    assert 0 < rec[2, 28] == want.value.offenders < bodies.body[2][0].size and rec[2, 29] == want.value.lowest_member
    assert rec[2, 4] > before["position"][0]  # the record reports the state that was refused
    assert bodies.state[2] == before and rec[9, 0] == 0 and rec[9, 2] == 1 and rec[9, 3] > 0
    m2, m9 = bodies.body[2][0].astype(np.int64), bodies.body[9][0].astype(np.int64)
    assert scenes.bits_equal(bodies.pos[m2], pos[m2]) and not scenes.bits_equal(bodies.pos[m9], pos[m9])
    # a state that is not finite: status 2, nothing moves
    bodies.state[9] = dict(bodies.state[9], velocity=[1e308, 0.0, 0.0], force=[1e308, 0.0, 0.0], locks=14, mass=1e-300)
    set_dynamics(hip, 9, bodies.state[9])
    bodies.advances[9] = 0
    rec = bodies.advance_and_check("non-finite")
    assert rec[9, 0] == 2 and rec[2, 0] == 1
    for slot in (2, 9):
        hip.body_set_dynamics(slot)
        hip.body_set_pose(slot, frames.pose_identity())
        hip.body_release(slot)
    back = read_state(hip)
    assert np.array_equal(back[0], pos) and np.array_equal(back[1], vel)  # (as numbers: an identity pose turns a -0 normal word into +0)


def bodies_ref(hip, slot):
    return hip.body_read(slot)[1]


def test_member_count_edges_and_the_whole_shell(wide):
    sc, hip = wide
    cfg = sc["cfg"]
    _, hp, _ = bd.constants(cfg)
    pos0, vel0 = read_state(hip)
    shell = br.region_members(pos0)
    assert shell.size > 100000
    v = 0.125 * float(cfg.r0) / hp
    start = 7
    bodies = Bodies(hip, cfg)
    for slot, n in enumerate((1, 63, 64, 65, 255, 256, 257)):
        ids = shell[start:start + n][::-1] if n % 2 else shell[start:start + n]
        start += n
        assert hip.body_define_ids(slot, ids) == n
        ref = bodies_ref(hip, slot)
        inwards = np.where(ref[:, :3].astype(np.float64).mean(0) < [0.5 * cfg.xmax, 0.5 * cfg.ymax, 0.5 * cfg.zmax], 1.0, -1.0)  # wide ids: stay in the box
        inertia = frames.body_mass_properties(ref, n * float(f32(cfg.mass)))[1]
        spin_up = inertia @ np.array([0.0, 0.0, 0.01 / hp])  # L for a turn of 0.01 rad per step about z
        bodies.add(slot, mass_state(cfg, ref, locks=7, velocity=list(inwards * [v, 0.75 * v, 0.5 * v]), angularMomentum=spin_up))
    rec = bodies.advance_and_check("member counts")
    assert rec[:7, 1].tolist() == [1, 63, 64, 65, 255, 256, 257] and (rec[:7, 0] == 0).all() and (rec[:7, 3] > 0).all()
    for slot in range(7):
        hip.body_set_dynamics(slot)  # kinematic again, back to the reference placement, gone
        hip.body_set_pose(slot, frames.pose_identity())
        hip.body_release(slot)
    assert np.array_equal(hip.read_position_buffer(), pos0)
    assert hip.body_define_region(0, None) == shell.size
    whole = Bodies(hip, cfg)
    whole.add(0, mass_state(cfg, bodies_ref(hip, 0), locks=15, velocity=[v, 0.0, -v]))
    rec = whole.advance_and_check("the whole shell")
    assert rec[0, 0] == 0 and rec[0, 1] == shell.size and rec[0, 3] > 0
    hip.body_set_dynamics(0)
    hip.body_set_pose(0, frames.pose_identity())
    hip.body_release(0)


# ---------------------------------------------------------------------------------------------- tree, wide rows, elastic matter
def test_two_upper_levels_on_more_than_a_million_particles():
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    cfg = sc["cfg"]
    assert cfg.particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    assert hip.body_define_region(A, (-INF, -INF, -INF, f32(0.5) * f32(cfg.xmax), f32(cfg.r0), INF)) > 0
    lift = frames.pose_translate((0.0, 2.4 * float(f32(cfg.r0)), 0.0))
    hip.body_set_pose(A, lift)
    hip.step(0)
    state = mass_state(cfg, bodies_ref(hip, A), lift)
    hip.body_set_dynamics(A, **state)
    D = load_records(hip, (A,))[A]
    rec = hip.bodies_advance()
    _, _, want = bd.advance(D, state, *bd.constants(cfg))
    assert same_numbers(rec[A, 4:28], want[4:28]), (rec[A, 4:28], want[4:28])
    assert rec[A, 0] == 0 and rec[A, 26] == D[1] > 1000 and rec[A, 27] == D[2] > 1000 and rec[A, 21] < 0
    hip.close()


def test_rows_without_a_16_bit_copy():
    sc = wall_cases.dense_on_floor()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    assert hip.body_define_region(A, (-INF, -INF, -INF, f32(5) * f32(cfg.r0), f32(cfg.r0), INF)) > 0  # the cube stands on the body's edge
    hip.step(0)
    counters = hip.buffer("debugCounters")[:4].astype(np.int64)
    assert int(counters[0] + counters[1]) > 100  # particles served by the exact walk: rows in 32 bits only
    bodies = Bodies(hip, cfg)
    bodies.add(A, mass_state(cfg, bodies_ref(hip, A)))
    rec = bodies.advance_and_check("dense cube")
    assert rec[A, 0] == 0 and rec[A, 27] > 0 and rec[A, 26] >= rec[A, 27] and rec[A, 21] != 0
    hip.close()


def test_with_elastic_matter():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(20):
        hip.step(it)
    pos = hip.read_position_buffer()
    mid = f32(0.5) * f32(cfg.xmax)
    assert hip.body_define_region(A, (-INF, -INF, -INF, mid, INF, INF)) > 0 and hip.body_define_region(B, (mid, -INF, -INF, INF, INF, INF)) > 0
    hip.step(20)
    bodies = Bodies(hip, cfg)
    for slot in (A, B):
        bodies.add(slot, mass_state(cfg, bodies_ref(hip, slot), gravity=(0, 0, 0)))
    rec = bodies.advance_and_check("tiny_elastic")
    assert (rec[[A, B], 0] == 0).all() and np.abs(rec[A, 20:23]).max() > 0 and np.abs(rec[B, 20:23]).max() > 0
    scenes.staged_step(hip, 21)
    assert np.isfinite(hip.read_position_buffer()).all()
    hip.close()


# ---------------------------------------------------------------------------------------------- interactions
def test_analysis_state_and_fields_survive_an_advance():
    hip, case, bodies = dynamic_floor("tiny")
    cfg = case["cfg"]
    pos = bodies.pos
    box = er.liquid_quantile_box(pos, 0.1, 0.9)
    assert hip.select(box, (1,), (("density", 0.0, INF),)) > 0
    sel = hip.selection()
    assert hip.label_components()[1] > 0
    comp = hip.components()
    hip.field_create(1, np.random.default_rng(3).random(hip.N, np.float32))
    dye = hip.field_read(1)
    diag = hip.diagnostics()
    walls = hip.wall_measure(A)
    bodies.advance_and_check("interactions")
    for a, b in zip(hip.selection(), sel):
        assert scenes.bits_equal(a, b)
    for a, b in zip(hip.components(), comp):
        assert scenes.bits_equal(a, b)
    assert scenes.bits_equal(hip.field_read(1), dye) and scenes.bits_equal(hip.diagnostics(), diag)
    assert scenes.bits_equal(hip.wall_measure(A), walls)
    # a pose on a dynamic body moves the particles only: the next advance places them from the dynamic state again
    state = dict(bodies.state[A])
    hip.body_set_pose(A, frames.pose_translate((0.0, 1.0 * float(cfg.r0), 0.0)))
    got = hip.body_dynamics(A)
    assert all(same_numbers(got[k], v) for k, v in state.items())
    bodies.pos, bodies.vel = read_state(hip)
    bodies.advance_and_check("after a pose")
    hip.close()


def test_edits_redefinition_and_overlap():
    sc = scenes.SCENES["tiny"]()
    cfg0 = sc["cfg"]
    n, r0 = cfg0.particleCount, f32(cfg0.r0)
    hip = sphmi.owHIPSolver(er.with_count(cfg0, n, n + 64), sc["position"], sc["velocity"])
    hip.step(0)
    pos, vel = read_state(hip)
    floor = br.region_members(pos, (-INF, -INF, -INF, INF, r0, INF))
    assert hip.body_define_ids(3, floor[:100]) == 100 and hip.body_define_ids(4, floor[60:]) == floor.size - 60
    st3 = mass_state(cfg0, bodies_ref(hip, 3))
    hip.body_set_dynamics(3, **st3)
    # overlap: 40 members of slot 4 are members of the dynamic body 3
    with pytest.raises(sphmi.SphError) as ei:
        hip.body_set_dynamics(4, **mass_state(cfg0, bodies_ref(hip, 4)))
    assert scenes.error_status(ei) == ERR_INVALID and hip.body_dynamics(4) is None
    m = re.search(r"(\d+) of the (\d+) members of slot 4 .* lowest shared id is (\d+)", str(ei.value))
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (40, floor.size - 60, int(floor[60]))
    assert hip.body_define_ids(4, floor[100:]) == floor.size - 100
    hip.body_set_dynamics(4, **mass_state(cfg0, bodies_ref(hip, 4)))
    hip.body_set_dynamics(3, **st3)  # setting a dynamic body again does not collide with itself
    # a removal that shifts every id carries the dynamics along, unchanged
    liquid = np.flatnonzero(pos[:, 3].astype(np.int32) == 1)[:10]
    assert liquid.max() < floor.min() and hip.remove_ids(liquid) == 10
    emap = hip.edit_map()
    got = hip.body_dynamics(3)
    assert all(same_numbers(got[k], v) for k, v in st3.items())
    assert np.array_equal(hip.body_read(3)[0], emap[floor[:100].astype(np.int64)].astype(np.uint32))
    with pytest.raises(sphmi.SphError) as ei:  # the sorted state is gone
        hip.bodies_advance()
    assert scenes.error_status(ei) == ERR_ORDER
    hip.step(1)
    bodies = Bodies(hip, cfg0)
    for slot in (3, 4):
        ids, rp, rn = hip.body_read(slot)
        bodies.body[slot], bodies.advances[slot] = (ids, rp, rn), 0
        bodies.state[slot] = bd.state_of(hip.body_dynamics(slot))
    rec = bodies.advance_and_check("after the removal")
    assert (rec[[3, 4], 0] == 0).all()
    # a body emptied by a removal loses its dynamics with the slot; redefinition and release clear them
    assert hip.remove_ids(hip.body_read(4)[0]) == floor.size - 100 and hip.body_count(4) == 0 and hip.body_dynamics(4) is None
    assert hip.body_define_ids(3, hip.body_read(3)[0][:50]) == 50 and hip.body_dynamics(3) is None
    hip.step(2)
    out = hip.bodies_advance()
    assert (out[:, 0] == -1).all() and not out[:, 1:].any()
    hip.body_set_dynamics(3, **st3)
    hip.body_set_dynamics(3)
    assert hip.body_dynamics(3) is None
    hip.body_set_dynamics(3, **st3)
    hip.body_release(3)
    assert hip.body_dynamics(3) is None
    hip.close()


# ---------------------------------------------------------------------------------------------- the calling rules
def _status(call):
    with pytest.raises(sphmi.SphError) as ei:
        call()
    return scenes.error_status(ei)


def test_calling_rules():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    floor = (-INF, -INF, -INF, INF, f32(cfg.r0), INF)
    assert hip.body_define_region(A, floor) > 0
    good = mass_state(cfg, bodies_ref(hip, A))
    assert _status(lambda: hip.bodies_advance()) == ERR_ORDER and _status(lambda: hip.bodies_advance(read=False)) == ERR_ORDER  # no step yet
    hip.step(0)
    out = hip.bodies_advance()  # nothing is dynamic: nothing to do
    assert (out[:, 0] == -1).all() and hip.bodies_advance(read=False) is None
    for slot in (-1, sphmi.MAX_BODIES, 1 << 20):
        assert _status(lambda: hip.body_set_dynamics(slot, **good)) == ERR_INVALID
        assert _status(lambda: hip.body_dynamics(slot)) == ERR_INVALID
    assert _status(lambda: hip.body_set_dynamics(B, **good)) == ERR_ORDER and _status(lambda: hip.body_set_dynamics(B)) == ERR_ORDER  # a free slot
    assert hip.body_dynamics(B) is None and hip.body_dynamics(A) is None
    bad = [dict(mass=0.0), dict(mass=-1.0), dict(mass=np.nan), dict(mass=np.inf), dict(com=(0, np.nan, 0)), dict(position=(np.inf, 0, 0)),
           dict(orientation=(0.1, 0.2, 0.0, 0.0)), dict(orientation=(2.0, 1.0, 0.0, 0.0)), dict(orientation=(0, 0, 0, 0)),
           dict(inertiaInv=(-1, 1, 1, 0, 0, 0)), dict(inertiaInv=(1, 1, 1, 2, 0, 0)), dict(inertiaInv=(1, 1, np.nan, 0, 0, 0)), dict(inertiaInv=(1, 1, 1, 0.9, 0.9, -0.9)),
           dict(velocity=(0, 0, np.nan)), dict(angularMomentum=(np.inf, 0, 0)), dict(spin=(0, np.nan, 0)), dict(gravity=(np.nan, 0, 0)),
           dict(force=(0, 0, np.inf)), dict(torque=(np.nan, 0, 0)), dict(contactGain=np.nan), dict(forceGain=np.inf), dict(locks=16)]
    for change in bad:
        assert _status(lambda: hip.body_set_dynamics(A, **dict(good, **change))) == ERR_INVALID, change
        assert hip.body_dynamics(A) is None
    assert hip._L.sph_body_get_dynamics(hip._h, A, None, None) == ERR_INVALID
    # the pseudo-inverse of a singular inertia (a row of particles along a diagonal) is semi-definite only up to rounding: accepted
    row = np.arange(7.0)[:, None] * np.array([[0.3, 0.7, -0.2]])
    jinv = frames.body_mass_properties(row, 1.0)[2]
    assert np.abs(jinv[3:]).min() > 0
    hip.body_set_dynamics(A, **dict(good, inertiaInv=jinv))
    assert same_numbers(hip.body_dynamics(A)["inertiaInv"], jinv)
    hip.body_set_dynamics(A)
    hip.body_set_dynamics(A, **dict(good, orientation=(1.5, 0.0, 0.0, 0.0), locks="yr"))
    got = hip.body_dynamics(A)
    assert got["orientation"].tolist() == [1.0, 0.0, 0.0, 0.0] and got["locks"] == 10  # normalised by the call
    assert hip.bodies_advance()[A, 0] == 0
    # a half-done staged step: SPH_ERR_ORDER from its first stage until the stage that leaves the arrays final
    seq = scenes.STAGE_SEQUENCE
    for i, st in enumerate(seq[:-1]):
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
        if i in (0, 1, 7, seq.index("integrate") - 1, seq.index("integrate"), len(seq) - 2):
            assert _status(lambda: hip.bodies_advance(read=False)) == ERR_ORDER, st
    getattr(hip, scenes.HIP_STAGE_METHOD[seq[-1]])()
    assert hip.bodies_advance()[A, 0] == 0
    # after an edit the sorted state is gone
    assert hip.remove_region((-INF, f32(0.5) * f32(cfg.ymax), -INF, INF, INF, INF), (1,)) > 0
    assert _status(lambda: hip.bodies_advance()) == ERR_ORDER
    hip.step(2)
    assert hip.bodies_advance()[A, 0] == 0
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _status(lambda: hip.bodies_advance()) == ERR_INVALID
    assert _status(lambda: hip.body_set_dynamics(0, mass=1.0, com=(0, 0, 0), position=(0, 0, 0))) == ERR_INVALID
    assert _status(lambda: hip.body_dynamics(0)) == ERR_INVALID
    hip.close()


# ---------------------------------------------------------------------------------------------- the driver
def test_cpp_driver_free_body():
    """sphmi_run --body-free prints one line per advance: the record's numbers, against a replay through the Python wrapper."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    r0 = float(f32(cfg.r0))
    args = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--quiet", "--body-region", "-inf", "-inf", "-inf", "inf",
            "%.9g" % r0, "inf", "--body-free", "--body-locks", "xzr", "--body-gains", "0.5", "1", "--body-velocity", "0", "%.17g" % (0.6 * r0), "0"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("_free: step")]
    assert len(lines) == 4 and "_body: step" not in r.stdout, r.stdout
    hip = scenes.hip_for(sc)
    assert hip.body_define_region(0, (-INF, -INF, -INF, INF, f32(r0), INF)) == 256
    ref = hip.body_read(0)[1]
    com = [0.0, 0.0, 0.0]
    for row in ref:  # the driver's sum: member order, in double
        for c in range(3):
            com[c] = com[c] + float(row[c])
    com = [x / 256.0 for x in com]
    hp = bd.constants(cfg)[1]
    rise = float("%.17g" % (0.6 * r0))  # the floor starts upwards at 0.6 r0 per step and meets the liquid within the run
    hip.body_set_dynamics(0, mass=256 * float(f32(cfg.mass)), com=com, position=com, locks="xzr", contactGain=0.5, forceGain=1.0,
                          velocity=(0.0 / hp, rise / hp, 0.0 / hp))
    for it in range(4):
        hip.step(it)
        rec = hip.bodies_advance()[0]
        words = [rec[0], rec[2], rec[3]] + list(rec[4:7]) + list(rec[11:14]) + list(rec[20:23])
        got = [float(x) for x in re.findall(r"[-+]?\d\.\d+e[-+]\d+|(?<=status )\d+|(?<=advances )\d+", lines[it])]
        assert lines[it].startswith("_free: step %d body 0 status 0 advances %d max_move " % (it + 1, it + 1)), lines[it]
        assert got == [float("%.0f" % words[0]), float("%.0f" % words[1])] + [float("%.9e" % x) for x in words[2:]], (lines[it], words)
    assert rec[21] < 0 and rec[27] > 0 and rec[11] == 0 and rec[13] == 0  # the liquid pushes the risen floor down; x and z are locked
    hip.close()
    r = subprocess.run([exe, "--steps", "1", "--body-free", "--body-locks", "q", "--body-region", "0", "0", "0", "1", "1", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip()
