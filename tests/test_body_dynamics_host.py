"""CPU tests of the free-body contract (include/sphmi.h, sph_bodies_advance) through its restatement tests/body_dyn_ref.py: one
advance by hand against literal numbers, free fall and torque-free motion over many steps, the premise of the feature on the oracle
and tests/wall_ref.py alone (the lifted floors of tests/wall_cases.py push the liquid up, so the liquid loads them downwards and a
free floor sinks without tunnelling), the mass-property helper and the binding. tests/test_body_dynamics.py compares the library
with the same restatement on the GPU."""
import functools
import math

import numpy as np
import pytest

import body_dyn_ref as bd
import body_ref as br
import diag_ref
import forces_ref as fr
import scenes
import sphmi
import wall_cases
import wall_ref as wr
from sphmi import frames

EVERYTHING = np.array([diag_ref.EVERYTHING], np.float32)
DT, HP, MP = 0.5, 2.0, 0.25  # exact binary numbers: the literals below are exact


def load_record(visc=(0, 0, 0), contact=(0, 0, 0), tc=(0, 0, 0), th=(0, 0, 0)):
    D = np.zeros(32)
    D[7:10], D[10:13], D[19:22], D[22:25] = contact, visc, tc, th
    D[1], D[2] = 7, 5
    return D


def test_unit_load_on_an_axis_aligned_body_by_hand():
    s = bd.make_state(2.0, com=(0.5, 0.25, 0.0), position=(1.0, 2.0, 3.0), inertiaInv=(2, 4, 8, 0, 0, 0))
    new, pose, rec = bd.advance(load_record(visc=(0, -4, 0)), s, DT, HP, MP)
    assert rec[20:23].tolist() == [0.0, 1.0, 0.0]                       # Fl = -(mp * H)
    assert rec[23:26].tolist() == [3.0, 0.0, -1.0]                      # Tl = -X x Fl
    assert new["velocity"] == [0.0, 0.25, 0.0] and new["position"] == [1.0, 2.5, 3.0]
    assert new["angularMomentum"] == [1.5, 0.0, -0.5] and rec[17:20].tolist() == [3.0, 0.0, -4.0]
    n = math.sqrt(26.0)                                                 # q* = (1, 3, 0, -4)
    assert new["orientation"] == [1.0 / n, 3.0 / n, 0.0 / n, -4.0 / n]
    assert rec[0] == 0 and rec[26] == 7 and rec[27] == 5 and not rec[28:].any()
    R = np.array(bd.rotation(new["orientation"]))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15)
    want_t = np.array(new["position"]) - R @ np.array(s["com"])
    assert np.array_equal(pose[:, :3], R.astype(np.float32)) and np.allclose(pose[:, 3], want_t, atol=1e-6)
    # the contact term: C / dt enters with the contact gain, H with the force gain
    s2 = dict(s, contactGain=3.0, forceGain=0.5)
    _, _, rec2 = bd.advance(load_record(visc=(0, -4, 0), contact=(1, 0, 0), tc=(0, 0, 2), th=(8, 0, 0)), s2, DT, HP, MP)
    assert rec2[20:23].tolist() == [-(0.25 * (3.0 * 2.0)), 0.5, 0.0]
    t0 = [-(0.25 * (0.5 * 8.0)), 0.0, -(0.25 * (3.0 * 4.0))]
    fl = rec2[20:23]
    assert rec2[23:26].tolist() == [t0[0] - (2.0 * fl[2] - 3.0 * fl[1]), t0[1] - (3.0 * fl[0] - 1.0 * fl[2]), t0[2] - (1.0 * fl[1] - 2.0 * fl[0])]


def test_a_locked_axis_and_locked_rotation_by_hand():
    s = bd.make_state(2.0, com=(0, 0, 0), position=(1.0, 2.0, 3.0), velocity=(0.5, -0.125, 0.0), inertiaInv=(2, 4, 8, 0, 0, 0),
                      angularMomentum=(1.0, 2.0, 3.0), spin=(0.0, 0.0, 0.5), gravity=(0.0, -8.0, 1.0), force=(2.0, 0.0, 0.0),
                      locks=bd.LOCK_Y | bd.LOCK_ROTATION)
    new, pose, rec = bd.advance(load_record(visc=(0, -4, 0)), s, DT, HP, MP)
    assert new["velocity"] == [0.5 + 0.5 * (2.0 / 2.0), -0.125, 0.0 + 0.5 * (2.0 / 2.0)]  # y keeps its value whatever pushes
    assert new["position"] == [1.0 + 2.0 * 1.0, 2.0 + 2.0 * -0.125, 3.0 + 2.0 * 0.5]
    assert new["angularMomentum"] == [1.0, 2.0, 3.0] and rec[17:20].tolist() == [0.0, 0.0, 0.5]
    n = math.sqrt(1.0 + 0.25)                                           # q* = (1, 0, 0, 0.5)
    assert new["orientation"] == [1.0 / n, 0.0, 0.0, 0.5 / n]
    assert rec[23:26].tolist() == [3.0, 0.0, -1.0]                      # the load's torque is reported although rotation is locked


def test_free_fall_is_the_plain_recurrence():
    g, mass, n = (0.0, -9.8, 0.3), 3.7, 500
    dt, hp = 1e-3, 0.7531
    s = bd.make_state(mass, com=(0.1, 0.2, 0.3), position=(1.0, 50.0, 2.0), velocity=(0.25, 0.0, -1.0), gravity=g, contactGain=0.0,
                      forceGain=0.0, locks=bd.LOCK_Z)
    D = load_record(visc=(3.0, 1.0, -2.0), contact=(1.0, 5.0, 2.0))  # a load that the zero gains switch off
    x, v = [1.0, 50.0, 2.0], [0.25, 0.0, -1.0]
    for _ in range(n):
        s, _, rec = bd.advance(D, s, dt, hp, 0.25)
        for c in range(3):
            if c != 2:
                v[c] = v[c] + dt * (((-0.0) + mass * g[c]) / mass)
            x[c] = x[c] + hp * v[c]
        assert rec[0] == 0
    assert s["velocity"] == v and s["position"] == x
    assert v[2] == -1.0 and s["orientation"] == [1.0, 0.0, 0.0, 0.0]


def test_torque_free_motion_keeps_L_and_the_quaternion_norm():
    L0 = [0.3, -1.1, 0.7]
    s = bd.make_state(1.5, com=(0, 0, 0), position=(0, 0, 0), inertiaInv=(1.0, 2.5, 0.4, 0.1, -0.2, 0.05), angularMomentum=L0,
                      orientation=(0.9, 0.1, -0.3, 0.2), contactGain=0.0, forceGain=0.0)
    D = load_record(visc=(3.0, 1.0, -2.0), th=(1.0, 2.0, 3.0))
    worst = 0.0
    q0 = list(s["orientation"])
    for _ in range(1000):
        s, _, _ = bd.advance(D, s, 1e-3, 0.05, 0.25)
        q = s["orientation"]
        worst = max(worst, abs(math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) - 1.0))
    ulp = 2.0 ** -52
    print("largest | |q| - 1 | over 1000 steps: %.3g = %.2f ulp" % (worst, worst / ulp))
    assert s["angularMomentum"] == L0          # bit-constant
    assert worst <= 4 * ulp                     # observed: at most 1 ulp (each step renormalises); asserted at 4 x that
    assert max(abs(a - b) for a, b in zip(q, q0)) > 0.01  # it did turn


# ---------------------------------------------------------------------------------------------- the premise, on the oracle alone
@functools.lru_cache(maxsize=None)
def premise_case(name):
    """The oracle through the step that follows the lift; the wall records of both halves of the floor on the state integrate read."""
    case = wall_cases.lifted(name)
    cfg = case["cfg"]
    N = cfg.particleCount
    ora = scenes.oracle_for(wall_cases.moved_scene(case))
    seq = scenes.STAGE_SEQUENCE
    k = seq.index("integrate")
    for st in seq[:k]:
        ora.run(st)
    state, ids, dist = wr.oracle_state(ora, N, cfg.gridCellCount)
    for st in seq[k:]:
        ora.run(st)
    pos = ora.buffer("position").reshape(-1, 4)[:N].copy()
    vel = ora.buffer("velocity").reshape(-1, 4)[:N].copy()
    ora.close()
    K, W = fr.constants(cfg), wr.constants(cfg)
    bodies = {wall_cases.SLOT_A: case["A"], wall_cases.SLOT_B: case["B"]}
    D = {}
    for slot in bodies:
        wall = wr.Wall(state, ids, dist, K, W, wr.wall_set(state, slot, bodies))
        D[slot] = wr.diag_records(state, wall.records, EVERYTHING, (1, 2, 3))[0]
    return dict(case=case, cfg=cfg, D=D, pos=pos, vel=vel, bodies=bodies)


def floor_state(case, ids, cfg, **kw):
    """The dynamic state of a half floor standing where the lift put it: equal point masses of cfg.mass each."""
    ref = case["pos"][np.asarray(ids, np.int64)]
    com, _, jinv = frames.body_mass_properties(ref, ids.size * float(cfg.mass))
    lift = np.asarray(case["pose"], np.float64)[:, 3]
    return bd.make_state(ids.size * float(cfg.mass), com=com, position=com + lift, inertiaInv=jinv, **kw)


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter"])
def test_the_liquid_loads_a_lifted_floor_downwards(name):
    c = premise_case(name)
    cfg, case = c["cfg"], c["case"]
    for slot, ids in c["bodies"].items():
        D = c["D"][slot]
        contact_y, stage_y = D[8], (D[11] + D[17]) + D[14]
        print("%s body %d: n contact %d, n share %d, contact sum y %.4g, force-stage sum y %.4g" % (name, slot, D[1], D[2], contact_y, stage_y))
        assert D[2] > 0 and contact_y > 0 and stage_y > 0
        for gains in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
            s = floor_state(case, ids, cfg, contactGain=gains[0], forceGain=gains[1])
            _, _, rec = bd.advance(D, s, *bd.constants(cfg))
            assert rec[21] < 0, gains
        # a free floor of the liquid's own particle mass, no gravity: it sinks, and by far less than r0 in a step
        s = floor_state(case, ids, cfg)
        body = br.define(case["pos"], case["vel"], ids)
        new, advances, rec, pos, vel = bd.advance_body(cfg, D, s, 0, body, c["pos"], c["vel"])
        print("%s body %d: V'.y %.4g, tunnelling number %.4g" % (name, slot, new["velocity"][1], rec[3]))
        assert rec[0] == 0 and advances == 1 and new["velocity"][1] < 0 and 0 < rec[3] < 0.25
        others = np.setdiff1d(np.arange(cfg.particleCount), ids)
        assert (pos[ids, 1] < c["pos"][ids, 1]).all() and scenes.bits_equal(pos[others], c["pos"][others])


# ---------------------------------------------------------------------------------------------- helpers and binding
def test_body_mass_properties():
    r0 = 0.5
    plate = np.stack(np.meshgrid(np.arange(4.0) * r0, [1.0], np.arange(6.0) * r0, indexing="ij"), -1).reshape(-1, 3)
    com, inertia, inv = frames.body_mass_properties(np.c_[plate, np.full(len(plate), 3.0)], 24.0)
    assert com.dtype == inertia.dtype == inv.dtype == np.float64
    assert np.allclose(com, [0.75, 1.0, 1.25])
    ixx = sum((z - 1.25) ** 2 for z in np.arange(6.0) * r0) * 4   # unit point masses
    izz = sum((x - 0.75) ** 2 for x in np.arange(4.0) * r0) * 6
    assert np.allclose(inertia, np.diag([ixx, ixx + izz, izz])) and np.allclose(inv, [1 / ixx, 1 / (ixx + izz), 1 / izz, 0, 0, 0])
    row = np.arange(5.0)[:, None] * np.array([[0.0, 0.0, 1.0]]) + np.array([[2.0, 3.0, 4.0]])
    com, inertia, inv = frames.body_mass_properties(row, 5.0)
    assert np.allclose(com, [2, 3, 6]) and np.allclose(inertia, np.diag([10.0, 10.0, 0.0]))
    assert inv.tolist() == [0.1, 0.1, 0.0, 0.0, 0.0, 0.0] or np.allclose(inv, [0.1, 0.1, 0, 0, 0, 0], atol=1e-15)
    assert inv[2] == 0.0                                              # the degenerate axis: a zero row, the body never turns about it
    com, inertia, inv = frames.body_mass_properties([[1.0, 2.0, 3.0]], 2.0)
    assert not inv.any()
    with pytest.raises(ValueError):
        frames.body_mass_properties(row, 0.0)


def test_body_state_summary():
    cfg = scenes.SCENES["tiny"]()["cfg"]
    rec = np.arange(48, dtype=np.float64)
    rec[0] = 1
    out = frames.body_state_summary(rec, cfg)
    assert out["status"] == 1 and out["members"] == 1 and out["lowest_member"] == 29 and out["offenders"] == 28
    assert np.array_equal(out["position"], rec[4:7] * float(cfg.simulationScale)) and np.array_equal(out["load_force"], rec[20:23])
    assert np.array_equal(out["velocity"], rec[11:14]) and out["max_move"] == 3


def test_binding_lists_the_free_body_calls():
    names = ["sph_body_set_dynamics", "sph_body_get_dynamics", "sph_bodies_advance"]
    L = sphmi.device_lib()
    for n in names:
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(L, n)
    assert sphmi.BODY_STATE_WORDS == bd.WORDS == 48
    used = sorted(w for first, count in sphmi.BODY_STATE_FIELDS.values() for w in range(first, first + count))
    assert used == list(range(30))
    for m in ("body_set_dynamics", "body_dynamics", "bodies_advance"):
        assert callable(getattr(sphmi.owHIPSolver, m))
    assert C_sizeof_matches()


def C_sizeof_matches():
    import ctypes
    return ctypes.sizeof(sphmi.SphBodyDynamics) == 8 * 37 + 8 and sphmi.SphBodyDynamics.locks.offset == 8 * 37
