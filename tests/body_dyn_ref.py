"""Restatement of the free-body contract (include/sphmi.h, sph_body_set_dynamics / sph_bodies_advance) in Python floats, which
are IEEE doubles: one operation at a time in the header's order, math.sqrt and `/` correctly rounded, nothing contracted. A state
is a dict named like sph_body_dynamics; `advance` takes a wall-diagnostics record (float64[32], wall_ref.diag_records or
sph_wall_diagnostics for slot, everything, types 1..3) and returns the new state, the float32 pose and the record of the advance.
`advance_body` adds the placement through body_ref.set_pose with its refusal rule. Nothing here calls the library."""
import math

import numpy as np

import body_ref as br

f32 = np.float32
WORDS = 48
VEC = {"com": 3, "inertiaInv": 6, "position": 3, "orientation": 4, "velocity": 3, "angularMomentum": 3, "spin": 3, "gravity": 3,
       "force": 3, "torque": 3}
LOCK_X, LOCK_Y, LOCK_Z, LOCK_ROTATION = 1, 2, 4, 8


def constants(cfg):
    """(dt, hp, mp): timeStep, posTimeStep = float(timeStep * simulationScaleInv) and cfg.mass, the floats widened."""
    dt = f32(cfg.timeStep)
    return float(dt), float(f32(dt * f32(cfg.simulationScaleInv))), float(f32(cfg.mass))


def make_state(mass, com, position, **kw):
    """A state with the wrappers' defaults (gravity has none here: pass it, or it is zero), q normalised as the call does it."""
    s = dict(mass=float(mass), contactGain=1.0, forceGain=1.0, locks=0)
    for k, n in VEC.items():
        s[k] = [0.0] * n
    s["orientation"] = [1.0, 0.0, 0.0, 0.0]
    s.update(com=com, position=position)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    for k, n in VEC.items():
        s[k] = [float(x) for x in np.asarray(s[k], np.float64).reshape(n)]
    w, x, y, z = s["orientation"]
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    s["orientation"] = [w / n, x / n, y / n, z / n]
    return s


def rotation(q):
    w, x, y, z = q
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def _row(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def advance(D, state, dt, hp, mp):
    """(new state, pose float32[3, 4], record float64[48]) of one advance under the load record D. The record's status is 0 or 2
    (non-finite); member count, advance count, tunnelling number and the refusal words are the caller's (advance_body)."""
    D = [float(x) for x in np.asarray(D, np.float64).reshape(32)]
    s = state
    cg, fg, mass = s["contactGain"], s["forceGain"], s["mass"]
    Fl, T0 = [0.0] * 3, [0.0] * 3
    for c in range(3):
        C, H, TC, TH = D[7 + c], (D[10 + c] + D[16 + c]) + D[13 + c], D[19 + c], D[22 + c]
        Fl[c] = -(mp * (cg * (C / dt) + fg * H))
        T0[c] = -(mp * (cg * (TC / dt) + fg * TH))
    X = s["position"]
    Tl = [T0[0] - (X[1] * Fl[2] - X[2] * Fl[1]), T0[1] - (X[2] * Fl[0] - X[0] * Fl[2]), T0[2] - (X[0] * Fl[1] - X[1] * Fl[0])]
    V, Xn = [0.0] * 3, [0.0] * 3
    for c in range(3):
        F = (Fl[c] + mass * s["gravity"][c]) + s["force"][c]
        V[c] = s["velocity"][c] if (s["locks"] >> c) & 1 else s["velocity"][c] + dt * (F / mass)
        Xn[c] = X[c] + hp * V[c]
    q = s["orientation"]
    if s["locks"] & LOCK_ROTATION:
        L, om = list(s["angularMomentum"]), list(s["spin"])
    else:
        L = [s["angularMomentum"][c] + dt * (Tl[c] + s["torque"][c]) for c in range(3)]
        R = rotation(q)
        J = s["inertiaInv"]  # xx yy zz xy xz yz
        u = [_row(R[0][c], L[0], R[1][c], L[1], R[2][c], L[2]) for c in range(3)]
        w = [_row(J[0], u[0], J[3], u[1], J[4], u[2]), _row(J[3], u[0], J[1], u[1], J[5], u[2]), _row(J[4], u[0], J[5], u[1], J[2], u[2])]
        om = [_row(R[c][0], w[0], R[c][1], w[1], R[c][2], w[2]) for c in range(3)]
    qw, qx, qy, qz = q
    d = [-((om[0] * qx + om[1] * qy) + om[2] * qz), (om[0] * qw + om[1] * qz) - om[2] * qy, (om[1] * qw + om[2] * qx) - om[0] * qz,
         (om[2] * qw + om[0] * qy) - om[1] * qx]
    hh = 0.5 * hp
    qs = [q[k] + hh * d[k] for k in range(4)]
    with np.errstate(all="ignore"):
        n = float(np.sqrt(np.float64(((qs[0] * qs[0] + qs[1] * qs[1]) + qs[2] * qs[2]) + qs[3] * qs[3])))
        qn = [float(np.float64(qs[k]) / np.float64(n)) for k in range(4)]
    Rn = rotation(qn)
    com = s["com"]
    pose = np.zeros((3, 4), np.float64)
    for r in range(3):
        pose[r, :3] = Rn[r]
        pose[r, 3] = Xn[r] - _row(Rn[r][0], com[0], Rn[r][1], com[1], Rn[r][2], com[2])
    with np.errstate(over="ignore"):
        pose = pose.astype(f32)
    new = dict(s, position=Xn, orientation=qn, velocity=V, angularMomentum=L)
    rec = np.zeros(WORDS, np.float64)
    rec[4:7], rec[7:11], rec[11:14], rec[14:17], rec[17:20], rec[20:23], rec[23:26] = Xn, qn, V, L, om, Fl, Tl
    rec[26], rec[27] = D[1], D[2]
    finite = np.isfinite(pose).all() and np.isfinite(rec[4:17]).all()
    rec[0] = 0.0 if finite else 2.0
    return new, pose, rec


def advance_body(cfg, D, state, advances, body, pos, vel):
    """(state, advances, record, position, velocity) after one advance of a body (ids, reference position, reference normal) on
    the arrays pos / vel: a refused pose (status 1) and a non-finite result (status 2) leave state, count and arrays as they were."""
    dt, hp, mp = constants(cfg)
    new, pose, rec = advance(D, state, dt, hp, mp)
    rec[1], rec[2] = len(body[0]), advances
    if rec[0] != 0:
        return state, advances, rec, pos, vel
    try:
        p, v, move = br.set_pose(cfg, pos, vel, body, pose)
    except br.Refused as e:
        rec[0], rec[28], rec[29] = 1.0, e.offenders, e.lowest_member
        return state, advances, rec, pos, vel
    rec[2], rec[3] = advances + 1, float(move)
    return new, advances + 1, rec, p, v


def state_of(dyn):
    """owHIPSolver.body_dynamics()' dict as a state of this module."""
    return {k: ([float(x) for x in v] if k in VEC else v) for k, v in dyn.items()}
