"""numpy restatement of the force-decomposition contract (include/sphmi.h, sph_force_measure / sph_force_diagnostics).

Works from the contract alone, slot by slot and vectorised over the particles: every operation a rounded float32 one in the
written order, the scales through float64 as the step computes them, the region sums float64 in the fixed tree of
diag_ref.tree_sum. The state is the existing exports (sortedPosition, sortedVelocity, rho with its predicted half, pressure,
the types and keys of particleIndex / position, the rows of sph_read_neighbor_rows) and the constants are derived from the
configuration the way sph_create derives them. tests/test_forces_host.py ties words 30..35 to the oracle's K7 and K12 stages."""
import numpy as np

import diag_ref

f32 = np.float32
f64 = np.float64
SLOTS = 32
WORDS = 40
DIAG_WORDS = 64
CLASSES = (1, 2, 3)  # liquid, elastic, boundary
BOUNDARY = 3


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def constants(cfg):
    """The step's constants as sph_create computes them (cfg: an SphConfig or sphmi.config_dict of one)."""
    mass, visc = f32(_get(cfg, "mass")), f32(_get(cfg, "viscosity"))
    h, ss = f32(_get(cfg, "h")), f32(_get(cfg, "simulationScale"))
    hs = f32(h * ss)
    half_hs = f32(hs / f32(2))
    close_r = 0.5 * float(half_hs)  # the double the reference compares with
    c = f32(close_r)  # the smallest float whose double value is >= closeR
    while float(c) < close_r:
        c = np.nextafter(c, f32(np.inf))
    while float(np.nextafter(c, f32(-np.inf))) >= close_r:
        c = np.nextafter(c, f32(-np.inf))
    return dict(massMu=f32(mass * visc), hs=hs, hq=f32(hs * f32(0.25)), closeRf=f32(c), simScale=ss,
                rho0delta=f32(f32(_get(cfg, "rho0")) * f32(_get(cfg, "delta"))),
                del2W=float(_get(cfg, "del2WviscosityCoefficient")),
                massGradW=float(mass) * float(_get(cfg, "gradWspikyCoefficient")),
                surfTens=f32(_get(cfg, "surfTensCoeff")), mass=float(mass),
                g=np.array([_get(cfg, "gravity_x"), _get(cfg, "gravity_y"), _get(cfg, "gravity_z")], np.float32))


class Forces:
    """records float32[N, 40]; S float32[4, 9, N], the unscaled sums (row 0 all used slots = the step's own, rows 1..3 per
    class; V xyz, T xyz, P xyz); A float64[9, N], the sums of |term| over the used slots; used_f / used_p bool[N, 32] and
    cls int[N, 32], which slots K7 / K12 used and the class of their neighbour."""

    def __init__(self, state, ids, dist, K):
        pos = np.asarray(state["pos"], np.float32)[:, :3]
        vel = np.asarray(state["vel"], np.float32)[:, :3]
        rho = np.asarray(state["rho"], np.float32)
        rho_star = np.asarray(state["rhoStar"], np.float32)
        p = np.asarray(state["p"], np.float32)
        with np.errstate(invalid="ignore"):
            types = np.trunc(np.asarray(state["types"], np.float32)).astype(np.int64)  # (int)position.w
        ids = np.asarray(ids, np.int64).reshape(-1, SLOTS)
        dist = np.asarray(dist, np.float32).reshape(-1, SLOTS)
        N = pos.shape[0]
        hs, hq, ss, half = K["hs"], K["hq"], K["simScale"], f32(0.5)
        moving = types != BOUNDARY
        S = np.zeros((4, 9, N), np.float32)
        A = np.zeros((9, N), np.float64)
        self.used_f, self.used_p = np.zeros((N, SLOTS), bool), np.zeros((N, SLOTS), bool)
        self.cls = np.zeros((N, SLOTS), np.int64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for k in range(SLOTS):
                j = ids[:, k]
                valid = j != -1
                jc = np.maximum(j, 0)
                cls = types[jc]
                xj, vj = pos[jc], vel[jc]  # a boundary neighbour's "velocity" is its wall normal (sphFluid.cl:653)
                term = np.zeros((9, N), np.float32)
                # K7
                rk = dist[:, k]
                use_f = valid & (rk < hs) & moving
                w = (hs - rk).astype(np.float32)
                for a in range(3):
                    term[a] = ((vj[:, a] - vel[:, a]) * w) / rho[jc]
                    term[3 + a] = K["surfTens"] * (pos[:, a] - xj[:, a])
                # K12
                e = (pos - xj).astype(np.float32)
                d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                r = (np.sqrt(d2).astype(np.float32) * ss).astype(np.float32)
                a1 = (hs - r).astype(np.float32)
                num = ((-a1 * a1) * half) * (p + p[jc])
                b1 = (hq - r).astype(np.float32)
                num = np.where(r < K["closeRf"], ((-b1 * b1) * half) * K["rho0delta"], num).astype(np.float32)
                value = (num / rho_star[jc]).astype(np.float32)
                for a in range(3):
                    term[6 + a] = (value * (e[:, a] * ss)) / r
                use_p = valid & (r < hs) & moving
                for q in range(9):
                    use = use_f if q < 6 else use_p
                    S[0, q] = np.where(use, S[0, q] + term[q], S[0, q])
                    A[q] += np.where(use, np.abs(term[q].astype(np.float64)), 0.0)
                    for c in CLASSES:
                        m = use & (cls == c)
                        S[c, q] = np.where(m, S[c, q] + term[q], S[c, q])
                self.used_f[:, k], self.used_p[:, k], self.cls[:, k] = use_f, use_p, cls
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            sF = (K["massMu"] * (K["del2W"] / rho.astype(np.float64)).astype(np.float32)).astype(np.float32)
            sP = (K["massGradW"] / rho_star.astype(np.float64)).astype(np.float32)
            rec = np.zeros((N, WORDS), np.float32)
            for c in CLASSES:
                o = 9 * (c - 1)
                for a in range(3):
                    rec[:, o + a] = S[c, a] * sF
                    rec[:, o + 3 + a] = S[c, 3 + a]
                    rec[:, o + 6 + a] = S[c, 6 + a] * sP
                rec[:, 27 + c - 1] = (self.used_f & (self.cls == c)).sum(1)
            for a in range(3):
                rec[:, 30 + a] = (S[0, a] * sF + K["g"][a]) + S[0, 3 + a]
                rec[:, 33 + a] = S[0, 6 + a] * sP
        rec[~moving] = 0  # a boundary particle's record is all zero
        self.records, self.S, self.A, self.moving = rec, S, A, moving


def diag_terms(records, pos, vel):
    """float32[48, N]: the per-particle terms of words 1..48 of a region record."""
    rec = np.asarray(records, np.float32)
    x, y, z = (np.asarray(pos, np.float32)[:, a] for a in range(3))
    vx, vy, vz = (np.asarray(vel, np.float32)[:, a] for a in range(3))
    t = np.zeros((48, rec.shape[0]), np.float32)
    t[:27] = rec[:, :27].T
    t[27:33] = rec[:, 30:36].T
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            q = rec[:, 9 * c:9 * c + 9]
            hx, hy, hz = ((q[:, a] + q[:, 6 + a]) + q[:, 3 + a] for a in range(3))
            t[33 + 3 * c] = y * hz - z * hy
            t[34 + 3 * c] = z * hx - x * hz
            t[35 + 3 * c] = x * hy - y * hx
            t[42 + c] = (hx * vx + hy * vy) + hz * vz
            t[45 + c] = rec[:, 27 + c]
    return t


def diag_records(state, records, regions, types):
    """float64[R, 64] of sph_force_diagnostics."""
    t = diag_terms(records, state["pos"], state["vel"]).astype(np.float64)
    regions = np.asarray(regions, np.float32).reshape(-1, 6)
    out = np.zeros((regions.shape[0], DIAG_WORDS), np.float64)
    for r, region in enumerate(regions):
        sel = diag_ref.selected(state, region, types)
        out[r, 0] = diag_ref.tree_sum(sel.astype(np.float64))
        if not sel.any():
            continue  # every term is +0.0: so is every sum of the tree
        for w in range(48):
            out[r, 1 + w] = diag_ref.tree_sum(np.where(sel, t[w], 0.0))
    return out


def solver_state(hip):
    """diag_ref.state_with_ids(hip) plus "rhoStar", the predicted density of the last predict-correct iteration."""
    st = diag_ref.state_with_ids(hip)
    st["rhoStar"] = hip.buffer("rho")[hip.N:2 * hip.N].copy()
    return st


def neighbor_rows(hip, piece=1 << 18):
    ids, dist = np.empty((hip.N, SLOTS), np.int32), np.empty((hip.N, SLOTS), np.float32)
    for first in range(0, hip.N, piece):
        n = min(piece, hip.N - first)
        ids[first:first + n], dist[first:first + n] = hip.neighbor_rows(first, n)
    return ids, dist


def oracle_state(ora, N, G):
    """The same state from the oracle's buffers (reference layouts)."""
    sp = ora.buffer("sortedPosition").reshape(-1, 4)[:N]
    pi = ora.buffer("particleIndex").reshape(-1, 2)[:N]
    rho = ora.buffer("rho")
    nm = ora.buffer("neighborMap").reshape(-1, 2)[:N * SLOTS]
    st = dict(pos=sp[:, :3].copy(), vel=ora.buffer("sortedVelocity").reshape(-1, 4)[:N, :3].copy(), rho=rho[:N].copy(),
              rhoStar=rho[N:2 * N].copy(), p=ora.buffer("pressure")[:N].copy(),
              types=ora.buffer("position").reshape(-1, 4)[pi[:, 1].astype(np.int64), 3].copy(), keys=pi[:, 0].copy(), G=int(G))
    return st, nm[:, 0].astype(np.int32).reshape(N, SLOTS), nm[:, 1].astype(np.float32).reshape(N, SLOTS)
