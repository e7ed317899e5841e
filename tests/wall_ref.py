"""numpy restatement of the wall-load contract (include/sphmi.h, sph_wall_measure / sph_wall_diagnostics).

Works from the contract alone, slot by slot and vectorised over the particles: every operation a rounded float32 one in the
written order. The nine force-stage words of a wall set come from forces_ref.Forces, asked for a state in which only the set's
boundary particles still have class 3; the region sums are float64 in the fixed tree of diag_ref.tree_sum. The state is
forces_ref's (solver_state / oracle_state) plus "vel4" (sortedVelocity with its .w lane), "acc" (buffer "acceleration", float32
[2N, 4]: both halves) and "orig" (the original id of every sorted particle); tests/test_wall_host.py ties words 19..25 to the
oracle's integrate stage."""
import numpy as np

import diag_ref
import forces_ref as fr

f32 = np.float32
SLOTS = 32
WORDS = 32
DIAG_WORDS = 32
TERMS = 26
BOUNDARY = 3
ALL, NO_BODY = -1, -2


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def constants(cfg):
    """What integrate reads of the configuration, as sph_create computes it."""
    dt = f32(_get(cfg, "timeStep"))
    return dict(dt=dt, posTimeStep=f32(dt * f32(_get(cfg, "simulationScaleInv"))), r0=f32(_get(cfg, "r0")),
                lo=np.array([_get(cfg, a + "min") for a in "xyz"], np.float32),
                hi=np.array([_get(cfg, a + "max") for a in "xyz"], np.float32),
                fold=int(_get(cfg, "numOfElasticP")) == 0)


def wall_set(state, slot, bodies):
    """bool[N] over SORTED indices: the wall set of `slot`. bodies: {slot: original ids}. ALL: every boundary particle; NO_BODY:
    the boundary particles that are members of no body; a body slot: its members."""
    types = _types(state)
    orig = np.asarray(state["orig"], np.int64)
    member = np.zeros(orig.size, bool)  # by original id
    if slot == ALL:
        return types == BOUNDARY
    for b, ids in bodies.items():
        if slot == NO_BODY or slot == b:
            member[np.asarray(ids, np.int64)] = True
    in_set = member[orig]
    return (types == BOUNDARY) & (~in_set if slot == NO_BODY else in_set)


def _types(state):
    with np.errstate(invalid="ignore"):
        return np.trunc(np.asarray(state["types"], np.float32)).astype(np.int64)  # (int)position.w


class Wall:
    """records float32[N, 32]; contact, reflected bool[N]; wsum, wS float32[N]; touching int[N]: boundary slots with w > 0."""

    def __init__(self, state, ids, dist, K, W, in_set):
        pos = np.asarray(state["pos"], np.float32)[:, :3]
        vel = np.asarray(state["vel4"], np.float32).reshape(-1, 4)
        N = pos.shape[0]
        acc = np.asarray(state["acc"], np.float32).reshape(-1, 4)
        a0, a1 = acc[:N, :3], acc[N:2 * N, :3]
        types = _types(state)
        in_set = np.asarray(in_set, bool) & (types == BOUNDARY)
        ids = np.asarray(ids, np.int64).reshape(-1, SLOTS)
        dt, pts, r0, half = W["dt"], W["posTimeStep"], W["r0"], f32(0.5)
        moving = types != BOUNDARY
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = (a0 + a1).astype(np.float32)
            nv = np.empty((N, 4), np.float32)
            nv[:, :3] = vel[:, :3] + dt * a
            nv[:, 3] = vel[:, 3] + dt * f32(0)
            x0 = (pos + pts * nv[:, :3]).astype(np.float32)
            for c in range(3):
                x0[:, c] = np.where(x0[:, c] < W["lo"][c], W["lo"][c], x0[:, c])
                top = f32(W["hi"][c] - f32(0.000001))
                x0[:, c] = np.where(x0[:, c] > top, top, x0[:, c])
            u0 = ((vel + nv) * half).astype(np.float32)
            n = np.zeros((N, 4), np.float32)
            wsum, wsum2, wS = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
            mS, cS, touching = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.int64)
            for k in range(SLOTS):
                j = ids[:, k]
                jc = np.maximum(j, 0)
                use = (j != -1) & (types[jc] == BOUNDARY) & moving
                pb, nb = pos[jc], vel[jc]
                dx, dy, dz = x0[:, 0] - pb[:, 0], x0[:, 1] - pb[:, 1], x0[:, 2] - pb[:, 2]
                d = dx * dx
                d = d + dy * dy
                d = d + dz * dz
                d = np.sqrt(d).astype(np.float32)
                w = np.fmax(f32(0), (r0 - d) / r0).astype(np.float32)  # fmaxf: a NaN operand gives the other one
                for c in range(4):
                    n[:, c] = np.where(use, n[:, c] + nb[:, c] * w, n[:, c])
                wsum = np.where(use, wsum + w, wsum)
                wsum2 = np.where(use, wsum2 + w * (r0 - d), wsum2)
                mine = use & in_set[jc]
                wS = np.where(mine, wS + w, wS)
                mS = np.where(mine, mS + f32(1), mS)
                cS = np.where(mine & (w > 0), cS + f32(1), cS)
                touching += use & (w > 0)
            len2 = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) + n[:, 3] * n[:, 3]
            contact = (len2 != 0) & moving
            ln = np.sqrt(len2).astype(np.float32)
            sh = np.zeros((N, 3), np.float32)
            for c in range(3):
                sh[:, c] = np.where(contact, ((n[:, c] / ln) * wsum2) / wsum, f32(0))
            x1 = np.where(contact[:, None], x0 + sh, x0).astype(np.float32)
            vn = (n[:, 0] * u0[:, 0] + n[:, 1] * u0[:, 1]) + n[:, 2] * u0[:, 2]
            reflected = contact & (vn < 0)
            u1 = u0.copy()
            for c in range(3):
                u1[:, c] = np.where(reflected, (u0[:, c] - n[:, c] * vn) * f32(0.99), u0[:, c])
            u1[:, 3] = np.where(reflected, u0[:, 3] * f32(0.99), u0[:, 3])
            dv = (u1 - u0).astype(np.float32)
            share = np.where(contact, wS / wsum, f32(0)).astype(np.float32)
            if W["fold"]:
                x1 = (x1 + f32(0)).astype(np.float32)
            # the set's nine force-stage words: class 3 of the decomposition when only the set still has class 3
            st = dict(state)
            ty = np.asarray(state["types"], np.float32).copy()
            ty[(types == BOUNDARY) & ~in_set] = f32(0)
            st["types"] = ty
            F = fr.Forces(st, ids, dist, K)
            rec = np.zeros((N, WORDS), np.float32)
            rec[:, 0:3] = sh * share[:, None]
            rec[:, 3:6] = dv[:, :3] * share[:, None]
            rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9] = share, wS, cS, mS
            rec[:, 10:19] = F.records[:, 18:27]
            rec[:, 19:22] = x1
            rec[:, 22:26] = u1
            rec[:, 26], rec[:, 27] = contact, reflected
        rec[~moving] = 0  # a boundary particle's record is all zero
        assert rec.dtype == np.float32
        self.records, self.contact, self.reflected, self.moving = rec, contact, reflected & moving, moving
        self.wsum, self.wS, self.touching = np.where(moving, wsum, f32(0)), np.where(moving, wS, f32(0)), np.where(moving, touching, 0)


def diag_terms(records, pos):
    """float32[26, N]: the per-particle terms of words 1..26 of a region record."""
    rec = np.asarray(records, np.float32)
    x, y, z = (np.asarray(pos, np.float32)[:, a] for a in range(3))
    t = np.zeros((TERMS, rec.shape[0]), np.float32)
    t[0] = rec[:, 26]
    t[1] = rec[:, 6] > 0
    t[2] = (rec[:, 27] != 0) & (rec[:, 6] > 0)
    t[3:9] = rec[:, 0:6].T
    t[9:18] = rec[:, 10:19].T
    with np.errstate(invalid="ignore", over="ignore"):
        q = rec[:, 10:19]
        h = [(q[:, a] + q[:, 6 + a]) + q[:, 3 + a] for a in range(3)]
        for o, (bx, by, bz) in ((18, (rec[:, 3], rec[:, 4], rec[:, 5])), (21, h)):
            t[o] = y * bz - z * by
            t[o + 1] = z * bx - x * bz
            t[o + 2] = x * by - y * bx
    t[24], t[25] = rec[:, 6], rec[:, 7]
    return t


def diag_records(state, records, regions, types):
    """float64[R, 32] of sph_wall_diagnostics."""
    t = diag_terms(records, state["pos"]).astype(np.float64)
    regions = np.asarray(regions, np.float32).reshape(-1, 6)
    out = np.zeros((regions.shape[0], DIAG_WORDS), np.float64)
    for r, region in enumerate(regions):
        sel = diag_ref.selected(state, region, types)
        out[r, 0] = diag_ref.tree_sum(sel.astype(np.float64))
        if not sel.any():
            continue  # every term is +0.0: so is every sum of the tree
        for w in range(TERMS):
            out[r, 1 + w] = diag_ref.tree_sum(np.where(sel, t[w], 0.0))
    return out


def solver_state(hip):
    """forces_ref.solver_state(hip) plus "vel4", "acc" and "orig" (the same as "ids")."""
    st = fr.solver_state(hip)
    N = hip.N
    st["vel4"] = hip.buffer("sortedVelocity").reshape(-1, 4)[:N].copy()
    st["acc"] = hip.buffer("acceleration").reshape(-1, 4)[:2 * N].copy()
    st["orig"] = np.asarray(st["ids"], np.int64)
    return st


def oracle_state(ora, N, G):
    """The same state from the oracle's buffers (reference layouts); (state, ids, dist)."""
    st, ids, dist = fr.oracle_state(ora, N, G)
    st["vel4"] = ora.buffer("sortedVelocity").reshape(-1, 4)[:N].copy()
    st["acc"] = ora.buffer("acceleration").reshape(-1, 4)[:2 * N].copy()
    st["orig"] = ora.buffer("particleIndex").reshape(-1, 2)[:N, 1].astype(np.int64)
    return st, ids, dist
