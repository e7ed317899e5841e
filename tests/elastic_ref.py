"""numpy restatement of the elastic-matter diagnostics contract (include/sphmi.h, sph_elastic_measure / sph_muscle_diagnostics /
sph_membrane_measure).

Works from the contract alone, slot by slot: every operation a rounded float32 one in the written order, the group sums float64
in the fixed tree of diag_ref.tree_sum, extremes by float compares canonicalised with + 0.0f. The state is three arrays: the
sorted positions [N, >=3], particleIndexBack [N] (original id -> sorted index) and the muscle signal; the tables are the ones the
solver was created with."""
import numpy as np

import diag_ref

f32 = np.float32
SLOTS = 32
ELASTIC_WORDS, MUSCLE_WORDS, MEMBRANE_WORDS = 12, 16, 8
K_SPRING, K_MUSCLE = f32(600000000.0), f32(800.0)


class Connections:
    """The per-connection quantities of the contract, arrays of shape [E, 32] (vectors [E, 32, 3]); dead slots hold zeros."""

    def __init__(self, sorted_pos, back, elastic, offset, sim_scale, muscle_count, signal):
        pos = np.asarray(sorted_pos, np.float32).reshape(-1, np.asarray(sorted_pos).shape[-1])[:, :3]
        back = np.asarray(back).astype(np.int64).reshape(-1)
        N = back.shape[0]
        conn = np.asarray(elastic, np.float32).reshape(-1, SLOTS, 4)
        E = conn.shape[0]
        signal = np.zeros(max(int(muscle_count), 1), np.float32) if signal is None else np.asarray(signal, np.float32).reshape(-1)
        with np.errstate(invalid="ignore"):
            jo = np.trunc(conn[:, :, 0]).astype(np.int64)  # (int)conn.x: toward zero
            mz = np.trunc(conn[:, :, 2]).astype(np.int64)
        ends = jo == -1
        first = np.where(ends.any(1), ends.argmax(1), SLOTS)  # a row ends at its first -1
        self.live = np.arange(SLOTS)[None, :] < first[:, None]
        self.bad = bool((self.live & ((jo < 0) | (jo >= N))).any())
        self.live &= (jo >= 0) & (jo < N)
        self.E, self.N = E, N
        i = back[np.arange(E) + int(offset)]
        j = back[np.where(self.live, jo, 0)]
        xi = np.broadcast_to(pos[i][:, None, :], (E, SLOTS, 3))
        xj = pos[j]
        s = f32(sim_scale)
        v = ((xi - xj) * s).astype(np.float32)
        vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
        r = np.sqrt(((vx * vx + vy * vy) + vz * vz) + f32(0.0) * f32(0.0)).astype(np.float32)
        L0 = conn[:, :, 1]
        dr = (r - L0).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(L0 > 0, (dr / L0).astype(np.float32), f32(0.0)).astype(np.float32)
        m = np.where((mz >= 1) & (mz <= int(muscle_count)), mz, 0)
        sig = np.where(m > 0, signal[np.clip(m - 1, 0, signal.shape[0] - 1)], f32(0.0)).astype(np.float32)
        self.has_s = self.live & (r != 0)
        self.has_c = self.has_s & (m > 0) & (sig > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (-(v / r[..., None])).astype(np.float32)
            sp = ((u * dr[..., None]).astype(np.float32) * K_SPRING).astype(np.float32)
            co = ((u * sig[..., None]).astype(np.float32) * K_MUSCLE).astype(np.float32)
        z = f32(0.0)
        lv = self.live
        self.owner = i
        self.xi = np.where(lv[..., None], xi, z).astype(np.float32)
        self.r, self.L0, self.dr, self.e = (np.where(lv, a, z).astype(np.float32) for a in (r, L0, dr, e))
        self.m = np.where(lv, m, 0)
        self.sig = np.where(lv, sig, z).astype(np.float32)
        self.s = np.where(self.has_s[..., None], sp, z).astype(np.float32)
        self.c = np.where(self.has_c[..., None], co, z).astype(np.float32)


def _canon(x):
    return f32(x) + f32(0.0)


def elastic_records(c):
    """(sorted_index int32[E], records float32[E, 12], connections float32[E, 32, 2]) of sph_elastic_measure."""
    rec = np.zeros((c.E, ELASTIC_WORDS), np.float32)
    for row in range(c.E):
        e_sum = d2 = f32(0.0)
        s = [f32(0.0)] * 3
        cc = [f32(0.0)] * 3
        n = nm = 0
        mn, mx = f32(np.inf), f32(-np.inf)
        for k in range(SLOTS):
            if not c.live[row, k]:
                continue
            n += 1
            nm += int(c.m[row, k] > 0)
            e = c.e[row, k]
            mn = e if e < mn else mn
            mx = e if e > mx else mx
            e_sum = f32(e_sum + e)
            d2 = f32(d2 + f32(c.dr[row, k] * c.dr[row, k]))
            if c.has_s[row, k]:
                s = [f32(s[a] + c.s[row, k, a]) for a in range(3)]
            if c.has_c[row, k]:
                cc = [f32(cc[a] + c.c[row, k, a]) for a in range(3)]
        rec[row] = [n, nm, _canon(mn) if n else 0, _canon(mx) if n else 0, e_sum, d2] + s + cc
    con = np.stack([np.where(c.live, c.r, f32(-1.0)), np.where(c.live, c.dr, f32(0.0))], axis=-1).astype(np.float32)
    return c.owner.astype(np.int32), rec, con


def elastic_records_fast(c):
    """elastic_records with the slot loop vectorised over the rows (the same float32 additions in the same order)."""
    E = c.E
    rec = np.zeros((E, ELASTIC_WORDS), np.float32)
    acc = np.zeros((E, 8), np.float32)  # eSum, d2, s.xyz, c.xyz
    mn, mx = np.full(E, np.inf, np.float32), np.full(E, -np.inf, np.float32)
    for k in range(SLOTS):
        lv = c.live[:, k]
        e = c.e[:, k]
        mn = np.where(lv & (e < mn), e, mn)
        mx = np.where(lv & (e > mx), e, mx)
        d2 = (c.dr[:, k] * c.dr[:, k]).astype(np.float32)
        acc[:, 0] = np.where(lv, acc[:, 0] + e, acc[:, 0])
        acc[:, 1] = np.where(lv, acc[:, 1] + d2, acc[:, 1])
        for a in range(3):
            acc[:, 2 + a] = np.where(c.has_s[:, k], acc[:, 2 + a] + c.s[:, k, a], acc[:, 2 + a])
            acc[:, 5 + a] = np.where(c.has_c[:, k], acc[:, 5 + a] + c.c[:, k, a], acc[:, 5 + a])
    n = c.live.sum(1)
    rec[:, 0] = n
    rec[:, 1] = (c.live & (c.m > 0)).sum(1)
    rec[:, 2] = np.where(n > 0, mn + f32(0.0), f32(0.0))
    rec[:, 3] = np.where(n > 0, mx + f32(0.0), f32(0.0))
    rec[:, 4:] = acc
    con = np.stack([np.where(c.live, c.r, f32(-1.0)), np.where(c.live, c.dr, f32(0.0))], axis=-1).astype(np.float32)
    return c.owner.astype(np.int32), rec, con


def muscle_records(c, muscle_count, signal, groups=None):
    """float64[muscle_count + 1, 16] of sph_muscle_diagnostics (`groups`: compute only these records, the others stay 0)."""
    signal = np.zeros(int(muscle_count), np.float32) if signal is None else np.asarray(signal, np.float32).reshape(-1)
    out = np.zeros((int(muscle_count) + 1, MUSCLE_WORDS), np.float64)
    flat = lambda a: np.asarray(a).reshape(-1)
    live, m = flat(c.live), flat(c.m)
    d2 = (c.dr * c.dr).astype(np.float32)
    spring = (c.dr * K_SPRING).astype(np.float32)
    contr = np.where((c.r != 0) & (c.sig > 0), (c.sig * K_MUSCLE).astype(np.float32), f32(0.0)).astype(np.float32)
    zero_len = (c.r == 0).astype(np.float32)
    terms = {2: c.L0, 3: c.r, 4: c.dr, 5: d2, 6: c.e, 9: spring, 10: contr, 11: c.xi[..., 0], 12: c.xi[..., 1], 13: c.xi[..., 2],
             14: zero_len}
    present = set(np.unique(m[live]).tolist())
    for g in (range(int(muscle_count) + 1) if groups is None else groups):
        out[g, 1] = float(signal[g - 1]) if g > 0 else 0.0
        if g not in present:
            continue  # every term is +0.0: so is every sum of the tree
        sel = live & (m == g)
        out[g, 0] = diag_ref.tree_sum(sel.astype(np.float64))
        for w, a in terms.items():
            out[g, w] = diag_ref.tree_sum(np.where(sel, flat(a).astype(np.float64), 0.0))
        e = flat(c.e)[sel]
        out[g, 7], out[g, 8] = np.float64(_canon(e.min())), np.float64(_canon(e.max()))
    return out


def membrane_records(sorted_pos, back, membranes):
    """(records float32[M, 8], totals float64[4]) of sph_membrane_measure."""
    pos = np.asarray(sorted_pos, np.float32).reshape(-1, np.asarray(sorted_pos).shape[-1])[:, :3]
    back = np.asarray(back).astype(np.int64).reshape(-1)
    tri = np.asarray(membranes, np.int64).reshape(-1, 3)
    a, b, c = (pos[back[tri[:, k]]] for k in range(3))
    e1, e2 = (b - a).astype(np.float32), (c - a).astype(np.float32)
    nx = (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]).astype(np.float32)
    ny = (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]).astype(np.float32)
    nz = (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]).astype(np.float32)
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz).astype(np.float32)
    area = (f32(0.5) * ln).astype(np.float32)
    rec = np.zeros((tri.shape[0], MEMBRANE_WORDS), np.float32)
    rec[:, 0] = area
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, n in enumerate((nx, ny, nz)):
            rec[:, 1 + k] = np.where(ln == 0, f32(0.0), (n / ln).astype(np.float32))
    rec[:, 4:7] = (((a + b).astype(np.float32) + c).astype(np.float32) / f32(3.0)).astype(np.float32)
    totals = np.zeros(4, np.float64)
    totals[0] = tri.shape[0]
    totals[1] = diag_ref.tree_sum(area.astype(np.float64))
    if tri.shape[0]:
        totals[2], totals[3] = np.float64(_canon(area.min())), np.float64(_canon(area.max()))
    return rec, totals


def solver_inputs(hip, scene, signal=None):
    """Connections of a GPU solver's last completed step: its exported sorted positions and particleIndexBack, the scene's table."""
    cfg = scene["cfg"]
    sp = hip.buffer("sortedPosition").reshape(-1, 4)[:hip.N]
    back = hip.buffer("particleIndexBack")[:hip.N]
    c = Connections(sp, back, scene["elastic"], cfg.elasticOffset, cfg.simulationScale, cfg.muscleCount, signal)
    return sp, back, c
