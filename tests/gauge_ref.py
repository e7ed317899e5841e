"""numpy restatement of the flow-gauge contract (include/sphmi.h, sph_gauge_define / sph_gauges_accumulate / sph_gauge_crossings).

Works from the contract alone: everything in float64, one operation at a time in the written order (numpy never contracts), the 16
sums of a record in the fixed tree of diag_ref.tree_sum over ascending sorted index. A state is a dict: "a" float32[N, 4], the
sorted positions of the step (sortedPosition, .w the type); "orig" int[N], the original id of every sorted particle
(particleIndex); "pos" / "vel" float32[N, 4], position and velocity after the step in original-id order; "fields" {slot:
float32[N]} in original-id order. A gauge is a dict with origin, u, v and optionally types, field, plane (the arguments of
owHIPSolver.gauge_define)."""
import numpy as np

import diag_ref

f64 = np.float64
MAX_GAUGES = 16
WORDS = 16
TOTAL_WORDS = 20


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f64)


def derive(g):
    """o, n, nn, A, B of the contract, float64, from the float32 words of the definition."""
    o, u, v = (np.asarray(g[k], np.float32).astype(f64) for k in ("origin", "u", "v"))
    n = _cross(u, v)
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        A, B = _cross(v, n) / nn, _cross(n, u) / nn
    return dict(o=o, n=n, nn=nn, A=A, B=B)


def valid(g, live_fields=()):
    """What sph_gauge_define accepts."""
    words = np.concatenate([np.asarray(g[k], np.float32).reshape(-1) for k in ("origin", "u", "v")])
    if words.size != 9 or not np.isfinite(words).all():
        return False
    nn = derive(g)["nn"]
    if not (nn > 0 and np.isfinite(nn)):
        return False
    mask = diag_ref.type_mask(g.get("types", (1,)))
    if mask == 0 or mask & ~0x6:
        return False
    return g.get("field") is None or g["field"] in live_fields


def _side(D, p):
    o, n = D["o"], D["n"]
    return (n[0] * (p[:, 0] - o[0]) + n[1] * (p[:, 1] - o[1])) + n[2] * (p[:, 2] - o[2])


class Crossings:
    """Per sorted particle, for one gauge: direction int[N] (+1, -1, 0: not counted), t, alpha, beta float64[N] (nan where the
    particle does not cross the plane), crossed bool[N]: crossed the plane, counted or not."""

    def __init__(self, state, g):
        a4 = np.asarray(state["a"], np.float32).reshape(-1, 4)
        orig = np.asarray(state["orig"], np.int64)
        b4 = np.asarray(state["pos"], np.float32).reshape(-1, 4)[orig]
        N = a4.shape[0]
        D = derive(g)
        a, b = a4[:, :3].astype(f64), b4[:, :3].astype(f64)
        with np.errstate(invalid="ignore"):
            types = np.trunc(a4[:, 3]).astype(np.int64)  # (int)position.w
            mask = diag_ref.type_mask(g.get("types", (1,)))
            considered = (types >= 1) & (types <= 2) & (((1 << np.clip(types, 0, 31)) & mask) != 0)
            sa, sb = _side(D, a), _side(D, b)
            plus = considered & (sa < 0) & (sb >= 0)
            minus = considered & (sa >= 0) & (sb < 0)
        crossed = plus | minus
        t, alpha, beta = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
        k = np.flatnonzero(crossed)
        tk = sa[k] / (sa[k] - sb[k])
        x = [a[k, c] + tk * (b[k, c] - a[k, c]) for c in range(3)]
        o = D["o"]
        for out, V in ((alpha, D["A"]), (beta, D["B"])):
            out[k] = (V[0] * (x[0] - o[0]) + V[1] * (x[1] - o[1])) + V[2] * (x[2] - o[2])
        t[k] = tk
        with np.errstate(invalid="ignore"):
            inside = crossed if g.get("plane") else crossed & (0 <= alpha) & (alpha < 1) & (0 <= beta) & (beta < 1)
        self.direction = np.where(inside & plus, 1, np.where(inside & minus, -1, 0))
        self.t, self.alpha, self.beta, self.crossed = t, alpha, beta, crossed
        self.orig = orig


def terms(state, g, C=None):
    """float64[16, N]: the per-particle terms of the record's words."""
    C = C or Crossings(state, g)
    orig = C.orig
    w = np.asarray(state["vel"], np.float32).reshape(-1, 4)[orig, :3].astype(f64)
    field = g.get("field")
    c = np.zeros(orig.size) if field is None else np.asarray(state["fields"][field], np.float32)[orig].astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        v2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    q = [np.ones(orig.size), w[:, 0], w[:, 1], w[:, 2], v2, c, C.alpha, C.beta]
    out = np.zeros((WORDS, orig.size), f64)
    for half, way in ((0, 1), (8, -1)):
        on = C.direction == way
        for k in range(8):
            out[half + k] = np.where(on, q[k], 0.0)
    return out


def record(state, g, C=None):
    """float64[16] of one gauge."""
    t = terms(state, g, C)
    out = np.zeros(WORDS, f64)
    for w in range(WORDS):
        if t[w].any() or np.isnan(t[w]).any():
            out[w] = diag_ref.tree_sum(t[w])
    return out  # (a word whose terms are all zero is +0.0, whatever the zeros' signs: the sign of a zero total is no contract)


def records(state, gauges):
    """float64[16, 16]: gauges = {slot: gauge}; a free slot is all +0.0."""
    out = np.zeros((MAX_GAUGES, WORDS), f64)
    for slot, g in gauges.items():
        out[slot] = record(state, g)
    return out


def empty_totals():
    t = np.zeros((MAX_GAUGES, TOTAL_WORDS), f64)
    t[:, 17:] = -1.0
    return t


def accumulate(totals, recs, defined, call):
    """totals after call number `call` with records `recs`; defined: the slots that took part."""
    t = totals.copy()
    for g in defined:
        t[g, :WORDS] = t[g, :WORDS] + recs[g]
        t[g, 16] = t[g, 16] + 1.0
        plus, minus = recs[g, 0] > 0, recs[g, 8] > 0
        if plus and t[g, 17] < 0:
            t[g, 17] = float(call)
        if minus and t[g, 18] < 0:
            t[g, 18] = float(call)
        if plus or minus:
            t[g, 19] = float(call)
    return t


def crossing_list(state, g):
    """(sorted index int32[n], original id uint32[n], direction int32[n], float32[n, 3] t alpha beta) of sph_gauge_crossings."""
    C = Crossings(state, g)
    idx = np.flatnonzero(C.direction != 0)
    tab = np.stack([C.t[idx], C.alpha[idx], C.beta[idx]], axis=1).astype(np.float32).reshape(-1, 3)
    return idx.astype(np.int32), C.orig[idx].astype(np.uint32), C.direction[idx].astype(np.int32), tab


def zero_sign_blind(x):
    """The bit patterns of float64 `x` with -0.0 mapped to +0.0 (the sign of a zero total is not part of the contract)."""
    return (np.asarray(x, f64) + 0.0).view(np.uint64)


def side_count(pos4, g, types=(1,)):
    """The number of particles of `types` in pos4 (float32[N, 4], any order) with s(p) >= 0: the half-space behind the gauge's plane."""
    p4 = np.asarray(pos4, np.float32).reshape(-1, 4)
    D = derive(g)
    with np.errstate(invalid="ignore"):
        ty = np.trunc(p4[:, 3]).astype(np.int64)
        ok = np.isin(ty, list(types))
        return int((ok & (_side(D, p4[:, :3].astype(f64)) >= 0)).sum())


def oracle_state(ora, N, fields=None):
    """The state of the oracle's last step (reference layouts)."""
    orig = ora.buffer("particleIndex").reshape(-1, 2)[:N, 1].astype(np.int64)
    pos = ora.buffer("position").reshape(-1, 4)[:N].copy()
    return dict(a=_sorted_with_type(ora.buffer("sortedPosition"), pos, orig, N), orig=orig, pos=pos,
                vel=ora.buffer("velocity").reshape(-1, 4)[:N].copy(), fields=fields or {})


def _sorted_with_type(sorted_position, pos, orig, N):
    """sortedPosition in the reference layout carries the cell id in .w; the library's array carries the type, which no step
    changes: position[orig].w."""
    a = np.asarray(sorted_position, np.float32).reshape(-1, 4)[:N].copy()
    a[:, 3] = pos[orig, 3]
    return a


def solver_state(hip, fields=None):
    """The same state from the solver's exported buffers."""
    N = hip.N
    orig = hip.read_particleIndex_buffer()[:, 1].astype(np.int64)
    pos = hip.read_position_buffer().copy()
    return dict(a=_sorted_with_type(hip.buffer("sortedPosition"), pos, orig, N), orig=orig, pos=pos,
                vel=hip.read_velocity_buffer().copy(), fields={k: hip.field_read(k).copy() for k in (fields or ())})
