"""numpy restatement of the surface-measure contract (include/sphmi.h, sph_measure_surface / sph_read_shells): shells by a plain
union-find, open sides from the set of directed sides, the per-triangle terms in double, their quantisation to exact int64
sums, and the float boxes.

measure(verts, tris, origin, spacing, dims) -> dict(vertexShell int32[V], table int64[S, 10], bbox float32[S, 6],
counts int64[4], exps int32[3]); table columns are named by FIELDS."""
import math

import numpy as np

WORDS = 10
FIELDS = ("root", "vertices", "triangles", "open", "bad", "a2", "d6", "mx", "my", "mz")


def shells(tris, V):
    """(vertexShell int64[V], roots int64[S]): components of the graph of the triangles' sides, numbered by ascending root."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(tris, np.int64).tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    roots = np.array([find(v) for v in range(V)], np.int64)
    ur = np.unique(roots)
    return np.searchsorted(ur, roots), ur


def open_sides(tris):
    """The contract's definition: the start vertex of every directed side (a, b) of a triangle for which no triangle has the
    side (b, a); one entry per such side of a triangle."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    have = set(zip(a.tolist(), b.tolist()))
    return np.array([x for x, y in zip(a.tolist(), b.tolist()) if (y, x) not in have], np.int64)


def open_vertices_by_sum(tris, V):
    """The kernel's method: bool[V], vertices whose sum of (next - prev) over the triangles at the vertex is not zero."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    d = np.zeros(V, np.int64)
    for k in range(3):
        np.add.at(d, t[:, k], t[:, (k + 1) % 3] - t[:, (k + 2) % 3])
    return d != 0


def exponents(T, spacing, dims):
    """(bT, kA, kV, kM) for a mesh of T triangles cut on a lattice of float32 `spacing` and integer `dims`."""
    sp = np.abs(np.asarray(spacing, np.float32).astype(np.float64))
    ext = max((int(dims[a]) - 1) * float(sp[a]) for a in range(3))
    big = float(sp.max())
    eL = 1 + (math.frexp(ext)[1] if math.isfinite(ext) and ext != 0.0 else 0)
    eS = 1 + (math.frexp(big)[1] if math.isfinite(big) and big != 0.0 else 0)
    bT = int(T).bit_length()  # ceil(log2(T + 1))
    return bT, 60 - bT - 2 * eS, 59 - bT - eL - 2 * eS, 58 - bT - eL - 2 * eS


def triangle_terms(verts, tris, origin):
    """float64[T, 5]: a2, d6, mx, my, mz of every triangle, in the contract's order of operations."""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3) - np.asarray(origin, np.float32).astype(np.float64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    p0, p1, p2 = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
        d6 = (p0[:, 0] * nx + p0[:, 1] * ny) + p0[:, 2] * nz
        m = a2[:, None] * ((p0 + p1) + p2)
    return np.concatenate([a2[:, None], d6[:, None], m], axis=1)


def quantise(terms, exps, bT):
    """(q int64[T, 5], bad bool[T]): q = rint(ldexp(x, k)); a triangle is bad unless all five scaled terms are below
    2^(62 - bT) in magnitude (a non-finite term is not)."""
    k = np.array([exps[0], exps[1], exps[2], exps[2], exps[2]], np.int64)
    with np.errstate(all="ignore"):
        scaled = np.ldexp(terms, k[None, :].astype(np.int32))
        ok = (np.abs(scaled) < math.ldexp(1.0, 62 - bT)).all(axis=1)
        q = np.where(ok[:, None], np.rint(np.where(ok[:, None], scaled, 0.0)), 0.0).astype(np.int64)
    return q, ~ok


def _ordered(f):
    i = np.ascontiguousarray(f, np.float32).view(np.int32)
    return i ^ ((i >> 31) & 0x7fffffff)


def _unordered(i):
    i = np.asarray(i, np.int32)
    return (i ^ ((i >> 31) & 0x7fffffff)).view(np.float32) + np.float32(0.0)


def measure(verts, tris, origin, spacing, dims):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    V, T = verts.shape[0], tris.shape[0]
    bT, kA, kV, kM = exponents(T, spacing, dims)
    exps = np.array([kA, kV, kM], np.int32)
    lab, roots = shells(tris, V)
    S = roots.shape[0]
    table = np.zeros((S, WORDS), np.int64)
    bbox = np.zeros((S, 6), np.float32)
    table[:, 0] = roots
    table[:, 1] = np.bincount(lab, minlength=S)[:S] if V else 0
    if T:
        ts = lab[tris[:, 0].astype(np.int64)]
        table[:, 2] = np.bincount(ts, minlength=S)
        table[:, 3] = np.bincount(lab[open_sides(tris)], minlength=S)
        q, bad = quantise(triangle_terms(verts, tris, origin), exps, bT)
        table[:, 4] = np.bincount(ts[bad], minlength=S)
        for w in range(5):
            np.add.at(table[:, 5 + w], ts, q[:, w])
    if V:
        img = _ordered(verts)
        lo = np.full((S, 3), 0x7fffffff, np.int32)
        hi = np.full((S, 3), -0x80000000, np.int32)
        for c in range(3):
            np.minimum.at(lo[:, c], lab, img[:, c])
            np.maximum.at(hi[:, c], lab, img[:, c])
        bbox[:, :3] = _unordered(lo)
        bbox[:, 3:] = _unordered(hi)
    counts = np.array([S, int((table[:, 3] == 0).sum()), int(table[:, 3].sum()), int(table[:, 4].sum())], np.int64)
    return {"vertexShell": lab.astype(np.int32), "table": table, "bbox": bbox, "counts": counts, "exps": exps}


def values(table, exps):
    """Per shell (area2 sum, d6 sum, m sums) as doubles: ldexp((double)sum, -k)."""
    t = np.asarray(table, np.int64).reshape(-1, WORDS)
    k = [exps[0], exps[1], exps[2], exps[2], exps[2]]
    return np.stack([np.ldexp(t[:, 5 + w].astype(np.float64), -int(k[w])) for w in range(5)], axis=1)
