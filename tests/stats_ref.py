"""numpy float64 restatement of the time statistics on a lattice (include/sphmi.h, sph_stats_*): the fold of one call's records into
the 24 accumulators of every node, and the 16 moment words. The records come from sample_ref.sample_reference (or from the device's
own sph_sample_grid); everything here works from the header's tables alone."""
import numpy as np

import sample_ref

WORDS, MOMENT_WORDS = 24, 16
CALL_WORDS = (1, 2, 17, 19, 21, 23)
INF = np.inf


def empty(nodes):
    """float64[nodes, 24] of the empty values."""
    a = np.zeros((int(nodes), WORDS), np.float64)
    a[:, list(CALL_WORDS)] = -1.0
    a[:, [16, 18, 20]] = -INF
    a[:, 22] = INF
    return a


def fold(acc, records, call):
    """Record r of call `call` (0-based) folded into acc, node by node; records float32[nodes, 8]. Returns a new array."""
    a = np.array(acc, np.float64).reshape(-1, WORDS)
    r = np.asarray(records, np.float32).reshape(-1, 8)
    assert a.shape[0] == r.shape[0]
    c = np.float64(call)
    wet = r[:, 6] > 0
    rho, vx, vy, vz, p = (r[:, w].astype(np.float64) for w in (0, 2, 3, 4, 5))
    with np.errstate(all="ignore"):
        new = a.copy()
        new[:, 0] = a[:, 0] + 1.0
        new[:, 1] = np.where(a[:, 1] < 0, c, a[:, 1])
        new[:, 2] = c
        new[:, 3] = a[:, 3] + rho
        new[:, 4] = a[:, 4] + rho * rho
        new[:, 5], new[:, 6], new[:, 7] = a[:, 5] + vx, a[:, 6] + vy, a[:, 7] + vz
        for w, (u, v) in enumerate(((vx, vx), (vy, vy), (vz, vz), (vx, vy), (vx, vz), (vy, vz))):
            new[:, 8 + w] = a[:, 8 + w] + u * v
        new[:, 14] = a[:, 14] + p
        new[:, 15] = a[:, 15] + p * p
        q = (vx * vx + vy * vy) + vz * vz
        for w, x, greater in ((16, rho, True), (18, q, True), (20, p, True), (22, p, False)):
            take = (x > a[:, w]) if greater else (x < a[:, w])  # (false for a NaN)
            new[:, w] = np.where(take, x, a[:, w])
            new[:, w + 1] = np.where(take, c, a[:, w + 1])
    return np.where(wet[:, None], new, a)


def moments64(acc, calls):
    """The moment words before their cast to float: float64[nodes, 16]. calls >= 1."""
    a = np.asarray(acc, np.float64).reshape(-1, WORDS)
    assert calls >= 1
    C = np.float64(calls)
    n = a[:, 0]
    m = np.zeros((a.shape[0], MOMENT_WORDS), np.float64)
    m[:, 14] = -1.0
    with np.errstate(all="ignore"):
        m[:, 0] = n / C
        mr = a[:, 3] / C
        m[:, 1] = mr
        m[:, 2] = a[:, 4] / C - mr * mr
        w = n > 0
        nw = n[w]
        mean = [a[w, 5 + k] / nw for k in range(3)]
        for k in range(3):
            m[w, 3 + k] = mean[k]
        for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            m[w, 6 + k] = a[w, 8 + k] / nw - mean[i] * mean[j]
        mp = a[w, 14] / nw
        m[w, 12] = mp
        m[w, 13] = a[w, 15] / nw - mp * mp
        m[w, 14] = a[w, 1]
        m[w, 15] = a[w, 20]
    return m


def moments(acc, calls):
    with np.errstate(all="ignore"):
        return moments64(acc, calls).astype(np.float32)


def lattice_records(state, lattice, types=None):
    """float32[nodes, 8]: the records sph_sample_grid returns on the lattice dict (origin, spacing, dims, typeMask), x fastest."""
    if types is None:
        types = tuple(t for t in (1, 2, 3) if lattice["typeMask"] >> t & 1)
    pts = sample_ref.grid_points(lattice["origin"], lattice["spacing"], lattice["dims"]).reshape(-1, 3)
    return sample_ref.sample_reference(state, pts, types)
