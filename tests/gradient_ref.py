"""numpy float32 restatement of the gradient-sampling contract (include/sphmi.h, sph_sample_gradient_points /
sph_sample_gradient_grid / sph_surface_normals).

Words 0..7 are sample_ref.sample_reference's records, unchanged. The other words use the same brute-force selection
(sample_ref.candidate_pairs, then the type, cell-table and distance tests), order the hits by sorted index per point and
accumulate the 18 gradient sums with sequential float32 additions, one hit rank at a time across all points."""
import numpy as np

import sample_ref

f32 = np.float32
WORDS = 32


def _hits(state, pts, types):
    """(point index, particle index, dx, dy, dz, r2) of every selected pair, ordered by point then ascending sorted index."""
    m = sample_ref.type_mask(types)
    t = state["types"].astype(np.int32)
    sel_particle = ((np.left_shift(1, np.clip(t, 0, 31)) & m) != 0) & (t >= 0) & (t <= 31) & (state["keys"] < state["G"])
    pidx, j = sample_ref.candidate_pairs(state["pos"], pts, float(state["h"]) * 1.001)
    keep = sel_particle[j]
    pidx, j = pidx[keep], j[keep]
    x = state["pos"][j]
    q = pts[pidx]
    dx, dy, dz = q[:, 0] - x[:, 0], q[:, 1] - x[:, 1], q[:, 2] - x[:, 2]
    r2 = dx * dx + dy * dy + dz * dz
    h = f32(state["h"])
    keep = r2 < h * h
    o = np.lexsort((j[keep], pidx[keep]))
    return tuple(a[keep][o] for a in (pidx, j, dx, dy, dz, r2))


def gradient_scale(state):
    """K = (float)(-6 * massWpoly6 * simScale), the product taken in double."""
    return f32(-6.0 * float(state["massWpoly6"]) * float(f32(state["simScale"])))


def gradient_reference(state, points, types=(1, 2, 3)):
    """float32[Q, 32] records of the contract for `points` ([Q, >=3]) over `state` (sample_ref.solver_state())."""
    pts = np.asarray(points, np.float32).reshape(-1, np.asarray(points).shape[-1])[:, :3]
    Q = pts.shape[0]
    out = np.zeros((Q, WORDS), np.float32)
    out[:, :8] = sample_ref.sample_reference(state, pts, types)
    fidx = np.flatnonzero(np.isfinite(pts).all(1))
    if fidx.size == 0:
        return out
    ss2 = f32(state["simScale"]) * f32(state["simScale"])
    hs = f32(state["h"]) * f32(state["simScale"])
    hs2 = hs * hs
    pidx, j, dx, dy, dz, r2 = _hits(state, pts[fidx], types)
    Qf = fidx.size
    # per hit: S's term, then B (3), C (3), E_vx, E_vy, E_vz, E_p (3 each) in that column order
    t = hs2 - r2 * ss2
    g = t * t
    w = g * t
    inv = f32(1) / state["rho"][j]
    v = w * inv
    q = g * inv
    d = (dx, dy, dz)
    cols = [v] + [g * c for c in d] + [q * c for c in d]
    for A in (state["vel"][j, 0], state["vel"][j, 1], state["vel"][j, 2], state["p"][j]):
        a = q * A
        cols += [a * c for c in d]
    col = np.stack(cols, axis=1).astype(np.float32)
    acc = np.zeros((Qf, col.shape[1]), np.float32)
    if j.size:
        n = np.bincount(pidx, minlength=Qf)
        first = np.concatenate([[0], np.cumsum(n)[:-1]])
        rank = np.arange(j.size) - first[pidx]
        order = np.argsort(rank, kind="stable")
        bounds = np.searchsorted(rank[order], np.arange(int(n.max()) + 1))
        for k in range(int(n.max())):  # each point at most once per rank: a sequential float32 sum per point
            h_ = order[bounds[k]:bounds[k + 1]]
            acc[pidx[h_]] = acc[pidx[h_]] + col[h_]
    S, B, C, E = acc[:, 0], acc[:, 1:4], acc[:, 4:7], acc[:, 7:19].reshape(Qf, 4, 3)
    K = gradient_scale(state)
    rec = out[fidx]
    rec[:, 8:11] = K * B
    rec[:, 11:14] = K * C
    nz = S != 0
    Ub = rec[nz, 2:6]  # vx, vy, vz, p of the sample record
    Cn, En = C[nz], E[nz]
    G = np.empty((int(nz.sum()), 4, 3), np.float32)
    for i in range(4):
        for c in range(3):
            G[:, i, c] = K * (En[:, i, c] - Ub[:, i] * Cn[:, c])
    r = np.zeros((G.shape[0], 17), np.float32)
    r[:, 0:9] = G[:, :3].reshape(-1, 9)
    r[:, 9:12] = G[:, 3]
    r[:, 12] = G[:, 2, 1] - G[:, 1, 2]
    r[:, 13] = G[:, 0, 2] - G[:, 2, 0]
    r[:, 14] = G[:, 1, 0] - G[:, 0, 1]
    r[:, 15] = (G[:, 0, 0] + G[:, 1, 1]) + G[:, 2, 2]
    s = np.zeros(G.shape[0], np.float32)
    for i in range(3):
        for k in range(3):
            s = s + G[:, i, k] * G[:, k, i]
    r[:, 16] = f32(-0.5) * s
    rec[nz, 14:31] = r
    out[fidx] = rec
    return out


FIELD_WORDS = {0: 8, 1: 11, 2: 14, 3: 17, 4: 20, 5: 23}  # sph_extract_surface field -> first gradient word


def normals_reference(records, field):
    """float32[V, 3] normals of sph_surface_normals from the gradient records at the vertices."""
    w = FIELD_WORDS[int(field)]
    gr = np.asarray(records, np.float32)
    gx, gy, gz = gr[:, w], gr[:, w + 1], gr[:, w + 2]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = (ln != 0) & np.isfinite(ln)
        n = np.zeros((gr.shape[0], 3), np.float32)
        n[ok, 0] = -(gx[ok] / ln[ok])
        n[ok, 1] = -(gy[ok] / ln[ok])
        n[ok, 2] = -(gz[ok] / ln[ok])
    return n
