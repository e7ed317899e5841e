"""numpy float32 restatement of the field-sampling contract (include/sphmi.h, sph_sample_points / sph_sample_grid).

Works from the contract alone: the selected set is found by brute force over a float64 bucket grid of its own (bucket edge
just above h, floor-based: unrelated to the solver's truncating 2h cell hash), then ordered by sorted index and accumulated
with sequential float32 operations, vectorised across points. It does not reuse the solver's cell walk, so it checks the
cell-range and dedupe logic of the kernels independently."""
import numpy as np

f32 = np.float32


def solver_state(hip):
    """The sorted state of the last completed step, from the exported buffers: positions (x, y, z), velocities, rho, pressure,
    particle types and masked cell keys, all in sorted order."""
    N = hip.N
    sp = np.empty(8 * N, np.float32)
    hip._chk(hip._L.sph_read_buffer(hip._h, b"sortedPosition", sp.ctypes.data, sp.nbytes, None))
    sv = np.empty(4 * N, np.float32)
    hip._chk(hip._L.sph_read_buffer(hip._h, b"sortedVelocity", sv.ctypes.data, sv.nbytes, None))
    rho = np.empty(2 * N, np.float32)
    hip._chk(hip._L.sph_read_buffer(hip._h, b"rho", rho.ctypes.data, rho.nbytes, None))
    pr = np.empty(N, np.float32)
    hip._chk(hip._L.sph_read_buffer(hip._h, b"pressure", pr.ctypes.data, pr.nbytes, None))
    pi = hip.read_particleIndex_buffer()
    # sortedPosition.w holds the cell id in the reference's layout: the type comes from the orig-order position
    types = hip.read_position_buffer()[pi[:, 1], 3]
    cfg = hip.cfg
    return dict(pos=sp.reshape(-1, 4)[:N, :3].copy(), vel=sv.reshape(-1, 4)[:, :3].copy(), rho=rho[:N].copy(), p=pr,
                types=types, keys=pi[:, 0].copy(), G=int(cfg.gridCellCount), h=float(cfg.h),
                simScale=float(cfg.simulationScale), massWpoly6=float(cfg.mass) * float(cfg.Wpoly6Coefficient))


def type_mask(types):
    m = 0
    for t in types:
        m |= 1 << int(t)
    return m


def candidate_pairs(pos, points, radius):
    """(point index, particle index) for every particle within `radius` (float64, with margin) of a point: floor buckets of
    edge `radius`, 27 neighbouring buckets per point."""
    pos = np.asarray(pos, np.float64)
    pts = np.asarray(points, np.float64)
    b = float(radius)
    lo = np.floor(np.minimum(pos.min(0), pts.min(0)) / b) - 2 if pts.size else np.floor(pos.min(0) / b) - 2
    pb = (np.floor(pos / b) - lo).astype(np.int64)
    qb = (np.floor(pts / b) - lo).astype(np.int64)
    M = int(max(pb.max(), qb.max() if qb.size else 0)) + 3
    pkey = (pb[:, 0] * M + pb[:, 1]) * M + pb[:, 2]
    order = np.argsort(pkey, kind="stable")
    skey = pkey[order]
    P, J = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                k = ((qb[:, 0] + ox) * M + (qb[:, 1] + oy)) * M + (qb[:, 2] + oz)
                a = np.searchsorted(skey, k, "left")
                e = np.searchsorted(skey, k, "right")
                cnt = e - a
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                pt = np.repeat(np.arange(len(k)), cnt)
                start = np.repeat(a - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
                P.append(pt)
                J.append(order[start + np.arange(tot)])
    if not P:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(P), np.concatenate(J)


def sample_reference(state, points, types=(1, 2, 3)):
    """float32[Q, 8] records of the contract for `points` ([Q, >=3]) over `state` (solver_state())."""
    pts = np.asarray(points, np.float32).reshape(-1, np.asarray(points).shape[-1])[:, :3]
    Q = pts.shape[0]
    out = np.zeros((Q, 8), np.float32)
    h = f32(state["h"])
    hh = h * h
    ss2 = f32(state["simScale"]) * f32(state["simScale"])
    hs = h * f32(state["simScale"])
    hs2 = hs * hs
    mwp = f32(state["massWpoly6"])
    finite = np.isfinite(pts).all(1)
    fidx = np.flatnonzero(finite)
    if fidx.size == 0:
        return out
    m = type_mask(types)
    t = state["types"].astype(np.int32)
    sel_particle = ((np.left_shift(1, np.clip(t, 0, 31)) & m) != 0) & (t >= 0) & (t <= 31) & (state["keys"] < state["G"])
    pidx, j = candidate_pairs(state["pos"], pts[fidx], float(state["h"]) * 1.001)
    keep = sel_particle[j]
    pidx, j = pidx[keep], j[keep]
    x = state["pos"][j]
    q = pts[fidx][pidx]
    dx, dy, dz = q[:, 0] - x[:, 0], q[:, 1] - x[:, 1], q[:, 2] - x[:, 2]
    r2 = dx * dx + dy * dy + dz * dz
    keep = r2 < hh
    pidx, j, r2 = pidx[keep], j[keep], r2[keep]
    # ascending sorted index within each point; pad into [points, max hits]
    o = np.lexsort((j, pidx))
    pidx, j, r2 = pidx[o], j[o], r2[o]
    Qf = fidx.size
    n = np.bincount(pidx, minlength=Qf)
    W = np.zeros(Qf, np.float32)
    S = np.zeros(Qf, np.float32)
    U = np.zeros((Qf, 3), np.float32)
    P = np.zeros(Qf, np.float32)
    if j.size:
        first = np.concatenate([[0], np.cumsum(n)[:-1]])
        rank = np.arange(j.size) - first[pidx]
        K = int(n.max())
        a = hs2 - r2 * ss2
        w = a * a * a
        v = w * (f32(1) / state["rho"][j])
        colW = np.zeros((Qf, K), np.float32)
        colV = np.zeros((Qf, K), np.float32)
        colU = np.zeros((Qf, K, 3), np.float32)
        colP = np.zeros((Qf, K), np.float32)
        has = np.zeros((Qf, K), bool)
        colW[pidx, rank] = w
        colV[pidx, rank] = v
        colU[pidx, rank] = v[:, None] * state["vel"][j]
        colP[pidx, rank] = v * state["p"][j]
        has[pidx, rank] = True
        for k in range(K):
            hk = has[:, k]
            W = np.where(hk, W + colW[:, k], W)
            S = np.where(hk, S + colV[:, k], S)
            U = np.where(hk[:, None], U + colU[:, k], U)
            P = np.where(hk, P + colP[:, k], P)
    rec = np.zeros((Qf, 8), np.float32)
    rec[:, 0] = mwp * W
    rec[:, 1] = mwp * S
    nz = S != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rec[nz, 2] = U[nz, 0] / S[nz]
        rec[nz, 3] = U[nz, 1] / S[nz]
        rec[nz, 4] = U[nz, 2] / S[nz]
        rec[nz, 5] = P[nz] / S[nz]
    rec[:, 6] = n.astype(np.float32)
    out[fidx] = rec
    return out


def grid_points(origin, spacing, dims):
    """The lattice of sph_sample_grid as [nz, ny, nx, 3] float32: origin + (float)i * spacing per axis."""
    o = np.asarray(origin, np.float32)
    s = np.asarray(spacing, np.float32)
    nx, ny, nz = (int(d) for d in dims)
    xs = o[0] + np.arange(nx, dtype=np.float32) * s[0]
    ys = o[1] + np.arange(ny, dtype=np.float32) * s[1]
    zs = o[2] + np.arange(nz, dtype=np.float32) * s[2]
    g = np.empty((nz, ny, nx, 3), np.float32)
    g[..., 0] = xs[None, None, :]
    g[..., 1] = ys[None, :, None]
    g[..., 2] = zs[:, None, None]
    return g


def axis_cell_range(c, h, cell_size_inv):
    """float32 restatement of the kernels' sample_axis_range (sph_sample_walk.h): the cell range [lo, hi] of one axis that
    holds every particle the coordinates `c` can select."""
    c = np.asarray(c, np.float32)
    h, inv = f32(h), f32(cell_size_inv)
    ul, uh = (c - h) * inv, (c + h) * inv
    ul = ul - np.minimum(np.abs(ul) * f32(2.0 ** -21) + f32(2.0 ** -10), f32(0.5))
    uh = uh + np.minimum(np.abs(uh) * f32(2.0 ** -21) + f32(2.0 ** -10), f32(0.5))
    lo = np.trunc(np.clip(ul, f32(-2.0 ** 30), f32(2.0 ** 30))).astype(np.int64)
    hi = np.trunc(np.clip(uh, f32(-2.0 ** 30), f32(2.0 ** 30))).astype(np.int64)
    return lo, np.minimum(hi, lo + 3)


def brick_box_cells(origin, spacing, dims, h, cell_size_inv):
    """Cells in the box of every 4x4x4 brick of the lattice (finite points only), as the brick walk forms it: the union of
    its points' axis_cell_range per axis. int64[nbz, nby, nbx]; a box above 64 cells takes the walk's per-lane form."""
    g = grid_points(origin, spacing, dims)
    widths = []
    for axis, coords in enumerate((g[0, 0, :, 0], g[0, :, 0, 1], g[:, 0, 0, 2])):
        lo, hi = axis_cell_range(coords, h, cell_size_inv)
        widths.append(np.array([hi[b:b + 4].max() - lo[b:b + 4].min() + 1 for b in range(0, len(coords), 4)], np.int64))
    return widths[2][:, None, None] * widths[1][None, :, None] * widths[0][None, None, :]


def brute_force_f64(pos, vel, rho, p, types, points, h, sim_scale, mass_wpoly6, types_sel=(1, 2, 3)):
    """The same interpolation in float64 with a plain all-pairs loop over points (for small clouds): density, shepard,
    velocity, pressure, count."""
    pos = np.asarray(pos, np.float64)
    out = np.zeros((len(points), 8))
    tsel = np.isin(np.asarray(types).astype(np.int32), list(types_sel))
    hs2 = (h * sim_scale) ** 2
    for i, q in enumerate(np.asarray(points, np.float64)):
        r2 = ((pos - q[:3]) ** 2).sum(1)
        s = tsel & (r2 < h * h)
        w = (hs2 - r2[s] * sim_scale ** 2) ** 3
        v = w / np.asarray(rho, np.float64)[s]
        out[i, 0] = mass_wpoly6 * w.sum()
        out[i, 1] = mass_wpoly6 * v.sum()
        if v.sum() != 0:
            out[i, 2:5] = (v[:, None] * np.asarray(vel, np.float64)[s]).sum(0) / v.sum()
            out[i, 5] = (v * np.asarray(p, np.float64)[s]).sum() / v.sum()
        out[i, 6] = s.sum()
    return out
