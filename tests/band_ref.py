"""The search bands of the fused step (csrc/sph_bands.hip) restated with numpy, float32 operation by float32
operation: the band radius, the flag byte of every sorted particle, the eight band arrays and their start tables — and the
statement the search kernel relies on, checked on a sorted state: every candidate of a y / z / yz neighbour cell within the
filter radius of a visiting particle is in the band the kernel stages for that row of cells.

Slot s of the kernel's row r = (sy + 1) + 3 (sz + 1), r != 4, is r - (r > 4); bit s of a flag byte is membership in band s:
    s      0        1     2        3     4     5        6     7
    (sy,sz)(-,-)    (0,-) (+,-)    (-,0) (+,0) (-,+)    (0,+) (+,+)     the step from the visiting particle's cell
    band   hiY&hiZ  hiZ   loY&hiZ  hiY   loY   hiY&loZ  loZ   loY&loZ   the face(s) of the candidate's own cell it is near"""
import numpy as np

F = np.float32
SLOT_STEP = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]  # (sy, sz) of slot s


def filter_r2(h):
    """binU[63] of sph_create: max(h, 31 h / 30)^2 (1 + 2^-20), every operation rounded to float32."""
    h = F(h)
    h2 = F(h * h)
    r = F(F(F(31.0) * h) / F(30.0))
    r2 = F(r * r)
    return F(max(r2, h2) * F(1.0 + 2.0 ** -20))


def band_radius(cfg):
    """sph_band_radius: Rf (1 + 2^-23) + L (kappa + 2^-22) in double, rounded up to float32."""
    rf = np.sqrt(np.float64(filter_r2(cfg.h)))
    cs, inv = np.float64(F(cfg.hashGridCellSize)), np.float64(F(cfg.hashGridCellSizeInv))
    kappa = abs(inv * cs - 1.0)
    L = cs * np.float64(max(cfg.gridCellsY, cfg.gridCellsZ) + 1)
    rb = rf * (1.0 + 2.0 ** -23) + L * (kappa + 2.0 ** -22)
    f = F(rb)
    if np.float64(f) < rb:
        f = np.nextafter(f, F(np.inf))
    return f


def premise(pos, keys, cfg):
    """True where the key is the id of the in-grid cell the coordinates truncate to (never where the id mask aliases cells)."""
    pos = np.asarray(pos, F)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (y >= 0) & (z >= 0) & (x < F(1.0e9)) & (y < F(1.0e9)) & (z < F(1.0e9))
    if cfg.gridCellCount > int(cfg.cellIdMask) + 1:  # the mask can change a cell id of the grid: keys are not cell ids
        ok[:] = False
    inv = F(cfg.hashGridCellSizeInv)
    safe = np.where(ok[:, None], pos[:, :3], F(0))
    c = (safe * inv).astype(F).astype(np.int64)  # truncation, as (int)(q * cellSizeInv)
    gx, gy, gz = cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellsZ
    ok &= (c[:, 0] < gx) & (c[:, 1] < gy) & (c[:, 2] < gz)
    ok &= np.asarray(keys, np.int64) == c[:, 0] + c[:, 1] * gx + c[:, 2] * gx * gy
    return ok, c


def band_flags(pos, keys, cfg, rb=None):
    """uint8[n]: the flag byte of every sorted particle (0xff where the premise fails)."""
    pos = np.asarray(pos, F)
    rb = band_radius(cfg) if rb is None else F(rb)
    ok, c = premise(pos, keys, cfg)
    cs = F(cfg.hashGridCellSize)
    y, z = pos[:, 1], pos[:, 2]
    cy, cz = c[:, 1].astype(F), c[:, 2].astype(F)
    cy1, cz1 = (c[:, 1] + 1).astype(F), (c[:, 2] + 1).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        loY = (y - (cy * cs).astype(F)).astype(F) <= rb
        hiY = ((cy1 * cs).astype(F) - y).astype(F) <= rb
        loZ = (z - (cz * cs).astype(F)).astype(F) <= rb
        hiZ = ((cz1 * cs).astype(F) - z).astype(F) <= rb
    face = {(-1, 0): hiY, (1, 0): loY, (0, -1): hiZ, (0, 1): loZ}
    f = np.zeros(pos.shape[0], np.uint8)
    for s, (sy, sz) in enumerate(SLOT_STEP):
        m = np.ones(pos.shape[0], bool)
        if sy:
            m &= face[(sy, 0)]
        if sz:
            m &= face[(0, sz)]
        f |= (m.astype(np.uint8) << s).astype(np.uint8)
    f[~ok] = 0xff
    return f


def band_arrays(pos, flags):
    """The eight band arrays: float32[count_s, 4] records (x, y, z, sorted index as bits), in sorted order."""
    pos = np.asarray(pos, F)
    out = []
    for s in range(8):
        idx = np.nonzero((flags >> s) & 1)[0]
        rec = np.zeros((idx.size, 4), F)
        rec[:, :3] = pos[idx, :3]
        rec[:, 3] = idx.astype(np.int32).view(F)
        out.append(rec)
    return out


def band_start(flags, cell_start):
    """uint32[8, G + 1]: band-s entries in front of cellStart[c]."""
    cell_start = np.asarray(cell_start, np.int64)
    out = np.zeros((8, cell_start.size), np.uint32)
    for s in range(8):
        before = np.concatenate([[0], np.cumsum((flags >> s) & 1, dtype=np.int64)])
        out[s] = before[np.minimum(cell_start, flags.size)]
    return out


def grid_allows_bands(cfg):
    """sph_bands_apply without the mode and slab tests: no aliased ids, three cells per axis, the 27 offsets distinct modulo G."""
    gx, gy, gz, G = cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellsZ, cfg.gridCellCount
    if G > int(cfg.cellIdMask) + 1 or min(gx, gy, gz) < 3 or gx * gy * gz != G:
        return False
    off = [(k % 3 - 1) + (k // 3 % 3 - 1) * gx + (k // 9 - 1) * gx * gy for k in range(27)]
    return all((a - b) % G != 0 for i, a in enumerate(off) for b in off[i + 1:])


def missing_from_bands(pos, keys, cell_start, cfg, flags=None):
    """The statement the kernel relies on, on one sorted state. For every particle P that satisfies the premise and every one of
    the 26 neighbour cells with a y or z step that is not wrapped (0 <= key + offset < G): the particles Q of that cell whose
    distance passes d^2 <= binU[63] — evaluated like the reference, float32 operation by operation — and that do NOT carry the
    flag of the row's band. Returns the list of (P, Q, slot); empty is what the kernel needs. All three x steps are checked, so
    the half-cell choice of the reference does not enter. Also returns the number of (P, Q) pairs tested inside the radius."""
    pos = np.asarray(pos, F)
    keys = np.asarray(keys, np.int64)
    cell_start = np.asarray(cell_start, np.int64)
    flags = band_flags(pos, keys, cfg) if flags is None else flags
    ok, _ = premise(pos, keys, cfg)
    r2 = filter_r2(cfg.h)
    gx, gy, G = cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellCount
    bad, tested = [], 0
    order = np.arange(keys.size)
    for s, (sy, sz) in enumerate(SLOT_STEP):
        for sx in (-1, 0, 1):
            cell = keys + sx + sy * gx + sz * gx * gy
            use = ok & (cell >= 0) & (cell < G)
            lo = cell_start[np.clip(cell, 0, G)]
            hi = cell_start[np.clip(cell + 1, 0, G)]
            n = np.where(use, hi - lo, 0)
            if n.sum() == 0:
                continue
            P = np.repeat(order, n)
            Q = np.repeat(lo - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(n.sum())
            e = (pos[P, :3] - pos[Q, :3]).astype(F)
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = ((e[:, 0] * e[:, 0]).astype(F) + (e[:, 1] * e[:, 1]).astype(F)).astype(F)
                d2 = (d2 + (e[:, 2] * e[:, 2]).astype(F)).astype(F)
                near = d2 <= r2
            tested += int(near.sum())
            miss = near & (((flags[Q] >> s) & 1) == 0)
            bad += [(int(p), int(q), s) for p, q in zip(P[miss], Q[miss])]
    return bad, tested


def band_totals(flags, keys, cell_start, cfg, tile=128):
    """Per workgroup of `tile` sorted particles: the candidates it stages when it serves its tile whole, with bands (own row from
    the cell table, the eight others from the band start tables) and without — the restatement of test_fn_staging.staged_totals."""
    keys = np.asarray(keys, np.int64)
    start = np.asarray(cell_start, np.int64)
    bstart = band_start(flags, start).astype(np.int64)
    G, gx, gy = start.size - 1, cfg.gridCellsX, cfg.gridCellsY
    first = np.arange(0, keys.size, tile)
    cLo, cHi = keys[first], keys[np.minimum(first + tile, keys.size) - 1]
    full = np.zeros(first.size, np.int64)
    banded = np.zeros(first.size, np.int64)
    for r in range(9):
        shift = (r % 3 - 1) * gx + (r // 3 - 1) * gx * gy
        a, b = np.clip(cLo - 1 + shift, 0, G), np.clip(cHi + 2 + shift, 0, G)
        full += np.maximum(start[b] - start[a], 0)
        tbl = start if r == 4 else bstart[r - (1 if r > 4 else 0)]
        banded += np.maximum(tbl[b] - tbl[a], 0)
    return banded, full
