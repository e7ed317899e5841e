"""What the lockstep walk of k_find_neighbors pays for a lane assignment (csrc/sph_neighbors.hip): a numpy
model of a liquid lattice, no GPU and no library needed.

The two lanes of a particle walk their four pieces in lockstep: the loop over the pieces is unrolled and the loop inside it is
wave-level, so piece i costs every lane of the wave the longest piece i of the wave. The model builds a cubic lattice (spacing and
jitter in units of r0 = h / 2), sorts it by cell (cells 2h wide, x fastest, ties in lattice order), builds the eight search bands
with the rule of band_flags (sph_band_flags.h) for a band radius Rb, lays the nine runs of every workgroup's tile of sorted particles
(--tile: 256 with bands, 128 without, as FN_PART) out as the kernel does (own row first, then rows 3 5 1 7 0 2 6 8; where the runs
exceed the LDS capacity the kernel's ladder of smaller batches: the aligned halves of a 256-particle tile, batches cut at x-row
boundaries, at most 32 particles, dropped runs) and counts, per wave of 32 particles:

  trips         sum over the four pieces of the longest walk of the wave, in trips of 8 candidates from the aligned start
  flush groups  the same with ceil(trips / 4): one flush per 32 candidates and one at the end of a piece
  floor         candidates of the particle's eight pieces / 2 lanes / 8, the mean over the particles: two perfectly balanced lanes

over the waves whose particles all lie two cells or more inside the lattice (every cell they visit is full). It also reports what
the staging costs: candidates staged per workgroup, staged records per particle, and the share of tiles that end on each rung of
the ladder — over the tiles whose particles all lie one cell or more inside the lattice (their rows exist; a compressed lattice
has few tiles two cells inside).

  python tools/fn_walk_model.py [--spacing 0.93] [--jitter 0] [--rb 3.4514] [--no-bands] [--lattice 48 | 160 24 24] [--tile 256]
                                [--assign 0457/1236 ...]
"""
import argparse

import numpy as np

H = 3.34            # smoothing radius, simulation units (the reference's h); r0 = h / 2, cells are 2h wide
R0, CELL = 0.5 * H, 2.0 * H
HALF, WAVE, CAND_CAP = 128, 32, 4096   # FN_HALF, FN_PER_WAVE, FN_CAND_CAP
RUNGS = ("whole tile", "aligned halves", "x-row batches", "at most 32 particles", "runs dropped")
ORDER = (4, 3, 5, 1, 7, 0, 2, 6, 8)    # layout of the staged rows; row = (y step + 1) + 3 (z step + 1)
STEPS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # cells 0..7: (x, y, z) steps


def lattice_state(n, spacing, jitter, seed=20261004):
    """Sorted positions [N, 3], keys, cell table and grid of an nx x ny x nz lattice (n: one number or three) that starts 3 r0 from
    the origin."""
    nx, ny, nz = (n, n, n) if np.isscalar(n) else n
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64),
                          indexing="ij")  # x fastest: the lattice order
    pos = 3.0 * R0 + spacing * R0 * np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    if jitter > 0.0:
        pos += np.random.default_rng(seed).uniform(-jitter * R0, jitter * R0, pos.shape)
    c = np.floor(pos / CELL).astype(np.int64)
    g = c.max(0) + 2
    key = c[:, 0] + g[0] * (c[:, 1] + g[1] * c[:, 2])
    order = np.argsort(key, kind="stable")
    pos, key = pos[order], key[order]
    G = int(g[0] * g[1] * g[2])
    start = np.searchsorted(key, np.arange(G + 1))
    return pos, key, start, g, G


def band_tables(pos, key, start, g, rb):
    """tables[r]: what the kernel reads where it reads cellStart, for staged row r: the cell table itself for the own row, the start
    table of the row's band for the others (rb None: no bands, every row reads the cell table)."""
    if rb is None:
        return [start] * 9
    cy, cz = (key // g[0]) % g[1], key // (g[0] * g[1])
    loY, hiY = pos[:, 1] - cy * CELL <= rb, (cy + 1) * CELL - pos[:, 1] <= rb
    loZ, hiZ = pos[:, 2] - cz * CELL <= rb, (cz + 1) * CELL - pos[:, 2] <= rb
    member = [hiY & hiZ, hiZ, loY & hiZ, hiY, loY, hiY & loZ, loZ, loY & loZ]  # band s = r - (r > 4), as band_flags
    out = []
    for r in range(9):
        if r == 4:
            out.append(start)
        else:
            out.append(np.searchsorted(np.flatnonzero(member[r - (r > 4)]), start))
    return out


def ladder(key, p0, block_hi, tables, gx, gxy, G, part):
    """The batches in which a workgroup serves its tile [p0, block_hi), as the kernel's retry ladder cuts them: (lo, hi, rung,
    staged candidates). Rung 0: the whole tile; 1: the aligned halves of a 256-particle tile; 2: batches that end at x-row boundaries
    (at most 128 particles, possibly across the two halves); 3: at most 32 particles; 4: runs dropped. A rung, once taken, holds for
    the rest of the tile."""
    out, lo, halves, retry = [], p0, False, 0
    while lo < block_hi:
        hi = block_hi
        if part > HALF and halves and not retry:
            hi = min(p0 + ((lo - p0) // HALF + 1) * HALF, block_hi)
        if retry:
            rows = key[lo:min(lo + HALF, block_hi)] // gx
            other = np.flatnonzero(rows != rows[0])
            stop = int(other[0]) if other.size else HALF
            hi = min(lo + (min(stop, WAVE) if retry == 2 else stop), block_hi)
        total, run_n = _total(key, lo, hi, tables, gx, gxy, G)[0], None
        rung = retry + 1 if retry else (1 if halves else 0)
        if total > CAND_CAP:
            if part > HALF and not halves:
                halves = True
                continue
            if retry < 2:
                retry += 1
                continue
            total, rung = _total(key, lo, hi, tables, gx, gxy, G, drop=True)[0], 4
        out.append((lo, hi, rung, total))
        lo = hi
    return out


def piece_trips(pos, key, start, g, G, tables, part=HALF):
    """trips[N, 8], candidates[N, 8] of every particle's eight pieces; -1 trips where the particle's batch does not fit the LDS. Also
    the ladder's batches of every tile."""
    N = key.size
    gx, gxy = int(g[0]), int(g[0] * g[1])
    cc = np.stack([key % gx, (key // gx) % g[1], key // gxy], 1)
    d = np.where(pos - cc * CELL < H, -1, 1)  # towards the nearer half of the cell
    trips = np.full((N, 8), -1, np.int64)
    cand = np.zeros((N, 8), np.int64)
    tiles = []
    for p0 in range(0, N, part):
        tiles.append(ladder(key, p0, min(p0 + part, N), tables, gx, gxy, G, part))
        for lo, hi, rung, _ in tiles[-1]:
            if rung >= 3:
                continue  # (batches of 32 particles and dropped runs: such batches are left out of the walk model)
            total, run_lo, base = _total(key, lo, hi, tables, gx, gxy, G)
            idx = np.arange(lo, hi)
            for k, (X, Y, Z) in enumerate(STEPS):
                raw = key[idx] + X * d[idx, 0] + Y * d[idx, 1] * gx + Z * d[idx, 2] * gxy
                row = (Y * d[idx, 1] + 1) + 3 * (Z * d[idx, 2] + 1)
                raw = np.clip(raw, 0, G - 1)
                a = np.empty(idx.size, np.int64)
                b = np.empty(idx.size, np.int64)
                for r in np.unique(row):
                    m = row == r
                    a[m] = base[r] + tables[r][raw[m]] - run_lo[r]
                    b[m] = base[r] + tables[r][raw[m] + 1] - run_lo[r]
                cand[idx, k] = b - a
                trips[idx, k] = np.where(b > a, (b - (a & ~3) + 7) // 8, 0)
    return trips, cand, tiles


def _total(key, lo, hi, tables, gx, gxy, G, drop=False):
    """Candidates of the nine runs of the batch [lo, hi), each run's first table entry and first LDS slot (drop: runs that no longer
    fit the capacity are left out, in layout order, as on the kernel's last rung)."""
    c_lo, c_hi = int(key[lo]), int(key[hi - 1])
    run_lo, base, total = {}, {}, 0
    for r in ORDER:
        shift = (r % 3 - 1) * gx + (r // 3 - 1) * gxy
        a = int(tables[r][min(max(c_lo - 1 + shift, 0), G)])
        b = int(tables[r][min(max(c_hi + 2 + shift, 0), G)])
        n = max(b - a, 0)
        if drop and total + n > CAND_CAP:
            n = 0
        run_lo[r], base[r] = a, total
        total += n
    return total, run_lo, base


def staging_report(tiles, interior):
    """(workgroups, mean and max candidates staged per workgroup, staged records per particle, share of tiles by their last rung)
    over the tiles whose particles are all `interior`."""
    staged, parts, rungs = [], 0, np.zeros(len(RUNGS))
    for batches in tiles:
        if not interior[batches[0][0]:batches[-1][1]].all():
            continue
        staged.append(sum(b[3] for b in batches))
        parts += batches[-1][1] - batches[0][0]
        rungs[max(b[2] for b in batches)] += 1
    return len(staged), float(np.mean(staged)), int(np.max(staged)), float(np.sum(staged)) / parts, rungs / len(staged)


def wave_cost(trips, interior, lane_a, lane_b):
    """(trips, flush groups) per wave for the assignment, mean over the waves whose particles are all interior and modelled."""
    N = trips.shape[0]
    t, f = [], []
    for w0 in range(0, N - WAVE + 1, WAVE):
        sl = slice(w0, w0 + WAVE)
        if not interior[sl].all() or (trips[sl] < 0).any():
            continue
        worst = [max(trips[sl, a].max(), trips[sl, b].max()) for a, b in zip(lane_a, lane_b)]
        t.append(sum(worst))
        f.append(sum((x + 3) // 4 for x in worst))
    if not t:  # (a compressed lattice of few cells has no wave two cells inside)
        return float("nan"), float("nan"), 0
    return float(np.mean(t)), float(np.mean(f)), len(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spacing", type=float, default=0.93, help="lattice spacing in r0 (the headline box: 0.93)")
    ap.add_argument("--jitter", type=float, default=0.0, help="uniform jitter per axis in r0")
    ap.add_argument("--rb", type=float, default=3.4514, help="band radius in simulation units (h = 3.34)")
    ap.add_argument("--no-bands", action="store_true", help="every row is staged from whole cells (k_find_neighbors<false>)")
    ap.add_argument("--lattice", type=int, nargs="+", default=[48], help="particles per axis: one number, or x y z")
    ap.add_argument("--tile", type=int, default=0, choices=(0, HALF, 2 * HALF),
                    help="particles per workgroup (default: 256 with bands, 128 without, as the kernel's two instances)")
    ap.add_argument("--assign", nargs="*", default=["0567/1234", "0457/1236", "0236/1457"],
                    help="lane assignments, cells of lane A / cells of lane B, piece by piece")
    a = ap.parse_args()
    assert len(a.lattice) in (1, 3), "--lattice takes one number or three"
    part = a.tile or (HALF if a.no_bands else 2 * HALF)
    pos, key, start, g, G = lattice_state(a.lattice[0] if len(a.lattice) == 1 else tuple(a.lattice), a.spacing, a.jitter)
    tables = band_tables(pos, key, start, g, None if a.no_bands else a.rb)
    trips, cand, tiles = piece_trips(pos, key, start, g, G, tables, part)
    lo, hi = pos.min(0) + 2.0 * CELL, pos.max(0) - 2.0 * CELL
    interior = ((pos >= lo) & (pos <= hi)).all(1)
    mean = cand[interior].mean(0)
    print("lattice %s, spacing %.3f r0, jitter %.3f r0, %s: %d particles, %d interior, %.1f candidates in a particle's own cell"
          % (" x ".join("%d" % n for n in a.lattice) + ("^3" if len(a.lattice) == 1 else ""), a.spacing, a.jitter,
             "no bands" if a.no_bands else "Rb %.4f" % a.rb, key.size, int(interior.sum()), mean[0]))
    lo, hi = pos.min(0) + CELL, pos.max(0) - CELL
    n, st_mean, st_max, per_particle, rungs = staging_report(tiles, ((pos >= lo) & (pos <= hi)).all(1))
    print("tile %d: %d interior workgroups stage %.0f candidates on average, %d at most (capacity %d): %.2f staged records per particle"
          % (part, n, st_mean, st_max, CAND_CAP, per_particle))
    print("tiles by the last rung of the ladder they need: %s" % ", ".join("%s %.1f %%" % (w, 100.0 * x) for w, x in zip(RUNGS, rungs)))
    print("candidates per piece relative to the own cell's, cells 0..7: %s" % " ".join("%.2f" % x for x in mean / mean[0]))
    floor = cand[interior].sum(1).mean() / 2.0 / 8.0
    for s in a.assign:
        lane_a, lane_b = ([int(ch) for ch in part] for part in s.split("/"))
        assert sorted(lane_a + lane_b) == list(range(8)) and len(lane_a) == 4, s
        t, f, waves = wave_cost(trips, interior, lane_a, lane_b)
        if not waves:
            print("assignment %s | %s: no wave lies two cells inside this lattice" % (lane_a, lane_b))
            continue
        print("assignment %s | %s: %.1f trips, %.1f flush groups per wave (%d waves)" % (lane_a, lane_b, t, f, waves))
    print("floor (candidates / 2 / 8): %.1f trips" % floor)


if __name__ == "__main__":
    main()
