"""What the lockstep walk of k_find_neighbors pays for a lane assignment (csrc/sph_neighbors.hip): a numpy
model of a liquid lattice, no GPU and no library needed.

The two lanes of a particle walk their four pieces in lockstep: the loop over the pieces is unrolled and the loop inside it is
wave-level, so piece i costs every lane of the wave the longest piece i of the wave. The model builds a cubic lattice (spacing and
jitter in units of r0 = h / 2), sorts it by cell (cells 2h wide, x fastest, ties in lattice order), builds the eight search bands
with the rule of band_flags (sph_band_flags.h) for a band radius Rb, lays the nine runs of every workgroup of 128 sorted particles
out as the kernel does (own row first, then rows 3 5 1 7 0 2 6 8; batches cut at x-row boundaries where the runs exceed the LDS
capacity) and counts, per wave of 32 particles:

  trips         sum over the four pieces of the longest walk of the wave, in trips of 8 candidates from the aligned start
  flush groups  the same with ceil(trips / 4): one flush per 32 candidates and one at the end of a piece
  floor         candidates of the particle's eight pieces / 2 lanes / 8, the mean over the particles: two perfectly balanced lanes

over the waves whose particles all lie two cells or more inside the lattice (every cell they visit is full).

  python tools/fn_walk_model.py [--spacing 0.93] [--jitter 0] [--rb 3.4514] [--no-bands] [--lattice 48] [--assign 0457/1236 ...]
"""
import argparse

import numpy as np

H = 3.34            # smoothing radius, simulation units (the reference's h); r0 = h / 2, cells are 2h wide
R0, CELL = 0.5 * H, 2.0 * H
PART, WAVE, CAND_CAP = 128, 32, 4096   # FN_PART, FN_PER_WAVE, FN_CAND_CAP
ORDER = (4, 3, 5, 1, 7, 0, 2, 6, 8)    # layout of the staged rows; row = (y step + 1) + 3 (z step + 1)
STEPS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # cells 0..7: (x, y, z) steps


def lattice_state(n, spacing, jitter, seed=20261004):
    """Sorted positions [N, 3], keys, cell table and grid of an n^3 lattice that starts 3 r0 from the origin."""
    i = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")  # x fastest: the lattice order
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


def piece_trips(pos, key, start, g, G, tables):
    """trips[N, 8], candidates[N, 8] of every particle's eight pieces; -1 trips where the particle's batch does not fit the LDS."""
    N = key.size
    gx, gxy = int(g[0]), int(g[0] * g[1])
    cc = np.stack([key % gx, (key // gx) % g[1], key // gxy], 1)
    d = np.where(pos - cc * CELL < H, -1, 1)  # towards the nearer half of the cell
    trips = np.full((N, 8), -1, np.int64)
    cand = np.zeros((N, 8), np.int64)
    for p0 in range(0, N, PART):
        hi_all = min(p0 + PART, N)
        cuts = [p0, hi_all]
        if _total(key, p0, hi_all, tables, gx, gxy, G)[0] > CAND_CAP:  # the kernel's retry 1: batches end at x-row boundaries
            rows = key[p0:hi_all] // gx
            cuts = [p0] + list(p0 + 1 + np.flatnonzero(rows[1:] != rows[:-1])) + [hi_all]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            total, run_lo, base = _total(key, lo, hi, tables, gx, gxy, G)
            if total > CAND_CAP:
                continue  # (the kernel goes on to batches of 32 particles; such workgroups are left out of the model)
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
    return trips, cand


def _total(key, lo, hi, tables, gx, gxy, G):
    c_lo, c_hi = int(key[lo]), int(key[hi - 1])
    run_lo, base, total = {}, {}, 0
    for r in ORDER:
        shift = (r % 3 - 1) * gx + (r // 3 - 1) * gxy
        a = int(tables[r][min(max(c_lo - 1 + shift, 0), G)])
        b = int(tables[r][min(max(c_hi + 2 + shift, 0), G)])
        run_lo[r], base[r] = a, total
        total += max(b - a, 0)
    return total, run_lo, base


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
    return float(np.mean(t)), float(np.mean(f)), len(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spacing", type=float, default=0.93, help="lattice spacing in r0 (the headline box: 0.93)")
    ap.add_argument("--jitter", type=float, default=0.0, help="uniform jitter per axis in r0")
    ap.add_argument("--rb", type=float, default=3.4514, help="band radius in simulation units (h = 3.34)")
    ap.add_argument("--no-bands", action="store_true", help="every row is staged from whole cells (k_find_neighbors<false>)")
    ap.add_argument("--lattice", type=int, default=48, help="particles per axis")
    ap.add_argument("--assign", nargs="*", default=["0567/1234", "0457/1236", "0236/1457"],
                    help="lane assignments, cells of lane A / cells of lane B, piece by piece")
    a = ap.parse_args()
    pos, key, start, g, G = lattice_state(a.lattice, a.spacing, a.jitter)
    tables = band_tables(pos, key, start, g, None if a.no_bands else a.rb)
    trips, cand = piece_trips(pos, key, start, g, G, tables)
    lo, hi = pos.min(0) + 2.0 * CELL, pos.max(0) - 2.0 * CELL
    interior = ((pos >= lo) & (pos <= hi)).all(1)
    mean = cand[interior].mean(0)
    print("lattice %d^3, spacing %.3f r0, jitter %.3f r0, %s: %d particles, %d interior, %.1f candidates in a particle's own cell"
          % (a.lattice, a.spacing, a.jitter, "no bands" if a.no_bands else "Rb %.4f" % a.rb, key.size, int(interior.sum()), mean[0]))
    print("candidates per piece relative to the own cell's, cells 0..7: %s" % " ".join("%.2f" % x for x in mean / mean[0]))
    floor = cand[interior].sum(1).mean() / 2.0 / 8.0
    for s in a.assign:
        lane_a, lane_b = ([int(ch) for ch in part] for part in s.split("/"))
        assert sorted(lane_a + lane_b) == list(range(8)) and len(lane_a) == 4, s
        t, f, waves = wave_cost(trips, interior, lane_a, lane_b)
        print("assignment %s | %s: %.1f trips, %.1f flush groups per wave (%d waves)" % (lane_a, lane_b, t, f, waves))
    print("floor (candidates / 2 / 8): %.1f trips" % floor)


if __name__ == "__main__":
    main()
