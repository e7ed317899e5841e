"""The 256-particle tiles of findNeighbors' band instance (csrc/sph_neighbors.hip), judged without a GPU. With search
bands a workgroup stages the nine runs of 256 consecutive sorted particles once, and each lane pair serves two particles in turn,
tile offsets t and t + 128, from that copy. Where the runs exceed the candidate capacity the workgroup goes down a ladder of
smaller batches: the aligned halves, batches that end at x-row boundaries (at most 128 particles, possibly across the halves), at
most 32 particles, dropped runs.

This module restates the run layout and the ladder from the oracle's sorted keys and cell table (as test_fn_staging.py restates the
totals, with the band tables of band_ref.py) and proves that the scenes of test_fn_tile.py contain what they are for. The
conditions are on the scenes, not tolerances."""
import numpy as np

import band_cases
import band_ref
import scenes
import test_fn_lane_order_host as lane_host
import test_fn_staging as staging
from test_gpu_parity import canon_ora

HALF, TILE, WAVE = 128, 256, 32   # FN_HALF, FN_PART(true), FN_PER_WAVE
CAP = 4096                        # FN_CAND_CAP: staged candidates per workgroup, both instances
WIN = 16                          # FN_WIN: table entries per row of the window; a batch of nc = cHi - cLo + 3 cells needs nc + 1
ORDER = (4, 3, 5, 1, 7, 0, 2, 6, 8)
RUNG = {"whole": 0, "halves": 1, "rows": 2, "small": 3, "dropped": 4}
STEPS = staging.STEPS

# the smallest counted boxes (band_cases.counted_box takes 37 449 .. 134 784 particles) with N = 127, 128, 129, 255, 0, 1 (mod 256)
COUNTED = (37503, 37504, 37505, 37631, 37632, 37633)
ROOMY = (37505, 37505 + 300)      # one case with capacity > N


def squeezed_scene():
    """The `tiny` box with wide ids at 0.55 r0 (at 0.70 r0 no tile of this small box comes near the capacity): with bands most
    tiles of 256 fit the capacity whole and two only as halves; a third of the particles keep to the lane pair. No jitter: with
    0.05 r0 or more the reference's second or third step leaves non-finite positions at this compression, and its next step
    does not survive them."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (18, 16, 18), spacing_in_r0=0.55, mask=0xffffffff)


def packed_scene():
    """The same box at 0.47 r0: tiles on every rung — whole, halves, x-row batches that start inside the second half, batches of at
    most 32 particles, dropped runs. Most particles have more than 96 others within h and take the exact walk."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (20, 18, 20), spacing_in_r0=0.47, mask=0xffffffff)


def coincident_scene():
    """test_search_bands.test_coincident_particles' scene: five coincident pairs, some in first and some in second halves of tiles."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), jitter_in_r0=0.03)
    pos = sc["position"].copy()
    pos[5:10, :3] = pos[200:205, :3]
    sc["position"] = pos
    return sc


SCENE = dict(staging.SCENE, jitter=lane_host.jitter_scene, squeezed=squeezed_scene, packed=packed_scene, stray=band_cases.stray_scene,
             coincident=coincident_scene)
for _n in COUNTED:
    SCENE["counted%d" % _n] = (lambda n=_n: band_cases.counted_box(n))
SCENE["roomy"] = lambda: band_cases.counted_box(*ROOMY)
_oracle = {}


def oracle_states(name):
    """Canonical oracle buffers after each of STEPS steps (the coincident scene: through computeDensity of the first step, beyond
    which the reference divides by zero): computed once per scene, shared, never changed."""
    if name in staging.SCENE:
        return staging.oracle_states(name)
    if name == "jitter":
        return lane_host.oracle_states(name)
    if name not in _oracle:
        sc = SCENE[name]()
        if name == "coincident":
            _oracle[name] = [band_cases.oracle_search(sc)]
        else:
            N = sc["cfg"].particleCount
            ora = scenes.oracle_for(sc, threads=8)
            out = []
            for _ in range(STEPS):
                ora.step()
                out.append(canon_ora(ora, N))
            ora.close()
            _oracle[name] = out
    return _oracle[name]


def tables(canon, cfg, bands=True):
    """(keys, the nine tables the kernel reads the run ends from — cell table for the own row, band start tables for the others —,
    cell table)."""
    pos, keys, start = band_cases.sorted_state(canon)
    start = np.asarray(start, np.int64)
    if not bands:
        return keys, [start] * 9, start
    bstart = band_ref.band_start(band_ref.band_flags(pos, keys, cfg), start).astype(np.int64)
    return keys, [start if r == 4 else bstart[r - (r > 4)] for r in range(9)], start


def runs(keys, lo, hi, tabs, start, cfg):
    """Candidates of the nine runs of the batch [lo, hi), in layout order."""
    G, gx, gy = start.size - 1, cfg.gridCellsX, cfg.gridCellsY
    cLo, cHi = int(keys[lo]), int(keys[hi - 1])
    n = []
    for r in ORDER:
        shift = (r % 3 - 1) * gx + (r // 3 - 1) * gx * gy
        a, b = min(max(cLo - 1 + shift, 0), G), min(max(cHi + 2 + shift, 0), G)
        n.append(max(int(tabs[r][b] - tabs[r][a]), 0))
    return n


def ladder(keys, p0, block_hi, tabs, start, cfg, cap=CAP, tile=TILE):
    """The batches in which a workgroup serves its tile [p0, block_hi): (lo, hi, rung, runs dropped, cells per row nc)."""
    gx = cfg.gridCellsX
    out, lo, halves, retry = [], p0, False, 0
    while lo < block_hi:
        hi = block_hi
        if tile > HALF and halves and not retry:
            hi = min(p0 + ((lo - p0) // HALF + 1) * HALF, block_hi)
        if retry:
            rows = keys[lo:min(lo + HALF, block_hi)] // gx
            other = np.flatnonzero(rows != rows[0])
            stop = int(other[0]) if other.size else HALF
            hi = min(lo + (min(stop, WAVE) if retry == 2 else stop), block_hi)
        n = runs(keys, lo, hi, tabs, start, cfg)
        fits = sum(n) <= cap
        rung, dropped = (retry + 1 if retry else (1 if halves else 0)), 0
        if not fits:
            if tile > HALF and not halves:
                halves = True
                continue
            if retry < 2:
                retry += 1
                continue
            total = 0
            for q in range(9):
                if total + n[q] > cap:
                    n[q] = 0
                    dropped += 1
                total += n[q]
            rung = RUNG["dropped"]
        out.append((lo, hi, rung, dropped, int(keys[hi - 1]) - int(keys[lo]) + 3))
        lo = hi
    return out


def tile_ladders(canon, cfg):
    keys, tabs, start = tables(canon, cfg)
    return keys, [ladder(keys, p0, min(p0 + TILE, keys.size), tabs, start, cfg) for p0 in range(0, keys.size, TILE)]


def test_counted_boxes_end_at_every_kind_of_tile_end():
    assert sorted(n % TILE for n in COUNTED) == [0, 1, 127, 128, 129, 255]
    assert all(37449 <= n for n in COUNTED) and ROOMY[1] > ROOMY[0]
    assert band_ref.grid_allows_bands(band_cases.counted_box(COUNTED[0])["cfg"])


def test_lane_order_scene_has_its_rows_in_both_halves_of_a_tile():
    """Particles with neighbours in all eight cells at tile offsets below 128 and at 128 or above, in every one of the three states
    the GPU test compares; full rows whose slot 31 lies in each of the eight cells in both halves too — over the three states taken
    together (rows that end in the own cell are rare: three, two and two of them in the three states)."""
    cfg = SCENE["jitter"]()["cfg"]
    assert band_ref.grid_allows_bands(cfg)
    ends = np.zeros((8, 2), np.int64)  # full rows by the cell of slot 31 and the half of the tile
    for it, canon in enumerate(oracle_states("jitter")):
        cells = lane_host.row_cells(canon, cfg)
        second = (np.arange(cells.shape[0]) % TILE) >= HALF
        everywhere = np.stack([(cells == k).any(1) for k in range(8)], 1).all(1)
        print("step %d: particles with neighbours in all eight cells: %d in first halves, %d in second halves"
              % (it + 1, int((everywhere & ~second).sum()), int((everywhere & second).sum())))
        assert (everywhere & second).any() and (everywhere & ~second).any()
        full = cells[:, 31] >= 0
        for k in range(8):
            last = full & (cells[:, 31] == k)
            ends[k] += (int((last & ~second).sum()), int((last & second).sum()))
    print("full rows whose slot 31 lies in cell 0..7, first / second halves: %s" % ends.tolist())
    assert (ends >= 1).all()


def test_scenes_reach_every_rung_of_the_ladder():
    """Bands on, capacity 4096: tiles that fit whole, fit only as halves, need batches cut at x-row boundaries with a boundary inside
    the second half, need batches of at most 32 particles, and drop runs; a batch wider than the window; totals on both sides of
    the capacity from the oracle's state alone."""
    seen = {}
    for name in ("squeezed", "packed", "dense", "tight", "sparse"):
        cfg = SCENE[name]()["cfg"]
        assert band_ref.grid_allows_bands(cfg), name
        keys, tiles = tile_ladders(oracle_states(name)[0], cfg)
        _, tabs, start = tables(oracle_states(name)[0], cfg)
        whole = np.array([sum(runs(keys, p0, min(p0 + TILE, keys.size), tabs, start, cfg)) for p0 in range(0, keys.size, TILE)])
        last = np.array([max(b[2] for b in t) for t in tiles])
        seen[name] = (tiles, last, whole)
        print("%s: N %d, banded candidates per 256-tile %d .. %d, tiles by last rung %s, widest batch %d cells"
              % (name, keys.size, whole.min(), whole.max(), np.bincount(last, minlength=5).tolist(), max(b[4] for t in tiles for b in t)))
    tiles, last, whole = seen["squeezed"]
    assert (whole <= CAP).any() and (whole > CAP).any()                   # on both sides of the capacity
    assert (last == RUNG["whole"]).any() and (last == RUNG["halves"]).any()
    inside_second = False  # an x-row batch that starts strictly inside the second half of its tile
    for name in seen:
        for t in seen[name][0]:
            p0 = t[0][0]
            inside_second |= any(b[2] == RUNG["rows"] and HALF < b[0] - p0 < TILE for b in t)
    assert inside_second
    assert (seen["packed"][1] == RUNG["dropped"]).any()
    assert any(b[2] == RUNG["small"] for t in seen["packed"][0] for b in t)  # (batches of at most 32 particles that fit)
    assert (seen["dense"][1] == RUNG["halves"]).any() and (seen["dense"][1] == RUNG["rows"]).any()
    assert any(b[4] + 1 > WIN for t in seen["sparse"][0] for b in t)      # the direct-table path
    assert SCENE["sparse"]()["cfg"].particleCount % TILE not in (0, HALF)


def test_exact_walks_start_from_second_halves():
    """Particles the fast path cannot serve at tile offsets of 128 and above: the stray scene's moved particles (premise fails), the
    overcrowded scene's particles with more than 96 others within h, and the coincident pairs' scene has pairs in a second half."""
    sc = SCENE["stray"]()
    canon = oracle_states("stray")[0]
    pos, keys, _ = band_cases.sorted_state(canon)
    ok, _ = band_ref.premise(pos, keys, sc["cfg"])
    off = np.flatnonzero(~ok) % TILE
    print("stray: %d particles fail the premise, %d of them in second halves" % (off.size, int((off >= HALF).sum())))
    assert off.size >= sc["moved"].size and (off >= HALF).any() and (off < HALF).any()
    crowded = scenes.crowded_particles(oracle_states("dense")[0], SCENE["dense"]()["cfg"].h) % TILE
    assert (crowded >= HALF).any() and (crowded < HALF).any()
    d = oracle_states("coincident")[0]["neighborDist"].reshape(-1, 32)
    zero = np.flatnonzero((d == 0.0).any(1)) % TILE
    assert (zero >= HALF).any() and (zero < HALF).any()
