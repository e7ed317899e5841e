"""Plain numpy restatement of what a slab solver must hold after a step — its cell table, the cells the reference walk of a
particle visits, the particles each stage computes, neighbour rows keyed by global id — and the corner scene the slab
structure tests run on (tests/test_slab_structures_host.py, tests/test_slab_structures.py).

Imports nothing from the code under test but the config and the helpers of sphmi/slab.py."""
import numpy as np

import scenes
from sphmi import slab as S

SEARCH_DEPTH, DENSITY_DEPTH, FORCES_DEPTH = 3, 1, 0  # ghost depth in layers of the stages at maxIteration = 3 (stage_depth)


def stage_depth(hops, ghost_layers=S.GHOST_LAYERS):
    """Layers beyond the owned range that a stage `hops` neighbour hops (<= 31/60 of a layer each) before the end of the step runs
    on: 5 hops for the neighbour search at maxIteration = 3, 1 for the density, 0 for the forces."""
    return min((hops * 31 + 59) // 60, ghost_layers)


def cell_coords(position, cfg):
    inv = np.float32(cfg.hashGridCellSizeInv)
    return [(np.ascontiguousarray(position[:, k], np.float32) * inv).astype(np.int32) for k in range(3)]


def cell_ids(position, cfg):
    """hashParticles: cx + cy * gx + cz * gx * gy from (int)(coordinate * hashGridCellSizeInv) in f32, masked (int64[n])."""
    cx, cy, cz = (c.astype(np.int64) for c in cell_coords(position, cfg))
    cell = cx + cy * cfg.gridCellsX + cz * cfg.gridCellsX * cfg.gridCellsY
    return (cell & 0xffffffff & int(cfg.cellIdMask)).astype(np.int64)


def true_cell_table(position, cfg):
    """gridCellIndexFixedUp of a particle set: table[c] = particles whose cell id is below c (int64[G + 1]); [0] = 0, [G] = n."""
    G = cfg.gridCellCount
    keys = np.sort(cell_ids(position, cfg), kind="stable")
    table = np.searchsorted(keys, np.arange(G + 1), side="left").astype(np.int64)
    table[0], table[G] = 0, position.shape[0]
    return table


def reference_cells(position, cfg, wrap=True):
    """(raw, wrapped): int64[n, 8] cells of the reference's neighbour walk in its order — own cell, x, y, z, xy, xz, yz, xyz, each
    step towards the half of the cell the particle lies in — as raw indices and after searchCell's two sequential corrections
    (c < 0 -> c + G, then c >= G -> c - G). wrap=False leaves the second array unwrapped (the mutation the host tests catch)."""
    f = np.float32
    gx, gy, G = cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellCount
    size, h = f(cfg.hashGridCellSize), f(cfg.h)
    step = []
    for k, (c, lo) in enumerate(zip(cell_coords(position, cfg), (cfg.xmin, cfg.ymin, cfg.zmin))):
        p = np.ascontiguousarray(position[:, k], np.float32)
        corner = c.astype(np.float32) * size
        step.append(np.where((p - f(lo)) - corner < h, -1, 1).astype(np.int64))
    dx, dy, dz = step[0], step[1] * gx, step[2] * gx * gy
    zero = np.zeros_like(dx)
    own = cell_ids(position, cfg)
    raw = own[:, None] + np.stack([zero, dx, dy, dz, dx + dy, dx + dz, dy + dz, dx + dy + dz], axis=1)
    wrapped = raw.copy()
    if wrap:
        wrapped = np.where(wrapped < 0, wrapped + G, wrapped)
        wrapped = np.where(wrapped >= G, wrapped - G, wrapped)
    return raw, wrapped


def in_layers(position, cfg, slab, depth):
    """bool[n]: the particles a stage of ghost depth `depth` computes — those of layers [layerLo - depth, layerHi + depth),
    clipped to the grid."""
    lay = S.particle_layers(position, cfg)
    lo, hi = max(int(slab.layerLo) - depth, 0), min(int(slab.layerHi) + depth, cfg.gridCellsZ)
    return (lay >= lo) & (lay < hi)


def rows_by_global_id(neighbor_map, particle_index, global_ids):
    """A solver's neighborMap (rows and entries in sorted-index space, (id as float, distance) pairs) as rows keyed by global id:
    (gid int64[n] ascending, ids int64[n, 32] as global ids with -1 for empty slots, distance bits uint32[n, 32]).
    particle_index is the solver's particleIndex ((cell, local id) per sorted index), global_ids the global id of each local id.
    Works for the oracle and for the HIP solver alike."""
    nm = np.ascontiguousarray(neighbor_map, np.float32).reshape(-1, 32, 2)
    n = nm.shape[0]
    local = np.asarray(particle_index).reshape(-1, 2)[:n, 1].astype(np.int64)
    gid_of_sorted = np.asarray(global_ids).astype(np.int64)[local]
    ids = nm[:, :, 0].astype(np.int64)
    ids_g = np.where(ids >= 0, gid_of_sorted[np.clip(ids, 0, n - 1)], -1)
    bits = np.ascontiguousarray(nm[:, :, 1]).view(np.uint32)
    order = np.argsort(gid_of_sorted, kind="stable")
    return gid_of_sorted[order], ids_g[order], bits[order]


def by_global_id(values, particle_index, global_ids):
    """A per-sorted-particle array (rho, ...) reordered to ascending global id."""
    n = np.asarray(particle_index).size // 2
    local = np.asarray(particle_index).reshape(-1, 2)[:, 1].astype(np.int64)
    order = np.argsort(np.asarray(global_ids).astype(np.int64)[local], kind="stable")
    return np.asarray(values)[:n][order]


def first_row_difference(got, want, select, position, cfg):
    """None, or a description of the first selected global id whose row differs: the id, its cell, both rows."""
    gid, ids_a, bits_a = got
    gid_b, ids_b, bits_b = want
    assert np.array_equal(gid, gid_b)
    bad = select & ((ids_a != ids_b).any(1) | (bits_a != bits_b).any(1))
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    cell = int(cell_ids(position[i:i + 1], cfg)[0])
    return ("%d of %d rows differ; first: global id %d, type %d, cell %d, reference cells %s\n got  %s\n want %s\n distances: %s"
            % (int(bad.sum()), int(select.sum()), int(gid[i]), int(position[i, 3]), cell,
               reference_cells(position[i:i + 1], cfg)[0][0].tolist(), ids_a[i].tolist(), ids_b[i].tolist(),
               scenes.diff_report(bits_a[i].view(np.float32), bits_b[i].view(np.float32))))


CORNER_CUTS3 = [0, 8, 16, 20]  # three slabs of the corner scene (balanced_cuts wants more layers for three)


def corner_scene(origin_in_r0=1.5, tall=False):
    """Liquid resting in the low corner of the box, half a cell from the walls: 14,192 particles (9,000 liquid) on a 9 x 9 x 41
    grid, layers 0..19 occupied. Liquid in cells 0, gx, gx*gy and gx*gy + gx has reference cells with raw index -1, which
    searchCell wraps to G - 1; balanced_cuts(layers, 2) is [0, 8, 20], so rank 0 of 2 computes its cell table up to layer 14 only.
    The liquid ends in layer 9, so all of it is local to rank 0 (layers below 12) from the start. tall=True: a narrower column
    (13 x 13 x 56, 14,656 particles, same cuts, same corner) that reaches layer 13: when it drifts down, rank 0 receives liquid it
    did not hold before and its local count grows."""
    o = float(origin_in_r0)
    return scenes.liquid_box((8.0, 8.0, 40.0), (13, 13, 56) if tall else (15, 15, 40), mask=0xffffffff, jitter_in_r0=0.05,
                             origin_in_r0=(o, o, o))


def rank_setup(sc, cuts, rank):
    """(slab, local global ids) of one rank of the scene under the given cuts."""
    world = len(cuts) - 1
    layers = S.particle_layers(sc["position"], sc["cfg"])
    slab = S.make_slab(cuts, rank, world, sc["cfg"].particleCount)
    return slab, S.local_indices(layers, slab)


def oracle_step_on(sc, idx, threads=4):
    """One oracle step on the local set `idx` (ascending global ids) of the scene: the solver, still open, for its buffers."""
    import sphmi
    from oracle import oraclebind as O
    d = sphmi.config_dict(sc["cfg"])
    d["N"] = d["particleCount"] = int(idx.size)
    o = O.OracleSolver(d, sc["position"][idx], sc["velocity"][idx], threads=threads)
    o.step()
    return o
