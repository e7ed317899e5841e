"""The neighbourhood bytes of the predict-correct loop restated in numpy from a canonical state.

A wave is 64 consecutive sorted particles. A wave whose flag is set marks every wave that could hold a particle with a neighbour in
it, judged by cells as findNeighbors looks them up: a particle with key ki searches the cells wrap(ki + delta) for the 27 offsets
delta = dx + dy gx + dz gx gy, so a particle with key kj is a possible neighbour of the particles in the cells wrap(kj - delta); the
sorted range [lo, hi) of such a cell marks the waves lo >> 6 .. (hi - 1) >> 6. Keys are the masked cell ids of the sorted order."""
import numpy as np

BOUNDARY = 3


def search_tables(canon):
    """(sorted keys, cell table with G + 1 entries) of the search of the step that left `canon`."""
    return canon["particleIndex"].reshape(-1, 2)[:, 0].astype(np.int64), canon["gridCellIndexFixedUp"].astype(np.int64)


def sorted_liquid(canon):
    """Per sorted particle: it is not a boundary particle."""
    pi = canon["particleIndex"].reshape(-1, 2)[:, 1].astype(np.int64)
    return canon["position"][:, 3].astype(np.int32)[pi] != BOUNDARY


def wave_any(per_particle):
    n = per_particle.size
    return np.bincount(np.arange(n) >> 6, weights=per_particle, minlength=(n + 63) // 64) > 0


def neighbourhood(keys, cell_start, flagged, gx, gy, G, active=None):
    """(marked waves, a flagged wave holds a key outside [0, G), cells that were wrapped back into [0, G)).
    flagged: bool per wave. active: bool per sorted particle, the particles whose keys a flagged wave takes (None: all)."""
    n = keys.size
    W = (n + 63) // 64
    take = np.asarray(flagged, bool)[np.arange(n) >> 6]
    if active is not None:
        take = take & active
    kj = np.unique(keys[take])
    closed = bool((kj >= G).any() or (kj < 0).any())
    kj = kj[(kj >= 0) & (kj < G)]
    diff = np.zeros(W + 1, np.int64)
    wrapped = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                raw = kj - (dx + dy * gx + dz * gx * gy)
                ki = np.where(raw < 0, raw + G, raw)
                ki = np.where(ki >= G, ki - G, ki)
                ok = (ki >= 0) & (ki < G)
                wrapped += int((ok & (ki != raw)).sum())
                ki = ki[ok]
                lo, hi = cell_start[ki], np.minimum(cell_start[ki + 1], n)
                full = hi > lo
                np.add.at(diff, lo[full] >> 6, 1)
                np.add.at(diff, ((hi[full] - 1) >> 6) + 1, -1)
    return np.cumsum(diff)[:W] > 0, closed, wrapped


def readers_by_rows(ids, flagged):
    """Per wave: one of its particles has a valid neighbour in a flagged wave (ids: int[N, 32] sorted indices, -1 empty), or lies
    in a flagged wave itself."""
    n = ids.shape[0]
    flagged = np.asarray(flagged, bool)
    near = ((ids >= 0) & flagged[np.clip(ids, 0, n - 1) >> 6]).any(1)
    return wave_any(near | flagged[np.arange(n) >> 6])
