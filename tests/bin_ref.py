"""numpy restatement of the binned-diagnostics contract (include/sphmi.h, sph_bin_diagnostics / sph_bin_index).

Works from the contract alone: the float32 edges origin + (float32)i * spacing, a particle's bin by searchsorted on those edges
(the largest i with edge[i] <= x, so a particle on an edge belongs to the upper bin and a run of coinciding edges is a run of
empty bins), the type and key rule of diag_ref.selected, and as records the diag_ref records of the bins' boxes: the restatement
of the arithmetic stays the one in diag_ref.py. A lattice is what sphmi.bin_lattice returns."""
import numpy as np

import diag_ref

f32 = np.float32


def parts(lattice):
    g = np.asarray(lattice).reshape(1)
    return g["origin"][0].astype(np.float32), g["spacing"][0].astype(np.float32), tuple(int(v) for v in g["dims"][0])


def types_of(lattice):
    m = int(np.asarray(lattice).reshape(1)["typeMask"][0])
    return tuple(t for t in range(32) if m >> t & 1)


def edges(lattice):
    """Per axis the dims + 1 float32 edges; (-inf, +inf) for a whole axis (dims 1, spacing 0)."""
    o, sp, dims = parts(lattice)
    out = []
    for a in range(3):
        if dims[a] == 1 and sp[a] == 0:
            out.append(np.array([-np.inf, np.inf], np.float32))
            continue
        e = np.empty(dims[a] + 1, np.float32)
        for i in range(dims[a] + 1):
            e[i] = f32(o[a] + f32(f32(i) * sp[a]))  # one rounded multiply, one rounded add
        out.append(e)
    return out


def boxes(lattice):
    """float32[bins, 6], bin (i, j, k) at row (k * ny + j) * nx + i."""
    ex, ey, ez = edges(lattice)
    rows = []
    for k in range(ez.size - 1):
        for j in range(ey.size - 1):
            for i in range(ex.size - 1):
                rows.append((ex[i], ey[j], ez[k], ex[i + 1], ey[j + 1], ez[k + 1]))
    return np.array(rows, np.float32).reshape(-1, 6)


def axis_index(e, x):
    """int64[N]: the i with e[i] <= x < e[i + 1], -1 where there is none (below e[0], at or above e[-1], NaN)."""
    x = np.asarray(x, np.float32)
    i = np.searchsorted(e, x, side="right").astype(np.int64) - 1  # the largest i with e[i] <= x
    i[(i >= e.size - 1) | np.isnan(x)] = -1
    if e.size == 2 and np.isinf(e[0]) and np.isinf(e[1]):  # the whole axis: -inf <= x < +inf
        i = np.where((x >= -np.inf) & (x < np.inf), 0, -1).astype(np.int64)
    return i


def index(state, lattice):
    """int32[N]: the flat bin of every sorted particle, -1 for one that is unselected by type or key or lies in no bin."""
    ex, ey, ez = edges(lattice)
    pos = np.asarray(state["pos"], np.float32)
    i, j, k = axis_index(ex, pos[:, 0]), axis_index(ey, pos[:, 1]), axis_index(ez, pos[:, 2])
    ok = diag_ref.selected(state, diag_ref.EVERYTHING, types_of(lattice)) & (i >= 0) & (j >= 0) & (k >= 0)
    nx, ny = ex.size - 1, ey.size - 1
    return np.where(ok, (k * ny + j) * nx + i, -1).astype(np.int32)


def outer_box(lattice):
    ex, ey, ez = edges(lattice)
    return np.array([ex[0], ey[0], ez[0], ex[-1], ey[-1], ez[-1]], np.float32)


def records(state, lattice, rho0, ids=None):
    """float64[bins, 32]: diag_ref.records over the bins' boxes."""
    return diag_ref.records(state, boxes(lattice), types_of(lattice), rho0, ids)
