"""The lattices of the binned-diagnostics tests (tests/test_bins_host.py on the oracle, tests/test_bins.py on the GPU), made from a
scene's input alone so that both sides bin the same boxes. Inputs only.

Every lattice but "outside" starts one bin in front of the matter on its first binned axis, so it always has empty bins, and is
sized to the matter its mask selects, so that fewer than half of its bins are empty for every mask. tests/test_bins_host.py asserts on the oracle's state what the GPU test relies on."""
import numpy as np

import sphmi

f32 = np.float32
SCENES = ("tiny_jitter", "tiny_compressed", "tiny_elastic")
MASKS = [(1,), (1, 2), (1, 2, 3)]
NAMES = ("plan", "zprofile", "fine3d", "part", "outside")
FULL = ("plan", "zprofile", "fine3d")  # the lattices that cover all the matter


def extent(scene, types):
    """(lo, hi) of the scene's initial particles of the given types, with a margin of one smoothing length: where the selected
    matter is, and still is after the few steps the tests take."""
    pos = np.asarray(scene["position"], np.float32)
    t = pos[:, 3].astype(np.int32)
    sel = np.isin(t, list(types))
    assert sel.any()
    h = float(scene["cfg"].h)
    return pos[sel, :3].astype(np.float64).min(0) - h, pos[sel, :3].astype(np.float64).max(0) + h


def lattices(scene, types):
    """The five lattices for one mask, sized to the extent of the matter that mask selects, so that most bins hold particles
    whichever mask it is."""
    lo, hi = extent(scene, types)
    ext = hi - lo
    h = float(scene["cfg"].h)
    out = {}
    # a plan-view map: y is the whole axis; 5 x 4 bins over the matter and a column in front of it on x
    out["plan"] = sphmi.bin_lattice((lo[0] - ext[0] / 5, 0, lo[2]), (ext[0] / 5, 0, ext[2] / 4), (6, 1, 4), types)
    # a z profile: 6 bins over the matter, one in front, one behind
    out["zprofile"] = sphmi.bin_lattice((0, 0, lo[2] - ext[2] / 6), (0, 0, ext[2] / 6), (1, 1, 8), types)
    # 3-D with a spacing below the cell size h in x: one chunk of 1024 holds many bins
    nx = int(np.ceil(ext[0] / (0.45 * h))) + 1
    out["fine3d"] = sphmi.bin_lattice((lo[0] - 0.45 * h, lo[1], lo[2]), (0.45 * h, ext[1] / 2, ext[2] / 2), (nx, 2, 2), types)
    # part of the matter only
    out["part"] = sphmi.bin_lattice(lo + ext * (0.3, 0.1, 0.25), ext * (0.15, 0.3, 0.2), (3, 2, 2), types)
    # wholly outside: every record is the empty record
    out["outside"] = sphmi.bin_lattice(hi + 100, (1, 1, 1), (2, 2, 2), types)
    assert tuple(out) == NAMES
    return out


def edge_lattices(cfg, types):
    """For the chunk-edge scenes (tests/tree_edge_cases.py): a few bins per axis over the whole box and a margin around it, and the
    (1, 1, 1) lattice of three whole axes, whose one record is the record of everything."""
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float64) - 1.0
    ext = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float64) + 1.0 - lo
    return {"few": sphmi.bin_lattice(lo, ext / (3, 2, 3), (3, 2, 3), types), "one": sphmi.bin_lattice((0, 0, 0), (0, 0, 0), (1, 1, 1), types)}


def chunks_of(index, bins):
    """int[bins]: in how many different chunks of 1024 sorted particles each bin has members."""
    idx = np.asarray(index)
    sel = np.flatnonzero(idx >= 0)
    pairs = np.unique(np.stack([idx[sel].astype(np.int64), sel // 1024], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=bins)
