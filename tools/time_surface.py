"""Time sph_extract_surface (marching cubes over a sampled field) on the 1M cube of config #2 or on config #4
(16.5 M particles), on a lattice of spacing `spacing_over_h` * h over the whole box. Prints, per scene, the wall time of the
extract call followed by a device synchronise (sampling + extraction kernels; the call itself blocks only for the counts), the
wall time of the blocking mesh read (sph_read_surface), the mesh sizes and the algorithmic bytes of each extraction kernel.
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_surface.py ...` and read k_sample_grid
and k_surface_* in the stats.

    python tools/time_surface.py [1M|16M|both] [reps] [spacing_over_h] [field] [iso] [types, e.g. 1 or 12]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import sphmi  # noqa: E402
from sphmi import frames  # noqa: E402

WORK = {"1M": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "16M": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}
SURF_BLOCK = 256  # points per block of the classify / emit kernels (sph_surface.hip)


def kernel_bytes(P, V, T):
    """Bytes each extraction kernel must move at least: the lattice (4 B per point), codes (2 B), vertex bases (4 B), per-block
    totals (8 B) and offsets (16 B), vertices and triangles (12 B each). k_surface_field reads whole 32-B records."""
    nb = (P + SURF_BLOCK - 1) // SURF_BLOCK
    return {"k_surface_field": 32 * P + 4 * P, "k_surface_classify": 4 * P + 2 * P + 8 * nb,
            "k_surface_scan": 8 * nb + 16 * nb, "k_surface_vertices": 2 * P + 8 * nb + 4 * P + 8 * V + 12 * V,
            "k_surface_triangles": 2 * P + 8 * nb + 12 * T}


def run(name, reps, spacing_over_h, field, iso, types):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    sp = np.float32(cfg.h) * np.float32(spacing_over_h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    extent = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) - origin
    dims = np.array([int(e / sp) + 1 for e in extent], np.int32)
    P = int(dims[0]) * int(dims[1]) * int(dims[2])
    spacing = np.array([sp, sp, sp], np.float32)
    word = frames.GRID_FIELDS.index(field) if not field.isdigit() else int(field)
    counts = np.zeros(2, np.int64)
    L, h = hip._L, hip._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=iso, field=word, types=types)  # warm-up (allocates)
    t_ext, t_read = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip._chk(L.sph_extract_surface(h, ptr(origin), ptr(spacing), ptr(dims), sphmi.type_mask(types), word, iso, ptr(counts)))
        hip._chk(L.sph_synchronize(h))
        t1 = time.perf_counter()
        hip._chk(L.sph_read_surface(h, ptr(verts), ptr(tris)))
        t2 = time.perf_counter()
        t_ext.append((t1 - t0) * 1e3)
        t_read.append((t2 - t1) * 1e3)
    V, T = int(counts[0]), int(counts[1])
    assert (V, T) == verts.shape[:1] + tris.shape[:1]
    res = dict(scene=name, particles=int(cfg.particleCount), dims=dims.tolist(), points=P, spacing_over_h=spacing_over_h,
               field=frames.GRID_FIELDS[word], iso=iso, types=list(types), vertices=V, triangles=T,
               mesh_bytes=12 * (V + T), extract_ms_median=float(np.median(t_ext)), extract_ms_min=float(np.min(t_ext)),
               read_ms_median=float(np.median(t_read)), read_ms_min=float(np.min(t_read)),
               kernel_bytes=kernel_bytes(P, V, T))
    hip.close()
    return res


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    spacing_over_h = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
    field = sys.argv[4] if len(sys.argv) > 4 else "shepard"
    iso = float(sys.argv[5]) if len(sys.argv) > 5 else 0.5
    types = tuple(int(c) for c in sys.argv[6]) if len(sys.argv) > 6 else (1,)
    for name in (["1M", "16M"] if which == "both" else [which]):
        print(json.dumps(run(name, reps, spacing_over_h, field, iso, types)), flush=True)
