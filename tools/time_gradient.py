"""Time sph_sample_gradient_grid (the brick kernel k_gradient_grid) beside sph_sample_grid, and sph_surface_normals
on the liquid's Shepard = 0.5 surface, on the 1M cube of config #2 or on config #4 (16.5 M particles), lattices of spacing h/2
over the whole box with all particle types. Prints, per scene, the wall times of the blocking sample_grid and
sample_gradient_grid calls (kernels + device-to-host copies of the 32-B / 128-B records), of the blocking normals call and the
mesh size. The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_gradient.py ...` and read
k_sample_grid, k_gradient_grid and k_surface_normals in the stats (the same workload for both grid kernels in one run).

    python tools/time_gradient.py [1M|16M|both] [reps]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import sphmi  # noqa: E402

WORK = {"1M": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "16M": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}


def run(name, reps):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    sp = np.float32(cfg.h) / np.float32(2)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    extent = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) - origin
    dims = np.array([int(e / sp) + 1 for e in extent], np.int32)
    npts = int(dims[0]) * int(dims[1]) * int(dims[2])
    spacing = np.array([sp, sp, sp], np.float32)
    L, h = hip._L, hip._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    mask_all = sphmi.type_mask((1, 2, 3))
    fields = np.empty((npts, 8), np.float32)
    grads = np.empty((npts, 32), np.float32)
    hip._chk(L.sph_sample_grid(h, ptr(origin), ptr(spacing), ptr(dims), mask_all, ptr(fields)))  # warm-up (allocates)
    hip._chk(L.sph_sample_gradient_grid(h, ptr(origin), ptr(spacing), ptr(dims), mask_all, ptr(grads)))
    t_s, t_g = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip._chk(L.sph_sample_grid(h, ptr(origin), ptr(spacing), ptr(dims), mask_all, ptr(fields)))
        t1 = time.perf_counter()
        hip._chk(L.sph_sample_gradient_grid(h, ptr(origin), ptr(spacing), ptr(dims), mask_all, ptr(grads)))
        t2 = time.perf_counter()
        t_s.append((t1 - t0) * 1e3)
        t_g.append((t2 - t1) * 1e3)
    hit = grads[:, 6] > 0
    vort = np.linalg.norm(grads[hit, 26:29], axis=1)
    verts, _ = hip.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1,))
    normals = np.empty_like(verts)
    hip._chk(L.sph_surface_normals(h, ptr(normals)))  # warm-up
    t_n = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip._chk(L.sph_surface_normals(h, ptr(normals)))
        t_n.append((time.perf_counter() - t0) * 1e3)
    res = dict(scene=name, particles=int(cfg.particleCount), dims=dims.tolist(), points=npts, spacing_over_h=0.5,
               sample_grid_ms_median=float(np.median(t_s)), sample_grid_ms_min=float(np.min(t_s)),
               gradient_grid_ms_median=float(np.median(t_g)), gradient_grid_ms_min=float(np.min(t_g)),
               gradient_bytes=128 * npts, mean_count=float(grads[:, 6].mean()),
               vorticity_median_where_hit=float(np.median(vort)) if vort.size else 0.0,
               vertices=int(verts.shape[0]), normals_ms_median=float(np.median(t_n)), normals_ms_min=float(np.min(t_n)),
               unit_normals=float((np.abs(np.linalg.norm(normals, axis=1) - 1) < 1e-6).mean()) if verts.size else 0.0)
    hip.close()
    return res


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for name in (["1M", "16M"] if which == "both" else [which]):
        print(json.dumps(run(name, reps)), flush=True)
