"""Time sph_measure_surface (shells, area and enclosed volume of the extracted mesh) on the 1M cube of config #2 or
on config #4 (16.5 M particles), on the mesh sph_extract_surface cuts on a lattice of spacing `spacing_over_h` * h over the whole
box (tools/time_surface.py's lattices). Prints, per scene, the wall time of the blocking measure call, of the blocking table read
(sph_read_shells), of one extraction (call + device synchronise, for scale), and of the host route the measure replaces: the
blocking mesh read (sph_read_surface) plus tests/shell_ref.py on one core (once: it takes seconds to minutes).
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_shells.py ...` and read k_sh_*, k_cc_* and,
for the extraction, k_sample_grid and k_surface_* in the stats.

    python tools/time_shells.py [1M|16M|both] [reps] [spacing_over_h] [host: 1 or 0]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import shell_ref  # noqa: E402
import sphmi  # noqa: E402

WORK = {"1M": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "16M": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}


def run(name, reps, spacing_over_h, host):
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
    spacing = np.array([sp, sp, sp], np.float32)
    L, h = hip._L, hip._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    counts2, counts4, exps = np.zeros(2, np.int64), np.zeros(4, np.int64), np.zeros(3, np.int32)
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=0.5, field="shepard", types=(1,))  # warm-up (allocates)
    m = hip.measure_surface()
    vs, table, bb = hip.surface_shells()
    t_ext, t_measure, t_read = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip._chk(L.sph_extract_surface(h, ptr(origin), ptr(spacing), ptr(dims), sphmi.type_mask((1,)), 1, 0.5, ptr(counts2)))
        hip._chk(L.sph_synchronize(h))
        t1 = time.perf_counter()
        hip._chk(L.sph_measure_surface(h, ptr(counts4), ptr(exps)))
        t2 = time.perf_counter()
        hip._chk(L.sph_read_shells(h, ptr(vs), ptr(table), ptr(bb)))
        t3 = time.perf_counter()
        t_ext.append((t1 - t0) * 1e3)
        t_measure.append((t2 - t1) * 1e3)
        t_read.append((t3 - t2) * 1e3)
    res = dict(scene=name, particles=int(cfg.particleCount), dims=dims.tolist(), spacing_over_h=spacing_over_h,
               vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), measure=m,
               measure_ms_median=float(np.median(t_measure)), measure_ms_min=float(np.min(t_measure)),
               read_shells_ms_median=float(np.median(t_read)), extract_ms_median=float(np.median(t_ext)))
    if host:
        t0 = time.perf_counter()
        hip._chk(L.sph_read_surface(h, ptr(verts), ptr(tris)))
        t1 = time.perf_counter()
        ref = shell_ref.measure(verts, tris, origin, spacing, dims)
        t2 = time.perf_counter()
        res.update(host_read_surface_ms=(t1 - t0) * 1e3, host_shell_ref_ms=(t2 - t1) * 1e3,
                   host_equal=bool(np.array_equal(ref["table"], table) and np.array_equal(ref["vertexShell"], vs)
                                   and ref["counts"].tolist() == counts4.tolist()))
    hip.close()
    return res


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    spacing_over_h = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
    host = bool(int(sys.argv[4])) if len(sys.argv) > 4 else True
    for name in (["1M", "16M"] if which == "both" else [which]):
        print(json.dumps(run(name, reps, spacing_over_h, host)), flush=True)
