"""Time sph_sample_grid (the brick kernel) on the 1M cube of config #2 and on config #4 (16.5 M particles), grids of spacing h/2
over the whole box (config #4: about as many grid points as particles). Prints, per scene, the wall time of a blocking
sample_grid call (kernel + device-to-host copy of the records) and points/s. The kernel time alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_sample.py` and read k_sample_grid in the stats.

    python tools/time_sample.py [1M|16M|both] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402

WORK = {"1M": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "16M": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}


def run(name, reps):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    h = np.float32(cfg.h)
    sp = h / np.float32(2)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    extent = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) - origin
    dims = [int(e / sp) + 1 for e in extent]
    npts = dims[0] * dims[1] * dims[2]
    g = hip.sample_grid(origin, (sp, sp, sp), dims)  # warm-up (allocates the scratch)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip.sample_grid(origin, (sp, sp, sp), dims)
        ts.append((time.perf_counter() - t0) * 1e3)
    liquid = g[..., 1][g[..., 6] > 0]
    res = dict(scene=name, particles=int(cfg.particleCount), dims=dims, points=npts, spacing_over_h=0.5,
               wall_ms_median=float(np.median(ts)), wall_ms_min=float(np.min(ts)), points_per_s=npts / (float(np.min(ts)) * 1e-3),
               mean_count=float(g[..., 6].mean()), shepard_median_where_hit=float(np.median(liquid)) if liquid.size else 0.0)
    hip.close()
    return res


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for name in (["1M", "16M"] if which == "both" else [which]):
        print(json.dumps(run(name, reps)), flush=True)
