"""Time sph_probes_record on config #2 (the 1 M cube) after 3 steps: a 128 x 128 map of 128-point lines along z over
the whole box (frames.level_columns: the Shepard sum of the liquid against 0.5), and 4096 point probes spread through the box.
  (a) probes_record(read=False) with a synchronise behind it, lines alone          (b) the same with read=True
  (c) the same two with the point probes alone
  (d) the route the level probes replace, in the same process: sample_grid of the same 128 x 128 x 128 lattice with its read-back
      (32 bytes a lattice point), then frames.free_surface_height on the host. With a library that has no probes
      (SPHMI_LIB=<the parent commit's build>) only (d) and the step are timed: the yardstick at the parent.
  (e) sample_points of the same 4096 points: the blocking route a point probe replaces.
Prints one JSON line; `agree` says whether the two routes put the level into the same lattice interval in every column. The kernel
times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_probes.py` and read k_probe_levels against
k_sample_grid in the stats (the brick walk is cheaper per point, the level search stops at the first chunk that decides a line).
The method and its caveats are those of tools/time_gauges.py: wall clock from Python, the first call a warm-up.

    python tools/time_probes.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
from sphmi import frames  # noqa: E402

BOX, LATTICE, MASK = (50.0, 50.0, 50.0), (100, 100, 100), 0xffff
DIMS = (128, 128, 128)
POINTS = 4096
STEPS = 3


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def run(reps):
    sc = scenes.liquid_box(BOX, LATTICE, mask=MASK)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    t_step = 0.0
    for it in range(STEPS):
        hip.synchronize()
        t0 = time.perf_counter()
        hip.step(it)
        hip.synchronize()
        if it >= 1:
            t_step += time.perf_counter() - t0
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
    extent = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) - origin
    spacing = (extent / (np.array(DIMS, np.float32) - np.float32(1))).astype(np.float32)
    pts = (origin + np.random.default_rng(5).uniform(0.0, 1.0, (POINTS, 3)).astype(np.float32) * extent).astype(np.float32)
    out = dict(scene="config2", particles=hip.N, step_ms=t_step * 1e3 / (STEPS - 1), dims=list(DIMS), lines=DIMS[0] * DIMS[1],
               line_points=DIMS[2], spacing_over_h=[float(s / np.float32(cfg.h)) for s in spacing], points=POINTS)

    def lattice_route():
        grid = hip.sample_grid(origin, spacing, DIMS, (1,))
        return frames.free_surface_height(grid, origin, spacing, 0.5)

    height, med, mn = timed(lattice_route, reps)
    out["lattice_route"] = dict(median_ms=med, min_ms=mn, readback_bytes=int(np.prod(DIMS)) * 32)
    _, med, mn = timed(lambda: hip.sample_grid(origin, spacing, DIMS, (1,)), reps)
    out["sample_grid_with_readback"] = dict(median_ms=med, min_ms=mn)
    _, med, mn = timed(lambda: hip.sample_points(pts, (1,)), reps)
    out["sample_points"] = dict(median_ms=med, min_ms=mn)
    if hasattr(hip._L, "sph_probes_record"):
        def no_wait():
            hip.probes_record(read=False)
            hip.synchronize()

        hip.probes_set_lines(frames.level_columns(origin, spacing, DIMS, axis=2, field="shepard", iso=0.5, types=(1,)))
        hip.probes_history(64)
        _, med, mn = timed(no_wait, reps)
        out["levels_no_read"] = dict(median_ms=med, min_ms=mn)
        rec, med, mn = timed(lambda: hip.probes_record(read=True)[1], reps)
        out["levels_read"] = dict(median_ms=med, min_ms=mn, readback_bytes=int(rec.nbytes))
        status = rec[:, 4].astype(int)
        out["found_dry_submerged"] = [int((status == s).sum()) for s in (0, 1, 2)]
        out["mean_points_from_far_end"] = float((DIMS[2] - 1 - rec[status == 0, 5]).mean()) if (status == 0).any() else None
        got = frames.level_heights(rec, 2).reshape(DIMS[1], DIMS[0])
        same = np.isnan(got) == np.isnan(height)
        both = ~np.isnan(got) & ~np.isnan(height)
        out["agree"] = bool(same.all() and (np.abs(got[both] - height[both]) <= float(spacing[2])).all())
        hip.probes_set_lines(None)
        hip.probes_set_points(pts, (1,))
        _, med, mn = timed(no_wait, reps)
        out["points_no_read"] = dict(median_ms=med, min_ms=mn)
        _, med, mn = timed(lambda: hip.probes_record(read=True), reps)
        out["points_read"] = dict(median_ms=med, min_ms=mn)
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
