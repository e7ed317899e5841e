"""Time sph_stats_accumulate on config #2 (the 1 M cube) after 3 steps: a 128 x 128 x 128 lattice over the whole box
(spacing about 0.39 h: the brick route), masked to liquid.
  (a) stats_accumulate(0) with a synchronise behind it: the new call, nothing read
  (b) the route it replaces, in the same process: sample_grid of the same lattice with its read-back (32 bytes a node), then the
      numpy fold of the records into float64[nodes, 24] on the host (tests/stats_ref.fold). With a library that has no statistics
      (SPHMI_LIB=<the parent commit's build>) only (b) and the step are timed: the yardstick at the parent.
  (c) sample_grid with its read-back alone, stats (the 192-byte read-back of every node) and stats_moments (64 bytes a node)
Prints one JSON line; `agree` says whether the device's accumulators after the timed calls equal the host fold of as many calls, bit
for bit. The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_stats.py` and read k_stats_grid
against k_sample_grid in the stats. The method and its caveats are those of tools/time_gauges.py: wall clock from Python, the first
call a warm-up.

    python tools/time_stats.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import stats_ref  # noqa: E402

BOX, LATTICE, MASK = (50.0, 50.0, 50.0), (100, 100, 100), 0xffff
DIMS = (128, 128, 128)
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
    nodes = int(np.prod(DIMS))
    out = dict(scene="config2", particles=hip.N, step_ms=t_step * 1e3 / (STEPS - 1), dims=list(DIMS), nodes=nodes,
               spacing_over_h=[float(s / np.float32(cfg.h)) for s in spacing])
    host = dict(acc=stats_ref.empty(nodes), calls=0)

    def host_route():
        rec = hip.sample_grid(origin, spacing, DIMS, (1,)).reshape(-1, 8)
        host["acc"] = stats_ref.fold(host["acc"], rec, host["calls"])
        host["calls"] += 1
        return rec

    rec, med, mn = timed(host_route, reps)
    out["host_route"] = dict(median_ms=med, min_ms=mn, readback_bytes=nodes * 32)
    out["wet_nodes"] = int((rec[:, 6] > 0).sum())
    _, med, mn = timed(lambda: hip.sample_grid(origin, spacing, DIMS, (1,)), reps)
    out["sample_grid_with_readback"] = dict(median_ms=med, min_ms=mn)
    if hasattr(hip._L, "sph_stats_accumulate"):
        def no_wait():
            hip.stats_accumulate(0)
            hip.synchronize()

        hip.stats_define(0, origin, spacing, DIMS, (1,))
        hip.synchronize()
        _, med, mn = timed(no_wait, reps)
        out["accumulate"] = dict(median_ms=med, min_ms=mn, accumulator_bytes=nodes * 8 * stats_ref.WORDS)
        (acc, calls), med, mn = timed(lambda: hip.stats(0), 3)
        out["read"] = dict(median_ms=med, min_ms=mn, readback_bytes=int(acc.nbytes))
        _, med, mn = timed(lambda: hip.stats_moments(0), 3)
        out["read_moments"] = dict(median_ms=med, min_ms=mn, readback_bytes=nodes * 4 * stats_ref.MOMENT_WORDS)
        # the same number of calls on the same state, on either route
        out["agree"] = bool(calls == host["calls"] and
                            np.array_equal(acc.reshape(-1, stats_ref.WORDS).view(np.uint64), host["acc"].view(np.uint64)))
        out["speedup"] = out["host_route"]["median_ms"] / out["accumulate"]["median_ms"]
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
