"""Time sph_gauges_accumulate on config #2 (the 1 M cube) and config #4 (the 16.5 M box) whose liquid was given the
velocities of tests/gauge_cases.py (+-0.25 per axis), with 1 and with 16 gauges across the moving liquid (the gauges of
gauge_cases.gauges_of: planes, rectangles, tilted parallelograms):
  (a) gauges_accumulate(read=False) with a synchronise behind it      (b) the same with read=True
  (c) with --host, the only route there is without the call: sph_read_position + sph_read_velocity + the particle index and the
      sorted positions, and the numpy restatement of tests/gauge_ref.py for one gauge
  (d) sph_diagnostics with one region on the same state: the yardstick, a pass that streams at least as many bytes through a wider
      tree. With a library that has no gauges (SPHMI_LIB=<the parent commit's build>) only (d) and the step are timed.
Prints one JSON line per scene. The leaf streams 36 B per particle (sortedPos 16, vals 4, the gather of posOrig 16). The kernel
times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_gauges.py` and read k_gauge_leaf, k_gauge_final and
k_tree_upper (shared by every tree: this tool's diagnostics_1 calls are in the same row) in the stats. The method and its caveats are those of tools/time_wall.py: wall clock from Python, the first call a
warm-up.

    python tools/time_gauges.py [config2|config4|both] [reps] [--host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import gauge_cases as gc  # noqa: E402
import gauge_ref as gr  # noqa: E402
import scenes  # noqa: E402

WORK = {"config2": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "config4": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}
STREAM_BYTES_PER_PARTICLE = 16 + 4 + 16
STEPS = 3


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def run(name, reps, host):
    box, lattice, mask = WORK[name]
    sc = gc.seeded(scenes.liquid_box(box, lattice, mask=mask))
    gauges = gc.gauges_of(sc, (1,))
    hip = scenes.hip_for(sc)
    t_step = 0.0
    for it in range(STEPS):
        hip.synchronize()
        t0 = time.perf_counter()
        hip.step(it)
        hip.synchronize()
        if it >= 1:
            t_step += time.perf_counter() - t0
    N = hip.N
    out = dict(scene=name, particles=N, step_ms=t_step * 1e3 / (STEPS - 1), stream_bytes=N * STREAM_BYTES_PER_PARTICLE)
    everything = [(-np.inf,) * 3 + (np.inf,) * 3]
    _, med, mn = timed(lambda: hip.diagnostics(everything, (1,)), reps)
    out["diagnostics_1"] = dict(median_ms=med, min_ms=mn)
    if hasattr(hip._L, "sph_gauges_accumulate"):
        def no_wait():
            hip.gauges_accumulate(read=False)
            hip.synchronize()

        for count in (1, 16):
            for slot in range(16):
                hip.gauge_define(slot) if slot >= count else hip.gauge_define(slot, **gauges[slot])
            _, med, mn = timed(no_wait, reps)
            out["accumulate_%d_no_read" % count] = dict(median_ms=med, min_ms=mn)
            rec, med, mn = timed(lambda: hip.gauges_accumulate(read=True), reps)
            out["accumulate_%d_read" % count] = dict(median_ms=med, min_ms=mn)
            out["crossings_%d" % count] = [int(rec[:count, 0].sum()), int(rec[:count, 8].sum())]
        # the same 16 gauges moved out of the scene: the side tests of every particle, no crossing, no tree
        away = np.full(3, 4.0 * max(float(sc["cfg"].xmax), float(sc["cfg"].ymax), float(sc["cfg"].zmax)), np.float32)
        for slot in range(16):
            hip.gauge_define(slot, **dict(gauges[slot], origin=np.asarray(gauges[slot]["origin"], np.float32) + away))
        _, med, mn = timed(no_wait, reps)
        rec = hip.gauges_accumulate(read=True)
        out["accumulate_16_away_no_read"] = dict(median_ms=med, min_ms=mn)
        out["crossings_16_away"] = [int(rec[:, 0].sum()), int(rec[:, 8].sum())]
        for slot in range(16):
            hip.gauge_define(slot, **gauges[slot])
        _, med, mn = timed(lambda: hip.gauge_crossings(0), reps)
        out["crossing_list_gauge_0"] = dict(median_ms=med, min_ms=mn)
    if host:
        t0 = time.perf_counter()
        state = gr.solver_state(hip)
        t1 = time.perf_counter()
        gr.record(state, gauges[0])
        t2 = time.perf_counter()
        out["host_route_1"] = dict(export_ms=(t1 - t0) * 1e3, numpy_ms=(t2 - t1) * 1e3, bytes=int(N * (16 + 16 + 8 + 32)))
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "config2"
    for scene in (("config2", "config4") if which == "both" else (which,)):
        run(scene, int(args[1]) if len(args) > 1 else 10, host="--host" in sys.argv)
