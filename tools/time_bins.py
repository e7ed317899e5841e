"""Time sph_bin_diagnostics (k_bin_index, k_bin_scan, k_bin_leaf, k_bin_upper) on the 1M cube of config #2 after two
steps, for a 64 x 64 plan-view map, a 64-bin z profile and a 16 x 16 x 16 lattice, each beside the route a caller had before it:
the loop of sph_diagnostics over the same boxes, 16 per call. Prints one JSON line: medians and minima of the wall times of the
blocking calls, their ratio, and that both routes returned the same bits. The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_bins.py ...` and read the four k_bin_* kernels against k_diag_leaf and
k_tree_upper (each lattice runs reps + 1 bin calls, then loop_reps + 1 loops).

    python tools/time_bins.py [reps] [loop_reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import sphmi  # noqa: E402
from sphmi import frames  # noqa: E402

WORK = ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff)
TYPES = (1, 2)


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def loop(hip, boxes):
    return np.concatenate([hip.diagnostics(boxes[b:b + 16], TYPES) for b in range(0, boxes.shape[0], 16)])


def run(reps, loop_reps):
    box, lat, mask = WORK
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float64)
    ext = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float64) - lo
    lattices = {"plan_64x64": sphmi.bin_lattice((lo[0], 0, lo[2]), (ext[0] / 64, 0, ext[2] / 64), (64, 1, 64), TYPES),
                "z_profile_64": sphmi.bin_lattice((0, 0, lo[2]), (0, 0, ext[2] / 64), (1, 1, 64), TYPES),
                "lattice_16x16x16": sphmi.bin_lattice(lo, ext / 16, (16, 16, 16), TYPES)}
    res = dict(scene="1M", particles=int(cfg.particleCount), reps=reps, loop_reps=loop_reps)
    for name, g in lattices.items():
        boxes = frames.bin_boxes(g)
        rec, b_med, b_min = timed(lambda: hip.bin_diagnostics(g), reps)
        want, l_med, l_min = timed(lambda: loop(hip, boxes), loop_reps)
        same = bool(np.array_equal(rec.reshape(-1, 32).view(np.uint64), want.view(np.uint64)))
        res[name] = dict(bins=int(boxes.shape[0]), occupied=int((rec[..., 0] > 0).sum()), selected=int(rec[..., 0].sum()),
                         bin_diagnostics_ms_median=b_med, bin_diagnostics_ms_min=b_min, diagnostics_loop_ms_median=l_med,
                         diagnostics_loop_ms_min=l_min, loop_over_bins=l_med / b_med, same_bits=same)
    hip.close()
    return res


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    loop_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps(run(reps, loop_reps)), flush=True)
