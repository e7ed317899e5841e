"""Time the carried-field calls on config #2 (the 1 M cube) and config #4 (the 16.5 M box), beside the K7
(`forces`) stage time of the same session (the staged kernel re-run on the same state, as tools/time_forces.py does). K7 streams
the same rows and issues two 16-byte gathers per neighbour plus its pack pass where k_field_diffuse issues one 8-byte gather, so
a substep slower than K7 is a defect to explain. Prints one JSON line per scene: the wall times of the blocking calls
(field_diffuse with 0, 1 and 8 substeps -- each includes the pack pass and the one wait for the stability number, so the cost
of a substep is (t8 - t1) / 7 --, field_diagnostics with 1 and 16 regions, field_set_region) and the algorithmic bytes a substep
streams per particle (216: the 8-byte record read and written, 64 of 16-bit ids, 128 of stored distances, 4 of the row base, 4 of
vals on the last one; its 32 x 8 B of neighbour gathers are not counted). The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_fields.py ...` and read k_field_pack, k_field_diffuse, k_field_leaf beside
k_forces in the stats.

    python tools/time_fields.py [config2|config4|all] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402

SUBSTEP_BYTES_PER_PARTICLE = 8 + 8 + 64 + 128 + 4 + 4


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def scene(name):
    if name == "config4":
        return scenes.liquid_box((78.0, 50.0, 470.0), (160, 100, 1000), mask=0xffffffff)
    return scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100))


def run(name, reps):
    sc = scene(name)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    hip.synchronize()
    t0 = time.perf_counter()
    for it in range(3, 8):
        hip.step(it)
    hip.synchronize()
    N = hip.N
    out = dict(scene=name, particles=N, step_ms=(time.perf_counter() - t0) * 1e3 / 5, substep_stream_bytes=N * SUBSTEP_BYTES_PER_PARTICLE)
    everything = [(-np.inf,) * 3 + (np.inf,) * 3]
    sixteen = everything + [(-np.inf, float(cfg.ymax) * k / 15, -np.inf, np.inf, float(cfg.ymax) * (k + 1) / 15, np.inf) for k in range(15)]
    half = (-np.inf, -np.inf, -np.inf, 0.5 * float(cfg.xmax), np.inf, np.inf)
    hip.field_create(0)
    out["painted"] = hip.field_set_region(0, 1.0, half, (1,))
    sigma = hip.field_diffuse(0, 1e-9, 0, (1,))
    coefficient = 0.25e-9 / sigma  # a quarter of the stability limit
    out["stability"] = hip.field_diffuse(0, coefficient, 0, (1,))
    calls = {
        "field_diffuse_0": lambda: hip.field_diffuse(0, coefficient, 0, (1,)),
        "field_diffuse_1": lambda: hip.field_diffuse(0, coefficient, 1, (1,)),
        "field_diffuse_8": lambda: hip.field_diffuse(0, coefficient, 8, (1,)),
        "field_diagnostics_1": lambda: hip.field_diagnostics(0, everything, (1,)),
        "field_diagnostics_16": lambda: hip.field_diagnostics(0, sixteen, (1,)),
        "field_set_region": lambda: hip.field_set_region(0, 1.0, half, (1,)),
        "diagnostics_1": lambda: hip.diagnostics(everything, (1,)),  # the existing reduction over the same particles
    }
    for key, fn in calls.items():
        _, med, mn = timed(fn, reps)
        out[key] = dict(median_ms=med, min_ms=mn)
    out["substep_ms"] = (out["field_diffuse_8"]["median_ms"] - out["field_diffuse_1"]["median_ms"]) / 7
    # K7 of the same session, re-run on the same state (its stage time includes its pack pass)
    for _ in range(3):
        hip._run_pcisph_computeForcesAndInitPressure()
    hip.synchronize(); hip.set_stage_timing(True); hip.reset_stage_times()
    for _ in range(reps):
        hip._run_pcisph_computeForcesAndInitPressure()
    hip.synchronize()
    ms, n = hip.stage_times()["forces"]
    out["k7_forces_ms"] = ms / n
    out["substep_over_k7"] = out["substep_ms"] / out["k7_forces_ms"]
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "all"
    reps = int(args[1]) if len(args) > 1 else 10
    for name in (("config2", "config4") if which == "all" else (which,)):
        run(name, reps)
