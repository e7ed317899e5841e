"""Time sph_elastic_measure, sph_muscle_diagnostics and sph_membrane_measure on the worm scene (10,143 elastic
particles, 96 muscles, 11,386 triangles) and on the stacked sheets of tests/test_elastic.py (33,792 elastic particles, 264
muscles, 66,120 triangles: a three-level group tree), beside the route they replace: the exports a user needs today (the sorted
positions and particleIndexBack through sph_read_buffer) and the numpy restatement of tests/elastic_ref.py on the host. Prints,
per scene, the wall times of the blocking calls and the bytes each copies to the host. The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_elastic.py ... --no-host` and read k_elastic_terms, k_muscle_fill,
k_muscle_leaf, k_tree_upper (the upper levels of the group tree and of the area tree), k_muscle_final and k_membrane_measure beside the step's k_elastic in the trace.

    python tools/time_elastic.py [worm|sheets|both] [reps] [--no-host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import elastic_ref as er  # noqa: E402
import scenes  # noqa: E402
import sphmi  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def host_route(hip, sc, signal):
    """The same numbers without the library calls: (export ms, numpy ms, bytes exported)."""
    cfg = sc["cfg"]
    t0 = time.perf_counter()
    sp, back, c = er.solver_inputs(hip, sc, signal)
    t1 = time.perf_counter()
    er.elastic_records_fast(c)
    er.muscle_records(c, cfg.muscleCount, signal)
    if cfg.numOfMembranes:
        er.membrane_records(sp, back, sc["membranes"])
    t2 = time.perf_counter()
    # sph_read_buffer copies the whole buffers: sortedPosition (both halves) and particleIndexBack; building the connection
    # terms is counted as numpy time above (solver_inputs does both: split by a second clock inside would say the same)
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(hip.N * (32 + 4))


def run(name, reps, host=True):
    if name == "worm":
        sc = scenes.worm_scene()
        signal = sphmi.muscle_signal(100, sc["cfg"].muscleCount)
    else:
        import test_elastic
        sc = test_elastic.stacked_sheets()
        signal = np.random.default_rng(20261017).uniform(-0.5, 1.0, sc["cfg"].muscleCount).astype(np.float32)
    cfg = sc["cfg"]
    E, M, G = cfg.numOfElasticP, cfg.numOfMembranes, cfg.muscleCount
    hip = scenes.hip_for(sc)
    hip.updateMuscleActivityData(signal)
    t0 = time.perf_counter()
    for it in range(10):
        hip.step(it)
    hip.synchronize()
    out = dict(scene=name, particles=hip.N, elastic=E, slots=E * 32, muscles=G, triangles=M, step_ms=(time.perf_counter() - t0) * 1e3 / 10)
    calls = {
        "elastic_measure": (lambda: hip.elastic_measure(), E * (4 + 4 + 48 + 256)),
        "elastic_measure_records_only": (lambda: hip.elastic_measure(connections=False), E * (4 + 4 + 48)),
        "muscle_diagnostics": (lambda: hip.muscle_diagnostics(), (G + 1) * 128),
        "membrane_measure": (lambda: hip.membrane_measure(), M * 32 + 136),
        "membrane_measure_totals_only": (lambda: hip.membrane_measure(records=False), 136),
    }
    for key, (fn, nbytes) in calls.items():
        _, med, mn = timed(fn, reps)
        out[key] = dict(median_ms=med, min_ms=mn, bytes=nbytes)
    if host:
        t = [host_route(hip, sc, signal) for _ in range(3)]
        out["host_route"] = dict(export_ms=float(np.median([x[0] for x in t])), numpy_ms=float(np.median([x[1] for x in t])), bytes=t[0][2])
    mus = hip.muscle_diagnostics()
    out["connections"] = float(mus[:, 0].sum())
    hip.close()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 30
    for name in (("worm", "sheets") if which == "both" else (which,)):
        run(name, reps, host="--no-host" not in sys.argv)
