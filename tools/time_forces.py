"""Time sph_force_measure and sph_force_diagnostics on config #4 (the 16.5 M box), config #2 (the 1 M cube) and
the worm, beside the K7 and K12 stage times of the same session (the staged kernels re-run on the same state, as
tools/time_stage.py does; they do the same gathers) and, with --host, beside the route the calls replace: the exports
(sortedPosition, sortedVelocity, rho, pressure, particleIndex, position, the neighbour rows) plus the numpy restatement of
tests/forces_ref.py. Prints one JSON line per scene: the wall times of the blocking calls, the bytes each copies to the host,
and the algorithmic bytes the full-record pass streams (400 B per particle: 240 read -- position, velocity, rho, (rho*, p), the
16-bit ids and their base, the stored distances -- and 160 written; its 32 x 40 B of neighbour gathers are not counted). The
kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_forces.py ...` and read k_force_records,
k_terms_leaf<64, 49, 7>, k_tree_upper (one row for every tree of the run: here the force totals' and the diagnostics') and
k_terms_final<64, 49> beside k_forces and k_pressure_force in the stats.

    python tools/time_forces.py [config4|config2|worm|all] [reps] [--host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import forces_ref as fr  # noqa: E402
import scenes  # noqa: E402

STREAM_BYTES_PER_PARTICLE = 16 + 16 + 4 + 8 + 64 + 4 + 128 + 160


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
    if name == "config2":
        return scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100))
    return scenes.worm_scene()


def host_route(hip):
    """The same records without the library calls: (export ms, numpy ms, bytes exported)."""
    t0 = time.perf_counter()
    state = fr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    t1 = time.perf_counter()
    fr.Forces(state, ids, dist, fr.constants(hip.cfg))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(hip.N * (32 + 16 + 8 + 4 + 8 + 16 + 256))


def run(name, reps, host):
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
    out = dict(scene=name, particles=N, step_ms=(time.perf_counter() - t0) * 1e3 / 5, stream_bytes=N * STREAM_BYTES_PER_PARTICLE)
    everything = [(-np.inf,) * 3 + (np.inf,) * 3]
    sixteen = everything + [(-np.inf, float(cfg.ymax) * k / 15, -np.inf, np.inf, float(cfg.ymax) * (k + 1) / 15, np.inf) for k in range(15)]
    types = (2,) if cfg.numOfElasticP else (1,)
    n_sel = hip.select(types=types, terms=() if cfg.numOfElasticP else (("surface", 0.10, np.inf),))
    buf = {}

    def full():  # into one array: the call, not numpy's allocation of 160 B per particle
        if "a" not in buf:
            buf["a"] = np.empty((N, 40), np.float32)
        hip._chk(hip._L.sph_force_measure(hip._h, 0, buf["a"].ctypes.data))

    calls = {
        "force_measure": (full, N * 160),
        "force_measure_selection": (lambda: hip.force_measure(selection=True), n_sel * 160),
        "force_diagnostics_1": (lambda: hip.force_diagnostics(everything, types), 512),
        "force_diagnostics_16": (lambda: hip.force_diagnostics(sixteen, types), 16 * 512),
        "diagnostics_1": (lambda: hip.diagnostics(everything, types), 256),  # the existing reduction over the same particles
    }
    for key, (fn, nbytes) in calls.items():
        _, med, mn = timed(fn, reps)
        out[key] = dict(median_ms=med, min_ms=mn, bytes=nbytes)
    out["selected"] = n_sel
    if host:
        e, c, b = host_route(hip)
        out["host_route"] = dict(export_ms=e, numpy_ms=c, bytes=b)
    # K7 and K12 of the same session, re-run on the same state (K7's stage time includes its 0.2 ms pack pass)
    for _ in range(3):
        hip._run_pcisph_computeForcesAndInitPressure()
    hip.synchronize(); hip.set_stage_timing(True); hip.reset_stage_times()
    for _ in range(reps):
        hip._run_pcisph_computeForcesAndInitPressure()
    hip.synchronize()
    ms, n = hip.stage_times()["forces"]
    out["k7_forces_ms"] = ms / n
    hip._run_pcisph_predictPositions(); hip._run_pcisph_predictDensity(); hip._run_pcisph_correctPressure()
    for _ in range(3):
        hip._run_pcisph_computePressureForceAcceleration()
    hip.synchronize(); hip.reset_stage_times()
    for _ in range(reps):
        hip._run_pcisph_computePressureForceAcceleration()
    hip.synchronize()
    ms, n = hip.stage_times()["pressure_force"]
    out["k12_pressure_force_ms"] = ms / n
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "all"
    reps = int(args[1]) if len(args) > 1 else 10
    for name in (("worm", "config2", "config4") if which == "all" else (which,)):
        run(name, reps, host="--host" in sys.argv)
