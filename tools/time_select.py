"""Time sph_select_particles, sph_read_selection and sph_particle_measure on the 1M cube of config #2 or on
config #4 (16.5 M particles) for (a) a box and a type only, (b) the liquid with a surface measure >= 0.10, (c) one component of a
labelling, beside the route they replace: the full exports (sorted positions, velocities, density, pressure, the index pairs, the
orig-order positions for the types, and for (b) the neighbour rows) and the numpy filter of tests/select_ref.py on the host.
Prints, per scene, the wall times of the blocking calls and the bytes each read-back moved. The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_select.py ... --no-host` and read the k_select_* / k_particle_measure
kernels in the trace (the selections come in the order (a), (b), (c), each reps + 1 times, each followed by its read-back).

The host route with the rows runs on config2 only (on config4 the 528 M row entries alone are 4 GB of read-back) unless --host-all.

    python tools/time_select.py [config2|config4|both] [reps] [--no-host] [--host-all]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import components_ref as cr  # noqa: E402
import diag_ref  # noqa: E402
import scenes  # noqa: E402
import select_ref as sr  # noqa: E402

WORK = {"config2": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "config4": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}
RECORD_BYTES = 4 + 4 + 48  # per selected particle: sorted index, original id, 12-word record


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def host_route(hip, region, types, terms, with_rows):
    """The same selection without the library calls: (export ms, filter ms, bytes exported, selected)."""
    t0 = time.perf_counter()
    state = diag_ref.state_with_ids(hip)
    N = hip.N
    nbytes = N * (32 + 16 + 8 + 4 + 8 + 16)  # sortedPosition (both halves), sortedVelocity, rho (both halves), pressure, index, position
    rows = None
    if with_rows:
        rows = cr.neighbor_rows(hip)
        nbytes += N * (128 + 64 + 4)  # what sph_read_neighbor_rows copies per particle: both id rows and the base
    t1 = time.perf_counter()
    q = sr.Quantities(state, rows)
    idx = sr.select(state, q, region, types, terms)
    sr.records(state, q, idx)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(nbytes), int(idx.size)


def run(name, reps, host=True, host_rows=True):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    N = int(cfg.particleCount)
    span = [float(getattr(cfg, ax + "max") - getattr(cfg, ax + "min")) for ax in "xyz"]
    region = (0.25 * span[0], 0.25 * span[1], 0.25 * span[2], 0.5 * span[0], 0.5 * span[1], 0.5 * span[2])
    surface = [("surface", 0.10, np.inf)]
    res = dict(scene=name, particles=N, reps=reps, record_bytes=RECORD_BYTES)
    m, med, mn = timed(hip.particle_measure, reps)
    res.update(measure_ms_median=med, measure_ms_min=mn, measure_bytes=4 * N)
    n_sel, C = hip.label_components(np.inf, (1, 2, 3))
    _, rc, _ = hip.components()
    cases = (("box", dict(region=region, types=(1,))), ("surface", dict(types=(1,), terms=surface)),
             ("component", dict(types=(1, 2, 3), component=int(np.argmax(rc[:, 1])))))
    for key, kw in cases:
        n, med, mn = timed(lambda: hip.select(**kw), reps)
        (idx, ids, rec), rmed, rmn = timed(hip.selection, reps)
        assert idx.size == n and (np.diff(idx) > 0).all()
        if key == "surface":
            assert (rec[:, 10] >= np.float32(0.10)).all()
        if key == "component":
            assert n == rc[kw["component"], 1]
        res.update({key + "_selected": int(n), key + "_select_ms_median": med, key + "_select_ms_min": mn,
                    key + "_read_ms_median": rmed, key + "_read_ms_min": rmn, key + "_read_bytes": int(n) * RECORD_BYTES})
    res.update(components=C, measure_quantiles={str(p): float(np.quantile(m, p)) for p in (0.5, 0.9, 0.99)})
    if host:
        ex, fl, nb, n = host_route(hip, region, (1,), (), False)
        assert n == res["box_selected"]
        res.update(host_box_export_ms=ex, host_box_filter_ms=fl, host_box_bytes=nb)
        if host_rows:
            ex, fl, nb, n = host_route(hip, None, (1,), surface, True)
            assert n == res["surface_selected"]
            res.update(host_surface_export_ms=ex, host_surface_filter_ms=fl, host_surface_bytes=nb)
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 5
    for name in (["config2", "config4"] if which == "both" else [which]):
        host = "--no-host" not in sys.argv
        print(json.dumps(run(name, reps, host=host, host_rows=name == "config2" or "--host-all" in sys.argv)), flush=True)
