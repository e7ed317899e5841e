"""Time sph_label_components (k_cc_hook, k_cc_flatten, the numbering and the table) with +inf and with a finite
link radius (h / 2), sph_read_components and sph_component_diagnostics, on the 1M cube of config #2 or on config #4 (16.5 M
particles), beside what the same answer costs without them: the neighbour rows and the sorted positions read back through
sph_read_neighbor_rows / sph_read_buffer and a union-find on the host (here: numpy hooking and pointer jumping over the row
graph). Prints, per scene, the wall times of the blocking calls. The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_components.py ...` and read the k_cc_* kernels in the trace (the
labellings come in the order +inf over liquid + elastic, +inf over all types, h / 2 over liquid + elastic, each reps + 1 times;
k_cc_hook<false> is the +inf form).

The host-side alternative runs on config2 only (on config4 the 528 M row entries alone are 4 GB of read-back) unless --host-all.

    python tools/time_components.py [config2|config4|both] [reps] [--no-host] [--host-all]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402

WORK = {"config2": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "config4": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}
ROW_BYTES = 64 + 4 + 4  # per particle: the 16-bit id row, nbrBase, parent (+ 16 B per row entry gathered with a finite radius)


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def host_answer(hip, types=(1, 2), piece=1 << 18):
    """Components of the same graph from read-back rows, as a caller without sph_label_components gets them: (read-back ms,
    labelling ms, number of components, size of the largest)."""
    t0 = time.perf_counter()
    N = hip.N
    rows = np.empty((N, 32), np.int32)
    for first in range(0, N, piece):
        n = min(piece, N - first)
        rows[first:first + n] = hip.neighbor_rows(first, n)[0]
    pi = hip.read_particleIndex_buffer()
    ptype = hip.read_position_buffer()[pi[:, 1], 3].astype(np.int32)
    t1 = time.perf_counter()
    sel = np.isin(ptype, types) & (pi[:, 0] < hip.cfg.gridCellCount)
    i = np.repeat(np.arange(N, dtype=np.int64), 32)
    j = rows.reshape(-1).astype(np.int64)
    ok = j >= 0
    i, j = i[ok], j[ok]
    ok = sel[i] & sel[j] & (i != j)
    i, j = i[ok], j[ok]
    lab = np.where(sel, np.arange(N, dtype=np.int64), -1)
    while True:
        a, b = lab[i], lab[j]
        differ = a != b
        if not differ.any():
            break
        a, b = a[differ], b[differ]
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))
        while True:
            nxt = np.where(lab >= 0, lab[np.maximum(lab, 0)], -1)
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    roots, counts = np.unique(lab[sel], return_counts=True)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(roots.size), int(counts.max()) if counts.size else 0


def run(name, reps, host=True):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    N = int(cfg.particleCount)
    half_h = float(np.float32(cfg.h) / np.float32(2))
    (n_inf, c_inf), inf_med, inf_min = timed(lambda: hip.label_components(np.inf, (1, 2)), reps)
    (labels, rc, bbox), read_med, read_min = timed(hip.components, reps)
    top = np.lexsort((np.arange(c_inf), -rc[:, 1].astype(np.int64)))[:16]
    rec, cd_med, cd_min = timed(lambda: hip.component_diagnostics(top), reps)
    assert rec[0, 0] == rc[top[0], 1]
    (n_all, c_all), all_med, all_min = timed(lambda: hip.label_components(np.inf, (1, 2, 3)), reps)
    (n_fin, c_fin), fin_med, fin_min = timed(lambda: hip.label_components(half_h, (1, 2)), reps)
    res = dict(scene=name, particles=N, reps=reps, selected=n_inf, row_bytes=ROW_BYTES * N,
               components_inf=c_inf, largest_inf=int(rc[:, 1].max()), components_inf_all_types=c_all,
               components_half_h=c_fin, half_h=half_h,
               label_inf_ms_median=inf_med, label_inf_ms_min=inf_min,
               label_inf_all_types_ms_median=all_med, label_inf_all_types_ms_min=all_min,
               label_half_h_ms_median=fin_med, label_half_h_ms_min=fin_min,
               read_components_ms_median=read_med, read_components_ms_min=read_min,
               component_diagnostics_ms_median=cd_med, component_diagnostics_ms_min=cd_min, component_diagnostics_ids=int(top.size))
    if host:
        rb, lab_ms, c_host, largest_host = host_answer(hip)
        assert c_host == c_inf and largest_host == res["largest_inf"]
        res.update(host_readback_ms=rb, host_labelling_ms=lab_ms, host_components=c_host)
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 5
    for name in (["config2", "config4"] if which == "both" else [which]):
        host = "--no-host" not in sys.argv and (name == "config2" or "--host-all" in sys.argv)
        print(json.dumps(run(name, reps, host=host)), flush=True)
