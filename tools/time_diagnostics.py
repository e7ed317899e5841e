"""Time sph_diagnostics (k_diag_leaf and the upper tree levels) for 1 and 16 regions and sph_histogram (density,
neighbour count), on the 1M cube of config #2 or on config #4 (16.5 M particles), beside what the same answer costs without
them: read_position_buffer + read_velocity_buffer + read_density_buffer and the numpy reductions on the host. Prints, per scene,
the wall times of the blocking calls. The kernel times alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/time_diagnostics.py ...` and read k_diag_leaf, k_tree_upper (the upper levels of every tree share
this kernel; this tool runs no other tree) and k_histogram in the stats (the calls come in the order 1 region, 16 z-slab regions, 16 whole-scene regions, density, neighbours, each
reps + 1 times).

    python tools/time_diagnostics.py [1M|16M|both] [reps] [--no-host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402

WORK = {"1M": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "16M": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}
BYTES_PER_PARTICLE = 48  # sortedPos 16 + sortedVel 16 + rho 4 + rp 8 + keys 4


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def host_answer(hip):
    """The whole-scene numbers from read-back arrays, as a caller without sph_diagnostics gets them."""
    pos = hip.read_position_buffer()
    vel = hip.read_velocity_buffer()
    rho = hip.read_density_buffer()
    t = pos[:, 3].astype(np.int32)
    sel = (t == 1) | (t == 2)
    p, v = pos[sel, :3].astype(np.float64), vel[sel, :3].astype(np.float64)
    v2 = (v * v).sum(1)
    return dict(n=int(sel.sum()), sum_x=p.sum(0).tolist(), sum_v=v.sum(0).tolist(), sum_l=np.cross(p, v).sum(0).tolist(),
                sum_v2=float(v2.sum()), max_v2=float(v2.max()), rho_mean=float(rho.astype(np.float64).mean()),
                rho_min=float(rho.min()), rho_max=float(rho.max()), bbox=(p.min(0).tolist(), p.max(0).tolist()))


def run(name, reps, host=True):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    N = int(cfg.particleCount)
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float64)
    ext = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float64) - lo
    regions = [(-np.inf,) * 3 + (np.inf,) * 3]
    for k in range(15):  # slabs along z, a sixteenth of the box each
        r = [-np.inf, -np.inf, lo[2] + ext[2] * k / 16, np.inf, np.inf, lo[2] + ext[2] * (k + 1) / 16]
        regions.append(tuple(r))
    regions = np.array(regions, np.float32)
    rec1, d1_med, d1_min = timed(lambda: hip.diagnostics(regions[:1], (1, 2)), reps)
    rec16, d16_med, d16_min = timed(lambda: hip.diagnostics(regions, (1, 2)), reps)
    assert np.array_equal(rec1[0].view(np.uint64), rec16[0].view(np.uint64))
    # the worst case for 16 regions: every particle in every region (z-slabs are the best: a chunk of the sorted order meets few)
    recw, dw_med, dw_min = timed(lambda: hip.diagnostics(np.repeat(regions[:1], 16, 0), (1, 2)), reps)
    assert np.array_equal(recw[15].view(np.uint64), rec1[0].view(np.uint64))
    hd, hd_med, hd_min = timed(lambda: hip.histogram("density", 900.0, 1100.0, 256, None, (1, 2)), reps)
    hn, hn_med, hn_min = timed(lambda: hip.histogram("neighbors", 0.0, 33.0, 33, None, (1, 2, 3)), reps)
    res = dict(scene=name, particles=N, reps=reps, selected=int(rec1[0, 0]), bytes_read=BYTES_PER_PARTICLE * N,
               diagnostics_1_region_ms_median=d1_med, diagnostics_1_region_ms_min=d1_min,
               diagnostics_16_regions_ms_median=d16_med, diagnostics_16_regions_ms_min=d16_min,
               diagnostics_16_full_regions_ms_median=dw_med, diagnostics_16_full_regions_ms_min=dw_min,
               histogram_density_ms_median=hd_med, histogram_density_ms_min=hd_min,
               histogram_neighbors_ms_median=hn_med, histogram_neighbors_ms_min=hn_min,
               at_neighbor_cap=int(hn[33]), kinetic_energy=0.5 * float(cfg.mass) * float(rec1[0, 10]),
               rho_min=float(rec1[0, 16]), rho_max=float(rec1[0, 17]))
    if host:
        t0 = time.perf_counter()
        pos, vel, rho = hip.read_position_buffer(), hip.read_velocity_buffer(), hip.read_density_buffer()
        t1 = time.perf_counter()
        del pos, vel, rho
        ans, h_med, h_min = timed(lambda: host_answer(hip), max(1, min(reps, 3)))
        res.update(host_readback_ms=(t1 - t0) * 1e3, host_readback_and_numpy_ms_median=h_med, host_readback_and_numpy_ms_min=h_min,
                   host_n=ans["n"])
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 5
    for name in (["1M", "16M"] if which == "both" else [which]):
        print(json.dumps(run(name, reps, host="--no-host" not in sys.argv)), flush=True)
