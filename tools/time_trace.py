"""Time the integral curves (sph_trace_streamlines / sph_tracers_advect) on the 1M cube of config #2 after enough
steps that the liquid moves: 4,096 and 65,536 seeds on a plane across the box's mid-height, midpoint rule, arc mode, step h/2,
maxSteps 256. One JSON line per measurement.

    python tools/time_trace.py call [reps]     wall time of one blocking streamlines() call, the curves' census and the share of
                                               lane-steps in which a lane waits for the longest curve of its wave
    python tools/time_trace.py loop            the same curves by the only way there was before: a host loop over sample_points
                                               (2 x 257 blocking calls), its wall time, and whether the two agree bit for bit
                                               (with a checkout of the parent commit's package first on sys.path, the loop is the
                                               parent's: nothing but sample_points is called)
    python tools/time_trace.py walk [reps]     streamlines(), then sample_points on as many points as the curves took walks, drawn
                                               from the curves' own vertices: run under `rocprofv3 --kernel-trace --stats` and
                                               divide the printed sample counts by the times of k_trace_streamlines / k_sample_points
    python tools/time_trace.py tracers [reps]  65,536 tracers: wall time of tracers_advect beside one step of the scene"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
import sphmi  # noqa: E402
import trace_ref  # noqa: E402

STEPS = 50
MAX_STEPS = 256
SEEDS = (64, 256)  # per side of the plane


def solver():
    sc = scenes.liquid_box((50.0, 50.0, 50.0), (100, 100, 100))
    hip = scenes.hip_for(sc)
    for it in range(STEPS):
        hip.step(it)
    hip.synchronize()
    return sc["cfg"], hip


def plane(cfg, n):
    """n x n seeds across the box at mid-height (frames.seed_plane's points, written out so that the host loop also runs on a
    checkout that has no seed_plane yet)."""
    f = np.float32
    dx, dz = (f(cfg.xmax) - f(cfg.xmin)) / f(n), (f(cfg.zmax) - f(cfg.zmin)) / f(n)
    i = np.arange(n, dtype=np.float32)
    p = np.empty((n, n, 3), np.float32)
    p[..., 0] = (f(cfg.xmin) + f(0.5) * dx + i * dx)[None, :]
    p[..., 1] = f(0.5) * (f(cfg.ymin) + f(cfg.ymax))
    p[..., 2] = (f(cfg.zmin) + f(0.5) * dz + i * dz)[:, None]
    return p.reshape(-1, 3)


def walks_per_curve(lengths, status):
    """Point walks a midpoint curve took: one per vertex (none at a non-finite one) and one per step taken. (A step that stopped at
    its midpoint walked once more: not counted.)"""
    ln = np.asarray(lengths, np.int64)
    return np.maximum(ln - (np.asarray(status) == sphmi.TRACE_NONFINITE) + (ln - 1), 0)


def idle_lane_share(walks, wave=64):
    w = np.asarray(walks, np.int64)
    w = np.concatenate([w, np.zeros((-w.shape[0]) % wave, np.int64)]).reshape(-1, wave)
    total = int((w.max(axis=1) * wave).sum())
    return 1.0 - float(w.sum()) / total if total else 0.0


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "call"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cfg, hip = solver()
    h = np.float32(cfg.h)
    kw = dict(types=(1,), step=h / np.float32(2), mode="arc", integrator="midpoint", max_steps=MAX_STEPS)
    base = dict(mode=mode, library=os.path.basename(sphmi.LIB_PATH), particles=int(cfg.particleCount), steps_before=STEPS, max_steps=MAX_STEPS)
    for n in SEEDS:
        seeds = plane(cfg, n)
        if mode == "call" or mode == "walk":
            (v, ln, st), ts = timed(lambda: hip.streamlines(seeds, **kw), reps)
            walks = walks_per_curve(ln, st)
            rec = dict(base, seeds=int(seeds.shape[0]), wall_ms_median=float(np.median(ts)), wall_ms_min=float(np.min(ts)),
                       vertices=int(ln.sum()), walks=int(walks.sum()), mean_length=float(ln.mean()),
                       status_counts=np.bincount(st, minlength=6).tolist(), idle_lane_share=idle_lane_share(walks),
                       idle_lane_share_if_sorted_by_length=idle_lane_share(np.sort(walks)), speed_max=float(v[..., 3].max()))
            if mode == "walk":
                keep = np.arange(MAX_STEPS + 1)[None, :] < ln[:, None]
                pts = v[..., :3][keep]
                pts = pts[np.random.default_rng(1).integers(0, pts.shape[0], int(walks.sum()))]
                _, ts2 = timed(lambda: hip.sample_points(pts, (1,)), reps)
                rec.update(streamlines_calls=reps + 1, sample_points_calls=reps + 1, sample_points=int(pts.shape[0]),
                           sample_points_wall_ms_median=float(np.median(ts2)))
            print(json.dumps(rec), flush=True)
        elif mode == "loop":
            t0 = time.perf_counter()
            lv, ll, ls = trace_ref.streamlines(lambda p, ty: hip.sample_points(p, ty), seeds, (1,), kw["step"], trace_ref.ARC,
                                               trace_ref.MIDPOINT, MAX_STEPS)
            loop_ms = (time.perf_counter() - t0) * 1e3
            rec = dict(base, seeds=int(seeds.shape[0]), host_loop_wall_ms=loop_ms, vertices=int(ll.sum()))
            if hasattr(hip._L, "sph_trace_streamlines"):
                v, ln, st = hip.streamlines(seeds, **kw)
                rec["call_equals_loop_bit_for_bit"] = bool(np.array_equal(v.view(np.uint32), lv.view(np.uint32)) and np.array_equal(ln, ll)
                                                           and np.array_equal(st, ls))
            print(json.dumps(rec), flush=True)
    if mode == "tracers":
        seeds = plane(cfg, 256)
        hip.tracers_set(seeds)
        counts, ts = timed(lambda: hip.tracers_advect((1,), dt=cfg.timeStep), reps)

        def step():
            hip.step(STEPS)
            hip.synchronize()
        _, ss = timed(step, reps)
        print(json.dumps(dict(base, tracers=int(seeds.shape[0]), advect_wall_ms_median=float(np.median(ts)), advect_wall_ms_min=float(np.min(ts)),
                              moving=counts[0], stopped=counts[1], step_wall_ms_median=float(np.median(ss)))), flush=True)
    hip.close()


if __name__ == "__main__":
    main()
