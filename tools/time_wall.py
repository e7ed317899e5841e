"""Time sph_wall_measure and sph_wall_diagnostics on the 1 M cube of config #2 with the wall at x = xmax as body
0 (the wall of tools/time_body.py), set 4 r0 inwards and then pushed 0.05 r0 per step so that the contact branch has work,
beside -- with --host -- the only route there is without the calls: the exports (sortedPosition, sortedVelocity, rho, pressure,
particleIndex, position, both halves of acceleration, the neighbour rows) plus the numpy restatement of tests/wall_ref.py. Prints one JSON line:
the wall times of the blocking calls, the bytes each copies to the host, the particles with a slot of the body and in contact,
and the algorithmic bytes the full-record pass streams (216 B per particle: 88 read -- position, velocity, both accelerations,
the boundary mask, rho, (rho*, p) -- and 128 written; the rows and gathers of the particles next to a wall are not counted).
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_wall.py` and read k_wall_records,
k_terms_leaf<32, 27, 9>, k_terms_final<32, 27>, k_wall_mask and k_tree_upper (one row for every tree of the run: the wall totals',
and those of this tool's force_diagnostics_1 calls) in the stats. The method and its caveats are those of
tools/time_forces.py: wall clock from Python, the first call a warm-up.

    python tools/time_wall.py [reps] [--host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import forces_ref as fr  # noqa: E402
import scenes  # noqa: E402
import sphmi  # noqa: E402
import wall_ref as wr  # noqa: E402
from sphmi import frames  # noqa: E402

BOX, LATTICE = (50.0, 50.0, 50.0), (100, 100, 100)  # config #2
STREAM_BYTES_PER_PARTICLE = 16 + 16 + 16 + 16 + 4 + 4 + 8 + 8 + 128
STEPS = 8


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def host_route(hip, members):
    """The same records without the library calls: (export ms, numpy ms, bytes exported)."""
    t0 = time.perf_counter()
    state = wr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    t1 = time.perf_counter()
    wr.Wall(state, ids, dist, fr.constants(hip.cfg), wr.constants(hip.cfg), wr.wall_set(state, 0, {0: members}))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(hip.N * (32 + 16 + 8 + 4 + 8 + 16 + 32 + 256))


def run(reps, host):
    sc = scenes.liquid_box(BOX, LATTICE)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    r0 = np.float32(cfg.r0)
    members = hip.body_define_region(0, (np.float32(cfg.xmax) - r0, -np.inf, -np.inf, np.inf, np.inf, np.inf))
    t_step = 0.0
    for it in range(STEPS):
        hip.body_set_pose(0, frames.pose_translate((-(4.0 + 0.05 * it) * float(r0), 0.0, 0.0)))  # (the lattice ends 4.4 r0 from the wall)
        hip.synchronize()
        t0 = time.perf_counter()
        hip.step(it)
        hip.synchronize()
        if it >= 3:
            t_step += time.perf_counter() - t0
    N = hip.N
    out = dict(scene="config2", particles=N, members=members, step_ms=t_step * 1e3 / (STEPS - 3), stream_bytes=N * STREAM_BYTES_PER_PARTICLE)
    everything = [(-np.inf,) * 3 + (np.inf,) * 3]
    sixteen = everything + [(-np.inf, float(cfg.ymax) * k / 15, -np.inf, np.inf, float(cfg.ymax) * (k + 1) / 15, np.inf) for k in range(15)]
    n_sel = hip.select(region=(np.float32(cfg.xmax) - np.float32(6) * r0, -np.inf, -np.inf, np.inf, np.inf, np.inf), types=(1,))
    buf = {}

    def full(slot):  # into one array: the call, not numpy's allocation of 128 B per particle
        if "a" not in buf:
            buf["a"] = np.empty((N, sphmi.WALL_WORDS), np.float32)
        hip._chk(hip._L.sph_wall_measure(hip._h, slot, 0, buf["a"].ctypes.data))
        return buf["a"]

    calls = {
        "wall_measure_body": (lambda: full(0), N * 128),
        "wall_measure_all": (lambda: full(sphmi.WALL_ALL), N * 128),
        "wall_measure_selection": (lambda: hip.wall_measure(0, selection=True), n_sel * 128),
        "wall_diagnostics_1": (lambda: hip.wall_diagnostics(0, everything, (1,)), 256),
        "wall_diagnostics_16": (lambda: hip.wall_diagnostics(0, sixteen, (1,)), 16 * 256),
        "wall_diagnostics_no_body_1": (lambda: hip.wall_diagnostics(sphmi.WALL_NO_BODY, everything, (1,)), 256),
        "force_diagnostics_1": (lambda: hip.force_diagnostics(everything, (1,)), 512),  # the existing totals over the same particles
    }
    for key, (fn, nbytes) in calls.items():
        res, med, mn = timed(fn, reps)
        out[key] = dict(median_ms=med, min_ms=mn, bytes=nbytes)
        if key == "wall_measure_body":
            out["with_a_slot_of_the_body"] = int((res[:, 9] > 0).sum())
            out["in_contact"] = int(res[:, 26].sum())
            out["reflected"] = int(res[:, 27].sum())
    out["selected"] = n_sel
    s = frames.wall_summary(hip.wall_diagnostics(0, everything, (1,))[0], cfg.mass, cfg.timeStep)
    out["body_load_N"] = [float(x) for x in s["body_load"]]
    if host:
        e, c, b = host_route(hip, hip.body_read(0)[0])
        out["host_route"] = dict(export_ms=e, numpy_ms=c, bytes=b)
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    run(int(args[0]) if args else 10, host="--host" in sys.argv)
