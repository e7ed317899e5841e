"""Time sph_bodies_advance on the 1 M cube of config #2 with the wall at x = xmax (the wall of tools/time_wall.py:
set 4 r0 inwards and pushed 0.05 r0 per step for 8 steps so that the contact branch has work) split along y into 1, 4 and 16
dynamic bodies, beside the host loop it replaces: per body a blocking wall_diagnostics, the integrator in numpy
(tests/body_dyn_ref.py) and a blocking body_set_pose. The bodies are fully locked with zero velocity, so every repetition places
them where they stand and the state being timed does not drift. Prints one JSON line per split: the wall times of
bodies_advance(read=False) as enqueued (the call returns without a wait) and with a synchronise behind it, of
bodies_advance(read=True), of the host loop, and of two wall_diagnostics calls for one body (the expectation the section
states: the fused pass for 16 bodies costs less than those). With a library that has no sph_bodies_advance (SPHMI_LIB=... pointing at
a build of the parent commit) only the host loop is timed. The kernel times alone: run under `rocprofv3 --kernel-trace --stats --
python tools/time_body_dynamics.py` and read k_bdyn_*. Method and caveats are those of tools/time_wall.py: wall clock from Python
around the calls, the first call a warm-up, the median of `reps` repetitions.

    python tools/time_body_dynamics.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import body_dyn_ref as bd  # noqa: E402
import scenes  # noqa: E402
from sphmi import frames  # noqa: E402

BOX, LATTICE = (50.0, 50.0, 50.0), (100, 100, 100)  # config #2
STEPS = 8
EVERYTHING = [(-np.inf,) * 3 + (np.inf,) * 3]


def timed(fn, reps):
    fn()  # warm-up (allocates the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)))


def run(split, reps):
    sc = scenes.liquid_box(BOX, LATTICE)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    r0 = np.float32(cfg.r0)
    edges = np.linspace(float(cfg.ymin) - 1.0, float(cfg.ymax) + 1.0, split + 1).astype(np.float32)
    members = [hip.body_define_region(b, (np.float32(cfg.xmax) - r0, edges[b], -np.inf, np.inf, edges[b + 1], np.inf)) for b in range(split)]
    pose = frames.pose_identity()
    t_step = 0.0
    for it in range(STEPS):
        pose = frames.pose_translate((-(4.0 + 0.05 * it) * float(r0), 0.0, 0.0))  # (the lattice ends 4.4 r0 from the wall)
        for b in range(split):
            hip.body_set_pose(b, pose)
        hip.synchronize()
        t0 = time.perf_counter()
        hip.step(it)
        hip.synchronize()
        if it >= 3:
            t_step += time.perf_counter() - t0
    states = {}
    for b in range(split):
        ref = hip.body_read(b)[1]
        mass = members[b] * float(np.float32(cfg.mass))
        com, _, jinv = frames.body_mass_properties(ref, mass)
        states[b] = bd.make_state(mass, com=com, position=com + pose[:, 3].astype(np.float64), inertiaInv=jinv, locks=15,
                                  gravity=(cfg.gravity_x, cfg.gravity_y, cfg.gravity_z))
    consts = bd.constants(cfg)

    def host_loop():
        for b in range(split):
            D = hip.wall_diagnostics(b, EVERYTHING, (1, 2, 3))[0]
            _, p, _ = bd.advance(D, states[b], *consts)
            hip.body_set_pose(b, p)

    def two_diagnostics():
        hip.wall_diagnostics(0, EVERYTHING, (1, 2, 3))
        hip.wall_diagnostics(0, EVERYTHING, (1, 2, 3))

    out = dict(scene="config2", particles=hip.N, bodies=split, members=int(sum(members)), step_ms=t_step * 1e3 / (STEPS - 3))
    out["host_loop"] = timed(host_loop, reps)
    out["two_wall_diagnostics"] = timed(two_diagnostics, reps)
    if hasattr(hip._L, "sph_bodies_advance"):
        for b in range(split):
            hip.body_set_dynamics(b, **states[b])

        def enqueue_and_wait():
            hip.bodies_advance(read=False)
            hip.synchronize()

        hip.synchronize()
        out["advance_enqueue"] = timed(lambda: hip.bodies_advance(read=False), reps)
        hip.synchronize()
        out["advance_and_synchronise"] = timed(enqueue_and_wait, reps)
        out["advance_read"] = timed(lambda: hip.bodies_advance(read=True), reps)
        rec = hip.bodies_advance()
        out["status"] = [int(x) for x in rec[:split, 0]]
        out["n_share"] = [int(x) for x in rec[:split, 27]]
        out["load_x_N"] = [float(x) for x in rec[:split, 20]]
    hip.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for split in (1, 4, 16):
        run(split, reps)
