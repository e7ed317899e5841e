"""Time one pose of a kinematic body on the 1M cube of config #2: the wall at x = xmax as body 0, moved by
sph_body_set_pose, beside the only route there is without the body calls: sph_read_position + sph_read_velocity, the same
float32 expressions in numpy on the wall's rows, sph_destroy and sph_create. Prints one JSON line with the wall times of the
blocking calls, the member count and the algorithmic bytes of a pose.

The first repetition is a warm-up and is not counted. Every timed pose follows a burst of 20 untimed sph_body_count calls and one
untimed pose, so that it runs on a busy GPU whatever the host did before. The method and its caveats are those of
tools/time_edit.py: wall clock from Python, few repetitions.

    python tools/time_body.py [reps] [--no-host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import body_ref as br  # noqa: E402
import scenes  # noqa: E402
import sphmi  # noqa: E402
from sphmi import frames  # noqa: E402

BOX, LATTICE = (50.0, 50.0, 50.0), (100, 100, 100)  # config #2


def stats(t):
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def run(reps, host=True):
    sc = scenes.liquid_box(BOX, LATTICE)
    cfg = sc["cfg"]
    N = int(cfg.particleCount)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    r0 = np.float32(cfg.r0)
    wall = (np.float32(cfg.xmax) - r0, -np.inf, -np.inf, np.inf, np.inf, np.inf)
    members = hip.body_define_region(0, wall)
    poses = [frames.pose_translate((-0.01 * float(r0) * k, 0.0, 0.0)) for k in range(1, reps + 3)]
    t = []
    for r in range(reps + 1):
        for _ in range(20):
            hip.body_count(0)
        hip.body_set_pose(0, frames.pose_identity())
        t0 = time.perf_counter()
        hip.body_set_pose(0, poses[r])
        hip.synchronize()  # (the commit pass is enqueued, not waited for)
        t1 = time.perf_counter()
        if r:
            t.append((t1 - t0) * 1e3)
    res = dict(scene="config2", particles=N, members=members, reps=reps,
               pose=dict(bytes=(32 + 4 + 16 + 4 + 16 + 32) * members, **stats(t)))
    if host:
        ids, ref_pos, ref_nrm = hip.body_read(0)
        th = []
        for r in range(reps):
            t0 = time.perf_counter()
            p, v = hip.read_position_buffer(), hip.read_velocity_buffer()
            p, v, _ = br.set_pose(cfg, p, v, (ids, ref_pos, ref_nrm), poses[r])
            t1 = time.perf_counter()
            hip.close()
            t2 = time.perf_counter()
            hip = sphmi.owHIPSolver(cfg, p, v)
            hip.synchronize()
            t3 = time.perf_counter()
            th.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        th = np.array(th)
        res["pose_host"] = dict(read_and_move_ms_median=float(np.median(th[:, 1])), destroy_ms_median=float(np.median(th[:, 2])),
                                create_ms_median=float(np.median(th[:, 3])), pcie_bytes=64 * N, **stats(th[:, 0]))
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    print(json.dumps(run(int(args[0]) if args else 5, host="--no-host" not in sys.argv)), flush=True)
