"""Time particle editing on the 1M cube of config #2 or on config #4 (16.5 M particles): remove_region with 10 %
and with 50 % of the particles removed, and emit_lattice of the same number of particles, beside the only route there is without
the editing calls: sph_read_position + sph_read_velocity, a numpy filter (or a numpy lattice and a concatenate), sph_destroy and
sph_create. Prints, per scene, one JSON line with the wall times of the blocking calls and the algorithmic bytes of each edit.

Every timed edit is undone outside the timed region (the removed particles are appended again / the emitted ones removed by id
range), so each repetition sees the same count. The first repetition is a warm-up (it allocates the scan scratch) and is not
counted. Every timed call follows a burst of 20 untimed count-only calls, so that it runs on a busy GPU whatever the host did before.
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_edit.py ... --no-host` and read
the k_edit_* / k_select_scan kernels in the trace.

    python tools/time_edit.py [config2|config4|both] [reps] [--no-host]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import edit_ref as er  # noqa: E402
import scenes  # noqa: E402
import sphmi  # noqa: E402

WORK = {"config2": ((50.0, 50.0, 50.0), (100, 100, 100), 0xffff), "config4": ((78.0, 50.0, 470.0), (160, 100, 1000), 0xffffffff)}


WARM_CALLS = 20  # untimed count_only calls right before every timed removal or count


def stats(t):
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def z_box_for_fraction(pos, fraction):
    """A box over all x and y and the lowest z up to the quantile that holds `fraction` of ALL particles (both types)."""
    z1 = np.float32(np.quantile(pos[:, 2].astype(np.float64), fraction))
    return (-np.inf, -np.inf, -np.inf, np.inf, np.inf, z1)


def run(name, reps, host=True):
    box, lat, mask = WORK[name]
    sc = scenes.liquid_box(box, lat, mask=mask)
    cfg0 = sc["cfg"]
    N = int(cfg0.particleCount)
    cfg = er.with_count(cfg0, N, N + N // 2 + 1)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    for it in range(2):
        hip.step(it)
    hip.synchronize()
    pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
    res = dict(scene=name, particles=N, reps=reps)
    for label, fraction in (("remove10", 0.10), ("remove50", 0.50)):
        region = z_box_for_fraction(pos, fraction)
        marked = er.region_marks(pos, region, (1, 3))
        t, tc = [], []
        for r in range(reps + 1):
            # the undo below keeps the host busy for a long time and the GPU idle: a burst of untimed calls brings the clocks back
            # up before EACH timed call, so that the two are timed alike
            for _ in range(WARM_CALLS):
                hip.remove_region(region, (1, 3), count_only=True)
            t0 = time.perf_counter()
            c = hip.remove_region(region, (1, 3), count_only=True)
            t1 = time.perf_counter()
            for _ in range(WARM_CALLS):
                hip.remove_region(region, (1, 3), count_only=True)
            t1b = time.perf_counter()
            n = hip.remove_region(region, (1, 3))
            t2 = time.perf_counter()
            assert n == c == marked.sum() and hip.N == N - n
            hip.add_particles(pos[marked], vel[marked])  # undo (the order differs; the next removal marks by position)
            if r:
                tc.append((t1 - t0) * 1e3)
                t.append((t2 - t1b) * 1e3)
            if r == 0:
                pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
                marked = er.region_marks(pos, region, (1, 3))
        removed = int(marked.sum())
        # algorithmic bytes: posOrig read by the mark pass; both streams read, the survivors' written, the 4-byte map written
        res[label] = dict(removed=removed, fraction=removed / N, bytes=16 * N + 32 * N + 32 * (N - removed) + 4 * N, **stats(t))
        res[label + "_count_only"] = dict(bytes=16 * N, **stats(tc))
        if host:
            th = []
            for r in range(reps):
                t0 = time.perf_counter()
                p, v = hip.read_position_buffer(), hip.read_velocity_buffer()
                keep = ~er.region_marks(p, region, (1, 3))
                p, v = p[keep], v[keep]
                t1 = time.perf_counter()
                hip.close()
                t2 = time.perf_counter()
                hip = sphmi.owHIPSolver(er.with_count(cfg0, p.shape[0], N + N // 2 + 1), p, v)
                hip.synchronize()
                t3 = time.perf_counter()
                th.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
                hip.add_particles(pos[marked], vel[marked])
            th = np.array(th)
            res[label + "_host"] = dict(read_and_filter_ms_median=float(np.median(th[:, 1])), destroy_ms_median=float(np.median(th[:, 2])),
                                        create_ms_median=float(np.median(th[:, 3])), pcie_bytes=32 * N + 32 * (N - removed), **stats(th[:, 0]))
            pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
    # emit: a lattice of N / 10 particles above everything else would leave the box; what is timed is the emitter alone, so
    # the lattice is placed inside the box over the existing particles and removed again by id range before any step
    k = int(round((N / 10) ** (1.0 / 3.0)))
    dims = (k, k, k)
    r0 = np.float32(cfg0.r0)
    origin, spacing = (3 * r0, 3 * r0, 3 * r0), (np.float32(0.5) * r0,) * 3
    t = []
    for r in range(reps + 1):
        for _ in range(WARM_CALLS):
            hip.remove_region(None, (1, 3), count_only=True)
        t0 = time.perf_counter()
        added = hip.emit_lattice(origin, spacing, dims)
        t1 = time.perf_counter()
        assert added == k ** 3 and hip.N == N + added
        hip.remove_ids(np.arange(N, N + added))
        if r:
            t.append((t1 - t0) * 1e3)
    res["emit"] = dict(added=k ** 3, bytes=32 * k ** 3, **stats(t))
    if host:
        th = []
        for r in range(reps):
            t0 = time.perf_counter()
            p, v = hip.read_position_buffer(), hip.read_velocity_buffer()
            lp, lv = er.lattice(origin, spacing, dims)
            p, v = np.concatenate([p, lp]), np.concatenate([v, lv])
            hip.close()
            hip = sphmi.owHIPSolver(er.with_count(cfg0, p.shape[0], N + N // 2 + 1), p, v)
            hip.synchronize()
            th.append((time.perf_counter() - t0) * 1e3)
            hip.remove_ids(np.arange(N, N + k ** 3))
        res["emit_host"] = dict(pcie_bytes=32 * N + 32 * (N + k ** 3), **stats(th))
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 5
    for name in (["config2", "config4"] if which == "both" else [which]):
        print(json.dumps(run(name, reps, host="--no-host" not in sys.argv)), flush=True)
