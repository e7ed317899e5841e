"""Time sph_render_particles and sph_read_render on config #4 (16.5 M particles, after 10 steps) or on the worm
scene: 1280 x 720, the liquid only, one perspective view from outside and one with the eye inside the liquid, thickness off and
on. Prints, per scene, the median and minimum wall time of `reps` blocking calls after a warm-up, the counts, the bytes the images
return to the host and, as the yardstick, the blocking sph_read_position on the same state in the same process: what a picture
costs today before anything is drawn. With --fragments the numpy restatement (tests/render_ref.py) counts the fragments of each
view on the exported state (seconds on the worm, minutes and gigabytes on config4), which gives fragments issued per second.
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_render.py ...` (no counters in that run)
and read the k_render_* kernels; the renders come in the order outside, outside + thickness, inside, inside + thickness, each
reps + 1 times.

    python tools/time_render.py [config4|worm|both] [reps] [--fragments]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import diag_ref  # noqa: E402
import render_ref as rr  # noqa: E402
import scenes  # noqa: E402
from sphmi import frames  # noqa: E402

SIZE = (1280, 720)


def timed(fn, reps):
    fn()  # warm-up (allocates the images)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t)), float(np.min(t))


def liquid_bbox(hip):
    """Bounding box of the liquid from one region record (no export)."""
    r = hip.diagnostics(None, (1,))[0]
    return np.array(r[23:26]), np.array(r[26:29])


def run(name, reps, fragments=False):
    if name == "worm":
        sc, steps = scenes.worm_scene(), 10
    else:
        sc, steps = scenes.liquid_box((78.0, 50.0, 470.0), (160, 100, 1000), mask=0xffffffff), 10
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(steps):
        hip.step(it)
    hip.synchronize()
    lo, hi = liquid_bbox(hip)
    centre, ext = 0.5 * (lo + hi), hi - lo
    a = int(np.argmax(ext))
    e = np.eye(3)
    radius = 0.5 * float(cfg.r0)
    views = {
        "outside": frames.render_view(lo, hi, SIZE[0], SIZE[1], eye=centre + 0.9 * np.linalg.norm(ext) * (0.55 * e[a] + 0.6 * e[(a + 1) % 3] + 0.6 * e[(a + 2) % 3]),
                                      up=e[(a + 1) % 3], radius=radius, colour="density"),
        "inside": frames.render_view(lo, hi, SIZE[0], SIZE[1], eye=centre - 0.38 * ext[a] * e[a], target=centre + 0.1 * ext[(a + 1) % 3] * e[(a + 1) % 3],
                                     up=e[(a + 2) % 3], scale=0.5 * SIZE[0], radius=radius, near=radius, max_radius_px=4096.0, colour="density"),
    }
    res = dict(scene=name, particles=int(cfg.particleCount), steps=steps, reps=reps, size=list(SIZE))
    pos = np.empty((hip.N, 4), np.float32)
    _, med, mn = timed(lambda: hip.read_position_buffer(pos), reps)
    res.update(read_position_ms_median=med, read_position_ms_min=mn, read_position_bytes=int(pos.nbytes))
    state = diag_ref.state_with_ids(hip) if fragments else None
    pixels = SIZE[0] * SIZE[1]
    for key, view in views.items():
        for thick in (False, True):
            tag = key + ("_thickness" if thick else "")
            (drawn, covered), med, mn = timed(lambda: hip.render(view, None, (1,), thick), reps)
            img, rmed, rmn = timed(lambda: hip.rendered(thickness=thick), reps)
            res.update({tag + "_drawn": drawn, tag + "_covered": covered, tag + "_render_ms_median": med, tag + "_render_ms_min": mn,
                        tag + "_read_ms_median": rmed, tag + "_read_ms_min": rmn, tag + "_read_bytes": int(sum(v.nbytes for v in img.values())),
                        tag + "_rgba_only_bytes": 4 * pixels})
            assert int((img["index"] >= 0).sum()) == covered
        if fragments:
            t0 = time.perf_counter()
            want = rr.render(state, view, None, (1,), True, float(cfg.rho0))
            res.update({key + "_fragments": want["fragments"], key + "_largest_box": want["max_box"], key + "_restatement_s": time.perf_counter() - t0})
            for k in ("depth", "index", "orig_id", "rgba", "thickness"):
                assert np.array_equal(img[k].view(np.uint8), want[k].view(np.uint8)), (key, k)
            for tag in (key, key + "_thickness"):
                res[tag + "_fragments_per_s"] = want["fragments"] / (res[tag + "_render_ms_median"] * 1e-3)
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 30
    for name in (["worm", "config4"] if which == "both" else [which]):
        print(json.dumps(run(name, reps, fragments="--fragments" in sys.argv)), flush=True)
