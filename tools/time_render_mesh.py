"""Time sph_render_mesh on config #4 (16.5 M particles, after 10 steps) with the Shepard-0.5 surface of the liquid
on a lattice of 256 points a side, or on the worm scene with its membranes: 1280 x 720, one perspective
view from outside and one with the eye inside the matter, as a fresh image and composed over a particle render. Prints, per
scene, the median and minimum wall time of `reps` blocking calls after a warm-up, the four counts, the bytes the images return
to the host and, timed on the same state in the same process, the yardsticks: the blocking sph_read_surface + sph_surface_normals
(the read-backs the picture replaces) and sph_render_particles.
The kernel times alone: run under `rocprofv3 --kernel-trace --stats -- python tools/time_render_mesh.py ...` (no counters in that
run) and read the k_rm_* kernels; the passes come in the order outside, outside composed, inside, inside composed, each reps + 1
times.

    python tools/time_render_mesh.py [config4|worm|both] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scenes  # noqa: E402
from sphmi import frames  # noqa: E402
from time_render import SIZE, liquid_bbox, timed  # noqa: E402

LATTICE = 256


def run(name, reps):
    if name == "worm":
        sc, steps = scenes.worm_scene(), 10
    else:
        sc, steps = scenes.liquid_box((78.0, 50.0, 470.0), (160, 100, 1000), mask=0xffffffff), 10
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(steps):
        hip.step(it)
    hip.synchronize()
    res = dict(scene=name, particles=int(cfg.particleCount), steps=steps, reps=reps, size=list(SIZE))
    radius = 0.5 * float(cfg.r0)
    e = np.eye(3)
    if name == "worm":
        source, shading, types = "membranes", "flat", (2,)
        r = hip.diagnostics(None, (2,))[0]
        lo, hi = np.array(r[23:26]), np.array(r[26:29])
        res.update(triangles=int(cfg.numOfMembranes))
    else:
        source, shading, types = "surface", "smooth", (1,)
        lo, hi = liquid_bbox(hip)
        pad = float(cfg.h)
        dims = [LATTICE] * 3  # the liquid is a long box: the spacing differs per axis
        spacing = [float(hi[k] - lo[k] + 2 * pad) / (LATTICE - 1) for k in range(3)]
        t0 = time.perf_counter()
        verts, tris = hip.extract_surface(lo - pad, spacing, dims, iso=0.5, field="shepard", types=(1,))
        res.update(lattice=dims, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]), extract_and_read_ms=(time.perf_counter() - t0) * 1e3)
        del verts, tris
        V, T = res["vertices"], res["triangles"]
        vbuf, tbuf = np.empty((V, 3), np.float32), np.empty((T, 3), np.int32)
        _, med, mn = timed(lambda: hip._chk(hip._L.sph_read_surface(hip._h, vbuf.ctypes.data, tbuf.ctypes.data)), reps)
        res.update(read_surface_ms_median=med, read_surface_ms_min=mn, read_surface_bytes=int(vbuf.nbytes + tbuf.nbytes))
        nrm, med, mn = timed(hip.surface_normals, reps)
        res.update(surface_normals_ms_median=med, surface_normals_ms_min=mn, surface_normals_bytes=int(nrm.nbytes))
    centre, ext = 0.5 * (lo + hi), hi - lo
    a = int(np.argmax(ext))
    views = {
        "outside": frames.render_view(lo, hi, SIZE[0], SIZE[1], eye=centre + 0.9 * np.linalg.norm(ext) * (0.55 * e[a] + 0.6 * e[(a + 1) % 3] + 0.6 * e[(a + 2) % 3]),
                                      up=e[(a + 1) % 3], radius=radius, colour="density"),
        "inside": frames.render_view(lo, hi, SIZE[0], SIZE[1], eye=centre - 0.38 * ext[a] * e[a], target=centre + 0.1 * ext[(a + 1) % 3] * e[(a + 1) % 3],
                                     up=e[(a + 2) % 3], scale=0.5 * SIZE[0], radius=radius, near=radius, max_radius_px=4096.0, colour="density"),
    }
    pixels = SIZE[0] * SIZE[1]
    for key, view in views.items():
        (drawn, covered), med, mn = timed(lambda: hip.render(view, None, types), reps)
        res.update({key + "_particles_drawn": drawn, key + "_particles_covered": covered, key + "_render_particles_ms_median": med,
                    key + "_render_particles_ms_min": mn})
        for compose in (False, True):
            tag = key + ("_composed" if compose else "")

            def once():
                if compose:  # a composed pass changes the images it is drawn over: render them again, and take their time off below
                    hip.render(view, None, types)
                return hip.render_mesh(view, source, shading, (0.35, 0.6, 0.95), compose=compose)
            counts, med, mn = timed(once, reps)
            if compose:
                med, mn = med - res[key + "_render_particles_ms_median"], mn - res[key + "_render_particles_ms_min"]
            img, rmed, rmn = timed(lambda: hip.rendered(triangle=True), reps)
            res.update({tag + "_counts": list(counts), tag + "_render_mesh_ms_median": med, tag + "_render_mesh_ms_min": mn,
                        tag + "_read_ms_median": rmed, tag + "_read_bytes": int(sum(v.nbytes for v in img.values())), tag + "_rgba_only_bytes": 4 * pixels})
            assert int((img["triangle"] >= 0).sum()) == counts[2]
    hip.close()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "both"
    reps = int(args[1]) if len(args) > 1 else 30
    for name in (["worm", "config4"] if which == "both" else [which]):
        print(json.dumps(run(name, reps)), flush=True)
