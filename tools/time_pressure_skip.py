"""Time the fused step on the states that bound the per-wave skipping of the predict-correct loop and report the share
of waves that skipped, from the decision bytes of the last launches. One JSON line per scene. SPHMI_LIB selects the library, as for
bench.py; a library without the decision bytes reports null shares.

  box085      the config #4 box with the lattice at 0.85 r0: steps 1 .. K of a fresh solver (pressure-active from the first step, the
              worst case: nearly every wave consults the flags and then takes the full path). Repeated --repeats times, each on a
              solver of its own; the first repeat also loads the code objects and is reported apart.
  box093      the same at 0.93 r0 (the headline scene: pressure-free for ~70 steps, the best case)
  config2     bench.py's config2_1M_cube block: 5 + K steps
  worm        bench.py's config3_worm block (muscles on): 5 + K steps
  dam_break   bench.py's evolved_dam_break block: --evolve steps, then K

--wave-skip MODE sets the solver's policy (sph_set_wave_skip: 0 the built-in one, 1 always mark and consult, 2 the flags off)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import scenes  # noqa: E402
import sphmi  # noqa: E402


def shares(hip):
    out = {}
    for key, name in (("k12_skipped", "pressureForceSkipped"), ("k10_skipped", "predictDensitySkipped")):
        try:
            out[key] = round(float((hip.buffer(name) != 0).mean()), 4)
        except sphmi.SphError:
            out[key] = None
    return out


def timed(hip, first, k, after_step=None):
    hip.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + k):
        hip.step(i)
        if after_step:
            after_step(i)
    hip.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", choices=["box085", "box093", "config2", "worm", "dam_break"])
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--evolve", type=int, default=1500)
    ap.add_argument("--wave-skip", type=int, default=None, choices=[0, 1, 2])
    a = ap.parse_args()
    out = {"scene": a.scene, "lib": os.path.basename(sphmi.LIB_PATH), "wave_skip": a.wave_skip}

    def policy(hip):
        if a.wave_skip is not None:
            hip.set_wave_skip(a.wave_skip)
        return hip
    if a.scene in ("box085", "box093"):
        box, lattice, mask = bench.WORKLOADS["config4_16M_box"]
        sc = scenes.liquid_box(box, lattice, spacing_in_r0=0.85 if a.scene == "box085" else 0.93, mask=mask)
        k = a.steps or 10
        ms = []
        for _ in range(a.repeats):
            hip = policy(scenes.hip_for(sc))
            ms.append(round(timed(hip, 0, k), 4))
            out.update(shares(hip))
            out["pressure_max"] = float(hip.buffer("pressure").max())
            hip.close()
        out.update(particles=sc["cfg"].particleCount, steps="1..%d" % k, ms_per_step_first_solver=ms[0], ms_per_step=ms[1:])
    elif a.scene == "config2":
        box, lattice, mask = bench.WORKLOADS["config2_1M_cube"]
        sc = scenes.liquid_box(box, lattice, mask=mask)
        hip = policy(scenes.hip_for(sc))
        k = a.steps or 50
        timed(hip, 0, 5)
        out.update(particles=sc["cfg"].particleCount, steps=k, ms_per_step=[round(timed(hip, 5 + r * k, k), 4) for r in range(a.repeats)], **shares(hip))
        hip.close()
    elif a.scene == "worm":
        cfg = sphmi.default_config()
        w = sphmi.generate_worm(cfg)
        hip = policy(sphmi.owHIPSolver(cfg, w["position"], w["velocity"], w["elastic"], w["membranes"], w["particle_membranes"]))
        k = a.steps or 50
        signal = lambda i: hip.updateMuscleActivityData(sphmi.muscle_signal(i, cfg.muscleCount))  # noqa: E731
        timed(hip, 0, 5, signal)
        out.update(particles=cfg.particleCount, steps=k, ms_per_step=[round(timed(hip, 5 + r * k, k, signal), 4) for r in range(a.repeats)], **shares(hip))
        hip.close()
    else:
        box, lattice, mask = bench.DAM_BREAK
        sc = scenes.liquid_box(box, lattice, mask=mask)
        hip = policy(scenes.hip_for(sc))
        k = a.steps or 50
        rest = timed(hip, 0, k)
        at_rest = shares(hip)
        for i in range(k, a.evolve):
            hip.step(i)
        out.update(particles=sc["cfg"].particleCount, steps=k, evolved_steps=a.evolve, ms_per_step_at_rest=round(rest, 4), at_rest=at_rest,
                   ms_per_step=[round(timed(hip, a.evolve + r * k, k), 4) for r in range(a.repeats)], **shares(hip))
        hip.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
