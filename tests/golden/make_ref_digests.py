"""Generates tests/golden/ref_live_digests.json: for the scenes of test_oracle_live_against_reference_kernels, the digest of every
buffer after every stage of three steps, run by the reference's own kernels (oracle/_ref/libsphref.so). The test compares the
oracle with these where the reference build is absent.

Run in the build container only (needs oracle/_ref, built by __graft_entry__.build()):   python tests/golden/make_ref_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "smoothed-particle-hydrodynamics_amd")):
    sys.path.insert(0, p)

import sphmi  # noqa: E402
import test_oracle as t  # noqa: E402


def main():
    if not t._ref_available():
        sys.exit("oracle/_ref/libsphref.so not built: fixtures can only be regenerated in the build container")
    out = {}
    for name in t.LIVE_SCENES:
        sc, stages = t.live_scene(name)
        S = t.ref_solver(sc)
        rows = []
        for it in range(3):
            for st in stages:
                S.run(st, it)
                rows.append({"stage": st, "digests": {b: t.buffer_digest(S.buffer(b)) for b in t.LIVE_BUFFERS}})
            if sc["elastic"] is not None:
                S.update_muscles(sphmi.muscle_signal(it))
        out[name] = rows
    with open(t.LIVE_DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
