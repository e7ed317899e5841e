"""Generates tests/golden/ref_elastic_digests.json: for the scenes of test_elastic_edges_host.EDGE_SCENES, the digests of every buffer
of the reference's own kernels (oracle/_ref/libsphref.so) at every recorded point of the scene's plan, and of the scene's inputs.
The test compares the oracle with these where the reference build is absent.

Run in the build container only (needs oracle/_ref, built by __graft_entry__.build()):   python tests/golden/make_ref_elastic_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "smoothed-particle-hydrodynamics_amd")):
    sys.path.insert(0, p)

import scenes  # noqa: E402
import test_elastic_edges_host as t  # noqa: E402


def main():
    if not t._ref_available():
        sys.exit("oracle/_ref/libsphref.so not built: fixtures can only be regenerated in the build container")
    out = {}
    for name in t.EDGE_SCENES:
        sc = scenes.elastic_hard_box(**t.EDGE_SCENES[name][0])
        S = t.ref_solver(sc, threads=8)
        rows = []
        t.edge_run(name, S.run, S.update_muscles, lambda k, label, it: rows.append(
            {"stage": label, "digests": {b: t.buffer_digest(S.buffer(b)) for b in t.LIVE_BUFFERS}}))
        out[name] = {"input": {k: scenes.sha(sc[k])[:16] for k in ("position", "elastic")}, "rows": rows}
    with open(t.EDGE_DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
