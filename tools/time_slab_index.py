"""Time the cell-table stage (SORT_POST: k_cell_start alone in slab mode) of a rank-0 slab solver on the grid of BASELINE config #4
(78 x 50 x 470 h, wide cell ids): tools/time_slab_index.py [steps per window] [windows]. A/B builds via SPHMI_LIB.

The liquid fills the lowest 30 layers only (2.1 M particles + the box's boundary shell below layer 36), so the scene is quick to
make; the stage's cost is one binary search per computed table entry, whatever the particle count. Rank 0 of 2, cut at layer 32:
it computes the entries of layers [0, 39) and, from DESIGN 28 on, the one layer at the far end of the table that a wrapped cell
can land in. Prints one JSON line: microseconds per step of the stage (device events around it), per window."""
import json
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import scenes
from sphmi import slab as S

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sc = scenes.liquid_box((78.0, 50.0, 470.0), (160, 100, 130), mask=0xffffffff)
cfg = sc["cfg"]
lay = S.particle_layers(sc["position"], cfg)
slab = S.make_slab([int(lay.min()), 32, int(lay.max()) + 1], 0, 2, cfg.particleCount)
idx = S.local_indices(lay, slab)
be = S.HipSlabBackend(cfg, sc["position"][idx], sc["velocity"][idx], idx, slab)
h = be.solver
for it in range(10):
    be.step(it)
h.synchronize()
h.set_stage_timing(True)
out = []
for w in range(windows):
    h.reset_stage_times()
    for it in range(steps):
        be.step(it)
    h.synchronize()
    t = h.stage_times()
    out.append(round(1e3 * t["sort_post"][0] / t["sort_post"][1], 3))
    step_ms = sum(v[0] for v in t.values()) / steps
print(json.dumps({"lib": os.path.basename(os.environ.get("SPHMI_LIB", "libsphmi.so")), "grid_cells": cfg.gridCellCount,
                  "layer_cells": cfg.gridCellsX * cfg.gridCellsY, "local_particles": int(idx.size), "steps_per_window": steps,
                  "sort_post_us_per_step": out, "median_us": float(np.median(out)), "all_stages_ms_per_step_last_window": round(step_ms, 3)}))
