"""One mid-run step of a rocprofv3 kernel trace (csv): python tools/trace_step.py t_kernel_trace.csv [step]. Times in us from the
step's first kernel (k_hash_compact)."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
step = int(sys.argv[2]) if len(sys.argv) > 2 else 15
ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Stream_Id"]) for r in rows))
starts = [i for i, e in enumerate(ev) if e[2].startswith("k_hash_compact")]
lo, hi = starts[step], starts[step + 1]
t0 = ev[lo][0]
short = lambda n: n.split("(")[0].replace("void ", "")
fn = [e for e in ev[lo:hi] if "k_find_neighbors" in e[2]]
print("step %d: %d launches, span to the next step's first kernel %.1f us" % (step, hi - lo, (ev[hi][0] - t0) / 1e3))
print("first kernel -> first k_find_neighbors start: %.1f us" % ((fn[0][0] - t0) / 1e3))
for i, e in enumerate(fn[:4]):
    print("  search launch %d (stream %s): %.1f .. %.1f" % (i, e[3], (e[0] - t0) / 1e3, (e[1] - t0) / 1e3))
print("  last search launch ends %.1f" % ((max(e[1] for e in fn) - t0) / 1e3))
for e in ev[lo:hi]:
    n = short(e[2])
    if n.startswith(("k_sort_post", "k_band_", "k_halo", "k_cell_start")):
        print("  %-32s stream %s: %.1f .. %.1f (%.1f)" % (n, e[3], (e[0] - t0) / 1e3, (e[1] - t0) / 1e3, (e[1] - e[0]) / 1e3))
first_forces = [e for e in ev[lo:hi] if "k_forces<" in e[2]]
pf = [e for e in ev[lo:hi] if "k_pressure_force<1>" in e[2] or "k_predict_density" in e[2]]
print("  first k_forces start %.1f; loop starts %.1f; step's last kernel ends %.1f" % (
    (first_forces[0][0] - t0) / 1e3, (min(e[0] for e in pf) - t0) / 1e3, (max(e[1] for e in ev[lo:hi]) - t0) / 1e3))
avg = {}
for e in ev[starts[5]:starts[-1]]:
    a = avg.setdefault(short(e[2]), [0, 0])
    a[0] += e[1] - e[0]
    a[1] += 1
for n in sorted(avg):
    if n.startswith(("k_find", "k_sort_post", "k_band_sc", "k_forces<", "k_density", "k_pack")):
        print("  avg %-34s %8.1f us x %d" % (n, avg[n][0] / avg[n][1] / 1e3, avg[n][1]))
