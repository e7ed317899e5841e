"""The scene and the line cases of the GPU probe tests (tests/test_probe.py). What each case claims is asserted on the numpy
restatement (tests/probe_ref.py) by tests/test_probe_host.py over the oracle's state, which the solver's equals bit for bit; without
that the GPU comparison could pass on lines that never meet a surface.

The scene is scenes.liquid_box((8, 8, 8) h, lattice (10, 8, 10), jitter) after STEPS steps: a jittered block of liquid inside the
boundary shell, gravity along -y, the smallest state in which the sums are generic. Lengths below are in r0 = h / 2; the liquid
spans about 3 .. 11.4 r0 in x and z and 3 .. 9.5 r0 in y (its Shepard level 0.5 lies near 10.1 r0), the box 0 .. 16 r0."""
import numpy as np

import probe_ref
import scenes

F = np.float32
STEPS = 2
COUNTS = (2, 3, 63, 64, 65, 128, 129, 1024)
SWEEP_LINES, SWEEP_COUNT = 134, 150
SHEPARD, VY = 1, 3
LIQUID, BOUNDARY, ALL = 1 << 1, 1 << 3, (1 << 1) | (1 << 2) | (1 << 3)


def scene():
    return scenes.liquid_box((8.0, 8.0, 8.0), (10, 8, 10), jitter_in_r0=0.2)


def oracle_state(sc, steps=STEPS):
    """A sample_ref state from the oracle's sorted state of step `steps` (no GPU)."""
    cfg = sc["cfg"]
    N = cfg.particleCount
    ora = scenes.oracle_for(sc, threads=8)
    for _ in range(steps):
        ora.step()
    pi = ora.buffer("particleIndex").reshape(-1, 2)
    state = dict(pos=ora.buffer("sortedPosition").reshape(-1, 4)[:N, :3].copy(), vel=ora.buffer("sortedVelocity").reshape(-1, 4)[:N, :3].copy(),
                 rho=ora.buffer("rho")[:N].copy(), p=ora.buffer("pressure")[:N].copy(),
                 types=ora.buffer("position").reshape(-1, 4)[:N][pi[:, 1].astype(np.int64), 3].copy(), keys=pi[:, 0].copy(),
                 G=int(cfg.gridCellCount), h=float(cfg.h), simScale=float(cfg.simulationScale),
                 massWpoly6=float(cfg.mass) * float(cfg.Wpoly6Coefficient))
    ora.close()
    return state


def line(origin, step, count, field=SHEPARD, iso=0.5, mask=LIQUID):
    ln = np.zeros(1, probe_ref.LINE_DTYPE)
    ln["origin"], ln["step"], ln["count"], ln["field"], ln["iso"], ln["typeMask"] = \
        np.asarray(origin, F), np.asarray(step, F), count, field, F(iso), mask
    return ln


def between(a, b, count, **kw):
    """The line of `count` points from a to b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return line(a, (b - a) / (count - 1), count, **kw)


def _cut_at_outside(state, ln):
    """ln shortened so that its far end is the highest of its points that is outside (there must be one above point 1)."""
    f = probe_ref.line_fields(state, ln)[0]
    out = np.flatnonzero(~(f >= ln["iso"][0]))
    assert out.size and out[-1] >= 2, "no outside point to end the line at"
    ln = ln.copy()
    ln["count"] = int(out[-1]) + 1
    return ln


def build(cfg, state):
    """[(name, lines)] in the order of the GPU test's one set; `state`: the sorted state the lines will be recorded on (two cases
    take a value from it: an iso equal to a sampled f_K, and the far end of the lines of a velocity field)."""
    r0 = float(cfg.r0)
    xc, zc = 7.1 * r0, 7.3 * r0  # a column near the middle of the liquid, off every lattice plane
    cases = []
    # a column from inside the liquid to the air above it, at every count: the crossing sits at about the same fraction of the line
    cases.append(("counts", np.concatenate([between((xc, 5.0 * r0, zc), (xc, 13.6 * r0, zc), n) for n in COUNTS])))
    # the sweep: origins one step apart, so the crossing index K takes SWEEP_LINES consecutive values
    dy = 0.05 * r0
    ys = 10.14 * r0  # about where the surface is: line 0 meets it near its point 10, line i near 10 + i
    cases.append(("sweep", np.concatenate([line((xc, ys - (10.5 + i) * dy, zc), (0.0, dy, 0.0), SWEEP_COUNT) for i in range(SWEEP_LINES)])))
    # through the block along x, outside at both ends, and reversed: the two faces
    a, b = (1.2 * r0, 6.1 * r0, zc), (14.9 * r0, 6.3 * r0, zc)
    cases.append(("faces", np.concatenate([between(a, b, 90), between(b, a, 90)])))
    cases.append(("submerged", between((5.0 * r0, 4.5 * r0, 5.0 * r0), (9.0 * r0, 7.5 * r0, 9.5 * r0), 10)))
    cases.append(("dry", between((xc, 11.5 * r0, zc), (xc, 14.5 * r0, 5.0 * r0), 70)))
    # iso equal to the sampled f_K: t == 0
    ln = between((xc + 0.3 * r0, 5.0 * r0, zc), (xc + 0.3 * r0, 13.6 * r0, zc), 65)
    f = probe_ref.line_fields(state, ln)[0]
    status, K, _ = probe_ref.level_of(f, 0.5)
    assert status == probe_ref.FOUND
    ln["iso"] = f[K]
    cases.append(("t zero", ln))
    # vy against 0 on a diagonal through the block (the floor pushes the lowest layer up while the rest falls): several crossings,
    # the far one wins
    cases.append(("vy", _cut_at_outside(state, between((12.8 * r0, 1.5 * r0, 12.6 * r0), (5.0 * r0, 9.6 * r0, 3.5 * r0), 257, field=VY, iso=0.0))))
    # iso <= 0 on lines that leave the grid: the zero record out there is inside
    cases.append(("leaves up", between((xc, 5.0 * r0, zc), (xc, 40.0 * r0, zc), 66, iso=0.0)))
    cases.append(("enters", _cut_at_outside(state, between((-9.0 * r0, -7.0 * r0, -5.0 * r0), (xc, 7.0 * r0, zc), 100, field=VY, iso=0.0))))
    cases.append(("below zero", between((xc, 5.0 * r0, zc), (40.0 * r0, 30.0 * r0, zc), 40, field=VY, iso=-1.0)))
    # three masks on a column from the liquid through the air and the lid of the box (the liquid's own level, or the lid's), and on
    # one from below the floor to the middle of the liquid (submerged, or the floor's level): between them no two masks agree
    masks = (LIQUID, BOUNDARY, ALL)
    lid = [between((xc, 5.0 * r0, zc), (xc, 17.5 * r0, zc), 130, mask=m) for m in masks]
    floor = [between((xc, -1.0 * r0, zc), (xc, 6.0 * r0, zc), 70, mask=m) for m in masks]
    cases.append(("masks", np.concatenate(lid + floor)))
    return cases


def all_lines(cases):
    return np.concatenate([lines for _, lines in cases])


def spans(cases):
    """name -> slice of the case's lines in all_lines(cases)."""
    out, at = {}, 0
    for name, lines in cases:
        out[name] = slice(at, at + lines.shape[0])
        at += lines.shape[0]
    return out


def check_claims(cases, records, fields):
    """Asserts what the cases claim, on records float32[L, 8] of all_lines(cases) and their field values (probe_ref.line_fields)."""
    sp = spans(cases)
    lines = all_lines(cases)
    status, K = records[:, 4].astype(int), records[:, 5].astype(int)
    s = sp["counts"]
    assert tuple(lines["count"][s]) == COUNTS and (status[s] == probe_ref.FOUND).all()
    assert K[s][-1] > 3 * 64 and lines["count"][s][-1] - K[s][-1] > 3 * 64  # the long line crosses several chunks from either end
    s = sp["sweep"]
    assert (status[s] == probe_ref.FOUND).all()
    assert s.stop - s.start >= 130 and np.array_equal(np.diff(K[s]), np.ones(s.stop - s.start - 1, int)), K[s]
    s = sp["faces"]
    assert (status[s] == probe_ref.FOUND).all() and records[s][0, 0] > records[s][1, 0] + 3.0  # the far face, then the near one
    assert status[sp["submerged"]][0] == probe_ref.SUBMERGED and status[sp["dry"]][0] == probe_ref.DRY
    i = sp["t zero"].start
    assert status[i] == probe_ref.FOUND and records[i, 3] == K[i] and records[i, 6] == lines["iso"][i]
    i = sp["vy"].start
    inside = fields[i] >= 0
    assert status[i] == probe_ref.FOUND and np.count_nonzero(inside[:-1] & ~inside[1:]) >= 3
    i = sp["leaves up"].start
    assert status[i] == probe_ref.SUBMERGED and records[i, 6] == 0 and records[i, 1] > 30.0
    i = sp["enters"].start
    assert status[i] == probe_ref.FOUND and (fields[i][:10] == 0).all() and records[i, 7] < 0
    i = sp["below zero"].start
    assert status[i] == probe_ref.SUBMERGED
    m = records[sp["masks"]]
    assert m[0].tobytes() != m[1].tobytes() and m[3].tobytes() != m[4].tobytes() and m[4].tobytes() != m[5].tobytes()
    assert (m[:3, 4] == probe_ref.FOUND).all() and tuple(m[3:, 4]) == (probe_ref.SUBMERGED, probe_ref.FOUND, probe_ref.SUBMERGED)
