"""Scenes that carry the search bands (csrc/sph_bands.hip) to the states where they can break: hand-placed pairs
across the y / z faces and the yz edges of a cell at the last separation the reference accepts, lone candidates whose face
distance is the band radius to the ulp, particles outside the box whose keys are not their cells, particle counts at the block
edges of the band scan, and grids with three and with two cells along an axis. Inputs only: nothing here calls the library's
solver. The oracle's states are computed once per scene and shared by the CPU and the GPU tests."""
import numpy as np

import band_ref
import edit_ref
import scenes
from test_fn_staging import STEPS
from test_gpu_parity import canon_ora

F = np.float32
INF = F(np.inf)
LIQUID = F(1.1)

# slot (band_ref.SLOT_STEP) -> the name of the kind: the face or edge of P's cell that Q lies across
KIND = {3: "y lo", 4: "y hi", 1: "z lo", 6: "z hi", 0: "y lo z lo", 2: "y hi z lo", 5: "y lo z hi", 7: "y hi z hi"}
OFFSETS = (0, -1, -2, -8, 1, 2, 8)  # ulps of Q's coordinate from the last accepted separation; > 0: farther from P


def ulp_steps(x, n):
    x = F(x)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, INF if n > 0 else -INF)
    return x


def cell_of(cfg, q):
    """(int)(q * cellSizeInv) for q >= 0, as k_hash."""
    return int(F(F(q) * F(cfg.hashGridCellSizeInv)))


def first_in_cell(cfg, b):
    """The smallest float that truncates to cell b: by nextafter steps from fl(b * cellSize)."""
    q = F(F(b) * F(cfg.hashGridCellSize))
    while cell_of(cfg, q) < b:
        q = np.nextafter(q, INF)
    while q > 0 and cell_of(cfg, np.nextafter(q, -INF)) >= b:
        q = np.nextafter(q, -INF)
    return q


def last_in_cell(cfg, b):
    return np.nextafter(first_in_cell(cfg, b + 1), -INF)


def search_r2(cfg):
    """r_thr^2 of the reference's second pass for a particle with fewer than 32 others within h: ((31 h) / 30)^2 in float."""
    r = F(F(F(31.0) * F(cfg.h)) / F(30.0))
    return F(r * r)


def accepts(cfg, p, q):
    """The reference's test d^2 <= r_thr^2 for the positions p and q, float operation by float operation."""
    e = (np.asarray(p, F) - np.asarray(q, F)).astype(F)
    d2 = F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))
    return bool(d2 <= search_r2(cfg))


def last_accepted(cfg, p, q, axis, away):
    """q moved along `axis` (away = +1 / -1: the direction that leads away from p) to the farthest coordinate the reference still
    accepts as a neighbour of p."""
    q = np.array(q, F)
    q[axis] = F(p[axis] + F(away) * np.sqrt(search_r2(cfg)))  # (one rounding away from it: the loops below take a few steps)
    while accepts(cfg, p, q):
        q[axis] = np.nextafter(q[axis], INF * F(away))
    while not accepts(cfg, p, q):
        q[axis] = np.nextafter(q[axis], -INF * F(away))
    return q[axis]


class _Placer:
    """Greedy placement: a cluster goes to the first site of its list at which every one of its particles is farther than `sep`
    from every particle placed before — so clusters are not each other's neighbours and no neighbour row fills up."""

    def __init__(self, sep):
        self.sep2 = float(sep) ** 2
        self.pts = np.zeros((0, 3), np.float64)

    def place(self, sites, what):
        for pts in sites:
            pts = np.asarray(pts, F).reshape(-1, 3)
            if self.pts.shape[0]:
                d2 = ((pts[:, None, :].astype(np.float64) - self.pts[None, :, :]) ** 2).sum(-1)
                if d2.min() <= self.sep2:
                    continue
            first = self.pts.shape[0]
            self.pts = np.concatenate([self.pts, pts.astype(np.float64)])
            return first, pts
        raise AssertionError("no free site for " + what)


def _free_grid(cfg, pitch=0.45):
    """Coordinates for the free axes of a cluster: inside the boundary shell, off the cell faces."""
    lo, hi = 1.1 * float(cfg.r0), float(cfg.xmax) - 1.1 * float(cfg.r0)
    return [F(v) for v in np.arange(lo, hi, pitch)]


def _pair_sites(cfg, slot, off, long_axis):
    """All placements of one pair of kind `slot`: P just inside its cell at the face(s), Q across, `off` ulps from the last accepted
    separation along `long_axis` (for an edge the other of y / z is one float across its face)."""
    sy, sz = band_ref.SLOT_STEP[slot]
    step = {1: sy, 2: sz}
    free = _free_grid(cfg)
    cells = {-1: (2, 1, 3), 1: (1, 2, 0)}  # P's cell along an axis with a step (interior faces only)

    def at_face(b, s):  # (P's coordinate, the first coordinate across the face)
        if s < 0:
            p = first_in_cell(cfg, b)
            return p, np.nextafter(p, -INF)
        p = last_in_cell(cfg, b)
        return p, np.nextafter(p, INF)

    other = 3 - long_axis
    for b in cells[step[long_axis]]:
        pl, ql = at_face(b, step[long_axis])
        others = [at_face(bo, step[other]) for bo in cells[step[other]]] if step[other] else [(t, t) for t in free]
        far = None  # Q's coordinate along the long axis: it depends on the differences only, so not on x or on a free coordinate
        for po, qo in others:
            p, q = np.zeros(3, F), np.zeros(3, F)
            p[long_axis], q[long_axis] = pl, ql
            p[other], q[other] = po, qo
            if far is None or step[other]:
                far = ulp_steps(last_accepted(cfg, p, q, long_axis, step[long_axis]), off * step[long_axis])
            q[long_axis] = far
            for x in free:
                p[0] = q[0] = x
                yield [p.copy(), q.copy()]


def _lone_list(cfg):
    """(axis, side, what, coordinate along the axis, bit, expected membership, exact distance or None) of the lone candidates."""
    rb, cs, h = band_ref.band_radius(cfg), F(cfg.hashGridCellSize), F(cfg.h)
    bits = {(1, "lo"): 4, (1, "hi"): 3, (2, "lo"): 6, (2, "hi"): 1}
    out = []
    for axis in (1, 2):
        # cell 0: the lo face is the coordinate 0, the hi face fl(cellSize) — both distances are exact differences on the grid of Rb
        face = F(F(1) * cs)
        for n in (-1, 0, 1):
            d = ulp_steps(rb, n)
            out.append((axis, "lo", "Rb%+d" % n, d, bits[axis, "lo"], n <= 0, d))
            q = F(face - d)
            assert F(face - q) == d and cell_of(cfg, q) == 0
            out.append((axis, "hi", "Rb%+d" % n, q, bits[axis, "hi"], n <= 0, d))
        # farther cells: the coordinate's grid is coarser than Rb's — the last coordinate inside the band and the first outside it.
        # Cell 2 inside the box; the cells 4 and 5 at the face 5 cellSize outside it (reference mode takes such input, the grid
        # declares nine cells per axis): fl(5 cellSize) is 6 ulps of Rb off the exact product, so there a face distance evaluated
        # with a contracted multiply-subtract changes the flag (the CPU test checks that it does)
        for lo_cell, hi_cell in ((2, 2), (5, 4)):
            lo_face, hi_face = F(F(lo_cell) * cs), F(F(hi_cell + 1) * cs)
            q = F(lo_face + rb)
            while F(q - lo_face) <= rb:
                q = np.nextafter(q, INF)
            while F(q - lo_face) > rb:
                q = np.nextafter(q, -INF)
            assert cell_of(cfg, q) == lo_cell
            out.append((axis, "lo", "last inside", q, bits[axis, "lo"], True, None))
            out.append((axis, "lo", "first outside", np.nextafter(q, INF), bits[axis, "lo"], False, None))
            q = F(hi_face - rb)
            while F(hi_face - q) <= rb:
                q = np.nextafter(q, -INF)
            while F(hi_face - q) > rb:
                q = np.nextafter(q, INF)
            assert cell_of(cfg, q) == hi_cell
            out.append((axis, "hi", "last inside", q, bits[axis, "hi"], True, None))
            out.append((axis, "hi", "first outside", np.nextafter(q, -INF), bits[axis, "hi"], False, None))
        # on a face exactly, on the half-cell plane, in the middle of a cell (within Rb of both faces: cells are 2 h wide)
        out.append((axis, "lo", "on a face", F(F(2) * cs), None, None, None))
        out.append((axis, "lo", "half-cell plane", F(F(F(1) * cs) + h), bits[axis, "lo"], True, None))
        out.append((axis, "hi", "middle of a cell", F(F(1.5) * cs), bits[axis, "hi"], True, None))
    return out


_face = {}


def face_scene():
    """The `tiny` box and its boundary shell with the liquid replaced by hand-placed particles, eight of the lone ones outside the
    box but inside the declared grid (the dict of scenes.liquid_box plus
    "pairs": (slot, long axis, offset in ulps, id of P, id of Q), "control": the same for one pair across an x face, "lone":
    (id, axis, side, what, bit, expected, distance))."""
    if "scene" in _face:
        sc = _face["scene"]
        return dict(sc, cfg=type(sc["cfg"]).from_buffer_copy(sc["cfg"]))
    base = scenes.SCENES["tiny"]()
    cfg = base["cfg"]
    rf = float(np.sqrt(np.float64(band_ref.filter_r2(cfg.h))))
    placer = _Placer(1.06 * rf)
    cs = F(cfg.hashGridCellSize)
    pairs, lone = [], []
    # the edges first (they have the fewest sites: the nine interior corners); the long axis of an edge pair is y for two of the
    # edges and z for the other two, so each term of the conjunction decides somewhere
    def place_pairs(kinds, offsets=OFFSETS):
        for slot, long_axis in kinds:
            for off in offsets:
                first, _ = placer.place(_pair_sites(cfg, slot, off, long_axis), "%s, %+d ulps" % (KIND[slot], off))
                pairs.append((slot, long_axis, off, first, first + 1))

    place_pairs(((0, 1), (7, 1), (2, 2), (5, 2)))
    # lone candidates next (their y and z are given): the other of y / z on a face or on a half-cell plane, x free
    free = _free_grid(cfg)
    for axis, side, what, coord, bit, member, dist in _lone_list(cfg):
        def sites():
            for t in [v for k in (2, 1, 3, 0) for v in ((F(F(k) * cs) if k else None), F(F(F(k) * cs) + F(cfg.h))) if v is not None]:
                for x in free:
                    p = np.zeros(3, F)
                    p[0], p[axis], p[3 - axis] = x, coord, t
                    yield [p]
        first, _ = placer.place(sites(), "lone %s %s" % (side, what))
        lone.append((first, axis, side, what, bit, member, dist))
    # the faces (the other of y / z is free) and the control last
    place_pairs(((3, 1), (4, 1), (1, 2), (6, 2)))
    place_pairs(((0, 2), (7, 2), (2, 1), (5, 1)), (0, 1, 8))  # the edges' other long axis, as far as the box has room
    # the control on the own row: P just inside x cell 2, Q across the x face, at the last accepted separation and 8 ulps beyond
    control = []
    for off in (0, 8):
        def sites():
            px = first_in_cell(cfg, 2)
            p, q = np.array([px, 0, 0], F), np.array([np.nextafter(px, -INF), 0, 0], F)
            qx = ulp_steps(last_accepted(cfg, p, q, 0, -1), -off)
            for y in _free_grid(cfg):
                for z in _free_grid(cfg):
                    yield [np.array([px, y, z], F), np.array([qx, y, z], F)]
        first, _ = placer.place(sites(), "the x control")
        control.append((off, first, first + 1))
    liq = np.zeros((placer.pts.shape[0], 4), F)
    liq[:, :3] = placer.pts.astype(F)
    assert np.array_equal(liq[:, :3].astype(np.float64), placer.pts)  # (the float coordinates were kept exactly)
    liq[:, 3] = LIQUID
    nl = base["numOfLiquidP"]
    pos = np.concatenate([liq, base["position"][nl:]]).astype(F)
    vel = np.concatenate([np.zeros_like(liq), base["velocity"][nl:]]).astype(F)
    cfg.particleCount = pos.shape[0]
    _face["scene"] = dict(base, cfg=cfg, position=pos, velocity=vel, numOfLiquidP=liq.shape[0], pairs=pairs, control=control,
                          lone=lone)
    return face_scene()


def _cut_grid(cfg, cells):
    """The declared grid cut to `cells` per axis (None: as declared), as test_fn_staging._tight does for z."""
    for name, n in zip(("gridCellsX", "gridCellsY", "gridCellsZ"), cells):
        if n is not None:
            setattr(cfg, name, int(n))
    cfg.gridCellCount = cfg.gridCellsX * cfg.gridCellsY * cfg.gridCellsZ
    return cfg


def stray_scene():
    """`tiny` in reference mode with x and y cut to the four cells the box occupies (4 x 4 x 9 cells: the bands apply), and a few
    dozen liquid particles moved out of the box, next to the boundary shell: below zero in x, y, z and their combinations (the
    coordinate truncates towards zero: the key is a real cell's, the premise fails), beyond gx cells in x (the key is the first
    cell of the next y row) and beyond gy cells in y (the key is a cell of the next z layer). Every key stays below G. Returns the
    scene with "moved": the original ids of the moved particles."""
    sc = scenes.SCENES["tiny"]()
    cfg = _cut_grid(sc["cfg"], (4, 4, None))
    pos = sc["position"].copy()
    r0, cs = F(cfg.r0), F(cfg.hashGridCellSize)
    out = F(-0.3) * r0                      # below zero: 0.8 r0 from the shell's layer at 0.5 r0
    over = F(F(4) * cs) + F(0.3) * r0       # beyond the fourth cell: the shell's last layer is 0.5 r0 inside the box
    along = [F(4.1) * r0 + F(k) * F(2.3) * r0 for k in range(4)]  # spots along a wall, cell rows 1 .. 2
    spots = []
    for a in along:
        b = F(a + F(1.3) * r0)
        spots += [(out, a, b), (a, out, b), (a, b, out),          # one coordinate below zero
                  (over, a, b), (over, F(3.6) * cs, a),           # x beyond the grid; from the last y row the key wraps into the next z layer
                  (a, over, b)]                                   # y beyond the grid: the key is (cx, 0, cz + 1)
    for a in along[:2]:
        spots += [(out, out, a), (out, a, out), (a, out, out)]    # along the box's edges
    spots += [(out, out, out), (over, out, along[0]), (out, over, along[1]), (over, F(0.2) * r0, out)]
    moved = np.arange(len(spots))
    pos[moved, :3] = np.array(spots, F)     # the first liquid particles of the lattice
    assert len(spots) < sc["numOfLiquidP"]
    sc["position"] = pos
    sc["moved"] = moved
    return sc


def counted_box(n, capacity=0):
    """A wide-mask liquid box of 134 784 particles (lattice with jitter 0.05 r0 first, then the boundary shell) trimmed from the
    end of the liquid to exactly n particles; capacity > n leaves room for added particles (bandCap != N)."""
    if "counted" not in _face:
        _face["counted"] = scenes.liquid_box((40.0, 40.0, 40.0), (46, 46, 46), jitter_in_r0=0.05, mask=0xffffffff)
    base = _face["counted"]
    total, nl = base["cfg"].particleCount, base["numOfLiquidP"]
    cut = total - n
    assert 0 <= cut < nl
    keep = np.concatenate([np.arange(nl - cut), np.arange(nl, total)])
    return dict(base, cfg=edit_ref.with_count(base["cfg"], n, capacity), position=np.ascontiguousarray(base["position"][keep]),
                velocity=np.ascontiguousarray(base["velocity"][keep]), numOfLiquidP=nl - cut)


BAND_SUPER = 1024  # waves per block of the band scan (sph_bands.hip)
COUNTS = (65536, 65537, 131072, 131073, 133001)  # waves: 1024, 1025, 2048 (the total stands alone in a third block), 2049, 2079


def grid_scene(name):
    """Boxes whose declared grid is cut to the cells they occupy along some axes: "333" — six h per axis, 3 x 3 x 3 cells, liquid in
    every layer; "3x" / "3y" / "3z" — three cells along one axis, the declared nine along the others; "2x" / "2y" / "2z" — two
    cells along one axis (four h), where the bands must stay off."""
    if name == "333":
        sc = scenes.liquid_box((6.0, 6.0, 6.0), (10, 10, 10), origin_in_r0=(1.5, 1.5, 1.5))
        _cut_grid(sc["cfg"], (3, 3, 3))
        return sc
    n, axis = int(name[0]), "xyz".index(name[1])
    box, lattice, cells = [8.0, 8.0, 8.0], [10, 10, 10], [None, None, None]
    box[axis], lattice[axis], cells[axis] = 2.0 * n, 10 if n == 3 else 5, n
    sc = scenes.liquid_box(tuple(box), tuple(lattice), origin_in_r0=(1.5, 1.5, 1.5))
    _cut_grid(sc["cfg"], cells)
    return sc


GRID_NAMES = ("333", "3x", "3y", "3z", "2x", "2y", "2z")
_oracle = {}


def scene(name):
    if name == "face":
        return face_scene()
    if name == "stray":
        return stray_scene()
    return grid_scene(name)


def oracle_states(name, steps=STEPS):
    """Canonical oracle buffers after each of `steps` steps of scene(name): computed once, shared, never changed."""
    if name not in _oracle:
        sc = scene(name)
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for _ in range(steps):
            ora.step()
            out.append(canon_ora(ora, N))
        ora.close()
        _oracle[name] = out
    assert len(_oracle[name]) >= steps
    return _oracle[name]


SEARCH_BUFFERS = ("particleIndex", "gridCellIndexFixedUp", "sortedPosition", "neighborIds", "neighborDist")


def oracle_search(sc, full_step=False):
    """The oracle's canonical buffers through computeDensity (or after one whole step) of a scene, uncached (the large boxes)."""
    N = sc["cfg"].particleCount
    ora = scenes.oracle_for(sc, threads=8)
    if full_step:
        ora.step()
    else:
        for st in scenes.STAGE_SEQUENCE[:scenes.STAGE_SEQUENCE.index("computeDensity") + 1]:
            ora.run(st)
    out = canon_ora(ora, N)
    ora.close()
    return out


def sorted_state(canon):
    """(positions, keys, cell table) of the sorted state a canonical set of buffers holds."""
    keys = canon["particleIndex"].reshape(-1, 2)[:, 0].astype(np.int64)
    return canon["sortedPosition"][:, :3], keys, canon["gridCellIndexFixedUp"]
