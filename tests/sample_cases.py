"""Scenes that carry the analysis chain (the cell walks of csrc/sph_sample_walk.h with their hit functions, the marching-cubes
kernels of csrc/sph_surface.hip) to the states where it can break: lone liquid particles with query points at the
support boundary r2 < h*h to the ulp, in the ring where the weights are zero or subnormal, across cell faces, edges and corners and
at negative coordinates; and a lattice of lone particles whose occupancy pattern is the inside / outside map of an isosurface, so
that marching cubes can be handed any case. Inputs only: nothing here calls the library's solver."""
import numpy as np

import sample_ref
import scenes
from band_cases import F, INF, LIQUID, _Placer, cell_of, first_in_cell, last_in_cell, ulp_steps

EDGE_OFFSETS = (0, -1, -2, -8, 1, 2, 8)  # ulps of the query's coordinate from the last accepted one; > 0: farther from the particle
# the kinds of a query, from the particle outward (the sums are those of the sampling contract for a lone particle):
KINDS = ("half",          # about half way: every sum normal
         "s_normal",      # the last coordinate with normal S = w * (1/rho): the products v * vel are subnormal
         "s_subnormal",   # the next one: S subnormal
         "w_normal",      # the last coordinate with normal W = w
         "w_subnormal",   # the next one
         "s_first",       # the last coordinate with S != 0
         "s_zero",        # the next one: W != 0, S == 0
         "w_first",       # the last coordinate with w != 0: the smallest W on this line
         "w_zero",        # the next one: n = 1, every sum 0
         ) + tuple("edge%+d" % o for o in EDGE_OFFSETS)  # the last coordinate with r2 < h*h, and ulps of it nearer and farther
TINY = F(np.finfo(np.float32).tiny)


class Constants:
    """The floats of the sampling contract as the step computes them."""

    def __init__(self, cfg):
        self.h = F(cfg.h)
        self.hh = F(self.h * self.h)
        sim = F(cfg.simulationScale)
        self.ss2 = F(sim * sim)
        hs = F(self.h * sim)
        self.hs2 = F(hs * hs)
        self.hs6 = F(F(self.hs2 * self.hs2) * self.hs2)
        self.massWpoly6 = float(cfg.mass) * float(cfg.Wpoly6Coefficient)
        self.rho_lone = F(float(self.hs6) * self.massWpoly6)  # computeDensity's clamp: the density of a particle without neighbours
        self.inv_rho = F(F(1) / self.rho_lone)


def r2_of(p, q):
    """dx*dx + dy*dy + dz*dz of the contract, d = q - p (q the query point)."""
    d = (np.asarray(q, F) - np.asarray(p, F)).astype(F)
    return F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))


def lone_sums(k, p, q):
    """(accepted, w, v) of the contract for the query q next to the lone particle p."""
    r2 = r2_of(p, q)
    a = F(k.hs2 - F(r2 * k.ss2))
    w = F(F(a * a) * a)
    return bool(r2 < k.hh), w, F(w * k.inv_rho)


def _ordinal(x):
    i = int(F(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _float_of(o):
    return np.array(o if o >= 0 else (-o) | 0x80000000, np.uint32).view(F)[()]


def last_true(pred, p, q, axis, away, reach):
    """q moved along `axis` (away = +1 / -1: the direction that leads away from p) to the farthest coordinate at which pred(q)
    holds: a search over the floats between q[axis] (where it holds) and p[axis] + away * reach (where it does not) for the place
    where the predicate, which is monotone along the line, changes; the two floats at the change are evaluated and checked."""
    q = np.array(q, F)
    lo, hi = _ordinal(q[axis]), _ordinal(F(p[axis] + F(away) * F(reach)))

    def holds(o):
        q[axis] = _float_of(o)
        return pred(q)

    assert holds(lo) and not holds(hi)
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if holds(mid):
            lo = mid
        else:
            hi = mid
    c = _float_of(lo)
    q[axis] = c
    assert pred(q)
    q[axis] = np.nextafter(c, INF * F(away))
    assert not pred(q)
    return c


def directions(s):
    """The twelve query directions of a particle whose `across` signs are s: (long axis, away, {other axis: signed offset in h});
    the six axis directions, four face diagonals, two body diagonals. The query moves along the long axis; its other coordinates
    are the particle's plus the offsets."""
    out = [(a, sg, {}) for a in range(3) for sg in (1, -1)]
    out += [(0, s[0], {1: 0.6 * s[1]}), (1, s[1], {2: 0.6 * s[2]}), (2, s[2], {0: 0.6 * s[0]}), (0, -s[0], {2: 0.6 * s[2]})]
    out += [(0, s[0], {1: 0.5 * s[1], 2: 0.5 * s[2]}), (2, s[2], {0: 0.5 * s[0], 1: -0.5 * s[1]})]
    return out


def line_queries(k, p, axis, away, offsets):
    """{kind: query point} along one direction from the lone particle p."""
    q0 = np.array(p, F)
    for b, o in offsets.items():
        q0[b] = F(p[b] + F(o) * k.h)
    q0[axis] = F(p[axis] + F(away) * F(0.3) * k.h)

    def coordinate(pred):
        return last_true(pred, p, q0, axis, away, F(1.1) * k.h)

    def sums(q):
        return lone_sums(k, p, q)

    last = {
        "s_normal": coordinate(lambda q: sums(q)[0] and sums(q)[2] >= TINY),
        "w_normal": coordinate(lambda q: sums(q)[0] and sums(q)[1] >= TINY),
        "s_first": coordinate(lambda q: sums(q)[0] and sums(q)[2] != 0),
        "w_first": coordinate(lambda q: sums(q)[0] and sums(q)[1] != 0),
        "edge": coordinate(lambda q: sums(q)[0]),
    }
    step = INF * F(away)
    coords = {"half": F(p[axis] + F(away) * F(0.5) * k.h), "s_normal": last["s_normal"], "s_subnormal": np.nextafter(last["s_normal"], step),
              "w_normal": last["w_normal"], "w_subnormal": np.nextafter(last["w_normal"], step),
              "s_first": last["s_first"], "s_zero": np.nextafter(last["s_first"], step),
              "w_first": last["w_first"], "w_zero": np.nextafter(last["w_first"], step)}
    for o in EDGE_OFFSETS:
        coords["edge%+d" % o] = ulp_steps(last["edge"], o * away)
    out = {}
    for kind in KINDS:
        q = q0.copy()
        q[axis] = coords[kind]
        out[kind] = q
    return out


# placements of the lone particles: (name, per axis "hi" (the last float of a cell: queries go across the high face), "lo" (the first
# float of a cell: across the low face), "zero" (cell 0, 0.9 h from the coordinate 0: queries go to negative coordinates) or None
# (free: off the faces))
PLACEMENTS = ([("middle", (None, None, None)),  # (first: it gets the middle of cell (1, 1, 1))
               ("corner hi hi hi", ("hi", "hi", "hi")), ("corner lo lo lo", ("lo", "lo", "lo")), ("corner hi lo hi", ("hi", "lo", "hi"))]
              + [("%s %s" % (w, "xyz"[a]), tuple(w if b == a else None for b in range(3))) for w in ("hi", "lo", "zero") for a in range(3)])
_cache = {}


def _axis_candidates(cfg, what):
    h = F(cfg.h)
    if what == "hi":
        return [last_in_cell(cfg, b) for b in (1, 2, 0)]
    if what == "lo":
        return [first_in_cell(cfg, b) for b in (2, 1, 3)]
    if what == "zero":
        return [F(F(0.9) * h)]
    return [F(F(t) * h) for t in (3.0, 5.2, 1.3, 6.7, 4.4, 2.3)]  # 3 h: the middle of cell 1


def ring_scene():
    """The `tiny` box and its boundary shell with the liquid lattice replaced by lone liquid particles, each farther than 2.1 h from
    every other one and at least 0.65 h from the shell's layer (its density stays the clamp), with a velocity of three different
    components of the order 1e-3. The dict of scenes.liquid_box plus
    "lone": [(name, placement per axis, across signs)] by particle id, and
    "queries": (points float32[Q, 3], particle id int[Q], direction number int[Q], kind number int[Q] (index into KINDS; -1: the
    particle itself, r = 0), crossed bool[Q, 3]: the axes along which the query lies across the face the particle was put at)."""
    if "ring" in _cache:
        sc = _cache["ring"]
        return dict(sc, cfg=type(sc["cfg"]).from_buffer_copy(sc["cfg"]))
    base = scenes.SCENES["tiny"]()
    cfg = base["cfg"]
    k = Constants(cfg)
    placer = _Placer(2.1 * float(k.h))
    lone = []
    for name, where in PLACEMENTS:
        def sites():
            for x in _axis_candidates(cfg, where[0]):
                for y in _axis_candidates(cfg, where[1]):
                    for z in _axis_candidates(cfg, where[2]):
                        yield [np.array([x, y, z], F)]
        placer.place(sites(), name)
        lone.append((name, where))
    n = len(lone)
    liq = np.zeros((n, 4), F)
    liq[:, :3] = placer.pts.astype(F)
    assert np.array_equal(liq[:, :3].astype(np.float64), placer.pts)
    liq[:, 3] = LIQUID
    lvel = np.zeros((n, 4), F)
    for i in range(n):
        lvel[i, :3] = np.array([1.5e-3, -2.5e-3, 0.75e-3], F) * F(1.0 + 0.0625 * i)
    points, owner, direction, kind, crossed = [], [], [], [], []
    out_lone = []
    mid = F(0.5) * F(cfg.xmax)
    for i, (name, where) in enumerate(lone):
        p = liq[i, :3]
        s = tuple({"hi": 1, "lo": -1, "zero": -1, None: (1 if p[a] < mid else -1)}[where[a]] for a in range(3))
        out_lone.append((name, where, s))
        points.append(p.copy()); owner.append(i); direction.append(-1); kind.append(-1); crossed.append((False,) * 3)
        for dn, (axis, away, offsets) in enumerate(directions(s)):
            moved = {axis: away}
            moved.update({b: (1 if o > 0 else -1) for b, o in offsets.items()})
            cr = tuple(where[a] in ("hi", "lo") and moved.get(a, 0) == s[a] for a in range(3))
            for kn, (_, q) in enumerate(line_queries(k, p, axis, away, offsets).items()):
                points.append(q); owner.append(i); direction.append(dn); kind.append(kn); crossed.append(cr)
    nl = base["numOfLiquidP"]
    pos = np.concatenate([liq, base["position"][nl:]]).astype(F)
    vel = np.concatenate([lvel, base["velocity"][nl:]]).astype(F)
    cfg.particleCount = pos.shape[0]
    queries = (np.array(points, F), np.array(owner), np.array(direction), np.array(kind), np.array(crossed, bool))
    _cache["ring"] = dict(base, cfg=cfg, position=pos, velocity=vel, numOfLiquidP=n, lone=out_lone, queries=queries)
    return ring_scene()


def synthetic_state(sc):
    """A sample_ref state of the scene as it stands (original order, keys in the table), every density the lone particle's clamp
    and every pressure 0: what the first step's sorted state holds for the liquid of these scenes, up to the order."""
    cfg = sc["cfg"]
    k = Constants(cfg)
    n = sc["position"].shape[0]
    return dict(pos=sc["position"][:, :3].copy(), vel=sc["velocity"][:, :3].copy(), rho=np.full(n, k.rho_lone, F), p=np.zeros(n, F),
                types=sc["position"][:, 3].copy(), keys=np.zeros(n, np.uint32), G=1, h=float(cfg.h), simScale=float(cfg.simulationScale),
                massWpoly6=k.massWpoly6)


def brick_subset(sc):
    """Indices into the queries for the brick-walk calls: every kind along one axis direction, one face diagonal and one body diagonal
    of the middle particle, and for every query direction that crosses a face, an edge or a corner, or that leads to negative
    coordinates, the kinds half, s_normal, s_first, w_first, w_zero, edge+0 and edge+1."""
    pts, owner, direction, kind, crossed = sc["queries"]
    names = [name for name, _, _ in sc["lone"]]
    middle = names.index("middle")
    few = [KINDS.index(n) for n in ("half", "s_normal", "s_first", "w_first", "w_zero", "edge+0", "edge+1")]
    pick = (owner == middle) & np.isin(direction, (0, 6, 10))
    pick |= (owner == middle) & (kind == -1)
    pick |= (crossed.any(1) | (pts < 0).any(1)) & np.isin(kind, few)
    return np.flatnonzero(pick)


def brick_calls(sc, dims):
    """(origin, spacing) of the grid calls of one query of brick_subset: the query is lattice point (0, 0, 0); the spacings are
    +-h/2 per axis, all toward the particle, all away from it, and alternating."""
    h = F(sc["cfg"].h)
    half = F(h / F(2))
    pts, owner = sc["queries"][0], sc["queries"][1]
    calls = []
    for qi in brick_subset(sc):
        q, p = pts[qi], sc["position"][owner[qi], :3]
        toward = np.where(p >= q, 1, -1)
        for signs in (toward, -toward, toward * np.array([1, -1, 1])):
            calls.append((qi, q.copy(), (signs * half).astype(F), tuple(dims)))
    return calls


# ---- the marching-cubes scene -----------------------------------------------------------------------------------------------------
MC_DIMS = (16, 15, 14)
MC_SEED = 2  # (of the seeds 1 .. 6, the seeds 2, 3 and 6 give all 256 cases at these dims; 1 and 4 give 255, 5 gives 254)
MC_BOX_IN_H = 22.0


def mc_lattice(cfg):
    """(origin, spacing, dims) of the scene's lattice: origin + (float)i * (1.25 h) per axis."""
    h = F(cfg.h)
    L = F(F(1.25) * h)
    return np.array([F(1.5) * h] * 3, F), np.array([L, L, L], F), MC_DIMS


def mc_scene(jitter):
    """A wide-mode box of 11 cells per axis without boundary shell or liquid lattice: a lone liquid particle on every point of
    mc_lattice that a seeded pattern selects (occupancy 0.5, the lattice's border layer empty), moved by jitter * h * U(-0.5, 0.5)
    per axis. Lattice points are 1.25 h apart, so a particle is more than 1.03 h from every other one (no neighbours: its density
    is the clamp) and more than h from every foreign lattice point: the sampled field at a lattice point is 0 or its own particle's.
    The dict of scenes.liquid_box plus "pattern": bool[nz, ny, nx]. vx is 0 for one particle in eight and of both signs otherwise."""
    key = ("mc", float(jitter))
    if key in _cache:
        sc = _cache[key]
        return dict(sc, cfg=type(sc["cfg"]).from_buffer_copy(sc["cfg"]))
    cfg = scenes.liquid_box_config((MC_BOX_IN_H,) * 3, mask=0xffffffff)
    origin, spacing, (nx, ny, nz) = mc_lattice(cfg)
    rng = np.random.default_rng(MC_SEED)
    pattern = rng.random((nz, ny, nx)) < 0.5
    pattern[0], pattern[-1], pattern[:, 0], pattern[:, -1], pattern[:, :, 0], pattern[:, :, -1] = (False,) * 6
    shift = rng.uniform(-0.5, 0.5, (nz, ny, nx, 3))
    vx = rng.uniform(-2e-3, 2e-3, (nz, ny, nx))
    vx[rng.random((nz, ny, nx)) < 0.125] = 0.0
    g = sample_ref.grid_points(origin, spacing, (nx, ny, nz))
    kk, jj, ii = np.nonzero(pattern)
    n = kk.size
    pos = np.zeros((n, 4), F)
    pos[:, :3] = g[kk, jj, ii]
    if jitter:
        pos[:, :3] += (F(jitter) * F(cfg.h) * shift[kk, jj, ii]).astype(F)
    pos[:, 3] = LIQUID
    vel = np.zeros((n, 4), F)
    vel[:, 0] = vx[kk, jj, ii]
    vel[:, 1] = F(1e-3)
    vel[:, 2] = F(-5e-4)
    cfg.particleCount = n
    _cache[key] = dict(cfg=cfg, position=pos, velocity=vel, elastic=None, membranes=None, particle_membranes=None, numOfLiquidP=n,
                       numOfElasticP=0, numOfBoundaryP=0, pattern=pattern)
    return mc_scene(jitter)


def mc_small_lattices(cfg):
    """{name: (origin, spacing, dims)} of lattices over the scene whose point counts lie at the edges of a 256-thread block (255, 256,
    258), and that are two points thick along one, two and three axes; "empty" lies in the lattice's empty border layer."""
    h = F(cfg.h)
    o, L, _ = mc_lattice(cfg)
    s = np.array([F(0.4) * h] * 3, F)
    inside = (o + F(1.9) * L[0]).astype(F)  # just below the lattice points (2, 2, 2): the second layer holds particles
    return {
        "255": (inside, s, (3, 5, 17)),
        "256": (inside, s, (2, 2, 64)),
        "258": (inside, s, (2, 3, 43)),
        "thin x": (inside, s, (2, 21, 19)),
        "thin xy": (inside, np.array([F(0.4) * h, F(0.45) * h, F(0.3) * h], F), (2, 2, 37)),
        "thin xyz": ((o + F(1.6) * L[0]).astype(F), np.array([F(0.6) * h] * 3, F), (2, 2, 2)),
        "empty": ((o - F(0.2) * L[0]).astype(F), np.array([F(0.1) * h] * 3, F), (2, 2, 2)),
    }


def r0_shepard(k):
    """Word 1 of the record at a lone particle's own position: (float)massWpoly6 * (hs6 * (1/rho)) with rho the clamp
    (float)(hs6 * massWpoly6) — three roundings, two ulps below 1 with the scenes' constants."""
    return F(F(k.massWpoly6) * F(k.hs6 * k.inv_rho))


def cases_of(inside):
    """The marching-cubes case of every cell of an inside / outside map bool[nz, ny, nx] (include/sphmi.h: corner c at
    (i + (c&1), j + ((c>>1)&1), k + (c>>2)))."""
    ins = np.asarray(inside).astype(np.int64)
    nz, ny, nx = ins.shape
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        case |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] << c
    return case


def edge_parameters(f, iso):
    """t = (iso - f0) / (f1 - f0) of every crossed lattice edge in the contract's vertex order (the edge's lower point x fastest,
    within a point +x, +y, +z), float32."""
    f = np.asarray(f, F)
    iso = F(iso)
    ins = f >= iso
    idx = np.arange(f.size).reshape(f.shape)
    lower = (np.s_[:, :, :-1], np.s_[:, :-1, :], np.s_[:-1, :, :])
    upper = (np.s_[:, :, 1:], np.s_[:, 1:, :], np.s_[1:, :, :])
    point, axes, ts = [], [], []
    for axis in range(3):
        m = ins[lower[axis]] != ins[upper[axis]]
        f0, f1 = f[lower[axis]][m], f[upper[axis]][m]
        ts.append(((iso - f0) / (f1 - f0)).astype(F))
        point.append(idx[lower[axis]][m])
        axes.append(np.full(f0.size, axis))
    point, axes, ts = np.concatenate(point), np.concatenate(axes), np.concatenate(ts)
    return ts[np.lexsort((axes, point))]


def zero_area(verts, tris):
    """Number of triangles whose area is exactly 0 (the cross product of two edges, exact in float64 for float32 corners whose
    differences are small, vanishes)."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    if t.size == 0:
        return 0
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return int((n == 0).all(1).sum())


def mc_iso_point(pattern):
    """(k, j, i) of the first occupied lattice point (x fastest) that has an empty neighbour below it and one above it along some
    axes: with iso equal to the field there, edges with t = 0 and with t = 1 meet in it."""
    p = np.asarray(pattern, bool)
    for k, j, i in zip(*np.nonzero(p)):
        lo = (not p[k, j, i - 1]) or (not p[k, j - 1, i]) or (not p[k - 1, j, i])
        hi = (not p[k, j, i + 1]) or (not p[k, j + 1, i]) or (not p[k + 1, j, i])
        if lo and hi:
            return int(k), int(j), int(i)
    raise AssertionError("no such lattice point")


def degenerate_counts(f, origin, spacing, iso, verts, tris):
    """(vertices with t == 0, vertices with t == 1, vertices that lie on a lattice point bit for bit, zero-area triangles)."""
    t = edge_parameters(f, iso)
    assert t.shape[0] == np.asarray(verts).shape[0]
    dims = (f.shape[2], f.shape[1], f.shape[0])
    pts = np.ascontiguousarray(sample_ref.grid_points(origin, spacing, dims).reshape(-1, 3))
    lattice = set(map(bytes, pts.view(np.uint8).reshape(-1, 12)))
    on = sum(bytes(x) in lattice for x in np.ascontiguousarray(verts, F).view(np.uint8).reshape(-1, 12))
    return int((t == 0).sum()), int((t == 1).sum()), int(on), zero_area(verts, tris)


# the curves traced from the ring's queries: a few steps, each a few hundred times the width of the subnormal ring
TRACE_MAX_STEPS = 3
TRACE_STEPS = {0: lambda k: F(40.0),           # mode "time": step * |u|, |u| about 3e-3: 0.04 h
               1: lambda k: F(0.02) * k.h}     # mode "arc": chords of 0.02 h
