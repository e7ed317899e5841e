"""Scenes that carry the analysis kernels which walk the neighbour rows of the last step (the force decomposition of
csrc/sph_forces.hip, the diffusion of sph_fields.hip, the surface measure and the row terms of sph_select.hip, the link test of
sph_components.hip, the histogram of sph_diag.hip) to the states where they can break: isolated pairs whose stored
distance is the last float below closeRf or below hs and ulps around it, pairs listed in a row beyond hs, (liquid, lone wall
particle) pairs, particles with an empty row, a particle whose key is the first that is not a cell; a dense block in which the close-range branch meets non-zero pressures and full
rows; coincident particles (r == 0). Inputs only: nothing here calls the library's solver. The oracle's state after one step is
computed once per scene and shared by the tests."""
import numpy as np

import forces_ref as fr
import scenes
from band_cases import F, INF, LIQUID, _Placer, first_in_cell, last_in_cell, ulp_steps
from sample_cases import last_true

BOUNDARY = F(3.1)
OFFSETS = (0, -1, -2, -8, 1, 2, 8)  # ulps of Q's coordinate from the last one whose stored distance is below the threshold; > 0: farther
DIRECTIONS = ("axis", "face diagonal", "body diagonal")
SEPARATION_IN_H = 2.1    # between the particles of different clusters
SHELL_MARGIN_IN_H = 1.04  # between a placed particle and the shell's layer: beyond the search's 31 h / 30
NORMALS = np.array([[1, 0, 0], [0, -1, 0], [0.70710677, 0, 0.70710677], [0.57735026, -0.57735026, 0.57735026], [0, 0.70710677, -0.70710677]], F)
_cache = {}


class Constants:
    """The floats of the row contracts as the step computes them (forces_ref.constants) and the thresholds in scene units."""

    def __init__(self, cfg):
        self.K = fr.constants(cfg)
        self.h = F(cfg.h)
        self.ss, self.hs, self.closeRf = self.K["simScale"], self.K["hs"], self.K["closeRf"]
        self.reach = {"close": float(self.closeRf) / float(self.ss), "hs": float(self.h)}
        self.limit = {"close": self.closeRf, "hs": self.hs}


def stored(k, p, q):
    """The distance the search stores for the pair and K12 recomputes: sqrtf(dx*dx + dy*dy + dz*dz) * simulationScale."""
    e = (np.asarray(p, F) - np.asarray(q, F)).astype(F)
    d2 = F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))
    return F(np.sqrt(d2) * k.ss)


def _line(direction, number):
    """(long axis, away, {other axis: share of the reach}) of pair `number` along one of DIRECTIONS: the long axis and the signs
    rotate with the number, so that every axis and both signs are met."""
    a, sg = number % 3, (1 if (number // 3) % 2 == 0 else -1)
    b, c = (a + 1) % 3, (a + 2) % 3
    return (a, sg, {}) if direction == 0 else (a, sg, {b: -0.6 * sg}) if direction == 1 else (a, -sg, {b: 0.5 * sg, c: -0.5})


def pair_list():
    """(kind, offset, direction, Q is a lone wall particle) of the pairs of pair_scene: the box has room for about fourteen
    pairs of length h at the separation the scenes keep, so each offset of the hs threshold goes along one direction (0 and +1
    along the same one), the offsets 0 and +1 of the closeRf threshold along all three. A third of the pairs have a wall particle."""
    hs_dir = {0: 0, 1: 0, -1: 1, 2: 1, -2: 2, 8: 2, -8: 0}
    out = [("hs", off, hs_dir[off], off in (-1, 2, -8)) for off in OFFSETS]
    for off in (0, 1):
        out += [("close", off, d, d == 1) for d in range(3)]
    out += [("close", off, n % 3, n % 3 == 2) for n, off in enumerate(o for o in OFFSETS if o not in (0, 1))]
    out += [("far", 0, 0, False), ("far", 0, 0, True), ("far", 0, 2, False), ("half", 0, 1, False)]
    return out


def _q_of(k, p, kind, off, direction, number, nominal=False):
    """Q of a pair whose P lies at p (nominal: at the threshold's nominal distance, without the search, for the placement)."""
    axis, away, shares = _line(direction, number)
    reach = k.reach["close" if kind == "close" else "hs"]
    q = np.array(p, F)
    t = {"far": 1.02, "half": 0.5, "hs": 1.0, "close": 1.0}[kind]
    for b, s in shares.items():
        q[b] = F(p[b] + F(s * t * reach))
    if kind in ("close", "hs") and not nominal:
        c = last_true(lambda x: stored(k, p, x) < k.limit[kind], p, q, axis, away, 1.1 * reach)
        q[axis] = ulp_steps(c, off * away)
    else:
        side = np.sqrt(1.0 - sum(s * s for s in shares.values()))
        q[axis] = F(p[axis] + F(away * side * t * reach))
    return q


def _grid(cfg, pitch_in_h=0.3):
    lo = 0.5 * float(cfg.r0) + SHELL_MARGIN_IN_H * float(cfg.h)
    return [F(v) for v in np.arange(lo, float(cfg.xmax) - lo, pitch_in_h * float(cfg.h))], lo


def _cluster_sites(cfg, offsets):
    """Every placement of a cluster (its first particle on a grid point, the others at the given offsets) inside the shell margin."""
    grid, lo = _grid(cfg)
    hi = float(cfg.xmax) - lo
    offsets = np.asarray(offsets, F).reshape(-1, 3)
    for z in grid:
        for y in grid:
            for x in grid:
                pts = (np.array([x, y, z], F) + offsets).astype(F)
                if pts.min() >= lo and pts.max() <= hi:
                    yield pts


def _one_sided_sites(cfg, k, q0, axis, away):
    """The placements of a pair along an axis, longer than h, that only Q's search finds: the reference searches the cells on the
    near side of the particle's half cell, so P, 0.99 h from the face of its cell that lies away from Q, does not look into Q's cell,
    while Q, just across the face, looks into P's."""
    for c in (1, 2):
        t = F(first_in_cell(cfg, c) + F(0.99) * k.h) if away > 0 else F(first_in_cell(cfg, c + 1) - F(0.99) * k.h)
        for pts in _cluster_sites(cfg, [np.zeros(3, F), q0]):
            shift = F(t - pts[0, axis])
            if abs(shift) < 0.3 * float(k.h):  # (the grid point next to t)
                pts = pts.copy()
                pts[:, axis] += shift
                yield pts


def _assemble(base, liquid, walls, extra):
    """The scene dict: the placed liquid (positions float32[n, 3]) first, then the lone wall particles, then the shell of `base`."""
    cfg = base["cfg"]
    nl0 = base["numOfLiquidP"]
    n, nw = len(liquid), len(walls)
    pos = np.zeros((n + nw, 4), F)
    vel = np.zeros((n + nw, 4), F)
    pos[:n, :3], pos[:n, 3] = np.array(liquid, F).reshape(n, 3), LIQUID
    for i in range(n):
        vel[i, :3] = np.array([1.5e-3, -2.5e-3, 0.75e-3], F) * F(1.0 + 0.0078125 * i) * F(1 if i % 2 == 0 else -1)
    if nw:
        pos[n:, :3], pos[n:, 3] = np.array(walls, F).reshape(nw, 3), BOUNDARY
        vel[n:, :3], vel[n:, 3] = NORMALS[np.arange(nw) % len(NORMALS)], BOUNDARY
    pos = np.concatenate([pos, base["position"][nl0:]]).astype(F)
    vel = np.concatenate([vel, base["velocity"][nl0:]]).astype(F)
    cfg.particleCount = pos.shape[0]
    return dict(base, cfg=cfg, position=pos, velocity=vel, numOfLiquidP=n, numOfBoundaryP=base["numOfBoundaryP"] + nw, walls=nw, **extra)


def _copy(sc):
    return dict(sc, cfg=type(sc["cfg"]).from_buffer_copy(sc["cfg"]))


def pair_scene():
    """The `tiny` box and its boundary shell with the liquid replaced by isolated pairs (P, Q), lone liquid particles, and two
    liquid particles far outside the box whose z is the last float of cell layer 8 (the key is a cell) and the first float of
    layer 9 (the key is gridCellCount or more: not a cell). The dict of scenes.liquid_box plus
    "pairs": [(kind, offset, direction, Q is a wall particle, id of P, id of Q)], "lone": ids, "stray": id, "control": id."""
    if "pair" in _cache:
        return _copy(_cache["pair"])
    base = scenes.SCENES["tiny"]()
    cfg = base["cfg"]
    assert cfg.cellIdMask == 0xffff
    k = Constants(cfg)
    placer = _Placer(SEPARATION_IN_H * float(k.h))
    liquid, walls, pairs = [], [], []
    order = sorted(enumerate(pair_list()), key=lambda e: {"far": 0, "hs": 1, "half": 2, "close": 3}[e[1][0]])  # the long ones first
    placed = {}
    for number, (kind, off, direction, wall) in order:
        ten = np.full(3, 10, F)
        q0 = _q_of(k, ten, kind, off, direction, number, nominal=True) - ten
        sites = _cluster_sites(cfg, [np.zeros(3, F), q0])
        if kind == "far" and direction == 0:
            sites = _one_sided_sites(cfg, k, q0, *_line(direction, number)[:2])
        _, pts = placer.place(sites, "pair %s %+d %s" % (kind, off, DIRECTIONS[direction]))
        p = pts[0]
        q = _q_of(k, p, kind, off, direction, number)
        assert np.abs(q - pts[1]).max() < 0.3 * float(k.h)
        placed[number] = (p, q)
    for number, (kind, off, direction, wall) in enumerate(pair_list()):
        p, q = placed[number]
        liquid.append(p)
        if wall:
            walls.append(q)
            pairs.append((kind, off, direction, True, len(liquid) - 1, ("wall", len(walls) - 1)))
        else:
            liquid.append(q)
            pairs.append((kind, off, direction, False, len(liquid) - 2, len(liquid) - 1))
    lone = []
    for n in range(3):
        _, pts = placer.place(_cluster_sites(cfg, [np.zeros(3, F)]), "lone particle")
        liquid.append(pts[0])
        lone.append(len(liquid) - 1)
    mid = F(0.5) * F(cfg.xmax)
    liquid.append(np.array([mid, F(mid - F(3) * k.h), last_in_cell(cfg, cfg.gridCellsZ - 1)], F))
    control = len(liquid) - 1
    liquid.append(np.array([F(mid + F(3) * k.h), mid, first_in_cell(cfg, cfg.gridCellsZ)], F))
    stray = len(liquid) - 1
    n = len(liquid)
    pairs = [(kd, o, d, w, ip, (n + iq[1]) if w else iq) for kd, o, d, w, ip, iq in pairs]
    _cache["pair"] = _assemble(base, liquid, walls, dict(pairs=pairs, lone=lone, stray=stray, control=control))
    return pair_scene()


BLOCK_SIDE = 5
BLOCK_SEED = 20261021


def block_scene(side):
    """The `tiny` box and its shell with a 5 x 5 x 5 liquid block of spacing 0.5 r0 and 0.02 r0 seeded jitter at (4 h, 4 h, 4 h):
    after ONE step (a second one blows up) every pressure is positive, rows are full, and hundreds of slots are closer than
    closeRf. One pair of x neighbours in the block's middle is nudged along x so that its stored distance is the last float below
    closeRf (side "in") or the first float not below it ("out"). The dict of scenes.liquid_box plus "pair": (id of P, id of Q)."""
    assert side in ("in", "out")
    if ("block", side) in _cache:
        return _copy(_cache["block", side])
    base = scenes.SCENES["tiny"]()
    cfg = base["cfg"]
    k = Constants(cfg)
    r0 = float(cfg.r0)
    rng = np.random.default_rng(BLOCK_SEED)
    g = np.arange(BLOCK_SIDE) * 0.5 * r0
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    pts = np.stack([xx, yy, zz], -1).reshape(-1, 3) + 4.0 * float(k.h) + rng.uniform(-0.02 * r0, 0.02 * r0, (BLOCK_SIDE ** 3, 3))
    pts = pts.astype(F)
    c = BLOCK_SIDE // 2
    ip = (c * BLOCK_SIDE + c) * BLOCK_SIDE + c
    iq = ip + 1
    p, q = pts[ip], pts[iq].copy()
    q[0] = p[0]
    x = last_true(lambda v: stored(k, p, v) < k.closeRf, p, q, 0, 1, 0.4 * float(k.h))
    pts[iq, 0] = x if side == "in" else np.nextafter(x, INF)
    _cache["block", side] = _assemble(base, list(pts), [], dict(pair=(ip, iq)))
    return block_scene(side)


def coincident_scene():
    """pair_scene's placement with coincident particles (r == 0): two liquid pairs, a liquid particle on a lone wall particle and a
    liquid triple, next to an ordinary pair at h / 2 and a lone particle. The dict of scenes.liquid_box plus "clusters":
    [(name, ids)]."""
    if "coincident" in _cache:
        return _copy(_cache["coincident"])
    base = scenes.SCENES["tiny"]()
    cfg = base["cfg"]
    k = Constants(cfg)
    placer = _Placer(SEPARATION_IN_H * float(k.h))
    liquid, walls, clusters = [], [], []
    zero = np.zeros(3, F)
    half = np.array([0.5 * float(k.h), 0, 0], F)
    for name, offsets, wall in (("pair", [zero, zero], False), ("pair", [zero, zero], False), ("wall pair", [zero, zero], True),
                                ("triple", [zero, zero, zero], False), ("half", [zero, half], False), ("lone", [zero], False)):
        _, pts = placer.place(_cluster_sites(cfg, offsets), name)
        ids = []
        for m, pt in enumerate(pts):
            if wall and m == 1:
                walls.append(pt)
                ids.append(("wall", len(walls) - 1))
            else:
                liquid.append(pt)
                ids.append(len(liquid) - 1)
        clusters.append((name, ids))
    n = len(liquid)
    clusters = [(name, [n + i[1] if isinstance(i, tuple) else i for i in ids]) for name, ids in clusters]
    _cache["coincident"] = _assemble(base, liquid, walls, dict(clusters=clusters))
    return coincident_scene()


SCENES = {"pair": pair_scene, "block_in": lambda: block_scene("in"), "block_out": lambda: block_scene("out"), "coincident": coincident_scene}
_oracle = {}


def oracle_step0(name):
    """(state, ids, dist, acceleration float32[2 N, 4]) of forces_ref.oracle_state plus "ids" (the original id of every sorted
    particle) after the oracle's first step of SCENES[name]: computed once, shared, never changed."""
    if name not in _oracle:
        sc = SCENES[name]()
        cfg = sc["cfg"]
        N = cfg.particleCount
        ora = scenes.oracle_for(sc, threads=8)
        ora.step()
        state, ids, dist = fr.oracle_state(ora, N, cfg.gridCellCount)
        state["ids"] = ora.buffer("particleIndex").reshape(-1, 2)[:N, 1].astype(np.int64)
        state["h"], state["simScale"] = float(cfg.h), float(cfg.simulationScale)
        acc = ora.buffer("acceleration").reshape(-1, 4)[:2 * N].copy()
        ora.close()
        _oracle[name] = (state, ids, dist, acc)
    return _oracle[name]


def sorted_of(state):
    """int64[N]: the sorted index of every original id."""
    back = np.empty(state["ids"].shape[0], np.int64)
    back[state["ids"]] = np.arange(back.size)
    return back


def slot_of(ids, i, j):
    """The slot of row i that names j, or -1."""
    at = np.flatnonzero(np.asarray(ids)[i] == j)
    return int(at[0]) if at.size else -1


def pair_slots(sc, state, ids, dist):
    """Per pair of pair_scene: (kind, offset, direction, wall, sorted P, sorted Q, slot of Q in P's row, slot of P in Q's row)."""
    back = sorted_of(state)
    out = []
    for kind, off, direction, wall, ip, iq in sc["pairs"]:
        sp, sq = int(back[ip]), int(back[iq])
        out.append((kind, off, direction, wall, sp, sq, slot_of(ids, sp, sq), slot_of(ids, sq, sp)))
    return out


def assert_pair_states(sc, state, ids, dist):
    """What pair_scene claims, on a set of rows (the oracle's in the CPU test; a device test hands it the device's): every pair's
    particles have each other and nobody else in reach; the stored distance is below the threshold for the offsets <= 0 and not
    below it for the offsets > 0, on both rows; the far pairs are stored beyond hs, at least one in one row only; the lone
    particles, the stray and the control have empty rows; the stray's key is not a cell, the control's and every other one is.
    Returns the counts {(kind, offset): pairs}."""
    cfg = sc["cfg"]
    k = Constants(cfg)
    ids, dist = np.asarray(ids), np.asarray(dist)
    back = sorted_of(state)
    n_placed = sc["numOfLiquidP"] + sc["walls"]
    placed = back[:n_placed]
    counts, asymmetric = {}, 0
    seen = np.zeros(ids.shape[0], bool)
    for kind, off, direction, wall, sp, sq, a, b in pair_slots(sc, state, ids, dist):
        want = stored(k, state["pos"][sp], state["pos"][sq])
        for i, j, slot in ((sp, sq, a), (sq, sp, b)):
            others = ids[i][(ids[i] >= 0) & (ids[i] != j)]
            assert others.size == 0, (kind, off, DIRECTIONS[direction], "a third particle in the row", others)
            if slot >= 0:
                assert dist[i, slot].view(np.uint32) == want.view(np.uint32), (kind, off, dist[i, slot], want)
            seen[i] = True
        if kind in ("close", "hs"):
            assert a >= 0 and b >= 0, (kind, off, DIRECTIONS[direction])
            assert (want < k.limit[kind]) == (off <= 0), (kind, off, DIRECTIONS[direction], want)
            if kind == "close":
                assert want < k.hs
        elif kind == "half":
            assert a >= 0 and b >= 0 and k.closeRf < want < k.hs
        else:
            assert a >= 0 or b >= 0
            assert want >= k.hs
            asymmetric += (a >= 0) != (b >= 0)
        counts[kind, off] = counts.get((kind, off), 0) + 1
    assert asymmetric >= 1
    back_lone = [int(back[i]) for i in sc["lone"] + [sc["stray"], sc["control"]]]
    assert not (ids[back_lone] >= 0).any()
    seen[back_lone] = True
    assert seen[placed].all() and int(seen.sum()) == n_placed
    keys = np.asarray(state["keys"]).astype(np.int64)
    assert keys[back[sc["stray"]]] >= cfg.gridCellCount > keys[back[sc["control"]]] and (np.delete(keys, back[sc["stray"]]) < cfg.gridCellCount).all()
    return counts


def expected_pair_counts():
    out = {}
    for kind, off, _, _ in pair_list():
        out[kind, off] = out.get((kind, off), 0) + 1
    return out


def block_pair(sc, state, ids, dist):
    """(sorted P, sorted Q, slot of Q in P's row, slot of P in Q's row, stored distance) of block_scene's nudged pair."""
    back = sorted_of(state)
    sp, sq = int(back[sc["pair"][0]]), int(back[sc["pair"][1]])
    return sp, sq, slot_of(ids, sp, sq), slot_of(ids, sq, sp), stored(Constants(sc["cfg"]), state["pos"][sp], state["pos"][sq])


def assert_block_states(sc, side, state, ids, dist):
    """What block_scene claims on a set of rows and a state: positive pressure on every block particle, slots on both sides of
    closeRf, full rows, finite positions, and the nudged pair in both rows at the last float below closeRf / the first not below."""
    k = Constants(sc["cfg"])
    ids, dist = np.asarray(ids), np.asarray(dist)
    back = sorted_of(state)
    block = back[:sc["numOfLiquidP"]]
    assert block.size == BLOCK_SIDE ** 3 and (state["p"][block] > 0).all() and np.isfinite(state["pos"]).all()
    rows, d = ids[block], dist[block]
    valid = rows >= 0
    assert ((d < k.closeRf) & valid).sum() > 0 and ((d >= k.closeRf) & (d < k.hs) & valid).sum() > 0
    assert (valid.sum(1) == 32).sum() > 0
    sp, sq, a, b, want = block_pair(sc, state, ids, dist)
    assert a >= 0 and b >= 0 and dist[sp, a].view(np.uint32) == want.view(np.uint32) == dist[sq, b].view(np.uint32)
    assert (want < k.closeRf) == (side == "in") and abs(float(want) - float(k.closeRf)) < 1e-6 * float(k.closeRf), (side, want, k.closeRf)
    return int(((d < k.closeRf) & valid).sum()), int(((d >= k.closeRf) & (d < k.hs) & valid).sum()), int((valid.sum(1) == 32).sum())


# ---- what the scenes are asked, built from a state and its rows ---------------------------------------------------------------------
FLT_MAX = F(np.finfo(np.float32).max)
TINY = F(np.finfo(np.float32).tiny)
SUBNORMAL = F(1e-42)
MASKS = [(1,), (1, 2), (1, 2, 3)]


def find_pair(sc, kind, off, direction):
    """(id of P, id of Q, Q is a wall particle) of the first such pair of pair_scene."""
    for kd, o, d, wall, ip, iq in sc["pairs"]:
        if (kd, o, d) == (kind, off, direction):
            return ip, iq, wall
    raise KeyError((kind, off, direction))


def extreme_field(sc, base):
    """A field of pair_scene in original-id order, finite values only: `base` with +-FLT_MAX on the two ends of a close pair and
    of a (liquid, wall) pair (the difference overflows), 2^127 next to 0 on the pair at h / 2 (with power_coefficient the first
    substep's a * S overflows, and the second meets inf - inf), the smallest normal next to a subnormal on the pair at the last
    distance below hs, and -0.0 next to +0.0. Returns (values, {name: (id, id)})."""
    v = np.asarray(base, F).copy()
    roles = {}
    for name, key, a, b in (("overflow", ("close", 0, 0), FLT_MAX, -FLT_MAX), ("overflow wall", ("close", 0, 1), FLT_MAX, -FLT_MAX),
                            ("power", ("half", 0, 1), F(2.0) ** 127, F(0)), ("tiny", ("hs", 0, 0), TINY, SUBNORMAL),
                            ("minus zero", ("close", -1, 0), F(-0.0), F(0.0))):
        ip, iq, wall = find_pair(sc, *key)
        assert wall == (name == "overflow wall")
        v[ip], v[iq] = a, b
        roles[name] = (ip, iq)
    assert np.isfinite(v).all()
    return v, roles


def power_coefficient(D, state, roles):
    """The coefficient with a_i * W_i = 4 on the "power" pair (fields_ref.Diffusion D of the state): a_i * S_i = -4 * 2^127."""
    i = int(sorted_of(state)[roles["power"][0]])
    return F(4.0 / (float(D.sD[i]) * float(D.W[i])))


def field_nan_ids(sc, state, roles, types, substeps):
    """The original ids whose value is NaN after `substeps` substeps of extreme_field with power_coefficient: from the second
    substep on, the participating ends of the pairs whose first substep overflowed, where both ends participate."""
    if substeps < 2:
        return []
    out = []
    for name in ("overflow", "overflow wall", "power"):
        ends = roles[name]
        kinds = [1 if i < sc["numOfLiquidP"] else 3 for i in ends]
        if all(t in types for t in kinds):
            out += list(ends)
    return sorted(out)


def force_nan_words(sc, state):
    """bool[N, 40]: the words of the force records of coincident_scene that are NaN: on a liquid particle that coincides with
    another, the pressure words of the classes of the particles it coincides with and the words 33..35 (tq = 0 / 0)."""
    back = sorted_of(state)
    out = np.zeros((back.size, 40), bool)
    nl = sc["numOfLiquidP"]
    for name, ids in sc["clusters"]:
        if name not in ("pair", "wall pair", "triple"):
            continue
        for i in ids:
            if i >= nl:
                continue  # the wall particle's record is all zero
            for j in ids:
                if j != i:
                    c = 1 if j < nl else 3
                    out[back[i], 9 * (c - 1) + 6:9 * (c - 1) + 9] = True
            out[back[i], 33:36] = True
    return out


def same_bits_or_nan(got, want):
    """bool array: the two words are bit-identical, or both are NaN (a NaN's sign and payload are not part of a contract)."""
    got, want = np.asarray(got), np.asarray(want)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(view) == np.ascontiguousarray(want).view(view)) | (np.isnan(got) & np.isnan(want))


def clamp_case(values):
    """(lo, hi, bins, q): q < hi, yet (q - lo) * scale reaches `bins` in float, so that the clamp min(., bins - 1) decides the bin."""
    for q in np.asarray(values, F):
        hi = np.nextafter(q, INF)
        for lo in (F(-3.0e5), F(-1.0e6), F(-77777.0)):
            for bins in range(2, 4097):
                scale = F(bins) / F(hi - lo)
                if F(F(q - lo) * scale) >= bins:
                    return lo, hi, bins, q
    raise AssertionError("no clamp case")
