"""Hand-made scenes and views that put the two renderers (sph_render_particles, sph_render_mesh) into their edge states: inputs
only, no solver. tests/test_render_edges_host.py shows on the CPU, with the oracle's state and the restatements alone, that every
case meets the condition it exists for; tests/test_render_edges.py then draws them on the device. What both assert about a case's
images is in tests/render_edge_checks.py.

Everything is dyadic. The sorted state a render reads after one step is the state the step started from, so a hand-placed
particle reaches the kernels bit for bit; the views look along +z with right = +x and up = +y, scales are powers of two and
the centres multiples of 1/2, so every projection below is exact in float32 and an intended equality is an equality.

Known uncovered states (see tests/test_render_edges.py): smooth shading, the density colour thresholds, thickness saturation."""
from collections import namedtuple

import numpy as np

import scenes
import sphmi

f32 = np.float32
# k_render_drain / k_rm_drain run RN_DRAIN_BLOCKS (RM_DRAIN_BLOCKS) = 1024 blocks of SPH_BLOCK = 256 lanes, one wave of 64 per
# queued item: 1024 * 256 / 64 waves. The bindings do not expose the constants.
DRAIN_WAVES = 4096
LABEL_COLOURS = 12  # SPH_RENDER_LABEL_COLOURS
LIMIT = 1048576.0   # |u|, |v| < 2^20

SplatCase = namedtuple("SplatCase", "name why view types region thickness label")
TriCase = namedtuple("TriCase", "name why view field bounds compose")


def below(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def make_view(width, height, centre, eye=(0.0, 0.0, 0.0), scale=8.0, radius=0.375, near=0.0, max_px=4096.0, perspective=False, mode=0,
              field=0, lo=0.0, hi=1.0, back=False):
    """Looking along +z from `eye`: u = (x - eye.x) k + centre.x, v = centre.y - (y - eye.y) k, cz = z - eye.z. `back`: along -z
    with the same right and up (a mirror image), cz = eye.z - z."""
    v = sphmi.SphRenderView()
    v.width, v.height, v.projection = width, height, 1 if perspective else 0
    for k, (r, u, f) in enumerate(zip((1, 0, 0), (0, 1, 0), (0, 0, -1 if back else 1))):
        v.eye[k], v.right[k], v.up[k], v.forward[k] = eye[k], r, u, f
    v.scale = scale
    v.centre[0], v.centre[1] = centre
    v.nearPlane, v.radius, v.maxRadiusPx = near, radius, max_px
    v.colourMode, v.field, v.lo, v.hi = mode, field, lo, hi
    for t, c in enumerate(((0.2, 0.4, 1.0), (1.0, 0.5, 0.0), (0.5, 0.5, 0.5))):
        for k in range(3):
            v.typeColour[t][k] = c[k]
    v.ambient = 0.25
    for k, b in enumerate((1, 2, 3, 4)):
        v.background[k] = b
    return v


def _scene(cfg, pos, elastic=None, membranes=None, pml=None, E=0):
    pos = np.asarray(pos, np.float32).reshape(-1, 4)
    cfg.particleCount = pos.shape[0]
    if membranes is not None:
        cfg.numOfElasticP, cfg.numOfMembranes, cfg.elasticOffset = E, int(membranes.shape[0]), 0
    lo = pos[:, :3].min(0)
    hi = pos[:, :3].max(0)
    assert (lo > 0.5).all() and (hi < np.array([cfg.xmax, cfg.ymax, cfg.zmax]) - 0.5).all(), (lo, hi)  # inside the box
    return dict(cfg=cfg, position=pos, velocity=np.zeros_like(pos), elastic=elastic, membranes=membranes, particle_membranes=pml)


# ---- particles ---------------------------------------------------------------------------------------------------------------
# The frame of the splat scene: a 131 x 67 image at 8 pixels per unit in which the particle P(c, d) has u = c + 0.5, v = d + 0.5
SW, SH = 131, 67
S_CENTRE = (0.5 - 16.0, SH - 0.5 + 16.0)
S_RADIUS = 0.375  # R = 3 pixels: the search box of a sphere on a pixel centre is 9 x 9 pixels (x1 - x0 == 8: queued)
# Box sizes are in pixels throughout: a side of 8 (x1 - x0 == 7) is the lane's, a side of 9 (x1 - x0 == 8) is queued.


def _P(c, d, z, t=1.1):
    return (2.0 + c / 8.0, 2.0 + (SH - 1 - d) / 8.0, z, t)


def splat_scene():
    """(scene, who): 104 particles (one whole wave and a partial one). `who` names original ids."""
    pts, who = [], {}

    def add(name, *p):
        who[name] = len(pts)
        pts.append(_P(*p))
    add("interior", 20, 20, 10.0)       # unclipped: 9 x 9, queued; (23, 20) lies at d2 == R2
    add("left", 3, 20, 11.0)            # x0 clipped from -1 to 0: 8 x 9, queued by y alone
    add("right", SW - 4, 20, 11.0)      # x1 clipped from 131 to 130
    add("top", 40, 3, 11.0)             # 9 x 8, queued by x alone
    add("bottom", 40, SH - 4, 11.0)
    add("corner_tl", 3, 3, 11.0)        # 8 x 8: the lane rasterises it
    add("corner_br", SW - 4, SH - 4, 11.0)
    add("edge_deep", 1, 44, 11.0)       # clipped by three columns: 6 x 9
    add("sub_x", 60.25, 20, 11.0)       # a quarter pixel off the centre: with R = 2.75 the boxes are 8 x 9, 9 x 8 and 8 x 8
    add("sub_y", 70, 20.25, 11.0)
    add("sub_xy", 80.25, 20.25, 11.0)
    add("off_image", SW + 20, 30, 11.0, 3.1)   # drawn, covers nothing
    add("far_above", 128, 40, 11.0)     # x = 18: with the eye at x = -131054, u = 2^20 + 0.5
    add("far_below", 127, 50, 11.0)     # x = 17.875: u = 2^20 - 0.5
    add("near_eq", 60, 50, 0.625)                       # perspective, nearPlane 0.625: cz == nearPlane
    add("near_3ulp", 70, 50, float(f32(1.0) + f32(3 * 2.0 ** -23)))  # perspective: R one rounding step above maxRadiusPx
    add("near_4ulp", 80, 50, float(f32(1.0) + f32(4 * 2.0 ** -23)))  # R == maxRadiusPx
    for k in range(14):                 # x = 3 .. 16, z = 6 .. 19: the ramp's q < lo, == lo, knots, == hi, > hi; labels 0 .. 12+
        add("row%d" % k, 8 + 8 * k, 34, 6.0 + k)
    for k in range(6):                  # y = 8 .. 3 at x = 17: boundary particles (label -1 when only liquid is labelled)
        add("col%d" % k, 120, 18 + 8 * k, 12.0, 3.1)
    for k in range(3):                  # the highest cells: the end of the sorted order
        add("last%d" % k, 30 + 10 * k, 50, 24.0)
    for k in range(4):                  # a whole wave's worth of boundary particles right of the image
        for j in range(4):
            for i in range(4):
                pts.append((21.0 + 1.5 * i, 4.0 + 1.5 * j, 4.0 + 1.5 * k, 3.1))
    sc = _scene(scenes.liquid_box_config((8.0, 8.0, 8.0)), pts)
    assert sc["cfg"].particleCount == 104
    return sc, who


LAST_REGION = (-np.inf, -np.inf, 23.0, np.inf, np.inf, np.inf)  # the three particles at z = 24


def splat_view(width=SW, height=SH, off=(0, 0), **kw):
    """The frame moved so that P(c, d) lands on pixel (c - off[0], d - off[1])."""
    kw.setdefault("radius", S_RADIUS)
    return make_view(width, height, (S_CENTRE[0] - off[0], S_CENTRE[1] - off[1]), **kw)


def splat_cases(sc, who):
    pos = sc["position"]
    near4 = f32(pos[who["near_4ulp"], 2])
    max_px = float(f32(S_RADIUS) * (f32(64.0) / near4))  # R of near_4ulp in the perspective view below, by its own expression
    ex, ey = float(pos[who["near_4ulp"], 0]), float(pos[who["near_4ulp"], 1])
    both, C = (1, 3), SplatCase
    return [
        C("threshold", "d2 == R2; boxes 9 x 9, 8 x 9, 9 x 8 (queued) and 8 x 8 (lane) by clipping at four edges and two corners; off-image",
          splat_view(), both, None, True, None),
        C("radius_2.5", "R = 2.5: every unclipped box is 8 x 8, nothing is queued by size", splat_view(radius=0.3125), both, None, True, None),
        C("radius_2.75", "R = 2.75: the quarter-pixel offsets give 8 x 9, 9 x 8, 8 x 8 beside 9 x 9", splat_view(radius=0.34375), both, None, False, None),
        C("far", "|u| = 2^20 - 0.5 (drawn, off-image) and 2^20 + 0.5 (not drawn)", make_view(SW, SH, (0.5, S_CENTRE[1]), eye=(-131054.0, 0.0, 0.0),
                                                                                          radius=S_RADIUS), both, None, False, None),
        C("near_eq", "nearPlane == cz of `interior`: not drawn", splat_view(near=10.0), both, None, True, None),
        C("near_below", "nearPlane one ulp below cz: drawn, only the nz == 0 fragments exist", splat_view(near=below(10.0)), both, None, True, None),
        C("near_cap", "nearPlane == cz - radius: the centre fragment is dropped", splat_view(near=10.0 - S_RADIUS), both, None, True, None),
        C("eye_inside", "the eye a quarter unit in front of `interior`'s centre: rim only", splat_view(eye=(0.0, 0.0, 9.75)), both, None, True, None),
        C("max_eq", "maxRadiusPx == R: drawn", splat_view(max_px=3.0), both, None, False, None),
        C("max_below", "maxRadiusPx one ulp below R: nothing is drawn", splat_view(max_px=below(3.0)), both, None, False, None),
        C("persp_radius", "perspective: cz == nearPlane; R one rounding step above maxRadiusPx (not drawn) and R == maxRadiusPx (drawn)",
          make_view(SW, SH, (65.5, 33.5), eye=(ex, ey, 0.0), scale=64.0, radius=S_RADIUS, near=0.625, max_px=max_px, perspective=True), both, None, True, None),
        C("persp_hair", "perspective: cz 3 and 4 ulps above nearPlane = 1, so cz > nearPlane holds by a hair and R = 6144 exceeds maxRadiusPx",
          make_view(SW, SH, (65.5, 33.5), eye=(ex, ey, 0.0), scale=16384.0, radius=S_RADIUS, near=1.0, max_px=4096.0, perspective=True), both, None, True, None),
        C("persp_behind", "perspective with particles behind the eye", make_view(SW, SH, (65.5, 33.5), eye=(9.0, 6.0, 8.0), scale=32.0, radius=S_RADIUS,
                                                                                near=0.5, perspective=True), both, None, False, None),
        C("1x1", "a one-pixel image on `interior`'s centre", splat_view(1, 1, (20, 20)), both, None, True, None),
        C("1x37", "one column", splat_view(1, 37, (120, 10)), both, None, True, None),
        C("37x1", "one row", splat_view(37, 1, (8, 34)), both, None, True, None),
        C("last_wave", "only particles of the last, partial wave are drawn", splat_view(), both, LAST_REGION, True, None),
        C("labels", "label -1, every palette entry and labels that wrap", splat_view(mode=3), both, None, False, (0.25, (1,))),
        C("ramp_x", "field x with lo, hi and the knots on particle coordinates", splat_view(mode=2, field=4, lo=5.0, hi=9.0), both, None, False, None),
        C("ramp_y", "field y", splat_view(mode=2, field=5, lo=4.0, hi=8.0), both, None, False, None),
        C("ramp_z", "field z", splat_view(mode=2, field=6, lo=8.0, hi=16.0), both, None, False, None),
    ]


DEEP_LATTICE = (17, 17, 15)  # 4335 = 4096 + 3 * 64 + 47 particles


def deep_splat_scene():
    """A liquid lattice (spacing 1.5, as test_render.tie_scene) with more particles than the drain grid has waves."""
    nx, ny, nz = DEEP_LATTICE
    pts = [(4.0 + 1.5 * i, 4.0 + 1.5 * j, 4.0 + 1.5 * k, 1.1) for k in range(nz) for j in range(ny) for i in range(nx)]
    return _scene(scenes.liquid_box_config((10.0, 10.0, 10.0)), pts)


def deep_splat_cases():
    # 4 pixels per unit, radius 0.75: R = 3, centres on pixel centres 6 pixels apart, every box 9 x 9 and on-image; 29 fragments a sphere
    frame = dict(centre=(4.5 - 16.0, 104.5 + 16.0), scale=4.0, radius=0.75, mode=1)
    return [SplatCase("deep_queue", "more queued splats than drain waves: the second trip of k_render_drain's loop (seen in the thickness)",
                      make_view(107, 109, **frame), (1,), None, True, None),
            SplatCase("deep_queue_back", "the same from behind: the last of the sorted order, the queue's tail, wins the pixels",
                      make_view(107, 109, eye=(0.0, 0.0, 32.0), back=True, **frame), (1,), None, True, None)]


# ---- triangles ---------------------------------------------------------------------------------------------------------------
# The frame of the triangle scene: 131 x 67 at 8 pixels per unit, eye at z = 5; the point at pixel coordinates (px, py) is
# x = 2 + px / 8, y = (83 - py) / 8. Most triangles lie in the plane z = 10 (cz = 5).
TW, TH = 131, 67
T_CENTRE = (-16.0, 83.0)
T_EYE = (0.0, 0.0, 5.0)


def _Q(px, py, z=10.0):
    return (2.0 + px / 8.0, (83.0 - py) / 8.0, z, 2.1)


class _Builder:
    def __init__(self):
        self.pts, self.tris, self.who = [], [], {}

    def point(self, px, py, z=10.0):
        self.pts.append(_Q(px, py, z))
        return len(self.pts) - 1

    def raw(self, x, y, z):
        self.pts.append((x, y, z, 2.1))
        return len(self.pts) - 1

    def tri(self, name, a, b, c):
        self.who[name] = len(self.tris)
        self.tris.append((a, b, c))

    def new(self, name, corners, z=10.0, order=(0, 1, 2)):
        zz = np.broadcast_to(np.asarray(z, np.float64), (3,))
        ids = [self.point(px, py, zz[k]) for k, (px, py) in enumerate(corners)]
        self.tri(name, *[ids[k] for k in order])
        return ids


def _membrane_scene(cfg, epos, tris, liquid):
    E = len(epos)
    membranes = np.asarray(tris, np.int32).reshape(-1, 3)
    verts = membranes.ravel()
    by_vertex = np.argsort(verts, kind="stable")
    rank = np.arange(verts.size) - np.searchsorted(verts[by_vertex], verts[by_vertex])
    assert rank.max() < 7  # at most 7 membranes a particle
    pml = -np.ones((E, 7), np.int32)
    pml[verts[by_vertex], rank] = (by_vertex // 3).astype(np.int32)
    elastic = np.zeros((E * 32, 4), np.float32)
    elastic[:, 0] = -1.0  # no springs
    return _scene(cfg, list(epos) + list(liquid), elastic, membranes, pml, E)


def triangle_scene():
    """(scene, who, spheres): hand-made membranes over hand-placed elastic particles, then a token of liquid. `who` names triangles,
    `spheres` the original ids of the three particles the compose cases are about."""
    b = _Builder()
    # coverage
    b.new("right", [(2, 2), (10, 2), (2, 10)])                          # the hypotenuse passes through the centres px + py == 11
    b.new("right_cw", [(14, 2), (22, 2), (14, 10)], order=(0, 2, 1))    # the same wound the other way
    p = [b.point(*q) for q in ((26, 2), (34, 2), (26, 10), (34, 10))]
    b.tri("sq_lower", p[0], p[1], p[2]); b.tri("sq_upper", p[1], p[3], p[2])
    p = [b.point(*q) for q in ((38, 2), (46, 2), (38, 10), (46, 10))]
    b.tri("sq2_upper", p[1], p[3], p[2]); b.tri("sq2_lower", p[0], p[1], p[2])   # the other table order
    p = [b.point(*q) for q in ((50.5, 2.5), (58.5, 2.5), (50.5, 10.5), (58.5, 10.5))]  # corners on pixel centres: all four sides carry centres
    b.tri("quad_a", p[0], p[1], p[2]); b.tri("quad_b", p[1], p[3], p[2])
    hub = b.point(70.5, 8.5)
    ring = [b.point(*q) for q in ((76.5, 8.5), (73.5, 3.5), (67.5, 3.5), (64.5, 8.5), (67.5, 13.5), (73.5, 13.5))]
    for k in range(6):
        b.tri("fan%d" % k, hub, ring[k], ring[(k + 1) % 6])
    b.new("sliver", [(80, 2.25), (90, 2.25), (80, 2.375)])             # covers no centre
    b.new("collinear", [(80, 6), (84, 8), (88, 10)])
    b.new("snap", [(94, 2), (94 + 1 / 1024, 2 + 1 / 1024), (104, 7)])   # two corners snap to one 1/256 position
    # the box threshold: x1 - x0 (y1 - y0) == 7 is the lane's, == 8 is queued
    b.new("x8", [(2, 20), (9.5, 20), (2, 24)]); b.new("x9", [(14, 20), (22, 20), (14, 24)])
    b.new("y8", [(26, 20), (30, 20), (26, 27.5)]); b.new("y9", [(34, 20), (38, 20), (34, 28)])
    b.new("left8", [(-2.5, 34), (7.5, 34), (-2.5, 38)]); b.new("left9", [(-2.5, 42), (8, 42), (-2.5, 46)])
    b.new("right8", [(123, 34), (140, 34), (123, 38)]); b.new("right9", [(122.5, 42), (140, 42), (122.5, 46)])
    b.new("top8", [(108, -2.5), (112, -2.5), (108, 7.5)]); b.new("top9", [(116, -2.5), (120, -2.5), (116, 8)])
    b.new("bottom8", [(44, 59), (48, 59), (44, 70)]); b.new("bottom9", [(52, 58.5), (56, 58.5), (52, 70)])
    b.new("off_image", [(150, 10), (160, 10), (150, 20)])
    b.new("marks", [(16.5, 30.5), (32.5, 30.5), (16.5, 32.5)])          # its corners' x are the ramp case's lo and hi
    # near plane: one corner at z = 8
    b.new("near_corner", [(62, 20), (66, 20), (62, 24)], z=(8.0, 9.0, 9.0))
    # parallel to the image plane at a cz whose reciprocal's reciprocal is below it (perspective: depth < cz)
    b.new("recip", [(70, 20), (78, 20), (70, 28)], z=6.0 + RECIP_CZ)
    # extremes, in front of the eye of the usual frame (z = 4) and seen by the views with their eye at z = 0 or 3:
    # corner offsets from (2, 2) of -2^-14, 16 - 2^-16 and 16 become -4, 2^20 - 1 and 2^20 pixels at 65536 pixels per unit
    e, big, over = 2.0 ** -14, 16.0 - 2.0 ** -16, 16.0
    ids = [b.raw(2.0 - e, 2.0 - e, 4.0), b.raw(2.0 + big, 2.0 - e, 4.0), b.raw(2.0 - e, 2.0 + big, 4.0)]
    b.tri("huge", *ids)
    ids = [b.raw(2.0 - 2 * e, 2.0 - 2 * e, 4.0), b.raw(2.0 + over, 2.0 - 2 * e, 4.0), b.raw(2.0 - 2 * e, 2.0 + big - 2 * e, 4.0)]
    b.tri("too_far", *ids)
    # compose: spheres of radius 0.375 at z = 14 (cz = 9, the cap at 8.625) on pixel centres, and a triangle through each cap
    spheres = {"tilted": b.point(20.5, 50.5, 14.0), "flat": b.point(70.5, 50.5, 14.0), "nearer": b.point(100.5, 50.5, 14.0)}
    b.new("tilted", [(8.5, 34.5), (40.5, 34.5), (8.5, 66.5)], z=(11.625, 11.625, 15.625))  # cz = 6.625 + 4 l2: 8.625 on row 50
    b.new("flat", [(62, 42), (80, 42), (62, 60)], z=13.625)
    b.new("nearer", [(92, 42), (110, 42), (92, 60)], z=below(13.625))
    liquid = [(22.0 + 1.5 * i, 4.0 + 1.5 * j, 20.0 + 1.5 * k, 1.1) for k in range(2) for j in range(2) for i in range(2)]
    return _membrane_scene(scenes.liquid_box_config((8.0, 8.0, 8.0)), b.pts, b.tris, liquid), b.who, spheres


def _recip_cz():
    """The first cz = 2 + m / 64 with 1 / (1 / cz) < cz in float32: a triangle parallel to the image plane at that cz has, under
    perspective, depth below its corners' cz."""
    for m in range(1, 120):
        c = f32(2.0 + m / 64.0)
        if f32(1.0) / (f32(1.0) / c) < c:
            return float(c)
    raise AssertionError("no such cz")


RECIP_CZ = _recip_cz()
RECIP_DEPTH = float(f32(1.0) / (f32(1.0) / f32(RECIP_CZ)))
RAMP_BOUNDS = (2.0 + 16.5 / 8.0, 2.0 + 32.5 / 8.0)  # x of the corners of `marks`: the knots are 4 pixels apart, on pixel centres


def tri_view(width=TW, height=TH, off=(0, 0), **kw):
    kw.setdefault("eye", T_EYE)
    return make_view(width, height, (T_CENTRE[0] - off[0], T_CENTRE[1] - off[1]), **kw)


def triangle_cases():
    C = TriCase
    persp = dict(eye=(0.0, 0.0, 6.0), scale=32.0, perspective=True)  # cz = 4 in the plane z = 10: the same 8 pixels per unit there
    extreme = (0.5, TH - 0.5)
    return [
        C("coverage", "edges and vertices on pixel centres, both windings, shared edges, a fan, boxes 8 and 9 by size and clipping, degenerates",
          tri_view(), None, None, None),
        C("near_eq", "one corner with cz == nearPlane: unusable", tri_view(near=3.0), None, None, None),
        C("near_below", "nearPlane one ulp below that corner: drawn", tri_view(near=below(3.0)), None, None, None),
        C("huge", "a corner at 2^20 - 0.5 pixels in u, another in v: queued, the box is the whole image; 2^20 + 0.5: unusable",
          make_view(TW, TH, extreme, eye=(2.0, 2.0, 0.0), scale=65536.0), None, None, None),
        C("persp", "the perspective twin of the coverage case", tri_view(**persp), None, None, None),
        C("persp_near_eq", "perspective, a corner with cz == nearPlane", tri_view(near=2.0, **persp), None, None, None),
        C("persp_depth_eq", "perspective, the interpolated depth of `recip` equals nearPlane at every pixel: drawn, no fragment",
          tri_view(near=RECIP_DEPTH, **persp), None, None, None),
        C("persp_depth_below", "nearPlane one ulp below that depth: its fragments exist", tri_view(near=below(RECIP_DEPTH), **persp), None, None, None),
        C("persp_huge", "the perspective twin of the 2^20 case (cz = 1)", make_view(TW, TH, extreme, eye=(2.0, 2.0, 3.0), scale=65536.0, perspective=True),
          None, None, None),
        C("1x1", "a one-pixel image on the fan's hub", tri_view(1, 1, (70, 8)), None, None, None),
        C("ramp", "field x with lo and hi on corner coordinates", tri_view(), 4, RAMP_BOUNDS, None),
        C("compose", "depth ties with a sphere's cap keep the particle, one ulp nearer takes the pixel, the tilted triangle goes each way",
          tri_view(), None, None, (tri_view(radius=S_RADIUS), (2,))),
    ]


SHEET = 48  # 47 x 47 cells: 4418 triangles, every vertex in at most 6


def sheet_scene():
    """One elastic sheet of 48 x 48 particles a unit apart, steeply inclined: vertex (i, j) at (3 + i, 2 + j / 8, 3 + j) so that
    along +z a cell is 8 x 1 pixels at 8 pixels per unit and the image stays small."""
    n = SHEET
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    epos = np.stack([3.0 + i.ravel(), 2.0 + j.ravel() / 8.0, 3.0 + j.ravel(), np.full(n * n, 2.1)], 1)
    a = (j * n + i)[:-1, :-1].ravel()
    tris = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)])
    liquid = [(4.0 + 1.5 * x, 12.0 + 1.5 * y, 4.0 + 1.5 * z, 1.1) for z in range(2) for y in range(2) for x in range(2)]
    return _membrane_scene(scenes.liquid_box_config((17.0, 6.0, 17.0)), [tuple(p) for p in epos], tris, liquid)


def sheet_cases():
    # corners on whole pixels 8 apart in x: x1 - x0 == 8 for every triangle, all on-image; the restatement of this case takes
    # about 0.03 s with the box search and about 10 s over all pixels (tests/test_render_edges_host.py prints both)
    view = make_view(379, 51, (-24.0, 48.0 + 16.0), scale=8.0)
    return [TriCase("deep_queue", "more queued triangles than drain waves: the second trip of k_rm_drain's loop", view, None, None, None),
            TriCase("deep_131x67", "the sheet across the left, right and top borders of a 131 x 67 image: clipped boxes in the drain loop",
                    make_view(131, 67, (-24.0 - 100.0, 48.0 + 16.0 - 20.0), scale=8.0), None, None, None),
            TriCase("deep_1x1", "the same sheet through one pixel", make_view(1, 1, (-24.0 - 100.0, 48.0 + 16.0 - 20.0), scale=8.0), None, None, None)]
