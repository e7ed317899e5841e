"""What a case of tests/render_edge_cases.py exists for, as far as its images and counts show it: asserted on the restatements'
output by tests/test_render_edges_host.py and again on the device's by tests/test_render_edges.py."""
import numpy as np

import components_ref as cr
import render_edge_cases as ec
from sphmi import frames

f32 = np.float32
BLUE, CYAN, GREEN, YELLOW, RED = (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0)


def expected_labels(st, types, N):
    """Isolated particles: every selected one is a component of its own, numbered in sorted order."""
    sel = cr.selected(st, types)
    lab = np.full(N, -1, np.int32)
    lab[sel] = np.arange(int(sel.sum()), dtype=np.int32)
    return lab


def splat_image_conditions(case, img, drawn, covered, st, who, labels=None):
    """What a case exists for, as far as the images and the two counts show it. `img`: depth, index, rgba and (where the case has
    it) thickness of the restatement or of the device."""
    back = st["back"] if "back" in st else np.argsort(st["ids"])
    j = {k: int(back[v]) for k, v in who.items()}
    index, depth, rgba, thick = img["index"], img["depth"], img["rgba"], img.get("thickness")
    N = st["pos"].shape[0]
    name = case.name
    assert covered == int((index >= 0).sum())
    if name in ("threshold", "max_eq", "labels", "ramp_x", "ramp_y", "ramp_z"):
        assert drawn == N and not (index == j["off_image"]).any()
        assert (index[20, 17:24] == j["interior"]).all() and index[20, 16] == -1 and index[20, 24] == -1
        assert depth[20, 23] == f32(10.0) and depth[20, 20] == f32(10.0) - f32(ec.S_RADIUS)  # d2 == R2: nz = 0, the depth is cz
        assert (index == j["corner_tl"]).sum() == (index == j["corner_br"]).sum() > 0  # the lane's splats, a quarter cut off twice
    if name == "threshold":
        assert thick[20, 23] == 0 and thick[20, 20] == 256 and thick[20, 24] == 0  # covered with thickness word 0
        for n in ("left", "right", "top", "bottom"):
            assert (index == j[n]).sum() == (index == j["left"]).sum() > 0
    if name == "far":
        assert drawn == N - 66 and covered == 0  # x >= 18: far_above, off_image and the 64 right of the image
    if name == "near_eq":
        assert not (index == j["interior"]).any() and index[20, 20] == -1
    if name == "near_below":
        mine = index == j["interior"]
        assert mine.sum() == 4 and mine[20, 17] and mine[20, 23] and mine[17, 20] and mine[23, 20]
        assert (depth[mine] == f32(10.0)).all() and (thick[mine] == 0).all()
    if name == "near_cap":
        assert index[20, 20] == -1 and thick[20, 20] == 0 and index[20, 21] == j["interior"] and index[20, 19] == j["interior"]
    if name == "eye_inside":
        mine = index == j["interior"]
        # nz < 2/3: d2 in {8, 9} and, by one rounding, d2 == 5 (1 - 5/9 rounds down: depth = 0.25 - 0.375 nz is a few 1e-8 above 0)
        assert mine.sum() == 16 and not mine[20, 20] and mine[20, 23] and mine[18, 18] and mine[19, 18] and not mine[19, 19]
        assert 0 < depth[19, 18] < f32(1e-7)
    if name == "max_below":
        assert (drawn, covered) == (0, 0)
    if name == "persp_radius":
        assert drawn == N - 2 and (index == j["near_4ulp"]).any() and not (index == j["near_3ulp"]).any() and not (index == j["near_eq"]).any()
    if name == "persp_hair":
        assert (drawn, covered) == (N - 3, 0)  # drawn, either of the two would cover the whole image
    if name == "persp_behind":
        assert drawn == int((st["pos"][:, 2] > f32(8.5)).sum()) < N  # cz > nearPlane = 0.5 with the eye at z = 8
    if name == "1x1":
        assert (drawn, covered) == (N, 1) and index[0, 0] == j["interior"] and thick[0, 0] == 256
    if name == "1x37":
        assert covered == 28 and index[8, 0] == j["col0"] and index[16, 0] == j["col1"] and index[12, 0] == -1
    if name == "37x1":
        assert covered == 32 and [int(index[0, 8 * k]) for k in range(5)] == [j["row%d" % k] for k in range(5)]
    if name == "last_wave":
        assert drawn == 3 and N % 64 != 0 and set(np.unique(index)) == {-1} | {j["last%d" % k] for k in range(3)}
        assert min(j["last%d" % k] for k in range(3)) >= N - N % 64
    if name == "labels":
        won = np.asarray(labels)[np.unique(index[index >= 0])]
        assert set(range(ec.LABEL_COLOURS)) <= set(won.tolist()) and -1 in won and won.max() >= 2 * ec.LABEL_COLOURS
        grey = int(f32(0.5) * f32(255.0) + f32(0.5))
        assert labels[j["col0"]] == -1 and tuple(rgba[18, 120]) == (grey, grey, grey, 255)  # nz = 1 at the centre: the full colour
        for k in range(14):  # the row's labels wrap round the palette
            lab = int(labels[j["row%d" % k]])
            want = (np.clip(frames.LABEL_PALETTE[lab % ec.LABEL_COLOURS], 0, 1) * f32(255.0) + f32(0.5)).astype(np.int32)
            assert lab >= 0 and tuple(rgba[34, 8 + 8 * k, :3]) == tuple(want), (k, lab)
        assert max(int(labels[j["row%d" % k]]) for k in range(14)) >= ec.LABEL_COLOURS
    if name == "ramp_x":  # x = 3 + k: below lo, lo = 5, the knots 6, 7, 8, hi = 9, above hi
        want = (BLUE, BLUE, BLUE, CYAN, GREEN, YELLOW, RED, RED, RED)
        assert [tuple(rgba[34, 8 + 8 * k, :3]) for k in range(9)] == list(want)
    if name == "ramp_z":  # z = 6 + k: lo = 8, knots 10, 12, 14, hi = 16
        want = {0: BLUE, 2: BLUE, 4: CYAN, 6: GREEN, 8: YELLOW, 10: RED, 13: RED}
        assert {k: tuple(rgba[34, 8 + 8 * k, :3]) for k in want} == want
    if name == "ramp_y":  # y = 8 - k down the column: hi = 8 .. lo = 4, then below lo
        want = (RED, YELLOW, GREEN, CYAN, BLUE, BLUE)
        assert [tuple(rgba[18 + 8 * k, 120, :3]) for k in range(6)] == list(want)


PLANE = ("right", "right_cw", "sq_lower", "sq_upper", "sq2_upper", "sq2_lower", "quad_a", "quad_b", "x8", "x9", "y8", "y9", "left8", "left9",
         "right8", "right9", "top8", "top9", "bottom8", "bottom9") + tuple("fan%d" % k for k in range(6))  # in the plane z = 10
HELD = dict(right=36, right_cw=36, sq_lower=36, sq_upper=28, sq2_upper=28, sq2_lower=36, quad_a=28, quad_b=36, sliver=0, off_image=0,
            marks=8, x8=16, x9=16, y8=16, y9=16, left8=11, left9=12, right8=24, right9=24, top8=11, top9=12, bottom8=20, bottom9=20)


def held(img, t):
    return int((img["triangle"] == t).sum())


def triangle_image_conditions(case, img, counts, st, who, spheres, coverage=None):
    """What a case exists for, as far as the images and the four counts show it; `coverage`: the images of the coverage case."""
    tri, index, depth, rgba = img["triangle"], img["index"], img["depth"], img["rgba"]
    name = case.name
    M = len(who)
    assert counts[0] + counts[1] == M and counts[2] == int((tri >= 0).sum()) and counts[3] == int(np.isfinite(depth).sum())
    if name in ("coverage", "near_below", "ramp"):
        assert counts[:2] == (34, 4)  # skipped: collinear, snap and the two in front of the eye
        assert {n: held(img, who[n]) for n in HELD} == HELD
        assert sum(held(img, who["fan%d" % k]) for k in range(6)) == 90 and tri[8, 70] in [who["fan%d" % k] for k in range(6)]
        px = np.arange(2, 10)
        assert (tri[11 - px, px] == who["right"]).all() and (tri[11 - px, px + 12] == who["right_cw"]).all()  # the hypotenuse's centres
        px = np.arange(26, 34)
        assert (tri[35 - px, px] == who["sq_lower"]).all() and (tri[35 - px, px + 12] == who["sq2_lower"]).all()  # whichever is listed first
        quad = np.isin(tri, [who["quad_a"], who["quad_b"]])
        yy, xx = np.nonzero(quad)
        # of a y-up scene's top and left edges the bottom and right ones on the screen own their centres
        assert (xx.min(), xx.max(), yy.min(), yy.max()) == (51, 58, 3, 10) and quad.sum() == 64
        assert not np.isin(tri, [who["collinear"], who["snap"], who["huge"], who["too_far"]]).any()
    if name == "near_eq":
        assert counts[:2] == (33, 5) and held(img, who["near_corner"]) == 0
    if name == "near_below":
        assert held(img, who["near_corner"]) == 10
    if name in ("huge", "persp_huge"):
        P = case.view.width * case.view.height
        assert counts[2] == P and (tri == who["huge"]).all()
    if name == "persp":
        assert {n: held(img, who[n]) for n in PLANE} == {n: held(coverage, who[n]) for n in PLANE}  # cz = 4, scale 32: the same pixels
    if name == "persp_near_eq":
        assert held(img, who["near_corner"]) == 0 and counts[1] == 5
    if name == "persp_depth_eq":
        assert held(img, who["recip"]) == 0
    if name == "persp_depth_below":
        assert held(img, who["recip"]) > 0 and (depth[tri == who["recip"]] == f32(ec.RECIP_DEPTH)).all()
    if name == "1x1":
        assert counts[2:] == (1, 1) and tri[0, 0] == coverage["triangle"][8, 70]
    if name == "ramp":
        for n in ("left8", "left9"):  # x below lo: the ramp's first colour, facing the eye
            assert (rgba[tri == who[n]] == BLUE + (255,)).all()
        for n in ("right8", "right9", "top9"):
            assert (rgba[tri == who[n]] == RED + (255,)).all()
        # along a row of `tilted` q is x: below lo, lo at column 16, the knots at 20, 24, 28, hi at 32, above hi
        assert (tri[35, 9:39] == who["tilted"]).all()
        c = {px: tuple(int(x) for x in rgba[35, px, :3]) for px in (12, 16, 20, 24, 28, 32, 36)}
        assert c[12] == c[16] and c[16][:2] == (0, 0) and c[16][2] > 0
        assert c[20][0] == 0 and c[20][1] == c[20][2] > 0
        assert c[24][0] == 0 and c[24][2] == 0 and c[24][1] > 0
        assert c[28][0] == c[28][1] > 0 and c[28][2] == 0
        assert c[32] == c[36] and c[32][1:] == (0, 0) and c[32][0] > 0
    if name == "compose":
        back = st["back"] if "back" in st else np.argsort(st["ids"])
        s = {k: int(back[v]) for k, v in spheres.items()}
        cap = f32(9.0) - f32(ec.S_RADIUS)
        assert index[50, 20] == s["tilted"] and tri[50, 20] == -1 and depth[50, 20] == cap  # the tie keeps the particle
        assert tri[49, 20] == who["tilted"] and index[51, 20] == s["tilted"] and tri[51, 20] == -1  # nearer above, farther below
        assert index[53, 20] == s["tilted"] and depth[53, 20] == f32(9.0)  # a second tie on the rim: cz = 6.625 + 4 * 19 / 32
        assert index[50, 70] == s["flat"] and tri[50, 70] == -1 and depth[50, 70] == cap
        assert tri[50, 71] == who["flat"] and tri[49, 70] == who["flat"] and depth[50, 71] == cap
        assert tri[50, 100] == who["nearer"] and index[50, 100] == -1 and depth[50, 100] == np.nextafter(cap, f32(0))  # one ulp nearer
        assert counts[3] > counts[2] > 0 and (index >= 0).sum() > 100
