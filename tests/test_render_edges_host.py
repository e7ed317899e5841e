"""CPU proof that the scenes and views of tests/render_edge_cases.py put the renderers into the edge states they are named for:
the oracle's state after one step and the restatements (tests/render_ref.py, tests/render_mesh_ref.py) alone. Every case is
rendered by the restricted search and over all pixels (the definition), which must agree; then the condition the case exists for
is asserted on the actual floats and integers, with the counts printed. The checks that only need images and counts
(tests/render_edge_checks.py) are asserted again on the device's output by tests/test_render_edges.py."""
import functools
import time

import numpy as np

import components_ref as cr
import render_edge_cases as ec
from render_edge_checks import expected_labels, splat_image_conditions, triangle_image_conditions
import render_mesh_cases as mc
import render_mesh_ref as mr
import render_ref as rr
import scenes

f32 = np.float32
RHO0 = 1000.0
SPLAT_IMAGES = ("depth", "index", "orig_id", "rgba", "sums")
TRI_IMAGES = ("depth", "index", "orig_id", "rgba", "triangle", "cover")


def oracle_run(sc):
    """(state, neighbour rows) of the oracle after one step."""
    ora = scenes.oracle_for(sc)
    ora.step()
    N = sc["cfg"].particleCount
    st = mc.oracle_state(ora, sc["cfg"])
    assert np.array_equal(st["pos"].view(np.uint32), sc["position"][st["ids"], :3].view(np.uint32))  # the inputs, bit for bit
    return st, ora.buffer("neighborIds").reshape(-1, 32)[:N].astype(np.int32)


@functools.lru_cache(maxsize=None)
def splat_setup():
    sc, who = ec.splat_scene()
    st, rows = oracle_run(sc)
    return sc, who, st, rows


@functools.lru_cache(maxsize=None)
def triangle_setup():
    sc, who, spheres = ec.triangle_scene()
    st, _ = oracle_run(sc)
    return sc, who, spheres, st


def both_ways(render, images):
    """The restricted search and the definition: equal in every image and count."""
    t0 = time.time()
    a = render(False)
    t1 = time.time()
    b = render(True)
    t2 = time.time()
    for k in images:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    for k in ("drawn", "covered", "fragments", "counts", "ties"):
        assert a.get(k) == b.get(k), k
    return a, t1 - t0, t2 - t1


def box_of(out, key, i):
    b = out["boxes"]
    k = np.flatnonzero(b[key] == i)
    assert k.size == 1, (key, i)
    return tuple(int(b[n][k[0]]) for n in ("x0", "x1", "y0", "y1"))


def sides(out, key, i):
    """The clipped box in pixels: a side of 8 (x1 - x0 == 7) is the lane's, a side of 9 is queued."""
    x0, x1, y0, y1 = box_of(out, key, i)
    return x1 - x0 + 1, y1 - y0 + 1


# ---- particles ---------------------------------------------------------------------------------------------------------------
# (drawn, covered, queued) of every splat case. Of the 104 particles 40 are placed by hand and 64 stand right of the image; a
# sphere of R = 3 on a pixel centre covers 29 pixels.
SPLAT_COUNTS = {
    "threshold": (104, 1117, 37),    # queued: the 40 but off_image and the two corners
    "radius_2.5": (104, 815, 0),
    "radius_2.75": (104, 823, 36),   # ... and sub_xy
    "far": (38, 0, 0),               # 104 - 66 with x >= 18
    "near_eq": (31, 856, 28),        # z > 10: not interior, row0 .. row4, the three near the eye, nor the 64 (z <= 8.5)
    "near_below": (33, 864, 30),     # ... plus interior and row4 at z = 10, four nz == 0 fragments each
    "near_cap": (33, 912, 30),       # z > 9.625: the same 33; the two at z = 10 lose their centre fragment alone
    "eye_inside": (33, 888, 30),     # z > 9.75: the same 33; the two at z = 10 keep 16 rim fragments each
    "max_eq": (104, 1117, 37),
    "max_below": (0, 0, 0),
    "persp_radius": (102, 2116, 4),  # not near_eq, not near_3ulp
    "persp_hair": (101, 0, 0),       # not near_eq, near_3ulp, near_4ulp; at 16384 pixels per unit nothing else meets the image
    "persp_behind": (34, 536, 13),
    "1x1": (104, 1, 0),
    "1x37": (104, 28, 4),            # col0 .. col3, 7 pixels of the column each
    "37x1": (104, 32, 4),            # row0 (4 pixels) .. row4; row0's box is clipped to 5 x 1
    "last_wave": (3, 87, 3),
    "labels": (104, 1117, 37),
    "ramp_x": (104, 1117, 37),
    "ramp_y": (104, 1117, 37),
    "ramp_z": (104, 1117, 37),
}
# (counts, queued, unusable, degenerate, partly_outside) of every triangle case. 38 membranes: collinear and snap are degenerate
# wherever their corners are usable, huge and too_far lie in front of the usual eye.
TRIANGLE_COUNTS = {
    "coverage": ((34, 4, 1444, 1444), 20, 2, 2, 8),
    "near_eq": ((33, 5, 1434, 1434), 20, 3, 2, 8),           # near_corner unusable: its 10 pixels go
    "near_below": ((34, 4, 1444, 1444), 20, 2, 2, 8),
    "huge": ((33, 5, 8777, 8777), 1, 4, 1, 1),               # at 65536 pixels per unit: too_far and three with corners past 2^20
    "persp": ((34, 4, 909, 909), 21, 2, 2, 13),
    "persp_near_eq": ((33, 5, 909, 909), 20, 3, 2, 12),
    "persp_depth_eq": ((33, 5, 873, 873), 20, 3, 2, 12),     # near_corner unusable; recip drawn, its 36 pixels go
    "persp_depth_below": ((33, 5, 909, 909), 20, 3, 2, 12),
    "persp_huge": ((37, 1, 8777, 8777), 1, 1, 0, 1),         # only too_far is skipped: nothing snaps together at this scale
    "1x1": ((34, 4, 1, 1), 0, 2, 2, 6),
    "ramp": ((34, 4, 1444, 1444), 20, 2, 2, 8),
    "compose": ((34, 4, 1042, 3006), 20, 2, 2, 8),
}
SHEET_COUNTS = {
    "deep_queue": ((4418, 0, 376 * 47, 376 * 47), 4418, 0, 0, 0),
    # columns -100 + 8 i, rows -19 .. 28: 28 rows of 131 pixels; the 15 whole columns of cells by the 29 rows of cells that meet
    # the image are queued; the two cut columns (2 * 29 cells) and the top row of the whole ones (15 cells) cross the border
    "deep_131x67": ((4418, 0, 131 * 28, 131 * 28), 2 * 15 * 29, 0, 0, 2 * (2 * 29 + 15)),
    "deep_1x1": ((4418, 0, 1, 1), 0, 0, 0, 4),
}


def triangle_counts(out):
    return out["counts"], out["queued"], out["unusable"], out["degenerate"], out["partly_outside"]


def test_splat_cases_meet_their_conditions():
    sc, who, st, rows = splat_setup()
    N = st["pos"].shape[0]
    back = st["back"]
    j = {k: int(back[v]) for k, v in who.items()}
    assert N == 104 and N % 64 == 40
    pos = st["pos"]
    d = pos[:, None, :] - pos[None, :, :]
    r2 = (d * d).sum(2) + np.eye(N) * 1e9
    assert r2.min() >= 0.375 ** 2  # distinct particles at distinct positions, further apart than the labels' link radius
    seen = {}
    for case in ec.splat_cases(sc, who):
        labels = None
        if case.label is not None:
            labels = cr.label_state(st, rows, case.label[1], case.label[0])[0]
            assert np.array_equal(labels, expected_labels(st, case.label[1], N))
        out, t_box, t_all = both_ways(lambda everywhere: rr.render(st, case.view, case.region, case.types, case.thickness, RHO0, labels,
                                                                   all_pixels=everywhere), SPLAT_IMAGES)
        print("%s: drawn %d covered %d queued %d winners %d ties %d fragments %d (%.2f s, all pixels %.2f s) -- %s" % (
            case.name, out["drawn"], out["covered"], out["queued"], out["winners"], out["ties"], out["fragments"], t_box, t_all, case.why))
        assert (out["drawn"], out["covered"], out["queued"]) == SPLAT_COUNTS[case.name], case.name
        splat_image_conditions(case, out, out["drawn"], out["covered"], st, who, labels)
        seen[case.name] = out
        u, v, R, R2, cz, ok = rr.project(case.view, pos)
        if case.name == "threshold":
            want = dict(interior=(9, 9), left=(8, 9), right=(8, 9), top=(9, 8), bottom=(9, 8), corner_tl=(8, 8), corner_br=(8, 8), edge_deep=(6, 9))
            assert {n: sides(out, "j", j[n]) for n in want} == want
            x0, x1, y0, y1 = box_of(out, "j", j["off_image"])
            assert x0 > x1 and ok[j["off_image"]]
            i = j["interior"]
            assert (u[i], v[i], R[i], R2[i], cz[i]) == (20.5, 20.5, 3.0, 9.0, 10.0)
            dx = (f32(23) + f32(0.5)) - u[i]
            dy = (f32(20) + f32(0.5)) - v[i]
            assert dx * dx + dy * dy == R2[i]  # the pixel at d2 == R2, in the kernel's own floats
            exists, nz, depth = rr.fragment(case.view, u[i], v[i], R2[i], cz[i], np.array([23]), np.array([20]))
            assert exists[0] and nz[0] == 0 and depth[0] == cz[i] and rr.thickness_word(nz)[0] == 0
        if case.name == "radius_2.5":
            assert R[0] == 2.5 and out["queued"] == 0 and sides(out, "j", j["interior"]) == (8, 8) and sides(out, "j", j["sub_xy"]) == (8, 8)
        if case.name == "radius_2.75":
            want = dict(interior=(9, 9), sub_x=(8, 9), sub_y=(9, 8), sub_xy=(8, 8))
            assert R[0] == 2.75 and {n: sides(out, "j", j[n]) for n in want} == want and out["queued"] == 36
        if case.name == "far":
            assert u[j["far_below"]] == f32(ec.LIMIT - 0.5) and ok[j["far_below"]] and u[j["far_above"]] == f32(ec.LIMIT + 0.5) and not ok[j["far_above"]]
        if case.name in ("near_eq", "near_below"):
            near = f32(case.view.nearPlane)
            assert (cz[j["interior"]] == near) == (case.name == "near_eq") and ok[j["interior"]] == (case.name == "near_below")
            assert cz[j["interior"]] - near in (0.0, float(np.spacing(near)))
        if case.name == "near_cap":
            assert cz[j["interior"]] - f32(case.view.radius) == f32(case.view.nearPlane)
        if case.name == "eye_inside":
            assert 0 < cz[j["interior"]] < f32(case.view.radius)
        if case.name in ("max_eq", "max_below"):
            assert (R[0] == f32(case.view.maxRadiusPx)) == (case.name == "max_eq") and f32(case.view.maxRadiusPx) <= R[0]
        if case.name == "persp_radius":
            a, b, c = j["near_eq"], j["near_3ulp"], j["near_4ulp"]
            near, cap = f32(case.view.nearPlane), f32(case.view.maxRadiusPx)
            assert cz[a] == near and cz[b] == 1 + 3 * np.spacing(f32(1.0)) and cz[c] == 1 + 4 * np.spacing(f32(1.0))
            assert R[b] > cap and R[c] == cap and not ok[a] and not ok[b] and ok[c]
        if case.name == "persp_hair":
            b, c = j["near_3ulp"], j["near_4ulp"]
            near, one = f32(case.view.nearPlane), np.spacing(f32(1.0))
            assert near == 1 and cz[b] == near + 3 * one and cz[c] == near + 4 * one and cz[j["near_eq"]] < near
            assert R[b] > 6143 and R[c] > 6143 and f32(case.view.maxRadiusPx) == 4096 and not ok[b] and not ok[c]
            others = np.ones(N, bool)
            others[[b, c, j["near_eq"]]] = False
            assert ok[others].all() and R[others].max() <= 4096
        if case.name == "persp_behind":
            assert (cz < 0).sum() >= 10 and not ok[cz < 0].any()
        if case.name == "ramp_x":
            x = [float(pos[j["row%d" % k], 0]) for k in range(9)]
            assert x[:7] == [3.0, 4.0, case.view.lo, 6.0, 7.0, 8.0, case.view.hi] and x[8] > case.view.hi
    assert len(seen) == 21 == len(SPLAT_COUNTS)


def test_deep_splat_queue_is_longer_than_the_drain_grid():
    sc = ec.deep_splat_scene()
    st, _ = oracle_run(sc)
    N = st["pos"].shape[0]
    for case in ec.deep_splat_cases():
        out, t_box, t_all = both_ways(lambda everywhere: rr.render(st, case.view, case.region, case.types, case.thickness, RHO0, None,
                                                                   all_pixels=everywhere), SPLAT_IMAGES)
        print("%s: drawn %d covered %d queued %d winners %d ties %d fragments %d (%.2f s, all pixels %.2f s) -- %s" % (
            case.name, out["drawn"], out["covered"], out["queued"], out["winners"], out["ties"], out["fragments"], t_box, t_all, case.why))
        assert out["queued"] == out["drawn"] == N == 4335 and out["queued"] > ec.DRAIN_WAVES and (out["queued"] - ec.DRAIN_WAVES) % 64 != 0
        b = out["boxes"]
        assert ((b["x1"] - b["x0"] == 8) & (b["y1"] - b["y0"] == 8)).all() and b["x0"].min() == 0 and b["x1"].max() < case.view.width - 1
        assert out["fragments"] == 29 * N  # a few fragments a sphere, 15 deep on every covered pixel
        assert out["sums"].max() == 15 * 256 and out["winners"] == 17 * 17
        winners = np.unique(out["index"][out["index"] >= 0])
        if case.name == "deep_queue_back":  # (a cell holds two z layers, so the sorted order interleaves the last two)
            print("    winners with a sorted index of %d or more: %d" % (ec.DRAIN_WAVES, int((winners >= ec.DRAIN_WAVES).sum())))
            assert (winners >= ec.DRAIN_WAVES).sum() >= 64  # whatever the order of arrival, some of the queue's tail wins pixels


# ---- triangles ---------------------------------------------------------------------------------------------------------------
def edge_values(S, t, px, py):
    """(w0, w1, w2, owns0, owns1, owns2) of drawn triangle t at the centre of pixel (px, py), in the kernel's integers."""
    k = int(np.flatnonzero(S.t == t)[0])
    Px, Py = 256 * px + 128, 256 * py + 128
    X, Y = [int(x[k]) for x in S.X], [int(y[k]) for y in S.Y]
    e = [(1, 2), (2, 0), (0, 1)]
    w = [int(mr.edge(X[p], Y[p], X[q], Y[q], Px, Py)) for p, q in e]
    o = [bool(mr.owns(X[p], Y[p], X[q], Y[q])) for p, q in e]
    return w, o


def test_triangle_cases_meet_their_conditions():
    sc, who, spheres, st = triangle_setup()
    verts, tris, corner = mr.membrane_vertices(st, st["back"], sc["membranes"])
    assert f32(ec.RECIP_DEPTH) < f32(ec.RECIP_CZ) and f32(ec.RECIP_CZ) - f32(ec.RECIP_DEPTH) == np.spacing(f32(ec.RECIP_DEPTH))
    seen = {}
    for case in ec.triangle_cases():
        base = None if case.compose is None else rr.render(st, case.compose[0], None, case.compose[1])
        scalar = None if case.field is None else st["pos"][corner, case.field - 4]
        lo, hi = case.bounds or (0.0, 1.0)
        out, t_box, t_all = both_ways(lambda everywhere: mr.render_mesh(case.view, verts, tris, scalar=scalar, lo=lo, hi=hi, base=base,
                                                                        all_pixels=everywhere), TRI_IMAGES)
        print("%s: counts %r queued %d unusable %d degenerate %d partly outside %d ties %d winners %d (%.2f s, all pixels %.2f s) -- %s" % (
            case.name, out["counts"], out["queued"], out["unusable"], out["degenerate"], out["partly_outside"], out["ties"], out["winners"],
            t_box, t_all, case.why))
        assert triangle_counts(out) == TRIANGLE_COUNTS[case.name], case.name
        triangle_image_conditions(case, out, out["counts"], st, who, spheres, seen.get("coverage"))
        seen[case.name] = out
        S = mr.Setup(case.view, verts, tris)
        X, Y, zi, usable = mr.project(case.view, verts)
        if case.name == "coverage":
            want = dict(x8=(8, 5), x9=(9, 5), y8=(5, 8), y9=(5, 9), left8=(8, 5), left9=(9, 5), right8=(8, 5), right9=(9, 5), top8=(5, 8), top9=(5, 9),
                        bottom8=(5, 8), bottom9=(5, 9), right=(9, 9), sliver=(11, 1), marks=(17, 3))
            assert {n: sides(out, "t", who[n]) for n in want} == want
            assert out["cover"].max() == 1 and out["ties"] == 0  # every shared edge and the fan's hub exactly once
            assert (out["cover"][2:10, 26:34] == 1).all() and (out["cover"][2:10, 38:46] == 1).all() and (out["cover"][3:11, 51:59] == 1).all()
            assert out["cover"][8, 70] == 1 and out["cover"][2, 50:59].sum() == 0 and out["cover"][2:11, 50].sum() == 0
            x0, x1, y0, y1 = box_of(out, "t", who["off_image"])
            assert x0 > x1
            assert int(X[3 * who["left8"]]) == -640 and int(Y[3 * who["top8"]]) == -640 and S.bx0[S.t == who["left8"]][0] == -3  # >> 8 floors
            a, b = 3 * who["snap"], 3 * who["snap"] + 1
            assert (X[a], Y[a]) == (X[b], Y[b]) and not np.array_equal(verts[a], verts[b])  # distinct in space, one snapped position
            # a centre on the hypotenuse (owned), on the quad's left and top (not owned), right and bottom (owned), at the hub
            for t, px, py, covered in ((who["right"], 9, 2, True), (who["right_cw"], 21, 2, True), (who["sq_lower"], 30, 5, True), (who["sq_upper"], 30, 5, False),
                                       (who["quad_a"], 50, 5, False), (who["quad_a"], 53, 2, False), (who["quad_b"], 58, 5, True), (who["quad_b"], 55, 10, True)):
                w, o = edge_values(S, t, px, py)
                zero = [k for k in range(3) if w[k] == 0]
                assert zero and min(w) == 0 and all(o[k] for k in zero) == covered, (t, px, py, w, o)
                assert (out["triangle"][py, px] == t) == covered
            hub = [edge_values(S, who["fan%d" % k], 70, 8) for k in range(6)]
            assert all(sorted(w)[:2] == [0, 0] for w, _ in hub)  # the hub's centre lies on two edges of each of the six
            assert sum(all(o[k] for k in range(3) if w[k] == 0) for w, o in hub) == 1
            assert S.A.size == 34 and set(np.unique(np.sign(mr.edge(X[tris[:, 0]], Y[tris[:, 0]], X[tris[:, 1]], Y[tris[:, 1]], X[tris[:, 2]], Y[tris[:, 2]])))) == {-1, 0, 1}
        if case.name in ("near_eq", "persp_near_eq"):
            c = 3 * who["near_corner"]
            assert not usable[c] and usable[c + 1] and out["unusable"] == 3
        if case.name in ("huge", "persp_huge"):
            assert box_of(out, "t", who["huge"]) == (0, case.view.width - 1, 0, case.view.height - 1) and out["queued"] == 1
            h, f = 3 * who["huge"], 3 * who["too_far"]
            assert int(X[h + 1]) == 2 ** 28 - 128 and int(Y[h + 2]) == -(2 ** 28) + 256 * case.view.height + 128 and usable[h:h + 3].all()
            assert not usable[f + 1] and usable[f] and usable[f + 2]
            A = int(S.A[S.t == who["huge"]][0])
            w, _ = edge_values(S, who["huge"], case.view.width - 1, 0)
            print("    huge: A = 2^%.2f, edge values at the far corner %r" % (np.log2(A), w))
            assert A > 2 ** 55 and max(w) > 2 ** 55
        if case.name == "persp_depth_eq":
            k = np.flatnonzero(S.t == who["recip"])
            _, exists, _, _, depth = mr.fragment(case.view, S, np.repeat(k, 1), np.array([S.x0[k[0]] + 1]), np.array([S.y0[k[0]] + 1]))
            assert depth[0] == f32(case.view.nearPlane) and not exists[0] and usable[3 * who["recip"]]
        if case.name == "compose":
            alone = mr.render_mesh(case.view, verts, tris)
            for n, (px, py) in (("tilted", (20, 50)), ("flat", (70, 50)), ("tilted", (20, 53))):
                assert alone["triangle"][py, px] == who[n] and alone["depth"][py, px].view(np.uint32) == base["depth"][py, px].view(np.uint32)
            assert alone["depth"][50, 100] == np.nextafter(base["depth"][50, 100], f32(0))
        if case.name == "ramp":
            a = 3 * who["marks"]
            assert (scalar[a], scalar[a + 1]) == case.bounds and (scalar < case.bounds[0]).any() and (scalar > case.bounds[1]).any()
    assert len(seen) == 12 == len(TRIANGLE_COUNTS)


def test_sheet_queue_is_longer_than_the_drain_grid():
    sc = ec.sheet_scene()
    st, _ = oracle_run(sc)
    verts, tris, _ = mr.membrane_vertices(st, st["back"], sc["membranes"])
    assert tris.shape[0] == 4418 and np.bincount(sc["membranes"].ravel()).max() == 6
    for case in ec.sheet_cases():
        out, t_box, t_all = both_ways(lambda everywhere: mr.render_mesh(case.view, verts, tris, all_pixels=everywhere), TRI_IMAGES)
        print("%s: counts %r queued %d partly outside %d winners %d (%.2f s, all pixels %.2f s) -- %s" % (
            case.name, out["counts"], out["queued"], out["partly_outside"], out["winners"], t_box, t_all, case.why))
        assert triangle_counts(out) == SHEET_COUNTS[case.name], case.name
        if case.name == "deep_queue":
            assert out["queued"] == 4418 > ec.DRAIN_WAVES and (4418 - ec.DRAIN_WAVES) % 64 != 0 and out["partly_outside"] == 0
            b = out["boxes"]
            assert (b["x1"] - b["x0"] == 8).all() and (b["y1"] - b["y0"] == 1).all()
            assert out["winners"] == 4418 and out["counts"] == (4418, 0, 376 * 47, 376 * 47)
            assert out["cover"].max() == 1 and (out["cover"][1:48, 0:376] == 1).all()  # every shared edge exactly once
        if case.name == "deep_131x67":
            assert out["cover"].max() == 1 and (out["cover"][0:28] == 1).all() and out["cover"][28:].sum() == 0
