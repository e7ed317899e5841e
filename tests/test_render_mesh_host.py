"""CPU tests of the triangle-rendering restatement (tests/render_mesh_ref.py): hand-made triangles at dyadic coordinates whose
images have exact answers, the properties the integer coverage rule promises (shared edges, closed meshes), and -- with the
oracle's state and the restatements alone -- the conditions that keep the scenes and views of the GPU tests
(tests/test_render_mesh.py, tests/render_mesh_cases.py) from comparing trivial images. The GPU tests compare the device's images
with this restatement word for word, so it is pinned here on its own."""
import ctypes
import os

import numpy as np
import pytest

import elastic_ref
import render_mesh_cases as mc
import render_mesh_ref as mr
import render_ref as rr
import scenes
import sphmi
from test_render_host import axis_view, make_state

f32 = np.float32
W, H = 64, 48


def at(pixels, z=10.0, height=H, scale=8.0):
    """Scene points that axis_view (u = 8 x, v = height - 8 y) projects to the given pixel coordinates, exactly."""
    p = np.asarray(pixels, np.float64).reshape(-1, 2)
    zz = np.broadcast_to(np.asarray(z, np.float64), (p.shape[0],))
    return np.stack([p[:, 0] / scale, (height - p[:, 1]) / scale, zz], 1).astype(np.float32)


def test_struct_layout_and_symbols_match_the_header():
    S = sphmi.SphRenderMeshStyle
    assert (S.source.offset, S.shading.offset, S.colourMode.offset, S.field.offset) == (0, 4, 8, 12)
    assert (S.lo.offset, S.hi.offset, S.colour.offset, S.compose.offset) == (16, 20, 24, 36) and ctypes.sizeof(S) == 40
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    lib = sphmi.device_lib()
    for name in ("sph_render_mesh", "sph_read_render_triangles"):
        assert name in sphmi.EXPORTED_SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in txt
    assert "typedef struct sph_render_mesh_style {" in txt
    assert lib.sph_abi_version() == sphmi.ABI_VERSION


def test_right_triangle_covers_the_pixels_written_out_by_hand():
    # corners at pixel coordinates (2, 2), (10, 2), (2, 10): the hypotenuse x + y = 12 passes through the centres with px + py = 11
    # and runs down the screen from b to c (dy > 0), so it owns them; the other two edges lie on pixel borders
    view = axis_view()
    want = np.zeros((H, W), bool)
    for row, last in ((2, 9), (3, 8), (4, 7), (5, 6), (6, 5), (7, 4), (8, 3), (9, 2)):  # row: columns 2 .. last
        want[row, 2:last + 1] = True
    assert want.sum() == 36
    pos = at([(2, 2), (10, 2), (2, 10)])
    for tri in ((0, 1, 2), (0, 2, 1), (1, 2, 0), (2, 1, 0)):  # any rotation, either winding
        for everywhere in (False, True):
            out = mr.render_mesh(view, pos, [tri], all_pixels=everywhere)
            assert np.array_equal(out["triangle"] == 0, want), tri
            assert out["counts"] == (1, 0, int(want.sum()), int(want.sum()))
            assert np.array_equal(out["cover"], want.astype(np.int64))
    assert (out["depth"][want] == f32(10.0)).all() and np.isinf(out["depth"][~want]).all()
    assert (out["index"] == -1).all() and (out["orig_id"] == 0xFFFFFFFF).all()
    assert (out["rgba"][~want] == (1, 2, 3, 4)).all()
    # the normal is (0, 0, +-1) and the view looks along z: facing 1, the full colour
    assert (out["rgba"][want] == (204, 204, 204, 255)).all()


def test_shared_diagonal_is_covered_exactly_once():
    view = axis_view()
    pos = at([(2, 2), (10, 2), (2, 10), (10, 10)])
    lower, upper = (0, 1, 2), (1, 3, 2)
    yy, xx = np.mgrid[0:H, 0:W]
    square = (xx >= 2) & (xx < 10) & (yy >= 2) & (yy < 10)
    diagonal = square & (xx + yy == 11)
    assert diagonal.sum() == 8
    for tris, first in (([lower, upper], 0), ([upper, lower], 1)):
        out = mr.render_mesh(view, pos, tris)
        assert np.array_equal(out["cover"], square.astype(np.int64))
        assert (out["triangle"][diagonal] == first).all()  # the triangle below the diagonal owns it, whichever is listed first
        assert out["ties"] == 0 and out["counts"] == (2, 0, 64, 64)
    # the same for a diagonal of the other slope and for windings that disagree
    out = mr.render_mesh(view, pos, [(0, 1, 3), (3, 0, 2)])
    assert np.array_equal(out["cover"], square.astype(np.int64))


def tetrahedron():
    pos = np.concatenate([at([(4.5, 4.5), (40.5, 8.5), (12.5, 36.5)], z=12.0), at([(20.5, 16.5)], z=6.0)])
    return pos, np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)])


def test_closed_meshes_cover_every_pixel_an_even_number_of_times():
    pos, tris = tetrahedron()
    out = mr.render_mesh(axis_view(), pos, tris)
    assert out["counts"][0] == 4 and (out["cover"] % 2 == 0).all() and (out["cover"] == 2).sum() > 300
    assert out["cover"][16, 20] == 2  # the apex projects onto a pixel centre, where three faces meet
    # a marching-cubes mesh of the oracle's tiny state, closed (surface_ref checks that), through orthographic views
    sc = mc.scene("tiny")
    ora = scenes.oracle_for(sc)
    ora.step()
    st = mc.oracle_state(ora, sc["cfg"])
    verts, tris = mc.reference_mesh(st, mc.lattice_for("tiny", st, sc["cfg"]))
    import surface_ref
    assert surface_ref.directed_edge_report(tris, verts.shape[0]) is None and tris.shape[0] > 1000
    seen = 0
    for name, view, _, _, _ in mc.views("tiny", st, sc["cfg"], mc.SIZES[1]):
        if view.projection == 0:
            out = mr.render_mesh(view, verts, tris)
            assert out["unusable"] == 0 and (out["cover"] % 2 == 0).all(), name
            assert (out["cover"] >= 2).sum() > 0.2 * view.width * view.height
            seen += 1
    assert seen == 2


def test_tie_rule_lower_triangle_index_wins():
    view = axis_view()
    pos = at([(2, 2), (30, 2), (2, 30), (2, 2), (30, 2), (2, 30)])
    one = mr.render_mesh(view, pos, [(0, 1, 2)])
    for tris in ([(0, 1, 2), (3, 4, 5)], [(3, 4, 5), (0, 1, 2)], [(0, 1, 2), (0, 2, 1)]):
        out = mr.render_mesh(view, pos, tris)
        assert np.array_equal(out["triangle"], one["triangle"]) and out["ties"] == out["counts"][2] > 300
        assert np.array_equal(out["cover"], 2 * one["cover"])
    # a nearer triangle with a higher index still wins
    pos2 = np.concatenate([pos[:3], at([(2, 2), (30, 2), (2, 30)], z=9.0)])
    out = mr.render_mesh(view, pos2, [(0, 1, 2), (3, 4, 5)])
    assert (out["triangle"][one["triangle"] == 0] == 1).all()


def test_zero_area_and_near_plane_triangles_are_skipped_and_counted():
    view = axis_view(near=5.0)
    pos = np.concatenate([at([(2, 2), (10, 10), (18, 18), (2, 30)]), at([(20, 20)], z=5.0), at([(21, 20)], z=12.0)])
    out = mr.render_mesh(view, pos, [(0, 1, 2), (0, 1, 1), (0, 1, 3), (0, 3, 4), (0, 3, 5)])
    assert out["counts"][:2] == (2, 3) and out["degenerate"] == 2 and out["unusable"] == 1  # cz > nearPlane is strict
    assert set(np.unique(out["triangle"])) == {-1, 2, 4}
    # two corners that snap to the same 1/256 pixel: collinear after the snap although not before
    pos = at([(2, 2), (2 + 1 / 1024, 2 + 1 / 1024), (30, 7)])
    assert mr.render_mesh(view, pos, [(0, 1, 2)])["counts"][:2] == (0, 1)
    # under perspective a fragment in front of the near plane does not exist although its triangle is drawn
    pv = axis_view(perspective=True, near=5.0, scale=40.0, centre=(32.0, 24.0))
    pos = np.array([(-1, -1, 5.5), (3, -1, 5.5), (-1, 3, 5.5)], np.float32)
    out = mr.render_mesh(pv, pos, [(0, 1, 2)])
    assert out["counts"][0] == 1 and out["counts"][2] > 100 and (out["depth"][out["triangle"] == 0] > f32(5.0)).all()


def test_clipping_at_the_four_edges_and_a_one_pixel_image():
    view = axis_view()
    pos = at([(-100, -100), (300, -100), (-100, 300)])
    for everywhere in (False, True):
        out = mr.render_mesh(view, pos, [(0, 1, 2)], all_pixels=everywhere)
        assert out["counts"] == (1, 0, W * H, W * H) and out["partly_outside"] == 1 and out["queued"] == 1
    # one triangle across each edge
    for corners, test in ((((-6, 10), (4, 20), (-6, 30)), lambda x, y: x < 4), (((70, 10), (60, 20), (70, 30)), lambda x, y: x >= 60),
                          (((10, -6), (30, -6), (20, 4)), lambda x, y: y < 4), (((10, 54), (20, 44), (30, 54)), lambda x, y: y >= 44)):
        a = mr.render_mesh(view, at(corners), [(0, 1, 2)])
        b = mr.render_mesh(view, at(corners), [(0, 1, 2)], all_pixels=True)
        yy, xx = np.nonzero(a["triangle"] == 0)
        assert yy.size > 10 and test(xx, yy).all() and np.array_equal(a["triangle"], b["triangle"]) and a["partly_outside"] == 1
    # wholly outside: drawn, no pixel
    assert mr.render_mesh(view, at([(-30, 5), (-10, 5), (-20, 20)]), [(0, 1, 2)])["counts"] == (1, 0, 0, 0)
    one = axis_view(width=1, height=1)
    assert mr.render_mesh(one, at([(-4, -4), (6, -4), (-4, 6)], height=1), [(0, 1, 2)])["counts"] == (1, 0, 1, 1)
    assert mr.render_mesh(one, at([(0.5, 0.5), (6, 0.5), (0.5, 6)], height=1), [(0, 1, 2)])["counts"] == (1, 0, 0, 0)  # its corner: not owned


def test_compose_over_a_particle_image():
    view = axis_view(centre=(0.5, 47.5))
    base = rr.render(make_state([(2.5, 3.0, 10.0)]), view)  # the sphere of test_render_host: centre pixel (20, 23), depth 8.5 there
    assert base["depth"][23, 20] == f32(8.5)
    # z = 6.5 + 4 l2 with l2 = 1/2 exactly on row 23: in front of the sphere above it, behind below, equal bits at (20, 23)
    v2 = axis_view(centre=(0.5, 47.5))  # u = 8 x + 0.5, v = 47.5 - 8 y
    pos = np.stack([(np.array([4.5, 36.5, 4.5]) - 0.5) / 8, (47.5 - np.array([7.5, 7.5, 39.5])) / 8, [6.5, 6.5, 10.5]], 1).astype(np.float32)
    alone = mr.render_mesh(v2, pos, [(0, 1, 2)])
    assert alone["depth"][23, 20].view(np.uint32) == base["depth"][23, 20].view(np.uint32)
    out = mr.render_mesh(v2, pos, [(0, 1, 2)], base=base)
    assert out["index"][23, 20] == 0 and out["triangle"][23, 20] == -1  # the tie stays with the particle
    assert np.array_equal(out["rgba"][23, 20], base["rgba"][23, 20])
    mesh, particle = out["triangle"] == 0, out["index"] == 0
    assert mesh.sum() > 100 and particle.sum() > 100 and not (mesh & particle).any()
    assert (out["triangle"][10:20, 20] == 0).all() and (out["index"][24:30, 20] == 0).all()
    assert np.array_equal(mesh | particle, (alone["triangle"] == 0) | (base["index"] == 0))
    assert out["counts"] == (1, 0, int(mesh.sum()), int((mesh | particle).sum()))
    assert (out["orig_id"][mesh] == 0xFFFFFFFF).all() and (out["index"][mesh] == -1).all()
    keep = ~mesh
    for k in ("depth", "index", "orig_id", "rgba"):
        assert np.array_equal(out[k][keep], base[k][keep])
    assert np.array_equal(out["depth"][mesh], alone["depth"][mesh]) and np.array_equal(out["rgba"][mesh], alone["rgba"][mesh])


def test_flat_normal_is_the_membrane_measure_normal():
    rng = np.random.default_rng(5)
    pos = rng.uniform(-3, 3, (30, 3)).astype(np.float32)
    pos[3] = pos[4]  # a zero-area triangle: normal 0
    membranes = np.array([(0, 1, 2), (2, 1, 0), (3, 4, 5), (6, 7, 8), (9, 11, 10)] + [tuple(rng.permutation(30)[:3]) for _ in range(20)])
    back = rng.permutation(30)
    rec, _ = elastic_ref.membrane_records(pos, back, membranes)
    verts, tris, j = mr.membrane_vertices(dict(pos=pos), back, membranes)
    assert np.array_equal(j, back[membranes.reshape(-1)]) and np.array_equal(tris, np.arange(75).reshape(25, 3))
    assert np.array_equal(mr.flat_normals(verts, tris).view(np.uint32), rec[:, 1:4].view(np.uint32))
    # ... and it is what shades the image: a tilted triangle, two-sided
    view = axis_view()
    view.ambient = 0.0
    p = at([(2, 2), (30, 2), (2, 30)], z=(8.0, 11.5, 8.0))
    n = mr.flat_normals(p, np.array([(0, 1, 2)]))[0]
    want = int(min(max(f32(0.8) * abs(n[2]), 0), 1) * f32(255.0) + f32(0.5))
    for tri in ((0, 1, 2), (0, 2, 1)):
        out = mr.render_mesh(view, p, [tri])
        assert (out["rgba"][out["triangle"] == 0] == (want, want, want, 255)).all() and 0 < want < 204


def test_ramp_endpoints_and_a_nan_scalar():
    view = axis_view()
    pos = at([(2, 2), (30, 2), (2, 30)])
    for q, colour in ((1.0, (0, 0, 255)), (0.5, (0, 0, 255)), (3.0, (255, 0, 0)), (9.0, (255, 0, 0)), (2.0, (0, 255, 0)), (np.nan, (0, 0, 255))):
        out = mr.render_mesh(view, pos, [(0, 1, 2)], scalar=np.full(3, q, np.float32), lo=1.0, hi=3.0)
        assert (out["rgba"][out["triangle"] == 0] == colour + (255,)).all(), q
    # one NaN corner poisons the interpolated scalar wherever its weight is not exactly zero times a finite number: s = 0
    out = mr.render_mesh(view, pos, [(0, 1, 2)], scalar=np.array([3.0, np.nan, 3.0], np.float32), lo=1.0, hi=3.0)
    assert (out["rgba"][out["triangle"] == 0] == (0, 0, 255, 255)).all()
    # a gradient: l1 = 1/2 halfway along a -> b
    out = mr.render_mesh(view, at([(2.5, 2.5), (34.5, 2.5), (2.5, 34.5)]), [(0, 1, 2)], scalar=np.array([1.0, 3.0, 1.0], np.float32), lo=1.0, hi=3.0)
    assert tuple(out["rgba"][3, 18]) == (0, 255, 0, 255)  # (row 2's centres lie on the edge a -> b, which does not own them)


def test_smooth_normals_interpolate_and_normalise():
    view = axis_view()
    view.ambient = 0.0
    pos = at([(2.5, 2.5), (34.5, 2.5), (2.5, 34.5)])
    normals = np.array([(0, 0, 1), (1, 0, 0), (0, 0, 1)], np.float32)
    out = mr.render_mesh(view, pos, [(0, 1, 2)], shading=1, normals=normals)
    # at pixel (18, 3): l1 = 1/2, n = (1/2, 0, 1/2) / len
    h = f32(0.5)
    ln = np.sqrt((h * h + f32(0) * f32(0)) + h * h)
    want = int(f32(0.8) * np.abs(h / ln) * f32(255.0) + f32(0.5))
    assert tuple(out["rgba"][3, 18]) == (want, want, want, 255)
    zero = mr.render_mesh(view, pos, [(0, 1, 2)], shading=1, normals=np.zeros((3, 3), np.float32))
    assert (zero["rgba"][zero["triangle"] == 0] == (0, 0, 0, 255)).all()  # len 0: n = 0, only the ambient term (0 here)


def test_bounding_box_search_equals_the_definition():
    rng = np.random.default_rng(11)
    for trial in range(6):
        perspective = trial % 2 == 1
        view = axis_view(width=53, height=37, perspective=perspective, scale=30.0 if perspective else 8.0, centre=(26.5, 18.5), near=0.5)
        n = 60
        pos = np.stack([rng.uniform(-4, 4, 3 * n), rng.uniform(-3, 3, 3 * n), rng.uniform(0.2, 12, 3 * n)], 1).astype(np.float32)
        pos[: 3 * 10] *= (40.0, 40.0, 1.0)  # far larger than the image
        pos[3 * 10: 3 * 20, :2] = np.round(pos[3 * 10: 3 * 20, :2] * 8) / 8 + 1 / 16  # corners on pixel centres
        tris = np.arange(3 * n).reshape(n, 3)
        a = mr.render_mesh(view, pos, tris)
        b = mr.render_mesh(view, pos, tris, all_pixels=True)
        for k in ("depth", "index", "orig_id", "rgba", "triangle", "cover"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (trial, k)
        assert a["counts"] == b["counts"] and a["counts"][0] > 20 and a["counts"][2] > 0.5 * 53 * 37 and a["queued"] >= 10
        if perspective:
            assert a["unusable"] > 0


# ---- the scenes and views of the GPU tests meet the conditions that keep them from hiding a failure --------------------------------
def check_conditions(name, st, sc, meshes, tag):
    for size in mc.SIZES:
        P = size[0] * size[1]
        for vname, view, pview, _, _ in mc.views(name, st, sc["cfg"], size):
            for mname, (verts, tris) in meshes.items():
                out = mr.render_mesh(view, verts, tris)
                what = (tag, mname, vname, size, out["counts"], out["winners"], out["queued"], out["partly_outside"], out["unusable"])
                if vname == "inside":
                    assert out["queued"] >= 1 and out["unusable"] >= 1 and out["partly_outside"] >= 1, what
                else:
                    assert out["counts"][2] >= 0.05 * P and out["winners"] >= 100, what
                for types in ((2,), (1, 2)):
                    if types == (2,) and name != "worm":
                        continue  # the boxes hold no elastic matter: nothing to compose over
                    base = rr.render(st, pview, None, types)
                    comp = mr.render_mesh(view, verts, tris, base=base)
                    held, particles = comp["counts"][2], int((comp["index"] >= 0).sum())
                    assert held >= 0.02 * P and particles >= 0.02 * P, what + (types, held, particles)


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter"])
def test_box_scenes_meet_the_conditions(name):
    sc = mc.scene(name)
    ora = scenes.oracle_for(sc)
    for step in range(3):
        ora.step()
        if step in (0, 2):
            st = mc.oracle_state(ora, sc["cfg"])
            check_conditions(name, st, sc, {"surface": mc.reference_mesh(st, mc.lattice_for(name, st, sc["cfg"]))}, "%s step %d" % (name, step + 1))


def test_worm_scene_meets_the_conditions():
    sc = mc.scene("worm")
    ora = scenes.oracle_for(sc)
    ora.step()
    st = mc.oracle_state(ora, sc["cfg"])
    lattice = mc.lattice_for("worm", st, sc["cfg"])
    assert max(lattice[2]) <= mc.LATTICE_SIDE
    verts, tris, _ = mr.membrane_vertices(st, st["back"], sc["membranes"])
    check_conditions("worm", st, sc, {"surface": mc.reference_mesh(st, lattice), "membranes": (verts, tris)}, "worm")
