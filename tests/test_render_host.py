"""CPU tests of the rendering restatement (tests/render_ref.py) and of the host-side helpers around it (sphmi.frames: look_at,
render_view, the PPM and PNG writers, the colour tables): hand-made particles whose images have exact answers. The GPU tests
(tests/test_render.py) compare the device's images with this restatement word for word, so it is pinned here on its own."""
import os
import re

import numpy as np
import pytest

import render_ref as rr
import scenes  # noqa: F401  (puts the package on sys.path)
import sphmi
from sphmi import frames

f32 = np.float32
RHO0 = 1000.0


def make_state(points, types=None, rho=None, vel=None):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    return dict(pos=p, vel=np.zeros((n, 3), np.float32) if vel is None else np.asarray(vel, np.float32),
                rho=np.full(n, RHO0, np.float32) if rho is None else np.asarray(rho, np.float32), p=np.zeros(n, np.float32),
                types=np.full(n, 1.1, np.float32) if types is None else np.asarray(types, np.float32),
                keys=np.zeros(n, np.uint32), G=1, ids=np.arange(n, dtype=np.int64)[::-1].copy(), h=1.0, simScale=1.0)


def axis_view(width=64, height=48, scale=8.0, radius=1.5, perspective=False, centre=None, near=0.0, max_px=4096.0, mode=0):
    """Looking along +z from the origin: right = +x, up = +y, so u = x*k + centre.x and v = centre.y - y*k."""
    v = sphmi.SphRenderView()
    v.width, v.height, v.projection = width, height, 1 if perspective else 0
    for k, (r, u, f) in enumerate(zip((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        v.eye[k], v.right[k], v.up[k], v.forward[k] = 0.0, r, u, f
    v.scale = scale
    v.centre[0], v.centre[1] = (0.0, float(height)) if centre is None else centre
    v.nearPlane, v.radius, v.maxRadiusPx = near, radius, max_px
    v.colourMode, v.field, v.lo, v.hi = mode, 0, 0.0, 1.0
    for t, c in enumerate(((0.2, 0.4, 1.0), (1.0, 0.5, 0.0), (0.5, 0.5, 0.5))):
        for k in range(3):
            v.typeColour[t][k] = c[k]
    v.ambient = 0.25
    for k, b in enumerate((1, 2, 3, 4)):
        v.background[k] = b
    return v


def test_struct_layout_matches_the_header():
    assert sphmi.SphRenderView.width.offset == 0 and sphmi.SphRenderView.eye.offset == 12
    assert sphmi.SphRenderView.scale.offset == 60 and sphmi.SphRenderView.colourMode.offset == 84
    assert sphmi.SphRenderView.typeColour.offset == 100 and sphmi.SphRenderView.background.offset == 140
    import ctypes
    assert ctypes.sizeof(sphmi.SphRenderView) == 144
    for name in ("sph_render_particles", "sph_read_render"):
        assert name in sphmi.EXPORTED_SYMBOLS


def test_colour_tables_equal_the_header():
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()

    def table(name):
        body = txt[txt.index("#define " + name + " "):]
        body = body[:body.index("}\n") + 1].replace("\\\n", " ")
        return np.array([float(x) for x in re.findall(r"(\d+\.\d*)f", body)], np.float32).reshape(-1, 3)
    assert np.array_equal(table("SPH_RENDER_FIELD_RAMP"), frames.FIELD_RAMP) and frames.FIELD_RAMP.shape == (5, 3)
    assert np.array_equal(table("SPH_RENDER_LABEL_PALETTE"), frames.LABEL_PALETTE) and frames.LABEL_PALETTE.shape == (12, 3)


def test_one_sphere_on_a_pixel_centre():
    # u = 2.5*8 = 20 + 0.5, v = 48 - 3.0*8 - 0.5 -> the centre of pixel (20, 23); R = 12
    view = axis_view(centre=(0.5, 47.5))
    st = make_state([(2.5, 3.0, 10.0)])
    out = rr.render(st, view)
    yy, xx = np.mgrid[0:48, 0:64]
    want = ((xx - 20) ** 2 + (yy - 23) ** 2) <= 144
    assert np.array_equal(out["index"] == 0, want) and out["covered"] == int(want.sum()) and out["drawn"] == 1
    assert out["depth"][23, 20] == f32(10.0) - f32(1.5)
    assert np.isinf(out["depth"][~want]).all() and (out["index"][~want] == -1).all()
    assert (out["orig_id"][~want] == 0xFFFFFFFF).all() and (out["orig_id"][want] == 0).all()
    assert (out["rgba"][~want] == (1, 2, 3, 4)).all()
    # nz = 1 at the centre: the full type colour; the rim (d2 == R2) is shaded by the ambient term alone
    assert tuple(out["rgba"][23, 20]) == (51, 102, 255, 255)
    assert tuple(out["rgba"][23, 32]) == (int(0.2 * 0.25 * 255 + 0.5), int(0.4 * 0.25 * 255 + 0.5), int(0.25 * 255 + 0.5), 255)
    assert out["depth"][23, 32] == f32(10.0)


def test_nearer_sphere_wins():
    view = axis_view(centre=(0.5, 47.5))
    st = make_state([(2.5, 3.0, 10.0), (3.0, 3.0, 6.0)], types=(1.1, 2.1))
    out = rr.render(st, view)
    both = (rr.render(make_state([(2.5, 3.0, 10.0)]), view)["index"] == 0) & \
           (rr.render(make_state([(3.0, 3.0, 6.0)]), view)["index"] == 0)
    assert both.sum() > 100 and (out["index"][both] == 1).all()
    assert (out["orig_id"][both] == 0).all()  # ids are reversed in make_state
    assert tuple(out["rgba"][23, 24]) == (255, 128, 0, 255)


def test_tie_rule_lower_sorted_index_wins():
    view = axis_view(width=128, height=64, centre=(0.5, 96.5))  # v = 16.5: dy is whole, dx = +-8, so |dy| <= 8
    st = make_state([(10.0, 10.0, 10.0), (12.0, 10.0, 10.0)])
    out = rr.render(st, view)
    a = rr.render(make_state([(10.0, 10.0, 10.0)]), view)
    b = rr.render(make_state([(12.0, 10.0, 10.0)]), view)
    col = 88
    covered = a["index"][:, col] == 0
    assert covered.sum() == 17 and np.array_equal(covered, b["index"][:, col] == 0)
    assert np.array_equal(a["depth"][covered, col].view(np.uint32), b["depth"][covered, col].view(np.uint32))
    assert (out["index"][covered, col] == 0).all()
    assert out["ties"] >= 17
    # swapping the two particles swaps nothing in the image but the ids
    sw = rr.render(make_state([(12.0, 10.0, 10.0), (10.0, 10.0, 10.0)]), view)
    assert np.array_equal(sw["depth"].view(np.uint32), out["depth"].view(np.uint32))
    assert (sw["index"][covered, col] == 0).all()


def test_coincident_particles():
    view = axis_view(centre=(0.5, 47.5))
    st = make_state([(2.5, 3.0, 10.0)] * 3)
    out = rr.render(st, view, thickness=True)
    one = rr.render(make_state([(2.5, 3.0, 10.0)]), view, thickness=True)
    assert np.array_equal(out["index"], one["index"]) and out["drawn"] == 3 and out["ties"] == out["covered"]
    assert np.array_equal(out["thickness"], 3 * one["thickness"])
    assert (out["orig_id"][out["index"] == 0] == 2).all()


def test_culls():
    st = make_state([(2.5, 3.0, 10.0)])
    assert rr.render(st, axis_view(near=10.0))["drawn"] == 0          # cz > nearPlane is strict
    assert rr.render(st, axis_view(near=9.99))["drawn"] == 1
    near = rr.render(st, axis_view(centre=(0.5, 47.5), near=9.0))      # the cap nearer than 9 is cut away, the rim stays
    assert near["index"][23, 20] == -1 and near["index"][23, 31] == 0 and near["drawn"] == 1
    assert rr.render(st, axis_view(max_px=11.9))["drawn"] == 0 and rr.render(st, axis_view(max_px=12.0))["drawn"] == 1
    assert rr.render(make_state([(2.5, 3.0, -10.0)]), axis_view(perspective=True))["drawn"] == 0
    assert rr.render(make_state([(np.nan, 3.0, 10.0)]), axis_view())["drawn"] == 0
    assert rr.render(make_state([(2.0e5, 3.0, 10.0)]), axis_view())["drawn"] == 0   # |u| >= 2^20
    far = rr.render(make_state([(1.0e5, 3.0, 10.0)]), axis_view())
    assert far["drawn"] == 1 and far["covered"] == 0
    # selection: type mask, key, box
    assert rr.render(st, axis_view(), types=(2, 3))["drawn"] == 0
    assert rr.render(st, axis_view(), region=(0, 0, 0, 2.5, 9, 99))["drawn"] == 0
    assert rr.render(st, axis_view(), region=(2.5, 0, 0, 2.6, 9, 99))["drawn"] == 1
    bad = make_state([(2.5, 3.0, 10.0)]); bad["keys"][0] = 1
    assert rr.render(bad, axis_view())["drawn"] == 0


def test_clipping_at_the_four_edges():
    view = axis_view(centre=(0.5, 47.5))
    for x, y in ((0.0, 3.0), (8.0, 3.0), (4.0, 0.0), (4.0, 6.0), (0.0, 6.0), (8.0, 0.0)):
        st = make_state([(x, y, 10.0)])
        out = rr.render(st, view)
        full = rr.render(st, view, all_pixels=True)
        yy, xx = np.mgrid[0:48, 0:64]
        want = ((xx - int(8 * x)) ** 2 + (yy - (47 - int(8 * y))) ** 2) <= 144
        assert np.array_equal(out["index"] == 0, want) and 0 < want.sum() < 452
        assert np.array_equal(out["depth"].view(np.uint32), full["depth"].view(np.uint32))


@pytest.mark.parametrize("perspective", [False, True])
def test_restricted_search_equals_the_definition(perspective):
    rng = np.random.default_rng(20261017 + perspective)
    n = 300
    pts = np.stack([rng.uniform(-1.0, 9.0, n), rng.uniform(-1.0, 7.0, n), rng.uniform(0.2, 12.0, n)], 1).astype(np.float32)
    st = make_state(pts, types=rng.choice([1.1, 2.1, 3.1], n), rho=rng.uniform(950, 1060, n))
    view = axis_view(scale=40.0 if perspective else 8.0, radius=0.3 if perspective else 1.2, perspective=perspective, centre=(3.3, 40.7), near=0.5, max_px=30.0, mode=1)
    a = rr.render(st, view, types=(1, 2, 3), thickness=True, rho0=RHO0)
    b = rr.render(st, view, types=(1, 2, 3), thickness=True, rho0=RHO0, all_pixels=True)
    assert a["covered"] > 300 and a["winners"] > 50 and a["max_box"] > rr.SMALL
    for k in ("depth", "index", "orig_id", "rgba", "thickness"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["fragments"] == b["fragments"] and a["drawn"] == b["drawn"]


def test_mode_1_is_the_viewers_ramp():
    rho = np.array([0.0, 900.0, 1000.0, 1004.0, 1010.0, 1015.0, 1020.0, 1027.0, 1030.0, 1036.0, 1040.0, 1050.0, 3000.0, np.nan], np.float32)
    n = rho.size
    view = axis_view(width=8 * n, height=8, scale=8.0, radius=0.4, centre=(0.5, 3.5), mode=1)
    view.ambient = 1.0
    st = make_state([(k + 0.5, 0.0, 5.0) for k in range(n)], rho=rho)
    out = rr.render(st, view, rho0=RHO0)
    want = np.clip(frames.density_colour(rho, RHO0), 0, 1)
    for k in range(n):
        assert out["index"][3, 8 * k + 4] == k
        assert tuple(out["rgba"][3, 8 * k + 4, :3]) == tuple((want[k] * f32(255.0) + f32(0.5)).astype(np.int32)), k


def test_field_ramp_endpoints_and_nan():
    q = np.array([-5.0, 0.0, 0.25, 0.5, 0.75, 1.0, 7.0, np.nan, 0.125], np.float32)
    c = rr.field_colour(q, 0.0, 1.0)
    blue, cyan, green, yellow, red = frames.FIELD_RAMP
    for k, want in enumerate((blue, blue, cyan, green, yellow, red, red, blue)):
        assert np.array_equal(c[k], want), k
    assert np.array_equal(c[8], (0, 0.5, 1))
    lab = rr.label_colour([-1, 0, 11, 12, 25])
    assert np.array_equal(lab[0], (0.5, 0.5, 0.5)) and np.array_equal(lab[3], frames.LABEL_PALETTE[0])
    assert np.array_equal(lab[2], frames.LABEL_PALETTE[11]) and np.array_equal(lab[4], frames.LABEL_PALETTE[1])


def test_thickness_of_one_sphere_and_saturation():
    view = axis_view(centre=(0.5, 47.5))
    out = rr.render(make_state([(2.5, 3.0, 10.0)]), view, thickness=True)
    assert out["thickness"][23, 20] == 256 and out["thickness"][23, 32] == 0 and out["thickness"][0, 0] == 0
    assert out["thickness"][23, 26] == int(np.sqrt(f32(1) - f32(36) / f32(144)) * f32(256) + f32(0.5))
    assert rr.render(make_state([(2.5, 3.0, 10.0)]), view)["thickness"] is None
    sums = np.array([0, 255, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFFFFFF], np.uint64)
    assert np.array_equal(rr.saturate(sums), np.array([0, 255, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32))
    assert np.array_equal(frames.thickness_in_scene_units(np.array([256, 128], np.uint32), 1.5), [3.0, 1.5])


def test_look_at_and_render_view():
    e, r, u, f = frames.look_at((1, 2, 3), (1, 2, -7))
    assert all(a.dtype == np.float32 for a in (e, r, u, f))
    assert np.array_equal(f, (0, 0, -1)) and np.array_equal(r, (1, 0, 0)) and np.array_equal(u, (0, 1, 0)) and np.array_equal(e, (1, 2, 3))
    e, r, u, f = frames.look_at((3, -2, 5), (0.5, 4, 1), up=(0, 0, 1))
    m = np.stack([r, u, f]).astype(np.float64)
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-6) and np.linalg.det(m) < 0  # (right, up, forward) is a left-handed triple
    with pytest.raises(ValueError):
        frames.look_at((0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError):
        frames.look_at((0, 0, 0), (0, 1, 0), up=(0, 2, 0))
    lo, hi = (0.0, 0.0, 0.0), (10.0, 20.0, 30.0)
    for persp in (False, True):
        v = frames.render_view(lo, hi, 320, 240, perspective=persp, colour="field", field="pressure", lo=-1, hi=2)
        assert (v.width, v.height, v.projection, v.colourMode, v.field) == (320, 240, int(persp), 2, 2) and v.lo == -1 and v.hi == 2
        corners = np.array([[x, y, z] for x in (0, 10) for y in (0, 20) for z in (0, 30)], np.float32)
        pu, pv, R, R2, cz, ok = rr.project(v, corners)
        assert ok.all() and (pu > 0).all() and (pu < 320).all() and (pv > 0).all() and (pv < 240).all()
        assert max(np.abs(pu - 160).max() / 160, np.abs(pv - 120).max() / 120) > 0.9  # ... and the box fills the frame
    with pytest.raises(ValueError):
        frames.render_view(lo, hi, colour="rainbow")


def test_ppm_and_png_round_trips(tmp_path):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    p = str(tmp_path / "a.ppm")
    assert frames.write_ppm(p, img) == (37, 53)
    back = frames.read_ppm(p)
    assert back.dtype == np.uint8 and np.array_equal(back, img[:, :, :3])
    with open(p, "rb") as f:
        assert f.read(13) == b"P6\n53 37\n255\n"
    assert os.path.getsize(p) == 13 + 37 * 53 * 3
    with open(p, "wb") as f:  # a header with a comment and other whitespace
        f.write(b"P6 # made by hand\n2\t1 255\n" + bytes(range(6)))
    assert np.array_equal(frames.read_ppm(p).reshape(-1), np.arange(6))
    q = str(tmp_path / "a.png")
    assert frames.write_png(q, img) == (37, 53)
    assert np.array_equal(frames.read_png(q), img)
    data = open(q, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[24:29] == bytes([8, 6, 0, 0, 0])
    frames.write_png(q, img[:, :, :3])
    assert np.array_equal(frames.read_png(q)[:, :, :3], img[:, :, :3]) and (frames.read_png(q)[:, :, 3] == 255).all()
    with open(q, "wb") as f:
        f.write(data[:40] + bytes([data[40] ^ 1]) + data[41:])
    with pytest.raises(ValueError):
        frames.read_png(q)
    with pytest.raises(ValueError):
        frames.write_ppm(p, img.astype(np.float32))
