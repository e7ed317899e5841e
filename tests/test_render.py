"""GPU tests of particle rendering (sph_render_particles / sph_read_render, include/sphmi.h): every word of the five images and
both counts equal to the numpy restatement (tests/render_ref.py), on the fused and the staged path, for orthographic and
perspective views from outside and from inside the liquid, every colour mode, a cut-away and thickness on and off; a hand-made
scene with depth ties; determinism, read-only behaviour and lifetime; the calling rules; and the driver's files. No tolerance
appears anywhere: integer images are compared for equality, depths as bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diag_ref
import render_ref as rr
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
INF = np.inf
SCENE_NAMES = ["tiny", "tiny_jitter", "tiny_elastic", "worm", "wide"]
IMAGES = ("depth", "index", "orig_id", "rgba", "thickness")


def _scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


def view_cases(state, cfg, size):
    """The four views of a state as (name, view keywords, types, region): an orthographic view along the longest axis of the
    moving matter with the boundary drawn and the wall in front of it cut away (so that the far wall, not one face of a lattice,
    supplies the winners), an orthographic oblique view, a perspective view from outside and a perspective view with the eye inside
    the matter near one end (small spheres, so that many of them are seen between the near ones, and the near plane at one
    radius, so that the spheres around the eye are large splats)."""
    W, H = size
    moving = diag_ref.selected(state, diag_ref.EVERYTHING, (1, 2))
    p = state["pos"][moving].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    centre, ext = 0.5 * (lo + hi), hi - lo
    a = int(np.argmax(ext))
    b, c = (a + 1) % 3, (a + 2) % 3
    e = np.eye(3)
    r0 = float(cfg.r0)
    radius = 0.5 * r0
    cut = [-INF] * 3 + [INF] * 3
    cut[a] = float(np.float32(lo[a] - r0))
    everything = diag_ref.selected(state, cut, (1, 2, 3))
    q = state["pos"][everything].astype(np.float64)
    qlo, qhi = q.min(0), q.max(0)
    diag = float(np.linalg.norm(ext))
    inside = centre - 0.38 * ext[a] * e[a]  # within the matter, most of it in front
    return [
        ("axis", dict(bbox=(qlo, qhi), eye=0.5 * (qlo + qhi) - e[a] * (qhi[a] - qlo[a] + 10 * r0), target=0.5 * (qlo + qhi), up=e[b],
                      perspective=False), (1, 2, 3), tuple(cut)),
        ("oblique", dict(bbox=(lo, hi), eye=centre + 2 * diag * (-1.0 * e[a] + 0.30 * e[b] + 0.20 * e[c]), target=centre, up=e[b],
                         perspective=False), (1, 2), None),
        ("outside", dict(bbox=(lo, hi), eye=centre + 1.2 * diag * (1.0 * e[a] - 0.35 * e[b] + 0.25 * e[c]), target=centre, up=e[c],
                         perspective=True), (1, 2), None),
        ("inside", dict(bbox=(lo, hi), eye=inside, target=inside + e[a] + 0.37 * e[b] + 0.21 * e[c], up=e[c], perspective=True, scale=0.35 * W,
                        radius=0.2 * r0, near=0.2 * r0, max_radius_px=4096.0), (1, 2), None),
    ], radius, (W, H)


def make_view(kw, radius, size, **more):
    kw = dict(kw)
    lo, hi = kw.pop("bbox")
    kw.update(more)
    kw.setdefault("radius", radius)
    return frames.render_view(lo, hi, size[0], size[1], **kw)


class Snapshot:
    """The state of the solver's last completed step and what the colour modes need of it."""

    def __init__(self, hip, rows=True):
        self.state = diag_ref.state_with_ids(hip)
        self.counts = diag_ref.neighbor_counts(hip) if rows else None
        self.rho0 = float(hip.cfg.rho0)


def check_render(hip, snap, view, what, region=None, types=(1, 2), thickness=False, labels=None):
    """One render against the restatement, word for word; returns the restatement's result."""
    want = rr.render(snap.state, view, region, types, thickness, snap.rho0, labels, snap.counts)
    drawn, covered = hip.render(view, region, types, thickness)
    got = hip.rendered(thickness=thickness)
    tag = "%s types %r region %r thickness %r mode %d" % (what, types, region, thickness, view.colourMode)
    print("%s: drawn %d (want %d) covered %d (want %d) of %d, winners %d, ties %d, fragments %d, largest box %d" % (
        tag, drawn, want["drawn"], covered, want["covered"], view.width * view.height, want["winners"], want["ties"], want["fragments"],
        want["max_box"]))
    assert (drawn, covered) == (want["drawn"], want["covered"]), tag
    assert got["depth"].dtype == np.float32 and got["index"].dtype == np.int32 and got["orig_id"].dtype == np.uint32
    assert got["rgba"].dtype == np.uint8 and got["rgba"].shape == (view.height, view.width, 4)
    for k in IMAGES:
        if k == "thickness" and not thickness:
            assert k not in got
            continue
        assert got[k].shape[:2] == (view.height, view.width)
        diff = got[k].view(np.uint8) != want[k].view(np.uint8)
        assert not diff.any(), "%s: image %s differs in %d bytes; first at %r" % (tag, k, int(diff.sum()), tuple(int(x[0]) for x in np.nonzero(diff)))
    assert int((got["index"] >= 0).sum()) == covered
    return want


def assert_not_trivial(want, view, name, tag):
    """What keeps a view from being trivially equal (asserted on the restatement's output)."""
    assert want["covered"] >= 0.05 * view.width * view.height, (tag, want["covered"])
    assert want["winners"] >= 200, (tag, want["winners"])
    if name == "inside":
        assert want["max_box"] > 8, (tag, want["max_box"])  # a footprint above 8 x 8: the queue of large splats runs


def sweep(hip, what, steps, full):
    """The four views of the solver's current state with the options dealt over them; `full`: every field and every mode too."""
    snap = Snapshot(hip)
    size = (320, 240) if hip.N > 50000 else (160, 120)
    cases, radius, size = view_cases(snap.state, hip.cfg, size)
    hip.label_components(np.inf, (1, 2, 3))
    labels = hip.components()[0]
    st = snap.state
    sel = diag_ref.selected(st, diag_ref.EVERYTHING, (1, 2))
    speed = diag_ref.field_values(st, 1)[sel]
    bounds = {0: (0.98 * snap.rho0, 1.05 * snap.rho0), 1: (0.0, max(float(speed.max()), 1e-3)), 2: (-1.0, max(float(st["p"][sel].max()), 1.0)),
              3: (0.0, 32.0)}
    for k in range(3):
        bounds[4 + k] = (float(st["pos"][sel][:, k].min()), float(st["pos"][sel][:, k].max()) + 1.0)
    out = {}
    for n, (name, kw, types, region) in enumerate(cases):
        tag = "%s step %d %s" % (what, steps, name)
        field = (2 * steps + n) % 7
        options = {"axis": dict(colour="type"), "oblique": dict(colour="density"),
                   "outside": dict(colour="field", field=field, lo=bounds[field][0], hi=bounds[field][1]), "inside": dict(colour="label")}[name]
        view = make_view(kw, radius, size, **options)
        thick = name in ("axis", "outside")
        want = check_render(hip, snap, view, tag, region, types, thick, labels)
        assert_not_trivial(want, view, name, tag)
        out[name] = hip.rendered(thickness=thick)
        if name == "axis":
            assert want["candidates"] < int(diag_ref.selected(st, diag_ref.EVERYTHING, types).sum())  # the cut-away removed the near wall
        if not full:
            continue
        # the other thickness setting and, on this view, the remaining options
        check_render(hip, snap, view, tag, region, types, not thick, labels)
        if name == "oblique":
            for f in range(7):
                check_render(hip, snap, make_view(kw, radius, size, colour="field", field=f, lo=bounds[f][0], hi=bounds[f][1]), tag + " field %d" % f,
                             region, types, False, labels)
        if name == "inside":
            for mode in ("type", "density", "field"):
                check_render(hip, snap, make_view(kw, radius, size, colour=mode, field=3, lo=0.0, hi=32.0), tag, region, (1, 2, 3), True, labels)
            lo3 = np.quantile(st["pos"][sel], 0.4, axis=0).astype(np.float32)
            check_render(hip, snap, view, tag + " cut", (-INF, float(lo3[1]), -INF, INF, INF, INF), (1, 2), True, labels)
    return out


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_images_equal_the_restatement(name):
    """After 1 and 3 steps, fused; the staged path gives the same state and therefore the same bytes."""
    sc = _scene(name)
    fused, staged = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        fused.step(it)
        staged_step(staged, it)
        if it in (0, 2):
            a = sweep(fused, name + " fused", it + 1, full=(it == 0))
            b = sweep(staged, name + " staged", it + 1, full=False)
            for view in a:
                for k in a[view]:
                    assert np.array_equal(a[view][k].view(np.uint8), b[view][k].view(np.uint8)), (view, k)
    fused.close()
    staged.close()


def tie_scene():
    """A liquid lattice at dyadic coordinates (spacing 1.5) and, away from it, two coincident boundary particles: every
    projection below is exact in float, so neighbours in one z layer tie on the pixels halfway between them."""
    cfg = scenes.liquid_box_config((8.0, 8.0, 8.0))
    pts = [(4 + 1.5 * i, 4 + 1.5 * j, 4 + 1.5 * k, 1.1) for k in range(4) for j in range(6) for i in range(6)]
    pts += [(20.0, 20.0, 10.0, 3.1)] * 2
    pos = np.array(pts, np.float32)
    cfg.particleCount = pos.shape[0]
    return dict(cfg=cfg, position=pos, velocity=np.zeros_like(pos), elastic=None, membranes=None, particle_membranes=None)


def test_depth_ties_on_the_device():
    sc = tie_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)  # the sorted state of the step is the state it started from: the input positions
    snap = Snapshot(hip)
    ids = snap.state["ids"]
    assert np.array_equal(snap.state["pos"].view(np.uint32), sc["position"][ids, :3].view(np.uint32))
    view = sphmi.SphRenderView()
    view.width, view.height, view.projection = 256, 256, 0
    for k, (r, u, f) in enumerate(zip((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        view.eye[k], view.right[k], view.up[k], view.forward[k] = 0.0, r, u, f
    view.scale, view.radius, view.nearPlane, view.maxRadiusPx, view.ambient = 8.0, 1.0, 0.0, 64.0, 0.25
    view.centre[0], view.centre[1] = 0.5, 255.5  # lattice centres on pixel centres, 12 pixels apart, R = 8
    view.colourMode = 1
    for thick in (False, True):
        want = check_render(hip, snap, view, "ties", None, (1, 2, 3), thick)
        assert want["ties"] >= 1 and want["drawn"] == hip.N
    # the coincident pair: every one of its pixels is a tie, won by the lower sorted index
    pair = np.flatnonzero(snap.state["types"].astype(np.int32) == 3)
    assert pair.size == 2
    got = hip.rendered()
    assert got["index"][255 - 160, 160] == pair.min() and not (got["index"] == pair.max()).any()
    # halfway between two lattice neighbours of the nearest layer: equal depth bits, the lower sorted index
    front = np.flatnonzero((snap.state["pos"][:, 2] == 4.0) & (snap.state["pos"][:, 1] == 4.0))
    x = snap.state["pos"][front, 0]
    a, b = front[x == 4.0][0], front[x == 5.5][0]
    assert got["index"][255 - 32, 38] == min(a, b)  # u = 32.5 and 44.5: column 38 has dx = +-6
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_deterministic_read_only_and_self_contained():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    for it in range(3):
        a.step(it)
        b.step(it)
    a.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
    normals = a.surface_normals()
    _, ncomp = a.label_components(1.5364, (1, 2, 3))
    comp = a.components()
    n_sel = a.select(None, (1, 2, 3), [("surface", 0.1, INF)])
    sel = a.selection()
    snap = Snapshot(a)
    cases, radius, size = view_cases(snap.state, cfg, (160, 120))
    before = {n: a.buffer(n) for n in BUFFERS}
    first = {}
    for name, kw, types, region in cases:
        for mode in ("type", "density", "field", "label"):
            view = make_view(kw, radius, size, colour=mode, field="neighbors", lo=0.0, hi=32.0)
            counts = a.render(view, region, types, thickness=True)
            img = a.rendered(thickness=True)
            assert a.render(view, region, types, thickness=True) == counts  # twice: the same bytes
            for k, v in a.rendered(thickness=True).items():
                assert np.array_equal(v.view(np.uint8), img[k].view(np.uint8)), (name, mode, k)
            first = img
    after = {n: a.buffer(n) for n in BUFFERS}
    for n in BUFFERS:
        assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    assert np.array_equal(a.surface_normals().view(np.uint32), normals.view(np.uint32))  # the mesh is still valid
    for x, y in zip(comp, a.components()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))  # ... and the labelling
    assert a.selection()[0].size == n_sel
    for x, y in zip(sel, a.selection()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))  # ... and the selection
    for it in range(3, 5):  # the images are self-contained: two more steps do not touch them
        a.step(it)
        b.step(it)
    for k, v in a.rendered(thickness=True).items():
        assert np.array_equal(v.view(np.uint8), first[k].view(np.uint8)), k
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    a.close()
    b.close()


def base_view():
    v = frames.render_view((0, 0, 0), (26, 26, 26), 64, 48, radius=0.8)
    return v


def _rc_render(hip, view=None, region=None, mask=0x6, thickness=0, null_view=False, null_counts=False):
    view = base_view() if view is None else view
    rg = None if region is None else np.ascontiguousarray(region, np.float32)
    out = np.full(2, -7, np.int64)
    rc = hip._L.sph_render_particles(hip._h, None if null_view else C.byref(view), None if rg is None else rg.ctypes.data, mask, thickness,
                                     None if null_counts else out.ctypes.data)
    return rc, int(out[0]), int(out[1])


def _rc_read(hip, thickness=False, pixels=64 * 48):
    bufs = [np.empty(pixels, np.float32), np.empty(pixels, np.int32), np.empty(pixels, np.uint32), np.empty(4 * pixels, np.uint8),
            np.empty(pixels, np.uint32) if thickness else None]
    return hip._L.sph_read_render(hip._h, *[None if x is None else x.ctypes.data for x in bufs])


def changed(**fields):
    v = base_view()
    for k, x in fields.items():
        if isinstance(x, tuple):
            for i, y in enumerate(x):
                getattr(v, k)[i] = y
        else:
            setattr(v, k, x)
    return v


def test_error_and_lifetime_rules():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    assert _rc_render(hip) == (ERR_ORDER, 0, 0) and _rc_read(hip) == ERR_ORDER  # a fresh solver
    with pytest.raises(sphmi.SphError):
        hip.render(base_view())
    with pytest.raises(sphmi.SphError):
        hip.rendered()
    hip.step(0)
    assert _rc_read(hip) == ERR_ORDER  # stepped, but nothing rendered yet
    rc, drawn, covered = _rc_render(hip)
    assert rc == 0 and drawn == 1440 and 0 < covered < 64 * 48 and _rc_read(hip) == 0
    assert hip._L.sph_read_render(hip._h, None, None, None, None, None) == 0  # any pointer may be NULL
    assert _rc_read(hip, thickness=True) == ERR_INVALID  # the render accumulated no thickness
    assert _rc_render(hip, thickness=1)[0] == 0 and _rc_read(hip, thickness=True) == 0 and _rc_read(hip) == 0
    assert _rc_render(hip, null_counts=True)[0] == ERR_INVALID
    assert _rc_read(hip) == ERR_ORDER  # a failed render leaves no image behind
    assert _rc_render(hip, null_view=True) == (ERR_INVALID, 0, 0)
    for mask in (0, 1, 0x10, 0x80000002):  # a bad typeMask
        assert _rc_render(hip)[0] == 0
        assert _rc_render(hip, mask=mask) == (ERR_INVALID, 0, 0) and _rc_read(hip) == ERR_ORDER
    assert _rc_render(hip, region=(0, 0, np.nan, 1, 1, 1)) == (ERR_INVALID, 0, 0)  # a NaN region bound
    assert _rc_render(hip, region=(5, 5, 5, 1, 1, 1)) == (0, 0, 0) and _rc_read(hip) == 0  # an empty region is legal
    bad = [dict(width=0), dict(width=8193), dict(height=0), dict(height=-3), dict(width=8192, height=4096), dict(projection=2), dict(projection=-1),
           dict(eye=(np.nan, 0, 0)), dict(right=(0, INF, 0)), dict(up=(0, 0, np.nan)), dict(forward=(-INF, 0, 0)),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=INF), dict(scale=np.nan), dict(centre=(np.nan, 0)), dict(centre=(0, INF)),
           dict(nearPlane=-0.5), dict(nearPlane=INF), dict(nearPlane=np.nan), dict(radius=0.0), dict(radius=-1.0), dict(radius=INF), dict(radius=np.nan),
           dict(maxRadiusPx=0.0), dict(maxRadiusPx=4097.0), dict(maxRadiusPx=np.nan), dict(colourMode=-1), dict(colourMode=4),
           dict(colourMode=2, field=-1, lo=0.0, hi=1.0), dict(colourMode=2, field=7, lo=0.0, hi=1.0), dict(colourMode=2, field=0, lo=1.0, hi=1.0),
           dict(colourMode=2, field=0, lo=0.0, hi=INF), dict(colourMode=2, field=0, lo=np.nan, hi=1.0), dict(colourMode=0, typeColour=((np.nan, 0, 0),)),
           dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=np.nan)]
    for fields in bad:
        assert _rc_render(hip)[0] == 0
        assert _rc_render(hip, view=changed(**fields)) == (ERR_INVALID, 0, 0), fields
        assert _rc_read(hip) == ERR_ORDER, fields
    ok = [dict(width=8192, height=2048, scale=1.0), dict(nearPlane=0.0), dict(maxRadiusPx=4096.0), dict(ambient=0.0), dict(ambient=1.0),
          dict(colourMode=2, field=6, lo=-1.0, hi=1.0), dict(colourMode=1, field=99, lo=np.nan)]  # field, lo, hi only matter in mode 2
    for fields in ok:
        assert _rc_render(hip, view=changed(**fields))[0] == 0, fields
    assert _rc_render(hip, view=changed(colourMode=3)) == (ERR_ORDER, 0, 0)  # no labelling at all
    hip.label_components(np.inf, (1, 2))
    assert _rc_render(hip, view=changed(colourMode=3))[0] == 0
    assert _rc_render(hip)[0] == 0
    hip.step(1)
    assert _rc_read(hip) == 0  # the images outlive the state they show
    assert _rc_render(hip, view=changed(colourMode=3)) == (ERR_ORDER, 0, 0)  # the labelling belongs to the previous state
    assert _rc_read(hip) == ERR_ORDER
    hip._runClearBuffers()  # any stage call: a new step has begun
    for st in scenes.STAGE_SEQUENCE[1:7]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc_render(hip) == (ERR_ORDER, 0, 0)  # density and pressure force have not run yet
    assert _rc_render(hip, view=changed(colourMode=2, field=3, lo=0.0, hi=1.0)) == (ERR_ORDER, 0, 0)
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(2) if st == "integrate" else m()
    assert _rc_render(hip)[0] == 0 and _rc_render(hip, view=changed(colourMode=2, field=3, lo=0.0, hi=1.0))[0] == 0
    with pytest.raises(sphmi.SphError):
        hip.render(base_view(), region=(0, 1, 2))
    with pytest.raises(sphmi.SphError):
        hip.render(base_view(), types=(0,))
    assert b"sph_render_particles" in hip._L.sph_last_error()
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_render(hip) == (ERR_INVALID, 0, 0) and _rc_read(hip) == ERR_ORDER
    hip.close()


def test_cpp_driver_frames(tmp_path):
    """sphmi_run --render-*: the PPM, depth and thickness files equal the Python images at the same steps; misuse exits with 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    eye, target, up = (55.5, -20.25, 61.0), (13.0, 9.5, 12.25), (0.0, 1.0, 0.0)
    camera = ["--render-eye"] + [repr(x) for x in eye] + ["--render-target"] + [repr(x) for x in target] + ["--render-up"] + [repr(x) for x in up]
    runs = {
        "persp": (["--render-size", "200", "150", "--render-focal", "260", "--render-colour", "density", "--render-thickness"] + camera,
                  dict(width=200, height=150, perspective=True, scale=260.0, colour="density"), True),
        "ortho": (["--render-size", "96", "128", "--render-ortho", "3.5", "--render-radius", "0.75", "--render-colour", "field:1:0:0.5"] + camera,
                  dict(width=96, height=128, perspective=False, scale=3.5, radius=0.75, colour="field", field=1, lo=0.0, hi=0.5), False),
        "label": (["--render-size", "64", "64", "--render-focal", "80", "--render-colour", "label"] + camera,
                  dict(width=64, height=64, perspective=True, scale=80.0, colour="label"), False),
        "type": (["--render-size", "64", "64", "--render-focal", "80", "--render-colour", "type"] + camera,
                 dict(width=64, height=64, perspective=True, scale=80.0, colour="type"), False),
    }
    hip = scenes.hip_for(scenes.SCENES["tiny"]())  # the same box
    cfg = hip.cfg
    want = {}
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            for key, (_, kw, thick) in runs.items():
                kw = dict(kw)
                kw.setdefault("radius", 0.5 * float(cfg.r0))
                view = frames.render_view((cfg.xmin, cfg.ymin, cfg.zmin), (cfg.xmax, cfg.ymax, cfg.zmax), eye=eye, target=target, up=up, **kw)
                if kw["colour"] == "label":
                    hip.label_components(np.inf, (1, 2))
                counts = hip.render(view, None, (1, 2), thick)
                want[key, it + 1] = (counts, hip.rendered(thickness=thick))
    hip.close()
    for key, (flags, kw, thick) in runs.items():
        d = str(tmp_path / key)
        os.makedirs(d)
        r = subprocess.run([exe] + box + ["--steps", "4", "--render-every", "2", "--render-out", d] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        names = ["frame_%d.%s" % (s, e) for s in (2, 4) for e in ("depth.f32", "ppm") + (("thickness.u32",) if thick else ())]
        assert sorted(os.listdir(d)) == sorted(names)
        for step in (2, 4):
            (drawn, covered), img = want[key, step]
            assert drawn == 1440 and covered > 0.05 * kw["width"] * kw["height"]
            assert ("_render: drew %d particles, covered %d of %d pixels" % (drawn, covered, kw["width"] * kw["height"])) in r.stdout
            base = os.path.join(d, "frame_%d" % step)
            assert np.array_equal(frames.read_ppm(base + ".ppm"), img["rgba"][:, :, :3]), (key, step)
            assert np.array_equal(np.fromfile(base + ".depth.f32", np.uint32), img["depth"].view(np.uint32).reshape(-1)), (key, step)
            if thick:
                assert np.array_equal(np.fromfile(base + ".thickness.u32", np.uint32), img["thickness"].reshape(-1)), (key, step)
    d = str(tmp_path / "quiet")
    os.makedirs(d)
    r = subprocess.run([exe] + box + ["--steps", "1", "--render-every", "1", "--render-out", d, "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "_render" not in r.stdout
    assert frames.read_ppm(os.path.join(d, "frame_1.ppm")).shape == (480, 640, 3)  # the defaults
    for bad in (["--render-every", "2"], ["--render-out", d], ["--render-every", "0", "--render-out", d], ["--render-thickness"],
                ["--render-every", "1", "--render-out", d, "--render-size", "0", "10"],
                ["--render-every", "1", "--render-out", d, "--render-size", "8192", "8192"],
                ["--render-every", "1", "--render-out", d, "--render-ortho", "2", "--render-focal", "100"],
                ["--render-every", "1", "--render-out", d, "--render-focal", "-1"],
                ["--render-every", "1", "--render-out", d, "--render-radius", "0"],
                ["--render-every", "1", "--render-out", d, "--render-colour", "rainbow"],
                ["--render-every", "1", "--render-out", d, "--render-colour", "field:7:0:1"],
                ["--render-every", "1", "--render-out", d, "--render-colour", "field:1:2:1"]):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
