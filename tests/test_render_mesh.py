"""GPU tests of triangle rendering (sph_render_mesh / sph_read_render_triangles, include/sphmi.h): every word of the depth, index,
id, rgba and triangle images and all four counts equal to the numpy restatement (tests/render_mesh_ref.py), for the extracted
surface and the membranes, on the fused and the staged path, through orthographic and perspective views from outside and inside
at two image sizes, flat and smooth shading, a constant colour and every field, fresh and composed over particle renders;
determinism, read-only behaviour and lifetime; the calling rules; and the driver's files. No tolerance appears anywhere: integer
images are compared for equality, depths as bit patterns. tests/test_render_mesh_host.py shows on the CPU that these scenes and
views meet the conditions that keep the comparison from being trivially true; the cheap ones are asserted again here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diag_ref
import render_mesh_cases as mc
import render_mesh_ref as mr
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
IMAGES = ("depth", "index", "orig_id", "rgba", "triangle")
COLOUR = (0.3, 0.7, 0.9)


class Snapshot:
    """The state of the solver's last completed step and what the vertex scalars need of it."""

    def __init__(self, hip):
        self.state = diag_ref.state_with_ids(hip)
        self.counts = diag_ref.neighbor_counts(hip)
        self.back = hip.buffer("particleIndexBack")[:hip.N].astype(np.int64)


class Mesh:
    """What the restatement draws: the device's mesh (or the membrane corners of the exported state) and, for the surface, the
    device's own normals and sample records at the vertices, which the contract names as the inputs of shading and colour."""

    def __init__(self, hip, snap, source, verts, tris, types=(1,), corner=None):
        self.hip, self.snap, self.source, self.verts, self.tris, self.types, self.corner = hip, snap, source, verts, tris, types, corner
        self._normals = self._records = None

    def normals(self):
        if self._normals is None:
            self._normals = self.hip.surface_normals()
        return self._normals

    def scalar(self, field):
        if self.source == "surface":
            if self._records is None:
                self._records = self.hip.sample_points(self.verts, self.types) if self.verts.shape[0] else np.zeros((0, 8), np.float32)
            return mr.surface_scalar(self._records, field)
        return diag_ref.field_values(self.snap.state, field, self.snap.counts)[self.corner]


def extract(hip, snap, lattice, iso=mc.ISO, types=(1,)):
    origin, spacing, dims = lattice
    verts, tris = hip.extract_surface(origin, spacing, dims, iso=iso, field="shepard", types=types)
    return Mesh(hip, snap, "surface", verts, tris, types)


def membrane_mesh(hip, snap, membranes):
    verts, tris, corner = mr.membrane_vertices(snap.state, snap.back, membranes)
    return Mesh(hip, snap, "membranes", verts, tris, corner=corner)


def bounds_of(mesh, field):
    q = mesh.scalar(field)
    q = q[np.isfinite(q)]
    lo = float(q.min()) if q.size else 0.0
    hi = float(q.max()) if q.size else 1.0
    return lo, (hi if hi > lo else lo + 1.0)


def check_mesh(hip, mesh, view, what, shading="flat", field=None, compose=None, bounds=None):
    """One sph_render_mesh against the restatement, word for word; compose: (particle view, types) of the render drawn over;
    bounds: (lo, hi) of the ramp, by default the extremes of the vertex scalar. Returns (the restatement's result, the device's
    images)."""
    base = None
    if compose is not None:
        hip.render(compose[0], None, compose[1])
        base = hip.rendered()  # (test_render compares these with their own restatement)
    lo, hi = (0.0, 1.0) if field is None else bounds_of(mesh, field) if bounds is None else bounds
    want = mr.render_mesh(view, mesh.verts, mesh.tris, 1 if shading == "smooth" else 0, mesh.normals() if shading == "smooth" else None, COLOUR,
                          None if field is None else mesh.scalar(field), lo, hi, base)
    counts = hip.render_mesh(view, mesh.source, shading, COLOUR, field, lo, hi, compose is not None)
    got = hip.rendered(triangle=True)
    P = view.width * view.height
    tag = "%s %s %s field %r compose %r" % (what, mesh.source, shading, field, None if compose is None else compose[1])
    print("%s: counts %r (want %r) of %d pixels, winners %d, queued %d, partly outside %d, unusable %d, degenerate %d, ties %d" % (
        tag, counts, want["counts"], P, want["winners"], want["queued"], want["partly_outside"], want["unusable"], want["degenerate"], want["ties"]))
    assert counts == want["counts"], tag
    assert got["triangle"].dtype == np.int32 and got["triangle"].shape == (view.height, view.width)
    for k in IMAGES:
        diff = got[k].view(np.uint8) != want[k].view(np.uint8)
        assert not diff.any(), "%s: image %s differs in %d bytes; first at %r" % (tag, k, int(diff.sum()), tuple(int(x[0]) for x in np.nonzero(diff)))
    assert int((got["triangle"] >= 0).sum()) == counts[2] and int(np.isfinite(got["depth"]).sum()) == counts[3]
    if compose is not None:
        keep = got["triangle"] < 0
        for k in ("depth", "index", "orig_id", "rgba"):
            assert np.array_equal(got[k][keep].view(np.uint8), base[k][keep].view(np.uint8)), (tag, k)
    return want, got


def assert_not_trivial(want, view, vname, tag, composed=False):
    P = view.width * view.height
    if composed:
        particles = int((want["index"] >= 0).sum())
        assert want["counts"][2] >= 0.02 * P and particles >= 0.02 * P, (tag, want["counts"], particles)
    elif vname == "inside":
        assert want["queued"] >= 1 and want["unusable"] >= 1 and want["partly_outside"] >= 1, (tag, want["queued"], want["unusable"])
    else:
        assert want["counts"][2] >= 0.05 * P and want["winners"] >= 100, (tag, want["counts"], want["winners"])


def sweep(hip, name, sc, what, steps, full):
    """The four views at both sizes with the options dealt over them; `full`: every field with either shading on one view too."""
    snap = Snapshot(hip)
    cfg = hip.cfg
    meshes = [extract(hip, snap, mc.lattice_for(name, snap.state, cfg))]
    if sc["membranes"] is not None:
        meshes.append(membrane_mesh(hip, snap, sc["membranes"]))
    out = {}
    n = steps
    for size in mc.SIZES:
        for vname, view, pview, _, _ in mc.views(name, snap.state, cfg, size):
            for mesh in meshes:
                n += 1
                tag = "%s step %d %s %r" % (what, steps, vname, size)
                surface = mesh.source == "surface"
                shading = "smooth" if surface and n % 2 else "flat"
                field = None if n % 8 == 7 else n % 8
                want, got = check_mesh(hip, mesh, view, tag, shading, field)
                assert_not_trivial(want, view, vname, tag)
                out[vname, size, mesh.source] = got
                for types in ((2,), (1, 2)):
                    want, got = check_mesh(hip, mesh, view, tag, "flat" if n % 4 < 2 else shading, None if n % 3 else field, compose=(pview, types))
                    if types == (1, 2) or sc["membranes"] is not None:
                        assert_not_trivial(want, view, vname, tag, composed=True)
                    out[vname, size, mesh.source, types] = got
                if full and vname == "oblique" and size == mc.SIZES[1]:
                    for f in list(range(7)) + [None]:
                        for sh in ("flat", "smooth") if surface else ("flat",):
                            check_mesh(hip, mesh, view, tag + " full", sh, f)
    return out


@pytest.mark.parametrize("name", ["tiny", "tiny_jitter"])
def test_surface_images_equal_the_restatement(name):
    """After 1 and 3 steps, fused; the staged path gives the same state and therefore the same bytes."""
    sc = mc.scene(name)
    fused, staged = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        fused.step(it)
        staged_step(staged, it)
        if it in (0, 2):
            a = sweep(fused, name, sc, name + " fused", it + 1, full=(it == 0))
            b = sweep(staged, name, sc, name + " staged", it + 1, full=False)
            assert a.keys() == b.keys()
            for key in a:
                for k in a[key]:
                    assert np.array_equal(a[key][k].view(np.uint8), b[key][k].view(np.uint8)), (key, k)
    fused.close()
    staged.close()


def test_worm_membranes_and_inner_surface_equal_the_restatement():
    sc = mc.scene("worm")
    hip = scenes.hip_for(sc)
    hip.step(0)
    sweep(hip, "worm", sc, "worm", 1, full=True)
    hip.close()


def test_zero_area_triangles_of_an_extraction_are_skipped():
    """iso equal to a lattice value: t = 0 on the three edges that leave that point, so their vertices coincide with it."""
    sc = mc.scene("tiny")
    hip = scenes.hip_for(sc)
    hip.step(0)
    snap = Snapshot(hip)
    origin, spacing, dims = mc.lattice_for("tiny", snap.state, hip.cfg)
    f = hip.sample_grid(origin, spacing, dims, (1,))[..., 1]
    inner = f[1:-1, 1:-1, 1:-1]
    iso = float(inner.reshape(-1)[np.argmin(np.abs(inner - np.float32(0.5)))])
    mesh = extract(hip, snap, (origin, spacing, dims), iso=iso)
    p = mesh.verts[mesh.tris]
    coincident = ((p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1) | (p[:, 0] == p[:, 2]).all(1))
    assert coincident.sum() >= 1
    for vname, view, pview, _, _ in mc.views("tiny", snap.state, hip.cfg, mc.SIZES[1]):
        for shading, field in (("flat", None), ("smooth", 1)):
            want, got = check_mesh(hip, mesh, view, "zero area " + vname, shading, field)
            assert want["degenerate"] >= coincident.sum() and not np.isin(got["triangle"], np.flatnonzero(coincident)).any()
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_deterministic_read_only_self_contained_and_stale():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        a.step(it)
        b.step(it)
    snap = Snapshot(a)
    lattice = mc.surface_lattice(snap.state, cfg)
    mesh = extract(a, snap, lattice)
    normals = a.surface_normals()
    a.label_components(1.5364, (1, 2, 3))
    comp = a.components()
    n_sel = a.select(None, (1, 2, 3), [("surface", 0.1, np.inf)])
    sel = a.selection()
    a.field_create(0, np.arange(a.N, dtype=np.float32))
    membranes = membrane_mesh(a, snap, sc["membranes"])
    before = {n: a.buffer(n) for n in BUFFERS}
    last = None
    for vname, view, pview, _, _ in mc.views("tiny_elastic", snap.state, cfg, mc.SIZES[1]):
        for m, shading, field, compose in ((mesh, "smooth", 6, False), (mesh, "flat", None, True), (membranes, "flat", 3, False), (membranes, "flat", 1, True)):
            lo, hi = bounds_of(m, field) if field is not None else (0.0, 1.0)
            imgs = []
            for _ in range(2):  # twice: the same bytes
                if compose:
                    a.render(pview, None, (1, 2), thickness=True)
                counts = a.render_mesh(view, m.source, shading, COLOUR, field, lo, hi, compose)
                imgs.append((counts, a.rendered(thickness=compose, triangle=True)))
            assert imgs[0][0] == imgs[1][0]
            for k, v in imgs[0][1].items():
                assert np.array_equal(v.view(np.uint8), imgs[1][1][k].view(np.uint8)), (vname, m.source, k)
            last = imgs[0][1]
    assert "thickness" in last and last["thickness"].any()  # a composed pass leaves the thickness image as it is
    after = {n: a.buffer(n) for n in BUFFERS}
    for n in BUFFERS:
        assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    assert np.array_equal(a.surface_normals().view(np.uint32), normals.view(np.uint32))  # the mesh is still valid
    for x, y in zip(comp, a.components()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))  # ... and the labelling
    assert a.selection()[0].size == n_sel
    for x, y in zip(sel, a.selection()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))  # ... and the selection
    assert np.array_equal(a.field_read(0), np.arange(a.N, dtype=np.float32))  # ... and the field
    for it in range(3, 5):  # the images are self-contained: two more steps do not touch them
        a.step(it)
        b.step(it)
    for k, v in a.rendered(thickness=True, triangle=True).items():
        assert np.array_equal(v.view(np.uint8), last[k].view(np.uint8)), k
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    # the mesh is stale now: flat shading with a constant colour still draws it, exactly; smooth shading and a field are refused
    view = mc.views("tiny_elastic", snap.state, cfg, mc.SIZES[0])[2][1]
    want, _ = check_mesh(a, mesh_without_device(mesh), view, "stale")
    assert want["counts"][2] >= 0.05 * view.width * view.height
    for kw in (dict(shading="smooth"), dict(field=0, lo=0.0, hi=1.0)):
        with pytest.raises(sphmi.SphError) as e:
            a.render_mesh(view, "surface", **kw)
        assert scenes.error_status(e) == ERR_ORDER
    with pytest.raises(sphmi.SphError):  # the failed fresh render left no image
        a.rendered()
    a.close()
    b.close()


def mesh_without_device(mesh):
    return Mesh(None, mesh.snap, mesh.source, mesh.verts, mesh.tris, mesh.types, mesh.corner)


# ---- the calling rules ---------------------------------------------------------------------------------------------------------
def base_view():
    return frames.render_view((0, 0, 0), (26, 26, 26), 64, 48, radius=0.8)


def style(**fields):
    st = sphmi.SphRenderMeshStyle()
    st.source, st.shading, st.colourMode, st.field, st.lo, st.hi, st.compose = 0, 0, 0, 0, 0.0, 1.0, 0
    for k in range(3):
        st.colour[k] = 0.5
    for k, x in fields.items():
        if isinstance(x, tuple):
            for i, y in enumerate(x):
                getattr(st, k)[i] = y
        else:
            setattr(st, k, x)
    return st


def _rc_mesh(hip, view=None, st=None, null=None):
    view = base_view() if view is None else view
    st = style() if st is None else st
    out = np.full(4, -7, np.int64)
    rc = hip._L.sph_render_mesh(hip._h, None if null == "view" else C.byref(view), None if null == "style" else C.byref(st),
                                None if null == "counts" else out.ctypes.data)
    return rc, tuple(int(x) for x in out)


def _rc_read(hip, pixels=64 * 48):
    bufs = [np.empty(pixels, np.float32), np.empty(pixels, np.int32), np.empty(pixels, np.uint32), np.empty(4 * pixels, np.uint8)]
    return hip._L.sph_read_render(hip._h, *[x.ctypes.data for x in bufs], None)


def _rc_tri(hip, pixels=64 * 48, null=False):
    out = np.empty(pixels, np.int32)  # (kept alive across the call)
    return hip._L.sph_read_render_triangles(hip._h, None if null else out.ctypes.data)


def changed(**fields):
    v = base_view()
    for k, x in fields.items():
        if isinstance(x, tuple):
            for i, y in enumerate(x):
                getattr(v, k)[i] = y
        else:
            setattr(v, k, x)
    return v


ZERO = (0, 0, 0, 0)


def test_error_and_lifetime_rules():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    lattice = ([2.5] * 3, [2.0] * 3, [12, 12, 12])
    assert _rc_mesh(hip) == (ERR_ORDER, ZERO) and _rc_tri(hip) == ERR_ORDER  # a fresh solver
    hip.step(0)
    assert _rc_mesh(hip) == (ERR_ORDER, ZERO)  # source 0 before any extraction
    assert _rc_mesh(hip, st=style(source=1)) == (ERR_INVALID, ZERO)  # no membranes
    assert _rc_mesh(hip, st=style(compose=1)) == (ERR_ORDER, ZERO)  # (no mesh either)
    hip.extract_surface(*lattice)
    assert _rc_mesh(hip, st=style(compose=1)) == (ERR_ORDER, ZERO)  # compose without a successful render
    assert _rc_tri(hip) == ERR_ORDER and _rc_read(hip) == ERR_ORDER
    rc, counts = _rc_mesh(hip)
    assert rc == 0 and counts[0] > 100 and 0 < counts[2] == counts[3] < 64 * 48 and _rc_read(hip) == 0 and _rc_tri(hip) == 0
    assert _rc_tri(hip, null=True) == ERR_INVALID
    for null in ("view", "style", "counts"):
        assert _rc_mesh(hip, null=null)[0] == ERR_INVALID
    assert _rc_mesh(hip)[0] == 0
    bad_styles = [dict(source=-1), dict(source=2), dict(shading=-1), dict(shading=2), dict(colourMode=-1), dict(colourMode=2), dict(compose=-1),
                  dict(compose=2), dict(colourMode=1, field=-1), dict(colourMode=1, field=7), dict(colourMode=1, lo=1.0, hi=1.0),
                  dict(colourMode=1, lo=np.nan), dict(colourMode=1, hi=np.inf), dict(colour=(np.nan, 0, 0)), dict(colour=(0, np.inf, 0)),
                  dict(source=1, shading=1)]
    for fields in bad_styles:
        assert _rc_mesh(hip)[0] == 0
        assert _rc_mesh(hip, st=style(**fields)) == (ERR_INVALID, ZERO), fields
        if fields.get("compose", 0) not in (-1, 2):
            assert _rc_read(hip) == ERR_ORDER and _rc_tri(hip) == ERR_ORDER, fields  # a failed fresh render leaves no image behind
    for fields in (dict(width=0), dict(height=8193), dict(projection=2), dict(eye=(np.nan, 0, 0)), dict(scale=0.0), dict(nearPlane=-1.0),
                   dict(radius=0.0), dict(ambient=1.5)):  # the view is checked as sph_render_particles checks it
        assert _rc_mesh(hip, view=changed(**fields)) == (ERR_INVALID, ZERO), fields
    ok = [dict(colourMode=0, field=99, lo=np.nan), dict(colourMode=1, field=6, lo=-1.0, hi=1.0), dict(shading=1), dict(colourMode=1, colour=(np.nan,) * 3)]
    for fields in ok:
        assert _rc_mesh(hip, st=style(**fields))[0] == 0, fields
    # compose: over a particle render, over a mesh render, and only through the same width .. nearPlane
    assert hip.render(base_view(), None, (1, 2))[1] > 0 and _rc_tri(hip) == ERR_ORDER  # a particle render drops the triangle image
    before = hip.rendered()
    rc, counts = _rc_mesh(hip, st=style(compose=1))
    assert rc == 0 and counts[3] >= counts[2] and _rc_tri(hip) == 0
    assert _rc_mesh(hip, view=changed(radius=3.0, ambient=0.9, colourMode=1), st=style(compose=1))[0] == 0  # fields behind nearPlane may differ
    for fields in (dict(width=65), dict(height=47), dict(projection=0), dict(eye=(1.0, 2.0, 3.0)), dict(scale=7.0), dict(centre=(1.0, 2.0)),
                   dict(nearPlane=0.125)):
        hip.render(base_view(), None, (1, 2))
        assert _rc_mesh(hip, view=changed(**fields), st=style(compose=1)) == (ERR_INVALID, ZERO), fields
        after = hip.rendered()  # a failed composed call leaves the previous images as they were
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (fields, k)
    assert _rc_mesh(hip, st=style(compose=1, shading=2))[0] == ERR_INVALID and _rc_read(hip) == 0
    hip.step(1)
    assert _rc_read(hip) == 0  # the images outlive the state they show
    assert _rc_mesh(hip)[0] == 0 and _rc_mesh(hip, st=style(compose=1))[0] == 0  # a stale mesh draws flat with a constant colour
    assert _rc_mesh(hip, st=style(shading=1)) == (ERR_ORDER, ZERO) and _rc_mesh(hip, st=style(colourMode=1)) == (ERR_ORDER, ZERO)
    hip._runClearBuffers()  # any stage call: a new step has begun
    for st_ in scenes.STAGE_SEQUENCE[1:7]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st_])()
    assert _rc_mesh(hip) == (ERR_ORDER, ZERO)  # density and pressure force have not run yet
    hip.close()
    # the wrapper refuses wrong lengths and types before the library sees them
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.extract_surface(*lattice)
    for kw in (dict(colour=(1, 2)), dict(source="mesh"), dict(shading="phong"), dict(field="vorticity"), dict(compose=1)):
        with pytest.raises(sphmi.SphError):
            hip.render_mesh(base_view(), **kw)
    with pytest.raises(sphmi.SphError):
        hip.render_mesh(None)
    counts = hip.render_mesh(base_view(), colour=(1.0, 0.5, 0.25))
    assert len(counts) == 4 and hip.rendered(triangle=True)["triangle"].shape == (48, 64)
    hip.render(base_view())
    with pytest.raises(sphmi.SphError):
        hip.rendered(triangle=True)
    hip.close()


def test_membrane_rules():
    sc = scenes.SCENES["tiny_elastic"]()
    hip = scenes.hip_for(sc)
    hip.step(0)
    field3 = style(source=1, colourMode=1, field=3, lo=0.0, hi=32.0)
    rc, counts = _rc_mesh(hip, st=field3)
    assert rc == 0 and counts[0] + counts[1] == sc["cfg"].numOfMembranes and counts[2] > 0
    assert _rc_mesh(hip, st=style(source=1, shading=1)) == (ERR_INVALID, ZERO)  # smooth shading needs the surface
    assert _rc_mesh(hip, st=style(source=1, colourMode=1, field=7)) == (ERR_INVALID, ZERO)
    hip._runClearBuffers()
    for st_ in scenes.STAGE_SEQUENCE[1:7]:
        getattr(hip, scenes.HIP_STAGE_METHOD[st_])()
    assert _rc_mesh(hip, st=style(source=1)) == (ERR_ORDER, ZERO) and _rc_mesh(hip, st=field3) == (ERR_ORDER, ZERO)
    for st_ in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st_])
        m(1) if st_ == "integrate" else m()
    assert _rc_mesh(hip, st=style(source=1))[0] == 0 and _rc_mesh(hip, st=field3)[0] == 0
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_mesh(hip) == (ERR_INVALID, ZERO) and _rc_tri(hip) == ERR_ORDER
    hip.close()


def test_cpp_driver_frames(tmp_path):
    """sphmi_run --render-surface / --render-membranes: the PPM and depth files equal the Python images at the same steps, one
    _render_mesh line per frame; misuse exits with 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    eye, target, up = (55.5, -20.25, 61.0), (13.0, 9.5, 12.25), (0.0, 1.0, 0.0)
    camera = ["--render-eye"] + [repr(x) for x in eye] + ["--render-target"] + [repr(x) for x in target] + ["--render-up"] + [repr(x) for x in up]
    worm_eye, worm_target = (202.0, 122.0, 415.0), (52.0, 22.0, 415.0)  # beside the worm's body
    worm_camera = ["--render-eye"] + [repr(x) for x in worm_eye] + ["--render-target"] + [repr(x) for x in worm_target]
    grid = [18, 17, 19]
    surface = ["--surface-grid"] + [str(n) for n in grid] + ["--render-surface"]
    runs = {
        "alone": (box, surface + ["--render-size", "131", "67", "--render-focal", "170"] + camera,
                  dict(width=131, height=67, perspective=True, scale=170.0), None, ("surface",)),
        "over": (box, surface + ["--render-size", "96", "64", "--render-ortho", "2.5", "--render-radius", "1.4", "--render-colour", "type", "--render-types", "1",
                                 "--render-thickness"] + camera,
                 dict(width=96, height=64, perspective=False, scale=2.5, radius=1.4, colour="type"), (1,), ("surface",)),
        "worm": (["--worm"], ["--render-membranes", "--render-size", "120", "90", "--render-focal", "100", "--render-radius", "0.25", "--render-colour",
                              "density", "--render-types", "2"] + worm_camera,
                 dict(width=120, height=90, perspective=True, scale=100.0, radius=0.25, colour="density"), (2,), ("membranes",)),
    }
    for key, (scene_flags, flags, kw, types, sources) in runs.items():
        worm = key == "worm"
        steps = 1 if worm else 2
        hip = scenes.hip_for(mc.scene("worm") if worm else scenes.SCENES["tiny"]())
        cfg = hip.cfg
        for it in range(steps):
            hip.step(it)
        lo3 = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32)
        hi3 = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32)
        kw = dict(kw)
        kw.setdefault("radius", 0.5 * float(cfg.r0))
        cam = dict(eye=worm_eye, target=worm_target) if worm else dict(eye=eye, target=target, up=up)
        view = frames.render_view((cfg.xmin, cfg.ymin, cfg.zmin), (cfg.xmax, cfg.ymax, cfg.zmax), **cam, **kw)
        drawn = None
        if types is not None:
            drawn = hip.render(view, None, types, thickness=not worm)
        counts = {"surface": (0, 0, 0, 0), "membranes": (0, 0, 0, 0)}
        if "surface" in sources:
            hip.extract_surface(lo3, (hi3 - lo3) / (np.array(grid, np.float32) - np.float32(1)), grid, iso=0.5, field="shepard", types=(1, 2))
            counts["surface"] = hip.render_mesh(view, "surface", "smooth", (0.35, 0.6, 0.95), compose=types is not None)
        if "membranes" in sources:
            counts["membranes"] = hip.render_mesh(view, "membranes", "flat", (0.95, 0.6, 0.25), compose=True)
        img = hip.rendered(thickness=types is not None and not worm)
        hip.close()
        d = str(tmp_path / key)
        os.makedirs(d)
        r = subprocess.run([exe] + scene_flags + ["--steps", str(steps), "--render-every", str(steps), "--render-out", d] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        P = kw["width"] * kw["height"]
        last = counts[sources[-1]]
        line = "_render_mesh: surface drew %d skipped %d holds %d, membranes drew %d skipped %d holds %d, covered %d of %d pixels" % (
            counts["surface"][:3] + counts["membranes"][:3] + (last[3], P))
        assert r.stdout.count("_render_mesh:") == 1 and line in r.stdout, (line, r.stdout)
        assert last[2] >= 0.02 * P and (r.stdout.count("_render: drew") == 1) == (types is not None)
        if drawn is not None:
            assert ("_render: drew %d particles, covered %d of %d pixels" % (drawn[0], drawn[1], P)) in r.stdout
            # (the worm's skin joins the particle centres, so only the caps of the small spheres reach through it)
            assert int((img["index"] >= 0).sum()) >= (1 if worm else 0.02 * P)
        base = os.path.join(d, "frame_%d" % steps)
        assert np.array_equal(frames.read_ppm(base + ".ppm"), img["rgba"][:, :, :3]), key
        assert np.array_equal(np.fromfile(base + ".depth.f32", np.uint32), img["depth"].view(np.uint32).reshape(-1)), key
        if "thickness" in img:
            assert np.array_equal(np.fromfile(base + ".thickness.u32", np.uint32), img["thickness"].reshape(-1)), key
    d = str(tmp_path / "bad")
    os.makedirs(d)
    out = ["--render-every", "1", "--render-out", d]
    for bad in (out + ["--render-surface"], out + ["--render-surface", "--surface-grid", "1", "8", "8"], out + ["--render-membranes"],
                out + ["--render-types", "1"], out + surface + ["--render-types"], out + surface + ["--render-types", "4"],
                out + surface + ["--render-thickness"], ["--render-surface", "--surface-grid", "8", "8", "8"]):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
