"""The scenes and lattices the surface-measure tests share (tests/test_surface_shells_host.py checks on the CPU, with the oracle's
state and the restatements alone, that each meets the conditions that make its comparison worth something;
tests/test_surface_shells.py then uses them on the device). Every scene is scenes.liquid_box with liquid rows dropped.

    pieces    a block of liquid with a hole in its middle and two small blocks apart from it: closed shells, one of them a cavity
    spray     single liquid particles more than 2 h apart, contoured at half the lattice maximum of the density: hundreds of
              shells of a few dozen triangles, several to a wave
    tiny      the block of scenes "tiny" on a lattice of h/4: one shell of thousands of triangles
    coarse    test_surface.py's coarse lattice that is not padded on the low side: a mesh with open sides"""
import numpy as np

import edit_ref
import sample_ref
import scenes
import surface_ref

f32 = np.float32
STEPS = 2
SPACING_IN_R0 = 0.93
ORIGIN_IN_R0 = 3.0


def _drop(sc, keep_fn):
    """The scene with only the liquid rows whose lattice index (i, j, k) keep_fn accepts; the boundary shell stays."""
    cfg, nl = sc["cfg"], sc["numOfLiquidP"]
    r0 = float(cfg.r0)
    ijk = np.rint((sc["position"][:nl, :3].astype(np.float64) - ORIGIN_IN_R0 * r0) / (SPACING_IN_R0 * r0)).astype(np.int64)
    keep = keep_fn(ijk[:, 0], ijk[:, 1], ijk[:, 2])
    rows = np.concatenate([np.flatnonzero(keep), np.arange(nl, cfg.particleCount)])
    n = int(rows.size)
    return dict(sc, cfg=edit_ref.with_count(cfg, n, 0), position=np.ascontiguousarray(sc["position"][rows]),
                velocity=np.ascontiguousarray(sc["velocity"][rows]), numOfLiquidP=int(keep.sum()))


def _in(i, j, k, lo, hi):
    return (i >= lo[0]) & (i < hi[0]) & (j >= lo[1]) & (j < hi[1]) & (k >= lo[2]) & (k < hi[2])


def pieces_scene():
    sc = scenes.liquid_box((12.0, 12.0, 12.0), (16, 16, 16))
    return _drop(sc, lambda i, j, k: (_in(i, j, k, (0, 0, 0), (10, 10, 10)) & ~_in(i, j, k, (3, 3, 3), (7, 7, 7)))
                 | _in(i, j, k, (13, 0, 0), (16, 3, 3)) | _in(i, j, k, (13, 13, 13), (16, 16, 16)))


def spray_scene():
    sc = scenes.liquid_box((18.0, 18.0, 16.0), (31, 31, 26))
    return _drop(sc, lambda i, j, k: (i % 5 == 0) & (j % 5 == 0) & (k % 5 == 0))


def scene(name):
    if name == "pieces":
        return pieces_scene()
    if name == "spray":
        return spray_scene()
    return scenes.SCENES["tiny_elastic" if name == "tiny_elastic" else "tiny"]()


def liquid_lattice(sc, spacing_over_h, pad_over_h=1.5):
    """A lattice around the scene's liquid as it was put in (a few steps move it by a small fraction of h), extended by pad_over_h * h
    on every side: more than h past every liquid particle, so the field of the liquid is 0 on its border."""
    cfg = sc["cfg"]
    h = f32(cfg.h)
    sp = h * f32(spacing_over_h)
    pad = h * f32(pad_over_h)
    t = sc["position"][:, 3].astype(np.int32)
    p = sc["position"][t != 3, :3]
    lo, hi = p.min(0).astype(np.float32) - pad, p.max(0).astype(np.float32) + pad
    dims = [int(np.ceil((hi[a] - lo[a]) / sp)) + 1 for a in range(3)]
    return lo, np.array([sp, sp, sp], np.float32), dims


def coarse_lattice(cfg):
    """The third lattice of test_surface.py's test_surface_matches_restatement."""
    h = f32(cfg.h)
    sp, pad = h * f32(0.5), h * f32(1.5)
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - pad
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float32) + pad
    dims = [int(np.ceil((hi[a] - lo[a]) / sp)) + 1 for a in range(3)]
    origin = np.array([cfg.xmin + 2.0, cfg.ymin + 2.0, cfg.zmin + 2.0], np.float32)
    return origin, np.array([sp, sp, sp], np.float32) * f32(1.3), [d // 2 for d in dims]


# name -> (scene name, field, types, iso or None = half the lattice maximum of the field, lattice builder)
CASES = {
    "pieces": ("pieces", "shepard", (1,), 0.5, lambda sc: liquid_lattice(sc, 0.5)),
    "spray": ("spray", "density", (1,), None, lambda sc: liquid_lattice(sc, 0.4)),
    "tiny": ("tiny", "shepard", (1,), 0.5, lambda sc: liquid_lattice(sc, 0.25)),
    "coarse": ("tiny", "shepard", (1, 2, 3), 0.5, lambda sc: coarse_lattice(sc["cfg"])),
    "tiny_elastic": ("tiny_elastic", "shepard", (1, 2), 0.5, lambda sc: liquid_lattice(sc, 0.5)),
}
HOST_CASES = ("pieces", "spray", "tiny", "coarse")  # tiny_elastic is compared on the device only
FIELD_WORD = {"density": 0, "shepard": 1}


def case(name):
    """(scene, field, types, iso, (origin, spacing, dims)) of a case."""
    scene_name, field, types, iso, lattice = CASES[name]
    sc = scene(scene_name)
    return sc, field, types, iso, lattice(sc)


def iso_of(field_lattice, iso):
    """The case's iso value: its own, or half the maximum of the sampled lattice (float32)."""
    return f32(iso) if iso is not None else f32(0.5) * f32(np.max(field_lattice))


def reference_mesh(state, field, types, iso, lattice):
    """(vertices, triangles, iso used) of the restatements on a sorted state (sample_ref.solver_state's dict)."""
    origin, spacing, dims = lattice
    pts = sample_ref.grid_points(origin, spacing, dims)
    f = sample_ref.sample_reference(state, pts.reshape(-1, 3), types)[:, FIELD_WORD[field]].reshape(dims[2], dims[1], dims[0])
    iso = iso_of(f, iso)
    v, t = surface_ref.surface_reference(f, origin, spacing, iso)
    return v, t, iso
