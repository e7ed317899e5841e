"""The scenes, meshes and views the triangle-rendering tests share (tests/test_render_mesh_host.py checks on the CPU, with the
oracle's state and the restatements alone, that they meet the conditions that keep a comparison from being trivially true;
tests/test_render_mesh.py then uses them on the device).

The state of a solver after k steps is, bit for bit, the oracle's (tests/test_gpu_parity.py), so `oracle_state` gives on the CPU
the dict sample_ref.solver_state / diag_ref.state_with_ids give on the device."""
import numpy as np

import diag_ref
import sample_ref
import scenes
import surface_ref
from test_render import make_view, view_cases  # the four views of a state

SIZES = ((96, 64), (131, 67))  # 131 is no multiple of 64: a row's pixels straddle waves
LATTICE_SIDE = 24
ISO = 0.5


def scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


def oracle_state(ora, cfg):
    """The sorted state of the oracle's last completed step, with the keys of diag_ref.state_with_ids, plus "back"."""
    N = ora.N
    pi = ora.buffer("particleIndex").reshape(-1, 2)[:N]
    types = ora.buffer("position").reshape(-1, 4)[:N][pi[:, 1], 3]
    return dict(pos=ora.buffer("sortedPosition").reshape(-1, 4)[:N, :3].copy(), vel=ora.buffer("sortedVelocity").reshape(-1, 4)[:N, :3].copy(),
                rho=ora.buffer("rho")[:N].copy(), p=ora.buffer("pressure")[:N].copy(), types=types, keys=pi[:, 0].copy(),
                G=int(cfg.gridCellCount), h=float(cfg.h), simScale=float(cfg.simulationScale),
                massWpoly6=float(cfg.mass) * float(cfg.Wpoly6Coefficient), ids=pi[:, 1].astype(np.int64),
                back=ora.buffer("particleIndexBack")[:N].astype(np.int64))


def surface_lattice(state, cfg, types=(1,), side=LATTICE_SIDE, pad_in_h=0.75):
    """(origin, spacing, dims) of a lattice of at most `side` points a side around the particles of `types`."""
    sel = diag_ref.selected(state, diag_ref.EVERYTHING, types)
    p = state["pos"][sel].astype(np.float64)
    pad = pad_in_h * float(cfg.h)
    lo, hi = p.min(0) - pad, p.max(0) + pad
    step = float(np.float32((hi - lo).max() / (side - 1)))
    dims = [int(min(side, np.ceil((hi[k] - lo[k]) / step) + 1)) for k in range(3)]
    return [float(np.float32(x)) for x in lo], [step] * 3, dims


def reference_mesh(state, lattice, types=(1,)):
    """The mesh sph_extract_surface returns for the Shepard-0.5 surface on `lattice`, from the restatements."""
    origin, spacing, dims = lattice
    pts = sample_ref.grid_points(origin, spacing, dims)
    f = sample_ref.sample_reference(state, pts.reshape(-1, 3), types)[:, 1].reshape(dims[2], dims[1], dims[0])
    return surface_ref.surface_reference(f, origin, spacing, ISO)


def worm_lattice(state, cfg, side=LATTICE_SIDE):
    """A lattice at half a smoothing length around the low end of the worm's body (its longest axis cut to `side` points): the
    liquid's surface there is the shell's two sides, closed by the end cap and open where the lattice stops."""
    sel = diag_ref.selected(state, diag_ref.EVERYTHING, (2,))
    p = state["pos"][sel].astype(np.float64)
    step = float(np.float32(0.5 * float(cfg.h)))
    lo, hi = p.min(0) - 2 * step, p.max(0) + 2 * step
    dims = []
    for k in range(3):
        n = int(np.ceil((hi[k] - lo[k]) / step)) + 1
        n = min(n, side)
        dims.append(n)
    return [float(np.float32(x)) for x in lo], [step] * 3, dims


def lattice_for(name, state, cfg):
    return worm_lattice(state, cfg) if name == "worm" else surface_lattice(state, cfg)


# the particle radius of a composed case in units of test_render's (half of r0): spheres that reach through the liquid's surface in
# the boxes (the Shepard-0.5 surface lies outside spheres of half r0 around the outermost centres), and spheres small enough to
# leave the membranes between their centres visible on the worm
COMPOSE_RADIUS = {"worm": 0.3}
COMPOSE_RADIUS_DEFAULT = 1.6


def views(name, state, cfg, size):
    """[(view name, mesh view, particle view of a composed case, types, region)]: test_render's four views at `size`, framed on
    the moving matter (for the worm on the part of its body inside worm_lattice: its liquid fills the whole box, and the rest
    of the body reaches out of the image). The two views differ in the radius alone, which sph_render_mesh does not read."""
    frame = state
    if name == "worm":
        origin, spacing, dims = worm_lattice(state, cfg)
        box = list(origin) + [origin[k] + spacing[k] * (dims[k] - 1) for k in range(3)]
        m = diag_ref.selected(state, box, (2,))
        frame = {k: (v[m] if isinstance(v, np.ndarray) and v.shape[:1] == m.shape else v) for k, v in state.items()}
    cases, radius, size = view_cases(frame, cfg, size)
    out = []
    for vname, kw, types, region in cases:
        pk = dict(kw)
        pk.setdefault("radius", COMPOSE_RADIUS.get(name, COMPOSE_RADIUS_DEFAULT) * radius)
        out.append((vname, make_view(kw, radius, size, colour="type"), make_view(pk, radius, size, colour="type"), types, region))
    return out
