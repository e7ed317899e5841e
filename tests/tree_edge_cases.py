"""The scenes of the chunk-edge tests of the reduction tree (tests/test_tree_edges_host.py on the oracle, tests/test_tree_edges.py on
the GPU): a liquid box of exactly 1024 and of exactly 1025 particles -- 640 of the boundary shell, the rest the first liquid
particles of a 9 x 5 x 9 lattice with seeded velocities -- whose floor's lower-x half is a body lifted to just under the liquid, so
that the wall and body trees have non-zero terms from the first step. Inputs only."""
import numpy as np

import body_dyn_ref as bd
import diag_ref
import gauge_cases as gc
import scenes
from sphmi import frames

f32 = np.float32
SIZES = (1024, 1025)
SLOT = 5            # the body
FIELD_SLOT = 2
TYPES = (1, 2, 3)   # with the shell, so that every region below holds particles
GAUGE_SLOTS = (7, 14)  # of gauge_cases.gauges_of: the tilted parallelogram and a diagonal plane; both are crossed both ways
LATTICE = (9, 5, 9)


def scene(n):
    sc = scenes.liquid_box((6.0, 5.0, 6.0), LATTICE, spacing_in_r0=0.85)
    liquid = sc["numOfLiquidP"]
    keep = n - sc["numOfBoundaryP"]
    assert 0 < keep <= liquid
    cfg = type(sc["cfg"]).from_buffer_copy(sc["cfg"])
    cfg.particleCount = n
    cut = lambda a: np.ascontiguousarray(np.concatenate([a[:keep], a[liquid:]]))  # noqa: E731
    sc = dict(sc, cfg=cfg, position=cut(sc["position"]), velocity=cut(sc["velocity"]), numOfLiquidP=keep)
    assert sc["position"].shape[0] == n
    return gc.seeded(sc)


def floor_half(cfg):
    """The floor's boundary particles with x below the middle of the box."""
    return (-np.inf, -np.inf, -np.inf, f32(0.5) * f32(cfg.xmax), f32(cfg.r0), np.inf)


def lift(cfg):
    return frames.pose_translate((0.0, 2.4 * float(f32(cfg.r0)), 0.0))  # the floor lies at 0.5 r0, the liquid stands from 3 r0


def gauges(sc):
    g = gc.gauges_of(sc, (1,))
    return {slot: g[slot] for slot in GAUGE_SLOTS}


def regions(cfg, count):
    """Everything, then slabs of an eighth of the box across x (eight) and across z (seven): each holds part of the shell."""
    inf = np.inf
    out = [diag_ref.EVERYTHING]
    for axis, size, slabs in ((0, f32(cfg.xmax), 8), (2, f32(cfg.zmax), 7)):
        for k in range(slabs):
            lo, hi = [-inf] * 3, [inf] * 3
            lo[axis], hi[axis] = size * f32(k) / f32(8), size * f32(k + 1) / f32(8)
            out.append(tuple(lo) + tuple(hi))
    return np.array(out[:count], np.float32)


def field(n):
    """A carried field in original-id order with zeros of both signs, so that the tagged count is not the particle count."""
    c = np.linspace(-0.5, 1.5, n, dtype=np.float32)
    c[::7] = 0
    c[3::11] = f32(-0.0)
    return c


def dynamics(cfg, ref_pos):
    """The state of a body of equal point masses of cfg.mass at ref_pos (its reference placement), standing at the lift."""
    m = ref_pos.shape[0] * float(f32(cfg.mass))
    com, _, jinv = frames.body_mass_properties(ref_pos, m)
    t = np.asarray(lift(cfg), np.float64).reshape(3, 4)[:, 3]
    return bd.make_state(m, com=com, position=com + t, inertiaInv=jinv, gravity=(cfg.gravity_x, cfg.gravity_y, cfg.gravity_z))
