"""The scene, the seeds and the parameter sets that the integral-curve tests share (tests/test_trace.py on the GPU,
tests/test_trace_host.py on a synthetic state of the same scene). Inputs only."""
import numpy as np

import scenes
import trace_ref as R

# The flow: a rigid rotation about the box's vertical axis (along z through the box centre) and an axial drift. Velocities are in
# m/s and a step moves a particle by v * timeStep / simulationScale (~2.5 scene units per unit of velocity): slow enough that
# the scenes stay calm over the few steps the tests take.
OMEGA, DRIFT = 1.0e-3, 5.0e-4
TIME_STEP = np.float32(80.0)  # a step of mode "time" that moves a curve by ~0.5 scene units at the flow's speeds


def flow(points, centre):
    """float32[n, 3] velocity of the rotation-plus-drift field about the axis through `centre` (x, y) at `points`."""
    p = np.asarray(points, np.float32)
    v = np.empty((p.shape[0], 3), np.float32)
    v[:, 0] = -np.float32(OMEGA) * (p[:, 1] - np.float32(centre[1]))
    v[:, 1] = np.float32(OMEGA) * (p[:, 0] - np.float32(centre[0]))
    v[:, 2] = np.float32(DRIFT)
    return v


def box_centre(cfg):
    return np.array([0.5 * (cfg.xmin + cfg.xmax), 0.5 * (cfg.ymin + cfg.ymax), 0.5 * (cfg.zmin + cfg.zmax)], np.float32)


def scene(name="tiny"):
    """A copy of scenes.SCENES[name]() whose liquid starts with the flow as its velocity: step(0) sorts it into the state that
    sampling reads (the sorted state holds the velocities of before the step's integration)."""
    sc = dict(scenes.SCENES[name]())
    vel = np.array(sc["velocity"], np.float32).reshape(-1, 4)
    pos = np.asarray(sc["position"], np.float32).reshape(-1, 4)
    liquid = pos[:, 3].astype(np.int32) == 1
    vel[liquid, :3] = flow(pos[liquid, :3], box_centre(sc["cfg"]))
    sc["velocity"] = vel
    return sc


def synthetic_state(sc):
    """A sample_ref state made of the scene's input alone (rest density, no pressure, every key inside the table): what the seeds
    and parameters below are chosen on without a GPU."""
    cfg = sc["cfg"]
    pos = np.asarray(sc["position"], np.float32).reshape(-1, 4)
    n = pos.shape[0]
    return dict(pos=pos[:, :3].copy(), vel=np.asarray(sc["velocity"], np.float32).reshape(-1, 4)[:, :3].copy(),
                rho=np.full(n, cfg.rho0, np.float32), p=np.zeros(n, np.float32), types=pos[:, 3].copy(), keys=np.zeros(n, np.uint32),
                G=1, h=float(cfg.h), simScale=float(cfg.simulationScale), massWpoly6=float(cfg.mass) * float(cfg.Wpoly6Coefficient))


def seeds(sc, rng=None):
    """300 seeds: a 16 x 16 seed_plane through the liquid, the axis point, 40 points just outside the liquid within h of it, two
    far points and a NaN point (the last three)."""
    from sphmi import frames
    cfg = sc["cfg"]
    rng = np.random.default_rng(34) if rng is None else rng
    pos = np.asarray(sc["position"], np.float32).reshape(-1, 4)
    liq = pos[pos[:, 3].astype(np.int32) == 1][:, :3]
    lo, hi = liq.min(0), liq.max(0)
    c = box_centre(cfg)
    inset = np.float32(1.0)
    zmid = np.float32(0.5) * (lo[2] + hi[2]) + np.float32(0.3)
    plane = frames.seed_plane((lo[0] + inset, lo[1] + inset, zmid), ((hi[0] - lo[0] - 2 * inset) / np.float32(15), 0, 0),
                              (0, (hi[1] - lo[1] - 2 * inset) / np.float32(15), 0), 16, 16)
    axis = np.array([[c[0], c[1], zmid]], np.float32)
    h = np.float32(cfg.h)
    near = rng.uniform(lo, hi, (40, 3)).astype(np.float32)
    face = rng.integers(0, 3, 40)
    side = rng.integers(0, 2, 40)
    depth = rng.uniform(0.05, 0.9, 40).astype(np.float32) * h
    for k in range(40):
        near[k, face[k]] = lo[face[k]] - depth[k] if side[k] == 0 else hi[face[k]] + depth[k]
    far = np.array([[cfg.xmax + 10 * h, cfg.ymax + 10 * h, cfg.zmax + 10 * h], [cfg.xmin - 7 * h, c[1], c[2]]], np.float32)
    nan = np.array([[np.nan, c[1], c[2]]], np.float32)
    return np.concatenate([plane, axis, near, far, nan]).astype(np.float32)


def region(sc):
    """A box that cuts the rotation: everything with x below a plane 6 units beyond the axis."""
    c = box_centre(sc["cfg"])
    return np.array([-np.inf, -np.inf, -np.inf, c[0] + 6.0, np.inf, np.inf], np.float32)


def census(sc):
    """The parameters under which the seeds must show every stop code, and at least half of the curves more than 8 vertices."""
    return dict(types=(1,), step=np.float32(sc["cfg"].h) / np.float32(4), mode=R.ARC, integrator=R.MIDPOINT, max_steps=32,
                min_speed=np.float32(1.5) * np.float32(DRIFT), region=region(sc))


def census_holds(lengths, status):
    codes = set(int(s) for s in status)
    return codes == {R.MAX_STEPS, R.LEFT_MATTER, R.LEFT_REGION, R.STAGNANT, R.NONFINITE} and 2 * int((lengths > 8).sum()) >= len(lengths)


def tracers_match_streamlines(pos, st, steps, verts, lengths, status, K):
    """K advects against the streamlines of the same seeds with maxSteps = K: a curve that reached vertex K is a tracer still
    moving there after K steps; one that stopped earlier is a tracer at its last vertex with its code."""
    moving = lengths == K + 1
    at = np.where(moving, K, lengths - 1)
    idx = np.arange(len(at))
    assert np.array_equal(pos[:, :3].view(np.uint32), verts[idx, at, :3].view(np.uint32))
    assert np.array_equal(st, np.where(moving, R.MOVING, status))
    assert np.array_equal(steps, np.where(moving, K, lengths))
    last_sampled = np.where(moving, K - 1, lengths - 1)
    assert np.array_equal(pos[:, 3].view(np.uint32), verts[idx, last_sampled, 3].view(np.uint32))
