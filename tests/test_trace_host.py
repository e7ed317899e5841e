"""CPU checks of the integral curves: the numpy restatement of the step (tests/trace_ref.py) against float64 single steps, its
stop codes, lengths and zero fill, the seed set the GPU test uses, and the seed and polyline helpers of sphmi/frames.py. No GPU
needed."""
import os

import numpy as np
import pytest

import sample_ref
import scenes
import sphmi
import trace_cases as T
import trace_ref as R
from sphmi import frames
from test_sample_host import _cloud

L = 20.0
AXIS = (L / 2, L / 2)
AXIAL = 0.5  # the drift of the synthetic cloud's flow


def _rotating_cloud():
    """test_sample_host's cloud with a rigid rotation about the box axis plus a small axial drift as its velocities."""
    state, rng = _cloud()
    pos = state["pos"]
    vel = np.empty_like(pos)
    vel[:, 0] = -(pos[:, 1] - np.float32(AXIS[1]))
    vel[:, 1] = pos[:, 0] - np.float32(AXIS[0])
    vel[:, 2] = np.float32(AXIAL)
    state["vel"] = vel
    return state, rng


def _velocity_f64(state, pts, types):
    rec = sample_ref.brute_force_f64(state["pos"], state["vel"], state["rho"], state["p"], state["types"], pts,
                                     float(np.float32(state["h"])), float(np.float32(state["simScale"])),
                                     float(np.float32(state["massWpoly6"])), types)
    return rec[:, 1] != 0, rec[:, 2:5]


@pytest.mark.parametrize("integrator,mode,step", [(R.EULER, R.TIME, 0.05), (R.MIDPOINT, R.TIME, 0.05), (R.MIDPOINT, R.ARC, 0.8),
                                                  (R.MIDPOINT, R.ARC, -0.8)])
def test_every_step_agrees_with_the_same_step_in_float64(integrator, mode, step):
    """Each vertex k + 1 of a restated float32 curve against the step redone in float64 from that curve's own vertex k."""
    state, rng = _rotating_cloud()
    types = (1, 2, 3)
    seeds = rng.uniform(5, 15, (40, 3)).astype(np.float32)
    verts, lengths, status = R.streamlines(state, seeds, types, step, mode, integrator, max_steps=12)
    assert (lengths == 13).sum() > 30 and set(status) <= {R.MAX_STEPS, R.LEFT_MATTER}
    k = np.arange(12)[None, :] < (lengths[:, None] - 1)  # steps that were taken
    p = verts[:, :12, :3][k].astype(np.float64)
    got = verts[:, 1:, :3][k]
    hit, u = _velocity_f64(state, p, types)
    assert hit.all()
    s = np.sqrt((u * u).sum(1))
    c = step / s if mode == R.ARC else np.full(s.shape, step)
    if integrator == R.EULER:
        want = p + c[:, None] * u
    else:
        q = p + (0.5 * c)[:, None] * u
        hit2, u2 = _velocity_f64(state, q, types)
        assert hit2.all()
        s2 = np.sqrt((u2 * u2).sum(1))
        c2 = step / s2 if mode == R.ARC else np.full(s.shape, step)
        want = p + c2[:, None] * u2
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # the speed written with a vertex is the float64 speed there
    np.testing.assert_allclose(verts[:, :12, 3][k], s, rtol=1e-5)
    if mode == R.ARC and integrator == R.EULER:
        np.testing.assert_allclose(np.sqrt(((got - p) ** 2).sum(1)), abs(step), rtol=1e-4)


def test_every_stop_code_from_a_seed_chosen_for_it():
    state, _ = _rotating_cloud()
    seeds = np.array([[1e4, 1e4, 1e4],              # far from everything
                      [np.nan, 10.0, 10.0],         # not a point
                      [10.0 + 4.0, 10.0, 10.0],     # rotates out of the region
                      [AXIS[0], AXIS[1], 10.0],     # on the axis: only the drift
                      [10.0 + 2.0, 10.0, 10.0]],    # goes round inside the region
                     np.float32)
    region = (-np.inf, -np.inf, -np.inf, np.inf, 10.0 + 3.0, np.inf)  # y <= 13 cuts the circle of radius 4, not that of radius 2
    verts, lengths, status = R.streamlines(state, seeds, (1, 2, 3), step=0.5, mode=R.ARC, integrator=R.MIDPOINT, max_steps=20,
                                           min_speed=AXIAL + 0.4, region=region)
    assert status.tolist() == [R.LEFT_MATTER, R.NONFINITE, R.LEFT_REGION, R.STAGNANT, R.MAX_STEPS]
    assert lengths[0] == 1 and lengths[1] == 1 and lengths[3] == 1 and lengths[4] == 21
    assert 3 < lengths[2] < 21
    assert verts.shape == (5, 21, 4)
    # lengths count the vertices written; the slots behind them are +0; vertex 0 is the seed, bit for bit
    for i in range(5):
        assert not verts[i, lengths[i]:].view(np.uint32).any()
        assert np.array_equal(verts[i, 0, :3].view(np.uint32), seeds[i].view(np.uint32))
    assert verts[0, 0, 3] == 0 and verts[1, 0, 3] == 0  # no hit, not finite: speed 0
    assert abs(verts[3, 0, 3] - AXIAL) < 0.3 and verts[4, :, 3].min() > AXIAL + 0.4
    last = verts[2, lengths[2] - 1]
    assert last[1] > 13.0 and (verts[2, :lengths[2] - 1, 1] <= 13.0).all()  # stopped at the first vertex outside
    # a midpoint that leaves the matter stops the curve without a further vertex
    top = np.array([[AXIS[0] + 0.3, AXIS[1] + 0.2, L + 1.5]], np.float32)  # above the cloud, near the axis: the drift carries it out
    v2, l2, s2 = R.streamlines(state, top, (1, 2, 3), step=6.0, mode=R.ARC, integrator=R.MIDPOINT, max_steps=4)
    e2, le2, se2 = R.streamlines(state, top, (1, 2, 3), step=3.0, mode=R.ARC, integrator=R.EULER, max_steps=4)
    assert se2[0] == R.LEFT_MATTER and le2[0] == 2 and e2[0, 1, 3] == 0  # Euler writes the vertex without a hit ...
    assert s2[0] == R.LEFT_MATTER and l2[0] == 1                         # ... the midpoint rule stops before it
    # maxSteps 0: the seed alone
    v0, l0, s0 = R.streamlines(state, seeds, (1, 2, 3), step=0.5, max_steps=0)
    assert l0.tolist() == [1] * 5 and s0.tolist() == [R.LEFT_MATTER, R.NONFINITE, R.MAX_STEPS, R.MAX_STEPS, R.MAX_STEPS]


def test_tracers_follow_the_streamline():
    state, rng = _rotating_cloud()
    seeds = np.concatenate([rng.uniform(4, 16, (30, 3)), [[1e4, 0, 0], [np.nan, 0, 0], [10.3, 10.2, 21.5]]]).astype(np.float32)
    kw = dict(types=(1, 2), step=0.7, mode=R.ARC, integrator=R.MIDPOINT, min_speed=0.0)
    K = 6
    verts, lengths, status = R.streamlines(state, seeds, max_steps=K, **kw)
    pos = np.zeros((seeds.shape[0], 4), np.float32)
    pos[:, :3] = seeds
    st = np.zeros(seeds.shape[0], np.int32)
    steps = np.zeros(seeds.shape[0], np.int32)
    for _ in range(K):
        pos, st, steps = R.tracers_advect(state, pos, st, steps, **kw)
    T.tracers_match_streamlines(pos, st, steps, verts, lengths, status, K)
    assert (st == R.MOVING).sum() > 20 and (st != R.MOVING).sum() >= 3


def test_gpu_seed_set_meets_its_conditions_on_a_synthetic_state():
    """The seeds and parameters of tests/test_trace.py, on the scene's input with rest densities: every stop code occurs, and at
    least half of the curves have more than 8 vertices (the GPU test asserts the same on the solver's state)."""
    sc = T.scene()
    seeds = T.seeds(sc)
    assert 290 <= seeds.shape[0] <= 310 and np.isnan(seeds[-1, 0]) and np.isfinite(seeds[:-1]).all()
    verts, lengths, status = R.streamlines(T.synthetic_state(sc), seeds, **T.census(sc))
    assert T.census_holds(lengths, status), (np.bincount(status, minlength=6), int((lengths > 8).sum()))
    liquid = np.asarray(sc["position"]).reshape(-1, 4)[:, 3].astype(np.int32) == 1
    v = np.asarray(sc["velocity"]).reshape(-1, 4)
    assert liquid.sum() == sc["numOfLiquidP"] and np.all(v[liquid, 2] == np.float32(T.DRIFT)) and np.abs(v[liquid, 0]).max() > 5 * T.OMEGA


def test_seed_rake_and_seed_plane_layouts():
    r = frames.seed_rake((1.0, 2.0, 3.0), (2.0, 2.0, 0.0), 5)
    assert r.dtype == np.float32 and r.shape == (5, 3)
    d = (np.float32([2.0, 2.0, 0.0]) - np.float32([1.0, 2.0, 3.0])) / np.float32(4)
    assert np.array_equal(r[3], np.float32([1.0, 2.0, 3.0]) + np.float32(3) * d)
    assert r[0].tolist() == [1.0, 2.0, 3.0] and r[4].tolist() == [2.0, 2.0, 0.0]
    assert frames.seed_rake((1.0, 2.0, 3.0), (9.0, 9.0, 9.0), 1).tolist() == [[1.0, 2.0, 3.0]]
    p = frames.seed_plane((0.1, 0.2, 0.3), (0.7, 0.0, 0.1), (0.0, 1.3, 0.0), 4, 3)
    assert p.dtype == np.float32 and p.shape == (12, 3)
    o, du, dv = np.float32([0.1, 0.2, 0.3]), np.float32([0.7, 0.0, 0.1]), np.float32([0.0, 1.3, 0.0])
    for j in range(3):
        for i in range(4):
            want = (o + np.float32(i) * du) + np.float32(j) * dv  # i fastest; one multiply and one add per direction
            assert np.array_equal(p[j * 4 + i].view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        frames.seed_plane((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 3)
    with pytest.raises(ValueError):
        frames.seed_rake((0, 0, 0), (1, 0, 0), 0)


def test_write_vtk_polylines_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    verts = rng.normal(0, 1, (6, 9, 4)).astype(np.float32)
    lengths = np.array([9, 1, 4, 0, 2, 9], np.int32)
    path = str(tmp_path / "curves.vtk")
    assert frames.write_vtk_polylines(path, verts, lengths) == 25
    points, got_lengths, speed = frames.read_polylines(path)
    keep = np.arange(9)[None, :] < lengths[:, None]
    assert np.array_equal(got_lengths, lengths)
    assert np.array_equal(points.view(np.uint32), verts[..., :3][keep].view(np.uint32))
    assert np.array_equal(speed.view(np.uint32), verts[..., 3][keep].view(np.uint32))
    head = open(path, "rb").read(200).split(b"\n")
    assert head[0] == b"# vtk DataFile Version 3.0" and head[2] == b"BINARY" and head[3] == b"DATASET POLYDATA"
    assert head[4] == b"POINTS 25 float"
    # other scalars than the fourth word; vertices without one
    other = rng.normal(0, 1, (6, 9)).astype(np.float32)
    frames.write_vtk_polylines(path, verts[..., :3], lengths, scalars=other)
    assert np.array_equal(frames.read_polylines(path)[2], other[keep])
    with pytest.raises(ValueError):
        frames.write_vtk_polylines(path, verts[..., :3], lengths)
    with pytest.raises(ValueError):
        frames.write_vtk_polylines(path, verts, np.array([10, 1, 1, 1, 1, 1]))
    frames.write_vtk_polylines(path, verts[:0], lengths[:0])
    assert frames.read_polylines(path)[0].shape == (0, 3)


def test_header_and_wrapper_agree_on_the_trace_constants():
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    for name in ("TIME", "ARC", "EULER", "MIDPOINT", "MOVING", "MAX_STEPS", "LEFT_MATTER", "LEFT_REGION", "STAGNANT", "NONFINITE",
                 "MAX_STEPS_LIMIT"):
        assert "#define SPH_TRACE_%s %d\n" % (name, getattr(sphmi, "TRACE_" + name)) in txt, name
        if hasattr(R, name):
            assert getattr(R, name) == getattr(sphmi, "TRACE_" + name)
    assert "#define SPHMI_ABI_VERSION 2" in txt and sphmi.ABI_VERSION == 2  # entry points were added, sph_config is unchanged
    assert [f[0] for f in sphmi.SphTraceParams._fields_] == ["step", "minSpeed", "maxSteps", "mode", "integrator"]
    for s in ("sph_trace_streamlines", "sph_tracers_set", "sph_tracers_advect", "sph_tracers_read"):
        assert s in sphmi.EXPORTED_SYMBOLS
