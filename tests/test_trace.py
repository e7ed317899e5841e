"""GPU tests of the integral curves (sph_trace_streamlines / sph_tracers_*, include/sphmi.h): vertices, lengths and codes
bit-identical to the numpy float32 restatement of the step (tests/trace_ref.py) and to a host loop over sample_points, independent of
the seeds' order and of the scratch pieces; tracers that follow the streamline and survive steps and edits; read-only on the
solver; the calling rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_ref
import sample_ref
import scenes
import sphmi
import trace_cases as T
import trace_ref as R
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_ORDER = -1, -3
MODES = {R.TIME: "time", R.ARC: "arc"}
INTEGRATORS = {R.EULER: "euler", R.MIDPOINT: "midpoint"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_streamlines(hip, seeds, types=(1,), step=1.0, mode=R.ARC, integrator=R.MIDPOINT, max_steps=32, min_speed=0.0, region=None):
    return hip.streamlines(seeds, types, step=step, mode=MODES[mode], integrator=INTEGRATORS[integrator], max_steps=max_steps,
                           min_speed=min_speed, region=region)


def assert_curves(got, want, what):
    (gv, gl, gs), (wv, wl, ws) = got, want
    assert gv.dtype == np.float32 and gl.dtype == np.int32 and gs.dtype == np.int32 and gv.shape == wv.shape, what
    assert np.array_equal(gl, wl), "%s: lengths differ at %s" % (what, np.flatnonzero(gl != wl)[:8])
    assert np.array_equal(gs, ws), "%s: status differs at %s: %s vs %s" % (what, np.flatnonzero(gs != ws)[:8], gs[gs != ws][:8], ws[gs != ws][:8])
    if not np.array_equal(bits(gv), bits(wv)):
        bad = np.argwhere((bits(gv) != bits(wv)).any(axis=-1))
        c, k = bad[0]
        raise AssertionError("%s: %d vertices differ; first: curve %d vertex %d: %r vs %r" % (what, len(bad), c, k, gv[c, k], wv[c, k]))


class Traced:
    """The tiny scene with the rotation-plus-drift flow after step(0), its state for the restatement, and the seeds."""

    def __init__(self, name="tiny", steps=1):
        self.sc = T.scene(name)
        self.hip = scenes.hip_for(self.sc)
        for it in range(steps):
            self.hip.step(it)
            if self.sc["cfg"].muscleCount and self.sc["elastic"] is not None:
                self.hip.updateMuscleActivityData(sphmi.muscle_signal(it, self.sc["cfg"].muscleCount))
        self.state = sample_ref.solver_state(self.hip)
        self.seeds = T.seeds(self.sc)
        self.h = np.float32(self.sc["cfg"].h)


@pytest.fixture(scope="module")
def tiny():
    t = Traced()
    yield t
    t.hip.close()


def _cases(h, region):
    """(euler, time), (midpoint, time) and (midpoint, arc), each with the liquid alone and with every type; a negative step and
    the region on half of them."""
    dt = T.TIME_STEP
    return {
        "euler-time-liquid": dict(types=(1,), step=dt, mode=R.TIME, integrator=R.EULER),
        "euler-time-all-upstream-region": dict(types=(1, 2, 3), step=-dt, mode=R.TIME, integrator=R.EULER, region=region),
        "midpoint-time-liquid-region": dict(types=(1,), step=dt, mode=R.TIME, integrator=R.MIDPOINT, region=region),
        "midpoint-time-all-upstream": dict(types=(1, 2, 3), step=-dt, mode=R.TIME, integrator=R.MIDPOINT),
        "midpoint-arc-liquid-upstream": dict(types=(1,), step=-h / np.float32(2), mode=R.ARC, integrator=R.MIDPOINT),
        "midpoint-arc-all-region-minspeed": dict(types=(1, 2, 3), step=h / np.float32(3), mode=R.ARC, integrator=R.MIDPOINT, region=region,
                                                 min_speed=np.float32(1.5) * np.float32(T.DRIFT)),
    }


CASE_NAMES = sorted(_cases(np.float32(1), None))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_streamlines_match_restatement(tiny, case):
    kw = _cases(tiny.h, T.region(tiny.sc))[case]
    got = gpu_streamlines(tiny.hip, tiny.seeds, max_steps=32, **kw)
    want = R.streamlines(tiny.state, tiny.seeds, max_steps=32, **kw)
    assert_curves(got, want, case)
    assert got[0].shape == (tiny.seeds.shape[0], 33, 4) and (got[1] > 8).sum() > 100
    # the far seeds and the NaN seed: one vertex, the seed itself, speed 0
    assert got[1][-3:].tolist() == [1, 1, 1] and got[2][-3:].tolist() == [R.LEFT_MATTER, R.LEFT_MATTER, R.NONFINITE]
    assert np.array_equal(bits(got[0][-3:, 0, :3]), bits(tiny.seeds[-3:])) and not bits(got[0][-3:, 0, 3]).any()


def test_seed_set_shows_every_stop_code_and_long_curves(tiny):
    """The condition the seeds were chosen under (tests/test_trace_host.py checks it on a synthetic state), on the solver's state."""
    kw = T.census(tiny.sc)
    got = gpu_streamlines(tiny.hip, tiny.seeds, **kw)
    assert T.census_holds(got[1], got[2]), (np.bincount(got[2], minlength=6), int((got[1] > 8).sum()))
    assert_curves(got, R.streamlines(tiny.state, tiny.seeds, **kw), "census")


def test_streamlines_on_every_particle_kind_after_five_steps():
    t = Traced("tiny_elastic", steps=5)
    assert (t.state["types"].astype(np.int32) == 2).any() and t.sc["cfg"].muscleCount > 0
    pos = t.hip.read_position_buffer()
    elastic = pos[pos[:, 3].astype(np.int32) == 2][:, :3]
    seeds = np.concatenate([t.seeds, elastic[::3]]).astype(np.float32)
    for name, kw, long_curves in (("arc", dict(types=(1, 2, 3), step=t.h / np.float32(2), mode=R.ARC, integrator=R.MIDPOINT), 100),
                                  ("elastic alone", dict(types=(2,), step=t.h / np.float32(4), mode=R.ARC, integrator=R.MIDPOINT), 0),
                                  ("time", dict(types=(1, 2), step=T.TIME_STEP, mode=R.TIME, integrator=R.MIDPOINT), 100)):
        got = gpu_streamlines(t.hip, seeds, max_steps=16, **kw)
        assert_curves(got, R.streamlines(t.state, seeds, max_steps=16, **kw), "tiny_elastic " + name)
        assert (got[1] > 4).sum() >= long_curves, name
    t.hip.close()


def test_streamlines_through_aliased_cells():
    """alias16: runs of masked keys mix far-apart cells; a short maxSteps keeps the restatement's search over 105 k particles cheap."""
    sc = T.scene("alias16")
    assert sc["cfg"].cellIdMask == 0xffff and sc["cfg"].gridCellCount > 65536
    hip = scenes.hip_for(sc)
    hip.step(0)
    state = sample_ref.solver_state(hip)
    seeds = T.seeds(sc)
    h = np.float32(sc["cfg"].h)
    for kw in (dict(types=(1, 2, 3), step=h / np.float32(2), mode=R.ARC, integrator=R.MIDPOINT),
               dict(types=(1,), step=-h / np.float32(4), mode=R.ARC, integrator=R.EULER)):
        got = gpu_streamlines(hip, seeds, max_steps=6, **kw)
        assert_curves(got, R.streamlines(state, seeds, max_steps=6, **kw), "alias16")
        assert (got[1] == 7).sum() > 100
    hip.close()


def test_euler_curve_is_the_host_loop_over_sample_points(tiny):
    """Tied to the existing API without numpy sums: vertex 1 = seed + step * sample_points(seed)[2:5] in float32, and the whole
    Euler curve equals the same step with the solver's own sample_points as velocity(p)."""
    step = T.TIME_STEP
    for types in ((1,), (1, 2, 3)):
        got = gpu_streamlines(tiny.hip, tiny.seeds, types, step, R.TIME, R.EULER, max_steps=32)
        rec = tiny.hip.sample_points(tiny.seeds, types)
        moved = got[1] > 1
        assert moved.sum() > 250
        want1 = tiny.seeds[moved] + step * rec[moved, 2:5]
        assert np.array_equal(bits(got[0][moved, 1, :3]), bits(want1))
        u = rec[:, 2:5]
        s = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
        assert np.array_equal(bits(got[0][moved, 0, 3]), bits(s[moved]))
        loop = R.streamlines(lambda p, ty: tiny.hip.sample_points(p, ty), tiny.seeds, types, step, R.TIME, R.EULER, max_steps=32)
        assert_curves(got, loop, "host loop %s" % (types,))
    # the midpoint rule through the same loop
    kw = dict(types=(1,), step=tiny.h / np.float32(2), mode=R.ARC, integrator=R.MIDPOINT, max_steps=8)
    assert_curves(gpu_streamlines(tiny.hip, tiny.seeds, **kw), R.streamlines(lambda p, ty: tiny.hip.sample_points(p, ty), tiny.seeds, **kw),
                  "host loop, midpoint")


def test_results_do_not_depend_on_the_seeds_order_or_number(tiny):
    kw = dict(T.census(tiny.sc))
    base = gpu_streamlines(tiny.hip, tiny.seeds, **kw)
    assert tiny.seeds.shape[0] % 64 != 0
    perm = np.random.default_rng(8).permutation(tiny.seeds.shape[0])
    got = gpu_streamlines(tiny.hip, tiny.seeds[perm], **kw)
    assert_curves(got, tuple(a[perm] for a in base), "permuted seeds")
    for pick in ([17], [298, 3], list(range(64)), list(range(65))):
        assert_curves(gpu_streamlines(tiny.hip, tiny.seeds[pick], **kw), tuple(a[pick] for a in base), "%d seeds" % len(pick))
    v, l, s = gpu_streamlines(tiny.hip, np.zeros((0, 3), np.float32), **kw)
    assert v.shape == (0, 33, 4) and l.shape == (0,) and s.shape == (0,)


def test_a_call_in_several_scratch_pieces_equals_two_calls(tiny):
    """The largest maxSteps makes a curve 1 MiB of scratch: 70 seeds do not fit one 64 MiB piece. Euler steps in time of a length
    that carries every curve out of the matter within a few vertices keep it cheap."""
    seeds = tiny.seeds[:70]
    kw = dict(types=(1,), step=np.float32(20) * T.TIME_STEP, mode=R.TIME, integrator=R.EULER, max_steps=sphmi.TRACE_MAX_STEPS_LIMIT)
    v, l, s = gpu_streamlines(tiny.hip, seeds, **kw)
    assert v.shape == (70, 65536, 4) and v.nbytes > (64 << 20)
    assert l.max() < 200 and (s == R.LEFT_MATTER).all() and l.min() >= 2
    a = gpu_streamlines(tiny.hip, seeds[:33], **kw)
    b = gpu_streamlines(tiny.hip, seeds[33:], **kw)
    assert np.array_equal(l, np.concatenate([a[1], b[1]])) and np.array_equal(s, np.concatenate([a[2], b[2]]))
    assert np.array_equal(bits(v[:33]), bits(a[0])) and np.array_equal(bits(v[33:]), bits(b[0]))
    short = gpu_streamlines(tiny.hip, seeds, **dict(kw, max_steps=255))
    assert np.array_equal(bits(v[:, :256]), bits(short[0])) and not bits(v[:, 256:]).any()


def _tracer_kw(kw):
    return dict(types=kw["types"], step=kw["step"], mode=MODES[kw["mode"]], integrator=INTEGRATORS[kw["integrator"]],
                min_speed=kw.get("min_speed", 0.0), region=kw.get("region"))


def test_tracers_follow_the_streamline_of_the_frozen_field(tiny):
    K = 7
    for kw in (T.census(tiny.sc), dict(types=(1, 2, 3), step=T.TIME_STEP, mode=R.TIME, integrator=R.EULER)):
        kw = {k: v for k, v in kw.items() if k != "max_steps"}
        curves = gpu_streamlines(tiny.hip, tiny.seeds, max_steps=K, **kw)
        tiny.hip.tracers_set(tiny.seeds)
        pos, st, steps = tiny.hip.tracers()
        assert np.array_equal(bits(pos[:, :3]), bits(tiny.seeds)) and not bits(pos[:, 3]).any() and not st.any() and not steps.any()
        want = (pos, st, steps)
        for k in range(K):
            moving, stopped = tiny.hip.tracers_advect(**_tracer_kw(kw))
            want = R.tracers_advect(tiny.state, *want, **kw)
            got = tiny.hip.tracers()
            assert moving == (got[1] == R.MOVING).sum() and moving + stopped == tiny.seeds.shape[0]
            for g, w, name in zip(got, want, ("position", "status", "steps")):
                assert np.array_equal(bits(g), bits(w)), "advect %d: %s" % (k, name)
        T.tracers_match_streamlines(*got, *curves, K)
        assert (got[1] == R.MOVING).sum() > 100 and (got[1] != R.MOVING).sum() > 10
    tiny.hip.tracers_set(None)


def test_tracers_survive_steps_and_edits():
    t = Traced()
    hip = t.hip
    kw = dict(types=(1,), step=T.TIME_STEP, mode=R.TIME, integrator=R.MIDPOINT)
    hip.tracers_set(t.seeds)
    hip.tracers_advect(**_tracer_kw(kw))
    before = hip.tracers()
    assert np.array_equal(bits(before[0]), bits(R.tracers_advect(t.state, *_fresh(t.seeds), **kw)[0]))
    hip.step(1)
    pos = hip.read_position_buffer()
    vel = hip.read_velocity_buffer()
    box = edit_ref.liquid_quantile_box(pos)
    marks = edit_ref.region_marks(pos, box, (1,))
    assert hip.remove_region(box, (1,)) == marks.sum() > 0
    assert hip.add_particles(pos[marks], vel[marks]) == pos.shape[0]
    for g, b in zip(hip.tracers(), before):
        assert np.array_equal(bits(g), bits(b)), "a step, a removal and an addition left the tracers alone"
    with pytest.raises(sphmi.SphError) as e:  # the edit invalidated the sorted state: as every analysis call, until the next step
        hip.tracers_advect(**_tracer_kw(kw))
    assert scenes.error_status(e) == ERR_ORDER
    hip.step(2)
    for g, b in zip(hip.tracers(), before):
        assert np.array_equal(bits(g), bits(b))
    hip.tracers_advect(**_tracer_kw(kw))
    want = R.tracers_advect(sample_ref.solver_state(hip), *before, **kw)
    got = hip.tracers()
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    assert got[2].max() == 2 and (got[1] == R.MOVING).sum() > 100
    # count 0 releases them
    hip.tracers_set(np.zeros((0, 3), np.float32))
    for call in (lambda: hip.tracers_advect(**_tracer_kw(kw)), hip.tracers):
        with pytest.raises(sphmi.SphError) as e:
            call()
        assert scenes.error_status(e) == ERR_ORDER
    hip.tracers_set(t.seeds[:5])
    assert hip.tracers()[0].shape == (5, 4)
    hip.close()


def _fresh(seeds):
    pos = np.zeros((seeds.shape[0], 4), np.float32)
    pos[:, :3] = seeds
    return pos, np.zeros(seeds.shape[0], np.int32), np.zeros(seeds.shape[0], np.int32)


def test_tracing_is_read_only():
    """A solver that traces and advects every step ends bit-identical to an untouched twin (the buffers test_sample.py's
    read-only test checks), step by step."""
    sc = T.scene("tiny_elastic")
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    seeds = T.seeds(sc)
    h = np.float32(sc["cfg"].h)
    a.tracers_set(seeds)
    buf = np.empty(4 * a.N, np.float32)
    for it in range(6):
        a.step(it)
        b.step(it)
        a.read_position_buffer_async(buf)
        a.streamlines(seeds, (1, 2, 3), step=h / 2, max_steps=16)
        a.tracers_advect((1, 2), dt=sc["cfg"].timeStep)
        a.wait_position_buffer()
        assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer())), it
        assert np.array_equal(bits(a.read_velocity_buffer()), bits(b.read_velocity_buffer())), it
        assert np.array_equal(bits(a.read_density_buffer()), bits(b.read_density_buffer())), it
    assert a.tracers()[2].max() == 6
    a.close()
    b.close()


def _params(step=0.5, min_speed=0.0, max_steps=8, mode=R.ARC, integrator=R.MIDPOINT):
    return sphmi.SphTraceParams(step, min_speed, max_steps, mode, integrator)


def _rc_stream(hip, prm, mask=0x2, count=4, seeds=True, region=None):
    p = np.zeros((max(count, 1), 4), np.float32)
    m = max(prm.maxSteps, 0) if prm is not None else 0
    v = np.zeros((max(count, 1), min(m, 65535) + 1, 4), np.float32)
    ln = np.zeros(max(count, 1), np.int32)
    st = np.zeros(max(count, 1), np.int32)
    rg = None if region is None else np.ascontiguousarray(region, np.float32)
    return hip._L.sph_trace_streamlines(hip._h, p.ctypes.data if seeds else None, count, mask, C.byref(prm) if prm is not None else None,
                                        None if rg is None else rg.ctypes.data, v.ctypes.data, ln.ctypes.data, st.ctypes.data)


def _rc_advect(hip, prm, mask=0x2, region=None):
    counts = np.zeros(2, np.int64)
    rg = None if region is None else np.ascontiguousarray(region, np.float32)
    return hip._L.sph_tracers_advect(hip._h, mask, C.byref(prm) if prm is not None else None, None if rg is None else rg.ctypes.data,
                                     counts.ctypes.data)


def test_calling_rules():
    sc = T.scene()
    hip = scenes.hip_for(sc)
    twin = scenes.hip_for(sc)
    assert _rc_stream(hip, _params()) == ERR_ORDER  # before the first step
    hip.tracers_set(np.zeros((3, 3), np.float32))  # (setting needs no step)
    assert _rc_advect(hip, _params()) == ERR_ORDER
    hip.step(0)
    twin.step(0)
    assert _rc_stream(hip, _params()) == 0 and _rc_advect(hip, _params()) == 0
    bad = [_params(max_steps=-1), _params(max_steps=65536), _params(mode=2), _params(mode=-1), _params(integrator=2),
           _params(integrator=-1), _params(min_speed=-0.5), _params(min_speed=float("nan")), _params(step=0.0),
           _params(step=float("inf")), _params(step=float("nan"))]
    for prm in bad:
        assert _rc_stream(hip, prm) == ERR_INVALID, (prm.step, prm.minSpeed, prm.maxSteps, prm.mode, prm.integrator)
        assert b"sph_trace_streamlines" in hip._L.sph_last_error()
    for prm in bad[2:]:  # (maxSteps is not read by an advect)
        assert _rc_advect(hip, prm) == ERR_INVALID
    assert _rc_advect(hip, bad[0]) == 0
    assert _rc_stream(hip, _params(max_steps=0)) == 0 and _rc_stream(hip, _params(max_steps=65535), count=1) == 0
    for mask in (0, 1, 0x10, 0x80000002):
        assert _rc_stream(hip, _params(), mask=mask) == ERR_INVALID and _rc_advect(hip, _params(), mask=mask) == ERR_INVALID
    assert _rc_stream(hip, None) == ERR_INVALID and _rc_advect(hip, None) == ERR_INVALID
    assert _rc_stream(hip, _params(), count=-1) == ERR_INVALID and _rc_stream(hip, _params(), seeds=False) == ERR_INVALID
    assert _rc_stream(hip, _params(), count=0, seeds=False) == 0
    nan_box = (0, 0, np.nan, 1, 1, 1)
    assert _rc_stream(hip, _params(), region=nan_box) == ERR_INVALID and _rc_advect(hip, _params(), region=nan_box) == ERR_INVALID
    assert hip._L.sph_tracers_set(hip._h, None, 3) == ERR_INVALID and hip._L.sph_tracers_set(hip._h, None, -1) == ERR_INVALID
    with pytest.raises(sphmi.SphError):
        hip.streamlines(np.zeros((2, 3), np.float32), step=1.0, mode="sideways")
    with pytest.raises(sphmi.SphError):
        hip.streamlines(np.zeros((2, 3), np.float32), dt=1e-5, mode="arc")
    # dt is seconds: dt / simulationScale scene units per unit of velocity
    kw = dict(types=(1,), integrator="euler", max_steps=4)
    a = hip.streamlines(T.seeds(sc), mode="time", dt=sc["cfg"].timeStep, **kw)
    b = hip.streamlines(T.seeds(sc), mode="time", step=np.float32(sc["cfg"].timeStep) / np.float32(sc["cfg"].simulationScale), **kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and (a[1] == 5).sum() > 100
    # a new step has begun: as sampling
    hip._runClearBuffers()
    hip._runHashParticles()
    assert _rc_stream(hip, _params()) == ERR_ORDER and _rc_advect(hip, _params()) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[2:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    twin.step(1)
    assert _rc_stream(hip, _params()) == 0
    hip.step(2)
    twin.step(2)
    assert np.array_equal(bits(hip.read_position_buffer()), bits(twin.read_position_buffer()))
    hip.close()
    twin.close()


def test_tracing_a_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    hip.tracers_set(np.zeros((3, 3), np.float32))
    assert _rc_stream(hip, _params()) == ERR_INVALID and _rc_advect(hip, _params()) == ERR_INVALID
    hip.close()


def test_cpp_driver_streamlines_and_tracers(tmp_path):
    """sphmi_run --streamlines / --tracers: the polyline files equal streamlines() of a Python solver on the same scene after the
    same steps, and the tracer counts those of tracers_advect."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--quiet", "--streamlines", "7", "5",
                        "--stream-every", "2", "--stream-out", str(tmp_path), "--stream-max-steps", "12", "--tracers", "6", "4",
                        "--tracers-every", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = scenes.SCENES["tiny"]()
    cfg = sc["cfg"]
    f = np.float32

    def plane(nu, nv):
        dx, dz = (f(cfg.xmax) - f(cfg.xmin)) / f(nu), (f(cfg.zmax) - f(cfg.zmin)) / f(nv)
        return frames.seed_plane((f(cfg.xmin) + f(0.5) * dx, f(0.5) * (f(cfg.ymin) + f(cfg.ymax)), f(cfg.zmin) + f(0.5) * dz),
                                 (dx, 0, 0), (0, 0, dz), nu, nv)

    hip = scenes.hip_for(sc)
    hip.tracers_set(plane(6, 4))
    lines = re.findall(r"tracers step=(\d+) moving=(\d+) stopped=(\d+)", r.stdout)
    assert [int(l[0]) for l in lines] == [2, 4]
    for it in range(4):
        hip.step(it)
        counts = hip.tracers_advect((1,), dt=cfg.timeStep)
        if (it + 1) % 2 == 0:
            assert counts == tuple(int(w) for w in lines[(it + 1) // 2 - 1][1:])
            v, l, s = hip.streamlines(plane(7, 5), (1, 2), step=f(0.5) * f(cfg.h), max_steps=12)
            points, lengths, speed = frames.read_polylines(str(tmp_path / ("streamlines_%d.vtk" % (it + 1))))
            keep = np.arange(13)[None, :] < l[:, None]
            assert np.array_equal(lengths, l)
            assert np.array_equal(bits(points), bits(v[..., :3][keep])) and np.array_equal(bits(speed), bits(v[..., 3][keep]))
    hip.close()
    assert sorted(os.listdir(tmp_path)) == ["streamlines_2.vtk", "streamlines_4.vtk"]
