"""GPU tests of the elastic-matter diagnostics (sph_elastic_measure / sph_muscle_diagnostics / sph_membrane_measure,
include/sphmi.h): every word of the three calls bit-identical to the numpy restatement (tests/elastic_ref.py, which
tests/test_elastic_host.py ties to the oracle's elastic-force stage), after one and after several steps, on the fused and the
staged path, on a synthetic stack of sheets whose group tree has three levels; consistent with themselves and with the existing
exports, read-only, the calling rules, and the driver's files. No tolerance appears anywhere: integers are compared for equality,
floats as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import elastic_ref as er
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
SCENE_NAMES = ["tiny_elastic", "elastic_offset_box", "worm"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scene(name):
    if name == "worm":
        sc = scenes.worm_scene()
        sc["cfg"].muscleCount = 96  # the fixture's muscles are 1..96: every muscle record then has connections
        return sc
    return scenes.elastic_offset_box() if name == "elastic_offset_box" else scenes.SCENES[name]()


def _signal(name, cfg, it):
    """The signal stored before step `it`: the reference's travelling wave on the worm (several groups positive), one active
    muscle on the small sheets."""
    if name == "worm":
        return sphmi.muscle_signal(60 + 25 * it, 100)[:cfg.muscleCount]
    s = np.zeros(cfg.muscleCount, np.float32)
    s[0] = f32(0.25) * f32(it + 1)
    s[1] = f32(-1.0)
    return s


def first_diff(got, want, view):
    d = np.argwhere(view(got) != view(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def check_against_restatement(hip, sc, signal, what, groups=None):
    """All three calls on the solver's current state against the restatement; returns (records, muscle records, totals)."""
    cfg = sc["cfg"]
    E = cfg.numOfElasticP
    sp, back, c = er.solver_inputs(hip, sc, signal)
    assert not c.bad
    idx, ids, rec, con = hip.elastic_measure()
    assert idx.dtype == np.int32 and ids.dtype == np.uint32 and rec.dtype == np.float32 and con.dtype == np.float32
    assert idx.shape == (E,) and ids.shape == (E,) and rec.shape == (E, 12) and con.shape == (E, 32, 2)
    want_idx, want_rec, want_con = er.elastic_records_fast(c)
    assert np.array_equal(idx, want_idx), what
    assert np.array_equal(ids, np.arange(E, dtype=np.uint32) + np.uint32(cfg.elasticOffset)), what
    assert np.array_equal(u32(con), u32(want_con)), "%s connections: %s" % (what, first_diff(con, want_con, u32))
    assert np.array_equal(u32(rec), u32(want_rec)), "%s records: %s" % (what, first_diff(rec, want_rec, u32))
    mus = hip.muscle_diagnostics()
    assert mus.dtype == np.float64 and mus.shape == (cfg.muscleCount + 1, 16)
    want_mus = er.muscle_records(c, cfg.muscleCount, signal, groups)
    rows = np.arange(cfg.muscleCount + 1) if groups is None else np.asarray(sorted(set(groups)))
    assert np.array_equal(u64(mus[rows]), u64(want_mus[rows])), "%s muscles: %s" % (what, first_diff(mus[rows], want_mus[rows], u64))
    totals = None
    if cfg.numOfMembranes > 0:
        tri, totals = hip.membrane_measure()
        want_tri, want_totals = er.membrane_records(sp, back, sc["membranes"])
        assert tri.shape == (cfg.numOfMembranes, 8) and totals.shape == (4,)
        assert np.array_equal(u32(tri), u32(want_tri)), "%s triangles: %s" % (what, first_diff(tri, want_tri, u32))
        assert np.array_equal(u64(totals), u64(want_totals)), (what, totals, want_totals)
        assert np.array_equal(u64(hip.membrane_measure(records=False)[1]), u64(totals))
    return c, (idx, ids, rec, con), mus, totals


def check_consistency(c, measured, mus):
    """The outputs agree with each other: the record's sums recomputed from `connections`, and the counts."""
    idx, ids, rec, con = measured
    live = con[:, :, 0] >= 0
    assert np.array_equal(live, c.live)
    assert np.array_equal(rec[:, 0], live.sum(1).astype(np.float32))
    d2 = np.zeros(rec.shape[0], np.float32)
    for k in range(32):  # ascending slot order
        dr = con[:, k, 1]
        d2 = np.where(live[:, k], d2 + (dr * dr).astype(np.float32), d2).astype(np.float32)
    assert np.array_equal(u32(rec[:, 5]), u32(d2))
    assert (con[~live] == np.array([-1, 0], np.float32)).all()
    assert rec[:, 0].astype(np.float64).sum() == mus[:, 0].sum() == live.sum()
    assert rec[:, 1].astype(np.float64).sum() == mus[1:, 0].sum()
    has = rec[:, 0] > 0
    assert (rec[has, 2] <= rec[has, 3]).all() and mus[mus[:, 0] > 0, 7].min() == rec[has, 2].min() and mus[mus[:, 0] > 0, 8].max() == rec[has, 3].max()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_calls_match_restatement(name):
    """After 1 and after several steps, with the muscle signal changing from step to step."""
    sc = _scene(name)
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    seen_contraction = False
    for it in range(5):
        signal = _signal(name, cfg, it)
        hip.updateMuscleActivityData(signal)
        hip.step(it)
        if it in (0, 2, 4):
            c, measured, mus, totals = check_against_restatement(hip, sc, signal, "%s step %d" % (name, it))
            check_consistency(c, measured, mus)
            assert np.array_equal(mus[1:, 1], signal.astype(np.float64)) and mus[0, 1] == 0
            seen_contraction |= bool((mus[:, 10] > 0).any())
            if name == "worm":  # nothing passes vacuously
                assert (mus[1:, 0] > 0).all() and (mus[:, 10] > 0).sum() >= 3 and mus[:, 0].sum() == 137804 and mus[0, 0] == 127436
                assert totals[0] == 11386 and totals[1] > 0
            # the sorted index and the original id are the pairs of read_particleIndex_buffer
            pi = hip.read_particleIndex_buffer()
            assert np.array_equal(pi[measured[0], 1], measured[1])
            # the spring and contraction sums moved the particle: they are not all zero, and strain is not constant
            assert np.abs(measured[2][:, 6:9]).max() > 0 and np.unique(measured[2][:, 4]).size > 1
    assert seen_contraction
    hip.close()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_fused_and_staged_paths_agree(name):
    sc = _scene(name)
    cfg = sc["cfg"]
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        signal = _signal(name, cfg, it)
        for hip in (a, b):
            hip.updateMuscleActivityData(signal)
        a.step(it)
        staged_step(b, it)
    check_against_restatement(b, sc, signal, "%s staged" % name)
    for x, y in zip(a.elastic_measure(), b.elastic_measure()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(u64(a.muscle_diagnostics()), u64(b.muscle_diagnostics()))
    if cfg.numOfMembranes:
        for x, y in zip(a.membrane_measure(), b.membrane_measure()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a.close()
    b.close()


def test_edge_rows_on_the_device():
    """The rows the hand-made CPU cases pin, on the device: a row that ends at slot 0, a full row of 32, a connection of length 0
    (a particle tied to itself), a rest length of 0, a group id above muscleCount and a signal <= 0."""
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    cfg.muscleCount = 5
    tab = sc["elastic"].reshape(-1, 32, 4)
    tab[0, :, 0] = -1.0                              # ends at slot 0 (the data behind the end stays and is dead)
    live = int((np.trunc(tab[9, :, 0]) != -1).argmin()) if (np.trunc(tab[9, :, 0]) == -1).any() else 32
    assert 0 < live < 32
    tab[9] = np.tile(tab[9, :live], (32 // live + 1, 1))[:32]  # a full row of 32: no terminator
    tab[10, 0] = (f32(10.1), tab[10, 0, 1], f32(3.3), 0)       # r == 0, in muscle 3
    tab[11, 1, 1] = 0.0                                        # L0 == 0
    tab[12, 0, 2] = f32(6.2)                                   # group 6 > muscleCount
    tab[13, 0, 2] = f32(2.2)                                   # muscle 2, whose signal is negative
    tab[14, 0, 2] = f32(4.2)                                   # muscle 4, whose signal is zero
    signal = np.array([0.5, -0.25, 1.0, 0.0, 2.0], np.float32)
    hip = scenes.hip_for(sc)
    hip.updateMuscleActivityData(signal)
    for it in range(2):
        hip.step(it)
        c, measured, mus, _ = check_against_restatement(hip, sc, signal, "edge rows step %d" % it)
        check_consistency(c, measured, mus)
    idx, ids, rec, con = measured
    assert rec[0, 0] == 0 and not rec[0].any() and rec[9, 0] == 32 and con[10, 0, 0] == 0 and mus[3, 14] == 1 and mus[3, 10] == 0
    assert con[11, 1, 0] == con[11, 1, 1] and mus[:, 0].tolist()[2:] == [1, 1, 1, 0] and mus[2, 10] == 0 and mus[4, 10] == 0 and mus[1, 10] > 0
    hip.close()


def stacked_sheets(layers=4, sx=96, sz=88, block=(16, 8), spare_groups=7):
    """layers x sz x sx elastic particles (more than 32,768 rows: the group tree of 32 slots per row has three levels) as flat
    sheets r0 apart, built with vectorised numpy: springs to the 8 in-plane neighbours and the particle above and below (rest
    length 0.95 r as the reference's generator), the x-springs of every block[0] x block[1] patch of a sheet a muscle group of
    their own, two membrane triangles per grid square. A chunk of 1024 slots is 32 consecutive particles of an x-row, so it
    holds two or three groups beside group 0 and lacks all the others. Order: elastic, a token 2 x 2 x 2 of liquid, boundary."""
    box = (f32(sx + 8) / 2 + 1, f32(layers + 12) / 2 + 1, f32(sz + 8) / 2 + 1)  # in h = 2 r0
    base = scenes.liquid_box(tuple(float(np.ceil(b)) for b in box), (2, 2, 2), mask=0xffffffff)
    cfg = base["cfg"]
    r0 = f32(cfg.r0)
    E = layers * sz * sx
    iy, iz, ix = np.meshgrid(np.arange(layers), np.arange(sz), np.arange(sx), indexing="ij")
    epos = np.zeros((E, 4), np.float32)
    epos[:, 0] = (f32(4.0) * r0 + ix.astype(np.float32) * r0).ravel()
    epos[:, 1] = (f32(8.0) * r0 + iy.astype(np.float32) * r0).ravel()
    epos[:, 2] = (f32(4.0) * r0 + iz.astype(np.float32) * r0).ravel()
    epos[:, 3] = f32(2.1)
    gx, gz = sx // block[0], sz // block[1]
    group = 1 + (ix // block[0]) + gx * ((iz // block[1]) + gz * iy)
    muscle_count = layers * gz * gx + spare_groups
    offsets = [(0, dz, dx) for dz in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dx) != (0, 0)] + [(-1, 0, 0), (1, 0, 0)]
    sim = f32(cfg.simulationScale)
    cand = np.zeros((E, len(offsets), 4), np.float32)
    valid = np.zeros((E, len(offsets)), bool)
    for k, (dy, dz, dx) in enumerate(offsets):
        jy, jz, jx = iy + dy, iz + dz, ix + dx
        ok = ((jy >= 0) & (jy < layers) & (jz >= 0) & (jz < sz) & (jx >= 0) & (jx < sx)).ravel()
        j = (np.clip(jy, 0, layers - 1) * sz + np.clip(jz, 0, sz - 1)) * sx + np.clip(jx, 0, sx - 1)
        j = j.ravel()
        d = epos[:, :3] - epos[j, :3]
        r = np.sqrt((d * d).sum(1).astype(np.float32))
        cand[:, k, 0] = j.astype(np.float32) + f32(0.1)
        cand[:, k, 1] = r * sim * f32(0.95)
        same = (dy == 0 and dz == 0) & (group.ravel() == group.ravel()[j])
        cand[:, k, 2] = np.where(same, group.ravel().astype(np.float32) + f32(0.2), f32(0.0))
        valid[:, k] = ok
    order = np.argsort(~valid, axis=1, kind="stable")  # a row's valid entries first, in offset order
    cand = np.take_along_axis(cand, order[:, :, None], axis=1)
    valid = np.take_along_axis(valid, order, axis=1)
    elastic = np.zeros((E, 32, 4), np.float32)
    elastic[:, :, 0] = -1.0
    elastic[:, :len(offsets)] = np.where(valid[:, :, None], cand, elastic[:, :len(offsets)])
    a = ((iy * sz + iz) * sx + ix)[:, :-1, :-1].ravel()
    tris = np.concatenate([np.stack([a, a + 1, a + sx], 1), np.stack([a + 1, a + sx + 1, a + sx], 1)]).astype(np.int32)
    verts = tris.ravel()
    by_vertex = np.argsort(verts, kind="stable")
    rank = np.arange(verts.size) - np.searchsorted(verts[by_vertex], verts[by_vertex])
    pml = -np.ones((E, 7), np.int32)
    pml[verts[by_vertex], rank] = (by_vertex // 3).astype(np.int32)
    nl = base["numOfLiquidP"]
    liq, bnd_p, bnd_v = base["position"][:nl], base["position"][nl:], base["velocity"][nl:]
    pos = np.concatenate([epos, liq, bnd_p]).astype(np.float32)
    vel = np.concatenate([np.zeros_like(epos), np.zeros_like(liq), bnd_v]).astype(np.float32)
    assert (pos[:E, :3].max(0) < np.array([cfg.xmax, cfg.ymax, cfg.zmax]) - 2 * r0).all()
    cfg.particleCount, cfg.numOfElasticP, cfg.numOfMembranes, cfg.elasticOffset, cfg.muscleCount = pos.shape[0], E, tris.shape[0], 0, int(muscle_count)
    return dict(cfg=cfg, position=pos, velocity=vel, elastic=elastic.reshape(-1, 4), membranes=tris, particle_membranes=pml,
                numOfLiquidP=nl, numOfElasticP=E, numOfBoundaryP=int(bnd_p.shape[0]))


def test_three_level_tree_with_many_groups():
    sc = stacked_sheets()
    cfg = sc["cfg"]
    E, G = cfg.numOfElasticP, cfg.muscleCount
    assert E > 32768 and E * 32 > 1024 * 1024 and G > 256 and cfg.numOfMembranes > 1024
    rng = np.random.default_rng(20261017)
    signal = rng.uniform(-0.5, 1.0, G).astype(np.float32)
    hip = scenes.hip_for(sc)
    hip.updateMuscleActivityData(signal)
    for it in range(2):
        hip.step(it)
    # the restatement's tree for a spread of groups (each is 12 sums over 1.08 M terms); counts and extremes for all of them
    some = sorted(set([0, 1, 2, G // 3, G // 2, G - 8, G - 7, G - 6, G] + rng.integers(1, G - 6, 12).tolist()))
    c, measured, mus, totals = check_against_restatement(hip, sc, signal, "sheets", groups=some)
    check_consistency(c, measured, mus)
    m, live = c.m[c.live], c.live
    counts = np.bincount(m, minlength=G + 1)
    assert np.array_equal(mus[:, 0], counts.astype(np.float64)) and (counts[1:G - 6] > 0).all() and (counts[G - 6:] == 0).all()
    assert not mus[G - 6:, 2:].any()
    mn, mx = np.full(G + 1, np.inf, np.float32), np.full(G + 1, -np.inf, np.float32)
    np.minimum.at(mn, m, c.e[live])
    np.maximum.at(mx, m, c.e[live])
    assert np.array_equal(u64(mus[:G - 6, 7]), u64((mn[:G - 6] + f32(0)).astype(np.float64)))
    assert np.array_equal(u64(mus[:G - 6, 8]), u64((mx[:G - 6] + f32(0)).astype(np.float64)))
    # a chunk of 1024 slots holds several groups and lacks most
    per_chunk = [np.unique(c.m[r:r + 32][c.live[r:r + 32]]).size for r in range(0, E, 32)]
    assert min(per_chunk) >= 2 and max(per_chunk) <= 8 and len(per_chunk) > 1024
    assert ((mus[1:, 10] > 0) == ((signal > 0) & (counts[1:] > 0))).all()
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_calls_are_read_only():
    """Every exported buffer, a mesh, a labelling, a selection and the following steps are unchanged by the three calls."""
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    h = np.float32(cfg.h)
    origin = np.array([cfg.xmin, cfg.ymin, cfg.zmin], np.float32) - 1.5 * h
    dims = [int(np.ceil((getattr(cfg, ax + "max") - getattr(cfg, ax + "min") + 3 * h) / (h / 2))) + 1 for ax in "xyz"]
    signal = _signal("tiny_elastic", cfg, 1)
    for it in range(4):
        for hip in (a, b):
            hip.updateMuscleActivityData(signal)
        a.step(it)
        b.step(it)
        a.extract_surface(origin, np.full(3, h / 2, np.float32), dims, iso=0.5, field="shepard", types=(1, 2))
        normals = a.surface_normals()
        n_sel, C = a.label_components(1.5364, (1, 2, 3))
        comp = a.components()
        rec = a.component_diagnostics([0, C - 1])
        assert a.select(None, (1, 2), [("surface", 0.05, np.inf)]) > 0
        sel = a.selection()
        before = {n: a.buffer(n) for n in BUFFERS}
        first = a.elastic_measure() + (a.muscle_diagnostics(),) + a.membrane_measure()
        again = a.elastic_measure() + (a.muscle_diagnostics(),) + a.membrane_measure()  # twice: the same arrays
        for x, y in zip(first, again):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
        assert np.array_equal(a.surface_normals().view(np.uint32), normals.view(np.uint32))  # the mesh is still valid
        for x, y in zip(comp, a.components()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(a.component_diagnostics([0, C - 1]).view(np.uint64), rec.view(np.uint64))  # ... and the labelling
        for x, y in zip(sel, a.selection()):  # ... and the selection
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    a.close()
    b.close()


def _rc_all(hip, E=1, G=100, M=1):
    idx, ids = np.empty(max(E, 1), np.int32), np.empty(max(E, 1), np.uint32)
    rec, con = np.empty((max(E, 1), 12), np.float32), np.empty((max(E, 1), 32, 2), np.float32)
    mus, tri, totals = np.empty((G + 1, 16), np.float64), np.empty((max(M, 1), 8), np.float32), np.empty(4, np.float64)
    L, h = hip._L, hip._h
    return (L.sph_elastic_measure(h, idx.ctypes.data, ids.ctypes.data, rec.ctypes.data, con.ctypes.data),
            L.sph_muscle_diagnostics(h, mus.ctypes.data), L.sph_membrane_measure(h, tri.ctypes.data, totals.ctypes.data))


def test_calling_rules():
    sc = scenes.SCENES["tiny_elastic"]()
    cfg = sc["cfg"]
    E, G, M = cfg.numOfElasticP, cfg.muscleCount, cfg.numOfMembranes
    hip = scenes.hip_for(sc)
    assert _rc_all(hip, E, G, M) == (ERR_ORDER,) * 3  # before a step
    for call in (hip.elastic_measure, hip.muscle_diagnostics, hip.membrane_measure):
        with pytest.raises(sphmi.SphError):
            call()
    hip.step(0)
    assert _rc_all(hip, E, G, M) == (0, 0, 0)
    L, h = hip._L, hip._h
    assert L.sph_elastic_measure(h, None, None, None, None) == 0  # any pointer may be NULL
    totals = np.empty(4, np.float64)
    assert L.sph_membrane_measure(h, None, totals.ctypes.data) == 0 and totals[0] == M
    assert L.sph_muscle_diagnostics(h, None) == ERR_INVALID and L.sph_membrane_measure(h, None, None) == ERR_INVALID
    assert b"sph_membrane_measure" in L.sph_last_error()
    for st in scenes.STAGE_SEQUENCE[:7]:  # a new step has begun: its density and pressure-force stages have not run yet
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc_all(hip, E, G, M) == (ERR_ORDER,) * 3
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    assert _rc_all(hip, E, G, M) == (0, 0, 0)
    hip.close()
    # elastic matter without membranes
    sc = scenes.elastic_offset_box()
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert _rc_all(hip, sc["cfg"].numOfElasticP, sc["cfg"].muscleCount, 1) == (0, 0, ERR_INVALID)
    hip.close()
    # a liquid-only scene
    hip = scenes.hip_for(scenes.SCENES["tiny"]())
    hip.step(0)
    assert _rc_all(hip) == (ERR_INVALID,) * 3
    with pytest.raises(sphmi.SphError):
        hip.muscle_diagnostics()
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc_all(hip) == (ERR_INVALID,) * 3
    hip.close()


def test_cpp_driver_elastic(tmp_path):
    """sphmi_run --worm --muscles --elastic-every: the CSV files parse and equal frames.muscle_summary of the same states."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    d = str(tmp_path)
    r = subprocess.run([exe, "--worm", "--muscles", "--steps", "4", "--elastic-every", "2", "--elastic-out", d], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(d)) == ["muscles_2.csv", "muscles_4.csv"]
    assert r.stdout.count("_elastic: connections 137804 ") == 2 and "membrane area" in r.stdout
    sc = scenes.worm_scene()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want = frames.muscle_summary(hip.muscle_diagnostics())
            got = frames.read_muscles_csv(os.path.join(d, "muscles_%d.csv" % (it + 1)))
            assert got.shape == (cfg.muscleCount + 1, 8) and np.array_equal(u64(got), u64(want)), it
            assert (want[1:97, 1] > 0).all() and np.unique(want[1:97, 3]).size > 1
            if it == 3:
                assert (want[:, 2] > 0).any()  # a signal of an earlier step is stored by now
        hip.updateMuscleActivityData(sphmi.muscle_signal(it, cfg.muscleCount))  # the driver's order: after the report
    hip.close()
    q = os.path.join(d, "quiet")
    os.makedirs(q)
    r = subprocess.run([exe, "--worm", "--steps", "1", "--elastic-every", "1", "--elastic-out", q, "--quiet"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "_elastic" not in r.stdout and os.listdir(q) == ["muscles_1.csv"]
    for bad in (["--worm", "--elastic-every", "2"], ["--worm", "--elastic-out", d], ["--worm", "--elastic-every", "0", "--elastic-out", d],
                ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--elastic-every", "1", "--elastic-out", d]):
        r = subprocess.run([exe, "--steps", "1"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip(), bad
