"""GPU tests of the carried particle fields (sph_field_*, include/sphmi.h): diffusion, the stability number and the region
records bit-identical to the numpy restatement (tests/fields_ref.py, which tests/test_fields_host.py ties to the force
decomposition's viscous sum), on the fused and the staged path, on 16-bit and 32-bit rows and a two-level tree; painting against
the removal's own count; the fields through removals and additions against a twin solver; passivity; the calling rules; the
driver's line. No tolerance appears anywhere: integers are compared for equality, floats as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import diag_ref
import edit_ref as er
import fields_ref as flr
import forces_ref as fr
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
MASKS = [(1,), (1, 2), (1, 2, 3)]
EVERYTHING = np.array([diag_ref.EVERYTHING], np.float32)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def first_diff(got, want, view):
    d = np.argwhere(view(got) != view(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def regions_of(cfg, count):
    """`count` regions (test_forces.py's): everything, halves and octants of the box, an empty one (x0 >= x1), one outside the
    scene, slabs."""
    mid = [f32(0.5) * f32(getattr(cfg, a + "max")) for a in "xyz"]
    inf = np.inf
    out = [diag_ref.EVERYTHING, (-inf, -inf, -inf, mid[0], inf, inf), (mid[0], -inf, -inf, inf, inf, inf),
           (0, 0, 0, mid[0], mid[1], mid[2]), (mid[0], mid[1], mid[2], mid[0], inf, inf), (-9, -9, -9, -1, -1, -1),
           (-inf, mid[1], -inf, inf, inf, inf), (-inf, -inf, mid[2], inf, inf, inf)]
    k = 0
    while len(out) < count:
        lo = f32(cfg.ymax) * f32(k) / f32(8)
        out.append((-inf, lo, -inf, inf, lo + f32(cfg.ymax) / f32(8), inf))
        k += 1
    return np.array(out[:count], np.float32)


def exported(hip):
    """(state with the original ids, neighbour ids, stored distances) of the last completed step."""
    state = fr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    return state, ids, dist


def make_fields(state, seed):
    """Two fields in ORIGINAL-id order: seeded random values in [-0.5, 1.5), and 1 on the particles below the median x of the
    LIQUID (so that the liquid, which every mask holds, is split whatever share of the scene is boundary shell), else 0."""
    n = state["rho"].shape[0]
    rnd = (np.random.default_rng(seed).random(n, dtype=np.float32) * f32(2) - f32(0.5)).astype(np.float32)
    x = state["pos"][:, 0]
    box = np.zeros(n, np.float32)
    box[state["ids"][x < np.median(x[np.trunc(state["types"]) == 1])]] = 1
    return rnd, box


def stable_coefficient(D):
    return f32(0.5 / float((D.sD.astype(np.float64) * D.W.astype(np.float64))[D.P].max()))


def check_diffusion(hip, what, seed, masks=MASKS):
    """field_diffuse with 0, 1 and 4 substeps on both fields and every mask against the restatement; slot 1 of the solver."""
    state, ids, dist = exported(hip)
    K = flr.constants(hip.cfg)
    for types in masks:
        D = flr.Diffusion(state, ids, dist, K, types)
        coefficient = stable_coefficient(D)
        for name, field in zip(("random", "box"), make_fields(state, seed)):
            want1, sigma, _ = flr.diffuse(state, ids, dist, K, field, coefficient, 1, types, D)
            want4 = flr.diffuse(state, ids, dist, K, want1, coefficient, 3, types, D)[0]  # Jacobi substeps compose: 4 = 1 + 3
            assert sigma > 0 and not np.array_equal(u32(want1), u32(field)) and not np.array_equal(u32(want4), u32(want1))
            for substeps, want in ((0, field), (1, want1), (4, want4)):
                hip.field_write(1, field)
                got_sigma = hip.field_diffuse(1, coefficient, substeps, types)
                got = hip.field_read(1)
                tag = "%s %s field types %r substeps %d" % (what, name, types, substeps)
                assert got.dtype == np.float32 and got.shape == field.shape
                assert np.array_equal(u32(got), u32(want)), "%s: %s" % (tag, first_diff(got, want, u32))
                assert u32([got_sigma])[0] == u32([sigma])[0], "%s: sigma %r vs %r" % (tag, got_sigma, sigma)
    return state, ids, dist


@pytest.mark.parametrize("name", ["tiny", "tiny_compressed", "tiny_elastic", "wide"])
def test_diffusion_matches_restatement(name):
    """After step 0 and after five more steps. `wide`: 32-bit cell ids and wide rows, about 105 k particles; `tiny_compressed`:
    full rows."""
    sc = scenes.SCENES[name]()
    hip = scenes.hip_for(sc)
    hip.field_create(1)
    hip.step(0)
    check_diffusion(hip, "%s step 0" % name, 1)
    for it in range(1, 6):
        hip.step(it)
    state, ids, dist = check_diffusion(hip, "%s step 5" % name, 2)
    if name == "tiny_compressed":
        assert ((ids >= 0).sum(1) == 32).any()
    if name == "tiny_elastic":  # the three masks are three different sets of participants
        assert len({int(flr.participates(state, t).sum()) for t in MASKS}) == 3
    hip.close()


def test_staged_path_gives_the_same_field():
    sc = scenes.SCENES["tiny_compressed"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        a.step(it)
        staged_step(b, it)
    state, ids, dist = exported(b)
    K = flr.constants(sc["cfg"])
    D = flr.Diffusion(state, ids, dist, K, (1, 3))
    coefficient = stable_coefficient(D)
    field = make_fields(state, 3)[0]
    want, sigma, _ = flr.diffuse(state, ids, dist, K, field, coefficient, 2, (1, 3), D)
    got = []
    for hip in (a, b):
        hip.field_create(0, field)
        assert u32([hip.field_diffuse(0, coefficient, 2, (1, 3))])[0] == u32([sigma])[0]
        got.append(hip.field_read(0))
        assert np.array_equal(u64(hip.field_diagnostics(0, regions_of(sc["cfg"], 3), (1, 3))),
                              u64(flr.diag_records(state, want[state["ids"]], regions_of(sc["cfg"], 3), (1, 3))))
    assert np.array_equal(u32(got[0]), u32(got[1])) and np.array_equal(u32(got[1]), u32(want)), first_diff(got[1], want, u32)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["tiny_elastic", "wide"])
def test_diagnostics_match_restatement(name):
    """1 and 16 regions, every mask, u64 equality; both scenes have more than one chunk (an upper tree level), `wide` 103."""
    sc = scenes.SCENES[name]()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    state = fr.solver_state(hip)
    assert hip.N > 1024
    field = make_fields(state, 4)[0]
    field[::7] = 0  # so that the tagged count is not the particle count
    field[3::11] = f32(-0.0)
    hip.field_create(3, field)
    c_sorted = field[state["ids"]]
    assert np.array_equal(u32(c_sorted), u32(frames.field_sorted(field, hip.read_particleIndex_buffer())))
    for count in (1, 16):
        rg = regions_of(cfg, count)
        for types in MASKS:
            got = hip.field_diagnostics(3, rg, types)
            assert got.dtype == np.float64 and got.shape == (count, 8)
            want = flr.diag_records(state, c_sorted, rg, types)
            assert np.array_equal(u64(got), u64(want)), "%s %d regions types %r: %s" % (name, count, types, first_diff(got, want, u64))
            assert got[0, 0] == hip.diagnostics(rg[:1], types)[0, 0] > 0 and 0 < got[0, 5] < got[0, 0] and got[0, 3] < 0 < got[0, 4]
            if count >= 6:
                assert not got[4].any() and not got[5].any() and got[0, 0] == got[1, 0] + got[2, 0]
    s = frames.field_summary(hip.field_diagnostics(3, types=(1, 2, 3))[0])
    sel = diag_ref.selected(state, diag_ref.EVERYTHING, (1, 2, 3))
    assert s["count"] == sel.sum() > 0 and s["tagged"] == int((c_sorted[sel] != 0).sum()) and s["variance"] > 0
    hip.close()


def test_painting():
    sc = scenes.SCENES["tiny"]()
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    pos = hip.read_position_buffer()
    start = np.arange(hip.N, dtype=np.float32)
    hip.field_create(0, start)
    box = er.liquid_quantile_box(pos)
    # exactly the ids the removal counts for the same box and types, on the CURRENT positions
    for types, region, value in (((1,), box, 2.5), ((3,), None, -4.0), ((1, 3), (-np.inf, box[1], -np.inf, np.inf, np.inf, np.inf), 0.0)):
        n = hip.field_set_region(0, value, region, types)
        start, want_n = flr.paint_region(start, pos, region, types, value)
        assert n == want_n == hip.remove_region(region, types, count_only=True) == er.region_marks(pos, region, types).sum() > 0
        assert np.array_equal(u32(hip.field_read(0)), u32(start))
    assert hip.field_set_region(0, 1.0, (-9, -9, -9, -1, -1, -1), (1, 2, 3)) == 0 and np.array_equal(u32(hip.field_read(0)), u32(start))
    # a bound that is exactly a particle's float32 x: inside as a lower bound, outside as an upper bound, inside one float above
    p = int(np.flatnonzero(er.region_marks(pos, box, (1,)))[0])
    x = pos[p, 0]
    inf = np.inf
    for region, inside in (((x, -inf, -inf, inf, inf, inf), True), ((-inf, -inf, -inf, x, inf, inf), False),
                           ((-inf, -inf, -inf, np.nextafter(x, f32(inf)), inf, inf), True)):
        hip.field_write(0, np.zeros(hip.N, np.float32))
        n = hip.field_set_region(0, 1.0, region, (1,))
        got = hip.field_read(0)
        assert (got[p] == 1) == inside and n == got.sum() == er.region_marks(pos, region, (1,)).sum() == hip.remove_region(region, (1,), count_only=True)
    # the selection's original ids
    hip.field_write(0, start)
    n_sel = hip.select(box, (1,), [("density", 0.0, np.inf)])
    idx, ids, _ = hip.selection()
    assert 0 < n_sel < hip.N and hip.field_set_selection(0, 7.0) == n_sel
    assert np.array_equal(u32(hip.field_read(0)), u32(flr.paint_ids(start, ids, 7.0)))
    assert hip.select((-9, -9, -9, -1, -1, -1)) == 0 and hip.field_set_selection(0, 8.0) == 0
    assert np.array_equal(u32(hip.field_read(0)), u32(flr.paint_ids(start, ids, 7.0)))
    hip.close()


ROOM = 400
DIMS = (6, 5, 4)


def test_fields_follow_edits():
    sc = scenes.SCENES["tiny"]()
    cfg0 = sc["cfg"]
    N0 = cfg0.particleCount
    cfg = er.with_count(cfg0, N0, N0 + ROOM)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    for it in range(2):
        hip.step(it)
    rng = np.random.default_rng(5)
    fields = {0: rng.random(N0, dtype=np.float32), 2: np.arange(N0, dtype=np.float32)}
    inflow = {0: f32(0.25), 2: f32(-1)}
    for slot in fields:
        hip.field_create(slot, fields[slot], inflow[slot])

    def assert_fields(what):
        for slot in fields:
            got = hip.field_read(slot)
            assert got.shape == fields[slot].shape and np.array_equal(u32(got), u32(fields[slot])), "%s, slot %d: %s" % (
                what, slot, first_diff(got, fields[slot], u32))

    pos = hip.read_position_buffer()
    box = er.liquid_quantile_box(pos)
    # edits that change nothing: a counting removal, a removal of nothing, an add beyond the capacity
    assert hip.remove_region(box, (1,), count_only=True) > 0
    assert hip.remove_region((-9, -9, -9, -1, -1, -1), (1, 3)) == 0
    with pytest.raises(sphmi.SphError):
        hip.add_particles(np.repeat(pos[:1], ROOM + 1, 0), np.zeros((ROOM + 1, 4), f32))
    assert hip.N == N0
    assert_fields("after the edits that change nothing")
    # a removal: every slot through the edit map
    removed = hip.remove_region(box, (1,))
    m = hip.edit_map()
    assert removed > 0 and (m < 0).sum() == removed and hip.N == N0 - removed
    for slot in fields:
        fields[slot] = flr.follow_removal(fields[slot], m)
    assert np.array_equal(fields[2], np.flatnonzero(m >= 0).astype(np.float32))  # old[kept]
    assert_fields("after the removal")
    # an emitter: the tail holds each slot's inflow (its place is cleared first: a second removal)
    pos = hip.read_position_buffer()
    r0 = f32(cfg0.r0)
    sp = f32(0.93) * r0
    origin, place = er.clear_origin(pos, cfg0, DIMS, sp, r0)
    if hip.remove_region(place, (1,)):
        m = hip.edit_map()
        for slot in fields:
            fields[slot] = flr.follow_removal(fields[slot], m)
    n_before = hip.N
    added = hip.emit_lattice(origin, (sp, sp, sp), DIMS, velocity=(0.0, -0.05, 0.0))
    assert added == 120 and hip.N == n_before + 120
    for slot in fields:
        fields[slot] = flr.follow_add(fields[slot], added, inflow[slot])
    assert_fields("after the emitter")
    assert (hip.field_read(0)[-120:] == f32(0.25)).all() and (hip.field_read(2)[-120:] == -1).all()
    # hand-made particles through add_particles
    pos = hip.read_position_buffer()
    o2, place2 = er.clear_origin(pos, cfg0, (7, 2, 3), f32(1.1) * r0, r0)
    if hip.remove_region(place2, (1,)):
        m = hip.edit_map()
        for slot in fields:
            fields[slot] = flr.follow_removal(fields[slot], m)
    ap, av = er.hand_made_particles(cfg0, o2)
    hip.add_particles(ap, av)
    for slot in fields:
        fields[slot] = flr.follow_add(fields[slot], ap.shape[0], inflow[slot])
    assert_fields("after add_particles")
    # diffusion needs a step after an edit; then it equals the restatement and a twin made from the edited arrays
    with pytest.raises(sphmi.SphError) as e:
        hip.field_diffuse(0, 1e-9)
    assert scenes.error_status(e) == ERR_ORDER
    pos, vel = hip.read_position_buffer(), hip.read_velocity_buffer()
    twin = sphmi.owHIPSolver(er.with_count(cfg0, hip.N, 0), pos, vel)
    twin.field_create(0)
    twin.field_write(0, fields[0])
    twin.field_create(2, fields[2], 9.0)
    hip.step(2)
    twin.step(2)
    state, ids, dist = exported(hip)
    K = flr.constants(cfg0)
    D = flr.Diffusion(state, ids, dist, K, (1,))
    coefficient = stable_coefficient(D)
    for slot in fields:
        want, sigma, _ = flr.diffuse(state, ids, dist, K, fields[slot], coefficient, 2, (1,), D)
        sa, sb = hip.field_diffuse(slot, coefficient, 2), twin.field_diffuse(slot, coefficient, 2)
        assert u32([sa])[0] == u32([sb])[0] == u32([sigma])[0]
        got = hip.field_read(slot)
        assert np.array_equal(u32(got), u32(want)), first_diff(got, want, u32)
        assert np.array_equal(u32(got), u32(twin.field_read(slot))) and not np.array_equal(u32(got), u32(fields[slot]))
    hip.close()
    twin.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_fields_are_passive():
    """Painting, diffusing and reducing every step changes nothing the step computes, and a labelling, a selection and an edit
    map made before the field calls are still readable after them."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    rg = regions_of(sc["cfg"], 5)
    a.field_create(0, inflow=1.0)
    a.field_create(3, np.linspace(0, 1, a.N, dtype=np.float32))
    for it in range(6):
        a.step(it)
        b.step(it)
        a.label_components(np.inf, (1, 2))
        comp = a.components()
        assert a.select(None, (1, 2), [("density", 0.0, np.inf)]) > 0
        sel = a.selection()
        assert a.remove_region((-9, -9, -9, -1, -1, -1), (1,)) == 0  # removes nothing: the edit map is the identity, the state stays
        emap = a.edit_map()
        assert a.field_set_region(0, 1.0, (-np.inf, -np.inf, -np.inf, f32(0.4) * f32(sc["cfg"].xmax), np.inf, np.inf), (1, 2)) > 0
        assert a.field_set_selection(3, 0.5) > 0
        for slot in (0, 3):
            assert a.field_diffuse(slot, 1e-9, 2, (1, 2)) > 0
            a.field_write(slot, a.field_read(slot))
        assert a.field_diagnostics(0, rg, (1, 2))[0, 5] > 0
        for x, y in zip(comp, a.components()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for x, y in zip(sel, a.selection()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(emap, a.edit_map()) and np.array_equal(emap, np.arange(a.N))
    for n in BUFFERS:
        assert np.array_equal(a.buffer(n).view(np.uint8), b.buffer(n).view(np.uint8)), n
    assert np.array_equal(u64(a.diagnostics(rg)), u64(b.diagnostics(rg)))
    a.close()
    b.close()


def _status(call):
    with pytest.raises(sphmi.SphError) as e:
        call()
    return scenes.error_status(e)


def test_calling_rules():
    sc = scenes.SCENES["tiny"]()
    cfg0 = sc["cfg"]
    hip = sphmi.owHIPSolver(er.with_count(cfg0, cfg0.particleCount, cfg0.particleCount + 8), sc["position"], sc["velocity"])
    N = hip.N
    zeros = np.zeros(N, np.float32)
    # a missing slot, and a new solver: the current-set calls work at once, the sorted-state calls need a step
    for call in (lambda: hip.field_read(0), lambda: hip.field_write(0, zeros), lambda: hip.field_release(0),
                 lambda: hip.field_set_region(0, 1.0), lambda: hip.field_set_selection(0, 1.0), lambda: hip.field_diffuse(0, 0.0),
                 lambda: hip.field_diagnostics(0)):
        assert _status(call) == ERR_ORDER
    hip.field_create(0)
    assert _status(lambda: hip.field_create(0)) == ERR_ORDER  # double create
    assert not hip.field_read(0).any() and hip.field_set_region(0, 1.0, None, (1,)) == sc["numOfLiquidP"]
    hip.field_write(0, zeros)
    assert _status(lambda: hip.field_diffuse(0, 0.0)) == ERR_ORDER and _status(lambda: hip.field_diagnostics(0)) == ERR_ORDER
    assert _status(lambda: hip.field_set_selection(0, 1.0)) == ERR_ORDER  # no selection
    hip.step(0)
    assert hip.field_diffuse(0, 0.0) == 0 and hip.field_diffuse(0, 1e-9, 0) > 0 and hip.field_diagnostics(0)[0, 0] == sc["numOfLiquidP"]
    # SPH_ERR_INVALID: slot 4 and -1 everywhere; masks; NaN bounds; negative coefficient or substeps; non-finite values
    for slot in (4, -1):
        for call in (lambda: hip.field_create(slot), lambda: hip.field_read(slot), lambda: hip.field_write(slot, zeros),
                     lambda: hip.field_release(slot), lambda: hip.field_set_region(slot, 1.0), lambda: hip.field_set_selection(slot, 1.0),
                     lambda: hip.field_diffuse(slot, 0.0), lambda: hip.field_diagnostics(slot)):
            assert _status(call) == ERR_INVALID
    for types in ((), (0,), (4,), (1, 4)):  # masks 0, 1, 0x10, 0x12
        assert _status(lambda: hip.field_set_region(0, 1.0, None, types)) == ERR_INVALID
        assert _status(lambda: hip.field_diffuse(0, 0.0, 1, types)) == ERR_INVALID
        assert _status(lambda: hip.field_diagnostics(0, None, types)) == ERR_INVALID
    nan = (0, 0, np.nan, 1, 1, 1)
    assert _status(lambda: hip.field_set_region(0, 1.0, nan)) == ERR_INVALID and _status(lambda: hip.field_diagnostics(0, [nan])) == ERR_INVALID
    assert _status(lambda: hip.field_diagnostics(0, np.zeros((17, 6), np.float32))) == ERR_INVALID
    assert _status(lambda: hip.field_diffuse(0, -1e-9)) == ERR_INVALID and _status(lambda: hip.field_diffuse(0, 1e-9, -1)) == ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        assert _status(lambda: hip.field_diffuse(0, bad)) == ERR_INVALID
        assert _status(lambda: hip.field_set_region(0, bad)) == ERR_INVALID and _status(lambda: hip.field_create(1, None, bad)) == ERR_INVALID
        v = zeros.copy()
        v[5] = bad
        assert _status(lambda: hip.field_write(0, v)) == ERR_INVALID and b"value 5" in hip._L.sph_last_error()
        assert _status(lambda: hip.field_create(1, v)) == ERR_INVALID
    assert not hip.field_read(0).any()  # nothing was written by the refused calls
    assert _status(lambda: hip.field_read(1)) == ERR_ORDER  # ... and slot 1 was not created
    L, h = hip._L, hip._h
    out = np.zeros(8, np.float64)
    assert L.sph_field_set_region(h, 0, None, 2, 1.0, None) == ERR_INVALID and L.sph_field_read(h, 0, None) == ERR_INVALID
    assert L.sph_field_diagnostics(h, 0, None, 1, 2, out.ctypes.data) == ERR_INVALID
    assert L.sph_field_diagnostics(h, 0, EVERYTHING.ctypes.data, 1, 2, None) == ERR_INVALID
    assert L.sph_field_diffuse(h, 0, 0.0, 1, 2, None) == 0  # the stability number may be left out
    # a selection paints until the state moves on
    assert hip.select(None, (1,)) > 0 and hip.field_set_selection(0, 2.0) == sc["numOfLiquidP"]
    hip.step(1)
    assert _status(lambda: hip.field_set_selection(0, 3.0)) == ERR_ORDER
    # after an edit until a step: the current-set calls work, the sorted-state calls do not
    pos = hip.read_position_buffer()
    extra = pos[:1].copy()
    extra[0, :3] = [0.5 * cfg0.xmax, 0.9 * cfg0.ymax, 0.5 * cfg0.zmax]
    extra[0, 3] = 1.1
    hip.add_particles(extra, np.zeros((1, 4), f32))
    assert hip.field_read(0).shape == (N + 1,) and hip.field_set_region(0, 1.0, None, (1,)) == sc["numOfLiquidP"] + 1
    assert _status(lambda: hip.field_diffuse(0, 0.0)) == ERR_ORDER and _status(lambda: hip.field_diagnostics(0)) == ERR_ORDER
    hip.step(2)
    assert hip.field_diffuse(0, 0.0) == 0 and hip.field_diagnostics(0)[0, 1] == sc["numOfLiquidP"] + 1
    # release, then create again
    hip.field_release(0)
    assert _status(lambda: hip.field_read(0)) == ERR_ORDER and _status(lambda: hip.field_release(0)) == ERR_ORDER
    hip.field_create(0, np.full(hip.N, 3, np.float32))
    assert (hip.field_read(0) == 3).all()
    for slot in (1, 2, 3):
        hip.field_create(slot)
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    zeros = np.zeros(n, np.float32)
    for call in (lambda: hip.field_create(0), lambda: hip.field_read(0), lambda: hip.field_write(0, zeros), lambda: hip.field_release(0),
                 lambda: hip.field_set_region(0, 1.0), lambda: hip.field_set_selection(0, 1.0), lambda: hip.field_diffuse(0, 0.0),
                 lambda: hip.field_diagnostics(0)):
        assert _status(call) == ERR_INVALID
    hip.close()


def test_cpp_driver_dye():
    """sphmi_run --dye-region --dye-diffusivity --dye-every 2 prints the numbers of the wrapper on the same scene."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12))
    cfg = sc["cfg"]
    region = [f32(0), f32(0), f32(0), f32(0.5) * f32(cfg.xmax), np.inf, np.inf]
    diffusivity = f32(1e-4)
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--quiet", "--dye-region"] +
                       ["%.9g" % x for x in region] + ["--dye-diffusivity", "%.9g" % diffusivity, "--dye-every", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("dye step=")]
    assert [int(d["step"]) for d in lines] == [2, 4], r.stdout
    hip = scenes.hip_for(sc)
    hip.field_create(0)
    painted = hip.field_set_region(0, 1.0, region, (1,))
    assert 0 < painted < sc["numOfLiquidP"]
    want = []
    for it in range(4):
        hip.step(it)
        sigma = hip.field_diffuse(0, diffusivity * f32(cfg.timeStep), 1, (1,))
        if it % 2:
            want.append((frames.field_summary(hip.field_diagnostics(0, types=(1,))[0]), hip.field_diagnostics(0, types=(1,))[0], sigma))
    for d, (s, rec, sigma) in zip(lines, want):
        assert float(d["n"]) == s["count"] == sc["numOfLiquidP"] and float(d["sum"]) == rec[1] and float(d["mean"]) == s["mean"]
        assert float(d["var"]) == s["variance"] and float(d["min"]) == s["min"] and float(d["max"]) == s["max"]
        assert float(d["stability"]) == float("%.9g" % sigma) and 0 < sigma < 1
    assert float(lines[0]["var"]) > float(lines[1]["var"]) > 0  # it mixes
    hip.close()
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "1"]
    for bad in (["--dye-every", "0"], ["--dye-diffusivity", "-1"], ["--dye-region", "0", "0", "nan", "1", "1", "1"], ["--dye-inflow", "inf"]):
        r = subprocess.run([exe] + box + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
