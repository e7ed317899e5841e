"""GPU tests of particle editing (sph_remove_region / sph_remove_selection / sph_remove_ids / sph_add_particles / sph_emit_lattice /
sph_read_edit_map, include/sphmi.h): counts, read-back and id maps equal to the numpy restatement (tests/edit_ref.py); an edited
solver continues bit for bit like a solver newly created from the restated arrays and like the C oracle created from them; the
block, wave and scan edges of the compaction; the calling rules; the driver's flags. No tolerance appears anywhere: integers are
compared for equality, floats as bit patterns."""
import os
import re
import subprocess

import numpy as np
import pytest

import edit_ref as er
import scenes
import sphmi
from sphmi import slab as S
from scenes import error_status as _status, staged_step

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_ORDER, ERR_SIZE = -1, -3, -5
f32 = np.float32
SCENE_NAMES = ["tiny", "tiny_jitter", "tiny_compressed", "tiny_elastic", "worm", "wide", "alias16"]
ROOM = 4096
DIMS = (6, 5, 4)


def _scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


def _hip(sc, cfg, pos, vel):
    return sphmi.owHIPSolver(cfg, pos, vel, sc["elastic"], sc["membranes"], sc["particle_membranes"])


def read_state(hip):
    return hip.read_position_buffer(), hip.read_velocity_buffer()


def assert_state(hip, pos, vel, what):
    assert hip.N == pos.shape[0] == hip._L.sph_particle_count(hip._h), "%s: count %d, restated %d" % (what, hip.N, pos.shape[0])
    gp, gv = read_state(hip)
    assert scenes.bits_equal(gp, pos), "%s: position: %s" % (what, scenes.diff_report(gp, pos))
    assert scenes.bits_equal(gv, vel), "%s: velocity: %s" % (what, scenes.diff_report(gv, vel))


class Edited:
    """The edits of test 1 on a scene's solver after 3 steps, each checked against the restatement when `check` is set:
    drain the 0.3-0.7 quantile box of the liquid; clear a place and emit a 6 x 5 x 4 block at 0.93 r0 into it; clear another and
    add seven hand-made particles, one a boundary particle with a normal."""

    def __init__(self, name, check):
        sc = self.sc = _scene(name)
        cfg0 = sc["cfg"]
        N0, E, off = cfg0.particleCount, cfg0.numOfElasticP, cfg0.elasticOffset
        self.cfg = er.with_count(cfg0, N0, N0 + ROOM)
        hip = self.hip = _hip(sc, self.cfg, sc["position"], sc["velocity"])
        for it in range(3):
            hip.step(it)
        pos, vel = read_state(hip)
        r0 = f32(cfg0.r0)
        sp = f32(0.93) * r0

        def drain(box, what):
            nonlocal pos, vel
            want = er.region_marks(pos, box, (1,))
            if check:
                assert hip.remove_region(box, (1,), count_only=True) == want.sum() and hip.N == pos.shape[0]
            n_before = pos.shape[0]
            p, v, m = er.remove(pos, vel, want, E, off)
            got = hip.remove_region(box, (1,))
            pos, vel = p, v
            if check:
                assert got == want.sum() and got > 0, what
                gm = hip.edit_map()
                assert gm.dtype == np.int32 and gm.shape == (n_before,) and np.array_equal(gm, m), what + ": edit map"
                assert_state(hip, pos, vel, what)

        drain(er.liquid_quantile_box(pos), "drain")
        origin, place = er.clear_origin(pos, cfg0, DIMS, sp, r0)
        drain(place, "clear the emitter's place")
        lp, lv = er.lattice(origin, (sp, sp, sp), DIMS, velocity=(0.0, -0.05, 0.0))
        pos, vel = er.append(pos, vel, lp, lv, cfg0, self.cfg.capacity)
        added = hip.emit_lattice(origin, (sp, sp, sp), DIMS, velocity=(0.0, -0.05, 0.0))
        if check:
            assert added == 120
            assert_state(hip, pos, vel, "emit")
        o2, place2 = er.clear_origin(pos, cfg0, (7, 2, 3), f32(1.1) * r0, r0)
        drain(place2, "clear the hand-made particles' place")
        ap, av = er.hand_made_particles(cfg0, o2)
        pos, vel = er.append(pos, vel, ap, av, cfg0, self.cfg.capacity)
        n = hip.add_particles(ap, av)
        if check:
            assert n == pos.shape[0]
            assert_state(hip, pos, vel, "add")
        self.pos, self.vel = pos, vel


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_edit_equals_restatement(name):
    e = Edited(name, check=True)
    assert e.hip.N != e.sc["cfg"].particleCount
    e.hip.close()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_continuation_equals_fresh_solver_and_oracle(name):
    """3 more steps on the edited solver (stage by stage for tiny_jitter), on a solver created from the restated arrays with
    capacity 0 and on the oracle created from them: bit-identical. The oracle runs for every scene: three steps of the largest
    (worm, 233 k particles) take under a second."""
    e = Edited(name, check=False)
    hip, N = e.hip, e.pos.shape[0]
    cfg = er.with_count(e.sc["cfg"], N, 0)
    fresh = _hip(e.sc, cfg, e.pos, e.vel)
    from oracle import oraclebind as O
    ora = O.OracleSolver(sphmi.config_dict(cfg), e.pos, e.vel, e.sc["elastic"], e.sc["membranes"], e.sc["particle_membranes"], threads=4)
    for it in range(3):
        staged_step(hip, it) if name == "tiny_jitter" else hip.step(it)
        fresh.step(it)
        ora.step()
    got = dict(position=hip.read_position_buffer(), velocity=hip.read_velocity_buffer(), rho=hip.read_density_buffer(),
               particleIndex=hip.read_particleIndex_buffer())
    new = dict(position=fresh.read_position_buffer(), velocity=fresh.read_velocity_buffer(), rho=fresh.read_density_buffer(),
               particleIndex=fresh.read_particleIndex_buffer())
    ref = dict(position=ora.buffer("position").reshape(-1, 4)[:N], velocity=ora.buffer("velocity").reshape(-1, 4)[:N],
               rho=ora.buffer("rho")[:N], particleIndex=ora.buffer("particleIndex").reshape(-1, 2)[:N])
    for k in got:
        assert scenes.bits_equal(got[k], new[k]), "%s, edited vs fresh: %s" % (k, scenes.diff_report(got[k], new[k]))
        assert scenes.bits_equal(got[k], ref[k]), "%s, edited vs oracle: %s" % (k, scenes.diff_report(got[k], ref[k]))
    # the analysis calls work again, and agree with the fresh solver's
    box = er.liquid_quantile_box(e.pos, 0.2, 0.8)
    regions = [(-np.inf,) * 3 + (np.inf,) * 3, tuple(box)]
    assert scenes.bits_equal(hip.diagnostics(regions, (1, 2, 3)), fresh.diagnostics(regions, (1, 2, 3)))
    n1, n2 = hip.select(box, (1,), (("density", 0.0, np.inf),)), fresh.select(box, (1,), (("density", 0.0, np.inf),))
    assert n1 == n2 and n1 > 0
    for a, b in zip(hip.selection(), fresh.selection()):
        assert scenes.bits_equal(a, b)
    hip.close(); fresh.close(); ora.close()


# ---------------------------------------------------------------------------------------------- block and scan edges
def _scan_threads():
    src = open(os.path.join(scenes.PKG, "csrc", "sph_select.hip")).read()
    return int(re.search(r"#define\s+SEL_SCAN_THREADS\s+(\d+)", src).group(1))


BLOCK = 256


def _patterns(N):
    rng = np.random.default_rng(7)
    b = (N // BLOCK // 2) * BLOCK  # a whole 256-aligned block
    one_block = [("one block", np.arange(b, b + BLOCK))] if N > BLOCK else []  # (at N <= 256 that would be every particle)
    return [("first", [0]), ("last", [N - 1]), ("every second", np.arange(0, N, 2))] + one_block + [
            ("all but the first", np.arange(1, N)), ("all but the last", np.arange(0, N - 1)),
            ("straddling a wave and a block", np.concatenate([np.arange(60, 70), np.arange(BLOCK - 3, min(BLOCK + 3, N))])),
            ("duplicates, unordered", rng.integers(0, N, 97).repeat(2)), ("empty", [])]


def _check_patterns(hip, pos, vel, names=None):
    """Every pattern against the restatement on the solver's current particles; the removed ones are added back afterwards, so
    that the count is the same for the next pattern (their order is not: the patterns are ids)."""
    for what, ids in _patterns(pos.shape[0]):
        if names is not None and what not in names:
            continue
        N = pos.shape[0]
        marked = er.id_marks(N, ids)
        p, v, m = er.remove(pos, vel, marked)
        assert hip.remove_ids(ids) == marked.sum(), what
        assert np.array_equal(hip.edit_map(), m), what + ": edit map"
        assert_state(hip, p, v, what)
        pos, vel = er.append(p, v, pos[marked], vel[marked])
        assert hip.add_particles(pos[p.shape[0]:], vel[p.shape[0]:]) == N, what
    assert_state(hip, pos, vel, "after the patterns")
    return pos, vel


@pytest.fixture(scope="module")
def big():
    """One liquid box with more than 8 * SEL_SCAN_THREADS blocks of 256 particles: each thread of the one-workgroup scan then has
    a run longer than 8 blocks, so its unrolled part and its tail both execute."""
    need = 8 * _scan_threads() * BLOCK + 1
    side = int(np.ceil(need ** (1.0 / 3.0)))
    box = float(np.ceil((side * 0.465 + 6.0) / 2.0) * 2.0)
    sc = scenes.liquid_box((box, box, box), (side, side, side), mask=0xffffffff)
    cfg = er.with_count(sc["cfg"], sc["cfg"].particleCount, sc["cfg"].particleCount)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    assert (hip.N + BLOCK - 1) // BLOCK > 8 * _scan_threads()
    state = dict(hip=hip, pos=sc["position"], vel=sc["velocity"])
    yield state
    hip.close()


@pytest.mark.parametrize("what", [w for w, _ in _patterns(1024)])
def test_block_and_scan_edges_large(big, what):
    big["pos"], big["vel"] = _check_patterns(big["hip"], big["pos"], big["vel"], (what,))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges_small(n):
    cfg = scenes.liquid_box_config((8.0, 8.0, 8.0))
    r0 = f32(cfg.r0)
    pos, vel = er.lattice((f32(3) * r0,) * 3, (f32(0.93) * r0,) * 3, (8, 8, 5), velocity=(0.1, 0.2, 0.3))
    pos, vel = pos[:n].copy(), vel[:n].copy()
    vel[:, 0] = np.arange(n, dtype=f32)  # every particle recognisable
    hip = sphmi.owHIPSolver(er.with_count(cfg, n, n), pos, vel)
    _check_patterns(hip, pos, vel)
    hip.close()


# ---------------------------------------------------------------------------------------------- remove_selection
def test_remove_selection_removes_exactly_the_selection():
    sc = _scene("tiny")
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    pos, vel = read_state(hip)
    n = hip.select_surface()
    _, ids, _ = hip.selection()
    assert 0 < n < (pos[:, 3].astype(np.int32) == 1).sum() and ids.size == n
    p, v, m = er.remove(pos, vel, er.id_marks(pos.shape[0], ids))
    assert hip.remove_selection() == n
    assert np.array_equal(np.flatnonzero(hip.edit_map() < 0), np.sort(ids)) and np.array_equal(hip.edit_map(), m)
    assert_state(hip, p, v, "remove_selection")
    with pytest.raises(sphmi.SphError) as ei:
        hip.selection()
    assert _status(ei) == ERR_ORDER
    with pytest.raises(sphmi.SphError) as ei:
        hip.remove_selection()  # the selection is of a state that no longer exists
    assert _status(ei) == ERR_ORDER
    hip.close()


# ---------------------------------------------------------------------------------------------- rules
def _refused(hip, status, call, pos, vel, what):
    with pytest.raises(sphmi.SphError) as ei:
        call()
    assert _status(ei) == status, what + ": " + str(ei.value)
    assert_state(hip, pos, vel, what + ": state untouched")
    return str(ei.value)


@pytest.fixture(scope="module")
def stepped():
    """`wide` with room for 64 more particles, after 3 steps."""
    sc = _scene("wide")
    n = sc["cfg"].particleCount
    cfg = er.with_count(sc["cfg"], n, n + 64)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    for it in range(3):
        hip.step(it)
    yield sc, cfg, hip
    hip.close()


def test_count_only_and_empty_removal_leave_everything_valid(stepped):
    sc, cfg, hip = stepped
    pos, vel = read_state(hip)
    box = er.liquid_quantile_box(pos)
    n_sel = hip.select_surface()
    sel = hip.selection()
    origin = (cfg.xmin, cfg.ymin, cfg.zmin)
    spacing = tuple((getattr(cfg, a + "max") - getattr(cfg, a + "min")) / f32(23) for a in "xyz")
    verts, _ = hip.extract_surface(origin, spacing, (24, 24, 24), iso=0.5, types=(1,))
    normals = hip.surface_normals()
    assert hip.remove_region(box, (1,), count_only=True) == er.region_marks(pos, box, (1,)).sum() > 0
    assert hip.remove_region(None, (1, 3), count_only=True) == hip.N  # counting everything is not removing everything
    assert_state(hip, pos, vel, "count_only")
    for a, b in zip(hip.selection(), sel):
        assert scenes.bits_equal(a, b)
    assert scenes.bits_equal(hip.surface_normals(), normals) and verts.shape[0] > 0
    with pytest.raises(sphmi.SphError) as ei:
        hip.edit_map()  # count_only makes no map
    assert _status(ei) == ERR_ORDER
    # the pinned choice: removing nothing changes nothing, keeps the analysis state, and leaves the identity as the map
    nowhere = (-3.0, -3.0, -3.0, -2.0, -2.0, -2.0)
    for call in (lambda: hip.remove_region(nowhere, (1, 3)), lambda: hip.remove_ids([])):
        assert call() == 0
        assert np.array_equal(hip.edit_map(), np.arange(hip.N))
        assert_state(hip, pos, vel, "empty removal")
        assert hip.selection()[0].size == n_sel and scenes.bits_equal(hip.surface_normals(), normals)
        hip.diagnostics()
    assert hip.add_particles(np.zeros((0, 4), f32), np.zeros((0, 4), f32)) == hip.N and hip.emit_lattice((0, 0, 0), (1, 1, 1), (3, 0, 2)) == 0
    assert hip.selection()[0].size == n_sel


def test_refusals_leave_the_state_untouched(stepped):
    sc, cfg, hip = stepped
    pos, vel = read_state(hip)
    N, r0 = hip.N, f32(cfg.r0)
    o, _ = er.clear_origin(pos, cfg, (2, 2, 2), r0, r0)
    good = np.array([[o[0], o[1], o[2], 1.0], [o[0] + r0, o[1], o[2], 1.0]], f32)
    zero = np.zeros_like(good)
    assert "id %d " % N in _refused(hip, ERR_INVALID, lambda: hip.remove_ids([3, N, 5]), pos, vel, "id out of range")
    _refused(hip, ERR_SIZE, lambda: hip.add_particles(np.repeat(good[:1], 65, 0), np.zeros((65, 4), f32)), pos, vel, "capacity (add)")
    _refused(hip, ERR_SIZE, lambda: hip.emit_lattice(o, (r0,) * 3, (5, 13, 1)), pos, vel, "capacity (emit)")
    for col, val, why in ((0, cfg.xmax + 1.0, "outside the box"), (2, -0.5, "outside the box"), (1, np.nan, "not finite"), (0, np.inf, "not finite"),
                          (3, 2.1, "type"), (3, 0.0, "type"), (3, 4.0, "type")):
        bad = good.copy()
        bad[1, col] = val
        msg = _refused(hip, ERR_INVALID, lambda: hip.add_particles(bad, zero), pos, vel, "add: " + why)
        assert "particle 1 " in msg and why in msg
    msg = _refused(hip, ERR_INVALID, lambda: hip.emit_lattice(o, (r0, cfg.ymax, r0), (2, 3, 2)), pos, vel, "emit outside the box")
    assert "point 2 = (0, 1, 0)" in msg
    _refused(hip, ERR_INVALID, lambda: hip.emit_lattice(o, (r0, np.nan, r0), (2, 2, 2)), pos, vel, "emit not finite")
    _refused(hip, ERR_INVALID, lambda: hip.emit_lattice(o, (r0,) * 3, (2, 2, 2), type_value=2.1), pos, vel, "emit elastic")
    _refused(hip, ERR_INVALID, lambda: hip.emit_lattice(o, (r0,) * 3, (2, -2, 2)), pos, vel, "negative dims")
    _refused(hip, ERR_INVALID, lambda: hip.remove_region(None, (1, 3)), pos, vel, "remove everything")
    _refused(hip, ERR_INVALID, lambda: hip.remove_ids(np.arange(N)), pos, vel, "remove everything by id")
    for types in ((), (0,), (4,), (1, 5)):
        _refused(hip, ERR_INVALID, lambda: hip.remove_region(None, types), pos, vel, "type mask %r" % (types,))
    _refused(hip, ERR_INVALID, lambda: hip.remove_region((0, 0, np.nan, 1, 1, 1), (1,)), pos, vel, "NaN bound")
    hip.diagnostics()  # nothing was invalidated by any of the refusals


def test_elastic_range_is_refused():
    for sc in (_scene("tiny_elastic"), scenes.elastic_offset_box()):
        cfg = sc["cfg"]
        E, off, N = cfg.numOfElasticP, cfg.elasticOffset, cfg.particleCount
        hip = scenes.hip_for(sc)
        hip.step(0)
        pos, vel = read_state(hip)
        msg = _refused(hip, ERR_INVALID, lambda: hip.remove_ids([N - 1, off + 2, off + 1]), pos, vel, "elastic id")
        assert "particle %d " % (off + 1) in msg
        _refused(hip, ERR_INVALID, lambda: hip.remove_region(None, (2,)), pos, vel, "elastic type")
        if off:
            assert "particle 0 " in _refused(hip, ERR_INVALID, lambda: hip.remove_region(None, (3,)), pos, vel, "walls in front of the block")
        liquid = er.region_marks(pos, None, (1,))
        p, v, m = er.remove(pos, vel, liquid, E, off)
        assert hip.remove_region(None, (1,)) == liquid.sum() and np.array_equal(hip.edit_map(), m)
        assert_state(hip, p, v, "drained liquid")
        hip.step(1)
        assert np.isfinite(hip.read_position_buffer()).all()
        hip.close()


def test_slab_solver_is_refused():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    n = sc["cfg"].particleCount
    cfg = er.with_count(sc["cfg"], n, n + 64)
    hip = sphmi.owHIPSolver(cfg, sc["position"], sc["velocity"])
    lay = S.particle_layers(sc["position"], sc["cfg"])
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    pos, vel, _, _ = hip.slab_read()
    r0 = f32(cfg.r0)
    one = np.array([[3 * r0, 3 * r0, 3 * r0, 1.0]], f32)
    for call in (lambda: hip.remove_region(None, (1,)), lambda: hip.remove_region(None, (1,), count_only=True), lambda: hip.remove_ids([1]),
                 lambda: hip.remove_selection(), lambda: hip.add_particles(one, np.zeros_like(one)),
                 lambda: hip.emit_lattice(one[0, :3], (r0,) * 3, (2, 2, 2))):
        with pytest.raises(sphmi.SphError) as ei:
            call()
        assert _status(ei) == ERR_INVALID
        p, v, _, _ = hip.slab_read()
        assert hip._L.sph_particle_count(hip._h) == n and scenes.bits_equal(p, pos) and scenes.bits_equal(v, vel)
    hip.close()


def test_order_rules_after_an_edit():
    sc = _scene("tiny")
    n = sc["cfg"].particleCount
    hip = sphmi.owHIPSolver(er.with_count(sc["cfg"], n, n + 64), sc["position"], sc["velocity"])
    for it in range(2):
        hip.step(it)
    hip.label_components()
    assert hip.remove_ids([7, 9]) == 2 and hip.N == n - 2
    hip.edit_map()
    for call in (hip.diagnostics, hip.particle_measure, lambda: hip.select(), lambda: hip.sample_points([(0.5, 0.5, 0.5)]),
                 lambda: hip.component_diagnostics([0]), lambda: hip.label_components()):
        with pytest.raises(sphmi.SphError) as ei:
            call()
        assert _status(ei) == ERR_ORDER
    hip.step(2)
    hip.diagnostics()
    with pytest.raises(sphmi.SphError) as ei:
        hip.edit_map()  # a step has run
    assert _status(ei) == ERR_ORDER
    assert hip.remove_ids([0]) == 1
    hip.edit_map()
    r0 = f32(sc["cfg"].r0)
    hip.add_particles(np.array([[8 * r0, 12 * r0, 8 * r0, 1.0]], f32), np.zeros((1, 4), f32))
    with pytest.raises(sphmi.SphError) as ei:
        hip.edit_map()  # another edit has run
    assert _status(ei) == ERR_ORDER
    hip.close()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("grow", [False, True])
def test_edit_while_an_asynchronous_read_back_is_outstanding(grow, staged):
    """The buffer holds the pre-edit positions, with the pre-edit byte count, whether the count fell or grew in between. staged:
    the library can page-lock eight caller buffers in place; with those taken the read goes through its pinned staging area and
    sph_read_position_wait's memcpy, the copy that has to use the byte count of the request."""
    sc = _scene("tiny")
    n = sc["cfg"].particleCount
    hip = sphmi.owHIPSolver(er.with_count(sc["cfg"], n, n + ROOM), sc["position"], sc["velocity"])
    hip.step(0)
    want = hip.read_position_buffer()
    held = []
    if staged:
        for _ in range(8):
            held.append(np.empty((n, 4), f32))
            hip.read_position_buffer_async(held[-1])
            hip.wait_position_buffer()
            assert scenes.bits_equal(held[-1], want)
    guard = 64
    raw = np.full((n + ROOM + guard) * 4 + 3, f32(-7.0), f32)[3:]  # (odd offset: not page-aligned, staged or pinned in place alike)
    out = raw[:4 * n]
    hip.read_position_buffer_async(out)
    r0 = f32(sc["cfg"].r0)
    if grow:
        assert hip.emit_lattice((4 * r0, f32(12.5) * r0, 4 * r0), (r0,) * 3, (8, 3, 8)) == 192  # above the liquid
    else:
        assert hip.remove_region(er.liquid_quantile_box(want), (1,)) > 0
    assert hip.N != n
    hip.wait_position_buffer()
    assert scenes.bits_equal(out.reshape(-1, 4), want)
    assert (raw[4 * n:] == f32(-7.0)).all(), "written past the requested bytes"
    hip.step(1)
    assert np.isfinite(hip.read_position_buffer()).all() and hip.read_position_buffer().shape[0] == hip.N
    for buf in held + [out]:
        hip._L.sph_host_unregister(hip._h, buf.ctypes.data)
    hip.close()


def test_edit_map_after_a_refused_removal_is_the_last_successful_one():
    sc = _scene("tiny")
    hip = scenes.hip_for(sc)
    hip.step(0)
    pos, vel = read_state(hip)
    N = hip.N
    _, _, m = er.remove(pos, vel, er.id_marks(N, [7, 9]))
    assert hip.remove_ids([7, 9]) == 2
    for call in (lambda: hip.remove_ids([hip.N]), lambda: hip.remove_region(None, (1, 3)), lambda: hip.remove_region(None, (0,)),
                 lambda: hip.remove_selection()):
        with pytest.raises(sphmi.SphError):
            call()
        got = hip.edit_map()  # the refused call changed nothing: still the map of the removal above, N entries
        assert got.shape == (N,) and np.array_equal(got, m)
    assert hip.remove_region(None, (1,), count_only=True) > 0 and np.array_equal(hip.edit_map(), m)
    hip.close()


def test_gate_and_emitted_wall_continue_like_a_fresh_solver():
    """Boundary particles go (a gate opens: types=(3,)) and come (emit_lattice with type_value=3.0, the velocity holding the
    normal); restatement, then 3 steps against a solver created from the restated arrays and against the oracle."""
    sc = _scene("tiny")
    cfg0 = sc["cfg"]
    n, r0 = cfg0.particleCount, f32(cfg0.r0)
    hip = sphmi.owHIPSolver(er.with_count(cfg0, n, n + ROOM), sc["position"], sc["velocity"])
    for it in range(2):
        hip.step(it)
    pos, vel = read_state(hip)
    gate = (f32(cfg0.xmax) - r0, -np.inf, -np.inf, np.inf, np.inf, np.inf)  # the wall at x = xmax
    marked = er.region_marks(pos, gate, (3,))
    assert 0 < marked.sum() < (pos[:, 3].astype(np.int32) == 3).sum()
    pos, vel, m = er.remove(pos, vel, marked)
    assert hip.remove_region(gate, (3,)) == marked.sum() and np.array_equal(hip.edit_map(), m)
    assert_state(hip, pos, vel, "gate")
    origin = (f32(8) * r0, f32(13) * r0, f32(4) * r0)  # a small plate above the liquid, normal +y
    lp, lv = er.lattice(origin, (r0, r0, r0), (5, 1, 6), velocity=(0.0, 1.0, 0.0), type_value=3.0)
    pos, vel = er.append(pos, vel, lp, lv, cfg0)
    assert hip.emit_lattice(origin, (r0, r0, r0), (5, 1, 6), velocity=(0.0, 1.0, 0.0), type_value=3.0) == 30
    assert_state(hip, pos, vel, "emitted wall")
    assert (pos[-30:, 3] == 3).all()
    cfg = er.with_count(cfg0, pos.shape[0], 0)
    fresh = sphmi.owHIPSolver(cfg, pos, vel)
    from oracle import oraclebind as O
    ora = O.OracleSolver(sphmi.config_dict(cfg), pos, vel, threads=4)
    for it in range(3):
        hip.step(it); fresh.step(it); ora.step()
    N = pos.shape[0]
    for a, b, c, what in ((hip.read_position_buffer(), fresh.read_position_buffer(), ora.buffer("position").reshape(-1, 4)[:N], "position"),
                          (hip.read_velocity_buffer(), fresh.read_velocity_buffer(), ora.buffer("velocity").reshape(-1, 4)[:N], "velocity"),
                          (hip.read_density_buffer(), fresh.read_density_buffer(), ora.buffer("rho")[:N], "rho")):
        assert scenes.bits_equal(a, b), what + ", edited vs fresh: " + scenes.diff_report(a, b)
        assert scenes.bits_equal(a, c), what + ", edited vs oracle: " + scenes.diff_report(a, c)
    hip.close(); fresh.close(); ora.close()


@pytest.mark.parametrize("async_read", [False, True])
def test_simulator_resizes_its_position_buffer(async_read):
    sc = _scene("tiny")
    cfg0 = sc["cfg"]
    n, r0 = cfg0.particleCount, f32(cfg0.r0)
    sim = sphmi.owPhysicsFluidSimulator(er.with_count(cfg0, n, n + ROOM), sc["position"], sc["velocity"])
    s = sim.ocl_solver
    sim.simulationStep(async_read_back=async_read)
    assert sim.getPosition_cpp().shape == (n, 4)
    for k in range(10):  # more resizes than the library has room for page-locked caller buffers
        if k % 2:
            assert s.remove_ids([s.N - 1, s.N - 2]) == 2
        else:
            assert s.emit_lattice((f32(4 + k) * r0, f32(13) * r0, f32(4) * r0), (r0, r0, r0), (1, 1, 3)) == 3
        sim.simulationStep(async_read_back=async_read)
        got = sim.getPosition_cpp()
        assert got.shape == (s.N, 4) and scenes.bits_equal(got, s.read_position_buffer())
    s._L.sph_host_unregister(s._h, sim.position_cpp.ctypes.data)
    s.close()


# ---------------------------------------------------------------------------------------------- driver
def test_driver_emits_and_drains(tmp_path):
    """sphmi_run --capacity --emit-* --drain-*: the `_edit:` lines and the final count equal the Python replay of the schedule."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12))
    cfg0 = sc["cfg"]
    n, r0 = cfg0.particleCount, f32(cfg0.r0)
    o = [float(f32(4) * r0), float(f32(12.5) * r0), float(f32(4) * r0)]
    # the drain clears the inlet (the space above the liquid) before a new block is emitted into it
    drain = [float(f32(3) * r0), float(f32(12) * r0), float(f32(3) * r0), float(f32(9) * r0), float(f32(14.5) * r0), float(f32(9) * r0)]
    out = str(tmp_path / "final.bin")
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "6", "--quiet", "--capacity", str(n + 600),
                        "--emit-lattice"] + ["%.9g" % x for x in o] + ["5", "2", "5", "--emit-velocity", "0", "-0.1", "0", "--emit-every", "2",
                        "--emit-until", "5", "--drain-region"] + ["%.9g" % x for x in drain] + ["--drain-every", "2", "--drain-at", "1",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [tuple(int(x) for x in re.match(r"_edit: step (\d+) removed (\d+) added (\d+) particles (\d+)", l).groups())
             for l in r.stdout.splitlines() if l.startswith("_edit:")]
    hip = sphmi.owHIPSolver(er.with_count(cfg0, n, n + 600), sc["position"], sc["velocity"])
    sp = f32(0.93) * r0
    want = []
    for step in range(6):
        removed = added = 0
        edited = False
        if (step > 0 and step % 2 == 0) or step == 1:
            removed, edited = hip.remove_region([f32(x) for x in drain], (1,)), True
        if step % 2 == 0 and step < 5:
            added, edited = hip.emit_lattice([f32(x) for x in o], (sp, sp, sp), (5, 2, 5), velocity=(0, f32(-0.1), 0)), True
        if edited:
            want.append((step, removed, added, hip.N))
        hip.step(step)
    assert lines == want and len(want) == 4 and [w[1] for w in want] == [0, 50, 0, 50] and [w[2] for w in want] == [50, 0, 50, 50]
    final = np.fromfile(out, f32).reshape(-1, 4)
    assert final.shape[0] == hip.N and scenes.bits_equal(final, hip.read_position_buffer())
    hip.close()
    # misuse exits with status 2 and a message
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "1"]
    for bad in (["--emit-lattice", "1", "1", "1", "2", "2", "2"], ["--capacity", "100000", "--emit-every", "2"],
                ["--capacity", "10", "--emit-lattice", "1", "1", "1", "2", "2", "2"], ["--drain-types", "1"],
                ["--drain-at", "0", "--drain-types", "4"], ["--drain-at", "0", "--drain-region", "0", "0", "nan", "1", "1", "1"]):
        r = subprocess.run([exe] + box + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
