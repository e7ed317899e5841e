"""The analysis chain on the GPU at the states where it can break (scenes: sample_cases.py; what each scene holds is proven on the
CPU by test_sample_edges_host.py). ring_scene(): lone liquid particles with queries at the support boundary
r2 < h*h to the ulp, in the ring where the weights are zero or subnormal, across cell faces, edges and corners, at negative
coordinates: sample_points, sample_gradient_points, the brick walk of sample_grid / sample_gradient_grid with the query as a
brick's first point, streamlines and tracers seeded there. mc_scene(): a lattice of lone particles whose pattern is the
isosurface's inside map: all 256 marching-cubes cases, lattice values equal to iso, velocity fields with iso <= 0, lattices at
the edges of a 256-thread block and two points thick, and the normals of vertices that coincide with their particle. Bit
equality with the numpy restatements throughout; the counts of the edge records are asserted on the device's own output."""
import numpy as np
import pytest

import gradient_ref
import sample_cases as C
import sample_ref
import scenes
import trace_ref
from band_cases import F, INF
from test_sample import assert_bits, bits
from test_sample_edges_host import LINES, PER_LINE, sum_kinds
from test_surface import check_surface
from test_surface_host import _ambiguous_faces

pytestmark = pytest.mark.gpu

MASKS = [(1,), (1, 2, 3)]


@pytest.fixture(scope="module")
def ring():
    sc = C.ring_scene()
    hip = scenes.hip_for(sc)
    hip.step(0)
    state = sample_ref.solver_state(hip)
    # the state the CPU proof was made on: the lone particles where they were put, with the clamp's density
    k = C.Constants(sc["cfg"])
    n = sc["numOfLiquidP"]
    back = hip.buffer("particleIndexBack")[:n].astype(np.int64)
    assert np.array_equal(bits(state["pos"][back]), bits(sc["position"][:n, :3]))
    assert np.array_equal(bits(state["vel"][back]), bits(sc["velocity"][:n, :3]))
    assert np.array_equal(bits(state["rho"][back]), bits(np.full(n, k.rho_lone, F)))
    yield sc, hip, state
    hip.close()


@pytest.mark.parametrize("types", MASKS)
def test_ring_points(ring, types):
    sc, hip, state = ring
    k = C.Constants(sc["cfg"])
    pts = sc["queries"][0]
    got = hip.sample_points(pts, types)
    assert_bits(got, sample_ref.sample_reference(state, pts, types), "sample_points %s" % (types,))
    grad = hip.sample_gradient_points(pts, types)
    assert_bits(grad, gradient_ref.gradient_reference(state, pts, types), "sample_gradient_points %s" % (types,))
    assert np.array_equal(bits(grad[:, :8]), bits(got))
    if types == (1,):
        # on the device's own records: two flushed results would agree with each other
        for rec in (got, grad[:, :8]):
            masks = sum_kinds(k, rec)
            for name, count in PER_LINE.items():
                assert int(masks[name].sum()) == count * LINES, (name, int(masks[name].sum()))
        kind = sc["queries"][3]
        accepted = {o: int(got[kind == C.KINDS.index("edge%+d" % o), 6].sum()) for o in C.EDGE_OFFSETS}
        assert accepted == {o: (LINES if o <= 0 else 0) for o in C.EDGE_OFFSETS}, accepted
        assert np.array_equal(bits(got[kind == -1, 1]), bits(np.full(13, C.r0_shepard(k), F)))
        # a record with n = 1 and zero sums: +0 in the words 0..5 (W = 0 + -0 where a < 0) and in the words behind S
        zero = sum_kinds(k, got)["zero_sums"]
        assert not bits(got[zero][:, :6]).any() and not bits(got[zero][:, 7]).any()
        assert not bits(grad[zero][:, 14:]).any()  # (the words 8..13 are not 0 there: g = t*t is a normal number where t*t*t is 0)
        none = got[:, 6] == 0
        assert none.sum() == 3 * LINES and (bits(grad[none][:, 8:14]) == 0x80000000).all()  # K * 0, K < 0


@pytest.mark.parametrize("types", MASKS)
@pytest.mark.parametrize("dims", [(2, 2, 2), (4, 4, 4)])
def test_ring_bricks(ring, dims, types):
    """The brick walk with an edge state in lane 0: the query is the first point of a brick whose other points lie h/2 apart,
    toward the particle, away from it, and alternating."""
    sc, hip, state = ring
    k = C.Constants(sc["cfg"])
    calls = C.brick_calls(sc, dims)
    assert len(calls) > 1000
    pts = np.concatenate([sample_ref.grid_points(o, s, d).reshape(-1, 3) for _, o, s, d in calls])
    want = gradient_ref.gradient_reference(state, pts, types)
    n = dims[0] * dims[1] * dims[2]
    got = np.empty((len(calls), n, 32), np.float32)
    got8 = np.empty((len(calls), n, 8), np.float32)
    for c, (_, o, s, d) in enumerate(calls):
        assert (sample_ref.brick_box_cells(o, s, d, k.h, sc["cfg"].hashGridCellSizeInv) <= 64).all()
        got8[c] = hip.sample_grid(o, s, d, types).reshape(n, 8)
        got[c] = hip.sample_gradient_grid(o, s, d, types).reshape(n, 32)
    assert_bits(got8.reshape(-1, 8), want[:, :8], "sample_grid %s %s" % (dims, types))
    assert_bits(got.reshape(-1, 32), want, "sample_gradient_grid %s %s" % (dims, types))
    if types == (1,):  # lane 0 holds the edge states, on the device's own output
        qi = np.array([c[0] for c in calls])
        lane0 = got8[:, 0]
        direct = hip.sample_points(sc["queries"][0][qi], types)
        assert np.array_equal(bits(lane0), bits(direct))
        masks = sum_kinds(k, lane0)
        assert all(int(masks[name].sum()) > 50 for name in PER_LINE), {name: int(m.sum()) for name, m in masks.items()}


@pytest.mark.parametrize("types", MASKS)
def test_ring_grid_at_the_path_threshold(ring, types):
    """Spacing 2 h / 3 as the library computes it takes the brick walk, one float above it the point walk."""
    sc, hip, state = ring
    k = C.Constants(sc["cfg"])
    pts, owner, direction, kind, _ = sc["queries"]
    lim = F(F(F(2.0) * k.h) / F(3.0))
    for name in ("edge+0", "w_first", "s_zero"):
        qi = int(np.flatnonzero((owner == 0) & (direction == 0) & (kind == C.KINDS.index(name)))[0])
        for sp in (lim, np.nextafter(lim, INF)):
            for sign in (1, -1):
                o, s, d = pts[qi], np.array([-sp, sign * sp, sp], F), (4, 4, 4)
                g = sample_ref.grid_points(o, s, d).reshape(-1, 3)
                assert_bits(hip.sample_grid(o, s, d, types).reshape(-1, 8), sample_ref.sample_reference(state, g, types), "grid at %r" % sp)
                assert_bits(hip.sample_gradient_grid(o, s, d, types).reshape(-1, 32), gradient_ref.gradient_reference(state, g, types),
                            "gradient grid at %r" % sp)


@pytest.mark.parametrize("mode", ["time", "arc"])
@pytest.mark.parametrize("integrator", ["euler", "midpoint"])
def test_ring_streamlines(ring, integrator, mode):
    sc, hip, state = ring
    k = C.Constants(sc["cfg"])
    pts = sc["queries"][0]
    m, i = trace_ref.TIME if mode == "time" else trace_ref.ARC, trace_ref.EULER if integrator == "euler" else trace_ref.MIDPOINT
    step = C.TRACE_STEPS[m](k)
    for types in MASKS:
        verts, lengths, status = hip.streamlines(pts, types, step=step, mode=mode, integrator=integrator, max_steps=C.TRACE_MAX_STEPS)
        rv, rl, rs = trace_ref.streamlines(state, pts, types, step=step, mode=m, integrator=i, max_steps=C.TRACE_MAX_STEPS)
        assert np.array_equal(lengths, rl) and np.array_equal(status, rs), (types, np.flatnonzero((lengths != rl) | (status != rs))[:8])
        assert_bits(verts.reshape(-1, 4), rv.reshape(-1, 4), "streamline vertices %s" % (types,))
        # one advect of tracers set on the seeds: vertex 1 where the curve has one, the seed and the curve's code elsewhere
        hip.tracers_set(pts)
        hip.tracers_advect(types, step=step, mode=mode, integrator=integrator)
        pos, tstatus, steps = hip.tracers()
        moved = lengths >= 2
        assert moved.any() and (~moved).any()
        assert np.array_equal(bits(pos[moved, :3]), bits(verts[moved, 1, :3])) and (tstatus[moved] == trace_ref.MOVING).all()
        assert np.array_equal(bits(pos[~moved, :3]), bits(pts[~moved])) and np.array_equal(tstatus[~moved], status[~moved])
        assert np.array_equal(bits(pos[:, 3]), bits(verts[:, 0, 3])) and (steps == 1).all()
        if types == (1,):
            rec = hip.sample_points(pts, types)
            s_zero = rec[:, 1] == 0
            assert (s_zero & (rec[:, 6] == 1)).sum() >= 7 * LINES and (s_zero & (rec[:, 6] == 0)).sum() == 3 * LINES
            assert (lengths[s_zero] == 1).all() and (status[s_zero] == trace_ref.LEFT_MATTER).all()  # whatever its n
            ringed = sum_kinds(k, rec)["s_subnormal"]
            still = ringed & (verts[:, 0, 3] == 0)  # every product v * vel vanished: the velocity is 0 / S
            assert still.sum() > 0 and (status[still] == trace_ref.STAGNANT).all()
            lost = ringed & (status == trace_ref.LEFT_MATTER)
            assert lost.sum() > 0  # the ring is one-sided: these went where S == 0
            if integrator == "euler":
                assert (lengths[ringed & ~still] >= 2).all()
            else:
                assert (lengths[ringed] >= 2).any() and (lost & (lengths == 1)).any()
    hip.tracers_set(None)


def test_ring_calls_are_read_only():
    sc = C.ring_scene()
    k = C.Constants(sc["cfg"])
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    a.step(0)
    b.step(0)
    pts = sc["queries"][0]
    a.sample_points(pts, (1, 2, 3))
    a.sample_gradient_points(pts, (1,))
    for _, o, s, d in C.brick_calls(sc, (4, 4, 4))[:40]:
        a.sample_grid(o, s, d, (1, 2, 3))
        a.sample_gradient_grid(o, s, d, (1,))
    a.streamlines(pts, (1,), step=C.TRACE_STEPS[1](k), mode="arc", integrator="midpoint", max_steps=C.TRACE_MAX_STEPS)
    a.tracers_set(pts)
    a.tracers_advect((1,), step=C.TRACE_STEPS[0](k), mode="time", integrator="euler")
    for read in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(bits(getattr(a, read)()), bits(getattr(b, read)())), read
    a.step(1)
    b.step(1)
    assert np.array_equal(bits(a.read_position_buffer()), bits(b.read_position_buffer()))
    a.close()
    b.close()


# ---- marching cubes ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc():
    out = {}
    for jitter in (0.2, 0):
        sc = C.mc_scene(jitter)
        hip = scenes.hip_for(sc)
        hip.step(0)
        out[jitter] = (sc, hip)
    yield out
    for _, hip in out.values():
        hip.close()


def _lattice_field(hip, lattice, word=1, types=(1,)):
    o, s, d = lattice
    return hip.sample_grid(o, s, d, types)[..., word]


def test_mc_every_case(mc):
    sc, hip = mc[0.2]
    lattice = C.mc_lattice(sc["cfg"])
    f = _lattice_field(hip, lattice)
    inside = f >= F(0.5)
    assert np.array_equal(inside, sc["pattern"])
    cases = np.unique(C.cases_of(inside))
    assert cases.size == 256
    ambiguous = set()
    for c in cases:
        ambiguous.update(_ambiguous_faces(int(c)))
    assert ambiguous == {(fi, d) for fi in range(6) for d in (0, 1)}
    check_surface(hip, *lattice, 0.5, "shepard", (1,), min_tris=5000)


def test_mc_iso_between_the_occupied_values(mc):
    sc, hip = mc[0.2]
    lattice = C.mc_lattice(sc["cfg"])
    f = _lattice_field(hip, lattice)
    occupied = f[sc["pattern"]]
    assert (occupied < F(0.95)).sum() > 100 and (occupied >= F(0.95)).sum() > 100  # some occupied points are outside
    check_surface(hip, *lattice, 0.95, "shepard", (1,), min_tris=1000)


def _degenerate(hip, lattice, iso):
    """check_surface, then the device's mesh against the restatement's counts of t == 0, t == 1, vertices on lattice points and
    zero-area triangles."""
    verts, tris = check_surface(hip, *lattice, iso, "shepard", (1,))  # (closed: the topology check works on indices)
    f = _lattice_field(hip, lattice)
    t0, t1, on, flat = C.degenerate_counts(f, lattice[0], lattice[1], iso, verts, tris)
    assert t0 > 0 and t1 > 0 and on == t0 + t1 and flat > 0, (t0, t1, on, flat)
    return verts, tris, (t0, t1, on, flat)


def test_mc_iso_on_a_lattice_value(mc):
    sc, hip = mc[0.2]
    lattice = C.mc_lattice(sc["cfg"])
    f = _lattice_field(hip, lattice)
    iso = f[C.mc_iso_point(sc["pattern"])]
    assert (f == iso).sum() == 1
    _degenerate(hip, lattice, iso)


def test_mc_every_vertex_on_a_particle(mc):
    """Particles on their lattice points, iso the field's value there (two ulps below 1: DESIGN.md 39): f >= iso holds with equality
    at every inside point, every t is 0 or 1, every vertex lies on its particle, where the gradient vanishes: the len == 0 branch of
    sph_surface_normals."""
    sc, hip = mc[0]
    k = C.Constants(sc["cfg"])
    lattice = C.mc_lattice(sc["cfg"])
    iso = C.r0_shepard(k)
    f = _lattice_field(hip, lattice)
    assert np.array_equal(bits(f[sc["pattern"]]), bits(np.full(int(sc["pattern"].sum()), iso, F))) and not f[~sc["pattern"]].any()
    verts, tris, (t0, t1, on, flat) = _degenerate(hip, lattice, iso)
    assert on == verts.shape[0] > 3000
    normals = hip.surface_normals()
    state = sample_ref.solver_state(hip)
    want = gradient_ref.normals_reference(gradient_ref.gradient_reference(state, verts, (1,)), 1)
    assert np.array_equal(bits(normals), bits(want))
    particles = set(map(bytes, np.ascontiguousarray(sc["position"][:, :3]).view(np.uint8).reshape(-1, 12)))
    on_particle = np.array([bytes(v) in particles for v in np.ascontiguousarray(verts).view(np.uint8).reshape(-1, 12)])
    assert on_particle.sum() == verts.shape[0]
    assert not bits(normals[on_particle]).any()  # (0, 0, 0), +0
    v, t = hip.extract_surface(*lattice, iso=np.nextafter(iso, INF), field="shepard", types=(1,))
    assert v.shape[0] == 0 and t.shape[0] == 0  # one ulp above: nothing is inside


def test_mc_normals(mc):
    sc, hip = mc[0.2]
    lattice = C.mc_lattice(sc["cfg"])
    verts, tris = check_surface(hip, *lattice, 0.5, "shepard", (1,))
    normals = hip.surface_normals()
    state = sample_ref.solver_state(hip)
    want = gradient_ref.normals_reference(gradient_ref.gradient_reference(state, verts, (1,)), 1)
    assert np.array_equal(bits(normals), bits(want))
    assert (np.abs(np.sqrt((normals.astype(np.float64) ** 2).sum(1)) - 1) < 1e-6).all()


def test_mc_other_fields(mc):
    sc, hip = mc[0.2]
    k = C.Constants(sc["cfg"])
    lattice = C.mc_lattice(sc["cfg"])
    check_surface(hip, *lattice, F(0.5) * k.rho_lone, "density", (1,), min_tris=5000)  # half a lone particle's density
    vx = _lattice_field(hip, lattice, 2)
    pat = sc["pattern"]
    assert (vx[pat] > 0).sum() > 100 and (vx[pat] < 0).sum() > 100 and (vx[pat] == 0).sum() > 20 and not bits(vx[~pat]).any()
    # empty space (+0) is inside for iso = 0 and for a negative iso, so the mesh reaches the border
    check_surface(hip, *lattice, 0.0, "vx", (1,), closed=False, min_tris=1000)
    check_surface(hip, *lattice, -5e-4, "vx", (1,), closed=False, min_tris=1000)
    check_surface(hip, *lattice, -0.0, "vx", (1,), closed=False, min_tris=1000)


@pytest.mark.parametrize("name", ["255", "256", "258", "thin x", "thin xy", "thin xyz", "empty"])
def test_mc_small_lattices(mc, name):
    sc, hip = mc[0.2]
    o, s, d = C.mc_small_lattices(sc["cfg"])[name]
    verts, tris = check_surface(hip, o, s, d, 0.5, "shepard", (1,), closed=False, min_tris=0)
    if name != "thin xyz":
        assert (tris.shape[0] == 0) == (name == "empty")
    check_surface(hip, o, s, d, 0.0, "vx", (1,), closed=False, min_tris=0)
