"""CPU proof that the scenes of tests/sample_cases.py hold the states they are meant to carry to the device: with
the numpy restatements of the contracts (sample_ref, trace_ref, surface_ref) on a state built from the scene, the query set of
ring_scene() holds, for every lone particle and every direction, queries accepted and rejected within 8 ulps of each other,
records with n = 1 and all-zero sums, with subnormal sums, with W != 0 and S == 0, with a normal S and subnormal velocity
products, and the r = 0 record; the pairs across faces, edges and corners lie in different cells; no accepted pair needs the
margin of sample_axis_range; mc_scene reaches all 256 marching-cubes cases and the degenerate vertices. No GPU needed."""
import numpy as np
import pytest

import sample_cases as C
import sample_ref
import scenes
import surface_ref
import trace_ref
from band_cases import F, INF, first_in_cell, last_in_cell, ulp_steps
from test_surface_host import _ambiguous_faces

LINES = 13 * 12  # lone particles x directions


@pytest.fixture(scope="module")
def ring():
    sc = C.ring_scene()
    state = C.synthetic_state(sc)
    pts = sc["queries"][0]
    return sc, state, sample_ref.sample_reference(state, pts, (1,))


def sum_kinds(k, rec):
    """Masks over sample records of a state of lone particles: what the sums W and S behind the words 0 and 1 were. The words are
    (float)massWpoly6 (1.7e33 with the scenes' constants) times the sums, so a subnormal sum shows as a word below massWpoly6 * 2^-126."""
    edge = F(k.massWpoly6) * C.TINY
    n1 = rec[:, 6] == 1
    return dict(zero_sums=n1 & (rec[:, :6] == 0).all(1), w_subnormal=n1 & (rec[:, 0] > 0) & (rec[:, 0] < edge),
                s_subnormal=n1 & (rec[:, 1] > 0) & (rec[:, 1] < edge), s_zero_w_not=n1 & (rec[:, 1] == 0) & (rec[:, 0] != 0))


# records per line (one particle, one direction) of each kind of sums, by construction of sample_cases.KINDS
PER_LINE = dict(zero_sums=5, w_subnormal=4, s_subnormal=4, s_zero_w_not=2)


def test_lone_particles_are_lone():
    sc = C.ring_scene()
    cfg = sc["cfg"]
    k = C.Constants(cfg)
    n = sc["numOfLiquidP"]
    assert n == 13 and len(sc["lone"]) == n
    p = sc["position"][:n, :3].astype(np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) + np.eye(n) * 1e9
    assert d.min() > 2.1 * float(k.h)
    vel = sc["velocity"][:n, :3]
    assert (np.abs(vel) > 5e-4).all() and (np.abs(vel) < 5e-3).all()
    assert all(len(set(np.abs(v).tolist())) == 3 for v in vel)
    # one oracle step: no neighbour weighs enough to lift a lone particle's density above the clamp
    ora = scenes.oracle_for(sc, threads=8)
    ora.step()
    back = ora.buffer("particleIndexBack")[:n].astype(np.int64)
    rho = ora.buffer("rho")[:cfg.particleCount][back]
    ora.close()
    assert np.array_equal(rho.view(np.uint32), np.full(n, k.rho_lone, F).view(np.uint32)), rho
    assert abs(float(k.rho_lone) - 164.2486) < 1e-3


def test_every_line_holds_every_kind(ring):
    sc, state, rec = ring
    k = C.Constants(sc["cfg"])
    pts, owner, direction, kind, _ = sc["queries"]
    assert pts.shape[0] == LINES * len(C.KINDS) + 13
    assert rec[:, 6].max() == 1  # no query selects two liquid particles
    masks = sum_kinds(k, rec)
    s_normal = C.KINDS.index("s_normal")
    for i in range(13):
        vel = sc["velocity"][i, :3]
        for dn in range(12):
            line = (owner == i) & (direction == dn)
            assert line.sum() == len(C.KINDS)
            accepted = [int(rec[line & (kind == C.KINDS.index("edge%+d" % o)), 6][0]) for o in C.EDGE_OFFSETS]
            assert accepted == [1, 1, 1, 1, 0, 0, 0], (i, dn, accepted)  # 4 accepted, 3 rejected, within 8 ulps of the last accepted
            for name, count in PER_LINE.items():
                assert int((masks[name] & line).sum()) == count, (i, dn, name)
            # normal S, subnormal velocity products: U = v * vel below 2^-126 in every component, and not 0
            q = pts[line & (kind == s_normal)][0]
            ok, w, v = C.lone_sums(k, sc["position"][i, :3], q)
            assert ok and v >= C.TINY
            u = np.abs((v * vel).astype(F))
            assert ((u > 0) & (u < C.TINY)).all(), (i, dn, u)
            r = rec[line & (kind == s_normal)][0]
            assert r[1] >= F(k.massWpoly6) * C.TINY and not np.array_equal(r[2:5].view(np.uint32), vel.view(np.uint32))
    for name, count in PER_LINE.items():
        assert int(masks[name].sum()) == count * LINES
    # r = 0: the query is the particle; its Shepard word is (float)massWpoly6 * (hs6 * (1 / rho)), two ulps below 1
    own = rec[kind == -1]
    assert own.shape[0] == 13
    assert np.array_equal(own[:, 1].view(np.uint32), np.full(13, C.r0_shepard(k), F).view(np.uint32))
    assert C.r0_shepard(k) == ulp_steps(F(1), -2)


def _cell(cfg, x):
    """(int)(x * cellSizeInv): truncation toward zero, also below zero."""
    return int(np.trunc(F(F(x) * F(cfg.hashGridCellSizeInv))))


def test_cross_pairs_lie_in_different_cells(ring):
    sc, _, rec = ring
    cfg = sc["cfg"]
    pts, owner, direction, kind, crossed = sc["queries"]
    seen = {}
    for qi in np.flatnonzero(crossed.any(1)):
        p = sc["position"][owner[qi], :3]
        for a in range(3):
            if crossed[qi, a]:
                assert _cell(cfg, p[a]) != _cell(cfg, pts[qi, a]), (qi, a)
        seen.setdefault((sc["lone"][owner[qi]][0], int(crossed[qi].sum())), []).append(int(rec[qi, 6]))
    for name, where, _ in sc["lone"]:
        faces = sum(w in ("hi", "lo") for w in where)
        for n_axes in range(1, faces + 1):  # a face particle: across its face; a corner particle: across a face, an edge and the corner
            got = seen[name, n_axes]
            assert 1 in got and 0 in got, (name, n_axes)
    # the particles of cell 0: queries at negative coordinates truncate to cell 0 too
    neg = np.flatnonzero((pts < 0).any(1))
    assert neg.size >= 3 * len(C.KINDS) - 3
    assert {sc["lone"][i][0] for i in owner[neg]} == {"zero x", "zero y", "zero z"}
    for qi in neg:
        a = int(np.flatnonzero(pts[qi] < 0)[0])
        assert _cell(cfg, pts[qi, a]) == 0 and _cell(cfg, sc["position"][owner[qi], a]) == 0
    assert set(rec[neg, 6].tolist()) == {0.0, 1.0}


def _range_without_margin(c, h, inv):
    ul, uh = (F(c) - F(h)) * F(inv), (F(c) + F(h)) * F(inv)
    return int(np.trunc(ul)), int(np.trunc(uh))


def test_no_accepted_pair_needs_the_margin(ring):
    """The margin witness: an accepted pair whose particle's cell the query's range misses once the margin terms of
    sample_axis_range are dropped. The search over every face of the declared grid (the particle on the last float below and the
    first float above the face, the query 0 .. 8 ulps inside the last accepted coordinate on either side) and over the scene's own
    accepted queries finds none, and the committed form holds every pair: r2 < h*h implies |c - x| <= h, so fl(c - h) <= x <= fl(c + h),
    and the product with cellSizeInv and the truncation are monotone."""
    sc, _, rec = ring
    cfg = sc["cfg"]
    k = C.Constants(cfg)
    h, inv = F(cfg.h), F(cfg.hashGridCellSizeInv)
    witnesses, pairs = [], 0

    def check(x, c):
        nonlocal pairs
        pairs += 1
        b = _cell(cfg, x)
        lo, hi = sample_ref.axis_cell_range(np.array([c], F), h, inv)
        assert lo[0] <= b <= hi[0], (x, c)
        lo0, hi0 = _range_without_margin(c, h, inv)
        if not lo0 <= b <= hi0:
            witnesses.append((x, c))

    for b in range(cfg.gridCellsX):
        for x in (last_in_cell(cfg, b), first_in_cell(cfg, b), F(F(0.01) * h) if b == 0 else first_in_cell(cfg, b)):
            for away in (1, -1):
                p = np.array([x, x, x], F)
                q0 = p.copy()
                q0[0] = F(x + F(away) * F(0.3) * h)
                edge = C.last_true(lambda q: C.lone_sums(k, p, q)[0], p, q0, 0, away, F(1.1) * h)
                for o in range(9):
                    check(x, ulp_steps(edge, -o * away))
    pts, owner = sc["queries"][0], sc["queries"][1]
    for qi in np.flatnonzero(rec[:, 6] == 1):
        for a in range(3):
            check(sc["position"][owner[qi], a], pts[qi, a])
    assert pairs > 1000
    assert witnesses == []  # the margin cannot be observed at these grids


def test_trace_on_the_ring(ring):
    """What the GPU test asserts about the curves, on the synthetic state: a seed with S == 0 stops at vertex 0 with LEFT_MATTER
    whatever its n, seeds in the subnormal ring take a step (or are STAGNANT where the velocity products vanish), and the ring is one-sided: some of them land where S == 0."""
    sc, state, rec = ring
    k = C.Constants(sc["cfg"])
    pts = sc["queries"][0]
    ringed = (rec[:, 1] > 0) & (rec[:, 1] < F(k.massWpoly6) * C.TINY)
    s_zero = rec[:, 1] == 0
    assert (s_zero & (rec[:, 6] == 1)).sum() > 0 and (s_zero & (rec[:, 6] == 0)).sum() > 0 and ringed.sum() > 0
    for integrator in (trace_ref.EULER, trace_ref.MIDPOINT):
        for mode, step in C.TRACE_STEPS.items():
            verts, lengths, status = trace_ref.streamlines(state, pts, (1,), step=step(k), mode=mode, integrator=integrator,
                                                           max_steps=C.TRACE_MAX_STEPS)
            assert (lengths[s_zero] == 1).all() and (status[s_zero] == trace_ref.LEFT_MATTER).all()
            lost = ringed & (status == trace_ref.LEFT_MATTER)
            assert lost.sum() > 0
            # where S is so small that every product v * vel is 0 the velocity is 0 / S: the seed is STAGNANT, not LEFT_MATTER
            still = ringed & (verts[:, 0, 3] == 0)
            assert still.sum() > 0 and (status[still] == trace_ref.STAGNANT).all() and (lengths[still] == 1).all()
            if integrator == trace_ref.EULER:
                assert (lengths[ringed & ~still] >= 2).all()  # the velocity is a quotient of subnormal sums, and a step is taken with it
            else:
                assert (lengths[ringed] >= 2).any() and (lost & (lengths == 1)).any()  # (the midpoint of some lies where S == 0)


# ---- mc_scene -----------------------------------------------------------------------------------------------------------------------
def _shepard_lattice(sc, lattice=None):
    o, s, dims = lattice or C.mc_lattice(sc["cfg"])
    g = sample_ref.grid_points(o, s, dims).reshape(-1, 3)
    rec = sample_ref.sample_reference(C.synthetic_state(sc), g, (1,)).reshape(dims[2], dims[1], dims[0], 8)
    return rec, o, s, dims


def test_mc_scene_is_lone_and_its_pattern_is_the_field():
    for jitter in (0.2, 0):
        sc = C.mc_scene(jitter)
        cfg = sc["cfg"]
        k = C.Constants(cfg)
        assert 1000 < cfg.particleCount < 1200 and cfg.cellIdMask == 0xffffffff
        ora = scenes.oracle_for(sc, threads=8)
        ora.step()
        rho = ora.buffer("rho")[:cfg.particleCount]
        ora.close()
        assert (rho.view(np.uint32) == k.rho_lone.view(np.uint32)).all()
        rec, o, s, dims = _shepard_lattice(sc)
        pat = sc["pattern"]
        assert np.array_equal(rec[..., 6] == 1, pat) and (rec[..., 6] <= 1).all()
        f = rec[..., 1]
        assert (f[~pat] == 0).all()
        if jitter:
            assert f[pat].min() > 0.9 and f[pat].max() < 1
        else:
            assert (f[pat].view(np.uint32) == C.r0_shepard(k).view(np.uint32)).all()
        # neighbouring lattice points are farther than 1.15 h from any foreign particle
        g = sample_ref.grid_points(o, s, dims).reshape(-1, 3).astype(np.float64)
        p = sc["position"][:, :3].astype(np.float64)
        d = np.sqrt(((g[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        own = np.full(g.shape[0], -1)
        own[pat.reshape(-1)] = np.arange(p.shape[0])
        d[np.flatnonzero(own >= 0), own[own >= 0]] = np.inf
        assert d.min() > 1.15 * float(k.h)


def test_mc_scene_reaches_every_case():
    sc = C.mc_scene(0.2)
    rec, o, s, dims = _shepard_lattice(sc)
    f = rec[..., 1]
    inside = f >= F(0.5)
    assert np.array_equal(inside, sc["pattern"])
    border = np.ones(inside.shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert not inside[border].any()
    cases = np.unique(C.cases_of(inside))
    assert cases.size == 256
    ambiguous = set()
    for c in cases:
        ambiguous.update(_ambiguous_faces(int(c)))
    assert ambiguous == {(fi, d) for fi in range(6) for d in (0, 1)}
    verts, tris = surface_ref.surface_reference(f, o, s, 0.5)
    assert tris.shape[0] > 5000
    assert surface_ref.directed_edge_report(tris, verts.shape[0]) is None


def test_mc_scene_degenerate_vertices():
    sc = C.mc_scene(0.2)
    rec, o, s, dims = _shepard_lattice(sc)
    f = rec[..., 1]
    k_, j_, i_ = C.mc_iso_point(sc["pattern"])
    iso = f[k_, j_, i_]
    assert (f == iso).sum() == 1 and iso > 0.9
    verts, tris = surface_ref.surface_reference(f, o, s, iso)
    t0, t1, on, flat = C.degenerate_counts(f, o, s, iso, verts, tris)
    assert t0 >= 1 and t1 >= 1 and on == t0 + t1 and flat >= 1, (t0, t1, on, flat)
    assert surface_ref.directed_edge_report(tris, verts.shape[0]) is None  # the topology check works on indices
    # every particle on its lattice point, iso the field's value there: every vertex lies on a lattice point
    sc = C.mc_scene(0)
    k = C.Constants(sc["cfg"])
    rec, o, s, dims = _shepard_lattice(sc)
    f = rec[..., 1]
    iso = C.r0_shepard(k)
    verts, tris = surface_ref.surface_reference(f, o, s, iso)
    t0, t1, on, flat = C.degenerate_counts(f, o, s, iso, verts, tris)
    assert verts.shape[0] > 3000 and t0 + t1 == verts.shape[0] == on and t0 > 0 and t1 > 0
    assert flat > 0
    assert surface_ref.directed_edge_report(tris, verts.shape[0]) is None
    # one ulp above, nothing is inside
    v, t = surface_ref.surface_reference(f, o, s, np.nextafter(iso, INF))
    assert v.shape[0] == 0 and t.shape[0] == 0


def test_mc_small_lattices_hold_their_counts():
    sc = C.mc_scene(0.2)
    lat = C.mc_small_lattices(sc["cfg"])
    sizes = {name: int(np.prod(d)) for name, (_, _, d) in lat.items()}
    assert (sizes["255"], sizes["256"], sizes["258"]) == (255, 256, 258)
    tri = {}
    for name, (o, s, d) in lat.items():
        rec, _, _, _ = _shepard_lattice(sc, (o, s, d))
        v, t = surface_ref.surface_reference(rec[..., 1], o, s, 0.5)
        tri[name] = t.shape[0]
    assert tri["empty"] == 0 and min(tri[n] for n in ("255", "256", "258", "thin x", "thin xy")) > 0, tri


def _oracle_state(sc, steps):
    """A sample_ref state from the oracle's sorted state of step `steps`."""
    cfg = sc["cfg"]
    N = cfg.particleCount
    ora = scenes.oracle_for(sc, threads=8)
    for _ in range(steps):
        ora.step()
    pi = ora.buffer("particleIndex").reshape(-1, 2)
    state = dict(pos=ora.buffer("sortedPosition").reshape(-1, 4)[:N, :3].copy(), vel=ora.buffer("sortedVelocity").reshape(-1, 4)[:N, :3].copy(),
                 rho=ora.buffer("rho")[:N].copy(), p=ora.buffer("pressure")[:N].copy(),
                 types=ora.buffer("position").reshape(-1, 4)[:N][pi[:, 1].astype(np.int64), 3].copy(), keys=pi[:, 0].copy(),
                 G=int(cfg.gridCellCount), h=float(cfg.h), simScale=float(cfg.simulationScale),
                 massWpoly6=float(cfg.mass) * float(cfg.Wpoly6Coefficient))
    ora.close()
    return state


@pytest.mark.parametrize("name", ["tiny", "tiny_elastic", "config1"])
def test_cases_the_liquid_lattices_reach(name):
    """A measurement (DESIGN.md 39 records it; the number is not asserted): how many of the 256 cases the lattices of
    test_surface.py's smooth-liquid tests reach (padded lattice at h/2, Shepard field of the liquid, iso 0.5, after 3 steps)."""
    from test_surface import padded_lattice
    sc = scenes.config1() if name == "config1" else scenes.SCENES[name]()
    state = _oracle_state(sc, 3)
    o, s, dims = padded_lattice(sc["cfg"], 0.5)
    g = sample_ref.grid_points(o, s, dims).reshape(-1, 3)
    f = sample_ref.sample_reference(state, g, (1,))[:, 1].reshape(dims[2], dims[1], dims[0])
    cases = np.unique(C.cases_of(f >= F(0.5)))
    print("%s: lattice %s, %d of 256 cases" % (name, dims, cases.size))
    assert 2 < cases.size <= 256
