"""CPU tests of the carried-field restatement (tests/fields_ref.py), the yardstick the GPU calls are held to
(tests/test_fields.py): hand-made neighbourhoods with exact answers, the tie of the diffusion sum to forces_ref.Forces (itself
tied to the oracle's K7 stage) bit for bit, a constant field, conservation where the used slots are symmetric, the bounds a
stable substep keeps, painting, edit-following and the region records on hand-made arrays, and the host-side helpers.

Steps before the examined state: `tiny` 1 and 6 (its rows are not truncated, so its used slots are symmetric), the others 4 to 6,
where their velocities differ from particle to particle and their boundary shell is within reach of the liquid."""
import ctypes
import functools
import os

import numpy as np
import pytest

import diag_ref
import fields_ref as flr
import forces_ref as fr
import scenes
import sphmi
from sphmi import frames

f32 = np.float32
HAND_K = dict(hs=f32(8), mass=f32(1), del2W=4.0)
MASKS = [(1,), (1, 2), (1, 2, 3)]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hand_state(types, rho, G=1):
    n = len(types)
    return dict(types=np.array(types, np.float32), rho=np.array(rho, np.float32), keys=np.zeros(n, np.uint32), G=G,
                pos=np.arange(3 * n, dtype=np.float32).reshape(n, 3), ids=np.arange(n)[::-1].copy())


def rows(n, entries):
    ids, dist = -np.ones((n, 32), np.int32), -np.ones((n, 32), np.float32)
    for i, row in entries.items():
        for k, (j, r) in enumerate(row):
            ids[i, k], dist[i, k] = j, r
    return ids, dist


# ---- 1. hand-made neighbourhoods --------------------------------------------------------------------------------------------
def test_two_particles_exchange_exactly():
    state = hand_state([1.1, 1.1], [2, 2])
    ids, dist = rows(2, {0: [(1, 4)], 1: [(0, 4)]})
    D = flr.Diffusion(state, ids, dist, HAND_K, (1,))
    # w = 8 - 4, S_0 = ((0 - 1) * 4) / 2, W = 4 / 2, sD = 1 * (4 / 2); a = 0.125 * 2
    c, sigma, A = D.run([1, 0], 0.125, 1)
    assert D.sD.tolist() == [2, 2] and D.W.tolist() == [2, 2] and D.sums(f32([1, 0]))[0].tolist() == [-2, 2]
    assert c.tolist() == [0.5, 0.5] and sigma == 0.5 and A == 0.25 * 2 + 0.25 * 2
    assert D.asymmetric_pairs() == (2, 0)
    # Jacobi: the second substep starts from (0.5, 0.5), not from a half-updated pair
    assert D.run([1, 0], 0.125, 2)[0].tolist() == [0.5, 0.5]
    assert D.run([1, 0], 0.0625, 2)[0].tolist() == [0.625, 0.375]  # (0.75, 0.25), then 0.75 - 0.125 * 1, 0.25 + 0.125 * 1
    # substeps == 0 measures and changes nothing; through the original-order entry the values land at the original ids (reversed)
    out, sigma0, _ = flr.diffuse(state, ids, dist, HAND_K, [0, 1], 0.125, 0, (1,))
    assert out.tolist() == [0, 1] and sigma0 == 0.5
    assert flr.diffuse(state, ids, dist, HAND_K, [0, 1], 0.0625, 1, (1,))[0].tolist() == [0.25, 0.75]


def test_empty_slot_reach_and_participation():
    """Particle 0: a neighbour, an EMPTY slot, a neighbour, one at dist == hs (not < hs), a boundary neighbour."""
    state = hand_state([1.1, 1.1, 1.1, 1.1, 3.1], [2, 2, 4, 1, 1])
    ids, dist = rows(5, {0: [(1, 4), (-1, -1), (2, 6), (3, 8), (4, 2)]})
    c0 = f32([1, 3, 5, 100, 100])
    D = flr.Diffusion(state, ids, dist, HAND_K, (1,))
    assert D.used[0, :6].tolist() == [True, False, True, False, False, False] and not D.used[1:].any()
    # S_0 = ((3-1)*4)/2 + ((5-1)*2)/4, W_0 = 4/2 + 2/4, sD_0 = 2, a_0 = 0.0625 * 2
    c, sigma, A = D.run(c0, 0.0625, 1)
    assert D.sums(c0)[0].tolist() == [6, 0, 0, 0, 0] and D.W.tolist() == [2.5, 0, 0, 0, 0]
    assert c.tolist() == [1.75, 3, 5, 100, 100] and sigma == f32(0.3125) and A == 0.125 * 6
    assert D.asymmetric_pairs() == (2, 2)  # neither neighbour holds particle 0 in its row
    # with the boundary participating its slot is used: + ((100-1)*6)/1 and + 6/1
    D3 = flr.Diffusion(state, ids, dist, HAND_K, (1, 3))
    assert D3.used[0, :6].tolist() == [True, False, True, False, True, False]
    assert D3.sums(c0)[0][0] == 600 and D3.W[0] == 8.5
    # a particle that does not participate keeps its value and exerts nothing: liquid masked out entirely
    Db = flr.Diffusion(state, ids, dist, HAND_K, (3,))
    assert not Db.used.any() and Db.run(c0, 1.0, 3)[0].tolist() == c0.tolist() and Db.sigma(1.0) == 0
    # an invalid cell key is as good as a foreign type
    state["keys"][1] = 5
    assert flr.Diffusion(state, ids, dist, HAND_K, (1,)).used[0, :3].tolist() == [False, False, True]


# ---- 2. the tie to pinned code ----------------------------------------------------------------------------------------------
SCENE_STEPS = {"tiny": 6, "tiny_compressed": 4, "tiny_elastic": 6}


@functools.lru_cache(maxsize=None)
def oracle_case(name, steps):
    sc = scenes.SCENES[name]()
    cfg = sc["cfg"]
    N = cfg.particleCount
    ora = scenes.oracle_for(sc)
    for _ in range(steps):
        ora.step()
    state, ids, dist = fr.oracle_state(ora, N, cfg.gridCellCount)
    state["ids"] = ora.buffer("particleIndex").reshape(-1, 2)[:N, 1].astype(np.int64)
    ora.close()
    return dict(cfg=cfg, N=N, state=state, ids=ids, dist=dist)


@functools.lru_cache(maxsize=None)
def diffusion_of(name, steps, types):
    c = oracle_case(name, steps)
    return flr.Diffusion(c["state"], c["ids"], c["dist"], flr.constants(c["cfg"]), types)


@pytest.mark.parametrize("name", list(SCENE_STEPS))
def test_sum_is_the_viscous_sum_of_the_force_decomposition(name):
    """With c = one velocity component of every particle (a boundary particle's wall normal included) and all three types
    participating, S_i is forces_ref's unscaled viscous sum, bit for bit, for every non-boundary i."""
    c = oracle_case(name, SCENE_STEPS[name])
    cfg, state = c["cfg"], c["state"]
    F = fr.Forces(state, c["ids"], c["dist"], fr.constants(cfg))
    D = diffusion_of(name, SCENE_STEPS[name], (1, 2, 3))
    mv = F.moving
    assert D.P.all() and mv.sum() > 0 and (~mv).sum() > 0
    assert np.array_equal(D.used[mv], F.used_f[mv])
    for a in range(3):
        S, _ = D.sums(state["vel"][:, a])
        assert np.array_equal(u32(S[mv]), u32(F.S[0, a][mv])), scenes.diff_report(S[mv], F.S[0, a][mv])
        assert np.abs(S[mv]).max() > 0
    # the scale: constants() of the force decomposition derives the same hs, mass and del2W, and sF is sD with the viscosity
    # folded into the mass first (two roundings apart)
    K, KF = flr.constants(cfg), fr.constants(cfg)
    assert K["hs"] == KF["hs"] and float(K["mass"]) == KF["mass"] and K["del2W"] == KF["del2W"]
    x = (KF["del2W"] / state["rho"].astype(np.float64)).astype(np.float32)
    assert np.array_equal(u32(D.sD), u32(K["mass"] * x))
    sF = (KF["massMu"] * x).astype(np.float64)
    assert (np.abs(float(f32(cfg.viscosity)) * D.sD.astype(np.float64) - sF) <= 2.0 ** -22 * sF).all()


@pytest.mark.parametrize("name", list(SCENE_STEPS))
def test_constant_field_is_returned_bit_for_bit(name):
    c = oracle_case(name, SCENE_STEPS[name])
    D = diffusion_of(name, SCENE_STEPS[name], (1, 2, 3))
    const = np.full(c["N"], f32(0.37), np.float32)
    for coefficient in (0.0, 1e-9, 1.0, 1e6):
        out, sigma, A = D.run(const, coefficient, 3)
        assert np.array_equal(u32(out), u32(const)) and A == 0
        assert (sigma > 0) == (coefficient > 0)


def box_field(state):
    """1 in the lower-x half of the particles, 0 elsewhere (sorted order)."""
    x = state["pos"][:, 0]
    return (x < np.median(x)).astype(np.float32)


def stable_coefficient(D):
    return f32(0.5 / float((D.sD.astype(np.float64) * D.W.astype(np.float64))[D.P].max()))


@pytest.mark.parametrize("steps", [1, 6])
@pytest.mark.parametrize("types", MASKS)
def test_conservation_where_the_used_slots_are_symmetric(steps, types):
    """`tiny`: no row is truncated, so every used slot has its mirror with the same stored distance; then the sum of c over
    the participants moves by rounding only: |sum c' - sum c| <= 2^-17 * A, A = sum_i a_i sum_k |term| (fewer than 40 roundings
    of relative size 2^-24 per particle, doubled for margin)."""
    c = oracle_case("tiny", steps)
    D = diffusion_of("tiny", steps, types)
    pairs, lonely = D.asymmetric_pairs()
    assert pairs > 30000 and lonely == 0, (pairs, lonely)
    c0 = box_field(c["state"])
    out, sigma, A = D.run(c0, stable_coefficient(D), 1)
    assert A > 0 and not np.array_equal(out, c0)
    before, after = c0[D.P].astype(np.float64).sum(), out[D.P].astype(np.float64).sum()
    print("tiny steps=%d types=%r: pairs %d, sum %r -> %r, |diff| %.3e, bound %.3e" % (steps, types, pairs, before, after,
                                                                                       abs(after - before), 2.0 ** -17 * A))
    assert abs(after - before) <= 2.0 ** -17 * A


@pytest.mark.parametrize("name", ["tiny_compressed", "tiny_jitter", "tiny_elastic"])
def test_truncated_rows_are_reported_as_asymmetric(name):
    """Rows cut at 32 entries lose the mirror of some slots: the restatement says so (these scenes are not used for conservation)."""
    pairs, lonely = diffusion_of(name, 4, (1, 2, 3)).asymmetric_pairs()
    assert pairs > 30000 and 0 < lonely < pairs // 10, (pairs, lonely)


@pytest.mark.parametrize("name", list(SCENE_STEPS))
@pytest.mark.parametrize("types", [(1,), (1, 2, 3)])
def test_a_stable_substep_keeps_the_bounds(name, types):
    """coefficient = 0.5 / max sD_i W_i: for c_i = 1 every term is <= 0 and the scaled sum >= -0.5; for c_i = 0 the mirror."""
    c = oracle_case(name, SCENE_STEPS[name])
    D = diffusion_of(name, SCENE_STEPS[name], types)
    c0 = box_field(c["state"])
    out, sigma, _ = D.run(c0, stable_coefficient(D), 1)
    assert out.min() >= 0 and out.max() <= 1 and not np.array_equal(out, c0)
    assert 0 < float(sigma) <= 0.5 * (1 + 2.0 ** -22)
    assert np.array_equal(u32(out[~D.P]), u32(c0[~D.P]))


# ---- 3. painting, the edits, the region records -------------------------------------------------------------------------------
def test_painting_follows_the_marking_rule():
    pos = np.array([[0, 0, 0, 1.1], [1, 0, 0, 1.1], [2, 0, 0, 3.1], [1, 5, 0, 1.1], [np.nan, 0, 0, 1.1], [1, 0, 0, 0.5]], np.float32)
    v = np.arange(6, dtype=np.float32)
    out, n = flr.paint_region(v, pos, (1, 0, 0, 2, 1, 1), (1,), 9)  # half-open: x == 1 is inside, x == 2 is not
    assert n == 1 and out.tolist() == [0, 9, 2, 3, 4, 5]
    out, n = flr.paint_region(v, pos, None, (1, 3), -1)  # everywhere: the NaN position fails every comparison, type 0 is no type
    assert n == 4 and out.tolist() == [-1, -1, -1, -1, 4, 5]
    assert flr.paint_region(v, pos, (0, 0, 0, 0, 1, 1), (1,), 9)[1] == 0
    assert flr.paint_ids(v, [5, 0, 5], 7).tolist() == [7, 1, 2, 3, 4, 7]


def test_fields_follow_the_edit_map():
    v = np.arange(6, dtype=np.float32) * f32(1.5)
    m = np.array([0, -1, 1, 2, -1, 3])
    out = flr.follow_removal(v, m)
    assert out.tolist() == [0, 3, 4.5, 7.5]
    ids, _ = frames.track_ids(np.arange(6), m)  # the same map the identities follow
    assert np.array_equal(out, v[ids])
    assert flr.follow_add(out, 2, 0.25).tolist() == [0, 3, 4.5, 7.5, 0.25, 0.25]


def test_region_records_on_a_hand_made_state():
    n = 5
    state = dict(pos=np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32),
                 types=np.array([1.1, 1.1, 2.1, 1.1, 3.1], np.float32), keys=np.array([0, 0, 0, 9, 0], np.uint32), G=4)
    c = f32([0.5, -2, 4, 100, 100])
    d = flr.diag_records(state, c, [diag_ref.EVERYTHING, (1, -1, -1, 9, 1, 1), (7, 7, 7, 8, 8, 8)], (1, 2))
    assert d.shape == (3, 8)
    assert d[0].tolist() == [3, 2.5, 0.25 + 4 + 16, -2, 4, 3, 0, 0]  # particle 3 has an invalid key, 4 is boundary
    assert d[1].tolist() == [2, 2, 20, -2, 4, 2, 0, 0] and not d[2].any()
    c[1] = 0
    d = flr.diag_records(state, c, [diag_ref.EVERYTHING], (1,))
    assert d[0].tolist() == [2, 0.5, 0.25, 0, 0.5, 1, 0, 0]
    s = frames.field_summary(d[0])
    assert s == dict(count=2, mean=0.25, variance=0.125 - 0.0625, min=0.0, max=0.5, tagged=1)
    assert frames.field_summary(np.zeros(8)) == dict(count=0, mean=0.0, variance=0.0, min=0.0, max=0.0, tagged=0)
    with pytest.raises(ValueError):
        frames.field_summary(np.zeros(7))


def test_frames_field_sorted():
    pi = np.array([[7, 2], [7, 0], [9, 1]], np.uint32)
    v = f32([10, 20, 30])
    assert frames.field_sorted(v, pi).tolist() == [30, 10, 20]
    assert np.array_equal(frames.field_sorted(v, pi), flr.field_sorted(v, pi[:, 1]))
    back = frames.invert_particle_index(pi)
    assert np.array_equal(frames.field_sorted(v, pi)[back], v)
    with pytest.raises(ValueError):
        frames.field_sorted(v[:2], pi)


def test_header_binding_and_constants():
    names = ["sph_field_create", "sph_field_release", "sph_field_write", "sph_field_read", "sph_field_set_region",
             "sph_field_set_selection", "sph_field_diffuse", "sph_field_diagnostics"]
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    lib = ctypes.CDLL(sphmi.LIB_PATH)
    for n in names:
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    assert "#define SPH_FIELD_SLOTS 4" in txt and "#define SPH_FIELD_DIAG_WORDS 8" in txt and "#define SPHMI_ABI_VERSION 2" in txt
    assert sphmi.FIELD_SLOTS == flr.FIELD_SLOTS == 4 and sphmi.FIELD_DIAG_WORDS == flr.DIAG_WORDS == len(frames.FIELD_DIAG_FIELDS) == 8
    assert sphmi.ABI_VERSION == 2
    for m in ("field_create", "field_release", "field_read", "field_write", "field_set_region", "field_set_selection",
              "field_diffuse", "field_diagnostics"):
        assert callable(getattr(sphmi.owHIPSolver, m))
