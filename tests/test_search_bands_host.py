"""The search bands without a GPU (band_ref.py restates csrc/sph_bands.hip). On sorted states of the oracle: every
candidate of a y / z / yz neighbour cell within the filter radius of a visiting particle carries the flag of the band the search
kernel stages for that row of cells, and the banded candidate totals of a workgroup never exceed the full ones. On hand-made
states: the face distances Rb exactly, one ulp inside and one ulp outside, on both sides of both axes; a particle exactly on a
cell face and one exactly on a half-cell plane; negative coordinates; a particle in the lo and the hi band of one axis."""
import numpy as np
import pytest

import band_ref
import scenes
from test_fn_staging import SCENE as FN_SCENE, oracle_states, staged_totals
from test_gpu_parity import canon_ora

F = np.float32


def _state(canon):
    keys = canon["particleIndex"].reshape(-1, 2)[:, 0]
    return canon["sortedPosition"][:, :3], keys, canon["gridCellIndexFixedUp"]


def _oracle_state(sc, steps=1):
    N = sc["cfg"].particleCount
    ora = scenes.oracle_for(sc, threads=8)
    for _ in range(steps):
        ora.step()
    out = canon_ora(ora, N)
    ora.close()
    return out


def _check(name, cfg, canon):
    pos, keys, start = _state(canon)
    flags = band_ref.band_flags(pos, keys, cfg)
    bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg, flags)
    assert not bad, "%s: %d candidates within the filter radius are not in their row's band, e.g. (P, Q, slot) %s" % (name, len(bad), bad[:4])
    banded, full = band_ref.band_totals(flags, keys, start, cfg)
    assert np.array_equal(full, staged_totals(canon, cfg)[0])
    assert (banded <= full).all()
    ok, _ = band_ref.premise(pos, keys, cfg)
    print("%s: %d pairs within the filter radius across a y / z face, all banded; premise holds for %d of %d; candidates per "
          "workgroup %d -> %d (mean)" % (name, tested, int(ok.sum()), ok.size, full.mean(), banded.mean()))
    return flags, ok, tested


@pytest.mark.parametrize("name", ["tiny", "tiny_long", "dense", "sparse", "tight"])
def test_neighbours_across_faces_are_banded(name):
    cfg = FN_SCENE[name]()["cfg"]
    assert band_ref.grid_allows_bands(cfg)
    for canon in oracle_states(name)[::2]:  # steps 1 and 3
        flags, ok, tested = _check(name, cfg, canon)
        assert ok.all() and tested > 0
        assert (flags != 0xff).any()


def test_column_at_085_r0():
    sc = scenes.SCENES["tiny_compressed"]()
    flags, ok, tested = _check("compressed", sc["cfg"], _oracle_state(sc, 2))
    assert ok.all() and tested > 0


def test_aliased_ids_put_every_particle_into_every_band():
    """The worm and alias16 declare 163 401 cells under 16-bit ids: keys are not cell ids, the premise fails everywhere, the flags are
    all ones (a superset trivially) and the step's automatic mode runs without bands."""
    for name, sc in (("worm", scenes.worm_scene()), ("alias16", scenes.SCENES["alias16"]())):
        cfg = sc["cfg"]
        assert not band_ref.grid_allows_bands(cfg)
        flags, ok, _ = _check(name, cfg, _oracle_state(sc))
        assert not ok.any() and (flags == 0xff).all()


def test_grids_the_proof_does_not_cover():
    cfg = scenes.SCENES["tiny"]()["cfg"]
    assert band_ref.grid_allows_bands(cfg)
    for axis in ("gridCellsX", "gridCellsY", "gridCellsZ"):
        c = type(cfg).from_buffer_copy(cfg)
        setattr(c, axis, 2)
        c.gridCellCount = c.gridCellsX * c.gridCellsY * c.gridCellsZ
        assert not band_ref.grid_allows_bands(c), axis
    c = type(cfg).from_buffer_copy(cfg)
    c.gridCellCount += 1  # not the product of the axes
    assert not band_ref.grid_allows_bands(c)


def _hand_made(cfg, pts):
    """pts in any order -> a sorted state (pos, keys, cellStart) hashed like k_hash (wide or harmless mask)."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    inv = F(cfg.hashGridCellSizeInv)
    with np.errstate(invalid="ignore"):
        c = (pts * inv).astype(F).astype(np.int64)  # truncation towards zero, negative coordinates included
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    keys = (c[:, 0] + c[:, 1] * gx + c[:, 2] * gx * gy) & int(cfg.cellIdMask)
    order = np.argsort(keys, kind="stable")
    keys, pts = keys[order], pts[order]
    start = np.searchsorted(keys, np.arange(cfg.gridCellCount + 1), side="left").astype(np.uint32)
    return pts, keys, start


def _ulp_steps(x, n):
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


def test_face_distances_at_the_band_radius():
    """A candidate at distance Rb from a face of its cell, one ulp nearer and one ulp farther, for the lo and the hi face of y and z:
    flagged up to and including Rb as the kernel evaluates the distance, not beyond."""
    cfg = scenes.SCENES["tiny"]()["cfg"]
    rb, cs = band_ref.band_radius(cfg), F(cfg.hashGridCellSize)
    assert rb < cs < 2 * rb  # cells are narrower than 2 Rb: the lo and the hi band of an axis overlap in the middle of a cell
    mid = F(1.5) * cs  # the middle of cell 1 on the other axes: in both bands there
    for axis, lo_bit, hi_bit in ((1, 4, 3), (2, 6, 1)):  # slots: loY 4, hiY 3; loZ 6, hiZ 1
        for cell in (1, 2):
            lo_face, hi_face = (F(cell) * cs).astype(F), (F(cell + 1) * cs).astype(F)
            for side, face, bit in (("lo", lo_face, lo_bit), ("hi", hi_face, hi_bit)):
                at = (face + rb).astype(F) if side == "lo" else (face - rb).astype(F)
                for step in range(-3, 4):
                    q = _ulp_steps(at, step)
                    p = np.array([mid, mid, mid], F)
                    p[axis] = q
                    pos, keys, _ = _hand_made(cfg, [p])
                    f = int(band_ref.band_flags(pos, keys, cfg)[0])
                    dist = (q - face).astype(F) if side == "lo" else (face - q).astype(F)  # as band_flags evaluates it
                    assert ((f >> bit) & 1) == int(dist <= rb), (axis, cell, side, step, float(q), float(dist), float(rb))
    # and the premise of the whole construction: Rb is the filter radius plus a margin that is positive and small
    rf = np.sqrt(np.float64(band_ref.filter_r2(cfg.h)))
    assert 0.0 < np.float64(rb) - rf < 1e-4 * rf


def test_two_particles_across_a_face_at_the_filter_radius():
    """P just above a y face, Q below it at y distance d: for d up to the filter radius (and a little beyond, by the margin) Q is in the
    hiY band; checked with the pair test on both sides of the radius, one ulp at a time, and the same across a z face and a yz edge."""
    cfg = scenes.SCENES["tiny"]()["cfg"]
    cs = F(cfg.hashGridCellSize)
    rf = F(np.sqrt(np.float64(band_ref.filter_r2(cfg.h))))
    face = (F(2) * cs).astype(F)
    x = F(1.5) * cs
    seen_near = seen_far = 0
    for dp in (F(0), _ulp_steps(face, 1) - face, F(0.25)):  # P on the face exactly, one ulp above, well inside
        for step in range(-4, 5):
            qy = _ulp_steps((face + dp - rf).astype(F), step)
            for pts in ([[x, face + dp, x], [x, qy, x]],                              # across a y face
                        [[x, x, face + dp], [x, x, qy]],                              # across a z face
                        [[x, face + dp, face], [x, qy, _ulp_steps(face, -1)]]):       # across a yz edge (z distance one ulp)
                pos, keys, start = _hand_made(cfg, pts)
                bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg)
                assert not bad, (float(dp), step, pts, bad)
                seen_near += tested
                seen_far += 2 - tested if tested <= 2 else 0
    assert seen_near > 0 and seen_far > 0  # the sweep crossed the radius


def test_particle_on_a_face_and_on_a_half_cell_plane():
    cfg = scenes.SCENES["tiny"]()["cfg"]
    cs, h = F(cfg.hashGridCellSize), F(cfg.h)
    mid = F(1.5) * cs
    # Exactly on the face coordinate 2 * cellSize between the y cells 1 and 2. Which of the two it hashes to is the truncation's
    # business ((int)(q * cellSizeInv), and cellSizeInv * cellSize is not exactly 1: here it lands in cell 1) — the margin of Rb
    # covers either answer, and both neighbours across that face must find it.
    on_face = [mid, (F(2) * cs).astype(F), mid]
    above, below = [mid, (F(2) * cs + F(0.5)).astype(F), mid], [mid, (F(2) * cs - F(0.5)).astype(F), mid]
    on_half = [mid, mid, ((F(1) * cs).astype(F) + h).astype(F)]  # exactly on the half-cell plane of z in cell 1
    pos, keys, start = _hand_made(cfg, [on_face, above, below, on_half])
    flags = band_ref.band_flags(pos, keys, cfg)
    ok, c = band_ref.premise(pos, keys, cfg)
    assert ok.all()
    i_face = int(np.nonzero(pos[:, 1] == on_face[1])[0][0])
    i_half = int(np.nonzero(pos[:, 2] == on_half[2])[0][0])
    assert c[i_face, 1] in (1, 2)
    near_bit = 3 if c[i_face, 1] == 1 else 4  # in cell 1 it lies on the hi face (hiY), in cell 2 on the lo face (loY)
    assert (flags[i_face] >> near_bit) & 1 and not (flags[i_face] >> (7 - near_bit)) & 1  # ... and a whole cell away from the other
    assert (flags[i_half] >> 6) & 1 and (flags[i_half] >> 1) & 1  # h from the lo face, h from the hi face: both within Rb
    bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg, flags)
    assert not bad and tested >= 2  # the pair across the face sees each other, whichever cell the particle on the face is in


def test_negative_and_non_finite_coordinates_are_in_every_band():
    cfg = scenes.SCENES["wide"]()["cfg"]
    cs = F(cfg.hashGridCellSize)
    pts = [[F(1.5) * cs, F(-0.5), F(1.5) * cs],   # truncates to cell row 0 from below zero: the key aliases a real cell
           [F(-0.25), F(1.5) * cs, F(1.5) * cs],
           [F(1.5) * cs, F(1.5) * cs, F(-1.0e-3)],
           [F(1.5) * cs, F(0.5) * cs, F(1.5) * cs],  # a real particle of the aliased cell
           [F(1.5) * cs, F(1.5) * cs, F(1.5) * cs]]
    pos, keys, start = _hand_made(cfg, pts)
    flags = band_ref.band_flags(pos, keys, cfg)
    ok, _ = band_ref.premise(pos, keys, cfg)
    neg = (pos < 0).any(1)
    assert neg.sum() == 3 and not ok[neg].any() and (flags[neg] == 0xff).all() and ok[~neg].all()
    assert not band_ref.missing_from_bands(pos, keys, start, cfg, flags)[0]
    bad = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, 3.0e38]], F)
    assert (band_ref.band_flags(bad, np.zeros(3, np.int64), cfg) == 0xff).all()


def test_a_particle_in_the_lo_and_the_hi_band_of_an_axis():
    """Cells are 2h wide and Rb > h, so the slab of a cell within Rb of both y faces is not empty: a particle in the middle is staged for
    the y row below and for the one above, and counted once in each of the two bands' tables."""
    cfg = scenes.SCENES["tiny"]()["cfg"]
    cs = F(cfg.hashGridCellSize)
    mid = F(1.5) * cs
    pos, keys, start = _hand_made(cfg, [[mid, mid, F(1.02) * cs], [mid, F(1.01) * cs, F(1.02) * cs]])
    flags = band_ref.band_flags(pos, keys, cfg)
    both = ((flags >> 4) & 1) & ((flags >> 3) & 1)
    assert both.sum() == 1  # the one in the middle of y; the other is more than Rb below the hi face
    bstart = band_ref.band_start(flags, start)
    assert bstart[4, -1] == 2 and bstart[3, -1] == 1
    arrays = band_ref.band_arrays(pos, flags)
    assert arrays[3].shape[0] == 1 and arrays[4].shape[0] == 2
    assert arrays[4][:, 3].view(np.int32).tolist() == [0, 1]  # sorted order kept
