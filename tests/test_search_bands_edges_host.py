"""The edge scenes of the search bands (band_cases.py) without a GPU: each scene holds the cases it claims, decided
with the oracle and the numpy restatement alone — so that the comparison on the device (test_search_bands_edges.py) proves what it
is meant to prove. The face scene: for every y / z face and every yz edge a pair the oracle accepts across it and one it rejects
within 8 ulps beyond; the pair statement holds with Rb and fails for EVERY one of the eight kinds with a band radius of Rf less 64
ulps; lone candidates whose flag changes between the face distances Rb and Rb + 1 ulp. The stray scene: the premise fails for
exactly the moved particles, and each has neighbours. The counted boxes: the block geometry of the band scan. The cut grids: what
sph_bands_apply decides, and keys that are cell ids."""
import numpy as np
import pytest

import band_cases
import band_ref

F = np.float32


def _row_step(cfg, keys, sp, sq):
    """(sx, sy, sz) with keys[sq] - keys[sp] = sx + gx sy + gx gy sz, each in -1 .. 1, or None."""
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    d = int(keys[sq]) - int(keys[sp])
    for sz in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sx in (-1, 0, 1):
                if d == sx + gx * sy + gx * gy * sz:
                    return sx, sy, sz
    return None


def _accepted_across_faces(cfg, canon):
    """Per kind: the neighbour entries of the oracle whose Q lies in that non-own row of P, by the key difference."""
    N = cfg.particleCount
    keys = canon["particleIndex"].reshape(-1, 2)[:, 0].astype(np.int64)
    rows = canon["neighborIds"].reshape(N, 32)
    P, k = np.nonzero(rows >= 0)
    d = keys[rows[P, k]] - keys[P]
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    return {band_cases.KIND[s]: int(sum((d == sx + gx * sy + gx * gy * sz).sum() for sx in (-1, 0, 1)))
            for s, (sy, sz) in enumerate(band_ref.SLOT_STEP)}


def test_face_scene_holds_its_cases():
    sc = band_cases.face_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert band_ref.grid_allows_bands(cfg)
    canon = band_cases.oracle_states("face", 1)[0]
    pos, keys, start = band_cases.sorted_state(canon)
    back = canon["particleIndexBack"].astype(np.int64)  # original id -> sorted id
    rows = canon["neighborIds"].reshape(N, 32)
    assert (rows[:, 31] < 0).all(), "a neighbour row is full: the clusters are not separate"
    ok, _ = band_ref.premise(pos, keys, cfg)
    assert ok.all()

    # the pairs: accepted up to the last accepted separation, rejected from one ulp beyond it; Q in the kind's row of P
    accepted = {s: 0 for s in band_cases.KIND}
    rejected = {s: 0 for s in band_cases.KIND}
    for slot, long_axis, off, p, q in sc["pairs"]:
        sp, sq = int(back[p]), int(back[q])
        assert _row_step(cfg, keys, sp, sq) == (0,) + band_ref.SLOT_STEP[slot], (band_cases.KIND[slot], off)
        inside = sq in rows[sp]
        assert inside == (off <= 0), (band_cases.KIND[slot], long_axis, off)
        if inside:
            accepted[slot] += 1
        elif off <= 8:
            rejected[slot] += 1
    for off, p, q in sc["control"]:
        sp, sq = int(back[p]), int(back[q])
        assert _row_step(cfg, keys, sp, sq) == (-1, 0, 0)  # the own row
        assert (sq in rows[sp]) == (off <= 0)
    assert all(accepted[s] >= 1 and rejected[s] >= 1 for s in band_cases.KIND), (accepted, rejected)

    # the statement the kernel relies on: holds with Rb, fails for every kind with a radius of Rf less 64 ulps
    flags = band_ref.band_flags(pos, keys, cfg)
    bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg, flags)
    assert not bad, bad[:4]
    rf = F(np.sqrt(np.float64(band_ref.filter_r2(cfg.h))))
    low = band_cases.ulp_steps(rf, -64)
    bad_low, _ = band_ref.missing_from_bands(pos, keys, start, cfg, band_ref.band_flags(pos, keys, cfg, rb=low))
    broken = sorted({s for _, _, s in bad_low})
    print("face scene: N %d (%d hand-placed), %d pairs within the filter radius across a y / z face, all banded with Rb %.9g"
          % (N, sc["numOfLiquidP"], tested, band_ref.band_radius(cfg)))
    for s in sorted(band_cases.KIND):
        print("  %-10s (slot %d): %d accepted, %d rejected within 8 ulps beyond; at Rf - 64 ulps (%.9g): %d missing"
              % (band_cases.KIND[s], s, accepted[s], rejected[s], low, sum(1 for b in bad_low if b[2] == s)))
    print("  kinds that break at Rf - 64 ulps:", [band_cases.KIND[s] for s in broken])
    assert broken == sorted(band_cases.KIND)
    # ... by the pairs placed for it: every Q at the last accepted separation is one of the missing (8 ulps of a coordinate near 30
    # are 64 ulps of Rf, so the nearer ones need not be)
    missing = {(p, q) for p, q, _ in bad_low}
    for slot, long_axis, off, p, q in sc["pairs"]:
        if off == 0:
            assert (int(back[p]), int(back[q])) in missing, (band_cases.KIND[slot], long_axis, off)

    # the lone candidates: the flag changes between the face distances Rb and Rb + 1 ulp, as band_flags evaluates them
    rb, cs = band_ref.band_radius(cfg), F(cfg.hashGridCellSize)
    seen = {"exact": 0, "both": 0, "on a face": 0, "half": 0, ("contracted", 1): 0, ("contracted", 2): 0}
    for i, axis, side, what, bit, member, dist in sc["lone"]:
        s = int(back[i])
        f = int(flags[s])
        c = band_cases.cell_of(cfg, pos[s, axis])
        lo_d, hi_d = F(pos[s, axis] - F(F(c) * cs)), F(F(F(c + 1) * cs) - pos[s, axis])
        d = lo_d if side == "lo" else hi_d
        if dist is not None:
            assert d == dist and abs(int(d.view(np.int32)) - int(rb.view(np.int32))) <= 1, (axis, side, what, d, dist)
            seen["exact"] += 1
        if what == "on a face":  # which cell it truncates to is the truncation's business: it is in the band of that face
            assert pos[s, axis] == F(F(2) * cs) and c in (1, 2)
            near = {1: {1: 3, 2: 4}, 2: {1: 1, 2: 6}}[axis][c]
            assert (f >> near) & 1
            seen["on a face"] += 1
        else:
            assert ((f >> bit) & 1) == int(member) == int(d <= rb), (axis, side, what, float(d), float(rb))
            # the same distance from a contracted multiply-subtract (the product exact, one rounding): it must not be what decides
            fused = F(np.float64(pos[s, axis]) - np.float64(c) * np.float64(cs)) if side == "lo" else \
                F(np.float64(c + 1) * np.float64(cs) - np.float64(pos[s, axis]))
            seen["contracted", axis] += int(bool(fused <= rb) != member)
        if (f >> (4 if axis == 1 else 6)) & 1 and (f >> (3 if axis == 1 else 1)) & 1:
            seen["both"] += 1  # within Rb of the lo and of the hi face of the axis
        t = pos[s, 3 - axis]
        seen["half"] += int(any(t == F(F(F(k) * cs) + F(cfg.h)) for k in range(4)))
        seen["on a face"] += int(any(t == F(F(k) * cs) for k in range(1, 4)))
    print("  lone candidates: %d, of them at Rb -1 / 0 / +1 ulp exactly %d, in the lo and the hi band of an axis %d, on a face %d, on "
          "a half-cell plane %d" % (len(sc["lone"]), seen["exact"], seen["both"], seen["on a face"], seen["half"]))
    print("  lone candidates whose flag a contracted multiply-subtract in the face distance would change: %d (y), %d (z)"
          % (seen["contracted", 1], seen["contracted", 2]))
    assert seen["exact"] == 12 and seen["both"] >= 2 and seen["on a face"] >= 2 and seen["half"] >= 2
    assert seen["contracted", 1] >= 1 and seen["contracted", 2] >= 1


def test_stray_scene_holds_its_cases():
    sc = band_cases.stray_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert band_ref.grid_allows_bands(cfg) and int(cfg.cellIdMask) == 0xffff
    canon = band_cases.oracle_states("stray", 2)[0]
    pos, keys, start = band_cases.sorted_state(canon)
    assert keys.max() < cfg.gridCellCount
    ok, _ = band_ref.premise(pos, keys, cfg)
    orig = canon["particleIndex"].reshape(-1, 2)[:, 1].astype(np.int64)  # sorted id -> original id
    assert sorted(orig[~ok].tolist()) == sc["moved"].tolist()
    rows = canon["neighborIds"].reshape(N, 32)
    assert ((rows[~ok] >= 0).sum(1) >= 1).all(), "a moved particle has no neighbour"
    flags = band_ref.band_flags(pos, keys, cfg)
    assert (flags[~ok] == 0xff).all() and (flags[ok] != 0xff).any()
    bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg, flags)
    assert not bad
    p = pos[~ok]
    gx, gy = cfg.gridCellsX * F(cfg.hashGridCellSize), cfg.gridCellsY * F(cfg.hashGridCellSize)
    print("stray scene: N %d, premise fails for %d: %d below zero in x, %d in y, %d in z, %d beyond the grid in x, %d in y; they have "
          "%d .. %d neighbours" % (N, int((~ok).sum()), int((p[:, 0] < 0).sum()), int((p[:, 1] < 0).sum()), int((p[:, 2] < 0).sum()),
                                   int((p[:, 0] >= gx).sum()), int((p[:, 1] >= gy).sum()), int((rows[~ok] >= 0).sum(1).min()),
                                   int((rows[~ok] >= 0).sum(1).max())))
    print("  neighbour entries across a face or edge, per kind:", _accepted_across_faces(cfg, canon))
    assert min((p[:, k] < 0).sum() for k in range(3)) >= 4 and (p[:, 0] >= gx).sum() >= 4 and (p[:, 1] >= gy).sum() >= 4
    assert ((p < 0).sum(1) == 3).any() and ((p < 0).sum(1) == 2).any()
    # after the step every particle is back in the box (integrate clamps): the second step sees no failure of the premise
    pos2, keys2, _ = band_cases.sorted_state(band_cases.oracle_states("stray", 2)[1])
    assert band_ref.premise(pos2, keys2, cfg)[0].all()


def test_counted_boxes_hold_the_block_cases():
    """Waves per count against the scan's blocks of 1024 waves: a total written by a block that owns no wave (one and two full
    blocks), a last wave with one live lane, a partial third block."""
    geo = {}
    for n in band_cases.COUNTS:
        waves = (n + 63) // 64
        blocks = (waves + 1 + band_cases.BAND_SUPER - 1) // band_cases.BAND_SUPER
        geo[n] = (waves, blocks, n - 64 * (waves - 1))
    print("counted boxes: N -> (waves, scan blocks, live lanes of the last wave):", geo)
    assert geo[65536] == (1024, 2, 64) and geo[131072] == (2048, 3, 64)     # the last block holds the total's entry alone
    assert geo[65537] == (1025, 2, 1) and geo[131073] == (2049, 3, 1)
    assert geo[133001][1] == 3 and geo[133001][0] % band_cases.BAND_SUPER not in (0, 1) and 1 < geo[133001][2] < 64
    sc = band_cases.counted_box(65537)
    cfg = sc["cfg"]
    assert cfg.particleCount == 65537 == sc["position"].shape[0] and band_ref.grid_allows_bands(cfg)
    assert (sc["position"][sc["numOfLiquidP"]:, 3] == F(3.0)).all() and (sc["position"][:sc["numOfLiquidP"], 3] != F(3.0)).all()
    assert band_cases.counted_box(131073, 131073 + 4096)["cfg"].capacity == 131073 + 4096


@pytest.mark.parametrize("name", band_cases.GRID_NAMES)
def test_cut_grids(name):
    sc = band_cases.grid_scene(name)
    cfg = sc["cfg"]
    cells = (cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellsZ)
    assert min(cells) == int(name[0]) and cfg.gridCellCount == cells[0] * cells[1] * cells[2]
    assert band_ref.grid_allows_bands(cfg) == (name[0] == "3")
    canon = band_cases.oracle_states(name)[0]
    pos, keys, start = band_cases.sorted_state(canon)
    assert keys.max() < cfg.gridCellCount
    ok, c = band_ref.premise(pos, keys, cfg)
    assert ok.all()  # every key is the id of the in-grid cell of its particle
    liquid = canon["position"][canon["particleIndex"].reshape(-1, 2)[:, 1].astype(np.int64), 3] != F(3.0)
    for axis in range(3):
        if cells[axis] <= 3:  # liquid in every layer of a cut axis
            assert sorted(set(c[liquid, axis].tolist())) == list(range(cells[axis])), (name, axis)
    if name[0] == "3":
        bad, tested = band_ref.missing_from_bands(pos, keys, start, cfg)
        assert not bad and tested > 0
        assert min(_accepted_across_faces(cfg, canon).values()) > 0  # neighbours across every face and edge
    print("%s: %d x %d x %d cells, N %d, bands %s; neighbour entries across a face or edge, per kind: %s"
          % ((name,) + cells + (cfg.particleCount, "allowed" if name[0] == "3" else "off", _accepted_across_faces(cfg, canon))))
