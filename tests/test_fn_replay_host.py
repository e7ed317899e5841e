"""The replay behind findNeighbors' walk (csrc/sph_neighbors.hip), judged without a GPU in numpy float32 / uint32.

The kernel counts `d^2 < U` (bisection) and `d^2 <= r2` (pass 1) as sign bits of packed subtractions shifted into mask words, and
places accepted entry e of a lane's list at popcount(accepted & bits below e) + (the partner lane's accepted entries in front of
e's piece). This module proves the two counting identities against plain comparisons on the values where they could break, the mask
words' bit order and count against the comparisons for every liveEnd, and the rank formula against a direct merge of the two lanes'
pieces A0 | B1 B2 B3 | A4 A5 | B6 | A7 — on random pieces and on the oracle's own rows. From the oracle's states it then proves
that the scenes of tests/test_fn_replay.py hold what that file is for. The conditions are on the scenes, not tolerances.

The lists restated here hold the candidates of a lane's four cells with d^2 <= binU[63] in the reference's float expression; the
kernel's filter evaluates a fused chain that accepts a superset (< 2^-21 relative), so its lists are these or a borderline entry longer."""
import numpy as np

import band_ref
import scenes
import test_fn_lane_order_host as lane_host
import test_fn_tile_host as tile_host

F = np.float32
U32 = np.uint32
INF = F(np.inf)
INF_BITS = U32(0x7f800000)
CAP, CHUNK, MAXN, RSEG = 48, 8, 32, 30   # FN_LIST_CAP, FN_CHUNK, SPH_MAXN, SPH_RSEG
LANE_OF_CELL = np.array([0, 1, 1, 1, 0, 0, 1, 0])  # lane A: cells 0 4 5 7, lane B: cells 1 2 3 6
PIECE_OF_CELL = np.array([0, 0, 1, 2, 1, 2, 3, 3])  # the cell's place among its lane's four pieces
NAMES = ("dense", "tight", "sparse", "squeezed", "packed", "coincident", "stray", "jitter", "lattice")
SCENE = dict(tile_host.SCENE, lattice=lane_host.lattice_scene)
# the scene test_step_overlap.py uses for rows without a 16-bit copy (test_exact_walks_on_both_sides_of_a_chunk_edge)
NO_COPY_SCENE = dict(box=(8.0, 8.0, 8.0), lattice=(18, 18, 18), spacing_in_r0=0.45, origin_in_r0=(4.0, 4.0, 4.0))


def oracle_states(name):
    return lane_host.oracle_states(name) if name == "lattice" else tile_host.oracle_states(name)


# ---------------------------------------------------------------------------------------------------- the host's tables
def radial_bin(d2, h):
    return int(F(F(np.sqrt(F(d2)) * F(RSEG)) / F(h)))


def bin_thresholds(h):
    """binU[0..62] as sph_create computes them (compute_bin_thresholds, csrc/sph_api.hip)."""
    h = F(h)
    h2 = F(h * h)
    h2next = int(h2.view(U32)) + 1
    top = int(F(F(16.0) * h2).view(U32))
    U = np.zeros(63, F)
    for j in range(RSEG):
        lo, hi = 0, top
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if radial_bin(U32(mid).view(F), h) >= j + 1:
                hi = mid
            else:
                lo = mid + 1
        U[j] = U32(min(lo, h2next)).view(F)
    U[RSEG] = U[RSEG + 1] = U32(h2next).view(F)
    for jb in range(RSEG + 1):
        r = F(F(F(jb + 1) * h) / F(RSEG))
        U[32 + jb] = F(r * r)
    return U


def canonical_d2(x):
    """The expansion's unsigned minimum of the bit pattern against +inf's: NaN of either sign becomes +inf."""
    return np.minimum(np.asarray(x, F).view(U32), INF_BITS).view(F)


def edge_values():
    U = bin_thresholds(scenes.SCENES["tiny"]()["cfg"].h)
    near = np.concatenate([np.nextafter(U, -INF), U, np.nextafter(U, INF)]).astype(F)
    nan = canonical_d2(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001], U32).view(F))
    d = np.concatenate([[F(0), U32(1).view(F), INF], near, nan]).astype(F)
    return d, np.unique(near)


def test_bisection_identity():
    """d < U  <=>  the sign bit of d - U, for zero, the smallest denormal, one ulp either side of every binU[0..62] of `tiny`,
    equal values, +inf and canonicalised NaNs of both signs against every finite threshold."""
    d, U = edge_values()
    assert np.isfinite(U).all() and (U > 0).all() and not np.isnan(d).any() and (d == INF).sum() >= 5
    D, T = np.meshgrid(d, np.concatenate([U, [F(0), U32(1).view(F)]]).astype(F), indexing="ij")
    diff = (D - T).astype(F)
    assert (D == T).sum() >= U.size and not np.signbit(diff[D == T]).any()          # equal values give +0
    assert np.array_equal(np.signbit(diff), D < T)
    assert (diff[(D != T) & np.isfinite(D)] != 0).all()                             # denormals kept: no difference rounds to zero


def test_pass1_identity():
    """d <= r2  <=>  the sign bit of r2 - d is clear, same values."""
    d, U = edge_values()
    D, R = np.meshgrid(d, np.concatenate([U, [F(0), U32(1).view(F)]]).astype(F), indexing="ij")
    assert np.array_equal(~np.signbit((R - D).astype(F)), D <= R)


def alignbit31(hi, lo):
    return ((U32(hi) << U32(1)) | (U32(lo) >> U32(31))) & U32(0xffffffff)


def test_mask_words_for_every_live_end():
    """The words the kernel builds, for every liveEnd and lists of every length: the bisection's two popcounts equal the number of
    `d < U`, and pass 1's inverted words have entry e in bit e — the entries past liveEnd, +inf everywhere, never shifted in."""
    rng = np.random.default_rng(48)
    U = bin_thresholds(scenes.SCENES["tiny"]()["cfg"].h)
    for total in list(range(0, CAP + 1)) * 2:
        d2 = np.full(CAP, INF, F)
        d2[:total] = rng.choice(np.concatenate([U[:30], np.nextafter(U[:30], -INF), rng.random(30).astype(F) * U[29]]), total)
        for live_end in range(max(CHUNK, -(-total // CHUNK) * CHUNK), CAP + 1, CHUNK):
            thr = U[rng.integers(0, 30)]
            w = [U32(0), U32(0)]
            for e in range(live_end):
                w[e >> 5] = alignbit31(w[e >> 5], (d2[e] - thr).astype(F).view(U32))
            assert bin(int(w[0])).count("1") + bin(int(w[1])).count("1") == int((d2 < thr).sum())
            rj = [U32(0xffffffff), U32(0xffffffff)]
            for e in range(live_end - 1, -1, -1):
                rj[e >> 5] = alignbit31(rj[e >> 5], (thr - d2[e]).astype(F).view(U32))
            acc = (int(~rj[1] & U32(0xffffffff)) << 32) | int(~rj[0] & U32(0xffffffff))
            assert acc == sum(1 << e for e in range(CAP) if d2[e] <= thr)


# ---------------------------------------------------------------------------------------------------- the rank formula
def slots_by_formula(seg_end, acc, other):
    """Slots of one lane's accepted entries: popcount(acc & bits below e) + base(e); base changes at segEnd[0] and segEnd[2] only.
    seg_end: ends of the lane's four pieces in its list; other: the partner lane's accepted entries per piece."""
    lane_b = other["lane"] == 0  # (the partner is lane A)
    o = other["mine"]
    front = o[0] + o[1] + o[2]
    base = (o[0], o[0], front) if lane_b else (0, front, front + o[3])
    out = {}
    for e in range(seg_end[3]):
        if (acc >> e) & 1:
            b = base[0] if e < seg_end[0] else (base[1] if e < seg_end[2] else base[2])
            out[e] = bin(acc & ((1 << e) - 1)).count("1") + b
    return out


def test_rank_formula_against_a_direct_merge():
    rng = np.random.default_rng(7)
    above32 = empty_piece = 0
    for trial in range(600):
        lanes = []
        for lane in range(2):
            n = rng.integers(0, CAP + 1, 4) * (rng.random(4) > 0.25)
            while n.sum() > CAP:
                n[rng.integers(0, 4)] //= 2
            seg_end = np.cumsum(n).tolist()
            acc = int(rng.integers(0, 1 << 62)) & int(rng.integers(0, 1 << 62) if trial % 3 else -1) & ((1 << seg_end[3]) - 1)
            below = [(1 << s) - 1 for s in seg_end]
            mine = [bin(acc & below[0]).count("1")] + [bin(acc & below[i] & ~below[i - 1]).count("1") for i in (1, 2, 3)]
            lanes.append(dict(lane=lane, seg_end=seg_end, acc=acc, mine=mine))
            empty_piece += int((n == 0).any())
        A, B = lanes
        merged = []  # (lane, entry) of the accepted entries in the order A0 | B1 B2 B3 | A4 A5 | B6 | A7
        for lane, pieces in ((A, (0,)), (B, (0, 1, 2)), (A, (1, 2)), (B, (3,)), (A, (3,))):
            for i in pieces:
                lo = lane["seg_end"][i - 1] if i else 0
                merged += [(lane["lane"], e) for e in range(lo, lane["seg_end"][i]) if (lane["acc"] >> e) & 1]
        above32 += len(merged) > MAXN
        want = {k: s for s, k in enumerate(merged)}
        got = {(0, e): s for e, s in slots_by_formula(A["seg_end"], A["acc"], B).items()}
        got.update({(1, e): s for e, s in slots_by_formula(B["seg_end"], B["acc"], A).items()})
        assert got == want, (trial, A, B)
    assert above32 > 50 and empty_piece > 100


# ---------------------------------------------------------------------------------------------------- the scenes
_lists = {}


def lane_lists(name, step=0):
    """Per particle of the state the step's search saw: the two lanes' lists (entries within the filter radius, by piece and sorted
    index), the stopping bin's count and the accepted entries, restated from the oracle's sorted positions and keys."""
    if (name, step) in _lists:
        return _lists[name, step]
    sc = SCENE[name]()
    cfg = sc["cfg"]
    canon = oracle_states(name)[step]
    N = cfg.particleCount
    p = np.ascontiguousarray(canon["sortedPosition"][:N, :3], F)
    keys = canon["particleIndex"].reshape(-1, 2)[:N, 0].astype(np.int64)
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    cell = np.stack([keys % gx, (keys // gx) % gy, keys // (gx * gy)], 1)
    inv, size, h = F(cfg.hashGridCellSizeInv), F(cfg.hashGridCellSize), F(cfg.h)
    with np.errstate(invalid="ignore", over="ignore"):
        half = np.stack([np.where((p[:, k] - F(lo)) - (p[:, k] * inv).astype(np.int32).astype(F) * size < h, -1, 1)
                         for k, lo in enumerate((cfg.xmin, cfg.ymin, cfg.zmin))], 1)
        R2 = band_ref.filter_r2(h)
        I, J, D2 = [], [], []
        for a in range(0, N, 256):
            q = p[a:a + 256]
            ex, ey, ez = (q[:, None, k] - p[None, :, k] for k in range(3))
            d2 = (ex * ex + ey * ey) + ez * ez
            i, j = np.nonzero(d2 <= R2)
            keep = i + a != j
            I.append(i[keep] + a); J.append(j[keep]); D2.append(d2[i[keep], j[keep]])
    I, J, D2 = np.concatenate(I), np.concatenate(J), np.concatenate(D2)
    step3 = cell[J] - cell[I]
    member = ((step3 == 0) | (step3 == half[I])).all(1)  # the candidate lies in one of the particle's eight cells
    I, J, D2, step3 = I[member], J[member], D2[member], step3[member]
    moved = step3 != 0
    cellidx = np.array([0, 1, 2, 4, 3, 5, 6, 7])[moved[:, 0] + 2 * moved[:, 1] + 4 * moved[:, 2]]
    lane, piece = LANE_OF_CELL[cellidx], PIECE_OF_CELL[cellidx]
    order = np.lexsort((J, piece, lane, I))
    I, J, D2, lane, piece, cellidx = I[order], J[order], D2[order], lane[order], piece[order], cellidx[order]
    group = I * 2 + lane
    length = np.bincount(group, minlength=2 * N).reshape(N, 2)
    first = np.concatenate([[0], np.cumsum(length.reshape(-1))[:-1]])
    pos = np.arange(I.size) - first[group]  # place of the entry in its lane's list
    # pass 0: radial histogram of the candidates within h, the reference's stopping rule
    h2 = F(h * h)
    inh = D2 <= h2
    rbin = (np.sqrt(D2[inh]) * F(RSEG)).astype(F) / h
    rbin = rbin.astype(F).astype(np.int64)
    ok = rbin < RSEG
    hist = np.bincount(I[inh][ok] * RSEG + rbin[ok], minlength=N * RSEG).reshape(N, RSEG)
    cum = np.cumsum(hist, 1)
    reached = cum[:, -1] >= MAXN
    jstar = np.where(reached, (cum >= MAXN).argmax(1), RSEG)
    at = np.where(reached, cum[np.arange(N), np.minimum(jstar, RSEG - 1)], 0)
    jb = np.where(reached, np.where(at == MAXN, jstar, jstar - 1), RSEG)
    r = ((jb + 1).astype(F) * h).astype(F) / F(RSEG)
    r2 = (r.astype(F) * r.astype(F)).astype(F)
    accepted = D2 <= r2[I]
    out = dict(N=N, I=I, J=J, D2=D2, lane=lane, piece=piece, pos=pos, length=length, reached=reached, at=at, accepted=accepted,
               canon=canon, cfg=cfg)
    _lists[name, step] = out
    return out


def test_restated_lists_and_rank_formula_give_the_oracles_rows():
    """On the particles whose two lists fit (the lane pair serves them): the accepted entries, placed by the rank formula, are the
    oracle's neighbour ids slot by slot — the restatement above is the reference's search, and the formula its slot order."""
    for name in ("jitter", "lattice", "squeezed"):
        L = lane_lists(name)
        N = L["N"]
        ids = L["canon"]["neighborIds"].reshape(-1, 32)[:N]
        fits = (L["length"] <= CAP).all(1)
        a = L["accepted"]
        I, J, lane, piece = L["I"][a], L["J"][a], L["lane"][a], L["piece"][a]
        mine = np.zeros((N, 2, 4), np.int64)
        np.add.at(mine, (I, lane, piece), 1)
        order = np.lexsort((J, piece, lane, I))
        I, J, lane, piece = I[order], J[order], lane[order], piece[order]
        group = I * 2 + lane
        count = np.bincount(group, minlength=2 * N)
        rank = np.arange(I.size) - np.concatenate([[0], np.cumsum(count)[:-1]])[group]  # popcount(acc & bits below e)
        o = mine[I, 1 - lane]
        front = o[:, 0] + o[:, 1] + o[:, 2]
        base_a = np.where(piece == 0, 0, np.where(piece <= 2, front, front + o[:, 3]))
        base_b = np.where(piece <= 2, o[:, 0], front)
        slot = rank + np.where(lane == 0, base_a, base_b)
        got = np.full((N, 32), -1, np.int64)
        keep = slot < MAXN
        got[I[keep], slot[keep]] = J[keep]
        assert fits.sum() > 1000, name
        assert np.array_equal(got[fits], ids[fits]), name


def test_scenes_hold_every_class_of_list_and_stop():
    """Over the scenes of test_fn_replay.py: per lane, lists of 1-8, 9-16, ..., 41-48 entries and longer ones; rows that reach exactly
    32 at the stopping bin, that overshoot it, that never reach 32; accepted entries at list positions 32 and above (in lists that
    fit); coincident pairs in both halves of a tile."""
    classes = np.zeros((2, 7), np.int64)
    stops = np.zeros(3, np.int64)
    late = 0
    for name in NAMES:
        if name == "coincident":
            continue
        L = lane_lists(name)
        length = L["length"]
        c = np.stack([np.bincount(np.minimum((length[:, k] + 7) // 8, 7)[length[:, k] > 0] - 1, minlength=7) for k in range(2)])
        s = np.array([(L["reached"] & (L["at"] == MAXN)).sum(), (L["reached"] & (L["at"] > MAXN)).sum(), (~L["reached"]).sum()])
        fits = (length <= CAP).all(1)
        n_late = int((L["accepted"] & (L["pos"] >= 32) & fits[L["I"]]).sum())
        print("%s: N %d, lists by length class (lane A, lane B) %s, rows stopping at exactly 32 / overshooting / never reaching 32: %s, "
              "accepted entries at list positions >= 32: %d" % (name, L["N"], c.tolist(), s.tolist(), n_late))
        classes += c
        stops += s
        late += n_late
    assert (classes >= 1).all(), classes.tolist()
    assert (stops >= 1).all(), stops.tolist()
    assert late >= 1
    d = oracle_states("coincident")[0]["neighborDist"].reshape(-1, 32)
    zero = np.flatnonzero((d == 0.0).any(1)) % tile_host.TILE
    assert (zero >= tile_host.HALF).any() and (zero < tile_host.HALF).any()
