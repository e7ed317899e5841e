"""numpy restatement of the kinematic-body contract (include/sphmi.h, sph_body_define_ids / sph_body_define_region /
sph_body_set_pose and what a removal does to a body). The state is the pair (position, velocity), float32[N, 4] each, in
original-id order; a body is (ids, reference position, reference normal). Every function returns new arrays and leaves its inputs
alone; all arithmetic is float32, one operation at a time in the header's order. Nothing here calls the library."""
import numpy as np

import edit_ref as er

f32 = np.float32
Refused = er.Refused


def region_members(pos, region=None):
    """Original ids of the boundary particles in the half-open box, ascending: sph_remove_region's marks with types fixed to (3,)."""
    return np.flatnonzero(er.region_marks(pos, region, (3,))).astype(np.uint32)


def id_offenders(pos, ids):
    """(number of offending entries, lowest offending list index or -1): an entry offends when its id is >= N, when that particle
    is not a boundary particle ((int)position.w != 3), or when its id occurs more than once in the list (every occurrence)."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    ids = np.asarray(ids, np.int64).reshape(-1)
    N = pos.shape[0]
    in_range = (ids >= 0) & (ids < N)
    safe = np.where(in_range, ids, 0)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isfinite(pos[:, 3]) & (np.abs(pos[:, 3]) < 64), pos[:, 3], f32(0)).astype(np.int32)
    times = np.bincount(safe[in_range], minlength=N)
    bad = ~in_range | (t[safe] != 3) | (times[safe] > 1)
    hits = np.flatnonzero(bad)
    return int(hits.size), (int(hits[0]) if hits.size else -1)


def define(pos, vel, ids):
    """(ids uint32[M], reference position, reference normal) of a body made of `ids` in that order; Refused as the library refuses."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    vel = np.asarray(vel, f32).reshape(-1, 4)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if ids.size == 0:
        raise Refused("a body has at least one member")
    n, first = id_offenders(pos, ids)
    if n:
        raise Refused("%d offending entries, the lowest is entry %d" % (n, first))
    return ids.astype(np.uint32), pos[ids].copy(), vel[ids].copy()


def _row(m, x, y, z):
    return (m[0] * x + m[1] * y) + m[2] * z  # float32 scalars times float32 arrays: one rounding per operation


def placed(pose, ref_pos, ref_nrm):
    """(position, normal) float32[M, 4] of the members under `pose` (3 x 4, (R | t)): x' = ((R00 p.x + R01 p.y) + R02 p.z) + tx and
    nx' = (R00 n.x + R01 n.y) + R02 n.z, likewise y and z; both .w copied bit for bit."""
    m = np.asarray(pose, f32).reshape(3, 4)
    p = np.asarray(ref_pos, f32).reshape(-1, 4)
    n = np.asarray(ref_nrm, f32).reshape(-1, 4)
    out_p, out_n = p.copy(), n.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out_p[:, r] = _row(m[r], p[:, 0], p[:, 1], p[:, 2]) + m[r, 3]
            out_n[:, r] = _row(m[r], n[:, 0], n[:, 1], n[:, 2])
    assert out_p.dtype == out_n.dtype == np.float32
    return out_p, out_n


def pose_offenders(cfg, new_pos):
    """(number of members whose new position fails sph_add_particles' validation, lowest such member index or -1): not finite,
    or outside the box when cell ids are wide."""
    q = np.asarray(new_pos, f32).reshape(-1, 4)[:, :3]
    bad = ~np.isfinite(q).all(1)
    if cfg.cellIdMask == 0xffffffff:
        lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], f32)
        hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], f32)
        with np.errstate(invalid="ignore"):
            bad |= ~((q >= lo) & (q <= hi)).all(1)
    hits = np.flatnonzero(bad)
    return int(hits.size), (int(hits[0]) if hits.size else -1)


def max_move(cfg, new_pos, cur_pos):
    """float32: sqrtf(max over the members of (dx*dx + dy*dy) + dz*dz) / r0 with d = new - current, all in float32; the maximum is
    taken on the bit patterns of the non-negative floats."""
    a = np.asarray(new_pos, f32).reshape(-1, 4)
    b = np.asarray(cur_pos, f32).reshape(-1, 4)
    dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    top = np.ascontiguousarray(d2).view(np.uint32).max() if d2.size else np.uint32(0)
    return np.sqrt(np.array([top], np.uint32).view(f32)[0]) / f32(cfg.r0)


def set_pose(cfg, pos, vel, body, pose):
    """(position, velocity, max_move) after sph_body_set_pose. Refused (with .offenders and .lowest_member) if the pose holds a
    non-finite word or any member's new position fails; then nothing changes."""
    ids, ref_pos, ref_nrm = body
    m = np.asarray(pose, f32).reshape(3, 4)
    if not np.isfinite(m).all():
        raise Refused("a pose word is not finite")
    pos = np.asarray(pos, f32).reshape(-1, 4)
    vel = np.asarray(vel, f32).reshape(-1, 4)
    new_p, new_n = placed(m, ref_pos, ref_nrm)
    n, first = pose_offenders(cfg, new_p)
    if n:
        e = Refused("%d members fail, the lowest is member %d" % (n, first))
        e.offenders, e.lowest_member = n, first
        raise e
    idx = np.asarray(ids, np.int64)
    move = max_move(cfg, new_p, pos[idx])
    out_p, out_v = pos.copy(), vel.copy()
    out_p[idx] = new_p
    out_v[idx] = new_n
    return out_p, out_v, move


def follow_removal(body, new_id_of_old):
    """The body after a removal with the edit map `new_id_of_old`: every member id through the map, removed members dropped with
    their reference rows, order kept. None when no member is left (the slot is released)."""
    ids, ref_pos, ref_nrm = body
    m = np.asarray(new_id_of_old, np.int64)[np.asarray(ids, np.int64)]
    keep = m >= 0
    if not keep.any():
        return None
    return m[keep].astype(np.uint32), np.asarray(ref_pos, f32)[keep].copy(), np.asarray(ref_nrm, f32)[keep].copy()
