"""numpy restatement of the particle-editing contract (include/sphmi.h, sph_remove_region / sph_remove_selection / sph_remove_ids /
sph_add_particles / sph_emit_lattice / sph_read_edit_map). The state is the pair (position, velocity), float32[N, 4] each, in
original-id order; every function returns new arrays and leaves its inputs alone. Nothing here calls the library."""
import numpy as np

f32 = np.float32


class Refused(ValueError):
    """The contract refuses the edit (SPH_ERR_INVALID / SPH_ERR_SIZE); the state stays as it was."""


def region_marks(pos, region=None, types=(1,)):
    """bool[N]: (int)position.w is one of `types` (1..3) and the float32 position lies in the half-open box x0 <= x < x1, ...
    (float32 compares; +-inf bounds allowed; None = everywhere). A NaN bound is refused."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    types = [int(t) for t in types]
    if not types or any(t < 1 or t > 3 for t in types):
        raise Refused("types must be a non-empty subset of 1..3")
    box = np.array([-np.inf] * 3 + [np.inf] * 3 if region is None else region, f32).reshape(6)
    if np.isnan(box).any():
        raise Refused("a region bound is NaN")
    with np.errstate(invalid="ignore"):
        t = np.where(np.isfinite(pos[:, 3]) & (np.abs(pos[:, 3]) < 64), pos[:, 3], f32(0)).astype(np.int32)  # (int)w, truncating
    ok = np.isin(t, types)
    for ax in range(3):
        ok &= (box[ax] <= pos[:, ax]) & (pos[:, ax] < box[3 + ax])
    return ok


def id_marks(N, ids):
    """bool[N] for a list of original ids; duplicates are allowed, an id >= N is refused."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= N):
        raise Refused("id out of range")
    m = np.zeros(N, bool)
    m[ids] = True
    return m


def elastic_range_check(marked, num_elastic, elastic_offset):
    """With elastic matter no id below elasticOffset + numOfElasticP may be marked: returns None, or the lowest such id."""
    if num_elastic <= 0:
        return None
    bad = np.flatnonzero(np.asarray(marked, bool)[:elastic_offset + num_elastic])
    return int(bad[0]) if bad.size else None


def remove(pos, vel, marked, num_elastic=0, elastic_offset=0):
    """The stable compaction: (position, velocity, newIdOfOld) with newIdOfOld[o] = o - #marked below o, or -1 for a marked
    particle. Removing nothing returns copies and the identity. Refused: a marked id in the elastic range, removing everything."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    vel = np.asarray(vel, f32).reshape(-1, 4)
    marked = np.asarray(marked, bool).reshape(-1)
    assert marked.size == pos.shape[0] == vel.shape[0]
    if marked.any():
        bad = elastic_range_check(marked, num_elastic, elastic_offset)
        if bad is not None:
            raise Refused("particle %d lies below the end of the elastic range" % bad)
        if marked.all():
            raise Refused("every particle is marked")
    keep = ~marked
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return pos[keep].copy(), vel[keep].copy(), new_id


def lattice(origin, spacing, dims, velocity=(0, 0, 0), type_value=1.0):
    """(position, velocity) of sph_emit_lattice: point k = (iz*ny + iy)*nx + ix, x fastest, coordinate origin + (float)i * spacing
    per axis in float32 (one multiply, one add), position.w = type_value, velocity (vx, vy, vz, 0)."""
    o = np.asarray(origin, f32).reshape(3)
    s = np.asarray(spacing, f32).reshape(3)
    nx, ny, nz = (int(d) for d in dims)
    if nx < 0 or ny < 0 or nz < 0:
        raise Refused("negative dims")
    with np.errstate(invalid="ignore", over="ignore"):
        x = o[0] + np.arange(nx, dtype=np.int32).astype(f32) * s[0]
        y = o[1] + np.arange(ny, dtype=np.int32).astype(f32) * s[1]
        z = o[2] + np.arange(nz, dtype=np.int32).astype(f32) * s[2]
    assert x.dtype == y.dtype == z.dtype == np.float32
    pos = np.empty((nz, ny, nx, 4), f32)
    pos[..., 0] = x[None, None, :]
    pos[..., 1] = y[None, :, None]
    pos[..., 2] = z[:, None, None]
    pos[..., 3] = f32(type_value)
    vel = np.zeros((nz * ny * nx, 4), f32)
    vel[:, :3] = np.asarray(velocity, f32).reshape(3)
    return pos.reshape(-1, 4), vel


def validate_added(cfg, add_pos):
    """sph_create's validation of particles to be added, plus the type rule: returns None or (index, reason) of the first offender."""
    add_pos = np.asarray(add_pos, f32).reshape(-1, 4)
    wide = cfg.cellIdMask == 0xffffffff
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin], f32)
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax], f32)
    for k in range(add_pos.shape[0]):
        p = add_pos[k]
        if not np.isfinite(p[:3]).all():
            return k, "not finite"
        if wide and not ((p[:3] >= lo) & (p[:3] <= hi)).all():
            return k, "outside the box"
        if not (np.isfinite(p[3]) and int(p[3]) in (1, 3)):
            return k, "type"
    return None


def append(pos, vel, add_pos, add_vel, cfg=None, capacity=None):
    """(position, velocity) with the new particles at ids N .. N+K-1 in the given order. With cfg: validated as the library does
    (Refused names the first offender); with capacity: N + K must not exceed it."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    vel = np.asarray(vel, f32).reshape(-1, 4)
    add_pos = np.asarray(add_pos, f32).reshape(-1, 4)
    add_vel = np.asarray(add_vel, f32).reshape(-1, 4)
    assert add_pos.shape == add_vel.shape
    if capacity is not None and pos.shape[0] + add_pos.shape[0] > capacity:
        raise Refused("capacity")
    if cfg is not None:
        bad = validate_added(cfg, add_pos)
        if bad is not None:
            raise Refused("particle %d: %s" % bad)
    return np.concatenate([pos, add_pos]), np.concatenate([vel, add_vel])


def liquid_quantile_box(pos, lo=0.3, hi=0.7):
    """The box spanned by the lo..hi quantiles of the liquid's coordinates, as float32 (x0, y0, z0, x1, y1, z1)."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    liq = pos[pos[:, 3].astype(np.int32) == 1, :3].astype(np.float64)
    return np.concatenate([np.quantile(liq, lo, axis=0), np.quantile(liq, hi, axis=0)]).astype(f32)


def clear_origin(pos, cfg, dims, spacing, pad):
    """An origin for a lattice of `dims` points at `spacing` whose bounding box, grown by `pad`, holds no elastic or boundary
    particle and lies inside the scene's box: the liquid particle nearest to the liquid's centroid that qualifies (liquid inside
    that box is the caller's to drain). Returns (origin float32[3], padded box float32[6])."""
    pos = np.asarray(pos, f32).reshape(-1, 4)
    t = pos[:, 3].astype(np.int32)
    liq, other = pos[t == 1, :3], pos[t != 1, :3]
    ext = (np.asarray(dims, np.int32) - 1).astype(f32) * f32(spacing)
    lo_box = np.array([cfg.xmin, cfg.ymin, cfg.zmin], f32)
    hi_box = np.array([cfg.xmax, cfg.ymax, cfg.zmax], f32)
    order = np.argsort(((liq.astype(np.float64) - liq.astype(np.float64).mean(0)) ** 2).sum(1), kind="stable")
    for i in order:
        o = liq[i]
        lo, hi = o - f32(pad), o + ext + f32(pad)
        if (lo < lo_box).any() or (hi > hi_box).any():
            continue
        if ((other >= lo) & (other < hi)).all(1).any():
            continue
        return o.copy(), np.concatenate([lo, hi]).astype(f32)
    raise AssertionError("no clear place for the lattice")


def with_count(cfg, n, capacity=0):
    """A copy of the sph_config for a solver that starts with n particles."""
    c = type(cfg).from_buffer_copy(cfg)
    c.particleCount = int(n)
    c.capacity = int(capacity)
    return c


HAND_MADE = 7  # hand_made_particles returns this many


def hand_made_particles(cfg, origin):
    """Seven particles for add_particles near `origin` (a clear place): six liquid ones with assorted velocities, and one
    boundary particle whose velocity holds a wall normal."""
    r0 = f32(cfg.r0)
    o = np.asarray(origin, f32)
    pos = np.zeros((HAND_MADE, 4), f32)
    vel = np.zeros((HAND_MADE, 4), f32)
    for k in range(HAND_MADE):
        pos[k, :3] = o + np.array([f32(k) * f32(0.97) * r0, f32(k % 2) * f32(1.1) * r0, f32(k % 3) * f32(1.05) * r0], f32)
        pos[k, 3] = f32(1.0)
        vel[k, :3] = np.array([f32(0.01) * f32(k), f32(-0.02), f32(0.005) * f32(k * k)], f32)
    pos[4, 3] = f32(3.0)
    vel[4] = np.array([0.0, 1.0, 0.0, 0.0], f32)  # a boundary particle's velocity is its normal
    return pos, vel
