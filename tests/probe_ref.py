"""numpy float32 restatement of the probe contract (include/sphmi.h, sph_probes_*), built on sample_ref.sample_reference.

level_of is the crossing rule alone, on an array of field values; level_records applies it to lines over a state (every point of
every line sampled, whether the search would have reached it or not: the record must not depend on how far a kernel searched);
point_records restates the point probe."""
import numpy as np

import sample_ref

f32 = np.float32
FOUND, DRY, SUBMERGED = 0, 1, 2
LINE_DTYPE = np.dtype([("origin", np.float32, 3), ("step", np.float32, 3), ("count", np.int32), ("field", np.int32),
                       ("iso", np.float32), ("typeMask", np.uint32)])


def level_of(f, iso):
    """The crossing rule on the field values f[0 .. count-1] of one line: (status, K, t). SUBMERGED: K = count-1; FOUND: K is the
    largest k with k inside and k+1 outside and t = (iso - f_K)/(f_{K+1} - f_K) in float32; DRY: K = -1. t is None unless
    FOUND. Inside is f >= iso, a float32 compare; NaN is outside."""
    f = np.asarray(f, np.float32)
    iso = f32(iso)
    inside = f >= iso
    n = f.shape[0]
    if inside[n - 1]:
        return SUBMERGED, n - 1, None
    for k in range(n - 2, -1, -1):
        if inside[k] and not inside[k + 1]:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                t = (iso - f[k]) / (f[k + 1] - f[k])
            return FOUND, k, f32(t)
    return DRY, -1, None


def line_points(line):
    """q_k = origin + (float)k * step per component, float32[count, 3]."""
    k = np.arange(int(line["count"]), dtype=np.float32)[:, None]
    return (np.asarray(line["origin"], np.float32)[None, :] + k * np.asarray(line["step"], np.float32)[None, :]).astype(np.float32)


def mask_types(mask):
    return tuple(t for t in range(32) if (int(mask) >> t) & 1)


def line_fields(state, lines):
    """f_k of every line: a list of float32[count]. One sample_reference call per type mask in use."""
    lines = np.asarray(lines, LINE_DTYPE).reshape(-1)
    out = [None] * lines.shape[0]
    for mask in sorted(set(int(m) for m in lines["typeMask"])):
        which = [i for i in range(lines.shape[0]) if int(lines["typeMask"][i]) == mask]
        pts = np.concatenate([line_points(lines[i]) for i in which])
        rec = sample_ref.sample_reference(state, pts, mask_types(mask))
        at = 0
        for i in which:
            n = int(lines["count"][i])
            out[i] = rec[at:at + n, int(lines["field"][i])].copy()
            at += n
    return out


def record_of(line, f):
    """The 8-word record of `line` from its field values f (float32[count])."""
    q = line_points(line)
    iso = f32(line["iso"])
    status, K, t = level_of(f, iso)
    r = np.zeros(8, np.float32)
    if status == SUBMERGED:
        r[:3] = q[K]
        r[3], r[4], r[5], r[6] = f32(K), f32(2), f32(K), f[K]
    elif status == DRY:
        r[:3] = q[0]
        r[4], r[5] = f32(1), f32(-1)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            r[:3] = q[K] + t * (q[K + 1] - q[K])
            r[3] = f32(K) + t
        r[5], r[6], r[7] = f32(K), f[K], f[K + 1]
    return r


def level_records(state, lines, fields=None):
    """float32[L, 8]: the level-probe records of `lines` (LINE_DTYPE) over `state` (sample_ref.solver_state()). fields: the result of
    line_fields, if the caller has it."""
    lines = np.asarray(lines, LINE_DTYPE).reshape(-1)
    fields = line_fields(state, lines) if fields is None else fields
    return np.stack([record_of(lines[i], fields[i]) for i in range(lines.shape[0])]) if lines.shape[0] else np.zeros((0, 8), np.float32)


def point_records(state, points, types=(1, 2, 3)):
    """float32[P, 8]: the point-probe records, the sampling contract's."""
    return sample_ref.sample_reference(state, points, types)
