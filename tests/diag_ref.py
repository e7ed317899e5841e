"""numpy restatement of the diagnostics contract (include/sphmi.h, sph_diagnostics / sph_histogram).

Works from the contract alone: per-particle terms in float32 in the written order, widened to float64 and added in the fixed
tree (chunks of 1024, strides 512 ... 1, level by level), extremes by float compares canonicalised with + 0.0f, histogram bins
by the float32 rule. The state comes from sample_ref.solver_state(hip), the neighbour counts from hip.neighbor_rows."""
import numpy as np

f32 = np.float32
WORDS = 32
CHUNK = 1024
EVERYTHING = (-np.inf, -np.inf, -np.inf, np.inf, np.inf, np.inf)
FIELDS = ("density", "speed", "pressure", "neighbors", "x", "y", "z")


def tree_sum(terms):
    """The contract's reduce(): pad with +0.0 to whole chunks of 1024 (at least one); in each chunk a[i] += a[i + stride] for
    stride = 512 ... 1; repeat on the chunks' results until one chunk is left."""
    a = np.asarray(terms, np.float64).reshape(-1)
    while True:
        chunks = max(1, -(-a.size // CHUNK))
        b = np.zeros(chunks * CHUNK, np.float64)
        b[:a.size] = a
        b = b.reshape(chunks, CHUNK)
        s = CHUNK // 2
        while s >= 1:
            b = b[:, :s] + b[:, s:2 * s]
            s //= 2
        a = b[:, 0]
        if chunks == 1:
            return a[0]


def type_mask(types):
    m = 0
    for t in types:
        m |= 1 << int(t)
    return m


def selected(state, region, types):
    """bool[N]: the contract's selection rule for one region (x0, y0, z0, x1, y1, z1)."""
    pos = np.asarray(state["pos"], np.float32)
    t = np.asarray(state["types"], np.float32).astype(np.int32)
    mask = type_mask(types)
    ok = (t >= 1) & (t <= 3) & (((1 << np.clip(t, 0, 31)) & mask) != 0)
    ok &= np.asarray(state["keys"]).astype(np.int64) < int(state["G"])
    b = np.asarray(region, np.float32).reshape(6)
    for k in range(3):
        ok &= (b[k] <= pos[:, k]) & (pos[:, k] < b[3 + k])
    return ok


def terms(state, rho0):
    """float32[13, N]: x y z, vx vy vz, Lx Ly Lz, v2, rho, e2, p (record words 1..13), every operation a rounded float32 one."""
    pos = np.asarray(state["pos"], np.float32)
    vel = np.asarray(state["vel"], np.float32)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    vx, vy, vz = vel[:, 0], vel[:, 1], vel[:, 2]
    rho = np.asarray(state["rho"], np.float32)
    p = np.asarray(state["p"], np.float32)
    v2 = (vx * vx + vy * vy) + vz * vz
    e = rho - f32(rho0)
    return np.stack([x, y, z, vx, vy, vz, y * vz - z * vy, z * vx - x * vz, x * vy - y * vx, v2, rho, e * e, p]).astype(np.float32)


def _canon(x):
    return np.float64(f32(x) + f32(0.0))


def record(state, region, types, rho0, ids=None, t=None):
    """float64[32]: the record of one region. `ids`: original ids in sorted order (word 22); default state["ids"]."""
    sel = selected(state, region, types)
    if t is None:
        t = terms(state, rho0)
    out = np.zeros(WORDS, np.float64)
    out[0] = tree_sum(sel.astype(np.float64))
    for w in range(13):
        out[1 + w] = tree_sum(np.where(sel, t[w].astype(np.float64), 0.0))
    out[21] = out[22] = -1.0
    if sel.any():
        rho, p, v2 = t[10][sel], t[12][sel], t[9][sel]
        out[16], out[17] = _canon(rho.min()), _canon(rho.max())
        out[18], out[19] = _canon(p.min()), _canon(p.max())
        out[20] = _canon(v2.max())
        idx = int(np.flatnonzero(sel)[int(np.argmax(v2))])  # argmax: the first (lowest index) of equal maxima
        out[21] = float(idx)
        ids = state.get("ids") if ids is None else ids
        out[22] = float(ids[idx]) if ids is not None else -1.0
        for k in range(3):
            out[23 + k] = _canon(t[k][sel].min())
            out[26 + k] = _canon(t[k][sel].max())
    return out


def records(state, regions, types, rho0, ids=None):
    t = terms(state, rho0)
    return np.stack([record(state, r, types, rho0, ids, t) for r in np.asarray(regions, np.float32).reshape(-1, 6)])


def neighbor_counts(hip, piece=1 << 18):
    """float32[N]: valid entries (ids >= 0) of every sorted particle's neighbour row."""
    out = np.empty(hip.N, np.float32)
    for first in range(0, hip.N, piece):
        n = min(piece, hip.N - first)
        ids, _ = hip.neighbor_rows(first, n)
        out[first:first + n] = (ids >= 0).sum(1)
    return out


def field_values(state, field, nbr_counts=None):
    """float32[N] of histogram field `field` (name or number)."""
    if isinstance(field, str):
        field = FIELDS.index(field)
    pos = np.asarray(state["pos"], np.float32)
    if field == 0:
        return np.asarray(state["rho"], np.float32)
    if field == 1:
        v = np.asarray(state["vel"], np.float32)
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float32)
    if field == 2:
        return np.asarray(state["p"], np.float32)
    if field == 3:
        return np.asarray(nbr_counts, np.float32)
    return pos[:, field - 4]


def histogram_of(values, lo, hi, bins):
    """uint32[bins + 2] of float32 `values` by the contract's rule."""
    q = np.asarray(values, np.float32)
    lo, hi = f32(lo), f32(hi)
    scale = f32(bins) / (hi - lo)
    out = np.zeros(bins + 2, np.uint32)
    below, above = q < lo, q >= hi
    out[0] = below.sum()
    out[bins + 1] = above.sum()
    mid = q[~below & ~above]
    b = np.minimum(((mid - lo) * scale).astype(np.float32).astype(np.int64), bins - 1)
    out[1:bins + 1] = np.bincount(b, minlength=bins)[:bins]
    return out


def histogram(state, field, lo, hi, bins, region=None, types=(1, 2), nbr_counts=None):
    sel = selected(state, EVERYTHING if region is None else region, types)
    return histogram_of(field_values(state, field, nbr_counts)[sel], lo, hi, bins)


def state_with_ids(hip):
    """sample_ref.solver_state(hip) plus "ids": the original id of every sorted particle."""
    import sample_ref
    st = sample_ref.solver_state(hip)
    st["ids"] = hip.read_particleIndex_buffer()[:, 1].astype(np.int64)
    return st
