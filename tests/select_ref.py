"""numpy restatement of the particle-selection contract (include/sphmi.h, sph_particle_measure / sph_select_particles /
sph_read_selection), independent of the library's answer.

Works from the contract alone: the surface measure is accumulated slot by slot (0 .. 31, in order) with one rounded float32
operation per written operation, vectorised across particles; the selection is diag_ref's type / key / box rule, a conjunction
of half-open float32 range terms on diag_ref's histogram quantities (field 7: the measure) and an optional component
membership; the list is the selected sorted indices in ascending order; a record is the exported state at those indices.
The state comes from diag_ref.state_with_ids / components_ref.oracle_state, the rows from components_ref.neighbor_rows."""
import numpy as np

import diag_ref

f32 = np.float32
WORDS = 12
MAX_TERMS = 4
FIELDS = diag_ref.FIELDS + ("surface",)
SURFACE = 7


def constants(h, sim_scale):
    """(h, hs2, ss2) as float32, by the sampling contract: ss2 = simScale*simScale, hs2 = (h*simScale)^2."""
    h, ss = f32(h), f32(sim_scale)
    hs = h * ss
    return h, hs * hs, ss * ss


def measure(pos, rows, h, sim_scale):
    """float32[N]: the surface measure of every particle. pos float32[N, >=3] sorted positions, rows int32[N, 32]."""
    p = np.ascontiguousarray(np.asarray(pos, np.float32)[:, :3])
    rows = np.asarray(rows)
    N = p.shape[0]
    h, hs2, ss2 = constants(h, sim_scale)
    me = np.arange(N)
    W = np.zeros(N, np.float32)
    B = [np.zeros(N, np.float32) for _ in range(3)]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k in range(rows.shape[1]):
            j = rows[:, k].astype(np.int64)
            ok = (j >= 0) & (j != me)
            q = p[np.where(ok, j, 0)]
            dx, dy, dz = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
            r2 = (dx * dx + dy * dy) + dz * dz
            t = hs2 - r2 * ss2
            ok &= t > 0
            w = (t * t) * t
            W = np.where(ok, W + w, W)
            for c, d in enumerate((dx, dy, dz)):
                B[c] = np.where(ok, B[c] + w * d, B[c])
        m = np.ones(N, np.float32)
        nz = W != 0
        cx, cy, cz = B[0][nz] / W[nz], B[1][nz] / W[nz], B[2][nz] / W[nz]
        m[nz] = np.sqrt((cx * cx + cy * cy) + cz * cz) / h
    return m.astype(np.float32)


def measure_scalar(pos, row, i, h, sim_scale):
    """The same for one particle with a plain loop over its slots (the check of the vectorised form)."""
    p = np.asarray(pos, np.float32)
    h, hs2, ss2 = constants(h, sim_scale)
    W = Bx = By = Bz = f32(0)
    for j in row:
        j = int(j)
        if j < 0 or j == i:
            continue
        dx, dy, dz = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1], p[j, 2] - p[i, 2]
        r2 = f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz)
        t = f32(hs2 - f32(r2 * ss2))
        if not t > 0:
            continue
        w = f32(f32(t * t) * t)
        W = f32(W + w)
        Bx, By, Bz = f32(Bx + f32(w * dx)), f32(By + f32(w * dy)), f32(Bz + f32(w * dz))
    if W == 0:
        return f32(1.0)
    cx, cy, cz = f32(Bx / W), f32(By / W), f32(Bz / W)
    return f32(np.sqrt(f32(f32(f32(cx * cx) + f32(cy * cy)) + f32(cz * cz))) / h)


def neighbor_counts(rows):
    """float32[N]: the entries >= 0 of every row (sph_histogram's field 3)."""
    return (np.asarray(rows) >= 0).sum(1).astype(np.float32)


class Quantities:
    """The eight per-particle quantities a term can test. rows=None: a state without rows, for selections that use neither the
    neighbour count nor the measure (their record words are then 0)."""

    def __init__(self, state, rows, h=None, sim_scale=None):
        self.state = state
        self.count = self.m = None
        if rows is not None:
            h = state["h"] if h is None else h
            sim_scale = state["simScale"] if sim_scale is None else sim_scale
            self.count = neighbor_counts(rows)
            self.m = measure(state["pos"], rows, h, sim_scale)

    def field(self, field):
        if isinstance(field, str):
            field = FIELDS.index(field)
        if field in (3, SURFACE) and self.count is None:
            raise ValueError("field %d needs the neighbour rows" % field)
        return self.m if field == SURFACE else diag_ref.field_values(self.state, field, self.count)


def select(state, quantities, region=None, types=(1, 2), terms=(), component=None, labels=None):
    """int32[n]: the selected sorted indices in ascending order."""
    if len(terms) > MAX_TERMS:
        raise ValueError("at most %d terms" % MAX_TERMS)
    sel = diag_ref.selected(state, diag_ref.EVERYTHING if region is None else region, types)
    with np.errstate(invalid="ignore"):
        for field, lo, hi in terms:
            lo, hi = f32(lo), f32(hi)
            if np.isnan(lo) or np.isnan(hi) or not lo < hi:
                raise ValueError("a term needs lo < hi")
            q = quantities.field(field)
            sel &= (q >= lo) & (q < hi)  # (NaN compares false: a NaN q fails the term)
    if component is not None and component >= 0:
        sel &= np.asarray(labels) == int(component)
    return np.flatnonzero(sel).astype(np.int32)


def records(state, quantities, index):
    """(orig_id uint32[n], records float32[n, 12]) of the selected sorted indices."""
    idx = np.asarray(index, np.int64)
    rec = np.zeros((idx.size, WORDS), np.float32)
    rec[:, 0:3] = np.asarray(state["pos"], np.float32)[idx, :3]
    rec[:, 3] = np.asarray(state["types"], np.float32)[idx]
    rec[:, 4:7] = np.asarray(state["vel"], np.float32)[idx, :3]
    rec[:, 7] = np.asarray(state["rho"], np.float32)[idx]
    rec[:, 8] = np.asarray(state["p"], np.float32)[idx]
    if quantities.count is not None:
        rec[:, 9] = quantities.count[idx]
        rec[:, 10] = quantities.m[idx]
    return np.asarray(state["ids"])[idx].astype(np.uint32), rec

