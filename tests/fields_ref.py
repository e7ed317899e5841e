"""numpy restatement of the carried-field contract (include/sphmi.h, sph_field_*): diffusion along the neighbour rows, painting,
what the edits do to a field, and the region records.

Works from the contract alone, slot by slot and vectorised over the particles, like forces_ref.Forces: every operation a rounded
float32 one in the written order, the scale through float64 as the step computes it, the region sums float64 in the fixed tree
of diag_ref.tree_sum. The state is the existing exports (rho, the types and keys of the sorted particles, their original ids,
the rows of sph_read_neighbor_rows). tests/test_fields_host.py ties the sum S to forces_ref.Forces, which is tied to the oracle's
K7 stage."""
import numpy as np

import diag_ref

f32 = np.float32
f64 = np.float64
SLOTS = 32
DIAG_WORDS = 8
FIELD_SLOTS = 4


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def constants(cfg):
    """hs, mass and del2W as sph_create computes them (cfg: an SphConfig or a dict of one)."""
    return dict(hs=f32(f32(_get(cfg, "h")) * f32(_get(cfg, "simulationScale"))), mass=f32(_get(cfg, "mass")),
                del2W=float(_get(cfg, "del2WviscosityCoefficient")))


def participates(state, types):
    """bool[N]: P(x) of the contract: type 1..3 with its bit in the mask, and a valid cell key."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.asarray(state["types"], np.float32)).astype(np.int64)
    mask = diag_ref.type_mask(types)
    ok = (t >= 1) & (t <= 3) & (((1 << np.clip(t, 0, 31)) & mask) != 0)
    return ok & (np.asarray(state["keys"]).astype(np.int64) < int(state["G"]))


class Diffusion:
    """The rows of one state for one type mask. P bool[N]; used bool[N, 32]; w float32[N, 32] = hs - dist; sD float32[N];
    W float32[N], the weight sums; sums(c) gives S for a sorted field c."""

    def __init__(self, state, ids, dist, K, types):
        self.rho = np.asarray(state["rho"], np.float32)
        self.ids = np.asarray(ids, np.int64).reshape(-1, SLOTS)
        self.dist = np.asarray(dist, np.float32).reshape(-1, SLOTS)
        self.N = self.rho.shape[0]
        self.P = participates(state, types)
        self.hs = f32(K["hs"])
        self.jc = np.maximum(self.ids, 0)
        self.used = (self.ids != -1) & (self.dist < self.hs) & self.P[self.jc] & self.P[:, None]
        self.w = (self.hs - self.dist).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            self.sD = (f32(K["mass"]) * (K["del2W"] / self.rho.astype(np.float64)).astype(np.float32)).astype(np.float32)
            W = np.zeros(self.N, np.float32)
            for k in range(SLOTS):
                tw = (self.w[:, k] / self.rho[self.jc[:, k]]).astype(np.float32)
                W = np.where(self.used[:, k], W + tw, W).astype(np.float32)
        self.W = W
        self._lanes = [np.flatnonzero(self.used[:, k]) for k in range(SLOTS)]

    def sums(self, c, want_abs=True):
        """(S float32[N], A float64[N] = the sums of |term| over the used slots, or None) for the sorted field c. Only the
        lanes that use a slot do its arithmetic: a slot that is not used leaves the sums untouched."""
        c = np.asarray(c, np.float32)
        S = np.zeros(self.N, np.float32)
        A = np.zeros(self.N, np.float64) if want_abs else None
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for k in range(SLOTS):
                i = self._lanes[k]
                j = self.jc[i, k]
                term = (((c[j] - c[i]).astype(np.float32) * self.w[i, k]).astype(np.float32) / self.rho[j]).astype(np.float32)
                S[i] = (S[i] + term).astype(np.float32)
                if want_abs:
                    A[i] += np.abs(term.astype(np.float64))
        return S, A

    def sigma(self, coefficient):
        """The stability number: max over P(i) of a_i * W_i by float compares, starting from +0."""
        with np.errstate(invalid="ignore", over="ignore"):
            x = ((f32(coefficient) * self.sD).astype(np.float32) * self.W).astype(np.float32)[self.P]
        x = x[x > 0]  # a value counts when it is greater than what the maximum holds, which starts at +0 (a NaN never is)
        return f32(x.max()) if x.size else f32(0)

    def run(self, c, coefficient, substeps):
        """(c' float32[N] in sorted order, sigma, A): `substeps` Jacobi substeps; A = sum_i a_i sum_k |term| of the FIRST substep,
        in float64 (the scale of the rounding error of the sum of c)."""
        c = np.asarray(c, np.float32).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            a = (f32(coefficient) * self.sD).astype(np.float32)
        A = 0.0
        for n in range(substeps):
            S, absS = self.sums(c, want_abs=n == 0)
            if n == 0:
                A = float((a.astype(np.float64) * absS)[self.P].sum())
            with np.errstate(invalid="ignore", over="ignore"):
                new = (c + (a * S).astype(np.float32)).astype(np.float32)
            c = np.where(self.P, new, c).astype(np.float32)
        return c, self.sigma(coefficient), A

    def asymmetric_pairs(self):
        """(directed used pairs, those whose mirror is not used with the same stored distance)."""
        i, k = np.nonzero(self.used)
        j = self.ids[i, k]
        r = self.dist[i, k]
        key = i.astype(np.int64) * self.N + j
        mirror = j.astype(np.int64) * self.N + i
        order = np.argsort(key, kind="stable")
        key_s, r_s = key[order], r[order]
        at = np.searchsorted(key_s, mirror)
        at_c = np.minimum(at, key_s.size - 1)
        found = (at < key_s.size) & (key_s[at_c] == mirror)
        same = found & (r_s[at_c].view(np.uint32) == r.view(np.uint32))
        return int(key.size), int((~same).sum())


def field_sorted(values, orig_ids):
    return np.asarray(values, np.float32)[np.asarray(orig_ids, np.int64)]


def diffuse(state, ids, dist, K, values, coefficient, substeps, types, D=None):
    """sph_field_diffuse on a field in ORIGINAL-id order: (values', sigma, A). state["ids"]: the original id of every sorted
    particle. D: a Diffusion of the same state and types, to share among calls."""
    if D is None:
        D = Diffusion(state, ids, dist, K, types)
    orig = np.asarray(state["ids"], np.int64)
    c, sigma, A = D.run(field_sorted(values, orig), coefficient, substeps)
    out = np.asarray(values, np.float32).copy()
    if substeps > 0:
        out[orig[D.P]] = c[D.P]
    return out, sigma, A


# ---- painting and the edits (the CURRENT particle set, original-id order) -------------------------------------------------------
def marked(position4, region, types):
    """bool[N]: the marking rule of sph_remove_region on float32[N, 4] positions: type and half-open box, no key condition."""
    pos = np.asarray(position4, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        t = np.trunc(pos[:, 3]).astype(np.int64)
    mask = diag_ref.type_mask(types)
    ok = (t >= 1) & (t <= 3) & (((1 << np.clip(t, 0, 31)) & mask) != 0)
    b = np.asarray(diag_ref.EVERYTHING if region is None else region, np.float32).reshape(6)
    for k in range(3):
        ok &= (b[k] <= pos[:, k]) & (pos[:, k] < b[3 + k])
    return ok


def paint_region(values, position4, region, types, value):
    m = marked(position4, region, types)
    out = np.asarray(values, np.float32).copy()
    out[m] = f32(value)
    return out, int(m.sum())


def paint_ids(values, orig_ids, value):
    out = np.asarray(values, np.float32).copy()
    out[np.asarray(orig_ids, np.int64)] = f32(value)
    return out


def follow_removal(values, edit_map):
    """The field after a removal whose old-to-new map is edit_map (-1: removed)."""
    m = np.asarray(edit_map, np.int64)
    keep = m >= 0
    out = np.empty(int(keep.sum()), np.float32)
    out[m[keep]] = np.asarray(values, np.float32)[keep]
    return out


def follow_add(values, count, inflow):
    return np.concatenate([np.asarray(values, np.float32), np.full(count, f32(inflow), np.float32)])


# ---- region records -------------------------------------------------------------------------------------------------------------
def diag_records(state, c_sorted, regions, types):
    """float64[R, 8] of sph_field_diagnostics for the field in SORTED order."""
    c = np.asarray(c_sorted, np.float32)
    cd = c.astype(np.float64)
    regions = np.asarray(regions, np.float32).reshape(-1, 6)
    out = np.zeros((regions.shape[0], DIAG_WORDS), np.float64)
    for r, region in enumerate(regions):
        sel = diag_ref.selected(state, region, types)
        out[r, 0] = diag_ref.tree_sum(sel.astype(np.float64))
        if not sel.any():
            continue
        out[r, 1] = diag_ref.tree_sum(np.where(sel, cd, 0.0))
        out[r, 2] = diag_ref.tree_sum(np.where(sel, cd * cd, 0.0))
        out[r, 3] = np.float64(f32(c[sel].min()) + f32(0.0))
        out[r, 4] = np.float64(f32(c[sel].max()) + f32(0.0))
        out[r, 5] = diag_ref.tree_sum((sel & (c != 0)).astype(np.float64))
    return out
