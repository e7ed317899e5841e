"""numpy float32 restatement of the isosurface contract (include/sphmi.h, sph_extract_surface), vectorised over the lattice
(no Python loop over cells), plus the mesh checks the tests share.

surface_reference(f, origin, spacing, iso) takes the scalar lattice f[nz, ny, nx] (word `field` of sph_sample_grid's records)
and returns (vertices float32[V, 3], triangles int32[T, 3]) in the contract's order. The case table comes from
tools/gen_mc_table.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table  # noqa: E402

f32 = np.float32
TRI_COUNT = np.array([len(t) for t in gen_mc_table.TABLE], np.int64)
TRI_EDGES = np.zeros((256, gen_mc_table.MAX_TRIS, 3), np.int64)
for _c, _tris in enumerate(gen_mc_table.TABLE):
    for _q, _t in enumerate(_tris):
        TRI_EDGES[_c, _q] = _t
# cube edge e -> (first corner's lattice offset (dx, dy, dz), axis)
EDGE_START = np.array([gen_mc_table.CORNERS[a] for a, _ in gen_mc_table.EDGES], np.int64)
EDGE_AXIS = np.arange(12) // 4


def lattice_coords(origin, spacing, n, axis):
    """origin + (float)i * spacing of one axis, float32."""
    return f32(origin[axis]) + np.arange(n, dtype=np.float32) * f32(spacing[axis])


def surface_reference(f, origin, spacing, iso):
    f = np.asarray(f, np.float32)
    nz, ny, nx = f.shape
    iso = f32(iso)
    inside = f >= iso  # NaN: outside
    # crossed-edge masks per lattice point: bit a = the edge from the point along axis a
    mask = np.zeros(f.shape, np.int64)
    mask[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]).astype(np.int64)
    mask[:, :-1, :] |= (inside[:, :-1, :] != inside[:, 1:, :]).astype(np.int64) << 1
    mask[:-1, :, :] |= (inside[:-1, :, :] != inside[1:, :, :]).astype(np.int64) << 2
    pc = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1)
    flat_pc = pc.reshape(-1)
    base = np.concatenate([[0], np.cumsum(flat_pc)[:-1]]).reshape(f.shape)  # first vertex id of each point
    V = int(flat_pc.sum())
    # vertices: points in x-fastest order, within a point +x, +y, +z
    xs = lattice_coords(origin, spacing, nx, 0)
    ys = lattice_coords(origin, spacing, ny, 1)
    zs = lattice_coords(origin, spacing, nz, 2)
    verts = np.empty((V, 3), np.float32)
    kk, jj, ii = np.nonzero(mask != 0)  # x-fastest order
    for axis in range(3):
        sel = (mask[kk, jj, ii] >> axis) & 1 == 1
        k, j, i = kk[sel], jj[sel], ii[sel]
        vid = base[k, j, i] + sum(((mask[k, j, i] >> a) & 1) for a in range(axis))
        k1, j1, i1 = k + (axis == 2), j + (axis == 1), i + (axis == 0)
        f0, f1 = f[k, j, i], f[k1, j1, i1]
        t = (iso - f0) / (f1 - f0)
        p = np.stack([xs[i], ys[j], zs[k]], axis=1)
        c0 = (xs, ys, zs)[axis][(i, j, k)[axis]]
        c1 = (xs, ys, zs)[axis][(i1, j1, k1)[axis]]
        p[:, axis] = c0 + t * (c1 - c0)
        verts[vid] = p
    # cells: case of each cell, triangles in x-fastest cell order, table order within a cell
    ins = inside.astype(np.int64)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(gen_mc_table.CORNERS):
        case |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] << c
    ntri = TRI_COUNT[case]
    ck, cj, ci = np.nonzero(ntri > 0)
    cc = case[ck, cj, ci]
    rep = ntri[ck, cj, ci]
    T = int(rep.sum())
    which = np.arange(T) - np.repeat(np.cumsum(rep) - rep, rep)  # triangle index within its cell
    ck, cj, ci, cc = (np.repeat(a, rep) for a in (ck, cj, ci, cc))
    edges = TRI_EDGES[cc, which]  # [T, 3]
    tris = np.empty((T, 3), np.int64)
    for q in range(3):
        e = edges[:, q]
        pk, pj, pi = ck + EDGE_START[e, 2], cj + EDGE_START[e, 1], ci + EDGE_START[e, 0]
        axis = EDGE_AXIS[e]
        m = mask[pk, pj, pi]
        lower = np.where(axis >= 1, m & 1, 0) + np.where(axis >= 2, (m >> 1) & 1, 0)
        assert ((m >> axis) & 1 == 1).all()
        tris[:, q] = base[pk, pj, pi] + lower
    return verts, tris.astype(np.int32)


def directed_edge_report(tris, n_vertices):
    """Closedness and orientation of a triangle mesh: None when every directed edge (a, b) occurs exactly once together with
    (b, a) exactly once, every vertex is used and no triangle repeats a vertex; otherwise a description of the first fault."""
    t = np.asarray(tris, np.int64)
    if t.size == 0:
        return None if n_vertices == 0 else "no triangles but %d vertices" % n_vertices
    if ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any():
        return "a triangle repeats a vertex"
    if t.min() < 0 or t.max() >= n_vertices:
        return "vertex id out of range"
    used = np.zeros(n_vertices, bool)
    used[t.reshape(-1)] = True
    if not used.all():
        return "%d vertices unused" % int((~used).sum())
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    key = a * n_vertices + b
    u, cnt = np.unique(key, return_counts=True)
    if (cnt != 1).any():
        return "%d directed edges occur more than once" % int((cnt != 1).sum())
    rev = b * n_vertices + a
    if not np.isin(rev, u).all():
        return "%d directed edges lack their reverse" % int((~np.isin(rev, u)).sum())
    return None


def euler_characteristic(vertices, tris):
    t = np.asarray(tris, np.int64)
    nv = np.asarray(vertices).shape[0]
    e = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0).shape[0]
    return nv - e + t.shape[0]


def signed_volume(vertices, tris):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(tris, np.int64)
    v0, v1, v2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)
