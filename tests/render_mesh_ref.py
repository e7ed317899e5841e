"""numpy restatement of the triangle-rendering contract (include/sphmi.h, sph_render_mesh / sph_read_render_triangles).

Works from the contract alone: projection and snap in float32 in the written order, coverage from int64 edge functions with the
ownership rule on a zero, the fragment's depth in float32, the winner as np.minimum.at over uint64 keys, the resolve by the same
expressions. `render_mesh(..., all_pixels=True)` tests every pixel of the image against every triangle: the definition. The default
searches each triangle's clipped bounding box (vectorised per window offset up to SMALL pixels a side, per triangle above that),
which must equal it. Vertices are float32[V, 3] scene positions and triangles int[T, 3] vertex ids; for the membranes the caller
gathers the corners (membrane_vertices). `view` is an sphmi.SphRenderView."""
import numpy as np

import render_ref as rr

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL = 16
LARGE_BOX = 8  # the kernels queue a triangle whose clipped box is above LARGE_BOX pixels a side
LIMIT = f32(1048576.0)


def membrane_vertices(state, back, membranes):
    """(positions float32[3M, 3], triangles int64[M, 3], sorted index of every corner) of the membrane table `membranes`
    (original ids, [M, 3]) on a state with pos in sorted order and `back` = particleIndexBack."""
    corners = np.asarray(membranes, np.int64).reshape(-1)
    j = np.asarray(back, np.int64)[corners]
    pos = np.asarray(state["pos"], np.float32)[j, :3]
    return pos, np.arange(corners.size, dtype=np.int64).reshape(-1, 3), j


def project(view, pos):
    """(X, Y, zi, usable) of every vertex: the contract's VERTICES."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    eye, right, up, fwd = rr.vec(view.eye, 3), rr.vec(view.right, 3), rr.vec(view.up, 3), rr.vec(view.forward, 3)
    d = [pos[:, k] - eye[k] for k in range(3)]
    cx = (d[0] * right[0] + d[1] * right[1]) + d[2] * right[2]
    cy = (d[0] * up[0] + d[1] * up[1]) + d[2] * up[2]
    cz = (d[0] * fwd[0] + d[1] * fwd[1]) + d[2] * fwd[2]
    scale = f32(view.scale)
    with np.errstate(all="ignore"):
        k = scale / cz if view.projection else np.full_like(cz, scale)
        u = cx * k + f32(view.centre[0])
        v = f32(view.centre[1]) - cy * k
        usable = (cz > f32(view.nearPlane)) & (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
        X = np.where(usable, np.floor(u * f32(256.0) + f32(0.5)), 0).astype(np.int64)
        Y = np.where(usable, np.floor(v * f32(256.0) + f32(0.5)), 0).astype(np.int64)
        zi = (f32(1.0) / cz if view.projection else cz).astype(np.float32)
    return X, Y, zi, usable


def edge(Xp, Yp, Xq, Yq, Xr, Yr):
    return (Xq - Xp) * (Yr - Yp) - (Yq - Yp) * (Xr - Xp)


def owns(Xp, Yp, Xq, Yq):
    dx, dy = Xq - Xp, Yq - Yp
    return (dy > 0) | ((dy == 0) & (dx < 0))


class Setup:
    """The drawn triangles of a table: ids (b and c exchanged where the table order is clockwise), snapped corners, zi, A."""

    def __init__(self, view, pos, tris):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        X, Y, zi, usable = project(view, pos)
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ok = usable[a] & usable[b] & usable[c]
        A = edge(X[a], Y[a], X[b], Y[b], X[c], Y[c])
        drawn = ok & (A != 0)
        self.unusable = int((~ok).sum())
        self.degenerate = int((ok & (A == 0)).sum())
        swap = A < 0
        b, c = np.where(swap, c, b), np.where(swap, b, c)
        A = np.abs(A)
        t = np.flatnonzero(drawn)
        self.count, self.t = tris.shape[0], t
        self.table = tris[t]  # table order, for the flat normal
        self.a, self.b, self.c, self.A = a[t], b[t], c[t], A[t]
        self.X = [X[self.a], X[self.b], X[self.c]]
        self.Y = [Y[self.a], Y[self.b], Y[self.c]]
        self.z = [zi[self.a], zi[self.b], zi[self.c]]
        W, H = int(view.width), int(view.height)
        self.bx0, self.bx1 = np.minimum.reduce(self.X) >> 8, np.maximum.reduce(self.X) >> 8
        self.by0, self.by1 = np.minimum.reduce(self.Y) >> 8, np.maximum.reduce(self.Y) >> 8
        self.x0, self.x1 = np.maximum(self.bx0, 0), np.minimum(self.bx1, W - 1)
        self.y0, self.y1 = np.maximum(self.by0, 0), np.minimum(self.by1, H - 1)


def fragment(view, S, k, px, py):
    """(covered, exists, l1, l2, depth) of triangles S[k] at pixels (px, py), elementwise: COVERAGE and FRAGMENT."""
    Px, Py = 256 * np.asarray(px, np.int64) + 128, 256 * np.asarray(py, np.int64) + 128
    Xa, Xb, Xc = (x[k] for x in S.X)
    Ya, Yb, Yc = (y[k] for y in S.Y)
    w0 = edge(Xb, Yb, Xc, Yc, Px, Py)
    w1 = edge(Xc, Yc, Xa, Ya, Px, Py)
    w2 = edge(Xa, Ya, Xb, Yb, Px, Py)
    covered = ((w0 > 0) | ((w0 == 0) & owns(Xb, Yb, Xc, Yc))) & ((w1 > 0) | ((w1 == 0) & owns(Xc, Yc, Xa, Ya))) & \
              ((w2 > 0) | ((w2 == 0) & owns(Xa, Ya, Xb, Yb)))
    A = S.A[k].astype(np.float32)
    with np.errstate(all="ignore"):
        l1 = w1.astype(np.float32) / A
        l2 = w2.astype(np.float32) / A
        za, zb, zc = (z[k] for z in S.z)
        z = (za + l1 * (zb - za)) + l2 * (zc - za)
        depth = (f32(1.0) / z if view.projection else z).astype(np.float32)
        exists = covered & (depth > f32(view.nearPlane)) & np.isfinite(depth)
    return covered, exists, l1, l2, depth


def candidates(view, S, all_pixels):
    """Yields (k, px, py): positions in S and the pixels to test them at."""
    W, H = int(view.width), int(view.height)
    n = S.t.shape[0]
    if all_pixels:
        yy, xx = np.mgrid[0:H, 0:W]
        xx, yy = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
        step = max(1, (1 << 22) // max(W * H, 1))
        for first in range(0, n, step):
            k = np.arange(first, min(first + step, n), dtype=np.int64)
            yield np.repeat(k, xx.size), np.tile(xx, k.size), np.tile(yy, k.size)
        return
    bw, bh = S.x1 - S.x0 + 1, S.y1 - S.y0 + 1
    inside = (bw > 0) & (bh > 0)
    small = inside & (bw <= SMALL) & (bh <= SMALL)
    s = np.flatnonzero(small)
    if s.size:
        for oy in range(int(bh[s].max())):
            for ox in range(int(bw[s].max())):
                m = s[(ox < bw[s]) & (oy < bh[s])]
                if m.size:
                    yield m, S.x0[m] + ox, S.y0[m] + oy
    for k in np.flatnonzero(inside & ~small):
        yy, xx = np.mgrid[S.y0[k]:S.y1[k] + 1, S.x0[k]:S.x1[k] + 1]
        xx, yy = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
        yield np.full(xx.shape, k, np.int64), xx, yy


def flat_normals(pos, table):
    """sph_membrane_measure's unit normal of the triangles `table` (ids in table order): float32[n, 3]."""
    pos = np.asarray(pos, np.float32)
    a, b, c = pos[table[:, 0]], pos[table[:, 1]], pos[table[:, 2]]
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(all="ignore"):
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        flat = ln == 0
        n = np.stack([nx / ln, ny / ln, nz / ln], 1).astype(np.float32)
    n[flat] = 0
    return n


def render_mesh(view, pos, tris, shading=0, normals=None, colour=(0.8, 0.8, 0.8), scalar=None, lo=0.0, hi=1.0, base=None,
                all_pixels=False):
    """The images and counts of one sph_render_mesh, plus what the tests assert about it. `normals` float32[V, 3] (shading 1),
    `scalar` float32[V] (colour mode 1), `base`: the images of the render composed over (a dict with depth, index, orig_id,
    rgba), None for a fresh image. Extra keys: `cover` (how many drawn triangles cover each pixel centre, whether or not their
    fragment exists), `winners` (distinct winning triangles), `queued` (drawn triangles whose clipped box is above 8 pixels a
    side), `partly_outside` (drawn triangles whose box crosses the image border and still meets the image), `unusable` and
    `degenerate` (the two reasons for a skip), `ties` (pixels whose winning depth bits came from more than one triangle),
    `boxes` (the drawn triangles t and their clipped boxes)."""
    W, H = int(view.width), int(view.height)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    S = Setup(view, pos, tris)
    keys = np.full(W * H, EMPTY, np.uint64)
    cover = np.zeros(W * H, np.int64)
    allpix, allkey = [], []
    for k, px, py in candidates(view, S, all_pixels):
        covered, exists, _, _, depth = fragment(view, S, k, px, py)
        pix = py * W + px
        np.add.at(cover, pix[covered], 1)
        key = (depth[exists].view(np.uint32).astype(np.uint64) << np.uint64(32)) | S.t[k[exists]].astype(np.uint64)
        np.minimum.at(keys, pix[exists], key)
        allpix.append(pix[exists]); allkey.append(key)
    has = keys != EMPTY
    cp = np.flatnonzero(has)
    win_t = (keys[cp] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    depth = (keys[cp] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    if base is not None:
        take = depth < np.asarray(base["depth"], np.float32).reshape(-1)[cp]
        cp, win_t, depth = cp[take], win_t[take], depth[take]
        out_depth = np.array(base["depth"], np.float32).reshape(-1).copy()
        out_index = np.array(base["index"], np.int32).reshape(-1).copy()
        out_id = np.array(base["orig_id"], np.uint32).reshape(-1).copy()
        rgba = np.array(base["rgba"], np.uint8).reshape(-1, 4).copy()
    else:
        out_depth = np.full(W * H, np.inf, np.float32)
        out_index = np.full(W * H, -1, np.int32)
        out_id = np.full(W * H, 0xFFFFFFFF, np.uint32)
        rgba = np.empty((W * H, 4), np.uint8)
        rgba[:] = np.array([view.background[k] for k in range(4)], np.uint8)
    triangle = np.full(W * H, -1, np.int32)
    out_depth[cp] = depth
    out_index[cp] = -1
    out_id[cp] = 0xFFFFFFFF
    triangle[cp] = win_t
    if cp.size:
        k = np.searchsorted(S.t, win_t)  # the winner's set-up and fragment again, by the same expressions
        _, _, l1, l2, _ = fragment(view, S, k, cp % W, cp // W)
        with np.errstate(all="ignore"):
            if shading == 0:
                n = flat_normals(pos, S.table[k])
            else:
                nv = np.asarray(normals, np.float32)
                na, nb, nc = nv[S.a[k]], nv[S.b[k]], nv[S.c[k]]
                n = (na + l1[:, None] * (nb - na)) + l2[:, None] * (nc - na)
                ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
                none = ~((ln > 0) & np.isfinite(ln))
                n = (n / ln[:, None]).astype(np.float32)
                n[none] = 0
            fwd = rr.vec(view.forward, 3)
            facing = np.abs((n[:, 0] * fwd[0] + n[:, 1] * fwd[1]) + n[:, 2] * fwd[2])
            if scalar is None:
                c = np.tile(np.asarray(colour, np.float32).reshape(1, 3), (cp.size, 1))
            else:
                q = np.asarray(scalar, np.float32)
                qa, qb, qc = q[S.a[k]], q[S.b[k]], q[S.c[k]]
                c = rr.field_colour((qa + l1 * (qb - qa)) + l2 * (qc - qa), lo, hi)
            rgba[cp] = rr.shade_bytes(view, c, facing.astype(np.float32))
    pix = np.concatenate(allpix) if allpix else np.zeros(0, np.int64)
    key = np.concatenate(allkey) if allkey else np.zeros(0, np.uint64)
    tie = (key >> np.uint64(32) == keys[pix] >> np.uint64(32)) & (key != keys[pix])
    sides = np.maximum(S.x1 - S.x0 + 1, S.y1 - S.y0 + 1)
    inside = (S.x1 >= S.x0) & (S.y1 >= S.y0)
    crosses = inside & ((S.bx0 < 0) | (S.by0 < 0) | (S.bx1 > W - 1) | (S.by1 > H - 1))
    covered_any = int(cp.size) if base is None else int(np.isfinite(out_depth).sum())
    return dict(depth=out_depth.reshape(H, W), index=out_index.reshape(H, W), orig_id=out_id.reshape(H, W), rgba=rgba.reshape(H, W, 4),
                triangle=triangle.reshape(H, W), counts=(int(S.t.size), int(S.count - S.t.size), int(cp.size), covered_any),
                cover=cover.reshape(H, W), winners=int(np.unique(win_t).size), queued=int((inside & (sides > LARGE_BOX)).sum()),
                partly_outside=int(crosses.sum()), unusable=S.unusable, degenerate=S.degenerate, ties=int(np.unique(pix[tie]).size),
                fragments=int(pix.size), boxes=dict(t=S.t, x0=S.x0, x1=S.x1, y0=S.y0, y1=S.y1))


def surface_scalar(records, field):
    """The vertex scalar of source 0 from the sph_sample_points records at the vertices: word `field`, or the speed (6)."""
    r = np.asarray(records, np.float32)
    if field < 6:
        return r[:, field].copy()
    return np.sqrt((r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3]) + r[:, 4] * r[:, 4]).astype(np.float32)

