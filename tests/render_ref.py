"""numpy restatement of the rendering contract (include/sphmi.h, sph_render_particles / sph_read_render).

Works from the contract alone: projection, fragment, key, colour and thickness in float32 in the written order, the winner as
np.minimum.at over uint64 keys, the thickness as an integer sum. Vectorised over particles per window offset for footprints up
to SMALL pixels a side, per particle over its clipped box above that. `render(..., all_pixels=True)` tests every pixel of the
image against every particle instead: the definition the restricted search must equal. The state is diag_ref.state_with_ids(hip)
(or a hand-made dict with the same keys); `view` is an sphmi.SphRenderView."""
import numpy as np

import diag_ref
from sphmi import frames

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL = 16
LARGE_BOX = 8  # the kernels queue a splat whose clipped search box is above LARGE_BOX pixels a side
LIMIT = f32(1048576.0)


def vec(a, n):
    return np.array([a[k] for k in range(n)], np.float32)


def project(view, pos):
    """(u, v, R, R2, cz, drawn) of every particle: the contract's PROJECTION."""
    pos = np.asarray(pos, np.float32)
    eye, right, up, fwd = vec(view.eye, 3), vec(view.right, 3), vec(view.up, 3), vec(view.forward, 3)
    d = [pos[:, k] - eye[k] for k in range(3)]
    cx = (d[0] * right[0] + d[1] * right[1]) + d[2] * right[2]
    cy = (d[0] * up[0] + d[1] * up[1]) + d[2] * up[2]
    cz = (d[0] * fwd[0] + d[1] * fwd[1]) + d[2] * fwd[2]
    scale, radius = f32(view.scale), f32(view.radius)
    with np.errstate(all="ignore"):
        k = scale / cz if view.projection else np.full_like(cz, scale)
        u = cx * k + f32(view.centre[0])
        v = f32(view.centre[1]) - cy * k
        R = radius * k
        R2 = R * R
        drawn = (cz > f32(view.nearPlane)) & (R > 0) & (R <= f32(view.maxRadiusPx)) & (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
    return u, v, R, R2, cz, drawn


def fragment(view, u, v, R2, cz, px, py):
    """(exists, nz, depth) of the fragments of splats (u, v, R2, cz) at pixels (px, py), elementwise: the contract's FRAGMENTS."""
    dx = (np.asarray(px).astype(np.float32) + f32(0.5)) - u
    dy = (np.asarray(py).astype(np.float32) + f32(0.5)) - v
    d2 = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        covered = d2 <= R2
        nz = np.sqrt(f32(1.0) - d2 / R2).astype(np.float32)
        depth = cz - f32(view.radius) * nz
        exists = covered & (depth > f32(view.nearPlane))
    return exists, nz, depth


def search_box(view, u, v, R):
    """The clipped search box floor(u - R) - 1 .. floor(u + R) + 1 (likewise in y) of drawn splats, as int64 arrays."""
    x0 = np.maximum(np.floor(u - R).astype(np.int64) - 1, 0)
    x1 = np.minimum(np.floor(u + R).astype(np.int64) + 1, view.width - 1)
    y0 = np.maximum(np.floor(v - R).astype(np.int64) - 1, 0)
    y1 = np.minimum(np.floor(v + R).astype(np.int64) + 1, view.height - 1)
    return x0, x1, y0, y1


def density_colour(rho, rho0):
    return frames.density_colour(rho, rho0)


def field_colour(q, lo, hi):
    """float32[n, 3]: colour mode 2 of the quantity q."""
    q = np.asarray(q, np.float32)
    inv = f32(1.0) / (f32(hi) - f32(lo))
    with np.errstate(all="ignore"):
        s = np.fmin(np.fmax((q - f32(lo)) * inv, f32(0)), f32(1))
    a = s * f32(4.0)
    i = np.minimum(a.astype(np.int32), 3)
    f = a - i.astype(np.float32)
    stop = frames.FIELD_RAMP
    return (stop[i] + f[:, None] * (stop[i + 1] - stop[i])).astype(np.float32)


def label_colour(labels):
    lab = np.asarray(labels, np.int64)
    c = frames.LABEL_PALETTE[np.where(lab < 0, 0, lab % 12)].copy()
    c[lab < 0] = f32(0.5)
    return c


def shade_bytes(view, c, nz):
    """uint8[n, 4]: base colours c [n, 3] shaded by nz [n], A = 255."""
    amb = f32(view.ambient)
    shade = amb + (f32(1.0) - amb) * nz
    x = np.fmin(np.fmax(c * shade[:, None], f32(0)), f32(1)) * f32(255.0) + f32(0.5)
    out = np.full((nz.shape[0], 4), 255, np.uint8)
    out[:, :3] = x.astype(np.int32).astype(np.uint8)
    return out


def thickness_word(nz):
    return (nz * f32(256.0) + f32(0.5)).astype(np.int32).astype(np.uint32)


def saturate(sums):
    return np.minimum(np.asarray(sums, np.uint64), np.uint64(0xFFFFFFFF)).astype(np.uint32)


def fragments(view, j, u, v, R, R2, cz, all_pixels=False):
    """(pixel int64[F], splat int64[F] (position in j), nz float32[F], depth float32[F]) of every fragment of the drawn splats."""
    W, H = int(view.width), int(view.height)
    pix, who, nzs, deps = [], [], [], []

    def keep(ok, px, py, idx, nz, depth):
        pix.append((py * W + px)[ok]); who.append(idx[ok]); nzs.append(nz[ok]); deps.append(depth[ok])
    n = j.shape[0]
    if all_pixels:
        yy, xx = np.mgrid[0:H, 0:W]
        xx, yy = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
        for k in range(n):
            ok, nz, depth = fragment(view, u[k], v[k], R2[k], cz[k], xx, yy)
            keep(ok, xx, yy, np.full(xx.shape, k, np.int64), nz, depth)
    else:
        x0, x1, y0, y1 = search_box(view, u, v, R)
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        inside = (bw > 0) & (bh > 0)
        small = inside & (bw <= SMALL) & (bh <= SMALL)
        s = np.flatnonzero(small)
        if s.size:
            for oy in range(int(bh[s].max())):
                for ox in range(int(bw[s].max())):
                    m = s[(ox < bw[s]) & (oy < bh[s])]
                    if m.size == 0:
                        continue
                    px, py = x0[m] + ox, y0[m] + oy
                    ok, nz, depth = fragment(view, u[m], v[m], R2[m], cz[m], px, py)
                    keep(ok, px, py, m, nz, depth)
        for k in np.flatnonzero(inside & ~small):
            yy, xx = np.mgrid[y0[k]:y1[k] + 1, x0[k]:x1[k] + 1]
            xx, yy = xx.reshape(-1).astype(np.int64), yy.reshape(-1).astype(np.int64)
            ok, nz, depth = fragment(view, u[k], v[k], R2[k], cz[k], xx, yy)
            keep(ok, xx, yy, np.full(xx.shape, k, np.int64), nz, depth)
    if not pix:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, np.float32), np.zeros(0, np.float32)
    return np.concatenate(pix), np.concatenate(who), np.concatenate(nzs), np.concatenate(deps)


def render(state, view, region=None, types=(1, 2), thickness=False, rho0=None, labels=None, nbr_counts=None, all_pixels=False):
    """The five images and the counts of one render, plus what the tests assert about it: `ties` (pixels whose winning depth bits
    came from more than one particle), `winners` (distinct winning particles), `fragments`, `max_box` (the largest side of a
    clipped search box), `candidates`, `boxes` (the drawn particles j and their clipped search boxes) and `queued` (drawn
    particles whose box meets the image and is above 8 pixels a side)."""
    W, H = int(view.width), int(view.height)
    pos = np.asarray(state["pos"], np.float32)
    sel = diag_ref.selected(state, diag_ref.EVERYTHING if region is None else region, types)
    u, v, R, R2, cz, ok = project(view, pos)
    j = np.flatnonzero(sel & ok).astype(np.int64)
    u, v, R, R2, cz = u[j], v[j], R[j], R2[j], cz[j]
    pix, who, nz, depth = fragments(view, j, u, v, R, R2, cz, all_pixels)
    key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[who].astype(np.uint64)
    keys = np.full(W * H, EMPTY, np.uint64)
    np.minimum.at(keys, pix, key)
    sums = np.zeros(W * H, np.uint64)
    if thickness:
        np.add.at(sums, pix, thickness_word(nz).astype(np.uint64))
    covered = keys != EMPTY
    cp = np.flatnonzero(covered)
    win = (keys[cp] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out_depth = np.full(W * H, np.inf, np.float32)
    out_depth[cp] = (keys[cp] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    out_index = np.full(W * H, -1, np.int32)
    out_index[cp] = win
    out_id = np.full(W * H, 0xFFFFFFFF, np.uint32)
    out_id[cp] = np.asarray(state["ids"])[win].astype(np.uint32)
    rgba = np.empty((W * H, 4), np.uint8)
    rgba[:] = np.array([view.background[k] for k in range(4)], np.uint8)
    if cp.size:
        # the winner's fragment again, by the same expressions
        wu, wv, wR, wR2, wcz, _ = project(view, pos[win])
        _, wnz, _ = fragment(view, wu, wv, wR2, wcz, cp % W, cp // W)
        mode = int(view.colourMode)
        if mode == 0:
            t = np.asarray(state["types"], np.float32).astype(np.int32)[win]
            c = np.array([[view.typeColour[a][b] for b in range(3)] for a in range(3)], np.float32)[t - 1]
        elif mode == 1:
            c = density_colour(np.asarray(state["rho"], np.float32)[win], rho0)
        elif mode == 2:
            c = field_colour(diag_ref.field_values(state, int(view.field), nbr_counts)[win], view.lo, view.hi)
        else:
            c = label_colour(np.asarray(labels)[win])
        rgba[cp] = shade_bytes(view, c, wnz)
    tie = (key >> np.uint64(32) == keys[pix] >> np.uint64(32)) & (key != keys[pix])
    x0, x1, y0, y1 = search_box(view, u, v, R)
    sides = np.maximum(x1 - x0 + 1, y1 - y0 + 1)
    inside = (x1 >= x0) & (y1 >= y0)
    queued = int((inside & (sides > LARGE_BOX)).sum())
    sides = sides[inside]
    return dict(depth=out_depth.reshape(H, W), index=out_index.reshape(H, W), orig_id=out_id.reshape(H, W), rgba=rgba.reshape(H, W, 4),
                thickness=saturate(sums).reshape(H, W) if thickness else None, sums=sums.reshape(H, W), drawn=int(j.size),
                covered=int(cp.size), ties=int(np.unique(pix[tie]).size), winners=int(np.unique(win).size),
                fragments=int(pix.size), max_box=int(sides.max()) if sides.size else 0, candidates=int(sel.sum()),
                boxes=dict(j=j, x0=x0, x1=x1, y0=y0, y1=y1), queued=queued)
