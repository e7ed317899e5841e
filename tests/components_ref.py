"""numpy restatement of the connected-components contract (include/sphmi.h, sph_label_components / sph_read_components /
sph_component_diagnostics), independent of the library's answer.

Works from the contract alone: the nodes are the particles sph_diagnostics selects for the region "everything"; the edges are
the valid entries of the neighbour rows between two selected particles, from either end (symmetric closure), kept when
r2 < link2 with r2 = (dx*dx + dy*dy) + dz*dz in float32 and link2 = linkRadius * linkRadius in float32 (no test at all for
+inf); components are numbered by ascending lowest sorted index; the table holds root, members and the float32 bounding box
canonicalised by + 0.0f; per-component records come from diag_ref's terms / tree_sum machinery with the membership as selection.
The state comes from diag_ref.state_with_ids(hip), the rows from hip.neighbor_rows in pieces."""
import numpy as np

import diag_ref

f32 = np.float32


def neighbor_rows(hip, piece=1 << 18):
    """int32[N, 32]: every sorted particle's neighbour row (-1 = empty slot)."""
    out = np.empty((hip.N, 32), np.int32)
    for first in range(0, hip.N, piece):
        n = min(piece, hip.N - first)
        ids, _ = hip.neighbor_rows(first, n)
        out[first:first + n] = ids
    return out


def selected(state, types):
    return diag_ref.selected(state, diag_ref.EVERYTHING, types)


def row_pairs(rows, sel):
    """(i, j) int64 arrays: every row entry j >= 0 of a selected particle i that names another selected particle."""
    rows = np.asarray(rows)
    N, width = rows.shape
    i = np.repeat(np.arange(N, dtype=np.int64), width)
    j = rows.reshape(-1).astype(np.int64)
    ok = (j >= 0) & (j < N) & (i != j)
    i, j = i[ok], j[ok]
    ok = sel[i] & sel[j]
    return i[ok], j[ok]


def pair_r2(pos, i, j):
    """float32 squared distances of the contract: d = x_i - x_j per coordinate, (dx*dx + dy*dy) + dz*dz."""
    p = np.asarray(pos, np.float32)
    d = p[i] - p[j]
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def graph(rows, pos):
    """(a, b, r2): every undirected pair a < b that either particle's row holds, once, with its float32 r2; whatever the
    selection (row_pairs with everything selected). Reusable across type sets and radii of one state."""
    i, j = row_pairs(rows, np.ones(np.asarray(rows).shape[0], bool))
    N = np.asarray(rows).shape[0]
    key = np.unique(np.minimum(i, j) * N + np.maximum(i, j))
    a, b = key // N, key % N
    return a, b, pair_r2(pos, a, b)  # (float negation is exact: r2 is the same from either end)


def edges(rows, sel, pos, link_radius, g=None):
    """The contract's edge list as undirected pairs (a < b), each once. `g`: graph(rows, pos), if the caller has it."""
    link = f32(link_radius)
    if np.isnan(link) or not link > 0:
        raise ValueError("link_radius must be > 0")
    a, b, r2 = graph(rows, pos) if g is None else g
    keep = sel[a] & sel[b]
    if not np.isinf(link):
        with np.errstate(over="ignore"):
            link2 = f32(link * link)
        keep &= r2 < link2
    return a[keep], b[keep]


def roots_of(N, sel, i, j):
    """int64[N]: the lowest index of each selected particle's component (-1 where not selected). Hooking of the larger root
    under the smaller for every edge at once, then pointer jumping until flat; repeated until no edge joins two trees."""
    lab = np.where(sel, np.arange(N, dtype=np.int64), -1)
    for _ in range(N + 2):
        a, b = lab[i], lab[j]
        differ = a != b
        if not differ.any():
            return lab
        a, b = a[differ], b[differ]
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))
        while True:  # pointer jumping
            nxt = np.where(lab >= 0, lab[np.maximum(lab, 0)], -1)
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    raise AssertionError("labelling did not converge")


def label(rows, sel, pos, link_radius=np.inf, g=None):
    """(labels int32[N], root_count int32[C, 2], bbox float32[C, 6]) by the contract."""
    sel = np.asarray(sel, bool)
    N = sel.size
    i, j = edges(rows, sel, pos, link_radius, g)
    root = roots_of(N, sel, i, j)
    roots = np.unique(root[sel])  # ascending: the numbering
    labels = np.full(N, -1, np.int32)
    labels[sel] = np.searchsorted(roots, root[sel]).astype(np.int32)
    C = roots.size
    rc = np.zeros((C, 2), np.int32)
    rc[:, 0] = roots
    rc[:, 1] = np.bincount(labels[sel], minlength=C)
    p = np.asarray(pos, np.float32)[sel]
    bbox = np.empty((C, 6), np.float32)
    bbox[:, :3] = np.inf
    bbox[:, 3:] = -np.inf
    for k in range(3):
        np.minimum.at(bbox[:, k], labels[sel], p[:, k])
        np.maximum.at(bbox[:, 3 + k], labels[sel], p[:, k])
    return labels, rc, (bbox + f32(0.0)).astype(np.float32)


def label_state(state, rows, types, link_radius=np.inf, g=None):
    return label(rows, selected(state, types), state["pos"], link_radius, g)


def component_records(state, labels, ids, rho0):
    """float64[len(ids), 32]: diag_ref's record with "selected" = labels == id. diag_ref.record selects by type, key and box:
    a copy of the state whose non-members have type 0 makes its selection the membership."""
    t = diag_ref.terms(state, rho0)
    out = []
    for c in ids:
        member = np.asarray(labels) == int(c)
        st = dict(state)
        st["types"] = np.where(member, f32(1.0), f32(0.0)).astype(np.float32)
        st["keys"] = np.zeros(member.size, np.int64)
        st["G"] = 1
        out.append(diag_ref.record(st, diag_ref.EVERYTHING, (1,), rho0, state.get("ids"), t))
    return np.stack(out) if out else np.zeros((0, diag_ref.WORDS), np.float64)


def bfs_labels(N, sel, i, j):
    """Plain breadth-first labelling of the same graph, numbered by ascending root: the check of the restatement itself."""
    adj = [[] for _ in range(N)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        adj[a].append(b)
        adj[b].append(a)
    labels = np.full(N, -1, np.int32)
    c = 0
    for s in range(N):
        if not sel[s] or labels[s] >= 0:
            continue
        labels[s] = c
        queue = [s]
        while queue:
            nxt = []
            for u in queue:
                for v in adj[u]:
                    if labels[v] < 0:
                        labels[v] = c
                        nxt.append(v)
            queue = nxt
        c += 1
    return labels


def oracle_state(ora, cfg):
    """The same dict as diag_ref.state_with_ids, and the rows, from the C oracle's buffers (no GPU): for choosing radii."""
    N = int(cfg.particleCount)
    sp = ora.buffer("sortedPosition").reshape(-1, 4)[:N, :3].copy()
    sv = ora.buffer("sortedVelocity").reshape(-1, 4)[:N, :3].copy()
    pi = ora.buffer("particleIndex").reshape(-1, 2)
    types = ora.buffer("position").reshape(-1, 4)[:N][pi[:, 1], 3]
    state = dict(pos=sp, vel=sv, rho=ora.buffer("rho")[:N].copy(), p=ora.buffer("pressure")[:N].copy(), types=types,
                 keys=pi[:, 0].copy(), G=int(cfg.gridCellCount), ids=pi[:, 1].astype(np.int64))
    rows = ora.buffer("neighborIds").reshape(N, 32).astype(np.int32)
    return state, rows
