"""CPU tests of the connected-components restatement (tests/components_ref.py) against a plain breadth-first search on synthetic
neighbour rows, and of the frames helpers that go with the labelling. No GPU, no solver."""
import numpy as np
import pytest

import components_ref as cr
import diag_ref
import scenes  # noqa: F401  (puts the package on sys.path)
from sphmi import frames

f32 = np.float32


def make_rows(N, directed):
    """int32[N, 32] rows from (owner, neighbour) pairs, -1 padded, in the given order."""
    rows = np.full((N, 32), -1, np.int32)
    fill = np.zeros(N, np.int64)
    for i, j in directed:
        assert fill[i] < 32
        rows[i, fill[i]] = j
        fill[i] += 1
    return rows


def line_positions(N, step=1.0):
    pos = np.zeros((N, 3), np.float32)
    pos[:, 0] = np.arange(N, dtype=np.float32) * f32(step)
    return pos


def check_against_bfs(rows, sel, pos, link=np.inf):
    labels, rc, bbox = cr.label(rows, sel, pos, link)
    a, b = cr.edges(rows, sel, pos, link)
    want = cr.bfs_labels(len(sel), sel, a, b)
    assert np.array_equal(labels, want)
    C = rc.shape[0]
    assert C == (want.max() + 1 if (want >= 0).any() else 0)
    assert np.array_equal(labels >= 0, sel)
    for c in range(C):
        members = np.flatnonzero(labels == c)
        assert rc[c, 0] == members[0] and rc[c, 1] == members.size
        p = np.asarray(pos, np.float32)[members]
        assert np.array_equal(bbox[c, :3], p.min(0) + f32(0)) and np.array_equal(bbox[c, 3:], p.max(0) + f32(0))
    assert np.all(np.diff(rc[:, 0]) > 0)  # numbered by ascending root
    assert int(rc[:, 1].sum()) == int(np.sum(sel))
    return labels, rc, bbox


def test_chain_in_scrambled_edge_order():
    N = 200
    rng = np.random.default_rng(1)
    pairs = [(i, i + 1) if rng.random() < 0.5 else (i + 1, i) for i in range(N - 1)]
    order = rng.permutation(len(pairs))
    rows = make_rows(N, [pairs[k] for k in order])
    labels, rc, _ = check_against_bfs(rows, np.ones(N, bool), line_positions(N))
    assert rc.tolist() == [[0, N]] and (labels == 0).all()


def test_two_blobs_ring_and_isolated_particle():
    # blob A = 0..9 (complete), ring = 10..29, isolated = 30, blob B = 31..39 (star around 35)
    directed = [(i, j) for i in range(10) for j in range(10) if i != j]
    directed += [(10 + k, 10 + (k + 1) % 20) for k in range(20)]
    directed += [(35, j) for j in range(31, 40) if j != 35]
    rows = make_rows(40, directed)
    labels, rc, _ = check_against_bfs(rows, np.ones(40, bool), line_positions(40))
    assert rc.tolist() == [[0, 10], [10, 20], [30, 1], [31, 9]]
    assert labels[30] == 2 and labels[39] == 3


def test_star_at_the_cap_with_one_sided_rows():
    """The hub's row is full (32 entries); a 33rd spoke is linked only because the hub is in ITS row."""
    N = 40
    hub = 20
    spokes = [j for j in range(N) if j != hub][:32]
    late = [j for j in range(N) if j != hub][32]
    directed = [(hub, j) for j in spokes] + [(late, hub)]
    rows = make_rows(N, directed)
    assert (rows[hub] >= 0).all() and late not in rows[hub]
    labels, rc, _ = check_against_bfs(rows, np.ones(N, bool), line_positions(N))
    assert labels[late] == labels[hub] == 0 and rc[0, 1] == 34
    assert rc.shape[0] == 1 + (N - 34)  # the particles the hub does not reach are components of one


def test_unselected_bridge_splits_two_groups():
    # 0-1-2 and 4-5-6 are joined only through particle 3, which is a boundary particle
    directed = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 5)]
    rows = make_rows(7, directed)
    state = dict(pos=line_positions(7), types=np.array([1.1, 1.1, 1.1, 3.1, 1.1, 1.1, 1.1], np.float32), keys=np.zeros(7, np.uint32), G=8)
    labels, rc, _ = cr.label_state(state, rows, (1, 2))
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and rc.tolist() == [[0, 3], [4, 3]]
    labels, rc, _ = cr.label_state(state, rows, (1, 2, 3))
    assert labels.tolist() == [0] * 7 and rc.tolist() == [[0, 7]]
    state["keys"][5] = 8  # outside the cell table: not selected, whatever its type
    labels, rc, _ = cr.label_state(state, rows, (1, 2, 3))
    assert labels.tolist() == [0, 0, 0, 0, 0, -1, 1] and rc.tolist() == [[0, 5], [6, 1]]


def test_pair_at_exactly_the_link_radius_is_not_linked():
    pos = np.array([[0, 0, 0], [3, 4, 0], [3, 4, 12]], np.float32)  # distances 5 and 12, exact in float32
    rows = make_rows(3, [(0, 1), (2, 1)])
    sel = np.ones(3, bool)
    assert cr.label(rows, sel, pos, 5.0)[1].tolist() == [[0, 1], [1, 1], [2, 1]]  # r2 == link2: strict <
    assert cr.label(rows, sel, pos, np.nextafter(f32(5.0), f32(6.0)))[1].tolist() == [[0, 2], [2, 1]]
    assert cr.label(rows, sel, pos, 12.0)[1].tolist() == [[0, 2], [2, 1]]
    assert cr.label(rows, sel, pos, 12.5)[1].tolist() == [[0, 3]]
    assert cr.label(rows, sel, pos, np.inf)[1].tolist() == [[0, 3]]
    pos[2, 2] = np.nan  # +inf reads no position: the entry is kept; any finite radius drops it
    with np.errstate(all="ignore"):
        assert cr.label(rows, sel, pos, np.inf)[1].tolist() == [[0, 3]]
        assert cr.label(rows, sel, pos, 1e30)[1][:, 1].tolist() == [2, 1]  # (link2 overflows to +inf: the test is still made)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            cr.label(rows, sel, pos, bad)


def test_numbering_by_ascending_root():
    # components {5, 1}, {0, 9}, {2}, {3, 4, 8}, {6, 7}: roots 0, 1, 2, 3, 6
    rows = make_rows(10, [(5, 1), (9, 0), (8, 3), (4, 8), (7, 6)])
    labels, rc, _ = check_against_bfs(rows, np.ones(10, bool), line_positions(10))
    assert rc[:, 0].tolist() == [0, 1, 2, 3, 6]
    assert labels.tolist() == [0, 1, 2, 3, 3, 1, 4, 4, 3, 0]


def test_empty_selection():
    rows = make_rows(5, [(0, 1), (1, 2)])
    labels, rc, bbox = cr.label(rows, np.zeros(5, bool), line_positions(5))
    assert labels.tolist() == [-1] * 5 and rc.shape == (0, 2) and bbox.shape == (0, 6)


@pytest.mark.parametrize("seed,n,radius", [(3, 3000, 0.08), (4, 5000, 0.07), (5, 2000, 0.1)])
def test_random_geometric_graphs(seed, n, radius):
    """Points in the unit cube, rows = the up to 4 nearest points within `radius` (so rows are capped and one-sided), a third of
    the points unselected, several link radii from far below to above the row radius."""
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 3)).astype(np.float32)
    order = np.lexsort((pos[:, 0], pos[:, 1], pos[:, 2]))
    pos = pos[order]
    cell = np.floor(pos / radius).astype(np.int64)
    buckets = {}
    for idx, c in enumerate(map(tuple, cell)):
        buckets.setdefault(c, []).append(idx)
    rows = np.full((n, 32), -1, np.int32)
    for i in range(n):
        cand = []
        cx, cy, cz = cell[i]
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    cand += buckets.get((cx + dx, cy + dy, cz + dz), [])
        cand = np.array([c for c in cand if c != i], np.int64)
        if cand.size == 0:
            continue
        d2 = ((pos[cand].astype(np.float64) - pos[i]) ** 2).sum(1)
        near = cand[d2 < radius * radius][np.argsort(d2[d2 < radius * radius])][:4]  # a small cap makes the rows one-sided
        rows[i, :near.size] = near
    sel = rng.random(n) > 0.33
    one_sided = 0
    for i in range(0, n, 50):
        for j in rows[i][rows[i] >= 0]:
            one_sided += i not in rows[j]
    assert one_sided > 0
    counts = set()
    below_all = 0.5 * float(np.sqrt(cr.graph(rows, pos)[2].min()))  # below the smallest pair distance: nothing is linked
    for link in (np.inf, radius, 0.7 * radius, 0.4 * radius, below_all):
        _, rc, _ = check_against_bfs(rows, sel, pos, link)
        counts.add(rc.shape[0])
    assert len(counts) >= 4 and int(sel.sum()) in counts


def test_component_records_use_the_membership():
    rng = np.random.default_rng(7)
    N = 3000
    state = dict(pos=rng.random((N, 3)).astype(np.float32), vel=rng.standard_normal((N, 3)).astype(np.float32),
                 rho=(1000 + rng.standard_normal(N)).astype(np.float32), p=rng.random(N).astype(np.float32),
                 types=np.full(N, 1.1, np.float32), keys=np.zeros(N, np.uint32), G=4, ids=rng.permutation(N).astype(np.int64))
    labels = rng.integers(-1, 3, N).astype(np.int32)
    rec = cr.component_records(state, labels, [2, 0, 2], 1000.0)
    assert rec.shape == (3, 32) and np.array_equal(rec[0].view(np.uint64), rec[2].view(np.uint64))
    for r, c in ((0, 2), (1, 0)):
        m = labels == c
        assert rec[r, 0] == m.sum()
        assert rec[r, 1] == diag_ref.tree_sum(np.where(m, state["pos"][:, 0].astype(np.float64), 0.0))
        assert rec[r, 23] == state["pos"][m, 0].min() and rec[r, 28] == state["pos"][m, 2].max()
        v2 = diag_ref.terms(state, 1000.0)[9]
        idx = int(np.flatnonzero(m)[np.argmax(v2[m])])
        assert rec[r, 21] == idx and rec[r, 22] == state["ids"][idx]
    # one component holding everything: the record of the region "everything"
    everything = cr.component_records(state, np.zeros(N, np.int32), [0], 1000.0)
    want = diag_ref.records(state, [diag_ref.EVERYTHING], (1,), 1000.0)
    assert np.array_equal(everything.view(np.uint64), want.view(np.uint64))


def test_frames_component_summary_and_original_order():
    rc = np.array([[0, 5], [2, 40], [7, 1], [9, 40]], np.int32)
    bbox = np.arange(24, dtype=np.float32).reshape(4, 6)
    s = frames.component_summary(rc, bbox, 0.5)
    assert s["components"] == 4 and s["largest"] == 1 and s["largest_n"] == 40 and s["outside_largest"] == 46
    assert s["order"].tolist() == [1, 3, 0, 2] and s["sizes"].tolist() == [40, 40, 5, 1]
    assert s["mass"].tolist() == [2.5, 20.0, 0.5, 20.0] and s["largest_bbox"] == tuple(float(x) for x in bbox[1])
    empty = frames.component_summary(np.zeros((0, 2), np.int32), np.zeros((0, 6), np.float32), 1.0)
    assert empty["components"] == 0 and empty["largest"] == -1 and empty["outside_largest"] == 0
    with pytest.raises(ValueError):
        frames.component_summary(rc, bbox[:3], 1.0)
    # sorted position k holds orig particle pi[k, 1]
    pi = np.array([[0, 3], [0, 0], [1, 2], [4, 1]], np.uint32)
    labels = np.array([7, -1, 5, 6], np.int32)
    assert frames.labels_in_original_order(labels, pi).tolist() == [-1, 6, 5, 7]
    with pytest.raises(ValueError):
        frames.labels_in_original_order(labels[:3], pi)


def test_frame_writers_take_labels(tmp_path):
    pos = np.array([[0, 0, 0, 1.1], [1, 0, 0, 3.1], [2, 0, 0, 2.1]], np.float32)
    rho = np.array([1000, 1001, 1002], np.float32)
    plain, with_labels = str(tmp_path / "a.vtk"), str(tmp_path / "b.vtk")
    assert frames.write_vtk(plain, pos, rho) == 2
    assert frames.write_vtk(with_labels, pos, rho, labels=[4, -1, 9]) == 2
    a, b = open(plain, "rb").read(), open(with_labels, "rb").read()
    assert b.startswith(a) and b"component" not in a  # the default output is unchanged
    tail = b[len(a):]
    assert tail.startswith(b"SCALARS component int 1\nLOOKUP_TABLE default\n")
    assert np.frombuffer(tail[len(b"SCALARS component int 1\nLOOKUP_TABLE default\n"):-1], ">i4").tolist() == [4, 9]
    with pytest.raises(ValueError):
        frames.write_vtk(with_labels, pos, rho, labels=[1, 2])
    frames.write_npz(str(tmp_path / "a.npz"), pos, rho, step=3)
    frames.write_npz(str(tmp_path / "b.npz"), pos, rho, step=3, labels=[4, -1, 9])
    assert "component" not in np.load(str(tmp_path / "a.npz")).files
    z = np.load(str(tmp_path / "b.npz"))
    assert z["component"].dtype == np.int32 and z["component"].tolist() == [4, -1, 9] and int(z["step"]) == 3


def test_components_csv_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    steps = [2, 4]
    ids = [np.array([3, 0, 1]), np.array([0])]
    rc = [rng.integers(0, 1000, (3, 2)).astype(np.int32), rng.integers(0, 1000, (1, 2)).astype(np.int32)]
    bb = [rng.standard_normal((3, 6)).astype(np.float32), rng.standard_normal((1, 6)).astype(np.float32)]
    rec = [rng.standard_normal((3, 32)) * 1e6, rng.standard_normal((1, 32))]
    rec[0][1, 5] = -0.0
    path = str(tmp_path / "c.csv")
    frames.write_components_csv(path, steps, ids, rc, bb, rec)
    s, i, r, b, d = frames.read_components_csv(path)
    assert s.tolist() == [2, 2, 2, 4] and i.tolist() == [3, 0, 1, 0]
    assert np.array_equal(r, np.concatenate(rc))
    assert np.array_equal(b.view(np.uint32), np.concatenate(bb).view(np.uint32))
    assert np.array_equal(d.view(np.uint64), np.concatenate(rec).view(np.uint64))
    with open(path) as f:
        assert f.readline().startswith("step,component,root,n,min_x")
    bad = str(tmp_path / "bad.csv")
    with open(bad, "w") as f:
        f.write("step,region\n")
    with pytest.raises(ValueError):
        frames.read_components_csv(bad)
    with pytest.raises(ValueError):
        frames.write_components_csv(path, [1], [np.array([0, 1])], [rc[1]], [bb[1]], [rec[1]])
