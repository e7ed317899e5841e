"""CPU checks of the binned-diagnostics contract's numpy restatement (tests/bin_ref.py) on synthetic states -- the edge rules, the
whole axis, coinciding edges, the tiling -- of the helpers of sphmi/frames.py, and, on the C oracle's state of the scenes that
tests/test_bins.py runs on the GPU, that the lattices of tests/bin_cases.py give that test something to compare: bins with
members in more than one chunk of 1024, empty bins beside them, and mostly occupied bins. No GPU needed."""
import os

import numpy as np
import pytest

import bin_cases as bc
import bin_ref
import diag_ref
import forces_ref as fr
import scenes
import sphmi
import tree_edge_cases as tc
from sphmi import frames

f32 = np.float32
RHO0 = f32(1000.0)


def make_state(pos, vel=None, types=None, keys=None, G=1000):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n = pos.shape[0]
    return dict(pos=pos, vel=np.zeros((n, 3), np.float32) if vel is None else np.asarray(vel, np.float32).reshape(n, 3),
                rho=np.full(n, RHO0, np.float32), p=np.zeros(n, np.float32),
                types=np.ones(n, np.float32) if types is None else np.asarray(types, np.float32),
                keys=np.zeros(n, np.uint32) if keys is None else np.asarray(keys, np.uint32), G=G,
                ids=np.arange(n, dtype=np.int64)[::-1].copy())


def lattice(n=12, spacing=1.67):
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (ijk.astype(np.float32) * f32(spacing) + f32(3.0)).astype(np.float32)


# ---- the edge rules ----
def test_inner_edge_goes_to_the_upper_bin_and_the_outer_upper_edge_to_none():
    g = sphmi.bin_lattice((1.0, 0.0, 0.0), (0.5, 1.0, 1.0), (4, 1, 1), (1,))
    ex, ey, ez = frames.bin_edges(g)
    assert ex.dtype == np.float32 and ex.tolist() == [1.0, 1.5, 2.0, 2.5, 3.0] and ey.tolist() == [0.0, 1.0] == ez.tolist()
    below = np.nextafter(f32(1.0), f32(0))
    xs = [below, 1.0, np.nextafter(f32(1.5), f32(0)), 1.5, 2.0, 2.75, np.nextafter(f32(3.0), f32(0)), 3.0, np.nan]
    st = make_state([[x, 0.5, 0.5] for x in xs])
    assert bin_ref.index(st, g).tolist() == [-1, 0, 0, 1, 2, 3, 3, -1, -1]
    rec = bin_ref.records(st, g, RHO0)
    assert rec[:, 0].tolist() == [2, 1, 1, 2]
    # the same from the boxes, one region at a time: the tiling is the boxes' half-open rule
    boxes = frames.bin_boxes(g)
    assert np.array_equal(boxes, bin_ref.boxes(g)) and boxes.shape == (4, 6)
    sel = np.stack([diag_ref.selected(st, b, (1,)) for b in boxes])
    assert (sel.sum(0) <= 1).all() and sel.sum(1).tolist() == [2, 1, 1, 2]
    # y and z: on the upper edge of the only bin -> none; types and keys as diagnostics
    st = make_state([[1.2, 1.0, 0.5], [1.2, 0.5, 1.0], [1.2, 0.0, 0.0], [1.2, 0.5, 0.5], [1.2, 0.5, 0.5]], types=[1, 1, 1, 3, 1],
                    keys=[0, 0, 0, 0, 1000], G=1000)
    assert bin_ref.index(st, g).tolist() == [-1, -1, 0, -1, -1]


def test_edges_are_the_float32_expression():
    """origin + (float32)i * spacing with both roundings: not origin + i * spacing in double, and not an accumulated sum."""
    g = sphmi.bin_lattice((0.1, 0.0, 0.0), (0.1, 1.0, 1.0), (40, 1, 1))
    ex = frames.bin_edges(g)[0]
    want = np.array([f32(f32(0.1) + f32(f32(i) * f32(0.1))) for i in range(41)], np.float32)
    assert np.array_equal(ex.view(np.uint32), want.view(np.uint32)) and np.array_equal(ex, bin_ref.edges(g)[0])
    acc = np.cumsum(np.full(41, f32(0.1), np.float32), dtype=np.float32)
    assert not np.array_equal(ex, acc)  # (the accumulated sum drifts)
    assert (np.diff(ex) > 0).all()


def test_whole_axis():
    g = sphmi.bin_lattice((5.0, 0.0, 0.0), (0.0, 0.0, 2.0), (1, 1, 3), (1,))
    ex, ey, ez = frames.bin_edges(g)
    assert ex.tolist() == [-np.inf, np.inf] == ey.tolist() and ez.tolist() == [0.0, 2.0, 4.0, 6.0]
    st = make_state([[-1e30, 1e30, 0.0], [7.0, -3.0, 5.9], [0.0, 0.0, 6.0], [np.inf, 0.0, 1.0], [-np.inf, 0.0, 1.0], [0.0, np.nan, 1.0]])
    assert bin_ref.index(st, g).tolist() == [0, 2, -1, -1, 0, -1]  # -inf <= x < +inf, as the box (-inf, +inf) selects
    boxes = frames.bin_boxes(g)
    assert np.array_equal(boxes[1], np.array([-np.inf, -np.inf, 2.0, np.inf, np.inf, 4.0], np.float32))
    assert [int(diag_ref.selected(st, b, (1,)).sum()) for b in boxes] == [2, 0, 1]


def test_coinciding_edges_give_empty_bins_and_lose_no_particle():
    """An origin so large against the spacing that consecutive float edges coincide: the bins between equal edges are empty, and
    every particle between the outer edges is in exactly one bin."""
    o, s, n = f32(2.0 ** 24), f32(0.25), 64
    g = sphmi.bin_lattice((o, 0, 0), (s, 0, 0), (n, 1, 1), (1,))
    ex = frames.bin_edges(g)[0]
    assert (np.diff(ex) >= 0).all() and (np.diff(ex) == 0).sum() > n // 2 and ex[-1] > ex[0]
    xs = np.arange(float(ex[0]) - 4, float(ex[-1]) + 4, 1.0, dtype=np.float64).astype(np.float32)  # every float in reach (ulp 2 up there: some twice)
    st = make_state(np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], 1))
    idx = bin_ref.index(st, g)
    inside = (xs >= ex[0]) & (xs < ex[-1])
    assert inside.sum() > 4 and np.array_equal(idx >= 0, inside)
    cnt = np.bincount(idx[idx >= 0], minlength=n)
    assert (cnt[np.diff(ex) == 0] == 0).all() and cnt.sum() == inside.sum()
    for b in np.flatnonzero(cnt):
        assert ((xs[idx == b] >= ex[b]) & (xs[idx == b] < ex[b + 1])).all()
    rec = bin_ref.records(st, g, RHO0)
    assert np.array_equal(rec[:, 0], cnt.astype(np.float64))


def test_counts_add_up_to_the_outer_box():
    pos = lattice(12)
    rng = np.random.default_rng(3)
    st = make_state(pos, vel=rng.standard_normal(pos.shape).astype(np.float32), types=np.where(np.arange(len(pos)) % 3 == 0, 3.0, 1.0))
    for types in ((1,), (1, 3)):
        g = sphmi.bin_lattice((4.0, 3.0, 5.5), (1.9, 3.3, 2.45), (5, 3, 4), types)
        rec = bin_ref.records(st, g, RHO0)
        idx = bin_ref.index(st, g)
        outer = diag_ref.record(st, bin_ref.outer_box(g), types, RHO0)
        assert rec.shape == (60, 32) and 0 < outer[0] < diag_ref.record(st, diag_ref.EVERYTHING, types, RHO0)[0]
        assert rec[:, 0].sum() == outer[0] == (idx >= 0).sum()
        assert np.array_equal(np.bincount(idx[idx >= 0], minlength=60), rec[:, 0].astype(np.int64))
        assert np.allclose(rec[:, 4:7].sum(0), outer[4:7], rtol=1e-12, atol=1e-9)  # momentum is shared out, up to rounding
        assert rec[:, 26].max() == outer[26] and rec[rec[:, 0] > 0, 23].min() == outer[23]


# ---- frames ----
class Cfg:
    mass, rho0, simulationScale = 0.5, 1000.0, 0.25


def test_bin_profile_and_column_depth():
    rec = np.zeros((2, 1, 3, 32))
    rec[0, 0, 0, :14] = [4, 1, 2, 3, 8, -4, 2, 0, 0, 0, 0, 4400, 0, 10]
    rec[1, 0, 2, :14] = [1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 990, 0, 0]
    with np.errstate(all="raise"):  # empty bins: no division by zero, no NaN
        p = frames.bin_profile(rec, Cfg)
    assert p["n"].shape == (2, 1, 3) and p["mean_velocity"].shape == (2, 1, 3, 3) and np.isfinite(p["mean_velocity"]).all()
    assert p["mean_velocity"][0, 0, 0].tolist() == [2, -1, 0.5] and p["mean_density"][0, 0, 0] == 1100 and p["mass"][0, 0, 0] == 2
    assert p["mean_density"][1, 0, 2] == 990 and p["mean_density"][0, 0, 1] == 0 and p["mean_pressure"][0, 0, 0] == 2.5
    g = sphmi.bin_lattice((0, 0, 0), (2.0, 0.0, 4.0), (3, 1, 2))
    d = frames.bin_column_depth(rec, Cfg, g)
    volume = 0.5 / 1000.0 / 0.25 ** 3  # scene units cubed per particle
    assert d.shape == (2, 1, 3) and d[0, 0, 0] == 4 * (volume / 8.0) and d[0, 0, 1] == 0 and d[1, 0, 2] == volume / 8.0
    for bad in (sphmi.bin_lattice((0, 0, 0), (2, 1, 4), (3, 1, 2)), sphmi.bin_lattice((0, 0, 0), (0, 0, 4), (1, 1, 6))):
        with pytest.raises(ValueError):
            frames.bin_column_depth(rec, Cfg, bad)
    with pytest.raises(ValueError):
        frames.bin_profile(np.zeros((3, 31)), Cfg)


def test_csv_and_vtk_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    rec = rng.standard_normal((3, 2, 1, 4, 32)) * 10.0 ** rng.uniform(-300, 300, (3, 2, 1, 4, 32))
    rec[0, 0, 0, 0, :6] = [0.0, -0.0, np.inf, -np.inf, 5e-324, 1.7976931348623157e308]
    rec[1, 1, 0, 3, 21:23] = -1
    steps = [2, 4, 9]
    path = str(tmp_path / "bins.csv")
    frames.write_bins_csv(path, steps, rec)
    s, got = frames.read_bins(path)
    assert s.tolist() == steps and got.shape == (3, 8, 32)
    assert np.array_equal(got.view(np.uint64), rec.reshape(3, 8, 32).view(np.uint64))  # every bit
    assert open(path).readline().strip() == "step,bin," + ",".join(frames.DIAG_FIELDS)
    with pytest.raises(ValueError):
        frames.read_diagnostics_csv(path)  # (a table of bins is not a table of regions)
    g = sphmi.bin_lattice((1, 0, 2), (0.5, 0, 0.25), (4, 1, 2))
    rec = np.zeros((2, 1, 4, 32))
    rec[..., 0] = np.arange(8).reshape(2, 1, 4)
    rec[..., 11] = 1000.0 * rec[..., 0]
    rec[..., 4] = 3.0 * rec[..., 0]
    vtk = str(tmp_path / "bins.vtk")
    assert frames.write_vtk_bins(vtk, g, rec, Cfg) == 8
    raw = open(vtk, "rb").read()
    assert b"DIMENSIONS 5 2 3\n" in raw and b"ORIGIN 1 0 2\n" in raw and b"SPACING 0.5 1 0.25\n" in raw and b"CELL_DATA 8\n" in raw
    at = raw.index(b"SCALARS n float 1\nLOOKUP_TABLE default\n") + len(b"SCALARS n float 1\nLOOKUP_TABLE default\n")
    assert np.frombuffer(raw[at:at + 32], ">f4").tolist() == list(range(8))
    at = raw.index(b"VECTORS mean_velocity float\n") + len(b"VECTORS mean_velocity float\n")
    assert np.frombuffer(raw[at:at + 96], ">f4").reshape(8, 3)[:, 0].tolist() == [0.0] + [3.0] * 7
    with pytest.raises(ValueError):
        frames.write_vtk_bins(vtk, g, rec[0], Cfg)


def test_wrapper_and_header():
    for bad in (dict(origin=(1, 2)), dict(spacing=(1, 2, 3, 4)), dict(dims=(4, 4)), dict(dims=(4.0, 4.0, 4.0)), dict(dims=(1 << 31, 1, 1))):
        args = dict(origin=(0, 0, 0), spacing=(1, 1, 1), dims=(4, 4, 4))
        args.update(bad)
        with pytest.raises(sphmi.SphError):
            sphmi.bin_lattice(**args)
    g = sphmi.bin_lattice((1, 2, 3), (0.5, 0.25, 0), (4, 5, 1), types=(1, 3))
    assert g.dtype == sphmi.STATS_LATTICE_DTYPE and g.nbytes == 40 and int(g["typeMask"][0]) == 10 and bin_ref.types_of(g) == (1, 3)
    assert sphmi.BIN_MAX_BINS == 1 << 18
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    lib = sphmi.device_lib()
    for n in ("sph_bin_diagnostics", "sph_bin_index"):
        assert n in sphmi.EXPORTED_SYMBOLS and hasattr(lib, n) and ("int %s(" % n) in txt
    assert "#define SPH_BIN_MAX_BINS (1 << 18)" in txt and "} sph_bin_lattice;" in txt


# ---- the lattices of the GPU test, on the oracle's state ----
def oracle_state(sc, steps=2):
    cfg = sc["cfg"]
    ora = scenes.oracle_for(sc)
    for _ in range(steps):
        ora.step()
    st, _, _ = fr.oracle_state(ora, cfg.particleCount, cfg.gridCellCount)
    ora.close()
    return st


@pytest.mark.parametrize("name", bc.SCENES)
def test_the_lattices_of_the_gpu_test_hold_something(name):
    """After two steps of the oracle: for every mask, each lattice that covers the matter has a bin with members in two different
    chunks of 1024, an empty bin, and fewer than half of its bins empty (the lattices are sized to the matter the mask selects);
    the partial lattice is full and spans chunks; the outside one is empty."""
    sc = scenes.SCENES[name]()
    cfg = sc["cfg"]
    st = oracle_state(sc)
    for types in bc.MASKS:
        for ln, g in bc.lattices(sc, types).items():
            B = int(np.prod(g["dims"][0]))
            idx = bin_ref.index(st, g)
            cnt = np.bincount(idx[idx >= 0], minlength=B)
            spans = bc.chunks_of(idx, B)
            what = (name, types, ln, int((cnt == 0).sum()), B, int(spans.max()))
            if ln == "outside":
                assert cnt.sum() == 0, what
                continue
            assert spans.max() >= 2, what
            assert 0 < cnt.sum() < diag_ref.selected(st, diag_ref.EVERYTHING, types).sum() or ln in bc.FULL, what
            if ln in bc.FULL:
                assert (cnt == 0).any(), what
                assert cnt.sum() == diag_ref.selected(st, diag_ref.EVERYTHING, types).sum(), what  # it covers the matter
                assert 2 * (cnt == 0).sum() < B, what
            else:
                assert (cnt > 0).all(), what
    g = bc.lattices(sc, (1, 2, 3))["fine3d"]
    assert float(g["spacing"][0][0]) < float(cfg.h)
    idx = bin_ref.index(st, g)
    assert max(np.unique(idx[c * 1024:(c + 1) * 1024]).size for c in range((idx.size + 1023) // 1024)) > 16  # one chunk, many bins


@pytest.mark.parametrize("n", tc.SIZES)
def test_the_chunk_edge_lattices_hold_something(n):
    sc = tc.scene(n)
    cfg = sc["cfg"]
    st = oracle_state(sc)
    for ln, g in bc.edge_lattices(cfg, tc.TYPES).items():
        B = int(np.prod(g["dims"][0]))
        idx = bin_ref.index(st, g)
        cnt = np.bincount(idx[idx >= 0], minlength=B)
        assert cnt.sum() == n, (ln, cnt.sum())  # both cover everything
        assert 2 * (cnt == 0).sum() < B
        if n == 1025:
            assert idx[1024] >= 0 and bc.chunks_of(idx, B)[idx[1024]] == 2  # the second chunk's one term lands in a bin of both chunks
