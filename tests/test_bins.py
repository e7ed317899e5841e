"""GPU tests of the binned diagnostics (sph_bin_diagnostics / sph_bin_index, include/sphmi.h): every word of every bin's record
bit-identical to the numpy restatement (tests/bin_ref.py over tests/diag_ref.py) and to sph_diagnostics over the bins' boxes, on
the lattices of tests/bin_cases.py (tests/test_bins_host.py shows on the oracle that they hold bins spanning chunks and empty
bins); the chunk edges of the tree (1024 and 1025 particles), three tree levels, the tiling, independence of the rest of the
lattice, read-only behaviour, the calling rules and the driver's CSV."""
import os
import subprocess

import numpy as np
import pytest

import bin_cases as bc
import bin_ref
import diag_ref
import scenes
import sphmi
import tree_edge_cases as tc
from sphmi import frames
from sphmi import slab as S

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
EMPTY = np.zeros(32)
EMPTY[21] = EMPTY[22] = -1


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(u64(got), u64(want)):
        b, w = [int(x[0]) for x in np.nonzero(u64(got) != u64(want))]
        raise AssertionError("%s: %d words differ; first bin %d word %d (%s): %r vs %r"
                             % (what, int((u64(got) != u64(want)).sum()), b, w, frames.DIAG_FIELDS[w], got[b, w], want[b, w]))


def by_regions(hip, lattice):
    """The route a caller had before: diagnostics() over the bins' boxes, 16 per call."""
    boxes, types = frames.bin_boxes(lattice), bin_ref.types_of(lattice)
    return np.concatenate([hip.diagnostics(boxes[b:b + 16], types) for b in range(0, boxes.shape[0], 16)])


def flat(hip, lattice):
    rec = hip.bin_diagnostics(lattice)
    nx, ny, nz = (int(v) for v in lattice["dims"][0])
    assert rec.shape == (nz, ny, nx, 32) and rec.dtype == np.float64
    return rec.reshape(-1, 32)


def check_lattice(hip, state, lattice, what, restate=True):
    got = flat(hip, lattice)
    if restate:
        assert_records(got, bin_ref.records(state, lattice, hip.cfg.rho0), what + ": against the restatement")
    assert_records(got, by_regions(hip, lattice), what + ": against diagnostics() over the boxes")
    idx = hip.bin_index(lattice)
    assert idx.dtype == np.int32 and idx.shape == (hip.N,)
    if restate:
        assert np.array_equal(idx, bin_ref.index(state, lattice)), what
    assert np.array_equal(np.bincount(idx[idx >= 0], minlength=got.shape[0]), got[:, 0].astype(np.int64)), what
    outer = hip.diagnostics([bin_ref.outer_box(lattice)], bin_ref.types_of(lattice))[0]
    assert got[:, 0].sum() == outer[0] == (idx >= 0).sum(), what
    return got, idx


@pytest.mark.parametrize("name", bc.SCENES)
def test_records_and_index_match_restatement_and_diagnostics(name):
    sc = scenes.SCENES[name]()
    hip = scenes.hip_for(sc)
    it = 0
    for steps in (1, 5):  # after steps 0 and 4
        while it < steps:
            hip.step(it)
            it += 1
        state = diag_ref.state_with_ids(hip)
        for types in bc.MASKS:
            for ln, g in bc.lattices(sc, types).items():
                what = "%s step %d types %s %s" % (name, it - 1, types, ln)
                got, idx = check_lattice(hip, state, g, what)
                if ln == "outside":
                    assert_records(got, np.tile(EMPTY, (got.shape[0], 1)), what + ": the empty record")
                else:
                    assert got[:, 0].max() > 0 and bc.chunks_of(idx, got.shape[0]).max() >= 2, what  # (no case passes vacuously)
                if ln in bc.FULL:  # as tests/test_bins_host.py finds on the oracle: an empty bin, fewer than half of them empty
                    assert (got[:, 0] == 0).any() and 2 * (got[:, 0] == 0).sum() < got.shape[0], what
    hip.close()


@pytest.mark.parametrize("n", tc.SIZES)
def test_chunk_edges(n):
    """Exactly 1024 particles: one chunk, no upper level, so a record is the leaf's partial untouched; exactly 1025: the second
    chunk holds one term of the positional level."""
    hip = scenes.hip_for(tc.scene(n))
    assert hip.N == n
    for it in range(2):
        hip.step(it)
    state = diag_ref.state_with_ids(hip)
    for ln, g in bc.edge_lattices(hip.cfg, tc.TYPES).items():
        got, idx = check_lattice(hip, state, g, "n %d %s" % (n, ln))
        assert got[:, 0].sum() == n
    one = flat(hip, bc.edge_lattices(hip.cfg, tc.TYPES)["one"])
    assert_records(one, hip.diagnostics(None, tc.TYPES), "n %d: the (1, 1, 1) lattice is everything" % n)
    hip.close()


def test_three_tree_levels_on_more_than_a_million_particles():
    """More than 1024^2 particles: the level above the 1024 slots runs. Against diagnostics() over the same boxes (the numpy route
    over 1.3 M particles x 24 boxes is too slow for a test)."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    assert sc["cfg"].particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    cfg = hip.cfg
    ext = np.array([cfg.xmax, cfg.ymax, cfg.zmax], np.float64)
    for types in ((1,), (1, 2, 3)):
        prof = sphmi.bin_lattice((0, 0, -ext[2] / 6), (0, 0, ext[2] / 6), (1, 1, 8), types)
        plan = sphmi.bin_lattice((-ext[0] / 3, 0, 0), (ext[0] / 3, 0, ext[2] / 4), (4, 1, 4), types)
        for ln, g in (("z profile", prof), ("plan", plan)):
            got, idx = check_lattice(hip, None, g, "1.3M types %s %s" % (types, ln), restate=False)
            assert (got[:, 0] == 0).any() and got[:, 0].max() > 1024 * 64
            groups = [np.unique(np.flatnonzero(idx == b) // (1024 * 1024)).size for b in range(got.shape[0])]
            assert max(groups) == 2 and min(groups) == 0  # bins in both level-1 groups, in one, in none
    hip.close()


def test_a_record_does_not_depend_on_the_rest_of_the_lattice():
    """Origin 0 and a power-of-two spacing make the float edges of the common bins the same values when the lattice grows by bins
    on every side."""
    hip = scenes.hip_for(scenes.SCENES["tiny_compressed"]())
    for it in range(3):
        hip.step(it)
    types = (1, 2, 3)
    small = sphmi.bin_lattice((0, 0, 0), (4, 8, 4), (5, 3, 5), types)
    big = sphmi.bin_lattice((-8, -16, -12), (4, 8, 4), (9, 6, 10), types)
    es, eb = frames.bin_edges(small), frames.bin_edges(big)
    for a, off in enumerate((2, 2, 3)):
        assert np.array_equal(es[a], eb[a][off:off + es[a].size])
    a, b = hip.bin_diagnostics(small), hip.bin_diagnostics(big)
    assert (a[..., 0] > 0).sum() > a[..., 0].size // 2
    assert_records(b[3:8, 2:5, 2:7].reshape(-1, 32), a.reshape(-1, 32), "common bins")
    assert b[..., 0].sum() >= a[..., 0].sum()
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_bins_are_read_only():
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    lat = bc.lattices(sc, (1, 2, 3))
    for it in range(6):
        a.step(it)
        b.step(it)
        before = {n: a.buffer(n) for n in BUFFERS}
        for g in lat.values():
            a.bin_diagnostics(g)
            a.bin_index(g)
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    assert np.array_equal(a.buffer("neighborIds"), b.buffer("neighborIds"))
    a.close()
    b.close()


def _rc(hip, g, index=False, null_lattice=False, null_out=False):
    dims = [max(int(v), 1) for v in g["dims"][0]]
    bins = min(dims[0] * dims[1] * dims[2], sphmi.BIN_MAX_BINS)
    out = np.empty(max(hip.N, 1), np.int32) if index else np.empty((bins, 32), np.float64)
    f = hip._L.sph_bin_index if index else hip._L.sph_bin_diagnostics
    return f(hip._h, None if null_lattice else g.ctypes.data, None if null_out else out.ctypes.data)


def test_error_rules():
    hip = scenes.hip_for(scenes.SCENES["tiny"]())
    ok = sphmi.bin_lattice((0, 0, 0), (4, 0, 4), (6, 1, 6), (1, 2))

    def both(g, **kw):
        a, b = _rc(hip, g, **kw), _rc(hip, g, index=True, **kw)
        assert a == b, (a, b)
        return a
    assert both(ok) == ERR_ORDER  # a fresh solver
    with pytest.raises(sphmi.SphError):
        hip.bin_diagnostics(ok)
    hip.step(0)
    assert both(ok) == 0
    for st in scenes.STAGE_SEQUENCE[:7]:  # a new step has begun: its density and pressure-force stages have not run yet
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert both(ok) == ERR_ORDER
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(1) if st == "integrate" else m()
    assert both(ok) == 0
    for mask in (0, 1, 0x10, 0x80000002):
        g = ok.copy()
        g["typeMask"] = mask
        assert both(g) == ERR_INVALID
    assert both(ok, null_lattice=True) == ERR_INVALID and both(ok, null_out=True) == ERR_INVALID
    for field, axis, value in (("origin", 0, np.nan), ("origin", 2, np.inf), ("spacing", 0, np.nan), ("spacing", 2, np.inf),
                               ("spacing", 0, -4.0), ("spacing", 0, 0.0), ("dims", 0, 0), ("dims", 1, -1), ("dims", 1, 2)):
        g = ok.copy()
        g[field][0][axis] = value  # (the last: dims 2 on the axis whose spacing is 0)
        assert both(g) == ERR_INVALID, (field, axis, value)
    assert both(sphmi.bin_lattice((0, 0, 0), (1, 1, 1), (64, 64, 64), (1,))) == 0  # SPH_BIN_MAX_BINS itself
    assert both(sphmi.bin_lattice((0, 0, 0), (1, 1, 1), (64, 64, 65), (1,))) == ERR_INVALID
    assert both(sphmi.bin_lattice((0, 0, 0), (1, 1, 1), (1 << 20, 1 << 20, 1 << 20), (1,))) == ERR_INVALID
    assert both(sphmi.bin_lattice((0, 0, 0), (0, 0, 0), (1, 1, 1), (1,))) == 0
    assert b"sph_bin_" in hip._L.sph_last_error()
    with pytest.raises(sphmi.SphError):
        hip.bin_diagnostics(np.zeros(3))
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    g = sphmi.bin_lattice((0, 0, 0), (4, 0, 4), (6, 1, 6), (1, 2))
    assert _rc(hip, g) == ERR_INVALID and _rc(hip, g, index=True) == ERR_INVALID
    hip.close()


def test_blown_up_state_is_sticky():
    """Coincident particles turn NaN in the first step (the scene of test_gpu_parity's blown-up tests); the next step's hash counts
    them, and from then on the bin calls report SPH_ERR_INVALID like every blocking call, again and again."""
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), jitter_in_r0=0.03)
    pos = sc["position"].copy()
    pos[5:10, :3] = pos[200:205, :3]
    sc["position"] = pos
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.step(1)
    g = sphmi.bin_lattice((0, 0, 0), (4, 0, 4), (6, 1, 6), (1, 2))
    for _ in range(2):
        assert _rc(hip, g) == ERR_INVALID and _rc(hip, g, index=True) == ERR_INVALID
        assert b"not finite" in hip._L.sph_last_error()
    with pytest.raises(sphmi.SphError, match="not finite"):
        hip.bin_diagnostics(g)
    hip.close()


def test_cpp_driver_bins(tmp_path):
    """sphmi_run --bin-grid ... --bin-out: the CSV's rows equal the Python call at the same steps; misuse exits with status 2."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    csv = str(tmp_path / "bins.csv")
    box = ["--box", "8", "8", "8", "--lattice", "12", "10", "12"]
    grid = ["-5.5", "0", "0", "5.5", "0", "6.75", "6", "1", "4"]
    args = [exe] + box + ["--steps", "4", "--bin-grid"] + grid + ["--bin-types", "1 3", "--bin-every", "2", "--bin-out", csv]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("_bins: step ") == 2
    steps, got = frames.read_bins(csv)
    assert steps.tolist() == [2, 4] and got.shape == (2, 24, 32)
    hip = scenes.hip_for(scenes.SCENES["tiny"]())  # the same box
    g = sphmi.bin_lattice((-5.5, 0, 0), (5.5, 0, 6.75), (6, 1, 4), (1, 3))
    k = 0
    for it in range(4):
        hip.step(it)
        if (it + 1) % 2 == 0:
            want = flat(hip, g)
            assert (want[:, 0] > 0).sum() > 12 and (want[:, 0] == 0).any()
            assert_records(got[k], want, "csv rows of step %d" % (it + 1))
            k += 1
    hip.close()
    for bad in (["--bin-grid"] + grid, ["--bin-out", csv], ["--bin-grid"] + grid + ["--bin-out", csv, "--bin-every", "0"],
                ["--bin-grid"] + grid[:6] + ["0", "1", "4", "--bin-out", csv], ["--bin-grid"] + grid[:6] + ["64", "64", "65", "--bin-out", csv]):
        r = subprocess.run([exe] + box + ["--steps", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip(), bad
