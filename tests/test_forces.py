"""GPU tests of the force decomposition (sph_force_measure / sph_force_diagnostics, include/sphmi.h): every word of both calls
bit-identical to the numpy restatement (tests/forces_ref.py, which tests/test_forces_host.py ties to the oracle's K7 and K12
stages), after the first step and after five more, on the fused and the staged path, on a scene whose tree has three levels;
consistent with the solver's own acceleration export and with the selection, read-only, the calling rules, and the driver's
line. No tolerance appears anywhere: integers are compared for equality, floats as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import diag_ref
import forces_ref as fr
import scenes
import sphmi
from sphmi import frames
from sphmi import slab as S
from scenes import staged_step

pytestmark = pytest.mark.gpu

ERR_ORDER = -3  # SPH_ERR_ORDER
ERR_INVALID = -1  # SPH_ERR_INVALID
f32 = np.float32
SCENE_NAMES = ["tiny", "tiny_compressed", "tiny_elastic", "config1", "worm"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scene(name):
    if name == "worm":
        return scenes.worm_scene()
    return scenes.config1() if name == "config1" else scenes.SCENES[name]()


def first_diff(got, want, view):
    d = np.argwhere(view(got) != view(want))
    return "%d words differ; first at %r: %r vs %r" % (d.shape[0], tuple(d[0]), got[tuple(d[0])], want[tuple(d[0])]) if d.size else "equal"


def regions_of(cfg, count):
    """`count` regions: everything, halves and octants of the box, an empty one (x0 >= x1), one outside the scene, slabs."""
    mid = [f32(0.5) * f32(getattr(cfg, a + "max")) for a in "xyz"]
    inf = np.inf
    out = [diag_ref.EVERYTHING, (-inf, -inf, -inf, mid[0], inf, inf), (mid[0], -inf, -inf, inf, inf, inf),
           (0, 0, 0, mid[0], mid[1], mid[2]), (mid[0], mid[1], mid[2], mid[0], inf, inf), (-9, -9, -9, -1, -1, -1),
           (-inf, mid[1], -inf, inf, inf, inf), (-inf, -inf, mid[2], inf, inf, inf)]
    k = 0
    while len(out) < count:
        lo = f32(cfg.ymax) * f32(k) / f32(8)
        out.append((-inf, lo, -inf, inf, lo + f32(cfg.ymax) / f32(8), inf))
        k += 1
    return np.array(out[:count], np.float32)


def check_against_restatement(hip, what, counts=(1, 16), types=(1, 2)):
    """Both calls on the solver's current state against the restatement; returns (state, Forces, records)."""
    cfg = hip.cfg
    state = fr.solver_state(hip)
    ids, dist = fr.neighbor_rows(hip)
    F = fr.Forces(state, ids, dist, fr.constants(cfg))
    rec = hip.force_measure()
    assert rec.dtype == np.float32 and rec.shape == (hip.N, 40)
    assert np.array_equal(u32(rec), u32(F.records)), "%s records: %s" % (what, first_diff(rec, F.records, u32))
    for count in counts:
        rg = regions_of(cfg, count)
        got = hip.force_diagnostics(rg, types)
        assert got.dtype == np.float64 and got.shape == (count, 64)
        want = fr.diag_records(state, F.records, rg, types)
        assert np.array_equal(u64(got), u64(want)), "%s totals of %d regions: %s" % (what, count, first_diff(got, want, u64))
        assert got[0, 0] == diag_ref.selected(state, diag_ref.EVERYTHING, types).sum()
        if count >= 6:
            assert not got[4].any() and not got[5].any() and got[0, 0] == got[1, 0] + got[2, 0]
    return state, F, rec


def check_against_acceleration(hip, state, rec):
    """Words 30..35 against the solver's own export wherever no elastic term was added."""
    N = hip.N
    acc = hip.buffer("acceleration").reshape(-1, 4)
    types = np.trunc(state["types"]).astype(int)
    liquid, moving = types == 1, types != 3
    assert liquid.any()
    assert np.array_equal(u32(rec[liquid, 30:33]), u32(acc[:N][liquid, :3])), first_diff(rec[liquid, 30:33], acc[:N][liquid, :3], u32)
    assert np.array_equal(u32(rec[moving, 33:36]), u32(acc[N:2 * N][moving, :3])), first_diff(rec[moving, 33:36], acc[N:2 * N][moving, :3], u32)
    assert not rec[~moving].any()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_calls_match_restatement(name):
    """After step 0 and after five more steps."""
    sc = _scene(name)
    hip = scenes.hip_for(sc)
    hip.step(0)
    state, F, rec = check_against_restatement(hip, "%s step 0" % name)
    check_against_acceleration(hip, state, rec)
    if name in ("tiny_compressed", "worm"):  # (tiny_compressed has relaxed to zero pressure by its sixth step)
        assert np.abs(rec[:, 33:36]).max() > 0
    for it in range(1, 6):
        hip.step(it)
    state, F, rec = check_against_restatement(hip, "%s step 5" % name, types=(1, 2, 3))
    check_against_acceleration(hip, state, rec)
    # nothing passes vacuously: the liquid exerts something everywhere, the records differ, the counts are the used slots
    assert np.abs(rec[:, 0:9]).max() > 0 and np.unique(rec[:, 31]).size > 2
    assert np.array_equal(rec[:, 27:30].sum(1), F.used_f.sum(1).astype(np.float32)) and rec[:, 27].max() > 1
    if sc["cfg"].numOfElasticP:
        elastic = np.trunc(state["types"]) == 2
        assert (rec[elastic, 27] > 0).any() and (rec[~elastic, 28] > 0).any() and np.abs(rec[:, 9:18]).max() > 0
    if name == "worm":
        assert np.abs(rec[:, 33:36]).max() > 0
    hip.close()


@pytest.mark.parametrize("name", ["tiny_compressed", "tiny_elastic"])
def test_staged_path(name):
    sc = _scene(name)
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    for it in range(3):
        a.step(it)
        staged_step(b, it)
    state, F, rec = check_against_restatement(b, "%s staged" % name)
    check_against_acceleration(b, state, rec)
    assert np.array_equal(u32(a.force_measure()), u32(rec))
    rg = regions_of(sc["cfg"], 3)
    assert np.array_equal(u64(a.force_diagnostics(rg)), u64(b.force_diagnostics(rg)))
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["tiny_elastic", "worm"])
def test_selection_variant(name, tmp_path):
    """force_measure(selection=True) after select(types=(2,)) is the rows of the full result at sortedIndex."""
    sc = _scene(name)
    hip = scenes.hip_for(sc)
    for it in range(2):
        hip.step(it)
    full = hip.force_measure()
    n = hip.select(types=(2,))
    assert n == sc["cfg"].numOfElasticP
    idx, ids, _ = hip.selection()
    got = hip.force_measure(selection=True)
    assert got.shape == (n, 40) and np.array_equal(u32(got), u32(full[idx]))
    assert np.abs(got[:, 0:9]).max() > 0  # the liquid loads the elastic matter
    # a selection that is not a contiguous run, and an empty one
    n2 = hip.select(types=(1, 2), terms=[("surface", 0.05, np.inf)])
    idx2 = hip.selection()[0]
    assert 0 < n2 < hip.N and np.array_equal(u32(hip.force_measure(selection=True)), u32(full[idx2]))
    assert hip.select(region=(-9, -9, -9, -1, -1, -1)) == 0 and hip.force_measure(selection=True).shape == (0, 40)
    # the selection's records name the same particles
    hip.select(types=(2,))
    pos = hip.read_position_buffer()
    path = os.path.join(str(tmp_path), "forces.vtk")
    m = np.float32(sc["cfg"].mass)
    assert frames.write_vtk_forces(path, pos, ids, got, mass=m) == n
    # 96 payload bytes per point: position 12, vertex cell 8, id 4, three counts 12, five vectors 60
    data = open(path, "rb").read()
    assert 96 * n < len(data) < 96 * n + 1024
    at = data.index(b"POINTS %d float\n" % n) + len(b"POINTS %d float\n" % n)
    assert np.array_equal(np.frombuffer(data[at:at + 12 * n], ">f4").reshape(n, 3), pos[ids.astype(np.int64), :3])
    at = data.index(b"VECTORS load_liquid float\n") + len(b"VECTORS load_liquid float\n")
    want = m * ((got[:, 0:3] + got[:, 6:9]) + got[:, 3:6])
    assert np.array_equal(u32(np.frombuffer(data[at:at + 12 * n], ">f4").astype(np.float32).reshape(n, 3)), u32(want))
    assert want.any()
    hip.close()


def test_three_tree_levels_on_more_than_a_million_particles():
    """More than 1024^2 particles: the third level of the tree runs and the records travel in several pieces. The
    pressure-active 1.3 M box of test_diagnostics.py."""
    sc = scenes.liquid_box((60.0, 40.0, 60.0), (125, 85, 125), spacing_in_r0=0.85, mask=0xffffffff)
    assert sc["cfg"].particleCount > 1024 * 1024
    hip = scenes.hip_for(sc)
    hip.step(0)
    hip.step(1)
    state, F, rec = check_against_restatement(hip, "1.3M step 1", counts=(2,), types=(1, 2, 3))
    assert diag_ref.selected(state, diag_ref.EVERYTHING, (1,)).sum() > 1024 * 1024 and np.abs(rec[:, 33:36]).max() > 0
    check_against_acceleration(hip, state, rec)
    hip.close()


BUFFERS = ["position", "velocity", "sortedPosition", "sortedVelocity", "acceleration", "neighborMap", "neighborIds",
           "particleIndex", "particleIndexBack", "gridCellIndex", "gridCellIndexFixedUp", "pressure", "rho"]


def test_calls_are_read_only():
    """Every exported buffer, a labelling, a selection and the following steps are unchanged by the two calls."""
    sc = scenes.SCENES["tiny_elastic"]()
    a, b = scenes.hip_for(sc), scenes.hip_for(sc)
    rg = regions_of(sc["cfg"], 5)
    for it in range(4):
        a.step(it)
        b.step(it)
        n_sel, C = a.label_components(np.inf, (1, 2))
        comp = a.components()
        assert a.select(None, (1, 2), [("surface", 0.05, np.inf)]) > 0
        sel = a.selection()
        before = {n: a.buffer(n) for n in BUFFERS}
        first = (a.force_measure(), a.force_measure(selection=True), a.force_diagnostics(rg))
        again = (a.force_measure(), a.force_measure(selection=True), a.force_diagnostics(rg))  # twice: the same arrays
        for x, y in zip(first, again):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        after = {n: a.buffer(n) for n in BUFFERS}
        for n in BUFFERS:
            assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
        for x, y in zip(comp, a.components()):  # the labelling is still valid
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for x, y in zip(sel, a.selection()):  # ... and the selection
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for get in ("read_position_buffer", "read_velocity_buffer", "read_density_buffer"):
        assert np.array_equal(getattr(a, get)().view(np.uint32), getattr(b, get)().view(np.uint32)), get
    a.close()
    b.close()


def _rc(hip, from_selection=0, regions=None, count=1, mask=0x6, n=None):
    out = np.empty((max(hip.N if n is None else n, 1), 40), np.float32)
    rg = np.array([diag_ref.EVERYTHING] * max(count, 1), np.float32) if regions is None else np.ascontiguousarray(regions, np.float32)
    tot = np.empty((max(count, 1), 64), np.float64)
    L, h = hip._L, hip._h
    return (L.sph_force_measure(h, from_selection, out.ctypes.data), L.sph_force_diagnostics(h, rg.ctypes.data, count, mask, tot.ctypes.data))


def test_calling_rules():
    sc = scenes.SCENES["tiny_elastic"]()
    hip = scenes.hip_for(sc)
    assert _rc(hip) == (ERR_ORDER, ERR_ORDER)  # before a step
    with pytest.raises(sphmi.SphError):
        hip.force_measure()
    with pytest.raises(sphmi.SphError):
        hip.force_diagnostics()
    hip.step(0)
    assert _rc(hip) == (0, 0)
    L, h = hip._L, hip._h
    assert _rc(hip, from_selection=1)[0] == ERR_ORDER  # no selection yet
    n = hip.select(types=(2,))
    assert _rc(hip, from_selection=1, n=n)[0] == 0
    for bad in (2, -1):
        assert _rc(hip, from_selection=bad)[0] == ERR_INVALID
    assert b"sph_force_measure" in L.sph_last_error()
    assert L.sph_force_measure(h, 0, None) == ERR_INVALID
    tot = np.empty((1, 64), np.float64)
    rg = np.array([diag_ref.EVERYTHING], np.float32)
    assert L.sph_force_diagnostics(h, None, 1, 0x6, tot.ctypes.data) == ERR_INVALID
    assert L.sph_force_diagnostics(h, rg.ctypes.data, 1, 0x6, None) == ERR_INVALID
    for mask in (0, 1, 0x10, 0x16):
        assert _rc(hip, mask=mask)[1] == ERR_INVALID
    for count in (0, -1, 17):
        assert _rc(hip, count=count)[1] == ERR_INVALID
    nan = np.array([diag_ref.EVERYTHING], np.float32)
    nan[0, 4] = np.nan
    assert _rc(hip, regions=nan)[1] == ERR_INVALID and b"sph_force_diagnostics" in L.sph_last_error()
    with pytest.raises(sphmi.SphError):
        hip.force_diagnostics(np.zeros((17, 6), np.float32))
    hip.step(1)  # a further step: the selection is of another state
    assert _rc(hip, from_selection=1, n=n)[0] == ERR_ORDER and _rc(hip) == (0, 0)
    with pytest.raises(sphmi.SphError):
        hip.force_measure(selection=True)
    for st in scenes.STAGE_SEQUENCE[:7]:  # a new step has begun: its density, force and pressure-force stages have not run yet
        getattr(hip, scenes.HIP_STAGE_METHOD[st])()
    assert _rc(hip) == (ERR_ORDER, ERR_ORDER)
    for st in scenes.STAGE_SEQUENCE[7:]:
        m = getattr(hip, scenes.HIP_STAGE_METHOD[st])
        m(2) if st == "integrate" else m()
    assert _rc(hip) == (0, 0)
    hip.close()


def test_slab_solver_is_invalid():
    sc = scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)
    cfg = sc["cfg"]
    n = cfg.particleCount
    hip = scenes.hip_for(sc)
    lay = S.particle_layers(sc["position"], cfg)
    hip.slab_init(S.make_slab([int(lay.min()), int(lay.max()) + 1], 0, 1, n), np.arange(n, dtype=np.uint32))
    hip.step(0)
    assert _rc(hip) == (ERR_INVALID, ERR_INVALID)
    hip.close()


def test_cpp_driver_forces():
    """sphmi_run --worm --muscles --forces-every 10 prints the liquid's load on the worm, the numbers of force_summary."""
    exe = os.path.join(scenes.PKG, "sphmi_run")
    r = subprocess.run([exe, "--worm", "--muscles", "--steps", "10", "--forces-every", "10", "--quiet"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("_forces: step")]
    assert len(lines) == 1 and "liquid on elastic (n 10143)" in lines[0], r.stdout
    got = [float(x) for x in lines[0].split("load")[1].split("N")[0].split()]
    sc = scenes.worm_scene()
    cfg = sc["cfg"]
    hip = scenes.hip_for(sc)
    for it in range(10):
        hip.step(it)
        hip.updateMuscleActivityData(sphmi.muscle_signal(it, cfg.muscleCount))  # the driver's order
    s = frames.force_summary(hip.force_diagnostics(types=(2,))[0], cfg.mass)
    assert s["n"] == 10143 and np.abs(s["hydrodynamic"]).max() > 0
    assert got == [float("%.9e" % x) for x in s["hydrodynamic"]]
    hip.close()
    r = subprocess.run([exe, "--box", "8", "8", "8", "--lattice", "12", "10", "12", "--steps", "4", "--forces-every", "2", "--quiet"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("_forces: step") == 2 and "boundary load" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, "--worm", "--steps", "1", "--forces-every", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip()
