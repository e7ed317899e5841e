"""CPU tests of the force-decomposition restatement (tests/forces_ref.py), the yardstick the GPU calls are held to
(tests/test_forces.py): hand-made neighbourhoods with exact answers, the tie to the oracle's K7 and K12 stages bit for bit, the
replay of the elastic-force stage on top of it, the class sums against the step's own sum, the properties of the fixed tree and
the host-side helpers of sphmi.frames.

Steps before the examined one, chosen so that nothing passes vacuously: the resting lattice of `tiny` needs about 200 steps
before its outer layer comes within h of the boundary shell, `tiny_compressed` 4 (one more and its pressure has relaxed to
zero), `tiny_elastic` 20. The worm's matter does not come within h of the shell in its first 60 steps (probed with the oracle),
so on the worm the classes met are liquid and elastic; all three classes are asserted on `tiny_elastic`."""
import functools
import os

import numpy as np
import pytest

import diag_ref
import elastic_ref as er
import forces_ref as fr
import scenes
import sphmi
from sphmi import frames

f32 = np.float32
SCENE_STEPS = {"tiny": 200, "tiny_compressed": 4, "tiny_elastic": 20, "worm": 1}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. hand-made neighbourhoods --------------------------------------------------------------------------------------------
HAND_CFG = dict(mass=1.0, viscosity=1.0, h=8.0, simulationScale=1.0, rho0=4.0, delta=0.5, del2WviscosityCoefficient=4.0,
                gradWspikyCoefficient=2.0, surfTensCoeff=0.5, gravity_x=0.0, gravity_y=-8.0, gravity_z=0.0)


def hand_made():
    """Seven particles on integer coordinates at simulationScale 1, hs = 8, h/4 = closeRf = 2. Particle 0 (liquid) has one
    neighbour per class, an empty slot, a slot beyond hs and a liquid neighbour closer than h/4; particle 3 is a boundary
    particle with a neighbour; particle 6 has an empty row."""
    #               0 liquid    1 liquid   2 elastic  3 boundary  4 liquid   5 liquid   6 liquid
    pos = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, -2], [9, 0, 0], [0, 0, 1], [20, 20, 20]], np.float32)
    vel = np.array([[1, 0, 0], [3, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [1, 2, 0], [0, 0, 0]], np.float32)  # 3: the wall normal
    types = np.array([1.1, 1.1, 2.1, 3.1, 1.1, 1.1, 1.1], np.float32)
    rho = np.array([2, 2, 4, 1, 2, 1, 2], np.float32)
    rho_star = np.array([4, 2, 4, 1, 2, 0.5, 2], np.float32)
    p = np.array([8, 8, 0, 0, 8, 3, 0], np.float32)
    ids = -np.ones((7, 32), np.int32)
    dist = -np.ones((7, 32), np.float32)
    for k, (j, r) in enumerate([(1, 4), (-1, -1), (2, 3), (3, 2), (4, 9), (5, 1)]):
        ids[0, k], dist[0, k] = j, r
    ids[3, 0], dist[3, 0] = 0, 2
    state = dict(pos=pos, vel=vel, rho=rho, rhoStar=rho_star, p=p, types=types, keys=np.zeros(7, np.uint32), G=1)
    return state, ids, dist


def test_constants_follow_sph_create():
    K = fr.constants(HAND_CFG)
    assert (K["hs"], K["hq"], K["closeRf"], K["massMu"], K["rho0delta"], K["del2W"], K["massGradW"]) == (8, 2, 2, 1, 2, 4.0, 2.0)
    cfg = sphmi.default_config()
    K = fr.constants(cfg)
    hs = f32(f32(cfg.h) * f32(cfg.simulationScale))
    assert K["hs"] == hs and float(K["closeRf"]) >= 0.5 * float(f32(hs / f32(2))) > float(np.nextafter(K["closeRf"], f32(-np.inf)))
    assert K["massMu"] == f32(f32(cfg.mass) * f32(cfg.viscosity)) and K["massGradW"] == float(cfg.mass) * cfg.gradWspikyCoefficient
    assert fr.constants(sphmi.config_dict(cfg))["closeRf"] == K["closeRf"]


def test_hand_made_neighbourhoods_have_exact_answers():
    state, ids, dist = hand_made()
    F = fr.Forces(state, ids, dist, fr.constants(HAND_CFG))
    rec = F.records
    assert rec.shape == (7, 40) and rec.dtype == np.float32
    # sF = massMu * (float)(del2W / rho_0) = 2, sP = (float)(massGradW / rhoStar_0) = 0.5
    # liquid: slot 0 (r = 4): tv = ((3-1)*(8-4))/2, tt = 0.5*(0-4), num = -(4*4)*0.5*(8+8) = -128, value = -64, tq = (-64*-4)/4
    #         slot 5 (r = 1 < h/4): tv_y = ((2-0)*(8-1))/1, tt_z = 0.5*(0-1), num = -((2-1)*(2-1))*0.5*2 = -1, value = -1/0.5, tq_z = (-2*-1)/1
    assert rec[0, 0:9].tolist() == [8, 28, 0, -2, 0, -0.5, 32, 0, 1]
    # elastic: slot 2 (r = 3): tv = ((0-1)*5)/4, ((1-0)*5)/4; tt_y = 0.5*(0-3); num = -(5*5)*0.5*(8+0) = -100, value = -25, tq_y = (-25*-3)/3
    assert rec[0, 9:18].tolist() == [-2.5, 2.5, 0, 0, -1.5, 0, 0, 12.5, 0]
    # boundary: slot 3 (r = 2, not < 2): v_j is the wall normal (0, 0, 1): tv = ((0-1)*6)/1, 0, ((1-0)*6)/1; tt_z = 0.5*(0+2);
    #           num = -(6*6)*0.5*8 = -144, value = -144, tq_z = (-144*2)/2
    assert rec[0, 18:27].tolist() == [-12, 0, 12, 0, 0, 1, 0, 0, -72]
    assert rec[0, 27:30].tolist() == [2, 1, 1]  # the slot beyond hs (r = 9) and the empty slot count nowhere
    # aF = V*sF + g + T with V = (4 - 1.25 - 6, 1.25 + 14, 6), T = (-2, -1.5, 1 - 0.5); aP = P*sP with P = (64, 25, -144 + 2)
    assert rec[0, 30:36].tolist() == [-8.5, 21, 12.5, 32, 12.5, -71] and not rec[0, 36:].any()
    assert F.S[0, :, 0].tolist() == [-3.25, 15.25, 6, -2, -1.5, 0.5, 64, 25, -142]
    assert F.used_f[0, :6].tolist() == [True, False, True, True, False, True] and not F.used_f[0, 6:].any()
    # a boundary particle: all zero although its row has a neighbour in reach; an empty row: gravity alone
    assert not rec[3].any() and not F.used_f[3].any()
    assert rec[6, 30:33].tolist() == [0, -8, 0] and not rec[6, :30].any() and not rec[6, 33:].any()
    for i in (1, 2, 4, 5):
        assert rec[i, 30:33].tolist() == [0, -8, 0]
    # totals over everything but the boundary, and the helpers: h_1 = (visc + pres) + tens = (38, 28, 0.5) at x = 0: no torque
    d = fr.diag_records(state, rec, [diag_ref.EVERYTHING, (0, 0, 0, 1, 1, 1), (50, 50, 50, 60, 60, 60)], (1, 2))
    assert d.shape == (3, 64) and d[0, 0] == 6 and d[1, 0] == 1 and d[2, 0] == 0 and not d[2].any() and not d[:, 49:].any()
    assert d[1, 1:28].tolist() == rec[0, :27].tolist() and d[1, 28:34].tolist() == rec[0, 30:36].tolist()
    assert d[0, 29] == 21 - 8 * 5 and d[1, 34:43].tolist() == [0] * 9 and d[1, 46:49].tolist() == [2, 1, 1]
    # power: w_c = h_c . v_0 with v_0 = (1, 0, 0)
    assert d[1, 43:46].tolist() == [(8 + 32) - 2, -2.5, -12]
    # torque with the particle off the origin
    state["pos"] = state["pos"] + f32(1)
    d2 = fr.diag_records(state, rec, [diag_ref.EVERYTHING], (1, 2, 3))
    hx, hy, hz = 38.0, 28.0, 0.5
    assert d2[0, 0] == 7 and d2[0, 34:37].tolist() == [hz - hy, hx - hz, hy - hx]


# ---- 2.-5. the tie to the oracle ------------------------------------------------------------------------------------------------
def _scene(name):
    return scenes.worm_scene() if name == "worm" else scenes.SCENES[name]()


def _signal(name, cfg):
    if name == "worm":
        return sphmi.muscle_signal(100, cfg.muscleCount)
    s = np.zeros(cfg.muscleCount, np.float32)
    s[0] = f32(0.75)
    return s


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle driven stage by stage through the examined step: the acceleration right after K7, after K8 and the pressure
    acceleration after the last K12, and the restatement on the state the oracle then holds."""
    sc = _scene(name)
    cfg = sc["cfg"]
    N = cfg.particleCount
    ora = scenes.oracle_for(sc)
    signal = _signal(name, cfg)
    if cfg.numOfElasticP:
        ora.update_muscles(signal)
    for _ in range(SCENE_STEPS[name]):
        ora.step()
    seq = scenes.STAGE_SEQUENCE
    k7 = seq.index("computeForcesAndInitPressure")
    last12 = len(seq) - 1 - seq[::-1].index("computePressureForceAcceleration")
    for st in seq[:k7 + 1]:
        ora.run(st)
    after7 = ora.buffer("acceleration").reshape(-1, 4)[:N, :3].copy()
    ora.run(seq[k7 + 1])
    assert seq[k7 + 1] == "computeElasticForces"
    after8 = ora.buffer("acceleration").reshape(-1, 4)[:N, :3].copy()
    for st in seq[k7 + 2:last12 + 1]:
        ora.run(st)
    pressure = ora.buffer("acceleration").reshape(-1, 4)[N:2 * N, :3].copy()
    state, ids, dist = fr.oracle_state(ora, N, cfg.gridCellCount)
    back = ora.buffer("particleIndexBack")[:N].copy()
    ora.close()
    F = fr.Forces(state, ids, dist, fr.constants(cfg))
    return dict(sc=sc, cfg=cfg, N=N, state=state, ids=ids, dist=dist, F=F, after7=after7, after8=after8, pressure=pressure,
                back=back, signal=signal)


@pytest.mark.parametrize("name", list(SCENE_STEPS))
def test_words_30_to_35_are_the_oracles_k7_and_k12(name):
    """Words 30..32 equal the oracle's acceleration right after K7 and words 33..35 its pressure acceleration after the last
    K12, bit for bit, for every non-boundary particle, elastic ones included."""
    c = oracle_case(name)
    F, mv = c["F"], c["F"].moving
    assert mv.sum() > 0 and (~mv).sum() > 0
    assert scenes.bits_equal(F.records[mv, 30:33], c["after7"][mv]), scenes.diff_report(F.records[mv, 30:33], c["after7"][mv])
    assert scenes.bits_equal(F.records[mv, 33:36], c["pressure"][mv]), scenes.diff_report(F.records[mv, 33:36], c["pressure"][mv])
    assert not F.records[~mv].any() and not c["after7"][~mv].any() and not c["pressure"][~mv].any()
    if c["cfg"].numOfElasticP:
        assert (np.trunc(c["state"]["types"]) == 2).sum() == c["cfg"].numOfElasticP


@pytest.mark.parametrize("name", ["tiny_elastic", "worm"])
def test_replay_of_the_elastic_stage(name):
    """Word 30..32 plus elastic_ref's per-slot spring and contraction terms, in k_elastic's order, is the oracle's acceleration
    after K8, bit for bit."""
    c = oracle_case(name)
    cfg = c["cfg"]
    con = er.Connections(c["state"]["pos"], c["back"], c["sc"]["elastic"], cfg.elasticOffset, cfg.simulationScale, cfg.muscleCount,
                         c["signal"])
    assert not con.bad and con.has_s.any() and con.has_c.any()
    acc = c["F"].records[:, 30:33].copy()
    rows = con.owner
    assert np.unique(rows).size == rows.size
    for k in range(32):  # per slot: the spring term, then the contraction term (the stage's order)
        for has, term in ((con.has_s[:, k], con.s[:, k]), (con.has_c[:, k], con.c[:, k])):
            acc[rows[has]] = (acc[rows[has]] + term[has]).astype(np.float32)
    mv = c["F"].moving
    assert scenes.bits_equal(acc[mv], c["after8"][mv]), scenes.diff_report(acc[mv], c["after8"][mv])
    assert not scenes.bits_equal(c["after7"], c["after8"])


@pytest.mark.parametrize("name", list(SCENE_STEPS))
def test_class_sums_against_the_steps_sum(name):
    """One class among the used slots: that class's sum IS the step's sum. Otherwise |sum_c S_c - S| <= 2^-18 * sum|t| per
    component: each sequential float sum of at most 32 terms errs by at most 31 * 2^-24 * sum|t| to first order and two such
    sums are compared, so 64 * 2^-24 covers it (derived, not measured)."""
    c = oracle_case(name)
    F = c["F"]
    S, A = F.S, F.A
    worst = 0.0
    for lo, hi, used in ((0, 6, F.used_f), (6, 9, F.used_p)):
        n_c = np.stack([(used & (F.cls == k)).sum(1) for k in fr.CLASSES])
        single = ((n_c > 0).sum(0) == 1) & F.moving
        mixed = ((n_c > 0).sum(0) >= 2) & F.moving
        assert single.any()
        which = n_c.argmax(0) + 1
        for q in range(lo, hi):
            own = S[which, q, np.arange(S.shape[2])]
            assert np.array_equal(u32(own[single]), u32(S[0, q][single])), (name, q)
            others = S[1:, q].astype(np.float64).sum(0) - own.astype(np.float64)
            assert not others[single].any()
            diff = np.abs(S[1:, q].astype(np.float64).sum(0) - S[0, q].astype(np.float64))
            bound = 2.0 ** -18 * A[q]
            assert (diff[mixed] <= bound[mixed]).all(), (name, q, float((diff[mixed] - bound[mixed]).max()))
            if mixed.any() and (bound[mixed] > 0).any():
                worst = max(worst, float((diff[mixed][bound[mixed] > 0] / bound[mixed][bound[mixed] > 0]).max()))
        # particles without a used slot: every sum is +0
        none = ((n_c > 0).sum(0) == 0)
        assert not S[:, lo:hi][:, :, none].any()
    print("%s: largest |sum_c S_c - S| / (2^-18 sum|t|) = %.3g" % (name, worst))


@pytest.mark.parametrize("name", list(SCENE_STEPS))
def test_nothing_passes_vacuously(name):
    c = oracle_case(name)
    F, rec = c["F"], c["F"].records
    types = np.trunc(c["state"]["types"]).astype(int)
    n = rec[:, 27:30]
    classes = (n > 0).sum(1)
    met = [int((n[:, k] > 0).sum()) for k in range(3)]
    print("%s after %d steps: particles with used neighbours of class 1, 2, 3: %s; of two or more classes: %d; of one: %d; "
          "max |aP| %.6g" % (name, SCENE_STEPS[name], met, int((classes >= 2).sum()), int((classes == 1).sum()),
                             float(np.abs(rec[:, 33:36]).max())))
    assert (classes >= 2).any() and (classes == 1).any()
    if name in ("tiny", "tiny_compressed"):
        assert met[0] > 0 and met[2] > 0 and met[1] == 0  # the liquid has reached the boundary shell
    if name == "tiny_elastic":
        assert min(met) > 0 and (classes == 3).any()  # all three classes
    if name == "tiny_compressed":
        assert np.abs(rec[:, 33:36]).max() > 0 and np.abs(F.S[0, 6:9]).max() > 0
    if name == "worm":
        elastic = types == 2
        assert elastic.sum() == c["cfg"].numOfElasticP and (n[elastic, 0] > 0).sum() > 1000  # the liquid loads the cuticle
        assert met[0] > 0 and met[1] > 0
    # K7 and K12 use the same slots except where the stored and the recomputed distance straddle hs
    assert (F.used_f == F.used_p).mean() > 0.999


# ---- 6. tree properties -----------------------------------------------------------------------------------------------------
def test_a_record_does_not_depend_on_the_other_regions():
    c = oracle_case("tiny_elastic")
    state, rec, cfg = c["state"], c["F"].records, c["cfg"]
    mid = [f32(0.5) * f32(getattr(cfg, a + "max")) for a in "xyz"]
    regions = [diag_ref.EVERYTHING, (-np.inf, -np.inf, -np.inf, mid[0], np.inf, np.inf), (mid[0], -np.inf, -np.inf, np.inf, np.inf, np.inf),
               (0, 0, 0, mid[0], mid[1], mid[2]), (5, 5, 5, 5, 6, 6), (-5, -5, -5, -1, -1, -1)]
    full = fr.diag_records(state, rec, regions, (1, 2))
    for r, region in enumerate(regions):
        alone = fr.diag_records(state, rec, [region], (1, 2))
        assert np.array_equal(u64(alone[0]), u64(full[r])), r
        assert full[r, 0] == diag_ref.record(state, region, (1, 2), cfg.rho0)[0]
    assert full[0, 0] == full[1, 0] + full[2, 0] > 0 and not full[4].any() and not full[5].any()
    # the tree's sums are the exactly rounded sums here, so the two halves add up to the whole to rounding
    assert np.allclose(full[1, 1:49] + full[2, 1:49], full[0, 1:49], rtol=1e-12, atol=1e-6)
    # every type: the boundary's all-zero records change the count and nothing else
    every = fr.diag_records(state, rec, [diag_ref.EVERYTHING], (1, 2, 3))
    assert every[0, 0] == cfg.particleCount and np.allclose(every[0, 1:49], full[0, 1:49], rtol=1e-12, atol=1e-9)
    # the liquid's pressure push on the elastic matter and the elastic matter's on the liquid: opposite in sign, equal only
    # approximately (the term divides by rhoStar_j)
    on_elastic = fr.diag_records(state, rec, [diag_ref.EVERYTHING], (2,))[0]
    on_liquid = fr.diag_records(state, rec, [diag_ref.EVERYTHING], (1,))[0]
    a, b = on_elastic[7:10], on_liquid[16:19]  # class 1 pressure on type 2; class 2 pressure on type 1
    assert np.abs(a).max() > 0 and np.abs(a + b).max() < 0.5 * np.abs(a).max()


# ---- 7. frames ----------------------------------------------------------------------------------------------------------------
def test_frames_force_summary_and_vtk(tmp_path):
    assert len(frames.FORCE_FIELDS) == fr.WORDS == sphmi.FORCE_WORDS == 40
    assert len(frames.FORCE_DIAG_FIELDS) == fr.DIAG_WORDS == sphmi.FORCE_DIAG_WORDS == 64
    assert frames.FORCE_FIELDS[0] == "liquid_viscous_x" and frames.FORCE_FIELDS[17] == "elastic_pressure_z" and frames.FORCE_FIELDS[27] == "n_liquid"
    assert frames.FORCE_DIAG_FIELDS[28] == "sum_step_x" and frames.FORCE_DIAG_FIELDS[34] == "sum_torque_liquid_x"
    assert frames.FORCE_DIAG_FIELDS[45] == "sum_power_boundary" and frames.FORCE_DIAG_FIELDS[48] == "sum_n_boundary"
    for name in ("sph_force_measure", "sph_force_diagnostics"):
        assert name in sphmi.EXPORTED_SYMBOLS
    txt = open(os.path.join(scenes.ROOT, "include", "sphmi.h")).read()
    assert "#define SPH_FORCE_WORDS 40" in txt and "#define SPH_FORCE_DIAG_WORDS 64" in txt and "#define SPHMI_ABI_VERSION 2" in txt
    state, ids, dist = hand_made()
    rec = fr.Forces(state, ids, dist, fr.constants(HAND_CFG)).records
    d = fr.diag_records(state, rec, [(0, 0, 0, 1, 1, 1)], (1, 2))[0]
    s = frames.force_summary(d, 0.25)
    assert s["n"] == 1
    assert s["viscous"].tolist() == [[2, 7, 0], [-0.625, 0.625, 0], [-3, 0, 3]]
    assert s["tension"].tolist() == [[-0.5, 0, -0.125], [0, -0.375, 0], [0, 0, 0.25]]
    assert s["pressure"].tolist() == [[8, 0, 0.25], [0, 3.125, 0], [0, 0, -18]]
    assert s["load"].tolist() == [[9.5, 7, 0.125], [-0.625, 3.375, 0], [-3, 0, -14.75]]
    assert s["hydrodynamic"].tolist() == [9.5, 7, 0.125] and s["neighbors"].tolist() == [2, 1, 1]
    assert s["power"].tolist() == [9.5, -0.625, -3] and not s["torque"].any()
    assert s["step"].tolist() == [0.25 * (-8.5 + 32), 0.25 * (21 + 12.5), 0.25 * (12.5 - 71)]
    p4 = np.concatenate([state["pos"], state["types"][:, None]], axis=1)
    vtk = os.path.join(str(tmp_path), "forces.vtk")
    assert frames.write_vtk_forces(vtk, p4, np.arange(7, dtype=np.uint32), rec, mass=0.25) == 7
    data = open(vtk, "rb").read()
    assert data.startswith(b"# vtk DataFile") and b"VECTORS load_liquid float" in data and b"VECTORS load_boundary float" in data
    assert b"SCALARS neighbors_elastic float 1" in data and b"VECTORS step float" in data
    at = data.index(b"VECTORS load_liquid float\n") + len(b"VECTORS load_liquid float\n")
    assert np.frombuffer(data[at:at + 12], ">f4").tolist() == [9.5, 7, 0.125]
    with pytest.raises(ValueError):
        frames.write_vtk_forces(vtk, p4, np.arange(6, dtype=np.uint32), rec)
