"""Per-wave skipping in the predict-correct loop. The pressure-force kernel (K12) leaves out its neighbour loop in a wave
of 64 sorted particles whose pressure sums are all +0 and that holds no pair closer than hs / 4; the predicted-density kernel (K10)
of iterations >= 1 leaves out its own where no predicted position it would read changed a bit. Both are exact, so every case
compares position, velocity, density, pressure and the neighbour ids and distances (and the rest of the canonical buffers) with the
oracle bit for bit. The waves' decisions are read back ("pressureForceSkipped", "predictDensitySkipped": one byte per wave, 1 =
skipped, the last launch's) and compared with the set the oracle's own buffers give: a wave must serve K12 in full iff one of its
non-boundary particles has p != 0, has a valid neighbour in a wave that holds a p != 0, or has a valid neighbour closer than hs / 4."""
import numpy as np
import pytest

import scenes
from test_gpu_parity import FUSED_SKIP, assert_same, canon_hip, canon_ora

BOX, LATTICE = (20.0, 16.0, 40.0), (38, 30, 78)   # 102,400 particles; the column reaches its walls and becomes pressure-active
BOUNDARY = 3
_oracle = {}


def mixed_scene(spacing=0.93):
    return scenes.liquid_box(BOX, LATTICE, spacing_in_r0=spacing, mask=0xffffffff)


def close_pair_scene():
    """The mixed scene with the liquid particle of the largest x + y + z moved to 0.15 h from its nearest liquid neighbour, along
    the line that joins them."""
    sc = mixed_scene()
    nl = sc["numOfLiquidP"]
    pos = sc["position"]
    liq = pos[:nl, :3].astype(np.float64)
    i = int(np.argmax(liq.sum(1)))
    d2 = ((liq - liq[i]) ** 2).sum(1)
    d2[i] = np.inf
    j = int(np.argmin(d2))
    u = (liq[i] - liq[j]) / np.sqrt(d2[j])
    pos[i, :3] = (liq[j] + u * 0.15 * float(sc["cfg"].h)).astype(np.float32)
    return sc


def minus_zero_scene():
    sc = mixed_scene()
    sc["velocity"][0:sc["numOfLiquidP"]:2, :3] = np.float32(-0.0)
    return sc


BUILDERS = {"mixed": mixed_scene, "compressed": lambda: mixed_scene(0.85), "close_pair": close_pair_scene, "minus_zero": minus_zero_scene}


def build(name, max_iteration=None):
    sc = BUILDERS[name]()
    if max_iteration is not None:
        sc["cfg"].maxIteration = max_iteration
    return sc


def oracle_states(name, steps, max_iteration=None):
    """Canonical buffers of the oracle after each step named in `steps` (CPU only): computed once per scene, shared, never changed."""
    key = (name, max_iteration)
    have = _oracle.setdefault(key, {})
    if not all(s in have for s in steps):
        assert not have, "ask for the longest list of steps first: the oracle runs once per scene"
        sc = build(name, max_iteration)
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        for it in range(1, max(steps) + 1):
            ora.step()
            if it in steps:
                have[it] = canon_ora(ora, N)
        ora.close()
    return have


MIXED_STEPS = (1, 10, 20)


def close_radius(cfg):
    """hs / 4 as the double the reference compares the stored distance with (sphFluid.cl:1166)."""
    hs = np.float32(cfg.h) * np.float32(cfg.simulationScale)
    return 0.5 * float(hs / np.float32(2))


def wave_sets(canon, cfg):
    """From the buffers a step left, per wave of 64 sorted particles: (holds a non-boundary particle, K12's last launch must serve
    it in full), and per sorted particle whether it is a non-boundary particle with a valid neighbour closer than hs / 4."""
    return _wave_sets(canon, cfg)[:3]


def _wave_sets(canon, cfg):
    N = cfg.particleCount
    pi = canon["particleIndex"].reshape(-1, 2)[:, 1].astype(np.int64)
    liquid = canon["position"][:, 3].astype(np.int32)[pi] != BOUNDARY  # by sorted id
    p = canon["pressure"][:N]
    ids = canon["neighborIds"].reshape(N, 32).astype(np.int64)
    dist = canon["neighborDist"].reshape(N, 32)
    W = (N + 63) // 64
    wave = np.arange(N) >> 6
    holds_p = np.bincount(wave, weights=(p != 0), minlength=W) > 0   # (!=: a NaN counts)
    valid = ids >= 0
    near_p = (valid & holds_p[np.clip(ids, 0, N - 1) >> 6]).any(1)
    close = liquid & (valid & (dist.astype(np.float64) < close_radius(cfg))).any(1)
    live = liquid & ((p != 0) | near_p) | close
    flagged = holds_p | (np.bincount(wave, weights=close, minlength=W) > 0)   # pBlk | cBlk set
    return np.bincount(wave, weights=liquid, minlength=W) > 0, np.bincount(wave, weights=live, minlength=W) > 0, close, flagged


def assert_k12_decisions(hip, canon, cfg, where):
    """No wave that must serve K12 in full skipped. Where no wave at all holds a pressure or a close pair, the launch-level gate in
    front of K12 is open whatever it samples, and the skipped waves are exactly those that may skip. Elsewhere the kernel is knowingly
    more conservative (a launch whose gate is closed consults nothing), so only the subset relation is asserted: results never depend
    on the gate, and this test does not restate it."""
    has_liquid, full, _, flagged = _wave_sets(canon, cfg)
    skipped = hip.buffer("pressureForceSkipped") != 0
    assert not (skipped & full).any(), "%s: a wave that must serve K12 in full skipped" % where
    if not flagged.any():
        assert np.array_equal(skipped, ~full), "%s: %d waves skipped, %d may" % (where, skipped.sum(), (~full).sum())


@pytest.mark.gpu
def test_mixed_state():
    sc = mixed_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    assert N == 102400
    want = oracle_states("mixed", MIXED_STEPS)
    has_liquid, full, close = wave_sets(want[20], cfg)
    share = full[has_liquid].mean()
    print("step 20: %.3f of the waves with liquid need K12 in full; %d particles have a neighbour closer than hs/4" % (share, close.sum()))
    assert 0.2 <= share <= 0.8
    assert close.sum() >= 1
    hip = scenes.hip_for(sc)
    for it in range(1, 21):
        hip.step(it - 1)
        if it in MIXED_STEPS:
            assert_same(canon_hip(hip, N), want[it], "mixed state, step %d" % it, FUSED_SKIP)
            assert_k12_decisions(hip, want[it], cfg, "step %d" % it)
    hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [3, 2])
def test_nothing_to_do(iterations):
    """Step 1: no pressure, no close pair. A byte holds the decision of the kernel's last launch: with three iterations that is K10 of
    iteration 2, with two K10 of iteration 1 (the same launch, on the same inputs, as iteration 1 of three)."""
    sc = build("mixed", iterations)
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states("mixed", MIXED_STEPS)[1] if iterations == 3 else oracle_states("mixed", (1,), iterations)[1]
    assert want["pressure"].max() == 0
    has_liquid, full, close = wave_sets(want, cfg)
    assert not full.any() and not close.any()
    hip = scenes.hip_for(sc)
    hip.step(0)
    assert_same(canon_hip(hip, N), want, "step 1, %d iterations" % iterations, FUSED_SKIP)
    assert (hip.buffer("pressureForceSkipped")[has_liquid] == 1).all()
    assert (hip.buffer("predictDensitySkipped")[has_liquid] == 1).all()
    hip.close()


@pytest.mark.gpu
def test_nothing_to_skip():
    sc = build("compressed")
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states("compressed", (1, 3))
    has_liquid, full, _ = wave_sets(want[1], cfg)
    print("step 1: %.3f of the waves with liquid need K12 in full" % full[has_liquid].mean())
    assert full[has_liquid].mean() >= 0.9
    hip = scenes.hip_for(sc)
    for it in (1, 2, 3):
        hip.step(it - 1)
        if it in want:
            assert_same(canon_hip(hip, N), want[it], "0.85 r0, step %d" % it, FUSED_SKIP)
            assert_k12_decisions(hip, want[it], cfg, "0.85 r0, step %d" % it)
    hip.close()


@pytest.mark.gpu
def test_close_pair_without_pressure():
    """The pair's term is -(hs/4 - r)^2 * 0.5 * rho0 * delta / rho*_j whatever the pressures are: a wave that judged by pressure
    alone would drop it."""
    sc = build("close_pair")
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states("close_pair", (1, 2, 3))
    hip = scenes.hip_for(sc)
    for it in (1, 2, 3):
        hip.step(it - 1)
        assert want[it]["pressure"].max() == 0
        _, full, close = wave_sets(want[it], cfg)
        assert close.sum() == 2, "step %d" % it
        assert_same(canon_hip(hip, N), want[it], "close pair, step %d" % it, FUSED_SKIP)
        assert_k12_decisions(hip, want[it], cfg, "close pair, step %d" % it)
        assert (hip.buffer("pressureForceSkipped")[np.flatnonzero(close) >> 6] == 0).all()
    hip.close()


@pytest.mark.gpu
def test_signs_of_zero():
    sc = build("minus_zero")
    N = sc["cfg"].particleCount
    want = oracle_states("minus_zero", (3,))
    hip = scenes.hip_for(sc)
    for it in range(3):
        hip.step(it)
    assert_same(canon_hip(hip, N), want[3], "every second liquid velocity -0.0, step 3", FUSED_SKIP)
    hip.close()


def _serial_timed(hip):
    hip.set_stage_timing(True)


def _chunks(chunks, depth=None):
    def setup(hip):
        hip.set_step_chunks(chunks)
        if depth is not None:
            hip.set_step_pipeline(depth)
    return setup


# (name, setup, the per-wave flags are in use)
PATHS = [("serial with stage timing", _serial_timed, True), ("2 chunks", _chunks(2), True), ("16 chunks", _chunks(16), True),
         ("2 chunks, pipeline depth 1", _chunks(2, 1), True), ("2 chunks, pipeline depth 3", _chunks(2, 3), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,setup,flags", PATHS, ids=[p[0] for p in PATHS])
def test_paths(name, setup, flags):
    """Ten steps of the mixed scene by every path the fused step has. All are compared with the oracle, and so with each other."""
    sc = mixed_scene()
    cfg = sc["cfg"]
    N = cfg.particleCount
    want = oracle_states("mixed", MIXED_STEPS)[10]
    hip = scenes.hip_for(sc)
    setup(hip)
    before = hip.buffer("pressureForceSkipped").copy()
    for it in range(10):
        hip.step(it)
    assert_same(canon_hip(hip, N), want, "%s, step 10" % name, FUSED_SKIP)
    if flags:
        assert_k12_decisions(hip, want, cfg, name)
    else:  # depth 3 runs without the flags: nothing wrote a decision
        assert np.array_equal(hip.buffer("pressureForceSkipped"), before)
    hip.close()
