"""The scenes and gauges the flow-gauge tests share (tests/test_gauge_host.py on the oracle, tests/test_gauge.py on the GPU). Inputs
only. The committed scenes at rest move about 2e-4 r0 per step and cross nothing, so a case gives every particle of its types
the velocity +-0.25 per axis (about 0.33 r0 per step), the three signs from bits 16, 17, 18 of id * 2654435761: neighbours
move against each other, and from the second step on every gauge sees both directions. The gauges stand 0.1 r0 behind the median
liquid coordinate: a plane midway between two lattice columns would see nothing in the first steps."""
import functools

import numpy as np

import gauge_ref as gr
import scenes

f32 = np.float32
STEPS = 6  # steps per case: the records of every one are compared, the crossing counts are asserted over all of them
SPEED = 0.25
# name -> (scene, types that are seeded and gauged)
CASES = {"tiny": ("tiny", (1,)), "tiny_jitter": ("tiny_jitter", (1,)), "elastic": ("tiny_elastic", (1, 2))}
SINGLE = (3,)              # the slots of the one-gauge runs
SPREAD = (0, 5, 7, 15)     # ... of the runs with gauges in non-adjacent slots


def seeded(sc, types=(1,), speed=SPEED):
    """The scene with velocity (+-speed, +-speed, +-speed) on the particles of `types`."""
    sc = dict(sc)
    pos, vel = sc["position"], np.array(sc["velocity"], np.float32)
    h = (np.arange(pos.shape[0], dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)
    on = np.isin(pos[:, 3].astype(np.int32), types)
    for c in range(3):
        sign = np.where((h >> np.uint64(16 + c)) & np.uint64(1), f32(1), f32(-1))
        vel[on, c] = (sign * f32(speed))[on]
    sc["velocity"] = vel
    return sc


def _plane(c, at, types, flip=False):
    e = np.eye(3, dtype=np.float32)
    o = np.zeros(3, np.float32)
    o[c] = at
    u, v = e[(c + 1) % 3], e[(c + 2) % 3]
    return dict(origin=o, u=v if flip else u, v=u if flip else v, types=types, plane=True)


def _rect(c, at, lo, size, types):
    """Axis-aligned rectangle in the plane coordinate c = at, from lo (two numbers, axes c+1, c+2) over size."""
    e = np.eye(3, dtype=np.float32)
    o = np.zeros(3, np.float32)
    o[c], o[(c + 1) % 3], o[(c + 2) % 3] = at, lo[0], lo[1]
    return dict(origin=o, u=e[(c + 1) % 3] * f32(size[0]), v=e[(c + 2) % 3] * f32(size[1]), types=types)


def gauges_of(sc, types):
    """{slot: gauge} for all 16 slots, from the scene's liquid: planes along the three axes (slot 3 is slot 0 turned round), an
    axis-aligned rectangle (4) and the two halves that tile it (5, 6), a tilted parallelogram whose u and v are neither
    axis-aligned nor orthogonal (7) and its whole plane (8), rectangles across y and z (9, 10), shifted and diagonal planes."""
    pos = sc["position"]
    liq = pos[pos[:, 3].astype(np.int32) == 1][:, :3]
    r0 = f32(sc["cfg"].r0)
    lo, hi = liq.min(0), liq.max(0)
    mid = np.array([np.sort(liq[:, c])[liq.shape[0] // 2] + f32(0.1) * r0 for c in range(3)], np.float32)
    ext = (hi - lo).astype(np.float32)
    g = {0: _plane(0, mid[0], types), 1: _plane(1, mid[1], types), 2: _plane(2, mid[2], types), 3: _plane(0, mid[0], types, flip=True)}
    size = np.array([ext[1] + r0, f32(0.625) * ext[2]], np.float32)  # the whole height (halved below), five eighths of the depth
    g[4] = _rect(0, mid[0], (lo[1] - r0, lo[2] - r0), size, types)
    g[5] = dict(g[4], u=g[4]["u"] * f32(0.5))
    g[6] = dict(g[5], origin=g[4]["origin"] + g[5]["u"])
    centre = (f32(0.5) * (lo + hi)).astype(np.float32)
    centre[0] = mid[0]
    u = np.array([0.3, 1.0, 0.2], np.float32) * f32(0.7) * ext[1]
    v = np.array([-0.2, 0.3, 1.0], np.float32) * f32(0.6) * ext[2]
    g[7] = dict(origin=(centre - f32(0.5) * u - f32(0.5) * v).astype(np.float32), u=u, v=v, types=types)
    g[8] = dict(g[7], plane=True)
    g[9] = _rect(1, mid[1], (lo[2] - r0, lo[0] - r0), (f32(0.8) * ext[2], f32(0.8) * ext[0]), types)
    g[10] = _rect(2, mid[2], (lo[0] + f32(0.2) * ext[0], lo[1] - r0), (f32(0.5) * ext[0], f32(0.8) * ext[1]), types)
    g[11] = _plane(0, mid[0] + f32(0.93) * r0, types)
    g[12] = _plane(1, mid[1] - f32(0.93) * r0, types, flip=True)
    g[13] = _plane(2, mid[2] - f32(1.86) * r0, types)
    g[14] = dict(origin=centre, u=np.array([1, -1, 0], np.float32), v=np.array([0, 0, 1], np.float32), types=types, plane=True)
    g[15] = dict(origin=centre, u=np.array([0, 1, -1], np.float32) * f32(0.7) * ext[1], v=np.array([1, 0.25, 0.25], np.float32) * f32(0.8) * ext[0],
                 types=types)
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: sc (the seeded scene), cfg, N, types, gauges {slot: gauge}, and from STEPS steps of the C oracle, computed once per
    process: pos0 (the seeded positions), states[k] (gauge_ref's state of step k), records[k] float64[16, 16] of all gauges."""
    scene, types = CASES[name]
    sc = seeded(scenes.SCENES[scene](), types)
    cfg = sc["cfg"]
    N = cfg.particleCount
    gauges = gauges_of(sc, types)
    ora = scenes.oracle_for(sc)
    states = []
    for _ in range(STEPS):
        ora.step()
        states.append(gr.oracle_state(ora, N))
    ora.close()
    records = [gr.records(st, gauges) for st in states]
    for st in states:
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    for r in records:
        r.setflags(write=False)
    return dict(sc=sc, cfg=cfg, N=N, types=types, gauges=gauges, pos0=sc["position"], states=states, records=records)


def counts(c):
    """Per slot over the case's steps: (positive, negative, counted, rejected by the (alpha, beta) test, counted of type 2)."""
    out = {}
    for slot, g in c["gauges"].items():
        p = m = rej = el = 0
        for st in c["states"]:
            C = gr.Crossings(st, g)
            p += int((C.direction == 1).sum())
            m += int((C.direction == -1).sum())
            rej += int((C.crossed & (C.direction == 0)).sum())
            el += int(((C.direction != 0) & (np.asarray(st["a"])[:, 3].astype(np.int32) == 2)).sum())
        out[slot] = (p, m, p + m, rej, el)
    return out


def liquid_only(n, spacing_in_r0=0.93):
    """A box with exactly n liquid particles: the first n of a 5 x 5 x 41 lattice column along z, then the boundary shell."""
    base = scenes.liquid_box((8.0, 8.0, 30.0), (5, 5, 41), spacing_in_r0=spacing_in_r0)
    nl = base["numOfLiquidP"]
    assert 1 <= n <= nl
    keep = np.r_[np.arange(n), np.arange(nl, base["position"].shape[0])]
    sc = dict(base)
    sc["position"], sc["velocity"] = base["position"][keep].copy(), base["velocity"][keep].copy()
    sc["numOfLiquidP"] = n
    cfg = scenes.liquid_box_config((8.0, 8.0, 30.0))
    cfg.particleCount = sc["position"].shape[0]
    sc["cfg"] = cfg
    return sc
