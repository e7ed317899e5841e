"""numpy float32 restatement of the integral-curve contract (include/sphmi.h, sph_trace_streamlines / sph_tracers_advect).

velocity(p) is taken from sample_ref.sample_reference (words 1..4 of its records; S != 0 is read off word 1), so the sampling sums
exist once, there. All live curves advance together: one sample_reference call per stage (the vertices, then the midpoints).

`state` is a sample_ref state (sample_ref.solver_state), or a function (points, types) -> float32[Q, 8] sample records in its
place, such as a solver's sample_points: the same step as a host loop over the existing API."""
import numpy as np

import sample_ref

f32 = np.float32
TIME, ARC = 0, 1
EULER, MIDPOINT = 0, 1
MOVING, MAX_STEPS, LEFT_MATTER, LEFT_REGION, STAGNANT, NONFINITE = 0, 1, 2, 3, 4, 5
CODES = {"max_steps": MAX_STEPS, "left_matter": LEFT_MATTER, "left_region": LEFT_REGION, "stagnant": STAGNANT,
         "nonfinite": NONFINITE}


def velocity(state, points, types):
    """(hit bool[Q], u float32[Q, 3], speed float32[Q]) at `points`; speed = sqrtf(ux*ux + uy*uy + uz*uz), summed left to right,
    and 0 without a hit."""
    rec = state(points, types) if callable(state) else sample_ref.sample_reference(state, points, types)
    hit = rec[:, 1] != 0
    u = rec[:, 2:5].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    return hit, u, np.where(hit, s, f32(0)).astype(np.float32)


def _finite(p):
    return np.isfinite(p).all(axis=1)


def _inside(p, region):
    if region is None:
        return np.ones(p.shape[0], bool)
    r = np.asarray(region, np.float32)
    with np.errstate(invalid="ignore"):
        return ((r[None, :3] <= p) & (p <= r[None, 3:])).all(axis=1)


def _scale(step, s, mode):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return step / s if mode == ARC else np.full(s.shape, step, np.float32)


def step_once(state, p, types, step, min_speed, mode, integrator, region=None, at_limit=None):
    """Items 1-7 at the vertices p [n, 3] (float32): (next float32[n, 3], the speed written with the vertex float32[n], code
    int32[n]). code is MOVING where the curve advanced (next is p_{k+1}); elsewhere next is p. at_limit (bool[n] or None): where
    item 6 holds."""
    p = np.ascontiguousarray(p, np.float32)
    step, min_speed = f32(step), f32(min_speed)
    n = p.shape[0]
    code = np.full(n, MOVING, np.int32)
    speed = np.zeros(n, np.float32)
    nxt = p.copy()
    fin = _finite(p)
    code[~fin] = NONFINITE
    live = np.flatnonzero(fin)
    if live.size:
        hit, u, s = velocity(state, p[live], types)
        speed[live] = s
        c = code[live]
        c[(c == MOVING) & ~hit] = LEFT_MATTER
        c[(c == MOVING) & ~_inside(p[live], region)] = LEFT_REGION
        with np.errstate(invalid="ignore"):
            c[(c == MOVING) & ~(s > min_speed)] = STAGNANT
        if at_limit is not None:
            c[(c == MOVING) & np.asarray(at_limit, bool)[live]] = MAX_STEPS
        code[live] = c
        go = live[c == MOVING]
        ug, sg = u[c == MOVING], s[c == MOVING]
        if go.size:
            cs = _scale(step, sg, mode)
            with np.errstate(over="ignore", invalid="ignore"):
                if integrator == EULER:
                    nxt[go] = p[go] + cs[:, None] * ug
                else:
                    q = p[go] + (f32(0.5) * cs)[:, None] * ug
                    qc = np.full(go.size, MOVING, np.int32)
                    qfin = _finite(q)
                    qc[~qfin] = NONFINITE
                    hit2 = np.zeros(go.size, bool)
                    u2 = np.zeros((go.size, 3), np.float32)
                    s2 = np.zeros(go.size, np.float32)
                    if qfin.any():
                        hit2[qfin], u2[qfin], s2[qfin] = velocity(state, q[qfin], types)
                    qc[(qc == MOVING) & ~hit2] = LEFT_MATTER
                    qc[(qc == MOVING) & ~(s2 > min_speed)] = STAGNANT
                    ok = qc == MOVING
                    c2 = _scale(step, s2[ok], mode)
                    nxt[go[ok]] = p[go[ok]] + c2[:, None] * u2[ok]
                    code[go] = qc
    return nxt, speed, code


def streamlines(state, seeds, types=(1,), step=1.0, mode=ARC, integrator=MIDPOINT, max_steps=32, min_speed=0.0, region=None):
    """(vertices float32[Q, max_steps + 1, 4], lengths int32[Q], status int32[Q]) of sph_trace_streamlines."""
    seeds = np.asarray(seeds, np.float32).reshape(-1, np.asarray(seeds).shape[-1])[:, :3]
    Q, M = seeds.shape[0], int(max_steps)
    verts = np.zeros((Q, M + 1, 4), np.float32)
    lengths = np.zeros(Q, np.int32)
    status = np.full(Q, MOVING, np.int32)
    p = seeds.copy()
    live = np.arange(Q)
    for k in range(M + 1):
        if live.size == 0:
            break
        nxt, speed, code = step_once(state, p[live], types, step, min_speed, mode, integrator, region,
                                     at_limit=np.full(live.size, k == M))
        verts[live, k, :3] = p[live]
        verts[live, k, 3] = speed
        lengths[live] = k + 1
        status[live] = code
        p[live] = nxt
        live = live[code == MOVING]
    assert live.size == 0
    return verts, lengths, status


def tracers_advect(state, pos4, status, steps, types=(1,), step=1.0, mode=TIME, integrator=MIDPOINT, min_speed=0.0, region=None):
    """One sph_tracers_advect on (pos4 float32[Q, 4], status, steps): the new three arrays."""
    pos4 = np.array(pos4, np.float32)
    status = np.array(status, np.int32)
    steps = np.array(steps, np.int32)
    live = np.flatnonzero(status == MOVING)
    if live.size:
        nxt, speed, code = step_once(state, pos4[live, :3], types, step, min_speed, mode, integrator, region)
        pos4[live, :3] = nxt
        pos4[live, 3] = speed
        status[live] = code
        steps[live] += 1
    return pos4, status, steps
