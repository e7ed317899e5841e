"""The scene, the lattices, the sequence and the claims that the statistics tests share (tests/test_stats_host.py on the oracle's
states, tests/test_stats.py on the device's). The claims are non-empty classes of nodes: without them the comparison could pass on
lattices that never see a node turn wet or dry.

The scene is probe_cases.scene(): a jittered block of liquid inside the boundary shell (8 x 8 x 8 h, lattice (10, 8, 10)). Lengths are
in r0. The sequence: two steps, call 0; a step, call 1; the liquid with x < 7 r0 is removed and a 2 x 2 x 2 block of liquid is added
in the air above what is left; a step, call 2; a step, call 3."""
import numpy as np

import edit_ref
import probe_cases
import stats_ref

F = np.float32
LIQUID = 1 << 1
CALLS = 4
STEPS_BEFORE_CALL = (2, 1, 1, 1)
EDIT_BEFORE_CALL = 2  # the edit is made in front of this call's step
CUT_X, BLOCK_AT, BLOCK_SPACING = 7.0, (9.0, 12.5, 7.0), 0.93


def scene():
    return probe_cases.scene()


def lattices(cfg):
    """{name: lattice dict}. A: the brick route (spacing 0.6 r0 = 0.3 h <= 2h/3), partial bricks on every axis, 5 x 5 x 3 = 75 bricks:
    72 go through the XCD remap and 3 do not. B: the point route (1.7 r0 = 0.85 h)."""
    r0 = F(cfg.r0)
    o = np.array([F(2.6) * r0] * 3, F)
    return {"A": dict(origin=o, spacing=np.array([F(0.6) * r0] * 3, F), dims=(17, 19, 9), typeMask=LIQUID),
            "B": dict(origin=o, spacing=np.array([F(1.7) * r0] * 3, F), dims=(6, 7, 6), typeMask=LIQUID)}


def edit_region(cfg):
    """remove_region's box of the liquid with x < CUT_X r0."""
    return (-np.inf, -np.inf, -np.inf, float(F(CUT_X) * F(cfg.r0)), np.inf, np.inf)


def added_block(cfg):
    """(position [8, 4], velocity [8, 4]) of the added liquid, at rest."""
    r0 = F(cfg.r0)
    pos = np.zeros((8, 4), F)
    for n in range(8):
        i, j, k = n & 1, (n >> 1) & 1, n >> 2
        pos[n] = (F(BLOCK_AT[0]) * r0 + F(i) * F(BLOCK_SPACING) * r0, F(BLOCK_AT[1]) * r0 + F(j) * F(BLOCK_SPACING) * r0,
                  F(BLOCK_AT[2]) * r0 + F(k) * F(BLOCK_SPACING) * r0, F(1.0))
    return pos, np.zeros((8, 4), F)


def edited_arrays(cfg, pos, vel):
    """The edit on host arrays in original order ([N, 4] each): what remove_region and add_particles leave."""
    pos, vel = np.asarray(pos, F).reshape(-1, 4), np.asarray(vel, F).reshape(-1, 4)
    gone = (pos[:, 3].astype(np.int32) == 1) & (pos[:, 0] < F(edit_region(cfg)[3]))
    ap, av = added_block(cfg)
    return np.concatenate([pos[~gone], ap]), np.concatenate([vel[~gone], av]), int(gone.sum())


def edited_scene(sc, pos, vel):
    p, v, removed = edited_arrays(sc["cfg"], pos, vel)
    out = dict(sc, cfg=edit_ref.with_count(sc["cfg"], p.shape[0]), position=p, velocity=v)
    return out, removed


def fold_sequence(records_per_call):
    """[(acc, calls)] after every call, from the records of every call (float32[nodes, 8] each)."""
    acc = stats_ref.empty(records_per_call[0].shape[0])
    out = []
    for c, rec in enumerate(records_per_call):
        acc = stats_ref.fold(acc, rec, c)
        out.append((acc, c + 1))
    return out


def check_claims(records_per_call):
    """Asserts the claims on the records of the four calls of one lattice; returns the class sizes."""
    assert len(records_per_call) == CALLS
    wet = np.stack([r[:, 6] > 0 for r in records_per_call])  # [calls, nodes]
    classes = {"never wet": ~wet.any(0), "wet then dry": wet[0] & wet[1] & ~wet[2] & ~wet[3],
               "dry then wet": ~wet[0] & ~wet[1] & wet[2] & wet[3], "always wet": wet.all(0)}
    sizes = {k: int(v.sum()) for k, v in classes.items()}
    assert all(sizes.values()), sizes
    for c in (0, 1):
        assert (records_per_call[c][:, 5] != 0).any(), "pressure is zero everywhere in call %d" % c
    acc = fold_sequence(records_per_call)[-1][0]
    peak_calls = set(acc[acc[:, 0] > 0, 19].tolist())
    assert len(peak_calls) >= 2, peak_calls
    assert (acc[classes["dry then wet"], 1] == 2).all() and (acc[classes["wet then dry"], 2] == 1).all()
    return sizes
