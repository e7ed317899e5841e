"""The scenes the wall-load tests share (tests/test_wall_host.py on the oracle, tests/test_wall.py on the GPU): committed scenes
whose floor -- the boundary particles with y < r0 -- is lifted into the liquid after a few steps, so that the contact branch of
integrate runs with a non-zero shift and its reflection branch runs at all, and the floor's split at the box's mid-x into two
bodies. Inputs only; the lifted state comes from the C oracle and the kinematic-body restatement, computed once per process."""
import functools

import numpy as np

import body_ref as br
import scenes
import sphmi
from sphmi import frames

f32 = np.float32
SLOT_A, SLOT_B = 2, 11  # body slots the tests use for the two halves of the floor
# name -> (scene, steps before the lift, lift in r0)
LIFTED = {"tiny": ("tiny", 3, 2.4), "tiny_jitter": ("tiny_jitter", 3, 2.3)}


@functools.lru_cache(maxsize=None)
def _lifted(name):
    scene_name, steps, lift = LIFTED[name]
    sc = scenes.SCENES[scene_name]()
    cfg = sc["cfg"]
    N, r0 = cfg.particleCount, f32(cfg.r0)
    ora = scenes.oracle_for(sc)
    for _ in range(steps):
        ora.step()
    pos = ora.buffer("position").reshape(-1, 4)[:N].copy()
    vel = ora.buffer("velocity").reshape(-1, 4)[:N].copy()
    ora.close()
    mid = f32(0.5) * f32(cfg.xmax)
    inf = np.inf
    a = br.region_members(pos, (-inf, -inf, -inf, mid, r0, inf))
    b = br.region_members(pos, (mid, -inf, -inf, inf, r0, inf))
    pose = frames.pose_translate((0.0, float(r0) * lift, 0.0))
    moved_pos, moved_vel = pos, vel
    for ids in (a, b):
        moved_pos, moved_vel, _ = br.set_pose(cfg, moved_pos, moved_vel, br.define(pos, vel, ids), pose)
    for x in (pos, vel, moved_pos, moved_vel, a, b, pose):
        x.setflags(write=False)
    return dict(sc=sc, cfg=cfg, N=N, steps=steps, pos=pos, vel=vel, moved_pos=moved_pos, moved_vel=moved_vel, A=a, B=b, pose=pose)


def lifted(name):
    """dict: sc / cfg / N of the scene, `steps` the steps before the lift, pos / vel the state after them (float32[N, 4],
    original-id order), moved_pos / moved_vel that state with the floor lifted, A / B the original ids of the floor's two halves
    (ascending), pose the lift. The arrays are shared and read-only."""
    return _lifted(name)


def moved_scene(case):
    """The scene dict of a solver created from the lifted state."""
    sc = dict(case["sc"])
    sc["position"], sc["velocity"] = case["moved_pos"], case["moved_vel"]
    return sc


def dense_on_floor():
    """A cube of liquid at 0.45 r0 standing 0.3 r0 above the floor's boundary layer (which lies at y = 0.5 r0): nearly every
    particle has more than 96 others within h, so findNeighbors serves it by the exact walk and its neighbour row has no 16-bit
    copy (scenes.crowded_particles), and the bottom layers have the floor among their 32 nearest and touch it in the first step."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (9, 6, 9), spacing_in_r0=0.45, origin_in_r0=(3.0, 0.8, 3.0))
