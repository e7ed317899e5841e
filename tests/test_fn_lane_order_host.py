"""The scene of test_fn_lane_order.py, judged without a GPU on the oracle's rows after one step. The lane pair of findNeighbors
(csrc/sph_neighbors.hip) walks the cells 0 4 5 7 | 1 2 3 6 of the reference's order and merges them as A0 | B1 B2 B3 | A4 A5 | B6 | A7
from per-piece counts; a wrong piece start shows only where the pieces on both sides of it hold neighbours, and the cut at 32 slots
only where it falls into that segment. So the scene must have particles with a neighbour in every one of the eight cells, particles
with neighbours in cells 4 and 6 and 7 at once (the three segments the order interleaves), full rows, and full rows whose last slot
lies in each of the eight cells. These are conditions on the scene, not tolerances."""
import numpy as np

import scenes
from test_gpu_parity import canon_ora

STEPS = 3
_state = {}


def jitter_scene():
    """The `tiny` box with wide cell ids: 9 x 9 x 9 cells, 2 792 particles, compressed lattice with strong jitter."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), spacing_in_r0=0.85, jitter_in_r0=0.2, mask=0xffffffff)


def lattice_scene():
    """The same box at the headline's local state: spacing 0.93 r0, no jitter."""
    return scenes.liquid_box((8.0, 8.0, 8.0), (12, 10, 12), mask=0xffffffff)


SCENE = {"jitter": jitter_scene, "lattice": lattice_scene}


def oracle_states(name):
    """Canonical oracle buffers after each of STEPS steps: computed once per scene, shared, never changed."""
    if name not in _state:
        sc = SCENE[name]()
        N = sc["cfg"].particleCount
        ora = scenes.oracle_for(sc, threads=8)
        out = []
        for _ in range(STEPS):
            ora.step()
            out.append(canon_ora(ora, N))
        ora.close()
        _state[name] = out
    return _state[name]


def row_cells(canon, cfg):
    """int[N, 32]: the reference cell 0..7 (own, x, y, z, xy, xz, yz, xyz) each slot's neighbour lies in, -1 for an empty slot."""
    N = cfg.particleCount
    gx, gy = cfg.gridCellsX, cfg.gridCellsY
    keys = canon["particleIndex"].reshape(-1, 2)[:N, 0].astype(np.int64)
    ids = canon["neighborIds"].reshape(-1, 32)[:N].astype(np.int64)
    cell = np.stack([keys % gx, (keys // gx) % gy, keys // (gx * gy)], 1)
    used = ids >= 0
    step = cell[np.where(used, ids, 0)] - cell[:, None, :]
    assert (np.abs(step[used]) <= 1).all()  # (no wrapped cells in this box)
    moved = step != 0
    index = np.array([0, 1, 2, 4, 3, 5, 6, 7])[moved[..., 0] + 2 * moved[..., 1] + 4 * moved[..., 2]]  # x | y << 1 | z << 2 -> 0..7
    return np.where(used, index, -1)


def test_scene_has_nine_cells_per_axis_and_allows_bands():
    import band_ref
    cfg = jitter_scene()["cfg"]
    assert (cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellsZ) == (9, 9, 9) and cfg.particleCount == 2792
    assert band_ref.grid_allows_bands(cfg)


def test_rows_exercise_every_piece_start_and_the_cut_in_every_segment():
    cfg = jitter_scene()["cfg"]
    cells = row_cells(oracle_states("jitter")[0], cfg)
    has = np.stack([(cells == k).any(1) for k in range(8)], 1)
    per_cell = has.sum(0)
    interleaved = int((has[:, 4] & has[:, 6] & has[:, 7]).sum())
    full = cells[:, 31] >= 0
    last = np.bincount(cells[full, 31], minlength=8)
    print("particles with a neighbour in cells 0..7: %s" % per_cell.tolist())
    print("particles with neighbours in cells 4 and 6 and 7: %d" % interleaved)
    print("rows with all 32 slots used: %d; of those, slot 31 lies in cell 0..7: %s" % (int(full.sum()), last.tolist()))
    assert (per_cell >= 1).all()
    assert interleaved >= 1
    assert full.sum() >= 1
    assert (last >= 1).all()


def test_slots_of_every_row_are_ordered_by_reference_cell():
    for name in SCENE:
        cells = row_cells(oracle_states(name)[0], SCENE[name]()["cfg"])
        used = cells >= 0
        assert (used[:, 1:] <= used[:, :-1]).all(), name + ": an empty slot in front of a used one"
        both = used[:, 1:] & used[:, :-1]
        assert (cells[:, 1:][both] >= cells[:, :-1][both]).all(), name
