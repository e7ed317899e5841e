"""The cell rule of the neighbourhood bytes (tests/wave_nb_ref.py) on oracle states, without a GPU: the waves it marks
contain every wave that the neighbour rows say reads a flagged wave — for the flags the state really has (a wave holds a pressure),
for every wave flagged and for a random tenth of the waves flagged."""
import numpy as np
import pytest

import scenes
import test_pressure_skip as tps
import wave_nb_ref as nb
from test_gpu_parity import canon_ora

_small = {}


def small_oracle(name, steps=2):
    """Canonical buffers of the oracle after `steps` steps of a scenes.SCENES scene: computed once, shared, never changed."""
    if name not in _small:
        sc = scenes.SCENES[name]()
        ora = scenes.oracle_for(sc, threads=8)
        for _ in range(steps):
            ora.step()
        _small[name] = (sc["cfg"], canon_ora(ora, sc["cfg"].particleCount))
        ora.close()
    return _small[name]


def check_superset(canon, cfg, where):
    N = cfg.particleCount
    keys, table = nb.search_tables(canon)
    ids = canon["neighborIds"].reshape(N, 32).astype(np.int64)
    gx, gy, G = cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellCount
    assert G > gx * gy + gx + 1
    W = (N + 63) // 64
    holds_p = nb.wave_any(canon["pressure"][:N] != 0)
    rng = np.random.default_rng(7)
    wrapped_any = 0
    for what, flagged in (("pressure", holds_p), ("every wave", np.ones(W, bool)), ("a tenth", rng.random(W) < 0.1)):
        cells, closed, wrapped = nb.neighbourhood(keys, table, flagged, gx, gy, G)
        rows = nb.readers_by_rows(ids, flagged)
        assert not closed, where
        assert not (rows & ~cells).any(), "%s, %s: %d waves read a flagged wave that the cell rule does not mark" % (where, what, (rows & ~cells).sum())
        wrapped_any += wrapped
    return wrapped_any


@pytest.mark.parametrize("step", [10, 20])
def test_mixed_column(step):
    cfg = tps.mixed_scene()["cfg"]
    canon = tps.oracle_states("mixed", tps.MIXED_STEPS)[step]
    check_superset(canon, cfg, "mixed column, step %d" % step)
    # the waves with liquid that must serve K12 in full: by rows (test_pressure_skip) and by cells
    has_liquid, full, close, _ = tps._wave_sets(canon, cfg)
    keys, table = nb.search_tables(canon)
    holds_p = nb.wave_any(canon["pressure"][:cfg.particleCount] != 0)
    cells, _, _ = nb.neighbourhood(keys, table, holds_p, cfg.gridCellsX, cfg.gridCellsY, cfg.gridCellCount)
    by_cells = cells | nb.wave_any(close)
    assert not (full & ~by_cells).any()
    share_rows, share_cells = full[has_liquid].mean(), by_cells[has_liquid].mean()
    print("step %d: share of the waves with liquid that serve K12 in full: %.3f by rows, %.3f by cells" % (step, share_rows, share_cells))
    if step == 20:
        assert 0.2 <= share_cells <= 0.8


def test_compressed_column():
    cfg = tps.build("compressed")["cfg"]
    canon = tps.oracle_states("compressed", (1, 3))[1]
    check_superset(canon, cfg, "0.85 r0 column, step 1")


def test_aliased_keys():
    cfg, canon = small_oracle("alias16")
    keys, _ = nb.search_tables(canon)
    assert cfg.cellIdMask == 0xffff and keys.max() < 65536 < cfg.gridCellCount
    check_superset(canon, cfg, "alias16")


def test_cells_wrapped_at_the_ends_of_the_table():
    """Particles of the first cell layers: kj - delta falls below 0 and is taken + G, as the search's wrap_cell turns it back."""
    cfg, canon = small_oracle("tiny")
    assert check_superset(canon, cfg, "tiny") > 0
