"""The prelude under the first search chunks, without a GPU: which band records the search launches that start at the
fork may read, and which launches are issued behind the deferred scatter.

The rule under test, from include/sphmi_chunks.h: with d = sphBandDeferFirst(C) the prelude scatters the band records of chunks
[0, d); the search of chunk c is issued behind the deferred scatter (evDeferred) iff c + 1 >= d and d < C. Under the premise of the
halo check the search of chunk c reads band records only of chunks c - 1 .. c + 1; the last test states that premise by brute force
over the cells a band run can span."""
import numpy as np
import pytest

import sphmi
from test_step_pipeline import PARITY_SCENES, edges_of, halo_check, oracle_states, search_tables

SEARCH_STREAMS = 2  # the search of chunk c runs on stream c & 1 (enqueue_search_overlapped)


def issued_behind_deferred(chunks, c):
    d = sphmi.step_band_defer_first(chunks)
    return d < chunks and c + 1 >= d


@pytest.mark.parametrize("chunks", range(1, 17))
def test_first_deferred_chunk(chunks):
    d = sphmi.step_band_defer_first(chunks)
    assert 1 <= d <= chunks
    assert (d == chunks) == (chunks <= 3), "nothing is deferred with three chunks or fewer, something with more"
    if d < chunks:
        # the launches that start at the fork: at least chunk 0, at most one per search stream
        assert 1 <= d - 1 <= SEARCH_STREAMS


@pytest.mark.parametrize("chunks", range(1, 17))
def test_every_search_chunk_reads_scattered_records(chunks):
    """For every depth: in the issue order of the schedule, a search launch either needs only band chunks of the prelude range or
    is issued behind evDeferred; the searches of one stream are issued in ascending chunk order, so a stream that has waited once
    stays behind the event."""
    d = sphmi.step_band_defer_first(chunks)
    for depth in range(7):
        _, items = sphmi.step_pipeline_schedule(chunks, depth, 3, False)
        searches = [c for stage, c in items if stage == 0]
        assert searches == list(range(chunks))
        for stream in range(SEARCH_STREAMS):
            mine = [c for c in searches if c & 1 == stream]
            assert mine == sorted(mine)
            behind = [issued_behind_deferred(chunks, c) for c in mine]
            assert behind == sorted(behind), "once behind the event, always behind it"
        for c in searches:
            needs = [b for b in (c - 1, c, c + 1) if 0 <= b < chunks]
            assert max(needs) < d or issued_behind_deferred(chunks, c), (chunks, depth, c)
            if not issued_behind_deferred(chunks, c) and d < chunks:
                assert c < d - 1 <= SEARCH_STREAMS, "only the launches at the fork go without the deferred records"


def test_bad_chunk_count_is_rejected():
    for bad in (0, -3):
        with pytest.raises(sphmi.SphError):
            sphmi.step_band_defer_first(bad)


def band_reads_stay_in_the_halo(keys, start, edges, gx, gy):
    """Brute force over what a search launch can read of the band arrays. A batch of chunk [lo, hi) has its cells in
    [keys[lo], keys[hi - 1]]; its eight band runs lie between the start-table entries of the cells keys[lo] - 1 - gx - gx gy and
    keys[hi - 1] + 2 + gx + gx gy (clamped to the table), and bandStart[cell] counts the band entries of the particles in front of
    cellStart[cell]: the records belong to sorted particles in [cellStart[first cell], cellStart[last cell + 1))."""
    keys, start = np.asarray(keys, np.int64), np.asarray(start, np.int64)
    G, chunks = start.size - 1, len(edges) - 1
    reach = gx * gy + gx + 1
    for c in range(chunks):
        lo, hi = edges[c], edges[c + 1]
        if hi <= lo:
            continue
        first = min(max(int(keys[lo]) - reach, 0), G)
        last = min(max(int(keys[hi - 1]) + reach + 1, 0), G)
        if start[last] > start[first] and (start[first] < edges[max(c - 1, 0)] or start[last] > edges[min(c + 2, chunks)]):
            return False
    return True


@pytest.mark.parametrize("name,chunks", [("tiny_long", c) for c in range(4, 9)] + [("tiny", 7), ("tiny", 16), ("thin", 16)])
def test_a_passed_halo_check_confines_the_band_reads(name, chunks):
    """On the scenes the GPU tests run: wherever the device's check passes, no search launch reads a band record of a chunk other
    than c - 1 .. c + 1; so the launches at the fork read only what the prelude scatters."""
    cfg = PARITY_SCENES[name]()["cfg"]
    d = sphmi.step_band_defer_first(chunks)
    for it, canon in enumerate(oracle_states(name)[:3]):
        keys, start = search_tables(canon)
        e = edges_of(keys.size, chunks)
        if halo_check(canon, cfg, chunks):
            assert band_reads_stay_in_the_halo(keys, start, e, cfg.gridCellsX, cfg.gridCellsY), "step %d" % it
            for c in range(chunks):
                if not issued_behind_deferred(chunks, c):
                    assert min(c + 2, chunks) <= d
