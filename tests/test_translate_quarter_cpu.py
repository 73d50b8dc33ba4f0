"""The inputs of tests/test_translate_quarter_gpu.py reach what they are meant to reach, judged from the oracle's ORF lists alone.

orf_tile_kernel gives a lane 24 nt, so a stop can sit at 24 in-lane positions, and the run it closes has been carried there
from the lane's own codons, from an earlier lane or from an earlier tile.  For each strand and each in-lane position of the
closing stop (the byte after the ORF's last, in memory order -- the order the kernel scans both strands in) the inputs must hold
an ORF of at least min_orf_len that closes there, one that began in another lane and one that began in another tile."""
import numpy as np

import translate_quarter_inputs as tq


def test_inputs_close_orfs_at_every_lane_position_over_every_seam():
    closes = np.zeros((2, tq.LANE_NT), np.int64)
    over_lane = np.zeros((2, tq.LANE_NT), np.int64)
    over_tile = np.zeros((2, tq.LANE_NT), np.int64)
    within_lane = 0
    for name, windows, ct, minlen in tq.cases():
        for w, strand, frame, start, end, res in tq.oracle_orfs(windows, ct, minlen):
            assert len(res) >= minlen
            lo, hi = tq.memory_extent(len(windows[w]), strand, start, end)
            assert 0 <= lo <= hi < len(windows[w]) and hi - lo + 1 == 3 * len(res), (name, w, strand, start, end)
            stop = hi + 1                                     # where the codon that closes the run starts (or would, past the end)
            pos = stop % tq.LANE_NT
            closes[strand, pos] += 1
            over_lane[strand, pos] += lo // tq.LANE_NT != stop // tq.LANE_NT
            over_tile[strand, pos] += lo // tq.TILE_NT != stop // tq.TILE_NT
            within_lane += lo // tq.LANE_NT == stop // tq.LANE_NT
    assert (closes > 0).all(), closes
    assert (over_lane > 0).all(), over_lane
    assert (over_tile > 0).all(), over_tile
    assert within_lane > 0                                    # and runs between two stops of one lane (min_orf_len <= 6 only)


def test_inputs_cover_the_lengths_and_block_shapes():
    by_name = {name: (windows, ct, minlen) for name, windows, ct, minlen in tq.cases()}
    lens = {len(w) for w in by_name["lengths_minlen20"][0]}
    assert set(range(15, 81)) <= lens
    for c in (384, 768, 1152):
        assert set(range(c - 26, c + 27)) <= lens
    assert {by_name["dense_minlen%d" % m][2] for m in (1, 2, 3, 4, 5, 6, 7, 8, 20)} == {1, 2, 3, 4, 5, 6, 7, 8, 20}
    for nw in (1, 2, 3, 5, 7):
        windows = by_name["block_of_%d" % nw][0]
        assert len(windows) == nw and all(100 <= len(w) <= 400 for w in windows)
    mixed = by_name["one_degenerate_between_canonical"][0]
    assert sum(int((w > 3).sum()) for w in mixed) == 1 and (mixed[0] <= 3).all() and (mixed[-1] <= 3).all()
    assert {by_name["genetic_code_4"][1], by_name["genetic_code_11"][1]} == {4, 11}
