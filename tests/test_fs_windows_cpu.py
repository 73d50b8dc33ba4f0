"""CPU tier, oracle only: the inputs of tests/fs_windows_inputs.py reach what they claim, so that nothing in tests/test_fs_windows_gpu.py
has to be skipped or called borderline.  What the oracle (bo_fs_build_windows, bo_fs_decide_window) makes of every case is the
expectation the GPU tier holds both drivers of bath_fs_windows.hip to."""
import numpy as np
import pytest

import fs_windows_inputs as I


def overlapping_neighbours(c):
    """Consecutive windows of one group that overlap: only the 2 * 3 * max_length cap can have kept them apart."""
    w, g = c.windows, c.grp
    same = (g[1:, 0] == g[:-1, 0])
    return int((same & (w["n"][:-1] + w["length"][:-1] - 1 >= w["n"][1:])).sum())


@pytest.mark.parametrize("n", I.SIZES)
def test_size_cases_have_the_sizes_they_name(n):
    c = I.case("n%d" % n)
    assert c.n == n and len(c.orfs) == n and c.accepts == (n <= 32768)
    assert sum(len(l[0]) for l in c.lanes()) == n and c.nhw <= 65536
    if n == 2049:
        assert c.nw == 2049                                           # one window per survivor: (2049 + 1023) // 1024 = 3 per thread
    elif n >= 255:
        assert c.nw < n and {0, 1} <= set(np.unique(c.found))         # windows were fused; ORFs with and without a hit window


def test_rank_grid_case_on_256_compute_units():
    assert I.first_split_n(256) == 8193 and 8193 in I.SIZES
    for n in (8193, 8449):
        gn = (n + 255) // 256
        cols = max(1, min(gn, 1024 // gn))
        assert cols < gn and gn % cols != 0
    gn = 8192 // 256
    assert max(1, min(gn, 1024 // gn)) == gn                          # ... and 8192 is the last n with a square grid


@pytest.mark.parametrize("size", I.GROUPS)
def test_group_cases(size):
    c = I.case("group%d" % size)
    assert size in c.group_sizes and max(c.group_sizes) == size and c.accepts == (size <= 1024)
    assert {1, 2} & set(c.group_sizes) or min(c.group_sizes) <= 5
    big = c.grp[:, 1] - c.grp[:, 0] == size
    assert 1 < big.sum() < size                                       # the dense group fused, and not into one window
    assert overlapping_neighbours(c) >= 1                             # a fuse chain that stopped at the cap


def test_group_sizes_one_and_two():
    sizes = set(I.case("n1").group_sizes) | set(I.case("n2").group_sizes) | set(I.case("density").group_sizes) | set(I.case("nohits").group_sizes)
    assert {1, 2} <= sizes


def test_straddling_group():
    c = I.case("straddle")
    assert c.group_sizes == [37, 1024, 50] and c.accepts
    o = c.orfs
    assert (o["w"][36], o["strand"][36]) == (0, 0) and (o["w"][37], o["strand"][37]) == (0, 1)            # the other strand of its sequence before it
    assert (o["w"][1060], o["strand"][1060]) == (0, 1) and (o["w"][1061], o["strand"][1061]) == (1, 1)    # the same strand of the next sequence after it
    assert 37 % 256 != 0 and (37 + 1024) // 256 > 37 // 256


def test_density_case_fuses_keeps_apart_and_stops_at_the_cap():
    c = I.case("density")
    per_group = {}
    for (g0, g1) in c.grp:
        per_group[(int(g0), int(g1))] = per_group.get((int(g0), int(g1)), 0) + 1
    sizes = {g1 - g0: nwin for (g0, g1), nwin in per_group.items()}
    assert sizes[6] == 6                                              # the sparse group: separate windows
    assert sizes[300] < 300 and sizes[200] < 200                      # the dense groups: fused pairs
    assert overlapping_neighbours(c) >= 1                             # ... and a pair kept apart by the cap alone
    w = c.windows
    assert (w["length"] < 2 * 3 * c.max_length).all()
    assert (w["orf_cnt"] > 1).any() and (w["orf_cnt"] == 1).any()


def test_equal_window_starts_within_a_group():
    found = False
    for name in ("density", "group1024", "open_ends"):
        c = I.case(name)
        o = c.orfs
        same = (o["g0"][1:] == o["g0"][:-1])
        order = np.lexsort((o["dw_n"], o["g0"]))
        s = o[order]
        found |= bool(((s["g0"][1:] == s["g0"][:-1]) & (s["dw_n"][1:] == s["dw_n"][:-1])).any())
        assert same.any()
    assert found


def test_no_hit_window_rules_and_ties():
    c = I.case("ties")
    M, o, p = c.M, c.orfs, c.pick
    assert M == 12 and (o["n"] >= M).any() and (o["n"] < M).any()
    a = p["none_short"]                                               # :500-510, n < M
    assert not c.found[a] and o["n"][a] < M and (o["dw_k"][a], o["kmin"][a], o["kmax"][a]) == (M - (M - o["n"][a]) // 2, M, 0)
    a = p["none_long"]                                                # n >= M: the centre of the ORF
    assert not c.found[a] and o["n"][a] >= M and o["dw_k"][a] == M
    assert c.found[p["score_length"]] and o["dw_k"][p["score_length"]] == 9           # score tie: the longer window, listed second
    assert o["dw_k"][p["score_length_start"]] == 8                    # score and length tie: the leftmost
    assert o["dw_k"][p["full_k"]] == 6                                # equal but for k: the smallest k, listed after k = 10 in a shuffled list
    owner, n, k, length, score = c.hits
    mine = owner == p["full_k"]
    assert sorted(k[mine & (score == 3.0)]) == [6, 8, 10]
    assert len(set(I.TIE_KINDS)) == len(p)
    nh = I.case("nohits")
    assert nh.nhw == 0 and not nh.found.any() and (nh.windows["k_min"] > nh.windows["k_max"]).all()


def test_open_ended_orfs_and_clamps_on_both_strands():
    c = I.case("open_ends")
    o = c.orfs
    n_seq = np.array([len(s) for s in c.seqs])[o["w"]]
    for strand in (0, 1):
        s = o["strand"] == strand
        assert (s & (o["end"] + 3 > n_seq)).sum() >= 2                               # ORFs still open at the sequence end, in more than one frame
        assert (s & (o["dw_n"] == 1) & (o["start"] > 3)).any()                        # clamped at position 1
        assert (s & (o["dw_n"] + o["dw_len"] - 1 == n_seq) & (o["end"] < n_seq - 3)).any()   # clamped at the sequence end
    # the open ORFs follow the closed ones of their strand, frame by frame
    for g0, g1 in {(int(a), int(b)) for a, b in zip(o["g0"], o["g1"])}:
        opened = o["end"][g0:g1] + 3 > n_seq[g0:g1]
        assert not opened[:-int(opened.sum())].any() if opened.any() else True


def test_far_start_case():
    c = I.case("far_start")
    owner, n, k, length, score = c.hits
    assert not c.accepts and (n > 0xfffff).sum() == 1 and c.orfs["n"][c.big] > 0x100000
    assert len(c.seqs) == 1 and len(c.seqs[0]) > 4000000
    assert c.found[c.big] and c.orfs["dw_k"][c.big] == 60             # the far window is the ORF's best: the oracle's window follows it


def test_lane_and_hit_window_cases():
    for K, empty in ((1, ()), (2, ()), (3, (1,)), (16, (0, 7, 15)), (17, (0, 8, 16))):
        c = I.case("lanes%d" % K)
        lanes = c.lanes()
        assert len(lanes) == K and c.accepts == (K <= 16)
        assert [k for k in range(K) if len(lanes[k][0]) == 0] == list(empty)
        assert sum(len(l[0]) for l in lanes) == c.n and sum(len(l[1]) for l in lanes) == c.nhw
        a, b = c.lanes(shuffle=1), c.lanes(shuffle=2)
        k = next(k for k in range(K) if len(lanes[k][0]) > 8)
        assert not np.array_equal(a[k][0], b[k][0]) and np.array_equal(np.sort(a[k][0], order="cand"), np.sort(b[k][0], order="cand"))
    assert I.case("hitwins65536").nhw == 65536 and I.case("hitwins65536").accepts
    assert I.case("hitwins65537").nhw == 65537 and not I.case("hitwins65537").accepts
    assert (I.case("fsonly").windows["P_tot"] == 1.0).all() and (I.case("density").windows["P_tot"] < 1.0).any()


@pytest.mark.parametrize("do_biasfilter,std_pipe", [(1, 1), (0, 1), (1, 0)])
def test_decide_cases_are_clear_or_exactly_tied(do_biasfilter, std_pipe):
    rec, bias, fsc, kinds, want = I.decide_cases(do_biasfilter, std_pipe)
    assert len(rec) >= 100 and set(kinds) == {"clear", "tied"}
    L3 = rec["length"] // 3
    assert {0, 1, 2} <= set(L3) and (L3 > 100).any()
    assert (rec["k_min"] > rec["k_max"]).any() and (rec["k_min"] <= rec["k_max"]).any()
    branches = {w[4] for w in want}
    assert branches == ({1, 2} if std_pipe else {0, 1})
    tied = [i for i, k in enumerate(kinds) if k == "tied"]
    assert {int(rec["orf_cnt"][i]) for i in tied} == {1, 2}
    for i in tied:
        assert want[i][3] == 1.0 and rec["P_tot"][i] == 1.0
    # among the tied records with one ORF, the P_min > F3 clause alone decides: both outcomes occur
    one = [i for i in tied if rec["orf_cnt"][i] == 1 and want[i][2] <= I.F3]
    two = [i for i in tied if rec["orf_cnt"][i] == 2 and want[i][2] <= I.F3]
    if do_biasfilter:
        assert {want[i][4] == 1 for i in one} == {True, False} and len(two) >= 3
        assert all((want[i][4] == 1) == (rec["P_min"][i] > I.F3) for i in one)
        assert all(want[i][4] == 1 for i in two)                      # P_null == P_tot and more than one ORF
    else:
        # without the bias filter the filter score is the null score: P_fs == P_null == 1.0 for every tied record, none passes F3
        assert not one and not two and all(w[0] == w[1] for w in want if np.isfinite(w[0]))
