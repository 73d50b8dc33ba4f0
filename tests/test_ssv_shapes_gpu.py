"""GPU parity of the two SSV kernels at every tile shape, with best diagonals steered over every seam of the tiling.

ssv_lane_kernel<NR, G> (the standalone filters) and ssv_orf_kernel<NR, G> (the cascade) are instantiated once per entry of
BATH_SSV_SHAPES (bath_tilings.hpp).  Every shape runs here at the smallest and the largest model that selects it, against the oracle,
bit for bit: no tolerance anywhere in this file.  test_tiling_coverage_cpu.py holds SSV_SHAPES, ssv_shape and SSV_M against the sources.

A lane's register r holds node r+1 of its tile in the low half and node NR+r+1 in the high half; tile g of a target's G lanes holds
nodes 2 NR g + 1 .. 2 NR (g + 1).  A diagonal therefore crosses a seam of the layout at every multiple of NR: an odd multiple is the
step from the low to the high halves (register NR-1 wraps into register 0), an even one the step to the next lane (the carry that
__shfl_up brings over 64/G lanes).  Node 1 takes the begin score from the left, node M is followed by padding.  The seam targets
put an ungapped pass over each of these places, and a condition on the inputs, evaluated from the oracle and a plain numpy Kadane
alone, says that a kernel which breaks a seam changes a score that is compared (seam_condition).  What the last seam guards is node
M's own entry in the table: the padding cells behind it feed no node, so their value, -1.0 or 0, cannot change a maximum."""
import atexit
import functools
import os
import shutil
import tempfile
import time

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# BATH_SSV_SHAPES, in the order of bath_tilings.hpp
SSV_SHAPES = ([(nr, 1) for nr in range(16, 77, 4)] + [(nr, 1) for nr in range(160, 209, 16)]
              + [(40, 2), (48, 2), (56, 2), (64, 2), (72, 2), (76, 2)] + [(nr, 2) for nr in range(112, 209, 16)]
              + [(nr, 4) for nr in range(112, 209, 16)] + [(112, 8), (128, 8), (144, 8), (160, 8)])
SSV_MAX_NODES = 2560                           # 8 lanes x 160 registers x 2 nodes: the largest cost table a workgroup's LDS holds
OPROFILE_MAX_NODES = 3328
CASCADE_MAX_NODES = 2048
LDS_MESSAGE = "model too long for the LDS-resident SSV cost table"


def ssv_shape(M):
    """(NR, G) of the SSV kernels for a model of M nodes: the rule of bath_profile.hip restated."""
    G = 2 if 152 < M <= 304 else 1
    while G < 8 and M > 416 * G:
        G *= 2
    assert M <= 416 * G
    NR = ((M + G - 1) // G + 1) // 2
    if G == 1 and NR <= 112:
        NR = (NR + 3) // 4 * 4
    elif G == 2 and NR <= 76:
        NR = 40 if NR <= 40 else ((NR + 7) // 8 * 8 if NR <= 72 else 76)
    else:
        NR = max((NR + 15) // 16 * 16, 112 if G > 1 else 16)
    return max(NR, 16), G


# per shape: the smallest and the largest model that select it
SSV_M = {
    (16, 1): (1, 32), (20, 1): (33, 40), (24, 1): (41, 48), (28, 1): (49, 56), (32, 1): (57, 64),
    (36, 1): (65, 72), (40, 1): (73, 80), (44, 1): (81, 88), (48, 1): (89, 96), (52, 1): (97, 104),
    (56, 1): (105, 112), (60, 1): (113, 120), (64, 1): (121, 128), (68, 1): (129, 136),
    (72, 1): (137, 144), (76, 1): (145, 152),
    (160, 1): (305, 320), (176, 1): (321, 352), (192, 1): (353, 384), (208, 1): (385, 416),
    (40, 2): (153, 160), (48, 2): (161, 192), (56, 2): (193, 224), (64, 2): (225, 256),
    (72, 2): (257, 288), (76, 2): (289, 304),
    (112, 2): (417, 448), (128, 2): (449, 512), (144, 2): (513, 576), (160, 2): (577, 640),
    (176, 2): (641, 704), (192, 2): (705, 768), (208, 2): (769, 832),
    (112, 4): (833, 896), (128, 4): (897, 1024), (144, 4): (1025, 1152), (160, 4): (1153, 1280),
    (176, 4): (1281, 1408), (192, 4): (1409, 1536), (208, 4): (1537, 1664),
    (112, 8): (1665, 1792), (128, 8): (1793, 2048), (144, 8): (2049, 2304), (160, 8): (2305, 2560),
}


def ssv_seams(M, NR, G):
    """The seam nodes of an M-node model under tile shape (NR, G), ascending: [(node, kind)].  "first": node 1; "half": an odd
    multiple of NR (to its right the high halves begin); "lane": an even multiple (to its right the next lane's tile begins);
    "last": node M.  A multiple of NR that is M itself is the last node: nothing lies to its right."""
    assert M <= 2 * NR * G
    seams = [(1, "first")]
    seams += [(s, "half" if (s // NR) % 2 else "lane") for s in range(NR, M, NR)]
    if M > 1:
        seams.append((M, "last"))
    return seams


DEFAULT_CASES = [(m, nr, g) for (nr, g), (lo, hi) in SSV_M.items() for m in sorted({lo, hi})]      # (M, NR, G) at both ends of every shape
CASCADE_CASES = [c for c in DEFAULT_CASES if c[0] <= CASCADE_MAX_NODES]
case_id = lambda c: "NR%d-G%d-M%d" % (c[1], c[2], c[0])

# ---------------------------------------------------------------------------------------------------------------------------------
# inputs, per model, seeded by M
# ---------------------------------------------------------------------------------------------------------------------------------
SEAM_SHARPEN = 3.0
SEAM_WIDTHS = (4, 3, 5, 2, 6)                  # nodes s-w+1 .. s+w; the first is the width every model starts from
SEAM_ROUND = 6                                 # candidates drawn per width
SEAM_CYCLES = 4                                # times the widths are gone through: a seam beside a node of flat emissions needs more draws
SEAM_WANTED = 3                                # ... until this many meet the condition (2 are required)
SEAM_FLANKS = (0, 3, 7, 12, 18, 25)            # flank lengths in turn, left and right out of step: the seam falls at different rows
_tmp = None


def _tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="bath_ssv_shapes_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def match_bits(model):
    """[M+1][20] log2 odds of the model's match emissions against the background (row 0 unused)."""
    M = model.M
    mat = np.ctypeslib.as_array(model.hmm.contents.mat, shape=((M + 1) * 20,)).reshape(M + 1, 20).astype(np.float64)
    S = np.zeros((M + 1, 20))
    S[1:] = np.log2(np.maximum(mat[1:], 1e-300) / common.BG)
    return mat, S


def diagonal_max(S, x, cut=None):
    """The best ungapped diagonal segment of target x over the model's match scores S, in bits: Kadane along every diagonal, in
    float64.  cut = c: no segment steps from node c to node c+1.  cut = 0: no segment holds node 1."""
    M = S.shape[0] - 1
    H = np.zeros(M + 1)
    best = 0.0
    for r in x:
        prev = np.maximum(H[:-1], 0.0)          # prev[k]: the segment that ends in node k on the row before, or none
        if cut:
            prev[cut] = 0.0
        H = np.concatenate([[0.0], prev + S[1:, r]])
        if cut == 0:
            H[1] = 0.0
        best = max(best, float(H.max()))
    return best


def seam_cut(M, s):
    """Where the diagonals are cut for seam node s: right of s; for the last node left of it; a one-node model loses its node."""
    return s if s < M else (M - 1 if M > 1 else 0)


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(M):
    """Model, targets and the oracle's results for the M-node synthetic model, built once per model and left unchanged."""
    t0 = time.time()
    I = Inputs()
    I.M, (I.NR, I.G) = M, ssv_shape(M)
    I.path = common.write_synthetic_bhmm(os.path.join(_tmpdir(), "s%d.bhmm" % M), M, seed=M)
    I.model = model = ol.Model(I.path, 0)
    mat, S = match_bits(model)
    rng = np.random.default_rng(M)
    seqs = common.random_aa(rng, 40, 20, 300)
    for L in sorted(set(range(1, 10)) | {n + d for n in range(4, 41, 4) for d in (-1, 0, 1)}):   # the lane kernel reads 4 residues at a time, the ORF kernel 8
        seqs += common.random_aa(rng, 1, L, L)
    seqs += common.emit_from_model(rng, model, 10) + common.emit_from_model(rng, model, 6, sharpen=3.0)      # the statuses that are not OK
    # seam targets: an ungapped pass through nodes s-w+1 .. s+w (kept inside 1..M at full length), background flanks
    I.seams = ssv_seams(M, I.NR, I.G)
    I.seam_targets = {}                          # seam node -> [(index in seqs, qualifies)]
    for s, _ in I.seams:
        kept, n_good, j = [], 0, 0
        for w in SEAM_WIDTHS * SEAM_CYCLES:
            a = min(max(1, s - w + 1), max(1, M - 2 * w + 1))
            b = min(M, a + 2 * w - 1)
            for _ in range(SEAM_ROUND):
                q = mat[a:b + 1] ** SEAM_SHARPEN
                q /= q.sum(axis=1, keepdims=True)
                core = np.array([rng.choice(20, p=q[i]) for i in range(b - a + 1)], np.uint8)
                left = common.random_aa(rng, 1, SEAM_FLANKS[j % 6], SEAM_FLANKS[j % 6], with_degenerate=False)[0]
                right = common.random_aa(rng, 1, SEAM_FLANKS[(j // 2 + 3) % 6], SEAM_FLANKS[(j // 2 + 3) % 6], with_degenerate=False)[0]
                j += 1
                t = np.concatenate([left, core, right]).astype(np.uint8)
                _, st = common.oracle_scores(model, [t], "bo_ssvfilter")
                good = False
                if st[0] == 0:
                    whole = diagonal_max(S, t)
                    good = whole >= diagonal_max(S, t, seam_cut(M, s)) + 1.0 and whole >= max(diagonal_max(S, left), diagonal_max(S, right)) + 1.0
                kept.append((len(seqs), good))
                seqs.append(t)
                n_good += good
            if n_good >= SEAM_WANTED:
                break
        I.seam_targets[s] = kept
    if len(seqs) % 64 == 0:
        seqs += common.random_aa(rng, 1, 30, 30)
    I.seqs = seqs
    I.ssv = common.oracle_scores(model, seqs, "bo_ssvfilter")
    I.msv = common.oracle_scores(model, seqs, "bo_msvfilter")
    I.seconds = time.time() - t0
    return I


def seam_condition(I):
    """For every seam of the model, the number of seam targets that meet all three: the oracle's status is OK, the best diagonal
    loses at least 1 bit when the diagonals are cut at the seam, and it lies at least 1 bit above what the target's flanks reach on
    their own.  At least 2 per seam are required: a kernel that breaks the seam then changes a score the test compares.  The
    figures come from the oracle and diagonal_max alone."""
    ost = I.ssv[1]
    counts = {s: sum(1 for i, good in I.seam_targets[s] if good and ost[i] == 0) for s, _ in I.seams}
    short = {s: n for s, n in counts.items() if n < 2}
    assert not short, "M=%d (NR=%d, G=%d): seams with fewer than 2 targets that meet the condition: %s" % (I.M, I.NR, I.G, short)
    return counts


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def check_standalone(ctx, M):
    """ba.SSVFilter and ba.MSVFilter against the oracle over the model's targets; the seam targets by name."""
    I = inputs(M)
    seam_condition(I)
    om = ba.OProfile(ctx, ba.Profile(ba.HMM(I.path, 0)))
    blk = ba.SeqBlock(ctx, I.seqs)
    assert len(I.seqs) % 64 != 0
    osc, ost = I.ssv
    sc, st = ba.SSVFilter(ctx, om, blk)
    ok = ost == 0
    assert ok.sum() > 0
    for s, kind in I.seams:                                          # first, so that a failure names the seam
        for i, good in I.seam_targets[s]:
            assert st[i] == ost[i] and (ost[i] != 0 or _bits(sc[i]) == _bits(osc[i])), \
                "SSVFilter: seam target %d at the %s seam, node %d of M=%d (NR=%d, G=%d): %r / %d, oracle %r / %d" % (i, kind, s, M, I.NR, I.G, sc[i], st[i], osc[i], ost[i])
    assert np.array_equal(st, ost)
    assert np.array_equal(_bits(sc[ok]), _bits(osc[ok]))
    # one target alone: with G > 1 the wave's other groups are dead
    i1 = I.seam_targets[I.seams[-1][0]][0][0]
    sc1, st1 = ba.SSVFilter(ctx, om, ba.SeqBlock(ctx, I.seqs[i1:i1 + 1]))
    assert st1[0] == ost[i1] and (ost[i1] != 0 or _bits(sc1[0]) == _bits(osc[i1]))
    # the full MSV filter: the targets SSV leaves undecided go on through the wave kernel, which takes up to 2048 nodes; beyond
    # them the call is made on the targets SSV decides
    msc, mst = I.msv
    if M <= CASCADE_MAX_NODES:
        sc, st = ba.MSVFilter(ctx, om, blk)
        assert np.array_equal(st, mst) and np.array_equal(_bits(sc), _bits(msc))
    else:
        dec = np.flatnonzero(ost != 19)                              # eslENORESULT: undecided
        sc, st = ba.MSVFilter(ctx, om, ba.SeqBlock(ctx, [I.seqs[i] for i in dec]))
        assert np.array_equal(st, mst[dec]) and np.array_equal(_bits(sc[mst[dec] == 0]), _bits(msc[dec][mst[dec] == 0]))
    return I


N_RANDOM_WINDOWS = 6
N_SEAM_WINDOWS = 12


def cascade_windows(I):
    """About 6 random windows of 900 nt, and one window per seam target picked: the target's reverse translation between two stop
    codons, so that the target itself is an ORF, with flanks, every other one on the bottom strand.  The picks go in turn over the
    seams, targets that meet the seam condition first, until every seam has one and there are at least 12.
    Returns (windows, [(window, index of the target in I.seqs)])."""
    rng = np.random.default_rng(10000 + I.M)
    wins = common.random_dna(rng, N_RANDOM_WINDOWS, 900)
    picks, depth = [], 0
    while depth == 0 or (len(picks) < N_SEAM_WINDOWS and depth < SEAM_WANTED):
        for s, _ in I.seams:
            t = sorted(I.seam_targets[s], key=lambda e: not e[1])
            if depth < len(t) and (depth == 0 or len(picks) < N_SEAM_WINDOWS):
                picks.append(t[depth][0])
        depth += 1
    stop = np.array([3, 0, 0], np.uint8)                                   # TAA
    planted = []
    for n, i in enumerate(picks):
        nt = common.revtranslate(rng, I.seqs[i], I.model.basic)
        w = np.concatenate([rng.integers(0, 4, size=int(rng.integers(0, 90))).astype(np.uint8), stop, nt, stop, rng.integers(0, 4, size=int(rng.integers(0, 90))).astype(np.uint8)])
        planted.append((len(wins), i))
        wins.append((3 - w[::-1]).astype(np.uint8) if n % 2 else w)
    return wins, planted


def check_cascade(ctx, M):
    """ssv_orf_kernel through the cascade with F1 = 1.0, where every ORF is handed on and reported: status and score of every ORF."""
    I = inputs(M)
    om = ba.OProfile(ctx, ba.Profile(ba.HMM(I.path, 0)))
    wins, planted = cascade_windows(I)
    stats, res = ba.Pipeline(ctx, om, fs_pipe=False, F1=1.0, min_orf_len=5).run(ba.SeqBlock(ctx, wins))
    pli, ores, per_seq = I.model.run_pipeline(wins, opts={"F1": 1.0, "minlen": 5})
    assert stats.n_orfs == stats.n_past_msv == pli.n_orfs and pli.n_orfs == pli.n_past_msv, (stats.n_orfs, stats.n_past_msv, pli.n_orfs, pli.n_past_msv)
    want = {(w, r.strand, r.frame, r.start, r.end): r for w, (a, b) in enumerate(per_seq) for r in ores[a:b]}
    assert len(want) == len(ores) == pli.n_orfs == len(res)
    n_ok = n_short = 0
    for g in res:
        key = (int(g["window"]), int(g["strand"]), int(g["frame"]), int(g["start"]), int(g["end"]))
        o = want.pop(key)
        assert g["msv_status"] == o.msv_status and _bits(g["usc"]) == _bits(o.usc), \
            "M=%d (NR=%d, G=%d) ORF %r of %d residues: %r / %d, oracle %r / %d" % (M, I.NR, I.G, key, o.n, g["usc"], g["msv_status"], o.usc, o.msv_status)
        n_ok += o.msv_status == 0
        n_short += o.n < 8
    assert not want and n_ok > 0 and n_short > 0        # ORFs shorter than one 8-residue read are there
    # every planted seam target is an ORF of its own, with the standalone oracle's SSV result: what the seam condition says of the
    # target holds for a record compared above
    by_window = {}
    for w, (a, b) in enumerate(per_seq):
        by_window[w] = ores[a:b]
    osc, ost = I.ssv
    for w, i in planted:
        if len(I.seqs[i]) >= 5:
            assert any(o.n == len(I.seqs[i]) and (ost[i] != 0 or (o.msv_status == 0 and _bits(o.usc) == _bits(osc[i]))) for o in by_window[w]), (M, w, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEFAULT_CASES, ids=case_id)
def test_ssv_standalone_every_shape(gpu_ctx, case):
    """ssv_lane_kernel<NR, G> at both ends of every shape's model range: ba.SSVFilter against bo_ssvfilter, status of every target
    and score bits wherever the status is OK, and ba.MSVFilter against bo_msvfilter (d_msv shares the tile layout up to NR = 76).
    The seam condition is asserted first, from the oracle alone."""
    M, NR, G = case
    assert ssv_shape(M) == (NR, G)
    I = check_standalone(gpu_ctx, M)
    print("M=%d NR=%d G=%d targets=%d OK=%d seams=%d inputs %.2f s" % (M, NR, G, len(I.seqs), (I.ssv[1] == 0).sum(), len(I.seams), I.seconds))


@pytest.mark.parametrize("case", CASCADE_CASES, ids=case_id)
def test_ssv_cascade_every_shape(gpu_ctx, case):
    """ssv_orf_kernel<NR, G> at both ends of every shape's model range up to the cascade's 2048 nodes: at F1 = 1.0 the emission
    table's threshold is -128, every ORF becomes a candidate and a record, and each one's status and MSV score bits are the
    oracle's.  min_orf_len = 5 brings in ORFs shorter than one 8-residue read.  (144, 8) and (160, 8) serve models beyond 2048 nodes:
    the standalone test is what reaches them."""
    M, NR, G = case
    check_cascade(gpu_ctx, M)


@pytest.mark.parametrize("M", [SSV_MAX_NODES + 1, OPROFILE_MAX_NODES])
def test_standalone_filters_refuse_a_table_beyond_the_lds(gpu_ctx, M):
    """An OProfile holds up to 3328 nodes (ssv_bath_kernel<52> needs them), the SSV cost table of a workgroup's 160 KB of LDS 2560:
    ba.SSVFilter and ba.MSVFilter refuse a longer model on the host, before any launch, with the limit in the message, and the
    context goes on to score a 2560-node model to the oracle's bits."""
    path = common.write_synthetic_bhmm(os.path.join(_tmpdir(), "s%d.bhmm" % M), M, seed=M)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))
    blk = ba.SeqBlock(gpu_ctx, common.random_aa(np.random.default_rng(M), 10, 20, 60))
    for f in (ba.SSVFilter, ba.MSVFilter):
        with pytest.raises(ba.BathError, match=LDS_MESSAGE + ".*up to %d nodes" % SSV_MAX_NODES):
            f(gpu_ctx, om, blk)
    check_standalone(gpu_ctx, SSV_MAX_NODES)

