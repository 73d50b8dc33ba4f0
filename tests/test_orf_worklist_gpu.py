"""The length-sorted ORF work list itself (bath_hip_orf_worklist): what orf_sort_kernel leaves for the SSV kernel.

Each list is checked against the oracle's ORFs (oracle/translate.c): the same multiset of (window, strand*3+frame, first codon,
length), each record's aa_off at its place in the amino-acid stream layout aa + 2*off[w] + 96*w + sf*pitch(n), lengths in
non-increasing bins (ORFs of 2047 residues and more share the first bin) and as many entries as the pipeline counts.  Inputs:
the bench shape scaled down (many sort blocks), windows under 15 nt, ORFs crossing tile edges, long windows (the wave stitch
kernel), degenerate nucleotides, other minimum lengths, one strand and initiation codons (the filtered path)."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BINS = 2048


def pitch(n):
    return (n // 3 + 16) & ~15


def stream_bases(lens):
    """{(w, sf): pool offset of codon 0 of that stream}: aa + 2*off[w] + 96*w + sf*pitch(n), off[w] 16-byte aligned."""
    out, off = {}, 0
    for w, n in enumerate(lens):
        for sf in range(6):
            out[(w, sf)] = 2 * off + 96 * w + sf * pitch(n)
        off += (n + 15) // 16 * 16
    return out


def oracle_keys(windows, ct, minlen, strands, initiator):
    """Multiset of (w, sf, first codon index in the stream, length) of the oracle's ORFs."""
    L_ = ol.lib()
    basic = np.zeros(64, np.uint8)
    is_init = np.zeros(64, np.uint8)
    assert L_.bo_gencode_basic(ct, ol.u8(basic)) == 0
    if initiator:
        assert L_.bo_gencode_initiators(ct, initiator, ol.u8(is_init)) == 0
    keep = {ba.STRAND_BOTH: (0, 1), ba.STRAND_TOPONLY: (0,), ba.STRAND_BOTTOMONLY: (1,)}[strands]
    out = []
    blk = ol.OrfBlock(); L_.bo_orfblock_init(C.byref(blk))
    for w, codes in enumerate(windows):
        n = len(codes)
        if n < 15:
            continue
        d = ol.dsq_from(codes)
        rc = np.zeros(n + 2, np.uint8)
        L_.bo_revcomp(ol.u8(d), n, ol.u8(rc))
        for strand, dsq in ((0, d), (1, rc)):
            if strand not in keep:
                continue
            L_.bo_orfblock_reuse(C.byref(blk))
            L_.bo_translate_orfs_init(ol.u8(dsq), n, ol.u8(basic), ol.u8(is_init) if initiator else None, 1 if initiator else 0,
                                      minlen, C.byref(blk))
            for i in range(blk.count):
                o = blk.orf[i]
                out.append((w, 3 * strand + o.frame, (o.start - 1 - o.frame) // 3, o.n))
    L_.bo_orfblock_free(C.byref(blk))
    return sorted(out)


def worklist(gpu_ctx, windows, ct=1, minlen=20, strands=ba.STRAND_BOTH, initiator=ba.INIT_ANY):
    dna = ba.SeqBlock(gpu_ctx, [np.asarray(w, np.uint8) for w in windows])
    orfs = ba.translate_orfs(gpu_ctx, dna, ct, minlen, strands=strands, initiator=initiator)
    wl = ba.orf_worklist(gpu_ctx)
    assert len(wl) == len(orfs)
    return wl


def check(gpu_ctx, windows, ct=1, minlen=20, strands=ba.STRAND_BOTH, initiator=ba.INIT_ANY):
    wl = worklist(gpu_ctx, windows, ct, minlen, strands, initiator)
    lens = (wl["len_sf"].astype(np.int64) & 0x0FFFFFFF)
    sfs = (wl["len_sf"].astype(np.int64) >> 28) & 0xF
    # longest first, by bin
    bins = np.minimum(lens, BINS - 1)
    assert (np.diff(bins) <= 0).all()
    assert (lens >= max(minlen, 1)).all() and (sfs < 6).all()
    base = stream_bases([len(w) for w in windows])
    got = sorted((int(w), int(sf), int(a) - base[(int(w), int(sf))], int(n))
                 for w, sf, a, n in zip(wl["window"], sfs, wl["aa_off"], lens))
    want = oracle_keys(windows, ct, minlen, strands, initiator)
    assert len(got) == len(want), (len(got), len(want))
    assert got == want
    return wl


def rand_dna(rng, n, p_degen=0.0, stop_poor=False):
    if stop_poor:
        x = rng.choice(4, size=n, p=[0.04, 0.46, 0.46, 0.04]).astype(np.uint8)
    else:
        x = rng.integers(0, 4, size=n, dtype=np.uint8)
    if p_degen > 0:
        m = rng.random(n) < p_degen
        x[m] = rng.choice([5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], size=int(m.sum())).astype(np.uint8)
    return x


def test_bench_shape_scaled_down(gpu_ctx):
    rng = np.random.default_rng(11)
    wins = [rand_dna(rng, 1000) for _ in range(3000)]            # 9000 tiles: a dozen sort blocks
    wl = check(gpu_ctx, wins)
    assert len(wl) > 50000


def test_short_windows_and_tile_edges(gpu_ctx):
    rng = np.random.default_rng(12)
    lens = list(range(0, 40)) + [383, 384, 385, 386, 395, 767, 768, 769, 1151, 1152, 1153]
    wins = [rand_dna(rng, L) for L in lens for _ in range(4)]
    wins += [rand_dna(rng, L, stop_poor=True) for L in (2000, 3001, 5002)]
    check(gpu_ctx, wins)


def test_long_windows_stitch_wave(gpu_ctx):
    rng = np.random.default_rng(13)
    wins = [rand_dna(rng, 300_000)] + [rand_dna(rng, 100_001, stop_poor=True)] + [rand_dna(rng, 40_000) for _ in range(3)]
    wl = check(gpu_ctx, wins)
    assert (np.asarray(wl["len_sf"]) & 0x0FFFFFFF).max() > 200


def test_very_long_orfs_share_the_first_bin(gpu_ctx):
    # stop-free runs far longer than 2047 codons (C/G only): the first bin holds several lengths
    rng = np.random.default_rng(14)
    wins = [rng.choice([1, 2], size=L).astype(np.uint8) for L in (7000, 9001, 12002)] + [rand_dna(rng, 5000) for _ in range(4)]
    wl = check(gpu_ctx, wins)
    assert ((np.asarray(wl["len_sf"]) & 0x0FFFFFFF) >= BINS - 1).sum() >= 6


@pytest.mark.parametrize("p_degen", [0.01, 0.2])
def test_degenerate_nucleotides(gpu_ctx, p_degen):
    rng = np.random.default_rng(15)
    check(gpu_ctx, [rand_dna(rng, int(L), p_degen=p_degen) for L in rng.integers(10, 3000, size=400)])


@pytest.mark.parametrize("ct,minlen", [(1, 1), (1, 2), (1, 5), (4, 20), (11, 60)])
def test_other_min_lengths(gpu_ctx, ct, minlen):
    rng = np.random.default_rng(16 + minlen)
    check(gpu_ctx, [rand_dna(rng, int(L)) for L in rng.integers(10, 2000, size=300)], ct, minlen)


@pytest.mark.parametrize("strands,initiator", [(ba.STRAND_TOPONLY, ba.INIT_ANY), (ba.STRAND_BOTTOMONLY, ba.INIT_ANY),
                                               (ba.STRAND_BOTH, ba.INIT_AUG), (ba.STRAND_BOTH, ba.INIT_TABLE),
                                               (ba.STRAND_TOPONLY, ba.INIT_AUG)])
def test_filtered_path(gpu_ctx, strands, initiator):
    rng = np.random.default_rng(17 + strands + 3 * initiator)
    check(gpu_ctx, [rand_dna(rng, int(L)) for L in rng.integers(10, 3000, size=600)], strands=strands, initiator=initiator)


def test_counts_match_the_pipeline(gpu_ctx):
    # the work list is what the cascade's SSV stage runs over: as many entries as the pipeline's n_orfs
    rng = np.random.default_rng(18)
    wins = [rand_dna(rng, 1000) for _ in range(500)]
    wl = worklist(gpu_ctx, wins)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(ol.GOLDEN + "/Caudal_act.bhmm")))
    stats, _ = ba.Pipeline(gpu_ctx, om, fs_pipe=False).run(ba.SeqBlock(gpu_ctx, wins))
    assert stats.n_orfs == len(wl)
