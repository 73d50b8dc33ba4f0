"""Inputs for the quarter-wave translation kernel (orf_tile_kernel: a tile of 384 nt is owned by 16 lanes of 24 nt, 8 codons
per stream and lane), shared by tests/test_translate_quarter_gpu.py, which runs them, and tests/test_translate_quarter_cpu.py,
which checks from the oracle alone that they reach every seam they are meant to reach.

A case is (name, windows, genetic code, min_orf_len); every case is one translate_orfs call on one block of windows.
Nucleotide codes: A C G T = 0 1 2 3, degenerate codes 5..15."""
import ctypes as C

import numpy as np

LANE_NT = 24
TILE_NT = 384
A, Cc, G, T = 0, 1, 2, 3
FWD_STOP = (T, A, A)             # TAA on the top strand
REV_STOP = (T, T, A)             # the bytes, in memory order, of a TAA codon of the bottom strand


def rand_dna(rng, n, p=None, p_degen=0.0):
    x = rng.choice(4, size=n, p=p).astype(np.uint8) if p is not None else rng.integers(0, 4, size=n, dtype=np.uint8)
    if p_degen > 0:
        m = rng.random(n) < p_degen
        x[m] = rng.choice(np.arange(5, 16), size=int(m.sum())).astype(np.uint8)
    return x


def stop_free(rng, n):
    """C and G only: no stop codon in any of the six frames, in any genetic code used here."""
    return rng.choice(np.array([Cc, G], np.uint8), size=n)


def plant_stop(x, p, strand):
    """One stop codon of <strand> on the bytes p..p+2 of a C/G window, and no other stop in any frame: GTA / TAC around it
    keep the overlapping triplets off the other strand's stops (CTA is one of the bottom strand's, TAG one of the top's)."""
    if strand == 0:
        x[p:p + 3] = FWD_STOP
        if p > 0:
            x[p - 1] = G
    else:
        x[p:p + 3] = REV_STOP
        if p + 3 < len(x):
            x[p + 3] = Cc


SEAM_LENGTHS = list(range(15, 81)) + [c + d for c in (384, 768, 1152) for d in range(-26, 27)]
STOP_POOR = [0.12, 0.38, 0.38, 0.12]
STOP_RICH = [0.35, 0.15, 0.15, 0.35]


def stop_position_windows(rng):
    """For each strand and each in-lane position 0..23: a window of three tiles and a bit whose only stops sit at that position in
    lanes 0, 7 and 15 of the middle tile.  The ORF closed by the first comes out of the previous tile, the other two cross lanes."""
    wins = []
    for strand in (0, 1):
        for pos in range(LANE_NT):
            x = stop_free(rng, 3 * TILE_NT + 31 + pos)
            for lane in (0, 7, 15):
                plant_stop(x, TILE_NT + LANE_NT * lane + pos, strand)
            wins.append(x)
    return wins


def two_stop_windows(rng):
    """Two stops of one frame 1..7 codons apart inside one lane (lane 5 of the second tile), each strand, each phase."""
    wins = []
    for strand in (0, 1):
        for d in range(1, 8):
            for a in range(3):
                x = stop_free(rng, 2 * TILE_NT + 50)
                p = TILE_NT + LANE_NT * 5 + a
                plant_stop(x, p, strand)
                plant_stop(x, p + 3 * d, strand)
                wins.append(x)
    return wins


def cases():
    rng = np.random.default_rng(1624)
    out = []
    # window lengths: the last lane holds 1..24 valid nucleotides at every n mod 3, with and without a partial fourth tile
    out.append(("lengths_minlen20", [rand_dna(rng, L, STOP_POOR) for L in SEAM_LENGTHS], 1, 20))
    out.append(("lengths_minlen3", [rand_dna(rng, L) for L in SEAM_LENGTHS], 1, 3))
    # stop positions
    sp = stop_position_windows(rng)
    out.append(("stop_positions_minlen20", sp, 1, 20))
    out.append(("stop_positions_minlen5", sp, 1, 5))
    ts = two_stop_windows(rng)
    out.append(("two_stops_minlen1", ts, 1, 1))
    out.append(("two_stops_minlen7", ts, 1, 7))
    # minimum lengths on both sides of the "only the lane's first stop closes an ORF" shortcut (it holds for min_orf_len > 6)
    dense = [rand_dna(rng, int(L), STOP_RICH if k % 2 else None) for k, L in enumerate(rng.integers(100, 1300, size=16))]
    for minlen in (1, 2, 3, 4, 5, 6, 7, 8, 20):
        out.append(("dense_minlen%d" % minlen, dense, 1, minlen))
    # tile counts that leave quarter waves idle and are no multiple of four
    for nw in (1, 2, 3, 5, 7):
        lens = [100, 400, 250, 390, 383, 384, 157][:nw]
        out.append(("block_of_%d" % nw, [rand_dna(rng, L, STOP_POOR) for L in lens], 1, 20))
    # one degenerate nucleotide in one of a wave's four tiles sends all four down the 18^3-table path
    mixed = [rand_dna(rng, 300, STOP_POOR) for _ in range(9)]
    mixed[4][137] = 15                                # N
    out.append(("one_degenerate_between_canonical", mixed, 1, 20))
    out.append(("degenerate_30_percent", [rand_dna(rng, 1500, STOP_POOR, p_degen=0.3), rand_dna(rng, 411, None, p_degen=0.3)], 1, 5))
    # other genetic codes
    other = [rand_dna(rng, int(L)) for L in rng.integers(15, 1300, size=12)]
    out.append(("genetic_code_4", other, 4, 20))
    out.append(("genetic_code_11", other, 11, 6))
    return out


def oracle_orfs(windows, ct=1, minlen=20):
    """[(window, strand, frame, start, end, residues)] from the oracle (oracle/translate.c), sorted like the GPU list."""
    import oracle_lib as ol
    L_ = ol.lib()
    basic = np.zeros(64, np.uint8)
    assert L_.bo_gencode_basic(ct, ol.u8(basic)) == 0
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
            L_.bo_orfblock_reuse(C.byref(blk))
            L_.bo_translate_orfs(ol.u8(dsq), n, ol.u8(basic), minlen, C.byref(blk))
            if blk.count == 0:
                continue
            aa = np.ctypeslib.as_array(blk.aa, shape=(int(blk.aa_n),))
            for i in range(blk.count):
                o = blk.orf[i]
                out.append((w, strand, o.frame, o.start, o.end, aa[o.off + 1:o.off + 1 + o.n].copy()))
    L_.bo_orfblock_free(C.byref(blk))
    out.sort(key=lambda r: r[:4])
    return out


def memory_extent(n, strand, start, end):
    """0-based first and last byte of an ORF in the window as stored (coordinates are 1-based on the strand that was translated)."""
    return (start - 1, end - 1) if strand == 0 else (n - end, n - start)
