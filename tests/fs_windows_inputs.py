"""Inputs for the DNA-window builder and the branch decision of the frameshift stage (bath_fs_windows.hip), shared by
tests/test_fs_windows_cpu.py (the inputs reach what they claim) and tests/test_fs_windows_gpu.py (both drivers against the oracle).

Geometry is the oracle's own: random DNA through bo_translate_orfs on both strands gives the ORFs, their order on a strand and the
ORFs still open at the sequence end.  What a cascade would add is synthetic and seeded: which ORFs pass F4, P, the Forward and null
scores, and 0-4 hit windows per ORF (1 <= k - length + 1, k <= M).  The expectation is bo_fs_build_windows run (sequence, strand) by
(sequence, strand), and bo_fs_decide_window.  A case is built once per process and never changed."""
import ctypes as C
import ctypes.util
import os
import tempfile

import numpy as np

import bath_amd as ba
import common
import oracle_lib as ol

F3, F4 = 1e-5, 5e-4                                   # the pipeline's defaults
MINLEN = 12                                           # amino acids; short, so that a strand of a few 10 kb carries > 1024 ORFs
ORF_DT = np.dtype([("start", "<i4"), ("end", "<i4"), ("n", "<i4"), ("frame", "<i4"), ("off", "<i8")])               # bo_orf
WIN_DT = np.dtype([("id", "<i4"), ("n", "<i4"), ("k", "<i4"), ("length", "<i4"), ("score", "<f4")])                 # bo_window
FSW_DT = np.dtype([("n", "<i8"), ("length", "<i4"), ("k", "<i4"), ("orf_cnt", "<i4"), ("k_min", "<i4"), ("k_max", "<i4"), ("tot_orfsc", "<f4"),
                   ("P_min", "<f8"), ("P_tot", "<f8")], align=True)                                                 # bo_fsw

_tmp = tempfile.TemporaryDirectory(prefix="fsw_inputs_")
_models = {}


def model(key):
    """(path, oracle model): 'pth2' (M = 116) or 'm12', a 12-node synthetic model, so that ORFs with n >= M exist."""
    if key not in _models:
        path = ol.GOLDEN + "/PTH2.bhmm" if key == "pth2" else common.write_synthetic_bhmm(os.path.join(_tmp.name, "m12.bhmm"), 12, seed=12)
        _models[key] = (path, ol.Model(path, 0))
        L = ol.lib()
        L.bo_fs_build_windows.argtypes = [C.POINTER(ol.OrfBlock), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(ol.WindowList), C.c_int, C.c_int,
                                          C.POINTER(ol.OProfile), C.POINTER(ol.ScoreData), C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int32)]
        L.bo_fs_decide_window.argtypes = [C.POINTER(ol.Bg), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_float, C.c_float, C.c_float,
                                          C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.bo_fs_decide_window.restype = None
        C.CDLL(None).free.argtypes = [C.c_void_p]
    return _models[key]


def translate(m, codes, minlen=MINLEN):
    """The ORFs of both strands of one sequence, each strand in the order the oracle emits them: [ORF_DT array, ORF_DT array]."""
    L = ol.lib()
    n = len(codes)
    top = ol.dsq_from(codes)
    bot = np.empty_like(top)
    L.bo_revcomp(ol.u8(top), n, ol.u8(bot))
    out = []
    for dsq in (top, bot):
        blk = ol.OrfBlock()
        L.bo_orfblock_init(C.byref(blk))
        assert L.bo_translate_orfs(ol.u8(dsq), n, ol.u8(m.basic), minlen, C.byref(blk)) == 0
        a = np.frombuffer((C.c_char * (blk.count * ORF_DT.itemsize)).from_address(C.addressof(blk.orf.contents)), dtype=ORF_DT).copy() if blk.count else np.zeros(0, ORF_DT)
        L.bo_orfblock_free(C.byref(blk))
        out.append(a)
    return out


def oracle_group(m, orfs, P, fwdsc, wins, n_seq, strand, std_pipe=1):
    """bo_fs_build_windows on one (sequence, strand): orfs ORF_DT[all ORFs of the strand], P / fwdsc per ORF, wins WIN_DT (id = index into orfs).
    Returns (FSW_DT windows, per_orf int32 [norf][4] = window start, length, k, best hit window or -1)."""
    L = ol.lib()
    orfs = np.ascontiguousarray(orfs)
    blk = ol.OrfBlock(orfs.ctypes.data_as(C.POINTER(ol.Orf)), len(orfs), len(orfs), None, 0, 0)
    P = np.ascontiguousarray(P, np.float64)
    fwdsc = np.ascontiguousarray(fwdsc, np.float32)
    wins = np.ascontiguousarray(wins, WIN_DT)
    wl = ol.WindowList(wins.ctypes.data_as(C.POINTER(ol.Window)), len(wins), len(wins))
    out, nout = C.c_void_p(), C.c_int(0)
    per = np.zeros((max(len(orfs), 1), 4), np.int32)
    st = L.bo_fs_build_windows(C.byref(blk), P.ctypes.data_as(C.POINTER(C.c_double)), ol.f32(fwdsc), C.byref(wl), n_seq, strand, m.om, m.sd, F4, std_pipe,
                               C.byref(out), C.byref(nout), per.ctypes.data_as(C.POINTER(C.c_int32)))
    assert st == 0
    res = np.zeros(0, FSW_DT)
    if nout.value:
        res = np.frombuffer((C.c_char * (nout.value * FSW_DT.itemsize)).from_address(out.value), dtype=FSW_DT).copy()
        C.CDLL(None).free(out)
    return res, per[:len(orfs)]


def random_hits(rng, M, orf_n, per_orf=(0, 5)):
    """0-4 hit windows for each of the ORFs of lengths orf_n: (owner, n, k, length, score), an ORF's windows in the order the Viterbi filter
    emits them (by start; equal starts, which it never emits, by k).  Few distinct scores and lengths: ties of every kind are common."""
    cnt = rng.integers(per_orf[0], per_orf[1], size=len(orf_n))
    owner = np.repeat(np.arange(len(orf_n)), cnt)
    W = len(owner)
    length = rng.integers(1, min(M, 40) + 1, size=W) if M > 12 else rng.integers(1, M + 1, size=W)
    length[rng.random(W) < 0.5] = min(M, 9)
    k = length + (rng.random(W) * (M - length + 1)).astype(np.int64)
    n = 1 + (rng.random(W) * np.minimum(orf_n[owner], 6)).astype(np.int64) * np.maximum(orf_n[owner] // 6, 1)
    n = np.minimum(n, orf_n[owner])
    score = (rng.integers(0, 3, size=W) * 0.5).astype(np.float32)
    order = np.lexsort((k, n, owner))
    return owner[order], n[order], k[order], length[order], score[order]


class Case:
    """One block: sequences, the lanes' lists (cands / wins per lane, ids the lane's own), and what the oracle makes of them."""

    def __init__(self, name, mkey, seqs, std_pipe=1):
        self.name, self.mkey, self.seqs, self.std_pipe = name, mkey, seqs, std_pipe
        self.accepts = True                                # the device driver takes the block

    def lanes(self, shuffle=None):
        """[(cands, wins, cand_base, first_window, dpool)]; shuffle: a seed -- every list in another order, as the select kernels leave them."""
        out = []
        rng = np.random.default_rng(shuffle) if shuffle is not None else None
        for c, w, base, first, dpool in self._lanes:
            if rng is not None:
                c, w = c[rng.permutation(len(c))], w[rng.permutation(len(w))]
            out.append((c, w, base, first, dpool))
        return out


def build_case(name, mkey, rng, specs, K=1, empty=(), hits="random", edit=None, std_pipe=1, minlen=MINLEN, seqs=None):
    """specs: per sequence (length, {strand: (count or None = every ORF, 'dense' | 'sparse' | 'medium')}).  K lanes, those in <empty> without a
    sequence.  hits: 'random' (0-4 per ORF), 'none', or ('range', lo, hi): lo..hi windows for every ORF.  edit(case, owner, n, k, length, score, E) -> the same five arrays,
    changed: a case's own hit windows (E: the expected ORFs before their windows are known)."""
    path, m = model(mkey)
    M = m.M
    case = Case(name, mkey, [], std_pipe)
    groups = []                                            # (seq, strand, ORF_DT all, surviving indices)
    for si, (length, want) in enumerate(specs):
        codes = seqs[si] if seqs is not None else rng.integers(0, 4, size=length).astype(np.uint8)
        case.seqs.append(codes)
        per_strand = translate(m, codes, minlen)
        for strand in (0, 1):
            if strand not in want:
                continue
            count, mode = want[strand]
            all_orfs = per_strand[strand]
            tot = len(all_orfs)
            count = tot if count is None else count
            assert tot >= count, (name, si, strand, tot, count)
            if mode == "dense":
                a = int(rng.integers(0, tot - count + 1))
                idx = np.arange(a, a + count)
            elif mode == "sparse":
                idx = np.unique(np.linspace(0, tot - 1, count).astype(np.int64))
                assert len(idx) == count
            else:
                idx = np.sort(rng.choice(tot, count, replace=False))
            if count:
                groups.append((si, strand, all_orfs, idx))
    # ---- the survivors in the expected order: sequence, strand, the oracle's emission order
    n = sum(len(g[3]) for g in groups)
    E = np.zeros(n, ba.FS_ORF_DTYPE)
    gi = np.zeros(n, np.int64)
    pos = 0
    for g, (si, strand, all_orfs, idx) in enumerate(groups):
        s = slice(pos, pos + len(idx))
        o = all_orfs[idx]
        E["w"][s], E["strand"][s], E["start"][s], E["end"][s], E["n"][s] = si, strand, o["start"], o["end"], o["n"]
        E["g0"][s], E["g1"][s] = pos, pos + len(idx)
        gi[s] = g
        pos += len(idx)
    E["P"] = np.where(rng.random(n) < 0.5, 10.0 ** rng.uniform(-12, -5.1, n), 10.0 ** rng.uniform(-4.9, np.log10(F4) - 0.01, n))
    fwd = rng.uniform(5.0, 60.0, n).astype(np.float32)
    nul = rng.uniform(-3.0, 0.0, n).astype(np.float32)
    E["fwd_null"] = fwd - nul
    local_off = rng.integers(0, 1 << 20, n) * 16
    # ---- hit windows
    if hits == "none":
        owner = hn = hk = hl = np.zeros(0, np.int64); hs = np.zeros(0, np.float32)
    else:
        owner, hn, hk, hl, hs = random_hits(rng, M, E["n"].astype(np.int64), (hits[1], hits[2] + 1) if isinstance(hits, tuple) else (0, 5))
    if edit is not None:
        owner, hn, hk, hl, hs = edit(case, owner, hn, hk, hl, hs, E)
        order = np.lexsort((hk, hn, owner))
        owner, hn, hk, hl, hs = owner[order], hn[order], hk[order], hl[order], hs[order]
    assert (hk <= M).all() and (hk - hl + 1 >= 1).all() and (hl >= 1).all()
    E["kmin"], E["kmax"] = M, 0
    np.minimum.at(E["kmin"], owner, (hk - hl + 1).astype(np.int32))
    np.maximum.at(E["kmax"], owner, hk.astype(np.int32))
    found = np.zeros(n, bool)
    found[owner] = True
    # ---- lanes: consecutive sequences; candidate ids the lane's own, with gaps (the cascade's candidates that did not pass F4)
    live = [k for k in range(K) if k not in empty]
    nseq = len(specs)
    assert len(live) >= 1
    bounds = np.linspace(0, nseq, len(live) + 1).astype(np.int64)
    case._lanes, base = [], 0
    cand_global = np.zeros(n, np.int64)
    for k in range(K):
        if k in empty:
            case._lanes.append((np.zeros(0, ba.FS_CAND_DTYPE), np.zeros(0, ba.FS_HITWIN_DTYPE), base, 0, 0))
            base += 7
            continue
        j = live.index(k)
        lo, hi = int(bounds[j]), int(bounds[j + 1])
        sel = np.flatnonzero((E["w"] >= lo) & (E["w"] < hi))
        ncand = 3 * len(sel) + 5
        local = rng.choice(ncand, len(sel), replace=False)
        dpool = int(k) << 34
        c = np.zeros(len(sel), ba.FS_CAND_DTYPE)
        c["window"], c["aa_off"], c["P"], c["cand"] = E["w"][sel] - lo, local_off[sel], E["P"][sel], local
        c["sf"], c["startj"], c["len"] = E["strand"][sel] * 3 + (E["start"][sel] - 1) % 3, (E["start"][sel] - 1) // 3, E["n"][sel]
        c["fwdsc"], c["nullsc"], c["fxoff"] = fwd[sel], nul[sel], -1
        cand_global[sel] = base + local
        E["aa_off"][sel] = local_off[sel] + dpool
        inv = np.full(n, -1, np.int64)
        inv[sel] = local
        mine = inv[owner] >= 0
        w = np.zeros(int(mine.sum()), ba.FS_HITWIN_DTYPE)
        w["cand"], w["n"], w["k"], w["length"], w["score"] = inv[owner[mine]], hn[mine], hk[mine], hl[mine], hs[mine]
        case._lanes.append((c, w, base, lo, dpool))
        base += ncand
    E["cand"] = cand_global
    case.nc_total = base
    case.n, case.nhw = n, len(owner)
    # ---- the oracle, (sequence, strand) by (sequence, strand)
    wins_out, grp = [], []
    per_orf = np.zeros((n, 4), np.int32)
    hw_lo = np.searchsorted(owner, np.arange(n), side="left")
    hw_hi = np.searchsorted(owner, np.arange(n), side="right")
    pos = 0
    case.group_sizes = []
    for g, (si, strand, all_orfs, idx) in enumerate(groups):
        cnt = len(idx)
        P_all = np.full(len(all_orfs), 1.0)                # the ORFs that did not pass F4 stay in the block: the oracle's own test drops them
        P_all[idx] = E["P"][pos:pos + cnt]
        P_all[np.setdiff1d(np.arange(len(all_orfs)), idx)] = 10.0 ** rng.uniform(np.log10(F4) + 0.01, 0, len(all_orfs) - cnt)
        f_all = np.zeros(len(all_orfs), np.float32)
        f_all[idx] = E["fwd_null"][pos:pos + cnt]
        a, b = int(hw_lo[pos]), int(hw_hi[pos + cnt - 1])
        w = np.zeros(b - a, WIN_DT)
        w["id"], w["n"], w["k"], w["length"], w["score"] = idx[owner[a:b] - pos], hn[a:b], hk[a:b], hl[a:b], hs[a:b]
        res, per = oracle_group(m, all_orfs, P_all, f_all, w, len(case.seqs[si]), strand, std_pipe)
        per_orf[pos:pos + cnt] = per[idx]
        r = np.zeros(len(res), ba._np_dtype(ba.FsWindow))
        r["window"], r["strand"], r["n"], r["length"] = si, strand, res["n"], res["length"]
        for f in ("orf_cnt", "k_min", "k_max", "tot_orfsc", "P_min", "P_tot"):
            r[f] = res[f]
        wins_out.append(r)
        grp += [(pos, pos + cnt)] * len(res)
        case.group_sizes.append(cnt)
        pos += cnt
    E["dw_n"], E["dw_len"], E["dw_k"] = per_orf[:, 0], per_orf[:, 1], per_orf[:, 2]
    assert np.array_equal(per_orf[:, 3] >= 0, found)
    case.orfs, case.found = E, found
    case.hits = (owner, hn, hk, hl, hs)
    case.windows = np.concatenate(wins_out) if wins_out else np.zeros(0, ba._np_dtype(ba.FsWindow))
    case.grp = np.array(grp, np.int32).reshape(-1, 2)
    case.nw = len(case.windows)
    case.M, case.max_length = M, m.om.contents.max_length
    return case


def pool_pitch(length):
    """A window's copy in the pool: padded to 16 bytes, plus 16."""
    return (np.asarray(length, np.int64) + 15) // 16 * 16 + 16


# ---- what the case list is made of
def spread(n, per=64, seq_len=6000):
    """n survivors as medium groups of <per> on the top strand of sequences of <seq_len> nt, the rest on the last sequence's bottom strand."""
    specs = []
    if n > 600:
        # small groups first: several group starts within one thread's run of the scan, and every later group off a multiple of its size
        for c in (1, 2, 3, 5, 7):
            specs.append((1500, {c % 2: (c, "medium")}))
            n -= c
    specs += [(seq_len, {0: (per, "medium")}) for _ in range(n // per)]
    if n % per:
        specs.append((seq_len, {1: (n % per, "medium")}))
    return specs


def size_case(n):
    """A block of exactly n surviving ORFs (the rank grid, the scans' tails, the ORF cap)."""
    rng = np.random.default_rng(1000 + n)
    if n <= 2:
        c = build_case("n%d" % n, "pth2", rng, [(1500, {0: (1, "medium")}), (1500, {1: (1, "medium")})][:n])
    elif n == 2049:
        # one sparse survivor per sequence: 2049 windows, three per thread in the scan and the layout
        c = build_case("n2049", "pth2", rng, [(400, {int(i % 2): (1, "medium")}) for i in range(2049)])
    else:
        # (0-3 hit windows per ORF from 32768 ORFs on: the block's hit windows stay under their own cap of 65536)
        c = build_case("n%d" % n, "pth2", rng, spread(n, 64 if n < 4096 else 256, 6000 if n < 4096 else 24000), hits=("range", 0, 3 if n >= 32768 else 4))
    assert c.n == n
    c.accepts = n <= 32768
    return c


def group_case(size):
    """One (sequence, strand) group of <size> survivors, every ORF of a run surviving (dense: fuse chains run into the cap), beside a small
    group on the other strand and small sequences around it."""
    rng = np.random.default_rng(2000 + size)
    specs = [(3000, {0: (3, "medium"), 1: (2, "medium")}), (110000, {0: (size, "dense"), 1: (5, "sparse")}), (3000, {0: (4, "medium")})]
    c = build_case("group%d" % size, "pth2", rng, specs)
    c.accepts = size <= 1024
    return c


def straddle_case():
    """A 1024-ORF group that starts at ORF 37 of the block: the other strand of its sequence before it, the same strand of the next sequence after it."""
    rng = np.random.default_rng(2100)
    return build_case("straddle", "pth2", rng, [(110000, {0: (37, "sparse"), 1: (1024, "dense")}), (9000, {1: (50, "medium")})])


def density_case():
    """A dense, a sparse and a medium group on sequences long enough for each."""
    rng = np.random.default_rng(2200)
    return build_case("density", "pth2", rng, [(30000, {0: (300, "dense"), 1: (6, "sparse")}), (30000, {0: (100, "medium"), 1: (200, "dense")})])


def lanes_case(K, empty=()):
    rng = np.random.default_rng(2300 + K)
    specs = [(5000, {0: (20 + i, "medium"), 1: (3 + i % 4, "medium")}) for i in range(20)]
    c = build_case("lanes%d" % K, "pth2", rng, specs, K=K, empty=empty)
    c.accepts = K <= 16
    return c


def nohits_case():
    rng = np.random.default_rng(2400)
    return build_case("nohits", "pth2", rng, [(5000, {0: (40, "medium"), 1: (30, "dense")}), (900, {0: (2, "medium")})], hits="none")


def hitwins_case(total):
    """65536 hit windows, the most the kernels take, and 65537: 16384 ORFs with four each (and one with a fifth)."""
    rng = np.random.default_rng(2500)

    def edit(case, owner, n, k, length, score, E):
        extra = total - len(owner)
        assert 0 <= extra <= 1
        if extra:
            j = len(owner) // 2
            owner, n, k, length, score = (np.append(a, a[j]) for a in (owner, n, k, length, score))
        return owner, n, k, length, score
    c = build_case("hitwins%d" % total, "pth2", rng, spread(16384, 256, 24000), hits=("range", 4, 4), edit=edit)
    assert c.nhw == total
    c.accepts = total <= 65536
    return c


TIE_KINDS = ("none_short", "none_long", "score_length", "score_length_start", "full_k")


def ties_case():
    """The per-ORF hit-window rules on the 12-node model (ORFs with n >= M and n < M exist): ORFs 0-4 of the first group carry, in TIE_KINDS'
    order, no window with n < M, none with n >= M, a score tie the longer window wins, a score and length tie the leftmost wins, and windows
    equal in score, length and start that differ only in k (the smallest k wins: DESIGN.md 4.5d).  The winner is never the first listed."""
    rng = np.random.default_rng(2600)
    M = model("m12")[1].M
    case_box = {}

    def edit(case, owner, n, k, length, score, E):
        on = E["n"]
        short = np.flatnonzero(on < M)
        long_ = np.flatnonzero(on >= M)
        assert len(short) >= 4 and len(long_) >= 1
        pick = {"none_short": short[0], "none_long": long_[0], "score_length": short[1], "score_length_start": short[2], "full_k": short[3]}
        keep = ~np.isin(owner, list(pick.values()))
        owner, n, k, length, score = owner[keep], n[keep], k[keep], length[keep], score[keep]
        add = []
        a = pick["score_length"]
        add += [(a, 1, 5, 3, 2.0), (a, 2, 9, 6, 2.0), (a, 3, 4, 2, 1.5)]                       # the longer of the two best scores, listed second
        a = pick["score_length_start"]
        add += [(a, 1, 7, 2, 0.5), (a, 3, 8, 4, 1.0), (a, 5, 11, 4, 1.0)]                       # best score and length twice: the leftmost
        a = pick["full_k"]
        add += [(a, 1, 3, 2, 0.0), (a, 2, 10, 5, 3.0), (a, 2, 6, 5, 3.0), (a, 2, 8, 5, 3.0)]   # equal but for k: 6 wins
        for o, wn, wk, wl, ws in add:
            owner, n, k, length, score = np.append(owner, o), np.append(n, wn), np.append(k, wk), np.append(length, wl), np.append(score, np.float32(ws))
        case_box["pick"] = pick
        return owner, n, k, length, score.astype(np.float32)
    c = build_case("ties", "m12", rng, [(4000, {0: (60, "medium"), 1: (60, "medium")}), (2500, {0: (30, "dense")})], edit=edit, minlen=5)
    c.pick = case_box["pick"]
    return c


def open_ends_case():
    """Sequences that end inside a stop-free stretch on both strands: ORFs open at the sequence end, frame by frame, and windows clamped at
    position 1 and at the sequence end on both strands."""
    rng = np.random.default_rng(2700)
    sense = np.array([c for c in range(64) if c not in (48, 50, 56)])                     # no TAA, TAG, TGA
    seqs = []
    for _ in range(3):
        mid = rng.integers(0, 4, size=2400).astype(np.uint8)
        cod = sense[rng.integers(0, len(sense), size=40)]
        tail = np.stack([cod >> 4, (cod >> 2) & 3, cod & 3], 1).reshape(-1).astype(np.uint8)
        head = (3 - tail[::-1]).astype(np.uint8)                                             # its reverse complement ends the bottom strand
        seqs.append(np.concatenate([head, mid, tail, rng.integers(0, 4, size=int(rng.integers(0, 3))).astype(np.uint8)]))
    return build_case("open_ends", "pth2", rng, [(len(s), {0: (None, "dense"), 1: (None, "dense")}) for s in seqs], seqs=seqs)


def far_start_case():
    """One 4 Mnt sequence whose top strand is stop-free in frame 0: an ORF of 1.4 M residues, with a hit window that starts beyond 0xfffff --
    more than the kernels' key holds.  The block goes to the host path."""
    rng = np.random.default_rng(2800)
    sense = np.array([c for c in range(64) if c not in (48, 50, 56)])
    cod = sense[rng.integers(0, len(sense), size=1400000)]
    seq = np.stack([cod >> 4, (cod >> 2) & 3, cod & 3], 1).reshape(-1).astype(np.uint8)

    def edit(case, owner, n, k, length, score, E):
        big = int(np.argmax(E["n"]))
        assert E["n"][big] > 0x100000 + 100
        return np.append(owner, big), np.append(n, 0x100000 + 77), np.append(k, 60), np.append(length, 20), np.append(score, np.float32(9.0))
    c = build_case("far_start", "pth2", rng, [(len(seq), {0: (40, "sparse"), 1: (25, "sparse")})], edit=edit, minlen=150, seqs=[seq])
    c.big = int(np.argmax(c.orfs["n"]))
    c.accepts = False
    return c


def fsonly_case():
    rng = np.random.default_rng(2900)
    return build_case("fsonly", "pth2", rng, [(8000, {0: (70, "medium"), 1: (90, "dense")})], std_pipe=0)


# (8193: the first n at which the rank grid has fewer column ranges than tiles on 256 compute units, 33 tiles over 31; 8449: 34 over 30)
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 8192, 8193, 8449, 32768, 32769)
GROUPS = (1023, 1024, 1025)
MAKERS = dict([("n%d" % n, (size_case, n)) for n in SIZES] + [("group%d" % g, (group_case, g)) for g in GROUPS] +
              [("straddle", (straddle_case,)), ("density", (density_case,)), ("nohits", (nohits_case,)), ("ties", (ties_case,)),
               ("open_ends", (open_ends_case,)), ("far_start", (far_start_case,)), ("fsonly", (fsonly_case,)),
               ("hitwins65536", (hitwins_case, 65536)), ("hitwins65537", (hitwins_case, 65537)),
               ("lanes1", (lanes_case, 1)), ("lanes2", (lanes_case, 2)), ("lanes3", (lanes_case, 3, (1,))),
               ("lanes16", (lanes_case, 16, (0, 7, 15))), ("lanes17", (lanes_case, 17, (0, 8, 16)))])
CASES = tuple(MAKERS)
_cases = {}


def case(name):
    if name not in _cases:
        f = MAKERS[name]
        _cases[name] = f[0](*f[1:])
    return _cases[name]


def first_split_n(cus):
    """The smallest n at which fsw_rank_kernel's grid has fewer column ranges than tiles, and they do not divide the tiles evenly."""
    gn = 1
    while True:
        cols = max(1, min(gn, (cus * 4) // gn))
        if cols < gn and gn % cols != 0:
            return (gn - 1) * 256 + 1
        gn += 1


def planted_block(ngenes=300):
    """For the end-to-end case: one sequence of about 120 kb carrying <ngenes> planted PTH2 genes on both strands, most with one to three
    single-nucleotide insertions or deletions, and a few short sequences."""
    rng = np.random.default_rng(4000)
    m = model("pth2")[1]
    genes = common.emit_from_model(rng, m, ngenes // 2, flank=5) + common.emit_from_model(rng, m, ngenes - ngenes // 2, flank=5, sharpen=2.0)
    parts = []
    for i, aa in enumerate(genes):
        nt = list(common.revtranslate(rng, aa, m.basic))
        for _ in range(int(rng.integers(0, 4))):
            p = int(rng.integers(10, max(11, len(nt) - 10)))
            if rng.random() < 0.5:
                del nt[p]
            else:
                nt.insert(p, int(rng.integers(0, 4)))
        g = np.array(nt, dtype=np.uint8)
        if i % 2:
            g = (3 - g[::-1]).astype(np.uint8)
        parts += [g, rng.integers(0, 4, size=int(rng.integers(20, 160))).astype(np.uint8)]
    big = np.concatenate(parts)
    short = [np.concatenate([rng.integers(0, 4, size=80).astype(np.uint8), parts[2 * j], rng.integers(0, 4, size=50).astype(np.uint8)]) for j in (0, 1, 2)]
    return [short[0], big, short[1], short[2]] + common.random_dna(rng, 2, 700)


# ---- the branch decision
DECIDE_DT = ba._np_dtype(ba.FsWindow)
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = C.c_float, [C.c_float]


def _logf(x):
    return _libm.logf(C.c_float(x))


def decide_fac(lam, fsc):
    """test_fs_pipeline_gpu.compare's factor: how far a P-value may move with the Forward score's tolerance."""
    tol = 5e-3 + 1e-4 * abs(float(fsc))
    return float(np.exp(lam * (tol + 1e-3) / np.log(2.0)) * 1.001)


def decide_cases(do_biasfilter=1, std_pipe=1):
    """Records as a build leaves them, bias[nw][2][3], fsc[nw]; the oracle's nullsc, filtersc, P_fs, P_null and branch; and per record its kind:
    'clear' (P_fs against F3 and P_null against P_tot apart by at least the factor of decide_fac) or 'tied' (P_null == P_tot == 1.0 exactly,
    through the x < tau -> 1.0 clamp).  Records of neither kind are not made."""
    path, m = model("pth2")
    L = ol.lib()
    gm3 = m.fs(3).contents
    tau3, lam = float(gm3.evparam[6]), float(gm3.evparam[5])
    rng = np.random.default_rng(3000 + 2 * do_biasfilter + std_pipe)
    rec, bias, fsc, kinds, want = [], [], [], [], []
    lengths = [0, 1, 2, 3, 4, 5, 6, 7, 8] + [int(x) for x in rng.integers(60, 3000, size=400)]        # L3 = 0, 1, 2 and typical values
    for i, length in enumerate(lengths):
        L3 = length // 3
        r = np.zeros(1, DECIDE_DT)[0]
        r["window"], r["strand"], r["n"], r["length"] = i % 7, i % 2, 1 + i, length
        tie = i % 5 == 4
        r["orf_cnt"] = 1 + (i // 5) % 2 if tie else int(rng.integers(1, 5))
        if i % 3 == 0:
            r["k_min"], r["k_max"] = m.M, 0                                                            # no hit window: no local pass
        else:
            r["k_min"] = int(rng.integers(1, m.M)); r["k_max"] = int(rng.integers(r["k_min"], m.M + 1))
        r["tot_orfsc"] = np.float32(rng.uniform(5, 60))
        r["P_min"] = 10.0 ** rng.uniform(-12, np.log10(F4))
        r["P_tot"] = 1.0 if (tie or not std_pipe) else 10.0 ** rng.uniform(-14, -2)
        b = rng.uniform(-4.0, 1.0, size=(2, 3)).astype(np.float32) - np.float32(1.1 * L3 / max(L3, 1))
        if tie and i % 20 in (4, 9):
            b -= np.float32(22.0)        # a filter score far below the null score: P_fs <= F3 although P_null is 1.0, and the P_min > F3 clause decides
        nullsc = np.float32(np.float32(L3 * np.log(L3 / (L3 + 1.0)) + np.log(1.0 - L3 / (L3 + 1.0))) + np.log(3.0)) if L3 > 0 else np.float32(np.log(3.0))
        # a Forward score well above or well below what F3 asks for; tied records: below tau3 against the null, so P_null is clamped to 1.0
        f = np.float32(nullsc + np.log(2.0) * (tau3 - rng.uniform(2.0, 6.0))) if tie else np.float32(nullsc + np.log(2.0) * (tau3 + rng.uniform(-8.0, 40.0)))
        out = [C.c_float(), C.c_float(), C.c_double(), C.c_double(), C.c_int()]
        bg = ol.Bg.from_buffer_copy(m.bg)
        sums = []
        for p in range(2):
            s = np.float32(-np.inf)
            for x in b[p]:
                s = np.float32(L.bo_flogsum(s, x))
            p1 = np.float32(L3) / np.float32(L3 + 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                # p7_bg.c:561 as bo_bg_fs_filterscore has it, with libm's logf (numpy's own float32 log is not libm's to the last bit)
                term = np.float32(np.float32(np.float32(L3) * np.float32(_logf(p1))) + np.float32(_logf(np.float32(1.0 - np.float64(p1)))))
                sums.append(np.float32(np.float64(s) + (np.float64(term) + np.log(3.0))))
        L.bo_fs_decide_window(C.byref(bg), length, int(r["k_min"]), int(r["k_max"]), int(r["orf_cnt"]), float(r["P_tot"]), float(r["P_min"]),
                              C.c_float(sums[0]), C.c_float(sums[1]), C.c_float(f), do_biasfilter, std_pipe, F3, tau3, lam, *[C.byref(o) for o in out])
        nsc, filt, P_fs, P_null, branch = (o.value for o in out)
        fac = decide_fac(lam, f)
        clear_fs = P_fs > F3 * fac or P_fs < F3 / fac
        if np.isnan(P_fs) or np.isnan(P_null):
            # L3 = 0: 0 * log(0) makes the null score, and with it both P-values, NaN.  No comparison with a NaN holds, so the window
            # does not take the frameshift branch whatever the last bits are: as clear as a decision gets
            assert L3 == 0 and np.isnan(nsc) and branch != 1
            kind = "clear"
        elif tie:
            if not (P_null == 1.0 and r["P_tot"] == 1.0 and clear_fs):
                continue
            kind = "tied"
        else:
            if not (clear_fs and (P_null > r["P_tot"] * fac * fac or P_null < r["P_tot"] / (fac * fac))):
                continue
            kind = "clear"
        rec.append(r); bias.append(b); fsc.append(f); kinds.append(kind); want.append((nsc, filt, P_fs, P_null, branch))
    return np.array(rec, DECIDE_DT), np.array(bias, np.float32).reshape(-1, 2, 3), np.array(fsc, np.float32), kinds, want
