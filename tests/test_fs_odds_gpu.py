"""The odds-ratio mode of the 3-codon frameshift parsers (BATH_LOGSUM_ODDS, bath_fs_odds.hip): what the reference's
bathsearch --fs runs (impl_sse/fwdback_fs.c:97-533, :565-1050), held against

  * the scalar oracle on EXACT log-sums (bo_flogsum_set_exact(1)) at the reference's own SIMD-vs-generic bars with exact
    log-sums (fwdback_fs.c:3189-3191) as tests/test_sse_cpu.py applies them: scores within 1e-3 + 1e-4 |s|, special-state rows
    within 2e-3 + 2e-4 |v| where the oracle's value is above -60 (Backward: within 40 nats of the row's largest value).  The
    table-driven modes sit up to ~1.4e-2 nats from exact arithmetic on a 2500-nt window, so these bars are the odds mode's own;
  * the SSE odds oracle (oracle/sse/sse_fs.c), kernel by kernel and through the --fs pipeline (bo_fs_use_sse(1)).

The session's context stays in strict mode: every test that switches odds mode on switches it off in a finally."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol
from test_frameshift_gpu import fs_windows
from test_fs_pipeline_gpu import frameshifted_windows

pytestmark = pytest.mark.gpu

ERANGE = 16


def odds_windows(rng, model, n):
    wins = fs_windows(rng, model, n)
    deg = common.random_dna(rng, 1, 400)[0].copy()
    deg[50:70] = 15                                  # an N run
    deg[120] = 4; deg[200] = 7; deg[333] = 11        # ambiguity codes
    wins += [deg, common.random_dna(rng, 1, 2500)[0], common.random_dna(rng, 1, 3)[0], common.random_dna(rng, 1, 7)[0]]
    return wins


@pytest.fixture(scope="module", params=["Caudal_act", "2OG-FeII_Oxy_3", "PTH2", "synth1024", "synth1200"])
def setup(request, gpu_ctx, tmp_path_factory):
    name = request.param
    if name.startswith("synth"):
        M = int(name[5:])
        path = str(tmp_path_factory.mktemp("odds") / (name + ".bhmm"))
        common.write_synthetic_bhmm(path, M, seed=M, name=name)
        n = 3
    else:
        path = ol.GOLDEN + "/" + name + ".bhmm"
        n = 16
    model = ol.Model(path)
    hmm = ba.HMM(path)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3))
    wins = odds_windows(np.random.default_rng(7), model, n)
    blk = ba.SeqBlock(gpu_ctx, wins)
    fsc, fx = ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_ODDS, want_xmx=True)
    bsc, bx = ba.FS3BackwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_ODDS, want_xmx=True)
    return model, wins, (fsc, fx), (bsc, bx)


def exact_oracle(model, wins, backward):
    """Scalar oracle, exact log-sums: (status, score, rows) per window."""
    L_ = ol.lib()
    gm3 = model.fs(3)
    L_.bo_fs_profile_reconfig_multihit(gm3, 100)
    out = []
    f = C.c_float()
    L_.bo_flogsum_set_exact(1)
    try:
        for w in wins:
            L = len(w)
            d = ol.dsq_from(w)
            L_.bo_fs_profile_reconfig_length(gm3, L // 3)
            gx = L_.bo_gmx_create(model.M, L + 1, L, 3)
            fn = L_.bo_gbackward_parser_fs3 if backward else L_.bo_gforward_parser_fs3
            st = fn(ol.u8(d), L, gm3, gx, C.byref(f))
            out.append((st, f.value, np.ctypeslib.as_array(gx.contents.xmx, shape=(L + 1, 5)).copy()))
            L_.bo_gmx_free(gx)
    finally:
        L_.bo_flogsum_set_exact(0)
    return out


def sse_oracle(model, wins, backward):
    """oracle/sse/sse_fs.c: (status, score, rows in log space) per window."""
    L_ = ol.lib()
    gm3 = model.fs(3)
    L_.bo_fs_profile_reconfig_multihit(gm3, 100)
    L_.bs_fsprofile_create.restype = C.c_void_p
    L_.bs_fsprofile_free.argtypes = [C.c_void_p]
    fn = L_.bs_fs3_backward_parser if backward else L_.bs_fs3_forward_parser
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    so = L_.bs_fsprofile_create(gm3)
    assert so
    out = []
    g = C.c_float()
    for w in wins:
        L = len(w)
        d = ol.u8(ol.dsq_from(w))
        L_.bo_fs_profile_reconfig_length(gm3, L // 3)
        rows = np.zeros((L + 1) * 5, np.float32)
        st = fn(C.cast(d, C.c_void_p), L, so, rows.ctypes.data, C.byref(g))
        out.append((st, g.value, rows.reshape(L + 1, 5)))
    L_.bs_fsprofile_free(so)
    return out


def check_rows(g, o, backward):
    """The bars of tests/test_sse_cpu.py; returns the worst |delta| over the compared cells."""
    top = np.where(np.isfinite(o), o, -np.inf).max(axis=1, keepdims=True)
    if backward:
        live = np.isfinite(o) & (o > top - 40.0)
    else:
        # above -60, and within 60 nats of the row's largest value: fp32 odds ratios hold about 87 nats below the running scale,
        # so where a window scores hundreds of nats (the synthetic models) N(i) of the late rows underflows -- in the
        # reference's SSE parser too -- while its log value is still above -60
        live = np.isfinite(o) & (o > -60.0) & (o > top - 60.0)
        dead = ~np.isfinite(o)
        assert np.all(~np.isfinite(g[dead]) | (g[dead] < -50.0))
    assert not np.isnan(g).any()
    d = np.abs(g[live].astype(np.float64) - o[live])
    assert np.all(d <= 2e-3 + 2e-4 * np.abs(o[live])), float(d.max())
    return float(d.max()) if d.size else 0.0


def compare_parser(model, wins, got, want, backward):
    sc, xm = got
    worst_sc = worst_row = 0.0
    n_cmp = 0
    for w, s, x, (st, o, orow) in zip(wins, sc, xm, want):
        assert not np.isnan(s)
        if len(w) < 3:
            assert s == -np.inf
            continue
        if st == ERANGE or (st == 0 and not np.isfinite(o)):
            assert s == -np.inf
            continue
        if st != 0:                                  # (the scalar Backward refuses windows too short for its row cases)
            continue
        assert abs(s - o) <= 1e-3 + 1e-4 * abs(o), (len(w), s, o)
        worst_sc = max(worst_sc, abs(s - o))
        worst_row = max(worst_row, check_rows(x, orow, backward))
        n_cmp += 1
    assert n_cmp >= len(wins) - 4
    return worst_sc, worst_row


def test_forward_odds_vs_exact_oracle(setup):
    model, wins, fwd, _ = setup
    ws, wr = compare_parser(model, wins, fwd, exact_oracle(model, wins, False), False)
    assert max(len(w) for w in wins) >= 2500
    print("odds Forward vs exact oracle (M=%d): worst |delta| score %.2e, rows %.2e nats" % (model.M, ws, wr))


def test_forward_odds_vs_sse_oracle(setup):
    model, wins, fwd, _ = setup
    ws, wr = compare_parser(model, wins, fwd, sse_oracle(model, wins, False), False)
    print("odds Forward vs SSE odds oracle (M=%d): worst |delta| score %.2e, rows %.2e nats" % (model.M, ws, wr))


def test_backward_odds_vs_exact_oracle(setup):
    model, wins, fwd, bwd = setup
    ws, wr = compare_parser(model, wins, bwd, exact_oracle(model, wins, True), True)
    fsc, bsc = fwd[0], bwd[0]
    fin = np.isfinite(fsc) & np.isfinite(bsc)
    assert np.all(np.abs(fsc[fin] - bsc[fin]) <= 2e-3 + 2e-4 * np.abs(fsc[fin]))           # Forward == Backward
    assert np.array_equal(np.isfinite(fsc), np.isfinite(bsc))
    ws2, wr2 = compare_parser(model, wins, bwd, sse_oracle(model, wins, True), True)
    print("odds Backward (M=%d): worst |delta| vs exact %.2e / %.2e, vs SSE %.2e / %.2e (score / rows)" % (model.M, ws, wr, ws2, wr2))


def test_short_and_empty_windows_give_minus_inf(gpu_ctx):
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(ba.HMM(path), 3))
    rng = np.random.default_rng(2)
    wins = [rng.integers(0, 4, size=L).astype(np.uint8) for L in (1, 2, 3, 300)]
    blk = ba.SeqBlock(gpu_ctx, wins)
    for fn in (ba.FS3ForwardParser, ba.FS3BackwardParser):
        sc = fn(gpu_ctx, om3, blk, logsum=ba.LOGSUM_ODDS)
        assert sc[0] == -np.inf and sc[1] == -np.inf and np.isfinite(sc[2]) and np.isfinite(sc[3])


def test_context_mode_and_fs5_refusal(gpu_ctx):
    """BATH_LOGSUM_CONTEXT resolves to the odds mode while the switch is on; the 5-codon entry points have no odds mode."""
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    hmm = ba.HMM(path)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5))
    wins = fs_windows(np.random.default_rng(9), ol.Model(path), 6)
    blk = ba.SeqBlock(gpu_ctx, wins)
    odds = ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_ODDS)
    strict = ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_TABLE_SERIAL)
    assert np.array_equal(ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_CONTEXT).view(np.uint32), strict.view(np.uint32))
    gpu_ctx.set_fs_odds(True)
    try:
        assert np.array_equal(ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_CONTEXT).view(np.uint32), odds.view(np.uint32))
    finally:
        gpu_ctx.set_fs_odds(False)
    with pytest.raises(Exception):
        ba.FS5Envelopes(gpu_ctx, om5, blk, logsum=ba.LOGSUM_ODDS)


def test_pipeline_odds_vs_sse_pipeline(gpu_ctx):
    """run_frameshift / run_frameshift_domains with the odds switch on against the oracle's --fs pipeline on the SSE odds parsers."""
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    hmm = ba.HMM(path)
    rng = np.random.default_rng(17)
    wins = frameshifted_windows(rng, model)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
    pipe = ba.Pipeline(gpu_ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
    gpu_ctx.set_fs_odds(True)
    try:
        stats, _, fw = pipe.run_frameshift(om3, ba.SeqBlock(gpu_ctx, wins))
        _, gfw, gdm, _ = pipe.run_frameshift_domains(om3, om5, ba.SeqBlock(gpu_ctx, wins))
    finally:
        gpu_ctx.set_fs_odds(False)
    L_ = ol.lib()
    L_.bo_fs_use_sse(1)
    try:
        pli, _, _, ofw, per_w = model.run_pipeline_fs(wins)
        _, _, _, odm, per_d, _ = model.run_pipeline_fsdom(wins)
    finally:
        L_.bo_fs_use_sse(0)
    want = sorted(((w, o) for w, (a, b) in enumerate(per_w) for o in ofw[a:b]), key=lambda t: (t[0], t[1].strand, t[1].n))
    got = sorted(fw, key=lambda g: (g.window, g.strand, g.n))
    assert len(got) == len(want) >= 20
    lam = model.om.contents.evparam[5]
    unsure = []
    for g, (w, o) in zip(got, want):
        assert (g.window, g.strand, g.n, g.length, g.orf_cnt) == (w, o.strand, o.n, o.length, o.orf_cnt)
        tol = 1e-3 + 1e-4 * abs(o.fwdsc)
        assert abs(g.fwdsc - o.fwdsc) <= tol, (g.fwdsc, o.fwdsc)
        fac = np.exp(lam * tol / np.log(2.0)) * 1.001
        clear = (o.P_fs > 1e-5 * fac or o.P_fs < 1e-5 / fac) and (o.P_null > o.P_tot * fac * fac or o.P_null < o.P_tot / (fac * fac))
        if clear:
            assert g.branch == o.branch, (w, g.n, g.fwdsc, o.fwdsc)
        elif g.branch != o.branch:
            unsure.append((w, o.strand, o.n, o.fwdsc))
    print("windows whose branch decision lies within the score tolerance and differs:", unsure)
    assert any(g.branch == 1 for g in got)
    # domains: same keys except at most one (an envelope end may move where a posterior sits on a threshold), bit scores within 0.05
    key = lambda d: (d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm)
    og = sorted((w, key(o), o.bitscore) for w, (a, b) in enumerate(per_d) for o in odm[a:b])
    gg = sorted((d.window, key(d), d.bitscore) for d in gdm)
    assert len(gg) == len(og) >= 5
    same = [(a, b) for a, b in zip(gg, og) if a[:2] == b[:2]]
    assert len(same) >= len(og) - 1, [(a[:2], b[:2]) for a, b in zip(gg, og) if a[:2] != b[:2]]
    assert all(abs(a[2] - b[2]) <= 0.05 for a, b in same)


def test_recorded_fs_run_in_odds_mode():
    """tutorial/AMP_N-fs.tbl byte for byte, and the recorded --fs pipeline counters, with the parsers in odds space."""
    import recorded
    from test_tblout_gpu import table_body
    ctx = ba.Context(0)
    ctx.set_fs_odds(True)
    try:
        hmm = ba.HMM(ol.GOLDEN + "/AMP_N.bhmm", 0)
        recs = ol.read_fasta(ol.GOLDEN + "/target-AMP_N.fa")
        seqs = [ba.digitize(s, ba.DNA_SYMS) for _, s in recs]
        om = ba.OProfile(ctx, ba.Profile(hmm))
        pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
        stats, _, dm, _ = pipe.run_frameshift_domains(om3, om5, ba.SeqBlock(ctx, seqs))
        assert any("odds" in k for k in pipe.kernel_times())
        th = ba.TopHits()
        th.add(dm, [n.split()[0] for n, _ in recs], [len(s) for s in seqs])
        th.finalize(stats.nres, hmm.max_length)
        assert th.tblout(hmm.name, hmm.acc, hmm.M, fs_pipe=True, show_cigar=True) == table_body(ol.GOLDEN + "/AMP_N-fs.tbl")
        assert th.statistics(stats, pipe.params, 1, hmm.M, len(seqs)) == recorded.statistics_blocks("AMP_N-fs.out")[0]
    finally:
        ctx.set_fs_odds(False)
        ctx.close()


def dom_records(dm):
    return [(d.window, d.strand, d.fs_window, d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm, np.float32(d.bitscore).view(np.uint32),
             np.float64(d.lnP).view(np.uint64), d.n_shifted_codons, d.n_stops) for d in dm]


def test_routing_and_switching_back(gpu_ctx):
    """An odds-mode pass runs the odds kernels and no chain kernel; after set_fs_odds(False) a pass gives what a fresh strict
    context gives, record for record."""
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    hmm = ba.HMM(path)
    wins = frameshifted_windows(np.random.default_rng(23), model)

    def run(ctx):
        om = ba.OProfile(ctx, ba.Profile(hmm))
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
        pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
        _, _, dm, _ = pipe.run_frameshift_domains(om3, om5, ba.SeqBlock(ctx, wins))
        return pipe, dom_records(dm)

    gpu_ctx.set_fs_odds(True)
    try:
        pipe, odds_dm = run(gpu_ctx)
        names = set(pipe.kernel_times())
    finally:
        gpu_ctx.set_fs_odds(False)
    assert "fs3_bwd_odds_kernel" in names, names
    assert not any("chain" in k for k in names) and not ({"fs3_fwd_kernel", "fs_bwd_kernel<3>"} & names), names
    _, back = run(gpu_ctx)
    fresh = ba.Context(0)
    try:
        _, strict = run(fresh)
    finally:
        fresh.close()
    assert back == strict and len(strict) >= 5
    assert len(odds_dm) >= 5
