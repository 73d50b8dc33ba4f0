"""The 5-codon odds-ratio mode (bath_hip_set_fs5_odds, bath_fs5_odds.hip): the envelopes' unihit Forward and Backward and the
regions' multihit Forward in fp32 odds ratios with sparse rescaling, what the reference's bathsearch --fs runs there
(impl_sse/fwdback_fs.c:2054-2610, :2634-2970).  Held against the scalar oracle on EXACT log-sums (oracle_fs5(..., exact=True),
bo_flogsum_set_exact(1)) at the bars of the header's contract:

  * scores within 1e-3 + 1e-4 |s|; Forward - Backward within 2e-3 + 2e-4 |s| of the oracle's own Forward - Backward;
  * posteriors within 2e-3, the optimal-accuracy matrix and score within 2e-2 + 1e-3 |s|, null2 within rtol 5e-3 / atol 1e-4;
  * the regions' matrices and special-state rows within 2e-3 + 2e-4 |v| where the exact value is above -60 and within 60 nats of
    its row's largest (fp32 odds ratios hold about 87 nats below the running scale);
  * every per-lane tiling (C = 1 .. 20 at both ends of its M range), the switch's semantics, the --fs pipeline against the oracle's
    on the SSE odds parsers, clustered regions, and the recorded AMP_N run.

Every test that switches the mode on switches it off in a finally: the session's context stays strict."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol
from test_frameshift_gpu import oa_matrices_agree, oracle_fs5
from test_fs_odds_gpu import dom_records
from test_fs_pipeline_gpu import compare_domains, frameshifted_windows

pytestmark = pytest.mark.gpu

FS_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16, 20]
FS_M = [1, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1280]
FS_MAX_NODES = 1280
ODDS5_SPANS = {"fs5_fwd_odds_kernel", "fs5_bwd_odds_kernel", "fs5_fwd_odds_kernel(regions)"}
LOG_SPANS = {"fs5_fwd_kernel", "fs_bwd_kernel<5>", "fs5_fwd_kernel(regions)"}


def fs_columns(M):
    return next(c for c in FS_COLUMNS if (M + 63) // 64 <= c)


class odds5:
    """with odds5(ctx): the 5-codon odds mode on (and the 3-codon one too, with both=True), off again afterwards."""
    def __init__(self, ctx, both=False):
        self.ctx, self.both = ctx, both

    def __enter__(self):
        self.ctx.set_fs5_odds(True)
        if self.both:
            self.ctx.set_fs_odds(True)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_fs5_odds(False)
        self.ctx.set_fs_odds(False)


def single_pass(rng, model, n, sharpen=1.0, flank=8):
    """Reverse-translated passes through the model's match states (common.emit_from_model without its second copy), with
    frameshift indels (+-1, +-2 nt) and in-frame stops as fs_windows plants them: what an envelope holds, one domain.

    (A window with two copies is no envelope: in the unihit configuration a later copy can only start from N(i), and once the
    first copy has lifted the running scale by more than ~87 nats, N(i) is below fp32's range -- in the reference's SSE Forward
    as here -- while exact log-sums still count the second copy.)"""
    h = model.hmm.contents
    M = h.M
    mat = np.ctypeslib.as_array(h.mat, shape=((M + 1) * 20,)).reshape(M + 1, 20)
    bg = common.BG / common.BG.sum()
    out = []
    for _ in range(n):
        a = int(rng.integers(1, max(2, M // 2)))
        b = int(rng.integers(min(M, a + 10), M + 1))
        core = []
        for k in range(a, b + 1):
            if rng.random() < 0.05:
                continue
            q = mat[k].astype(np.float64) ** sharpen
            core.append(rng.choice(20, p=q / q.sum()))
            if rng.random() < 0.03:
                core.extend(rng.choice(20, size=int(rng.integers(1, 4)), p=bg))
        aa = np.concatenate([rng.choice(20, size=int(rng.integers(0, flank)), p=bg), np.array(core, dtype=np.int64),
                             rng.choice(20, size=int(rng.integers(0, flank)), p=bg)]).astype(np.uint8)
        nt = list(common.revtranslate(rng, aa, model.basic))
        j = 6
        while j < len(nt) - 6:
            r = rng.random()
            if r < 0.010:
                del nt[j]
            elif r < 0.020:
                nt.insert(j, int(rng.integers(0, 4)))
            elif r < 0.025:
                del nt[j:j + 2]
            elif r < 0.030:
                nt[j:j] = [int(rng.integers(0, 4)), int(rng.integers(0, 4))]
            elif r < 0.032:
                nt[j:j + 3] = [3, 0, 0]          # TAA
            j += 3
        out.append(np.array(nt, dtype=np.uint8))
    return out


def envelope_windows(rng, model, n, cap):
    """Single-domain model passes, a sharpened one (strong: many rescales), random DNA, a window with an N run and ambiguity codes,
    degenerate codes scattered, and the short edge cases, 15 .. <cap> nt."""
    wins = [w[:cap] for w in single_pass(rng, model, n) + single_pass(rng, model, 1, sharpen=3.0) if len(w) >= 15]
    deg = common.random_dna(rng, 1, min(400, cap))[0].copy()
    deg[50:70] = 15                                  # an N run
    deg[120] = 4; deg[200] = 7; deg[333 % len(deg)] = 11        # ambiguity codes
    wins += [deg, common.random_dna(rng, 1, cap)[0]] + common.random_dna(rng, 1, 150, degenerate_frac=0.03)
    wins += [rng.integers(0, 4, size=L).astype(np.uint8) for L in (15, 16, 17)]
    return wins


def check_envelopes(ctx, model, om5, env):
    """FS5Envelopes through BATH_LOGSUM_CONTEXT with the odds switch on, against the exact-log-sum oracle.  Returns the worst
    |delta| of the scores and of the posteriors."""
    with odds5(ctx):
        got = ba.FS5Envelopes(ctx, om5, ba.SeqBlock(ctx, env), logsum=ba.LOGSUM_CONTEXT, want_pp=True, want_oa=True)
    ref = oracle_fs5(model, env, False, exact=True)
    fwd = np.array([r[0] for r in ref], np.float64); bwd = np.array([r[1] for r in ref], np.float64)
    gf, gb = got["fwdsc"].astype(np.float64), got["bcksc"].astype(np.float64)
    assert not np.isnan(gf).any() and not np.isnan(gb).any()
    assert np.all(np.abs(gf - fwd) <= 1e-3 + 1e-4 * np.abs(fwd)), (np.abs(gf - fwd).max(), [len(w) for w in env])
    assert np.all(np.abs(gb - bwd) <= 1e-3 + 1e-4 * np.abs(bwd)), np.abs(gb - bwd).max()
    # Forward == Backward, as far as the reference's own recursions agree: with exact log-sums its p7_Forward_Frameshift and
    # p7_Backward_Frameshift differ by up to ~4e-3 nats on short envelopes (the asymmetric edge rows), so F - B is held to the
    # oracle's own F - B at twice the score bar
    assert np.all(np.abs((gf - gb) - (fwd - bwd)) <= 2e-3 + 2e-4 * np.abs(fwd)), np.abs((gf - gb) - (fwd - bwd)).max()
    worst_pp = 0.0
    for i, r in enumerate(ref):
        d = np.abs(got["pp"][i][1:, 1:, 1:].astype(np.float64) - r[4][1:, 1:, 1:])
        worst_pp = max(worst_pp, float(d.max()))
        assert d.max() <= 2e-3, (i, len(env[i]), float(d.max()))                                   # posteriors
        assert abs(got["oasc"][i] - r[2]) <= 2e-2 + 1e-3 * abs(r[2]), (i, got["oasc"][i], r[2])
        assert oa_matrices_agree(got["oa"][i], r[5], 2e-2, 1e-3), i                              # the whole OA matrix
        assert np.allclose(got["null2"][i], r[3], rtol=5e-3, atol=1e-4), i
    return float(max(np.abs(gf - fwd).max(), np.abs(gb - bwd).max())), worst_pp


def forward_full(ctx, om5, env, M):
    """bath_hip_fs5_forward_full (the regions' multihit Forward of amino length 100): scores, matrices, special-state rows."""
    eb = ba.SeqBlock(ctx, env)
    foff = np.zeros(len(env) + 1, np.int64); np.cumsum([(len(w) + 1) * (M + 1) * 8 for w in env], out=foff[1:])
    xoff = np.zeros(len(env) + 1, np.int64); np.cumsum([(len(w) + 1) * 5 for w in env], out=xoff[1:])
    sc = np.zeros(len(env), np.float32); fwd = np.zeros(int(foff[-1]), np.float32); xmx = np.zeros(int(xoff[-1]), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ctx._check(ba.lib().bath_hip_fs5_forward_full(ctx._h, om5._h, eb._h, 100, fp(sc), fp(fwd), fp(xmx)), "fs5_forward_full")
    return sc, [fwd[foff[e]:foff[e + 1]].reshape(len(w) + 1, M + 1, 8) for e, w in enumerate(env)], \
        [xmx[xoff[e]:xoff[e + 1]].reshape(len(w) + 1, 5) for e, w in enumerate(env)]


def live_cells(o, top):
    return np.isfinite(o) & (o > -60.0) & (o > top - 60.0)


def check_forward_full(ctx, model, om5, env):
    """The multihit Forward with the switch on against bo_gforward_fs on exact log-sums: the score, then every matrix cell and
    special-state value above -60 and within 60 nats of its row's largest.  Returns the worst |delta| of score and cells."""
    M = model.M
    with odds5(ctx):
        sc, mats, rows = forward_full(ctx, om5, env, M)
    L_ = ol.lib()
    gm5 = model.fs(5)
    L_.bo_fs_profile_reconfig_multihit(gm5, 100)
    f = C.c_float()
    worst_sc = worst_cell = 0.0
    L_.bo_flogsum_set_exact(1)
    try:
        for e, w in enumerate(env):
            L = len(w)
            g8 = L_.bo_gmx_create(M, L + 1, L, 8)
            assert L_.bo_gforward_fs(ol.u8(ol.dsq_from(w)), L, gm5, g8, 0, C.byref(f)) == 0
            dp = np.ctypeslib.as_array(g8.contents.dp, shape=(L + 1, M + 1, 8)).astype(np.float64)
            ox = np.ctypeslib.as_array(g8.contents.xmx, shape=(L + 1, 5)).astype(np.float64)
            L_.bo_gmx_free(g8)
            o = float(f.value)
            assert not np.isnan(sc[e])
            assert abs(sc[e] - o) <= 1e-3 + 1e-4 * abs(o), (e, L, sc[e], o)
            worst_sc = max(worst_sc, abs(sc[e] - o))
            for g, ov in ((rows[e], ox), (mats[e][1:, 1:, :].reshape(L, -1), dp[1:, 1:, :].reshape(L, -1))):
                top = np.where(np.isfinite(ov), ov, -np.inf).max(axis=1, keepdims=True)
                live = live_cells(ov, top)
                assert not np.isnan(g).any()
                d = np.abs(g[live].astype(np.float64) - ov[live])
                assert np.all(d <= 2e-3 + 2e-4 * np.abs(ov[live])), (e, L, float(d.max()))
                if d.size:
                    worst_cell = max(worst_cell, float(d.max()))
    finally:
        L_.bo_flogsum_set_exact(0)
    return worst_sc, worst_cell


# ---- 1, 2: the golden models and two long synthetic ones

@pytest.fixture(scope="module", params=["Caudal_act", "2OG-FeII_Oxy_3", "PTH2", "synth1024", "synth1200"])
def model5(request, gpu_ctx, tmp_path_factory):
    name = request.param
    if name.startswith("synth"):
        M = int(name[5:])
        path = str(tmp_path_factory.mktemp("odds5") / (name + ".bhmm"))
        common.write_synthetic_bhmm(path, M, seed=M, name=name)
        n, cap = 2, 2500
    else:
        path = ol.GOLDEN + "/" + name + ".bhmm"
        n, cap = 10, 2500
    model = ol.Model(path)
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(ba.HMM(path), 5))
    env = envelope_windows(np.random.default_rng(11), model, n, cap)
    if model.M > 512:                                # the oracle's exact log-sums at 1200 nodes: a few long windows, the edge cases
        env = sorted(env, key=len, reverse=True)[:3] + env[-3:]
    assert max(len(w) for w in env) >= 1000 and min(len(w) for w in env) == 15
    return gpu_ctx, model, om5, env


def test_envelopes_vs_exact_oracle(model5):
    ctx, model, om5, env = model5
    ws, wp = check_envelopes(ctx, model, om5, env)
    print("fs5 odds envelopes (M=%d): worst |delta| score %.2e, posterior %.2e" % (model.M, ws, wp))


def test_multihit_forward_vs_exact_oracle(model5):
    ctx, model, om5, env = model5
    ws, wc = check_forward_full(ctx, model, om5, env[:4] + env[-1:])
    print("fs5 odds multihit Forward (M=%d): worst |delta| score %.2e, cells %.2e" % (model.M, ws, wc))


# ---- 3: every tiling

@pytest.mark.parametrize("M", FS_M, ids=["C%d-M%d" % (fs_columns(M), M) for M in FS_M])
def test_every_tiling(gpu_ctx, tmp_path, M):
    path = str(tmp_path / ("s%d.bhmm" % M))
    common.write_synthetic_bhmm(path, M, seed=M)
    model = ol.Model(path)
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(ba.HMM(path), 5))
    cap = 450 if M > 512 else 700
    env = envelope_windows(np.random.default_rng(M + 3), model, 2, cap)
    env = sorted(env, key=len, reverse=True)[:4] + env[-2:]
    check_envelopes(gpu_ctx, model, om5, env)
    check_forward_full(gpu_ctx, model, om5, [env[0], env[-1]])


def test_models_beyond_1280_nodes_are_refused(gpu_ctx, tmp_path):
    M = FS_MAX_NODES + 1
    path = str(tmp_path / ("s%d.bhmm" % M))
    common.write_synthetic_bhmm(path, M, seed=M)
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(ba.HMM(path), 5))
    rng = np.random.default_rng(M)
    blk = ba.SeqBlock(gpu_ctx, [rng.integers(0, 4, size=L).astype(np.uint8) for L in (300, 90, 15)])
    msg = "up to %d nodes" % FS_MAX_NODES
    with odds5(gpu_ctx):
        with pytest.raises(ba.BathError, match=msg):
            ba.FS5Envelopes(gpu_ctx, om5, blk, logsum=ba.LOGSUM_CONTEXT, want_pp=True, want_oa=True)
        with pytest.raises(ba.BathError, match=msg):
            forward_full(gpu_ctx, om5, [np.zeros(300, np.uint8)], M)


# ---- 4: the switch

def test_switch_semantics(gpu_ctx):
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    hmm = ba.HMM(path)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5))
    env = envelope_windows(np.random.default_rng(5), model, 6, 1200)
    blk = ba.SeqBlock(gpu_ctx, env)
    keys = ("fwdsc", "bcksc", "oasc", "null2")

    def run(mode, **kw):
        return ba.FS5Envelopes(gpu_ctx, om5, blk, logsum=mode, want_oa=True, **kw)

    def same(a, b):
        return all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)) for k in keys) and \
            all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a["oa"], b["oa"]))

    strict = run(ba.LOGSUM_TABLE_SERIAL)
    assert same(run(ba.LOGSUM_CONTEXT), strict)                                   # off: the strict kernels, bit for bit
    fs3_strict = ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_TABLE_SERIAL)
    with odds5(gpu_ctx):
        on = run(ba.LOGSUM_CONTEXT)
        assert same(run(ba.LOGSUM_CONTEXT), on)                                   # repeated runs: the same bits
        gpu_ctx.set_fs_strict(False)
        try:
            assert same(run(ba.LOGSUM_CONTEXT), on)                               # ahead of set_fs_strict
        finally:
            gpu_ctx.set_fs_strict(True)
        assert not same(on, strict)
        # the 3-codon parsers follow set_fs_odds only
        assert np.array_equal(ba.FS3ForwardParser(gpu_ctx, om3, blk, logsum=ba.LOGSUM_CONTEXT).view(np.uint32), fs3_strict.view(np.uint32))
        with pytest.raises(ba.BathError):
            run(ba.LOGSUM_ODDS)                                                   # an explicit LOGSUM_ODDS is still refused
        with pytest.raises(ba.BathError, match="c5_compat"):
            run(ba.LOGSUM_CONTEXT, c5_compat=True)
    assert same(run(ba.LOGSUM_CONTEXT), strict)                                   # off again
    with pytest.raises(ba.BathError):
        run(ba.LOGSUM_ODDS)


def pipeline_run(ctx, hmm, wins):
    om = ba.OProfile(ctx, ba.Profile(hmm))
    om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
    pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
    stats, fw, dm, nskip = pipe.run_frameshift_domains(om3, om5, ba.SeqBlock(ctx, wins))
    return pipe, stats, fw, dm, nskip


def test_switching_off_gives_a_fresh_strict_context_s_pass(gpu_ctx):
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    hmm = ba.HMM(path)
    wins = frameshifted_windows(np.random.default_rng(23), ol.Model(path))
    with odds5(gpu_ctx, both=True):
        pipe, _, _, odds_dm, _ = pipeline_run(gpu_ctx, hmm, wins)
        names = set(pipe.kernel_times())
    assert {"fs5_fwd_odds_kernel", "fs5_bwd_odds_kernel"} <= names, names
    back = dom_records(pipeline_run(gpu_ctx, hmm, wins)[3])
    fresh = ba.Context(0)
    try:
        strict = dom_records(pipeline_run(fresh, hmm, wins)[3])
    finally:
        fresh.close()
    assert back == strict and len(strict) >= 5 and len(odds_dm) >= 5


# ---- 5, 6: the --fs pipeline against the oracle's (SSE odds parsers, exact log-sums)

def oracle_pipeline(model, wins):
    L_ = ol.lib()
    L_.bo_fs_use_sse(1)
    L_.bo_flogsum_set_exact(1)
    try:
        return model.run_pipeline_fsdom(wins)
    finally:
        L_.bo_flogsum_set_exact(0)
        L_.bo_fs_use_sse(0)


def test_pipeline_vs_oracle(gpu_ctx, monkeypatch):
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    hmm = ba.HMM(path)
    wins = frameshifted_windows(np.random.default_rng(17), model)
    with odds5(gpu_ctx, both=True):
        pipe, stats, fw, gdm, nskip = pipeline_run(gpu_ctx, hmm, wins)
        names = set(pipe.kernel_times())
        recs = dom_records(gdm)
        for switch, value in (("BATH_HIP_ENV_MB", "1"), ("BATH_HIP_LANES", "2")):      # envelope batches split; cascade lanes
            monkeypatch.setenv(switch, value)
            try:
                assert dom_records(pipeline_run(gpu_ctx, hmm, wins)[3]) == recs, switch
            finally:
                monkeypatch.delenv(switch)
    assert {"fs5_fwd_odds_kernel", "fs5_bwd_odds_kernel"} <= names, names
    assert not (LOG_SPANS & names) and not any("chain" in k for k in names), names
    _, _, _, odm, per_d, _ = oracle_pipeline(model, wins)
    key = lambda d: (d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm)
    og = sorted((w, key(o), o.bitscore) for w, (a, b) in enumerate(per_d) for o in odm[a:b])
    gg = sorted((d.window, key(d), d.bitscore) for d in gdm)
    assert len(gg) == len(og) >= 5
    differ = [(a[:2], b[:2]) for a, b in zip(gg, og) if a[:2] != b[:2]]
    print("domains whose keys differ from the oracle's:", differ)
    assert len(differ) <= 2, differ
    assert all(abs(a[2] - b[2]) <= 0.05 for a, b in zip(gg, og) if a[:2] == b[:2])


def test_clustered_regions(gpu_ctx):
    """The two-copy PTH2 windows of test_strict_pipeline_is_exact_on_clustered_regions: multi-domain regions resolved by 200
    stochastic tracebacks through the odds-mode multihit Forward matrix.  Tolerance-equal matrices draw other samples, so these
    envelopes agree at the fast mode's bar (compare_domains: ends within 60 nt, scores within 2.5 bits)."""
    rng = np.random.default_rng(7)
    path = ol.GOLDEN + "/PTH2.bhmm"
    model = ol.Model(path, 0)
    genes = common.emit_from_model(rng, model, 12, flank=3, sharpen=2.0)
    wins = []
    for a, b in zip(genes[::2], genes[1::2]):
        nt = [list(common.revtranslate(rng, g, model.basic)) for g in (a, b)]
        for seq in nt:
            p = int(rng.integers(10, len(seq) - 10))
            del seq[p]                                         # one frameshift per copy
        wins.append(np.array(nt[0] + list(rng.integers(0, 4, size=int(rng.integers(20, 60)))) + nt[1], dtype=np.uint8))
    hmm = ba.HMM(path, 0)
    with odds5(gpu_ctx, both=True):
        pipe, stats, fw, dm, nskip = pipeline_run(gpu_ctx, hmm, wins)
        names = set(pipe.kernel_times())
    assert nskip >= 1, "no clustered region in this input"
    assert ODDS5_SPANS <= names and not (LOG_SPANS & names) and not any("chain" in k for k in names), names
    _, ofw, per_w, odm, per_d, oskip = oracle_pipeline(model, wins)
    assert nskip == oskip
    assert compare_domains(model, dm, odm, per_d, nskip) >= 4


# ---- 7: the recorded run

def test_recorded_fs_run_with_both_odds_switches():
    """tutorial/AMP_N-fs.tbl byte for byte, and the recorded --fs pipeline counters, in a fresh context with both switches on."""
    import recorded
    from test_tblout_gpu import table_body
    ctx = ba.Context(0)
    try:
        ctx.set_fs_odds(True)
        ctx.set_fs5_odds(True)
        hmm = ba.HMM(ol.GOLDEN + "/AMP_N.bhmm", 0)
        recs = ol.read_fasta(ol.GOLDEN + "/target-AMP_N.fa")
        seqs = [ba.digitize(s, ba.DNA_SYMS) for _, s in recs]
        pipe, stats, _, dm, _ = pipeline_run(ctx, hmm, seqs)
        names = set(pipe.kernel_times())
        assert {"fs5_fwd_odds_kernel", "fs5_bwd_odds_kernel"} <= names and not (LOG_SPANS & names), names
        th = ba.TopHits()
        th.add(dm, [n.split()[0] for n, _ in recs], [len(s) for s in seqs])
        th.finalize(stats.nres, hmm.max_length)
        assert th.tblout(hmm.name, hmm.acc, hmm.M, fs_pipe=True, show_cigar=True) == table_body(ol.GOLDEN + "/AMP_N-fs.tbl")
        assert th.statistics(stats, pipe.params, 1, hmm.M, len(seqs)) == recorded.statistics_blocks("AMP_N-fs.out")[0]
    finally:
        ctx.close()
