"""GPU tier of --arith: the score-only 5-codon odds-ratio Forward parser (fs5_fwd_odds_kernel<C, true, false>) at every per-lane
tiling, calibrate_fs in the reference's arithmetic against the CPU path on exact log-sums and the oracle's SSE odds parser,
bathconvert --arith odds on the 12-model fixture and its pin against the reference's recorded conversion, and bathsearch --arith on
the recorded runs, over --workers and --gpus.  Every command-line run is a fresh child process under a time limit of its own."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import calib_common as cc
import oracle_lib as ol
from bath_amd import bathconvert as bc
from bath_amd import synth
from test_calibrate_gpu import identical, oracle_fs5, read, run_convert, tbl_rows
from test_bathsearch_gpu import env_free_heads
from test_bathsearch_workers_gpu import normalise, search

pytestmark = pytest.mark.gpu

FS_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16, 20]                      # BATH_FS_COLUMNS (bath_tilings.hpp), held equal below
PARSER_M = sorted({1, 2} | {64 * c for c in FS_COLUMNS} | {64 * c + 1 for c in FS_COLUMNS[:-1]})
LENGTHS = [0, 4, 5, 6, 299, 300, 301]
STRICT_JSON = os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")
LN2 = cc.LN2


def score_bar(s):
    """tests/test_fs5_odds_gpu.py::check_forward_full's bar for this kernel's multihit score (and test_fs_odds_gpu.py::compare_parser's
    for the 3-codon odds parser, against the exact oracle and the SSE one alike), nats."""
    return 1e-3 + 1e-4 * np.abs(s)


class exact_logsums:
    def __enter__(self):
        ol.lib().bo_flogsum_set_exact(1)

    def __exit__(self, *exc):
        ol.lib().bo_flogsum_set_exact(0)


class switches:
    """with switches(ctx, odds3, odds5): the context's two odds switches as given, off again afterwards."""
    def __init__(self, ctx, o3, o5):
        self.ctx, self.o3, self.o5 = ctx, o3, o5

    def __enter__(self):
        self.ctx.set_fs_odds(self.o3); self.ctx.set_fs5_odds(self.o5)

    def __exit__(self, *exc):
        self.ctx.set_fs_odds(False); self.ctx.set_fs5_odds(False)


def test_parser_lengths_cover_the_tiling_list():
    from test_tiling_coverage_cpu import fs_options, lengths_per_column
    fs = fs_options()
    assert FS_COLUMNS == fs
    assert all(lo in PARSER_M and hi in PARSER_M for _, lo, hi in lengths_per_column(fs))
    assert "fs5_fwd_odds_kernel<CC, true, false>" in open(ba._ROOT + "/bath_amd/csrc/bath_fs5_odds.hip").read()


@pytest.mark.parametrize("M", PARSER_M)
def test_odds_parser_is_the_full_odds_forward_s_score(gpu_ctx, tmp_path, M):
    """bath_hip_fs5_forward_parser_odds: 0, 4, 5, 6, 299, 300 and 301 nt (one window with N codes) and five random lengths, as one
    block of 201 windows and as blocks of one.  The score is FS5ForwardFull's under set_fs5_odds bit for bit; 0 and 4 nt give -inf;
    against bo_gforward_fs on exact log-sums it is within 1e-3 + 1e-4 |s|."""
    ctx = gpu_ctx
    path = synth.write_synthetic_bhmm(str(tmp_path / "s.bhmm"), M, seed=M)
    om5 = ba.FSOProfile(ctx, ba.FSProfile(ba.HMM(path), 5, 100))
    model = ol.Model(path)
    rng = np.random.default_rng(M)
    distinct = [rng.integers(0, 4, n).astype(np.uint8) for n in LENGTHS]
    distinct[4][[7, 8, 150]] = 15                                 # N
    distinct += [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(5, 302, 5)]
    with switches(ctx, False, True):
        full = ba.FS5ForwardFull(ctx, om5, ba.SeqBlock(ctx, distinct), 100)[0]
    assert np.isneginf(full[:2]).all() and np.isfinite(full[2:]).all(), full
    pick = list(range(len(distinct))) + [int(v) for v in rng.integers(0, len(distinct), 201 - len(distinct))]
    got = ba.FS5ForwardParserOdds(ctx, om5, ba.SeqBlock(ctx, [distinct[p] for p in pick]), 100)
    assert len(got) == 201 and identical(got, full[pick]), (M, got[:12], full)
    for p in range(len(distinct)):                                # blocks of one window
        one = ba.FS5ForwardParserOdds(ctx, om5, ba.SeqBlock(ctx, [distinct[p]]), 100)
        assert identical(one, full[p:p + 1]), (M, p, one, full[p])
    with exact_logsums():
        want = oracle_fs5(model, distinct).astype(np.float64)
    d = np.abs(full[2:].astype(np.float64) - want[2:])
    print("fs5 odds parser (M=%d): worst |delta| against the exact oracle %.2e nats" % (M, d.max()))
    assert np.isneginf(want[:2]).all() and np.all(d <= score_bar(want[2:])), (M, d, want)


def test_odds_parser_ignores_the_switches_and_refuses_three_codons(gpu_ctx):
    ctx = gpu_ctx
    hmm = ba.HMM(os.path.join(ol.GOLDEN, "PTH2.bhmm"))
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, 100))
    rng = np.random.default_rng(3)
    blk = ba.SeqBlock(ctx, [rng.integers(0, 4, 300).astype(np.uint8) for _ in range(5)])
    base = ba.FS5ForwardParserOdds(ctx, om5, blk, 100)
    strict = ba.FS5ForwardParser(ctx, om5, blk, 100)
    assert np.isfinite(base).all() and not identical(base, strict)             # another arithmetic than the strict parser's
    assert np.all(np.abs(base.astype(np.float64) - strict) <= 0.05)             # ... of the same score (strict: table log-sums)
    for o3, o5, st in ((True, True, True), (False, True, False), (True, False, True)):
        try:
            ctx.set_fs_strict(st)
            with switches(ctx, o3, o5):
                assert identical(ba.FS5ForwardParserOdds(ctx, om5, blk, 100), base), (o3, o5, st)
        finally:
            ctx.set_fs_strict(True)
    assert identical(ba.FS5ForwardParser(ctx, om5, blk, 100), strict)
    om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, 100))
    with pytest.raises(ba.BathError, match="5-codon"):
        ba.FS5ForwardParserOdds(ctx, om3, blk, 100)


# ---- calibrate_fs in a chosen arithmetic

def synth129(tmp_path_factory):
    return synth.write_synthetic_bhmm(str(tmp_path_factory.mktemp("arith") / "s129.bhmm"), 129, seed=5)


@pytest.fixture(scope="module")
def calib_models(tmp_path_factory):
    return {"ATE_N": (cc.HMM_IN, 0), "synth129": (synth129(tmp_path_factory), 0)}


@pytest.mark.parametrize("name", ["ATE_N", "synth129"])
def test_calibrate_strict_is_the_existing_call(gpu_ctx, calib_models, name):
    path, index = calib_models[name]
    hmm = ba.HMM(path, index)
    s0 = ba.rng_state(42)
    for L, N in ((100, 200), (10, 8)):
        a = ba.calibrate_fs(gpu_ctx, hmm, 1, s0, L, N, want_xv=True)
        b = ba.calibrate_fs(gpu_ctx, hmm, 1, s0, L, N, want_xv=True, arith="strict")
        assert len(a) == len(b) == 5 and a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()
        assert ba.calibrate_fs(gpu_ctx, hmm, 1, s0, L, N, arith="strict") == a[:3]
        # ... and the C entry point's arith = 0
        st = C.c_uint32(s0); t3, t5 = C.c_double(0), C.c_double(0)
        x3, x5 = np.zeros(N), np.zeros(N)
        re2 = (C.c_int * 2)(7, 7)
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        gpu_ctx._check(ba.lib().bath_hip_calibrate_fs_arith(gpu_ctx._h, hmm._p, 1, C.byref(st), L, N, 0.04, C.byref(t3), C.byref(t5), dp(x3), dp(x5),
                                                            ba.ARITH_STRICT, re2), "calibrate_fs_arith")
        assert (t3.value, t5.value, st.value) == a[:3] and x3.tobytes() == a[3].tobytes() and x5.tobytes() == a[4].tobytes() and list(re2) == [0, 0]
    with pytest.raises(ba.BathError, match="arith"):
        gpu_ctx._check(ba.lib().bath_hip_calibrate_fs_arith(gpu_ctx._h, hmm._p, 1, C.byref(st), 100, 200, 0.04, C.byref(t3), C.byref(t5), None, None, 3, None), "x")


def sse_fs3_bits(path, index, dna, L):
    """The 3-codon bit scores of <dna> from the oracle's SSE odds parser (oracle/sse/sse_fs.c)."""
    from test_fs_odds_gpu import sse_oracle
    L_ = ol.lib()
    L_.bo_fs_use_sse(1)
    try:
        res = sse_oracle(ol.Model(path, index), list(dna), False)
    finally:
        L_.bo_fs_use_sse(0)
    assert all(st == 0 for st, _, _ in res)
    nullsc = np.float32(ba.bg_fs_nullone(L))
    return np.array([float(np.float32(o) - nullsc) / LN2 for _, o, _ in res])


@pytest.mark.parametrize("L,N", [(100, 200), (10, 8)])
@pytest.mark.parametrize("name", ["ATE_N", "synth129"])
def test_calibrate_odds_against_the_exact_cpu_path(gpu_ctx, calib_models, name, L, N):
    """arith="odds" (and "odds3"): the bit scores within the kernels' score bars / ln 2 of the CPU path on exact log-sums, the
    3-codon ones also of the SSE odds oracle's; nothing redrawn, so the generator ends where two calib_sample calls end; the taus
    are the fit of the returned scores; the context's switches play no part."""
    ctx = gpu_ctx
    path, index = calib_models[name]
    hmm = ba.HMM(path, index)
    s0 = ba.rng_state(42)
    t3, t5, s1, x3, x5, redrawn = ba.calibrate_fs(ctx, hmm, 1, s0, L, N, want_xv=True, arith="odds")
    assert redrawn == [0, 0], "sequences were redrawn (%r): the generator comparison below does not apply" % (redrawn,)
    d3, s = ba.calib_sample(s0, L, N, 1)
    _, s = ba.calib_sample(s, L, N, 1)
    assert s1 == s
    with exact_logsums():
        w3, w5, ws, wx3, wx5 = cc.oracle_model(path, index, 1, s0, L, N)
    assert ws == s1
    nullsc = float(np.float32(ba.bg_fs_nullone(L)))
    for which, x, wx in (("fs3", x3, wx3), ("fs5", x5, wx5)):
        d = np.abs(x - wx)
        print("calibrate_fs odds %s %s (L=%d, N=%d): worst |delta| %.2e bits" % (name, which, L, N, d.max()))
        assert np.all(d <= score_bar(wx * LN2 + nullsc) / LN2), (which, d.max())
    sx3 = sse_fs3_bits(path, index, d3, L)
    assert np.all(np.abs(x3 - sx3) <= score_bar(sx3 * LN2 + nullsc) / LN2), np.abs(x3 - sx3).max()
    lam = float(hmm.evparam[5])
    assert t3 == ba.calib_tau(x3, lam) and t5 == ba.calib_tau(x5, lam)
    assert ba.calibrate_fs(ctx, hmm, 1, s0, L, N, arith="odds") == (t3, t5, s1)
    # odds3: the same 3-codon scores, the strict call's 5-codon ones
    o3 = ba.calibrate_fs(ctx, hmm, 1, s0, L, N, want_xv=True, arith="odds3")
    strict = ba.calibrate_fs(ctx, hmm, 1, s0, L, N, want_xv=True)
    assert o3[3].tobytes() == x3.tobytes() and o3[4].tobytes() == strict[4].tobytes() and o3[5] == [0, 0] and o3[2] == s1
    assert x3.tobytes() != strict[3].tobytes() and x5.tobytes() != strict[4].tobytes()
    with switches(ctx, True, True):                               # neither read nor changed
        assert ba.calibrate_fs(ctx, hmm, 1, s0, L, N) == strict[:3]
        assert ba.calibrate_fs(ctx, hmm, 1, s0, L, N, arith="odds") == (t3, t5, s1)


# ---- bathconvert --arith odds

@pytest.fixture(scope="module")
def odds_taus(gpu_ctx):
    """calibrate_fs(arith="odds") carried through the 12-model file: [(tau3, tau5, redrawn)]."""
    state, out = ba.rng_state(ba.CALIB_SEED), []
    for i in range(12):
        t3, t5, state, _, _, re2 = ba.calibrate_fs(gpu_ctx, ba.HMM(cc.HMM_IN, i), 1, state, want_xv=True, arith="odds")
        out.append((t3, t5, re2))
    return out


@pytest.fixture(scope="module")
def converted_odds(tmp_path_factory):
    d = tmp_path_factory.mktemp("bathconvert_odds")
    out = str(d / "tRNA-proteins.bhmm")
    return out, run_convert(d, ["--arith", "odds", out, cc.HMM_IN])


def test_cli_converts_in_odds_arithmetic(converted_odds, odds_taus):
    out, text = converted_odds
    rec = cc.recorded(cc.BHMM_OUT)
    assert read(out) == bc.rewrite(read(cc.HMM_IN), [(t3, t5) for t3, t5, _ in odds_taus], [r[0] for r in rec])
    rows = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    assert [int(r.split()[0]) for r in rows] == list(range(1, 13))


def test_odds_taus_are_closer_to_the_recorded_conversion_than_the_strict_ones(odds_taus):
    """The pin's condition: the reference's arithmetic lands closer to the reference's record than the strict arithmetic does, on
    each of the 24 taus (profiles/bathconvert_odds_vs_recorded.json holds one run's figures)."""
    strict = json.load(open(STRICT_JSON))["models"]
    rec = cc.recorded(cc.BHMM_OUT)
    worst = {"fs3": 0.0, "fs5": 0.0}
    bad = []
    for i, ((t3, t5, re2), s, r) in enumerate(zip(odds_taus, strict, rec)):
        for key, tau, want in (("fs3", t3, r[1]), ("fs5", t5, r[2])):
            worst[key] = max(worst[key], abs(tau - want))
            if not abs(tau - want) < abs(s[key]["diff"]):
                bad.append((i, s["name"], key, tau - want, s[key]["diff"]))
    print("odds taus minus recorded: worst |diff| fs3 %.2e, fs5 %.2e; redrawn %r" % (worst["fs3"], worst["fs5"], [r for _, _, r in odds_taus]))
    assert not bad, bad


def test_search_with_the_odds_converted_file(converted_odds, tmp_path):
    from bath_amd import bathsearch as bs
    out, _ = converted_odds
    target = os.path.join(ol.GOLDEN, "target-PTH2.fa")
    a, b = str(tmp_path / "a.tbl"), str(tmp_path / "b.tbl")
    null = open(os.devnull, "w")
    assert bs.run(["--fs", "--arith", "odds", "--tblout", a, out, target], stdout=null) == 0
    assert bs.run(["--fs", "--arith", "odds", "--tblout", b, cc.BHMM_OUT, target], stdout=null) == 0
    assert tbl_rows(a) == tbl_rows(b)
    assert any(not ln.startswith("#") and ln.strip() for ln in tbl_rows(a))            # there are hits to compare


# ---- bathsearch --arith

AMP = ["AMP_N.bhmm", "target-AMP_N.fa"]


def statistics_block(lines):
    i = next(i for i, ln in enumerate(lines) if ln.startswith("Internal pipeline statistics summary"))
    return [ln for ln in lines[i:i + 11] if not ln.startswith(("# CPU time:", "# Mc/sec:"))]


def recorded_text(name):
    return normalise(open(os.path.join(ol.GOLDEN, name)).read())


def table_rows(lines):
    return lines[:lines.index("#") if "#" in lines else len(lines)]


@pytest.mark.parametrize("arith", ["odds", "odds3"])
def test_recorded_fs_run(tmp_path, arith):
    """bathsearch --fs --arith <arith> on the recorded AMP_N run: the recorded table body; with odds also the recorded pipeline
    statistics block and the whole main output."""
    tbl, out = "AMP_N-fs.tbl", "AMP_N-fs.out"                     # the recorded command's names: the header lines name them
    got = search(tmp_path, arith, ["--fs", "--arith", arith, "--cigar", "--tblout", tbl, "-o", out] + AMP, AMP, (tbl, out))
    want_tbl, want_out = recorded_text(tbl), recorded_text(out)
    assert table_rows(got[tbl]) == table_rows(want_tbl) and len(table_rows(want_tbl)) >= 3
    if arith == "odds":
        assert statistics_block(got[out]) == statistics_block(want_out)
        differ = [(a, b) for a, b in zip(env_free_heads(got[out]), env_free_heads(want_out)) if a != b]
        print("lines of the main output that differ from AMP_N-fs.out:", differ)
        assert env_free_heads(got[out]) == env_free_heads(want_out)


def hit_targets(lines):
    return sorted(ln.split()[0] + " " + ln.split()[2] for ln in lines if ln and not ln.startswith("#"))


def test_arith_reaches_every_worker_and_every_rank(tmp_path):
    """MET-ct4.bhmm (two models), --ct 4 --fs --arith odds: --workers 2 and --gpus 2 (two ranks sharing the device, gloo) write the
    one-context search's output; the strict search reports the same targets."""
    files = ["MET-ct4.bhmm", "target-MET.fa"]
    outs = ("o.out", "t.tbl")
    argv = ["--ct", "4", "--fs", "--arith", "odds", "--tblout", "t.tbl", "-o", "o.out"] + files
    one = search(tmp_path, "w1", ["--gpus", "1", "--workers", "1"] + argv, files, outs)
    assert sum(ln.startswith("Query:") for ln in one["o.out"]) == 2 and one["o.out"][-2] == "[ok]"
    assert search(tmp_path, "w2", ["--workers", "2"] + argv, files, outs) == one
    assert search(tmp_path, "g2", ["--gpus", "2"] + argv, files, outs, multi=True) == one
    strict = search(tmp_path, "strict", [a for a in argv if a not in ("--arith", "odds")], files, outs)
    assert hit_targets(strict["t.tbl"]) == hit_targets(one["t.tbl"]) and len(hit_targets(one["t.tbl"])) >= 1
