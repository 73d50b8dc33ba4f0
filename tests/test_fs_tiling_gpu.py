"""The frameshift kernels at every per-lane model tiling, against the oracle.

Every frameshift kernel is a template on C, the model nodes a lane owns, picked from the model length M out of one list
(BATH_FS_COLUMNS in bath_tilings.hpp, which every frameshift launcher dispatches over): C = 1 2 3 4 6 8 12 16 20, M from
64 C_prev + 1 to 64 C.  Each C has its own register layout and its own handling of the last, partly filled lane.  FS_M holds the
smallest and the largest length of each instantiation (the smallest leaves the last used lane partly filled, 257 = 42 * 6 + 5;
the largest fills all 64 lanes), each checked at the bars of test_frameshift_gpu.py and test_fs_odds_gpu.py:

  * fs3 strict: Forward and Backward scores and every {E,N,J,B,C} row bit-identical; fast within 1e-4 |s| + 5e-3; exact within
    1e-4 |s| + 1e-4; odds against the exact-log-sum and the SSE odds oracles, Forward == Backward;
  * FS5Envelopes, strict and scan: scores, posteriors, the whole optimal-accuracy matrix, its score and null2 (beyond 128 nodes
    the multi-wave decode / OA kernel at W = 1..8 waves of 2 nodes per lane, W = 6 / 7 of 3 beyond 1024);
  * bath_hip_fs5_forward_full (multihit, strict): the whole matrix and the rows bit-identical.

Then the fs5 wavefront's waves per envelope (fs_wf_waves in bath_fs_wavefront.hip: BATH_HIP_WF_WAVES, BATH_HIP_WF_RING_G, read once
per process, so each setting runs in a fresh process), the heuristic's own W = 1 on thousands of envelopes, and the refusal of
models beyond 1280 nodes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol
from test_frameshift_gpu import (check_fs5_envelopes, check_fs5_forward_full, close, fs_windows, identical, oracle_fs3, oracle_fs5,
                                 record_errors)
from test_fs_odds_gpu import compare_parser, exact_oracle, sse_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16, 20]
FS_M = [1, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1280]
WF_WAVES = [1, 2, 4, 8]
WF_M = [65, 256, 513, 1280]
FS_MAX_NODES = 1280


def fs_columns(M):
    return next(c for c in FS_COLUMNS if (M + 63) // 64 <= c)


def tandem(rng, model, reps):
    """Sharpened emissions back to back: a window long and strong enough for many odds-mode rescales (E(i) > 1e4)."""
    aa = np.concatenate(common.emit_from_model(rng, model, reps, flank=4, sharpen=3.0))
    return np.asarray(common.revtranslate(rng, aa, model.basic), dtype=np.uint8)


def tiling_windows(rng, model):
    """fs_windows / odds_windows at a size the oracle affords for this M: frameshifted model emissions, random DNA, degenerate
    codes and an N run, lengths 1, 2, 3, 15, 16, 17, 47, and a strong tandem.  Longer models: fewer and shorter windows."""
    M = model.M
    big = M > 512
    cap = 1500 if big else 3000
    wins = [w[:cap] for w in fs_windows(rng, model, 3 if big else 6)]
    deg = common.random_dna(rng, 1, 400)[0].copy()
    deg[50:70] = 15                                  # an N run
    deg[120] = 4; deg[200] = 7; deg[333] = 11        # ambiguity codes
    wins += [deg, common.random_dna(rng, 1, 1200 if big else 2500)[0], tandem(rng, model, 2 if big else 3)[:2 * cap]]
    wins += [rng.integers(0, 4, size=L).astype(np.uint8) for L in (1, 2, 3)]
    return wins


def envelopes(wins, model):
    """The windows FS5Envelopes / the multihit Forward take: at least 15 nt, cut so that (L+1)(M+1) 8 floats stay small."""
    cap, n = (600, 6) if model.M > 512 else (900, 12)
    env = [w[:cap] for w in wins if len(w) >= 15]
    env.sort(key=len, reverse=True)                  # the longest (the tandem, the emissions) first, then the short edge cases
    return env[:n - 3] + env[-3:]


@pytest.fixture(scope="module", params=FS_M, ids=["C%d-M%d" % (fs_columns(M), M) for M in FS_M])
def tiling(request, gpu_ctx, tmp_path_factory):
    M = request.param
    path = str(tmp_path_factory.mktemp("fs_tiling") / ("s%d.bhmm" % M))
    common.write_synthetic_bhmm(path, M, seed=M)
    model = ol.Model(path)
    hmm = ba.HMM(path)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5))
    wins = tiling_windows(np.random.default_rng(M + 7), model)
    assert max(len(w) for w in wins) >= 1200
    cache = {}                                       # oracle runs shared by the module's tests at this M
    return gpu_ctx, model, om3, om5, wins, ba.SeqBlock(gpu_ctx, wins), cache


def cached(cache, key, fn):
    if key not in cache:
        cache[key] = fn()
    return cache[key]


def oracle_rows_cmp(wins, backward):
    """The windows the scalar fs3 oracle accepts (it refuses L < 3, its Backward L <= 3)."""
    return [i for i, w in enumerate(wins) if len(w) >= (4 if backward else 3)]


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_fs3_strict_is_bit_identical(tiling, backward):
    ctx, model, om3, om5, wins, blk, cache = tiling
    fn = ba.FS3BackwardParser if backward else ba.FS3ForwardParser
    sc, xm = fn(ctx, om3, blk, logsum=ba.LOGSUM_TABLE_SERIAL, want_xmx=True)
    idx = oracle_rows_cmp(wins, backward)
    osc, oxm = cached(cache, ("table", backward), lambda: oracle_fs3(model, [wins[i] for i in idx], backward=backward))
    bad = [i for k, i in enumerate(idx) if not identical(sc[i], osc[k])]
    assert not bad, ("scores differ", [(len(wins[i]), sc[i]) for i in bad[:6]])
    bad = [i for k, i in enumerate(idx) if not identical(xm[i], oxm[k])]
    assert not bad, ("special-state rows differ", [len(wins[i]) for i in bad[:6]])
    if not backward:
        assert all(sc[i] == -np.inf for i, w in enumerate(wins) if len(w) < 3)


@pytest.mark.parametrize("mode,rtol,atol", [(ba.LOGSUM_TABLE, 1e-4, 5e-3), (ba.LOGSUM_EXACT, 1e-4, 1e-4)], ids=["fast", "exact"])
@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_fs3_fast_and_exact(tiling, backward, mode, rtol, atol, request):
    ctx, model, om3, om5, wins, blk, cache = tiling
    fn = ba.FS3BackwardParser if backward else ba.FS3ForwardParser
    sc, xm = fn(ctx, om3, blk, logsum=mode, want_xmx=True)
    idx = oracle_rows_cmp(wins, backward)
    if mode == ba.LOGSUM_EXACT:
        ex = [cached(cache, ("exact", backward), lambda: exact_oracle(model, wins, backward))[i] for i in idx]
        assert all(st == 0 for st, _, _ in ex)
        osc, oxm = np.array([o for _, o, _ in ex], np.float32), [r for _, _, r in ex]
    else:
        osc, oxm = cached(cache, ("table", backward), lambda: oracle_fs3(model, [wins[i] for i in idx], backward=backward))
    g = sc[idx]
    if mode == ba.LOGSUM_TABLE:
        record_errors("fs3_tiling/" + request.node.callspec.id, g, osc)
    assert close(g, osc, rtol, atol), np.abs(g - osc).max()
    if not backward:
        for k, i in enumerate(idx):                 # special-state rows, at the bars of test_fs3_forward_parser
            assert close(xm[i][2:], oxm[k][2:], rtol, 4 * atol), len(wins[i])
        assert all(sc[i] == -np.inf for i, w in enumerate(wins) if len(w) < 3)
    else:
        fsc = ba.FS3ForwardParser(ctx, om3, blk, logsum=mode)
        assert close(fsc[idx], g, 1e-4, 2e-2)       # Forward == Backward


def test_fs3_odds(tiling):
    ctx, model, om3, om5, wins, blk, cache = tiling
    fwd = ba.FS3ForwardParser(ctx, om3, blk, logsum=ba.LOGSUM_ODDS, want_xmx=True)
    bwd = ba.FS3BackwardParser(ctx, om3, blk, logsum=ba.LOGSUM_ODDS, want_xmx=True)
    # compare_parser allows four windows the oracle cannot score; the L = 1, 2 windows (-inf on the GPU) are checked apart from the rest
    short = [i for i, w in enumerate(wins) if len(w) < 3]
    rest = [i for i, w in enumerate(wins) if len(w) >= 3]
    for backward, (sc, xm) in ((False, fwd), (True, bwd)):
        ex = cached(cache, ("exact", backward), lambda: exact_oracle(model, wins, backward))
        sse = sse_oracle(model, wins, backward)
        for part in (short, rest):
            got = (sc[part], [xm[i] for i in part])
            pw = [wins[i] for i in part]
            compare_parser(model, pw, got, [ex[i] for i in part], backward)
            compare_parser(model, pw, got, [sse[i] for i in part], backward)
    fsc, bsc = fwd[0], bwd[0]
    fin = np.isfinite(fsc) & np.isfinite(bsc)
    assert np.all(np.abs(fsc[fin] - bsc[fin]) <= 2e-3 + 2e-4 * np.abs(fsc[fin]))           # Forward == Backward
    assert np.array_equal(np.isfinite(fsc), np.isfinite(bsc))
    assert fin.sum() >= len(wins) - 3


@pytest.mark.parametrize("mode", [ba.LOGSUM_TABLE, ba.LOGSUM_TABLE_SERIAL], ids=["scan", "strict"])
def test_fs5_envelopes(tiling, mode, request):
    ctx, model, om3, om5, wins, blk, cache = tiling
    check_fs5_envelopes(ctx, model, om5, envelopes(wins, model), mode, False, "tiling/" + request.node.callspec.id)


def test_fs5_multihit_forward_full(tiling):
    ctx, model, om3, om5, wins, blk, cache = tiling
    env = envelopes(wins, model)
    check_fs5_forward_full(ctx, model, om5, [env[0], env[-1]])


# ---- the fs5 wavefront's waves per envelope: each setting in a fresh process (the switches are read once)

WF_SCRIPT = r"""
import sys, os
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import bath_amd as ba, oracle_lib as ol, common
from test_frameshift_gpu import check_fs5_envelopes
from test_fs_tiling_gpu import tiling_windows, envelopes
ctx = ba.Context(0)
for M in {ms!r}:
    path = os.path.join({tmp!r}, "s%d.bhmm" % M)
    common.write_synthetic_bhmm(path, M, seed=M)
    model = ol.Model(path)
    om5 = ba.FSOProfile(ctx, ba.FSProfile(ba.HMM(path), 5))
    env = envelopes(tiling_windows(np.random.default_rng(M + 7), model), model)
    for mode in (ba.LOGSUM_TABLE_SERIAL, ba.LOGSUM_TABLE):
        check_fs5_envelopes(ctx, model, om5, env, mode, False)
    print("fs5 ok", M, len(env), flush=True)
ctx.close()
print("wavefront shape ok")
"""


def run_wf(tmp_path, switches, ms):
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-c", WF_SCRIPT.format(root=ROOT, tmp=str(tmp_path), ms=list(ms))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "wavefront shape ok" in r.stdout, (switches, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("W", WF_WAVES, ids=["W%d" % w for w in WF_WAVES])
def test_fs5_wavefront_waves_per_envelope(tmp_path, W):
    """BATH_HIP_WF_WAVES = W at M below and above the 64 W rows a block keeps in flight (fs_wf_period)."""
    run_wf(tmp_path, {"BATH_HIP_WF_WAVES": str(W)}, WF_M)


@pytest.mark.parametrize("W", [1, 4], ids=["W1", "W4"])
def test_fs5_wavefront_ring_in_global_memory(tmp_path, W):
    run_wf(tmp_path, {"BATH_HIP_WF_WAVES": str(W), "BATH_HIP_WF_RING_G": "1"}, WF_M)


def test_fs5_multiwave_decode_with_one_wave(tmp_path):
    """BATH_HIP_FS_OA_MW=1 at M = 1 and 64: the multi-wave decode / OA kernel with one wave and a mostly empty lane set."""
    run_wf(tmp_path, {"BATH_HIP_FS_OA_MW": "1"}, [1, 64])


def test_fs5_wavefront_heuristic_picks_one_wave_per_envelope(gpu_ctx):
    """3400 envelopes of 40..200 nt at M = 145: more than 12 per CU, so fs_wf_waves itself picks a wave per envelope (the
    bench's shape: 1024-thread blocks of 16 rings).  Strict scores of every envelope bit-identical; the optimal-accuracy matrix,
    its score and null2 of every 50th."""
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    assert model.M == 145
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(ba.HMM(path), 5))
    rng = np.random.default_rng(4000)
    src = fs_windows(rng, model, 400, with_degenerate=True)
    env = []
    while len(env) < 3400:
        w = src[int(rng.integers(0, len(src)))]
        L = int(rng.integers(40, 201))
        s = int(rng.integers(0, max(1, len(w) - L + 1)))
        if len(w[s:s + L]) >= 40:
            env.append(w[s:s + L].copy())
    got = ba.FS5Envelopes(gpu_ctx, om5, ba.SeqBlock(gpu_ctx, env), logsum=ba.LOGSUM_TABLE_SERIAL, want_oa=True)
    L_ = ol.lib()
    gm5 = model.fs(5)
    f, b = C.c_float(), C.c_float()
    bad = []
    for i, w in enumerate(env):
        L = len(w)
        d = ol.u8(ol.dsq_from(w))
        L_.bo_fs_profile_reconfig_unihit(gm5, L // 3)
        g8 = L_.bo_gmx_create(model.M, L + 1, L, 8)
        g3 = L_.bo_gmx_create(model.M, L + 1, L, 3)
        assert L_.bo_gforward_fs(d, L, gm5, g8, 0, C.byref(f)) == 0 and L_.bo_gbackward_fs(d, L, gm5, g3, C.byref(b)) == 0
        L_.bo_gmx_free(g8); L_.bo_gmx_free(g3)
        if not (identical(got["fwdsc"][i], f.value) and identical(got["bcksc"][i], b.value)):
            bad.append(i)
    L_.bo_fs_profile_reconfig_multihit(gm5, 100)
    assert not bad, ("strict scores differ", len(bad), bad[:8])
    from test_frameshift_gpu import oa_matrices_agree
    sample = list(range(0, len(env), 50))
    ref = oracle_fs5(model, [env[i] for i in sample], False)
    for i, r in zip(sample, ref):
        assert abs(got["oasc"][i] - r[2]) < 5e-4 + 1e-3 * abs(r[2])
        assert oa_matrices_agree(got["oa"][i], r[5], 5e-4, 1e-3)
        assert np.allclose(got["null2"][i], r[3], rtol=2e-3, atol=1e-4)


# ---- beyond the last tiling: refused, and the context stays usable

def test_models_beyond_1280_nodes_are_refused(gpu_ctx, tmp_path):
    M = FS_MAX_NODES + 1
    path = str(tmp_path / ("s%d.bhmm" % M))
    common.write_synthetic_bhmm(path, M, seed=M)
    hmm = ba.HMM(path)
    rng = np.random.default_rng(M)
    wins = [rng.integers(0, 4, size=L).astype(np.uint8) for L in (300, 90, 15)]
    blk = ba.SeqBlock(gpu_ctx, wins)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
    msg = "up to %d nodes" % FS_MAX_NODES
    for fn in (ba.FS3ForwardParser, ba.FS3BackwardParser):
        for mode in (ba.LOGSUM_TABLE, ba.LOGSUM_EXACT, ba.LOGSUM_TABLE_SERIAL, ba.LOGSUM_ODDS, ba.LOGSUM_CONTEXT):
            with pytest.raises(ba.BathError, match=msg):
                fn(gpu_ctx, om3, blk, logsum=mode, want_xmx=True)
    for mode in (ba.LOGSUM_TABLE, ba.LOGSUM_TABLE_SERIAL):
        with pytest.raises(ba.BathError, match=msg):
            ba.FS5Envelopes(gpu_ctx, om5, blk, logsum=mode, want_pp=True, want_oa=True)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    pipe = ba.Pipeline(gpu_ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
    with pytest.raises(ba.BathError, match=msg):
        pipe.run_frameshift_domains(om3, om5, blk)
    with pytest.raises(ba.BathError, match=msg):
        pipe.run_frameshift(om3, blk)
    # the same context, a 145-node model: the oracle's results
    path = ol.GOLDEN + "/Caudal_act.bhmm"
    model = ol.Model(path)
    hmm = ba.HMM(path)
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3))
    wins = fs_windows(np.random.default_rng(5), model, 6)
    sc, xm = ba.FS3ForwardParser(gpu_ctx, om3, ba.SeqBlock(gpu_ctx, wins), logsum=ba.LOGSUM_TABLE_SERIAL, want_xmx=True)
    osc, oxm = oracle_fs3(model, wins, backward=False)
    assert identical(sc, osc) and all(identical(g, o) for g, o in zip(xm, oxm))
    om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5))
    check_fs5_envelopes(gpu_ctx, model, om5, [w for w in wins if len(w) >= 15][:6], ba.LOGSUM_TABLE_SERIAL, False)
