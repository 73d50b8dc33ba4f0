"""fwd_group_kernel (bath_fwd_group.hip): the cascade's Forward parser with a quarter wave per target, four targets of a length-sorted
list per wave, for models of up to 160 nodes.

The contract is the Forward parser's (test_filters_gpu.py: test_forward_parser): status equal to the oracle's, score within
1e-4 relative / 2e-4 absolute nats of bo_forward_parser.  The kernel is not bit-identical to fwd_wave_kernel (its D scan and its
sum over the model associate differently); what must hold bit for bit is that a target's score does not depend on the targets
that share its wave.

Reached through ForwardParserGroup (every target of a block) and, in the cascade, through Context.set_fwd_group: 1 = the group
kernel whatever the block's size, 2 = never (0, the default, is 1's rule today)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol
from bath_amd import synth

pytestmark = pytest.mark.gpu

CAUDAL = os.path.join(ol.GOLDEN, "Caudal_act.bhmm")                 # M = 145: the bench model
# one lane and the lane seam at 10 nodes a lane; the last lane partly filled, one node short, full
MODELS = ["synthetic:1", "synthetic:9", "synthetic:10", "synthetic:11", "Caudal_act.bhmm", "synthetic:151", "synthetic:159", "synthetic:160"]
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 333]                          # the four-residue read's seam, a wave's 64, the longest ORF of a 1 kb window
LISTS = [1, 3, 4, 5, 257]                                           # a partly filled group of four, idle groups, full waves beside a partly filled one
RTOL, ATOL = 1e-4, 2e-4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fit(rng, seq, L):
    """<seq> cut or padded with background residues to L residues."""
    if len(seq) >= L:
        a = int(rng.integers(0, len(seq) - L + 1))
        return np.asarray(seq[a:a + L], dtype=np.uint8)
    pad = common.random_aa(rng, 1, L - len(seq), L - len(seq), with_degenerate=False)[0]
    return np.concatenate([seq, pad]).astype(np.uint8)


def load(gpu_ctx, tmp, name):
    if name.startswith("synthetic:"):
        M = int(name.split(":")[1])
        path = synth.write_synthetic_bhmm(str(tmp / ("s%d.bhmm" % M)), M, seed=M)
    else:
        path = os.path.join(ol.GOLDEN, name)
    return ol.Model(path, 0), ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))


@pytest.fixture(scope="module", params=MODELS)
def scored(request, gpu_ctx, tmp_path_factory):
    """257 targets of a model, every length of LENGTHS among the first nine and homologs beside background sequences, with the
    oracle's scores: computed once, shared by the lists below."""
    model, om = load(gpu_ctx, tmp_path_factory.mktemp("fwdg"), request.param)
    rng = np.random.default_rng(7 + model.M)
    hom = common.emit_from_model(rng, model, 97, flank=12) + common.emit_from_model(rng, model, 32, flank=12, sharpen=3.0)
    bg = common.random_aa(rng, 129, 20, 333)
    seqs = []
    for i in range(max(LISTS)):
        L = LENGTHS[i % len(LENGTHS)] if i < 2 * len(LENGTHS) else None
        src = hom[i // 2] if i % 2 == 0 else bg[i // 2]
        seqs.append(fit(rng, src, L if L is not None else min(len(src), 333)))
    assert sorted(set(len(s) for s in seqs[:len(LENGTHS)])) == LENGTHS
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    return gpu_ctx, model, om, seqs, osc, ost


@pytest.mark.parametrize("n", LISTS)
def test_group_kernel_against_the_oracle(scored, n):
    ctx, model, om, seqs, osc, ost = scored
    sc, st = ba.ForwardParserGroup(ctx, om, ba.SeqBlock(ctx, seqs[:n]))
    assert np.array_equal(st, ost[:n])
    ok = ost[:n] == 0
    assert ok.any()
    assert np.allclose(sc[ok], osc[:n][ok], rtol=RTOL, atol=ATOL), np.abs(sc[ok] - osc[:n][ok]).max()
    assert np.array_equal(bits(sc[~ok]), bits(osc[:n][~ok]))


@pytest.fixture(scope="module")
def caudal(gpu_ctx, tmp_path_factory):
    return load(gpu_ctx, tmp_path_factory.mktemp("fwdg_c"), "Caudal_act.bhmm")


def solo(ctx, om, seqs):
    """Each target scored alone through the same entry point."""
    out = [ba.ForwardParserGroup(ctx, om, ba.SeqBlock(ctx, [s])) for s in seqs]
    return np.array([o[0][0] for o in out], np.float32), np.array([o[1][0] for o in out], np.int32)


def test_a_group_does_not_depend_on_its_neighbours(gpu_ctx, caudal):
    """Lengths alternate 1 and 333: the sort puts the eight long ones into two waves and the eight short ones into two more, and a
    second list of five (333, 1, 333, 1, 333) makes one wave's four targets end at rows 1 and 333.  Bit for bit the solo scores."""
    model, om = caudal
    rng = np.random.default_rng(11)
    hom = common.emit_from_model(rng, model, 16, flank=12)
    seqs = [fit(rng, hom[i], 333 if i % 2 else 1) for i in range(16)]
    one_sc, one_st = solo(gpu_ctx, om, seqs)
    for lst in (list(range(16)), [1, 0, 3, 2, 5]):
        sc, st = ba.ForwardParserGroup(gpu_ctx, om, ba.SeqBlock(gpu_ctx, [seqs[i] for i in lst]))
        assert np.array_equal(st, one_st[lst]) and np.array_equal(bits(sc), bits(one_sc[lst]))
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    assert np.array_equal(one_st, ost) and np.allclose(one_sc, osc, rtol=RTOL, atol=ATOL)


def test_more_jobs_than_waves(gpu_ctx, caudal):
    """The grid is one block per CU, four waves each, a job of four targets per wave to begin with: a list of more than 16 targets
    per CU has waves take further jobs from the kernel's counter.  Short targets, so that the oracle stays quick."""
    model, om = caudal
    cus = ba.lib().bath_selftest_compute_units(gpu_ctx._h)
    assert cus > 0
    rng = np.random.default_rng(23)
    n = 16 * cus + 601
    seqs = common.random_aa(rng, n, 1, 24, with_degenerate=False)
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    sc, st = ba.ForwardParserGroup(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs))
    assert np.array_equal(st, ost) and (ost == 0).all()
    assert np.allclose(sc, osc, rtol=RTOL, atol=ATOL), np.abs(sc - osc).max()


def test_rescaling_is_a_groups_own(gpu_ctx, caudal):
    """One target carries the model's consensus from node 1 to node M, so that its xE passes 1e4 and the row rescales (asserted from
    the oracle's SCALE column), in a wave with three background targets that never rescale."""
    model, om = caudal
    h = model.hmm.contents
    mat = np.ctypeslib.as_array(h.mat, shape=((h.M + 1) * 20,)).reshape(h.M + 1, 20)
    rng = np.random.default_rng(13)
    flank = common.random_aa(rng, 2, 10, 10, with_degenerate=False)
    planted = np.concatenate([flank[0], mat[1:].argmax(axis=1).astype(np.uint8), flank[1]])
    seqs = common.random_aa(rng, 3, len(planted) - 2, len(planted), with_degenerate=False)
    seqs.insert(1, planted)
    L_ = ol.lib()
    out = C.c_float(0)
    scales = []
    for s in seqs:
        L_.bo_oprofile_reconfig_length(model.om, len(s))
        fx = np.zeros((len(s) + 1) * 6, np.float32)
        assert L_.bo_forward_parser(ol.u8(ol.dsq_from(s)), len(s), model.om, fx.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == 0
        scales.append(fx.reshape(-1, 6)[:, 5])
    assert (scales[1] > 1.0).any() and not any((scales[i] > 1.0).any() for i in (0, 2, 3))
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    sc, st = ba.ForwardParserGroup(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs))
    assert np.array_equal(st, ost) and np.allclose(sc, osc, rtol=RTOL, atol=ATOL)
    one_sc, one_st = solo(gpu_ctx, om, seqs)
    assert np.array_equal(st, one_st) and np.array_equal(bits(sc), bits(one_sc))


def test_a_longer_model_is_refused(gpu_ctx, tmp_path):
    model, om = load(gpu_ctx, tmp_path, "synthetic:161")
    rng = np.random.default_rng(17)
    seqs = common.random_aa(rng, 5, 20, 60)
    sq = ba.SeqBlock(gpu_ctx, seqs)
    sc, st = np.zeros(sq.n, np.float32), np.zeros(sq.n, np.int32)
    rc = ba.lib().bath_hip_fwdparser_group(gpu_ctx._h, om._h, sq._h, sc.ctypes.data_as(C.POINTER(C.c_float)), st.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == ba.EINVAL
    with pytest.raises(ba.BathError, match="160 nodes"):
        ba.ForwardParserGroup(gpu_ctx, om, sq)
    # the context goes on: the same targets by the wave kernel, and a model that fits by the group kernel
    wsc, wst = ba.ForwardParser(gpu_ctx, om, sq)
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    assert np.array_equal(wst, ost) and np.allclose(wsc, osc, rtol=RTOL, atol=ATOL)
    model2, om2 = load(gpu_ctx, tmp_path, "synthetic:160")
    gsc, gst = ba.ForwardParserGroup(gpu_ctx, om2, sq)
    osc, ost = common.oracle_scores(model2, seqs, "bo_forward_parser")
    assert np.array_equal(gst, ost) and np.allclose(gsc, osc, rtol=RTOL, atol=ATOL)


# ---- the cascade ----------------------------------------------------------------------------------------------------
COUNTERS = ("nres", "n_orfs", "n_past_msv", "n_past_bias", "n_past_vit", "n_past_fwd", "pos_past_msv", "pos_past_bias", "pos_past_vit", "pos_past_fwd")
PIPE_WINDOWS, PIPE_SEED, PIPE_PLANTED = 2000, 57, 0.05
F3_BAND = 1e-4              # a candidate whose Forward P-value is this close to F3 (relative) may fall on either side; the block has none


@contextlib.contextmanager
def cascade(ctx, mode, parts):
    """The cascade's Forward stage by the group kernel (mode 1) or never (2), the block as one part or as two (read at every call)."""
    old = os.environ.get("BATH_HIP_LANES")
    os.environ["BATH_HIP_LANES"] = str(parts)
    ctx.set_fwd_group(mode)
    try:
        yield
    finally:
        ctx.set_fwd_group(0)
        if old is None:
            del os.environ["BATH_HIP_LANES"]
        else:
            os.environ["BATH_HIP_LANES"] = old


def pipe_block(hmm):
    flat, _, _ = synth.dna_windows(PIPE_WINDOWS, 1000, seed=PIPE_SEED, hmm=hmm, planted_frac=PIPE_PLANTED)
    return list(flat.reshape(PIPE_WINDOWS, 1000))


def run_cascade(ctx, om, hmm, wins, mode, parts):
    with cascade(ctx, mode, parts):
        pipe = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct)
        stats, res = pipe.run(ba.SeqBlock(ctx, wins))
        launches = {n: k for n, _, k in pipe.timings()}["forward_final"]
    res = res[np.lexsort((res["start"], res["frame"], res["strand"], res["window"]))]
    return {c: int(getattr(stats, c)) for c in COUNTERS}, res, launches


@pytest.fixture(scope="module")
def pipeline_world(gpu_ctx):
    hmm = ba.HMM(CAUDAL)
    model = ol.Model(CAUDAL)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    wins = pipe_block(hmm)
    pli, ores, per_seq = model.run_pipeline(wins)
    want = {c: int(getattr(pli, c)) for c in COUNTERS}
    fwd = [(w, o) for w, (a, b) in enumerate(per_seq) for o in ores[a:b] if o.stage >= 3]
    runs = {(mode, parts): run_cascade(gpu_ctx, om, hmm, wins, mode, parts) for mode in (1, 2) for parts in (1, 2)}
    return hmm, model, want, pli.F3, fwd, runs


def test_no_forward_candidate_of_the_block_lies_at_f3(pipeline_world):
    """The counters below are compared without exception: in the oracle no Forward candidate's P-value is within 1e-4 relative of F3."""
    _, _, want, F3, fwd, _ = pipeline_world
    assert len(fwd) >= 100 and want["n_past_fwd"] >= 50 and want["n_past_fwd"] < len(fwd)
    assert not [o.P for _, o in fwd if abs(o.P - F3) <= F3_BAND * F3]


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("mode", [1, 2])
def test_cascade_counters_equal_the_oracles(pipeline_world, mode, parts):
    _, _, want, _, fwd, runs = pipeline_world
    got, res, launches = runs[(mode, parts)]
    assert got == want
    # the path taken: the sort's three kernels, the group kernel and final_kernel, or the wave kernel and final_kernel; per part
    assert launches == parts * (5 if mode == 1 else 2)
    key = sorted((w, o.strand, o.frame, o.start) for w, o in fwd)
    have = res[res["stage"] >= 3]
    assert sorted(zip(have["window"].tolist(), have["strand"].tolist(), have["frame"].tolist(), have["start"].tolist())) == key
    osc = {(w, o.strand, o.frame, o.start): o.fwdsc for w, o in fwd}
    o = np.array([osc[k] for k in zip(have["window"].tolist(), have["strand"].tolist(), have["frame"].tolist(), have["start"].tolist())], np.float32)
    assert np.allclose(have["fwdsc"], o, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("parts", [1, 2])
def test_cascade_records_of_the_two_kernels_are_equal_but_for_the_forward_score(pipeline_world, parts):
    """... and for P where it is Forward's: P = exp(-lambda (fwdsc - filtersc) / ln 2 + ...), so two scores that are each within
    tol of the oracle's leave ln P within lambda / ln 2 * 2 tol of each other (and the float seqsc's rounding, 1e-5)."""
    hmm, _, _, _, _, runs = pipeline_world
    a, b = runs[(1, parts)][1], runs[(2, parts)][1]
    assert len(a) == len(b)
    for f in a.dtype.names:
        if f not in ("fwdsc", "P"):
            assert np.array_equal(a[f], b[f]), f
    past = a["stage"] >= 3
    assert np.array_equal(bits(a["fwdsc"][~past]), bits(b["fwdsc"][~past])) and np.array_equal(a["P"][~past], b["P"][~past])
    tol = ATOL + RTOL * np.abs(b["fwdsc"][past])
    assert (np.abs(a["fwdsc"][past] - b["fwdsc"][past]) <= 2 * tol).all()
    lam = float(hmm.evparam[5])
    assert (np.abs(np.log(a["P"][past]) - np.log(b["P"][past])) <= lam / np.log(2.0) * 2 * tol + 1e-5).all()


def test_cascade_of_a_longer_model_keeps_the_wave_kernel(gpu_ctx, tmp_path):
    """M = 161 under mode 1: the stage falls back to fwd_wave_kernel and the counters are the oracle's."""
    path = synth.write_synthetic_bhmm(str(tmp_path / "s161.bhmm"), 161, seed=161)
    hmm, model = ba.HMM(path, 0), ol.Model(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    rng = np.random.default_rng(19)
    wins = [np.array(common.revtranslate(rng, aa, model.basic), dtype=np.uint8) for aa in common.emit_from_model(rng, model, 24, flank=10)]
    wins += common.random_dna(rng, 40, 900)
    pli, ores, _ = model.run_pipeline(wins)
    got, res, launches = run_cascade(gpu_ctx, om, hmm, wins, 1, 1)
    assert got == {c: int(getattr(pli, c)) for c in COUNTERS} and got["n_past_fwd"] > 0
    assert launches == 2
