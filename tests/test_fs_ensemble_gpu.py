"""GPU tier: the trace ensemble of multi-domain regions on the device (ENSEMBLE_STREAMS_DEVICE, fs_ensemble_kernel).

The kernel and the host twin compile one walk (bath_fs_ens_walk.hpp) and start every trace from the same state, so on the same
Forward matrix they must give the same status and the same segments for every one of a region's 200 traces, and therefore the same
envelopes: the first test holds bath_hip_fs5_region_ensembles in device mode against the twin fed the matrices that
bath_hip_fs5_forward_full reads back, strict and in the 5-codon odds mode.  The second runs the --fs pipeline in all three modes;
the third the bathsearch command line.

A region of L >= 5 whose multihit Forward is -inf cannot be built from DNA (nucleotide codes outside ACGT read the
profile's finite degenerate-codon row, stop codons are -inf only as whole 3-nt codons while the 1-, 2-, 4- and 5-nt quasi-codons
around them stay finite, and the multihit configuration always has the path N..B -> M -> E -> C..), so the score = -inf branch is
held by the regions the Forward kernels themselves refuse: L < 5, in the strict, the fast and the odds-ratio Forward."""
import io
import os
import sys

import numpy as np
import pytest

import bath_amd as ba
from bath_amd import bathsearch, synth
import common
import oracle_lib as ol
import shutil
import subprocess

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XNL, XNM, XE = ba.fs_ensemble_loop_scores(100)


def consensus_two_copy_window(hmm, seed, spacer):
    """flank + gene + <spacer> random nt + gene + flank; the gene is the model's consensus, reverse-translated per copy (bath_amd.synth)"""
    rng = np.random.default_rng(seed)
    aa = synth.hmm_match_emissions(hmm)[1:].argmax(axis=1).astype(np.uint8)
    basic = ba.gencode_basic(hmm.ct)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    return np.concatenate([rnd(30), synth.reverse_translate(rng, aa, basic), rnd(spacer), synth.reverse_translate(rng, aa, basic), rnd(30)])


def overlap_ok(a, b):
    """The project's link criterion (cluster_segments: min_overlap): shared nucleotides >= 0.8 of the shorter envelope."""
    nov = min(a[1], b[1]) - max(a[0], b[0]) + 1
    return nov / min(a[1] - a[0] + 1, b[1] - b[0] + 1) >= 0.8


def random_regions(rng, n, lo, hi):
    return [rng.integers(0, 4, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8) for _ in range(n)]


def consensus_regions(rng, hmm, n, lo, hi):
    """random DNA around the first nodes of the model's consensus, as many as fit: regions with a real domain in them"""
    aa = synth.hmm_match_emissions(hmm)[1:].argmax(axis=1).astype(np.uint8)
    basic = ba.gencode_basic(hmm.ct)
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        gene = synth.reverse_translate(rng, aa, basic)[: max(3, (L - 10) // 3 * 3)]
        w = rng.integers(0, 4, size=L, dtype=np.uint8)
        p = int(rng.integers(0, L - len(gene) + 1))
        w[p:p + len(gene)] = gene
        out.append(w)
    return out


def shapes(tmp, cus):
    """(name, model path, regions)"""
    rng = np.random.default_rng(5)
    out = []
    for M in (1, 7):
        path = common.write_synthetic_bhmm(str(tmp / ("e%d.bhmm" % M)), M, seed=10 + M)
        hmm = ba.HMM(path, 0)
        out.append(("M%d" % M, path, random_regions(rng, 3, 5, 40) + consensus_regions(rng, hmm, 4, 24, 70)))
    for name, wseed in (("PTH2.bhmm", 11), ("Caudal_act.bhmm", 21)):
        path = ol.GOLDEN + "/" + name
        hmm = ba.HMM(path, 0)
        out.append((name, path, [consensus_two_copy_window(hmm, wseed, 40), consensus_two_copy_window(hmm, wseed + 1, 300)[:700]] + random_regions(rng, 2, 90, 200)))
    path = common.write_synthetic_bhmm(str(tmp / "e1025.bhmm"), 1025, seed=1025)
    out.append(("M1025", path, consensus_regions(rng, ba.HMM(path, 0), 1, 120, 120)))       # the long-model Forward layout, one short region
    path = str(tmp / "e7.bhmm")
    out.append(("short", path, random_regions(rng, 3, 4, 4)))                               # L < 5
    n = max(300, 4 * cus + 44)                                                                 # more regions than blocks: the job loop wraps
    out.append(("batch", path, consensus_regions(rng, ba.HMM(path, 0), n, 50, 70)))
    return out


@pytest.mark.parametrize("arith", ["strict", "odds5", "fast"])
def test_device_ensemble_is_the_host_twin(gpu_ctx, tmp_path, arith):
    """The ensemble kernel must not care which Forward wrote the matrix: the strict chains, the 5-codon odds-ratio kernel, or the fast
    mode's fs5_fwd_kernel."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = gpu_ctx
    odds5 = arith == "odds5"
    ctx.set_fs_strict(arith != "fast")
    ctx.set_fs5_odds(odds5)
    before = ctx.fs_ensemble_counters()
    try:
        for name, path, regions in shapes(tmp_path, cus):
            hmm = ba.HMM(path, 0)
            gm5 = ba.FSProfile(hmm, 5, ncbi_table=hmm.ct)
            tsc = gm5.arrays()[0].astype(np.float32)
            om5 = ba.FSOProfile(ctx, gm5)
            blk = ba.SeqBlock(ctx, regions)
            M = hmm.M
            ctx.set_fs_ensemble(ba.ENSEMBLE_STREAMS_DEVICE)
            dev = ba.FS5RegionEnsembles(ctx, om5, blk, seed=42)
            sc, fwd, fx = ba.FS5ForwardFull(ctx, om5, blk, 100)
            n_ok = n_env = 0
            for r, w in enumerate(regions):
                L = len(w)
                if name == "short":                             # L < 5: every regions' Forward answers -inf, and the ensemble "no valid traces"
                    assert sc[r] == -np.inf
                if not sc[r] > -np.inf:
                    assert name == "short", (name, r, L)        # (no other shape underflows)
                    assert dev[r]["status"] == ba.ENS_REGION_NO_TRACES and dev[r]["envelopes"] == [] and len(dev[r]["segments"]) == 0
                    assert (dev[r]["trace_status"] == ba.ENS_IMPOSSIBLE).all()
                    continue
                twin = ba.fs_ensemble_streams(M, tsc, XNL, XNM, XE, 1, L, fwd[r], fx[r], seed=42)
                assert np.array_equal(dev[r]["trace_status"], twin["trace_status"]), (name, r, L)
                assert dev[r]["status"] == twin["status"], (name, r, L)
                assert np.array_equal(dev[r]["segments"], twin["segments"]), (name, r, L)
                assert dev[r]["envelopes"] == twin["envelopes"], (name, r, L)
                n_ok += twin["status"] == ba.ENS_REGION_OK
                n_env += len(twin["envelopes"])
            print(name, arith, "regions", len(regions), "with traces", n_ok, "envelopes", n_env)
            if name != "short":
                assert n_ok >= 1
            if name in ("PTH2.bhmm", "Caudal_act.bhmm"):
                assert n_env >= 3                               # the two-copy windows do cluster into their copies
            if name == "batch":                                 # ... and the host mode of the same entry point is the twin too
                ctx.set_fs_ensemble(ba.ENSEMBLE_STREAMS_HOST)
                sub = ba.SeqBlock(ctx, regions[:5])
                host = ba.FS5RegionEnsembles(ctx, om5, sub, seed=42)
                for r in range(5):
                    assert host[r]["envelopes"] == dev[r]["envelopes"] and np.array_equal(host[r]["segments"], dev[r]["segments"])
        after = ctx.fs_ensemble_counters()
        assert after["bound_fallbacks"] == before["bound_fallbacks"] and after["overflow_fallbacks"] == before["overflow_fallbacks"]
        assert after["matrix_bytes_kept"] > before["matrix_bytes_kept"]
    finally:
        ctx.set_fs_ensemble(ba.ENSEMBLE_SERIAL)
        ctx.set_fs5_odds(False)
        ctx.set_fs_strict(True)


# ---- the pipeline

def pipeline_block(hmm, seed=7):
    """About 200 windows built with bath_amd.synth: 20 with two frameshifted copies of a sampled domain a short spacer apart (their
    posterior profile is a multi-domain region), 20 with one frameshifted copy, the rest random.  Returns (windows, two-copy indices)."""
    rng = np.random.default_rng(seed)
    mat = synth.hmm_match_emissions(hmm)
    basic = ba.gencode_basic(hmm.ct)

    def copy():
        nt = list(synth.reverse_translate(rng, synth.sample_domain(rng, mat), basic))
        del nt[int(rng.integers(10, len(nt) - 10))]             # one frameshift per copy
        return nt
    rnd = lambda n: list(rng.integers(0, 4, size=n))
    wins, two = [], []
    for w in range(200):
        if w % 10 == 0:
            two.append(w)
            wins.append(np.array(copy() + rnd(int(rng.integers(20, 60))) + copy(), dtype=np.uint8))
        elif w % 10 == 5:
            wins.append(np.array(rnd(150) + copy() + rnd(150), dtype=np.uint8))
        else:
            wins.append(rng.integers(0, 4, size=800, dtype=np.uint8))
    return wins, two


def domain_key(d):
    return (d.window, d.strand, d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm, d.n_shifted_codons, E_bits(d.envsc), E_bits(d.bitscore), d.reported, d.cigar)


def E_bits(x):
    return int(np.float32(x).view(np.uint32))


def test_pipeline_modes(gpu_ctx):
    ctx = gpu_ctx
    ctx.set_fs_strict(True)
    path = ol.GOLDEN + "/PTH2.bhmm"
    hmm = ba.HMM(path, 0)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
    wins, two = pipeline_block(hmm)
    blk = ba.SeqBlock(ctx, wins)
    pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
    res = {}
    before = ctx.fs_ensemble_counters()
    try:
        for mode in (ba.ENSEMBLE_SERIAL, ba.ENSEMBLE_STREAMS_HOST, ba.ENSEMBLE_STREAMS_DEVICE):
            ctx.set_fs_ensemble(mode)
            stats, fw, dm, nclust = pipe.run_frameshift_domains(om3, om5, blk)
            res[mode] = (dm, pipe.traces(), nclust, pipe.kernel_times())
    finally:
        ctx.set_fs_ensemble(ba.ENSEMBLE_SERIAL)
    after = ctx.fs_ensemble_counters()
    d0, d1, d2 = (res[m][0] for m in (0, 1, 2))
    assert res[0][2] > 0 and res[0][2] == res[1][2] == res[2][2]            # n_clustered_regions
    assert "fs_ensemble_kernel" in res[2][3] and "fs_ensemble_kernel" not in res[0][3] and "fs_ensemble_kernel" not in res[1][3]
    assert after["bound_fallbacks"] == before["bound_fallbacks"] and after["overflow_fallbacks"] == before["overflow_fallbacks"]
    # host streams and device streams: the same domains record for record, the same traces
    assert [domain_key(d) for d in d1] == [domain_key(d) for d in d2]
    for (t1, *a1), (t2, *a2) in zip(res[1][1], res[2][1]):
        assert (t1.N, t1.off) == (t2.N, t2.off) and all(np.array_equal(x, y) for x, y in zip(a1, a2))
    assert len(res[1][1]) == len(res[2][1]) == len(d2)
    # against the serial mode: windows without a multi-domain region exactly; the two-copy windows as two seeds of the serial mode
    # agree (tests/test_fs_ensemble_cpu.py): the same number of domains, envelopes overlapping by >= 0.8 of the shorter
    by_win = lambda dm: {w: sorted((d for d in dm if d.window == w), key=lambda d: (d.strand, min(d.ienv, d.jenv))) for w in range(len(wins))}
    w0, w2 = by_win(d0), by_win(d2)
    # which windows hold a multi-domain region: the pipeline's own count on the window alone (a single copy can be one too)
    clustered = set()
    for w in range(len(wins)):
        if w % 10 in (0, 5) and pipe.run_frameshift_domains(om3, om5, ba.SeqBlock(ctx, [wins[w]]))[3] > 0:
            clustered.add(w)
    assert len(clustered) >= 3 and any(w % 10 == 5 and w not in clustered and w0[w] for w in range(len(wins)))     # both kinds are present
    n_two = 0
    for w in range(len(wins)):
        if w not in clustered:
            assert [domain_key(d) for d in w0[w]] == [domain_key(d) for d in w2[w]], w
            continue
        assert len(w0[w]) == len(w2[w]), (w, [(d.ienv, d.jenv) for d in w0[w]], [(d.ienv, d.jenv) for d in w2[w]])
        for a, b in zip(w0[w], w2[w]):
            ea, eb = sorted((a.ienv, a.jenv)), sorted((b.ienv, b.jenv))
            assert a.strand == b.strand and overlap_ok(ea, eb), (w, ea, eb)
        n_two += len(w2[w]) >= 2
    print("clustered regions", res[2][2], "windows holding one", len(clustered), "two-copy windows with two domains or more", n_two, "domains", len(d2),
          "fs_ensemble_kernel ms", res[2][3]["fs_ensemble_kernel"][0])


# ---- the command line

IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")      # timing lines; the tail echoes the command line


def strip(text):
    return [ln for ln in text.split("\n") if not ln.startswith(IGNORED)]


def golden_copy(d):
    d.mkdir()
    for f in ("AMP_N.bhmm", "target-AMP_N.fa"):
        shutil.copy(os.path.join(ol.GOLDEN, f), d / f)
    return d


def test_cli_device_equals_streams(tmp_path, monkeypatch):
    argv = lambda mode: ["--fs", "--ensemble", mode, "-o", "out.txt", "--tblout", "out.tbl", "--cigar", "AMP_N.bhmm", "target-AMP_N.fa"]
    outs = {}
    for mode in ("streams", "device"):
        d = golden_copy(tmp_path / mode)
        code = "import sys; from bath_amd import bathsearch as b; sys.exit(b.run(sys.argv[1:]))"
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code] + argv(mode), cwd=str(d), env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[mode] = (strip((d / "out.txt").read_text()), strip((d / "out.tbl").read_text()))
        assert not any("ensemble" in ln for ln in outs[mode][0] if ln.startswith("#")), "an extension option prints no header line"
    assert outs["streams"][0] == outs["device"][0]
    assert outs["streams"][1] == outs["device"][1]
    assert len(outs["device"][1]) > 3


def test_cli_device_equals_streams_on_multi_domain_regions(tmp_path, monkeypatch):
    """The recorded AMP_N search holds no multi-domain region (the counters say so below), so the same comparison on targets that do:
    the two-copy and one-copy windows of the pipeline test as FASTA records, PTH2 as the query, bathsearch.run in this process so that
    the counters of the context it made can be read."""
    made = []
    setter = ba.Context.set_fs_ensemble

    def keeping(self, mode):
        made.append(self)
        setter(self, mode)
    monkeypatch.setattr(ba.Context, "set_fs_ensemble", keeping)
    hmm = ba.HMM(ol.GOLDEN + "/PTH2.bhmm", 0)
    wins, _ = pipeline_block(hmm)
    d = tmp_path / "planted"
    d.mkdir()
    shutil.copy(os.path.join(ol.GOLDEN, "PTH2.bhmm"), d / "PTH2.bhmm")
    with open(d / "targets.fa", "w") as f:
        for w in range(0, len(wins), 5):                                     # the gene-bearing windows
            f.write(">win%d\n%s\n" % (w, "".join("ACGT"[c] for c in wins[w])))
    for f in ("AMP_N.bhmm", "target-AMP_N.fa"):
        shutil.copy(os.path.join(ol.GOLDEN, f), d / f)
    monkeypatch.chdir(d)
    outs, kept = {}, {}
    for mode, q, t in (("streams", "PTH2.bhmm", "targets.fa"), ("device", "PTH2.bhmm", "targets.fa"), ("device", "AMP_N.bhmm", "target-AMP_N.fa")):
        del made[:]
        assert bathsearch.run(["--fs", "--ensemble", mode, "-o", "out.txt", "--tblout", "out.tbl", "--cigar", q, t], stdout=io.StringIO()) == 0
        assert len(made) == 1
        c = made[0].fs_ensemble_counters()
        assert c["bound_fallbacks"] == 0 and c["overflow_fallbacks"] == 0
        outs[mode, q] = (strip((d / "out.txt").read_text()), strip((d / "out.tbl").read_text()))
        kept[mode, q] = c["matrix_bytes_kept"]
    assert kept["device", "PTH2.bhmm"] > 0 and kept["streams", "PTH2.bhmm"] == 0          # regions did go through the kernel
    assert kept["device", "AMP_N.bhmm"] == 0                                              # (the recorded search: none)
    assert outs["streams", "PTH2.bhmm"] == outs["device", "PTH2.bhmm"]
    assert sum(not ln.startswith("#") and ln != "" for ln in outs["device", "PTH2.bhmm"][1]) >= 20


def test_cli_refuses_an_unknown_ensemble_mode(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(golden_copy(tmp_path / "g"))
    assert bathsearch.run(["--fs", "--ensemble", "sideways", "AMP_N.bhmm", "target-AMP_N.fa"], stdout=io.StringIO()) == 1
    assert "--ensemble" in capsys.readouterr().err
