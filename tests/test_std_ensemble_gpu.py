"""GPU tier: the standard branch's trace ensemble of multi-domain regions on the device (set_std_ensemble: ENSEMBLE_STREAMS_DEVICE,
std_ensemble_kernel).

The kernel and the host twin compile one walk (bath_std_ens_walk.hpp) and start every trace from the same state, so on the same
Forward matrix every one of a region's 200 traces must come out with the same status and the same segments; the null2 corrections
are computed on the host from segments and path codes by one piece of code for both, so they and the envelopes must be identical
too.  Stage level: bath_hip_std_region_ensembles in mode 2 against mode 1.  Pipeline level: run_hits and the standard branch of
run_frameshift_domains.  Then the bathsearch command line."""
import os
import shutil

import numpy as np
import pytest

import bath_amd as ba
from bath_amd import synth
import common
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted_region(rng, aa, copies, spacer, flank=8):
    """flank + domain + (<spacer> random residues + domain) * (copies - 1) + flank, amino-acid codes"""
    rnd = lambda n: rng.integers(0, 20, size=n, dtype=np.uint8)
    parts = [rnd(flank), aa]
    for _ in range(copies - 1):
        parts += [rnd(spacer), aa]
    return np.concatenate(parts + [rnd(flank)])


def shapes(tmp):
    """(name, model path, regions, how many of them overflow the kernel's 8 segments per trace).  Models of 1, 64, 65 and 129 nodes and a
    golden one; per model a two-copy and a three-copy region of the consensus, a random region, and two regions that hold no path and
    score -inf: an EMPTY one, which nobody walks, and nine '*' symbols (code 27: no match state emits it, and a multihit path needs a
    match), which the kernel and the twin do walk, every trace into an impossible state.  The 7-node model's 12-copy regions have 10
    segments or more in every trace."""
    rng = np.random.default_rng(5)
    out = []
    for M in (1, 64, 65, 129):
        path = common.write_synthetic_bhmm(str(tmp / ("s%d.bhmm" % M)), M, seed=10 + M)
        aa = synth.hmm_match_emissions(ba.HMM(path, 0))[1:].argmax(axis=1).astype(np.uint8)
        cp = (8, 12) if M == 1 else (2, 3)                   # (a one-node model: more copies, still within 8 segments a trace)
        out.append(("M%d" % M, path, [planted_region(rng, aa, cp[0], 12), planted_region(rng, aa, cp[1], 9), rng.integers(0, 20, size=57, dtype=np.uint8),
                                      np.zeros(0, np.uint8), np.full(9, 27, np.uint8)], 0))
    path = ol.GOLDEN + "/PTH2.bhmm"
    aa = synth.hmm_match_emissions(ba.HMM(path, 0))[1:].argmax(axis=1).astype(np.uint8)
    out.append(("PTH2", path, [planted_region(rng, aa, 2, 40), planted_region(rng, aa, 3, 25)], 0))
    path = common.write_synthetic_bhmm(str(tmp / "s7.bhmm"), 7, seed=17)
    aa = synth.hmm_match_emissions(ba.HMM(path, 0))[1:].argmax(axis=1).astype(np.uint8)
    out.append(("M7x12", path, [planted_region(rng, aa, 12, 6, flank=5), planted_region(rng, aa, 2, 6), planted_region(rng, aa, 12, 12, flank=5)], 2))
    return out


@pytest.mark.parametrize("seed", [42, 1, 987654321])
def test_device_ensemble_is_the_host_twin(gpu_ctx, tmp_path, seed):
    ctx = gpu_ctx
    try:
        for name, path, regions, n_over in shapes(tmp_path):
            hmm = ba.HMM(path, 0)
            om = ba.OProfile(ctx, ba.Profile(hmm))
            blk = ba.SeqBlock(ctx, regions)
            cfg = np.array([len(r) + 40 for r in regions], np.int32)      # the ORF a region lies in is longer than the region
            before = ctx.std_ensemble_counters()
            ctx.set_std_ensemble(ba.ENSEMBLE_STREAMS_HOST)
            host = ba.StdRegionEnsembles(ctx, om, blk, cfg, seed=seed)
            mid = ctx.std_ensemble_counters()
            ctx.set_std_ensemble(ba.ENSEMBLE_STREAMS_DEVICE)
            dev = ba.StdRegionEnsembles(ctx, om, blk, cfg, seed=seed)
            after = ctx.std_ensemble_counters()
            n_env = over = 0
            for r, w in enumerate(regions):
                h, d = host[r], dev[r]
                assert d["status"] == h["status"], (name, r)
                assert np.array_equal(d["trace_status"], h["trace_status"]), (name, r)
                assert np.array_equal(d["segments"], h["segments"]), (name, r)
                assert d["envelopes"] == h["envelopes"], (name, r)
                assert np.array_equal(d["n2corr"].view(np.uint32), h["n2corr"].view(np.uint32)), (name, r)
                if len(w) == 0 or (w == 27).all():
                    assert d["status"] == ba.ENS_REGION_NO_TRACES and d["envelopes"] == [] and len(d["segments"]) == 0
                    assert (d["trace_status"] == ba.ENS_IMPOSSIBLE).all()
                    continue
                assert d["status"] == ba.ENS_REGION_OK and not d["trace_status"].any(), (name, r)
                seg = d["segments"]
                assert set(seg[:, 0]) == set(range(200))
                assert (seg[:, 1] >= 1).all() and (seg[:, 2] <= len(w)).all() and (seg[:, 3] >= 1).all() and (seg[:, 4] <= hmm.M).all()
                over += np.bincount(seg[:, 0]).max() > 8
                n_env += len(d["envelopes"])
            print(name, "seed", seed, "envelopes", n_env, "regions with a trace of more than 8 segments", over)
            # <over> is counted from the twin's own segments and the counter must equal it EXACTLY.  That the shapes are what they were built
            # to be is a second, looser statement: the 12-copy regions overflow, nothing else does -- except that a one-node model also matches
            # stray residues (up to 7 segments in a trace on these regions), so for it only the exact statement is made.
            assert over >= n_over and (over == n_over or name == "M1"), name
            assert mid == before                                           # the host mode counts nothing here
            assert after["twin_fallbacks"] - mid["twin_fallbacks"] == over and after["serial_fallbacks"] == mid["serial_fallbacks"]
            assert after["kernel_regions"] - mid["kernel_regions"] == sum(len(w) > 0 for w in regions)      # the '*' region included
            if name in ("M64", "M65", "M129", "PTH2"):
                assert n_env >= 5, name                                    # the planted copies come out as envelopes: 2 + 3
    finally:
        ctx.set_std_ensemble(ba.ENSEMBLE_SERIAL)


# ---- the pipeline

def pipeline_block(hmm, seed=7):
    """300 windows, the random ones of 900 nt: 8 with an ORF that holds two or three copies of a sampled domain a few residues apart (its posterior profile
    is a multi-domain region), 22 with one copy, the rest random.  No frameshifts: under --fs these windows take the standard branch."""
    rng = np.random.default_rng(seed)
    mat = synth.hmm_match_emissions(hmm)
    basic = ba.gencode_basic(hmm.ct)
    rnd_aa = lambda n: rng.integers(0, 20, size=n, dtype=np.uint8)
    wins = []
    for w in range(300):
        if w % 10 == 0:
            copies = (2 + (w % 40 == 0)) if w < 80 else 1
            aa = np.concatenate([rnd_aa(6)] + [np.concatenate([synth.sample_domain(rng, mat), rnd_aa(int(rng.integers(8, 25)))]) for _ in range(copies)])
            wins.append(np.concatenate([rng.integers(0, 4, size=60, dtype=np.uint8), synth.reverse_translate(rng, aa, basic), rng.integers(0, 4, size=60, dtype=np.uint8)]))
        else:
            wins.append(rng.integers(0, 4, size=900, dtype=np.uint8))
    return wins


def E_bits(x):
    return int(np.float32(x).view(np.uint32))


def domain_key(d):
    return (d.window, d.strand, d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm, E_bits(d.envsc), E_bits(d.oasc), E_bits(d.domcorrection), E_bits(d.bitscore),
            d.reported, d.cigar)


def test_pipeline_modes():
    """run_hits and the standard branch of run_frameshift_domains: device and streams give the same domains record for record, no region
    falls back, and the default mode's domains are those of a context whose switch was never touched."""
    path = ol.GOLDEN + "/PTH2.bhmm"
    hmm = ba.HMM(path, 0)
    wins = pipeline_block(hmm)
    fresh = ba.Context(0)                                                    # set_std_ensemble is never called on this one
    ctx = ba.Context(0)
    try:
        res = {}
        for c, mode in ((fresh, None), (ctx, "serial"), (ctx, "streams"), (ctx, "device")):
            if mode:
                c.set_std_ensemble(mode)
            c.set_fs_strict(True)
            om = ba.OProfile(c, ba.Profile(hmm))
            blk = ba.SeqBlock(c, wins)
            _, dm, nclust = ba.Pipeline(c, om, fs_pipe=False, ncbi_table=hmm.ct).run_hits(blk)
            walked_plain = c.std_ensemble_counters()["kernel_regions"]
            om3 = ba.FSOProfile(c, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
            om5 = ba.FSOProfile(c, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
            _, _, fdm, _ = ba.Pipeline(c, om, fs_pipe=True, ncbi_table=hmm.ct).run_frameshift_domains(om3, om5, blk)
            res[mode] = ([domain_key(d) for d in dm], nclust, [domain_key(d) for d in fdm])
        cnt = ctx.std_ensemble_counters()
        print("clustered regions", res["device"][1], "domains", len(res["device"][0]), "under --fs", len(res["device"][2]), cnt)
        assert res["device"][1] >= 4 and res["device"][1] == res["streams"][1] == res["serial"][1]
        assert res["device"][0] == res["streams"][0] and len(res["device"][0]) >= 20
        assert res["device"][2] == res["streams"][2] and len(res["device"][2]) >= 20
        assert cnt["serial_fallbacks"] == 0 and cnt["twin_fallbacks"] == 0
        # every clustered region of the plain search went through the kernel, and under --fs the standard branch sent it regions too
        assert walked_plain == res["device"][1] and cnt["kernel_regions"] > walked_plain
        assert res["serial"][0] == res[None][0] and res["serial"][2] == res[None][2]
        # the stream modes against the serial mode: as many domains per window
        per_win = lambda keys: np.bincount([k[0] for k in keys], minlength=len(wins))
        assert (per_win(res["device"][0]) == per_win(res["serial"][0])).all()
    finally:
        ctx.close(); fresh.close()


# ---- the command line

IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")      # timing lines; the tail echoes the command line


def strip(text):
    return [ln for ln in text.split("\n") if not ln.startswith(IGNORED)]


def test_cli_device_equals_streams(tmp_path, monkeypatch):
    """--ensemble-std device and streams write the same main output and --tblout (but for the timing lines and the echo of the command
    line) on a golden target and on targets that do hold multi-domain regions: the gene-bearing windows of the pipeline test as FASTA
    records, PTH2 as the query.  bathsearch.run in this process, so that the counters of the context it made can be read: they show
    that regions went through the kernel in the device run."""
    import io
    from bath_amd import bathsearch
    made = []
    setter = ba.Context.set_std_ensemble

    def keeping(self, mode):
        made.append(self)
        setter(self, mode)
    monkeypatch.setattr(ba.Context, "set_std_ensemble", keeping)
    wins = pipeline_block(ba.HMM(ol.GOLDEN + "/PTH2.bhmm", 0))
    for f in ("PTH2.bhmm", "AMP_N.bhmm", "target-AMP_N.fa"):
        shutil.copy(os.path.join(ol.GOLDEN, f), tmp_path / f)
    with open(tmp_path / "planted.fa", "w") as f:
        for w in range(0, len(wins), 10):
            f.write(">win%d\n%s\n" % (w, "".join("ACGT"[c] for c in wins[w])))
    monkeypatch.chdir(tmp_path)
    outs, walked = {}, {}
    for q, t in (("PTH2.bhmm", "planted.fa"), ("AMP_N.bhmm", "target-AMP_N.fa")):
        for mode in ("streams", "device"):
            del made[:]
            assert bathsearch.run(["--ensemble-std", mode, "-o", "out.txt", "--tblout", "out.tbl", q, t], stdout=io.StringIO()) == 0
            assert len(made) == 1
            c = made[0].std_ensemble_counters()
            assert c["serial_fallbacks"] == 0 and c["twin_fallbacks"] == 0
            walked[mode, q] = c["kernel_regions"]
            outs[mode, q] = (strip((tmp_path / "out.txt").read_text()), strip((tmp_path / "out.tbl").read_text()))
            assert not any("ensemble" in ln for ln in outs[mode, q][0] if ln.startswith("#")), "an extension option prints no header line"
        assert outs["streams", q] == outs["device", q], q
    assert walked["device", "PTH2.bhmm"] >= 4 and walked["streams", "PTH2.bhmm"] == 0      # the planted regions did go through the kernel
    assert sum(not ln.startswith("#") and ln != "" for ln in outs["device", "PTH2.bhmm"][1]) >= 20
    assert len(outs["device", "AMP_N.bhmm"][1]) > 3
