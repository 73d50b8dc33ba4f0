"""The bathsearch driver end to end on the GPU: `python -m bath_amd.bathsearch` in a fresh child process, in a directory holding
copies of the recorded inputs, with the recorded command lines.  Its main output and --tblout equal tests/golden byte for byte
except the timing lines, and the tail's option, directory and date lines.  A multi-target synthetic genome searched with several
blocks, chunk sizes and device budgets gives one output, the output of the same search assembled from the library's pieces."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import dist

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")

RUNS = [  # command line, files compared, query is a sequence (compare from 'Query:' on)
    (["-o", "PTH2.out", "--tblout", "PTH2.tbl", "--cigar", "PTH2.bhmm", "target-PTH2.fa"], [("PTH2.out", "PTH2.out"), ("PTH2.tbl", "PTH2.tbl")], False),
    (["--fs", "-o", "AMP_N-fs.out", "--tblout", "AMP_N-fs.tbl", "--cigar", "AMP_N.bhmm", "target-AMP_N.fa"],
     [("AMP_N-fs.out", "AMP_N-fs.out"), ("AMP_N-fs.tbl", "AMP_N-fs.tbl")], False),
    (["--fs", "--frameline", "-o", "AMP_N-frameline.out", "AMP_N.bhmm", "target-AMP_N.fa"], [("AMP_N-frameline.out", "AMP_N-frameline.out")], False),
    (["--ct", "4", "-o", "MET-ct4.out", "MET-ct4.bhmm", "target-MET.fa"], [("MET-ct4.out", "MET-ct4.out")], False),
    (["-o", "AMP_N.out", "AMP_N.bhmm", "target-AMP_N.fa"], [("AMP_N.out", "AMP_N.out")], True),
]


def run_cli(cwd, argv, timeout=600, **kw):
    """The driver in a child process; keyword arguments go to bathsearch.run (block budget, chunk size, device budget)."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    code = "import sys; from bath_amd import bathsearch as b; sys.exit(b.run(sys.argv[1:], **%r))" % (kw,)
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-c", code] + argv, cwd=str(cwd), env=env,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def strip(text):
    return [ln for ln in text.split("\n") if not ln.startswith(IGNORED)]


def golden_dir(tmp_path):
    for f in os.listdir(ol.GOLDEN):
        shutil.copy(os.path.join(ol.GOLDEN, f), tmp_path / f)
    return tmp_path


@pytest.mark.parametrize("argv,files,from_query", RUNS)
def test_cli_reproduces_recorded_runs(tmp_path, argv, files, from_query):
    d = golden_dir(tmp_path)
    made = [out for out, _ in files]
    for out in made:
        os.remove(d / out) if (d / out).exists() else None
    run_cli(d, argv)
    for out, rec in files:
        got = (d / out).read_text()
        want = open(os.path.join(ol.GOLDEN, rec)).read()
        if from_query:
            got, want = got[got.index("Query:"):], want[want.index("Query:"):]
        got, want = env_free_heads(strip(got)), env_free_heads(strip(want))
        assert got == want, "\n".join(got)


def env_free_heads(lines):
    """AMP_N.out, MET-ct4.out and AMP_N-frameline.out were recorded by a reference build whose annotation head also printed
    env-from / env-to; the reference source (p7_tophits_Domains) prints no env columns, and neither does the library (PTH2.out and
    AMP_N-fs.out, recorded without them, are matched as they are by tests/test_tblout_gpu.py).  So the two column-title lines are
    dropped and each hit line is compared as fields, without the env columns where the title names them."""
    out, i = [], 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith(">> "):
            out.append(ln)
            with_env = "env-from" in lines[i + 1]
            i += 3                                              # skip the two title lines
            toks = lines[i].split()
            if with_env:                                        # env-from, env-to and their bracket token follow ali-to's
                toks = toks[:10] + toks[13:]
            out.append(toks)
        else:
            out.append(ln)
        i += 1
    return out


def synthetic_fasta(path, seed=2024):
    """Several targets, one longer than block_length (several windows with context), 60-column lines."""
    from bath_amd import synth
    hmm = ba.HMM(ol.GOLDEN + "/Caudal_act.bhmm")
    g, _ = synth.genome(900_000, seed=seed, hmms=[hmm], genes_per_model=24, frameshift=True)
    lens = [420_000, 3_000, 180_000, 10, 297_000 - 10]
    recs, p = [], 0
    with open(path, "w") as fh:
        for i, n in enumerate(lens):
            s = "".join("ACGT"[c] for c in g[p:p + n])
            recs.append(("chr%d" % i, g[p:p + n]))
            fh.write(">chr%d synthetic target %d\n" % (i, i))
            for k in range(0, n, 60):
                fh.write(s[k:k + 60] + "\n")
            p += n
    return recs


def assembled(ctx, hmmfile, recs, fs, block_length):
    """The same search from the existing API: split_targets + a host SeqBlock with contexts + TopHits."""
    hmm = ba.HMM(hmmfile)
    wins = dist.split_targets([len(s) for _, s in recs], hmm.max_length, block_length)
    blk = ba.SeqBlock(ctx, [recs[t][1][s:s + n] for t, s, n, c in wins])
    blk.set_context([c for *_, c in wins])
    om = ba.OProfile(ctx, ba.Profile(hmm))
    pipe = ba.Pipeline(ctx, om, fs_pipe=fs, ncbi_table=hmm.ct)
    if fs:
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3)); om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5))
        stats, _, dm, _ = pipe.run_frameshift_domains(om3, om5, blk)
    else:
        stats, dm, _ = pipe.run_hits(blk)
    for d in dm:
        t, s, n, c = wins[d.window]
        d.ienv += s; d.jenv += s; d.iali += s; d.jali += s; d.window = t
    th = ba.TopHits()
    th.add(dm, [nm for nm, _ in recs], [len(s) for _, s in recs], descs=["synthetic target %d" % i for i in range(len(recs))])
    th.finalize(stats.nres, hmm.max_length)
    return th.tblout(hmm.name, hmm.acc, hmm.M, fs_pipe=fs, show_cigar=True), th.targets(fs_pipe=fs, textw=150)


@pytest.mark.parametrize("fs", [False, True])
def test_synthetic_genome_independent_of_blocking(gpu_ctx, tmp_path, fs):
    recs = synthetic_fasta(tmp_path / "genome.fa")
    shutil.copy(ol.GOLDEN + "/Caudal_act.bhmm", tmp_path / "q.bhmm")
    argv = (["--fs"] if fs else []) + ["--block_length", "100000", "-o", "out.txt", "--tblout", "hits.tbl", "--cigar", "q.bhmm", "genome.fa"]
    outs = []
    for kw in ({}, {"block_nt": 150_000, "chunk_bytes": 65_536}, {"block_nt": 400_000, "chunk_bytes": 100_003, "resident_bytes": 300_000}):
        run_cli(tmp_path, argv, **kw)
        outs.append((strip((tmp_path / "out.txt").read_text()), strip((tmp_path / "hits.tbl").read_text())))
    assert outs[0] == outs[1] == outs[2]
    tbl, targets = assembled(gpu_ctx, str(tmp_path / "q.bhmm"), recs, fs, 100_000)
    got_tbl = (tmp_path / "hits.tbl").read_text()
    assert got_tbl[:got_tbl.index("#\n# Program:")] == tbl
    assert targets in (tmp_path / "out.txt").read_text()
    assert tbl.count("\n") >= 2 + 3            # the planted genes are found
