"""GPU tier of `bathsearch --gpus N`: the N-rank search writes the single-GPU search's main output and --tblout byte for byte (but
for the timing lines and the tail's option, directory and date lines).  The ranks share device 0 and their collectives run over gloo
(BATH_SEARCH_SHARE_DEVICE=1, BATH_SEARCH_BACKEND=gloo): every rank computes with the HIP kernels on a one-GPU box.  Every search is
a fresh child process under a time limit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")
DB = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")

RECORDED = [  # command line, files compared
    (["-o", "PTH2.out", "--tblout", "PTH2.tbl", "--cigar", "PTH2.bhmm", "target-PTH2.fa"], ["PTH2.out", "PTH2.tbl"]),
    (["-o", "AMP_N.out", "AMP_N.bhmm", "target-AMP_N.fa"], ["AMP_N.out"]),
    (["--fs", "-o", "AMP_N-fs.out", "--tblout", "AMP_N-fs.tbl", "--cigar", "AMP_N.bhmm", "target-AMP_N.fa"], ["AMP_N-fs.out", "AMP_N-fs.tbl"]),
    (["--fs", "--frameline", "-o", "AMP_N-frameline.out", "AMP_N.bhmm", "target-AMP_N.fa"], ["AMP_N-frameline.out"]),
    (["--ct", "4", "-o", "MET-ct4.out", "MET-ct4.bhmm", "target-MET.fa"], ["MET-ct4.out"]),
]


def cli(cwd, argv, timeout=900, expect=0):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT, BATH_SEARCH_SHARE_DEVICE="1", BATH_SEARCH_BACKEND="gloo")
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "bath_amd.bathsearch"] + argv, cwd=str(cwd), env=env,
                       capture_output=True, text=True)
    assert p.returncode == expect, (p.returncode, p.stderr[-3000:])
    return p


def strip(text):
    return [ln for ln in text.split("\n") if not ln.startswith(IGNORED)]


def outputs(d, files):
    return {f: strip((d / f).read_text()) for f in files}


def fresh_dir(base, name, inputs):
    d = base / name
    d.mkdir()
    for f in inputs:
        shutil.copy(f, d / os.path.basename(f))
    return d


_single = {}


def single_run(tmp_path_factory, key, argv, files, inputs):
    """The single-process search of a command, run once per command."""
    if key not in _single:
        d = fresh_dir(tmp_path_factory.mktemp("single"), "run", inputs)
        cli(d, argv)
        _single[key] = outputs(d, files)
    return _single[key]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("case", range(len(RECORDED)))
def test_recorded_runs_over_n_ranks(tmp_path, tmp_path_factory, case, n):
    argv, files = RECORDED[case]
    inputs = [os.path.join(ol.GOLDEN, f) for f in argv[-2:]]
    want = single_run(tmp_path_factory, case, argv, files, inputs)
    d = fresh_dir(tmp_path, "n%d" % n, inputs)
    cli(d, ["--gpus", str(n)] + argv)
    got = outputs(d, files)
    for f in files:
        assert got[f] == want[f], f
        assert got[f][-2] == "[ok]" or f.endswith(".tbl")


def gene(rng, hmm, basic):
    """A gene sampled from <hmm>'s match emissions, on a random strand."""
    nt = synth.reverse_translate(rng, synth.sample_domain(rng, synth.hmm_match_emissions(hmm)), basic)
    return (3 - nt[::-1]).astype(np.uint8) if rng.random() < 0.5 else nt


def database_fasta(path, seed=77, block_length=50_000):
    """Records of several sizes -- some shorter than one window, some several windows long -- with the 12 models' genes planted at
    random, and for every model one gene ending just before a window boundary of its own: inside the overlap that the next window
    reads again as its context, so two windows find it and the duplicate has to go."""
    hmms = [ba.HMM(DB, q) for q in range(ba.HMM.count(DB))]
    lens = [180_000, 7_000, 120_000, 51_000, 2_500, 99_000, 260_000]
    g, _ = synth.genome(sum(lens), seed=seed, hmms=hmms, genes_per_model=3)
    rng = np.random.default_rng(seed + 1)
    basic = ba.gencode_basic(1)
    starts = np.cumsum([0] + lens)
    boundaries = [(r, k) for r, n in enumerate(lens) for k in range(1, (n - 1) // block_length + 1)]
    assert len(boundaries) >= len(hmms)
    for q, h in enumerate(hmms):
        r, k = boundaries[q]
        nt = gene(rng, h, basic)
        end = int(starts[r]) + k * block_length - 12 - 7 * q
        g[end - len(nt):end] = nt
    with open(path, "w") as fh:
        for i, n in enumerate(lens):
            s = "".join("ACGT"[c] for c in g[starts[i]:starts[i] + n])
            fh.write(">rec%d planted record %d\n" % (i, i))
            for k in range(0, n, 70):
                fh.write(s[k:k + 70] + "\n")


@pytest.fixture(scope="module")
def database_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("db")
    shutil.copy(DB, d / "db.bhmm")
    database_fasta(d / "genome.fa")
    return d


DB_RUNS = {
    "plain": ["--block_length", "50000", "-o", "out.txt", "--tblout", "hits.tbl", "--cigar", "db.bhmm", "genome.fa"],
    "fs": ["--fs", "--block_length", "50000", "-o", "out.txt", "--tblout", "hits.tbl", "--cigar", "db.bhmm", "genome.fa"],
}


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("mode", ["plain", "fs"])
def test_database_over_n_ranks(database_dir, tmp_path, tmp_path_factory, mode, n):
    argv = DB_RUNS[mode]
    inputs = [database_dir / "db.bhmm", database_dir / "genome.fa"]
    want = single_run(tmp_path_factory, "db-" + mode, argv, ["out.txt", "hits.tbl"], inputs)
    assert sum(1 for ln in want["hits.tbl"] if ln and not ln.startswith("#")) >= 12          # the planted genes are found
    assert sum(1 for ln in want["out.txt"] if ln.startswith("Query:")) == 12
    d = fresh_dir(tmp_path, "n%d" % n, inputs)
    cli(d, ["--gpus", str(n)] + argv)
    got = outputs(d, ["out.txt", "hits.tbl"])
    assert got["hits.tbl"] == want["hits.tbl"]
    assert got["out.txt"] == want["out.txt"]


def test_gpus_1_is_the_single_gpu_search(tmp_path):
    argv = ["-o", "PTH2.out", "--tblout", "PTH2.tbl", "--cigar", "PTH2.bhmm", "target-PTH2.fa"]
    inputs = [os.path.join(ol.GOLDEN, f) for f in argv[-2:]]
    a = fresh_dir(tmp_path, "a", inputs)
    b = fresh_dir(tmp_path, "b", inputs)
    cli(a, argv)
    cli(b, ["--gpus", "1"] + argv)
    assert outputs(a, ["PTH2.out", "PTH2.tbl"]) == outputs(b, ["PTH2.out", "PTH2.tbl"])


def test_stdout_output_over_n_ranks(tmp_path):
    inputs = [os.path.join(ol.GOLDEN, f) for f in ("MET-ct4.bhmm", "target-MET.fa")]
    d = fresh_dir(tmp_path, "d", inputs)
    one = cli(d, ["--ct", "4", "MET-ct4.bhmm", "target-MET.fa"]).stdout
    two = cli(d, ["--gpus", "2", "--ct", "4", "MET-ct4.bhmm", "target-MET.fa"]).stdout
    assert strip(two) == strip(one) and one.endswith("[ok]\n")


def test_fasta_error_over_n_ranks(tmp_path):
    """A byte the device parser refuses: status 1, the message (record and line) once, no [ok], no rank left running."""
    d = fresh_dir(tmp_path, "d", [os.path.join(ol.GOLDEN, "PTH2.bhmm")])
    with open(d / "bad.fa", "w") as fh:
        fh.write(">one\n" + "ACGT" * 30 + "\n>two\nACGTACGT\nACGJTACGT\n")
    p = cli(d, ["--gpus", "2", "-o", "out.txt", "--tblout", "t.tbl", "PTH2.bhmm", "bad.fa"], timeout=300, expect=1)
    assert p.stderr.count("Error:") == 1 and "FASTA format error, line 5" in p.stderr and "in record 2" in p.stderr, p.stderr
    assert "[ok]" not in ((d / "out.txt").read_text() if (d / "out.txt").exists() else "")
    assert "[ok]" not in ((d / "t.tbl").read_text() if (d / "t.tbl").exists() else "")
    live = []
    for pid in os.listdir("/proc"):
        try:
            if pid.isdigit() and os.readlink("/proc/%s/cwd" % pid).startswith(str(d)):
                live.append(pid)
        except OSError:
            pass
    assert not live
