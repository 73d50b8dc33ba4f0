"""GPU tier of bathsearch --qformat fasta: the tutorial's bathsearch --hmmout AMP_N.bhmm -o AMP_N.out AMP_N.fa target-AMP_N.fa against
its recorded output and model file, with and without --hmmout; a three-record query against a target built here, where the one
command must write what bathbuild followed by bathsearch writes, with --fs and plain, with --workers 2 and over two ranks; and the
taus of --arith odds.  The driver runs in child processes, as tests/test_bathsearch_gpu.py runs it."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import bathbuild_common as bc
from bath_amd import bathbuild as bb
from bath_amd import synth
from test_bathsearch_gpu import env_free_heads, strip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QFMT_LINE = "# query format asserted:                         fasta\n"
QUERY_LINES = ("# query HMM file:", "# hmm output:", "# query format asserted:", "# Query file:")     # what names the query differs by design
TUTORIAL = ["--qformat", "fasta", "--hmmout", "AMP_N.bhmm", "-o", "AMP_N.out", "AMP_N.fa", "target-AMP_N.fa"]


def cli(cwd, argv, timeout=300, **env):
    """The driver in a child process under a time limit; the temporary files of the run go to <cwd>/tmp."""
    os.makedirs(os.path.join(str(cwd), "tmp"), exist_ok=True)
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(PYTHONPATH=ROOT, TMPDIR=os.path.join(str(cwd), "tmp"), **env)
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "bath_amd.bathsearch"] + argv, cwd=str(cwd), env=e,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return p


def work_dir(base, name, files):
    d = base / name
    d.mkdir()
    for f in files:
        shutil.copy(f, d / os.path.basename(f))
    return d


def from_query(text):
    return env_free_heads(strip(text[text.index("Query:"):]))


def recorded(name):
    return open(bc.golden(name)).read()


def model_lines(path):
    """A model file's lines, DATE aside."""
    return [ln for ln in open(path, "rb").read().split(b"\n") if not ln.startswith(b"DATE ")]


def test_the_tutorial_command(tmp_path):
    """M = 134 against 411 nt: AMP_N.out from Query: on, its header plus the one line, and the model file written beside it."""
    d = work_dir(tmp_path, "run", [bc.golden("AMP_N.fa"), bc.golden("target-AMP_N.fa")])
    cli(d, TUTORIAL)
    got, want = (d / "AMP_N.out").read_text(), recorded("AMP_N.out")
    assert from_query(got) == from_query(want), got
    head = want[:want.index("Query:")]
    at = head.index("# - - -", head.index("# query HMM file:"))
    assert got[:got.index("Query:")] == head[:at] + QFMT_LINE + head[at:]
    built, rec = open(d / "AMP_N.bhmm", "rb").read(), open(bc.golden("AMP_N.bhmm"), "rb").read()
    assert bc.stable_lines(built)[:17] == bc.stable_lines(rec)[:17] and len(built) == len(rec)      # as tests/test_bathbuild_gpu.py holds a built file
    assert built.count(b"STATS LOCAL") == 5 and ba.HMM(str(d / "AMP_N.bhmm")).M == 134
    assert sorted(os.listdir(d)) == ["AMP_N.bhmm", "AMP_N.fa", "AMP_N.out", "target-AMP_N.fa", "tmp"] and os.listdir(d / "tmp") == []


def test_the_tutorial_command_without_hmmout(tmp_path):
    """The models go to a temporary file: the same text from Query: on, and no file left behind."""
    d = work_dir(tmp_path, "run", [bc.golden("AMP_N.fa"), bc.golden("target-AMP_N.fa")])
    cli(d, ["--qformat", "fasta", "-o", "AMP_N.out", "AMP_N.fa", "target-AMP_N.fa"])
    got = (d / "AMP_N.out").read_text()
    assert from_query(got) == from_query(recorded("AMP_N.out")), got
    assert "# hmm output:" not in got and QFMT_LINE in got
    assert sorted(os.listdir(d)) == ["AMP_N.fa", "AMP_N.out", "target-AMP_N.fa", "tmp"] and os.listdir(d / "tmp") == []


# ---- a three-record query (429, 245 and 358 nodes) and a target with its genes, one of them with a frameshift -------------------

FS_FILES = ["o.out", "t.tbl", "f.tbl"]
FS_ARGV = ["--qformat", "fasta", "--fs", "--tblout", "t.tbl", "--fstblout", "f.tbl", "--hmmout", "h.bhmm", "-o", "o.out", "three_seqs.fa", "target.fa"]
DELETED = 1                                  # the record whose gene loses one nucleotide


def write_target(path, seed=31):
    """Every query reverse-translated with seeded codon choices, the second without one nucleotide of its middle, each between
    stretches of seeded random DNA: about 5 kb in one record."""
    rng = np.random.default_rng(seed)
    basic = ba.gencode_basic(1)
    parts = [rng.integers(0, 4, 400).astype(np.uint8)]
    for k, (_, _, seq) in enumerate(bc.queries("three_seqs")):
        nt = synth.reverse_translate(rng, ba.strip_query(seq), basic)
        if k == DELETED:
            nt = np.delete(nt, len(nt) // 2 + 1)
        parts += [nt, rng.integers(0, 4, 400 + 7 * k).astype(np.uint8)]
    s = "".join("ACGT"[c] for c in np.concatenate(parts))
    with open(path, "w") as fh:
        fh.write(">chr planted genes\n" + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)))
    return len(s)


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """The inputs, bathbuild's model file for them, and the one-command --fs run, made once."""
    base = tmp_path_factory.mktemp("three")
    inputs = base / "inputs"
    inputs.mkdir()
    shutil.copy(bc.golden("three_seqs.fa"), inputs / "three_seqs.fa")
    assert 4000 < write_target(inputs / "target.fa") < 8000
    assert bb.run([str(inputs / "bathbuild.bhmm"), str(inputs / "three_seqs.fa")], stdout=io.StringIO()) == 0
    files = [str(inputs / "three_seqs.fa"), str(inputs / "target.fa")]
    d = work_dir(base, "fs", files)
    cli(d, FS_ARGV)
    return dict(base=base, files=files, bathbuild=str(inputs / "bathbuild.bhmm"), fs=d)


def kept(path):
    return [ln for ln in strip(open(path).read()) if not ln.startswith(QUERY_LINES)]


def test_three_records_with_fs(three):
    d = three["fs"]
    assert model_lines(d / "h.bhmm") == model_lines(three["bathbuild"])
    assert [ba.HMM(str(d / "h.bhmm"), k).M for k in range(3)] == [429, 245, 358]
    direct = work_dir(three["base"], "fs_direct", [str(d / "h.bhmm"), three["files"][1]])
    cli(direct, ["--fs", "--tblout", "t.tbl", "--fstblout", "f.tbl", "-o", "o.out", "h.bhmm", "target.fa"])
    for f in FS_FILES:
        assert kept(d / f) == kept(direct / f), f
    out = (d / "o.out").read_text()
    blocks = out.split("\nQuery: ")[1:]
    assert len(blocks) == 3 and all("\n>> chr" in b for b in blocks), out                    # every query reports a hit
    rows = [ln for ln in (d / "f.tbl").read_text().splitlines() if ln and not ln.startswith("#")]
    assert rows and any(bc.queries("three_seqs")[DELETED][0] in ln for ln in rows), rows     # the planted frameshift is in the table
    head = out[:out.index("Query:")]
    assert "# query HMM file:                                three_seqs.fa\n" in head and "# hmm output:                                    h.bhmm\n" in head
    tail = (d / "t.tbl").read_text()
    assert "# Query file:      h.bhmm\n" in tail and "# Query file:      h.bhmm\n" in (d / "f.tbl").read_text()
    assert os.listdir(d / "tmp") == []


def test_three_records_plain(three):
    """Without --fs and --hmmout the models are calibrated without the taus: the search of bathbuild's file, which has them, from
    Query: on."""
    d = work_dir(three["base"], "plain", three["files"])
    cli(d, ["--qformat", "fasta", "-o", "o.out", "--tblout", "t.tbl", "three_seqs.fa", "target.fa"])
    direct = work_dir(three["base"], "plain_direct", [three["bathbuild"], three["files"][1]])
    cli(direct, ["-o", "o.out", "--tblout", "t.tbl", "bathbuild.bhmm", "target.fa"])
    got, want = (d / "o.out").read_text(), (direct / "o.out").read_text()
    assert strip(got[got.index("Query:"):]) == strip(want[want.index("Query:"):]) and got.count("\n>> chr") >= 3
    assert kept(d / "t.tbl") == kept(direct / "t.tbl") and "# Query file:      three_seqs.fa\n" in (d / "t.tbl").read_text()
    assert sorted(os.listdir(d)) == ["o.out", "t.tbl", "target.fa", "three_seqs.fa", "tmp"] and os.listdir(d / "tmp") == []


@pytest.mark.parametrize("mode", ["workers", "gpus"])
def test_run_modes_write_the_bytes_of_the_single_run(three, mode):
    d = work_dir(three["base"], mode, three["files"])
    if mode == "workers":
        cli(d, ["--workers", "2"] + FS_ARGV)
    else:
        cli(d, ["--gpus", "2"] + FS_ARGV, BATH_SEARCH_SHARE_DEVICE="1", BATH_SEARCH_BACKEND="gloo")
    for f in FS_FILES:
        assert strip((d / f).read_text()) == strip((three["fs"] / f).read_text()), f
    assert model_lines(d / "h.bhmm") == model_lines(three["fs"] / "h.bhmm") and os.listdir(d / "tmp") == []


def test_arith_odds_builds_bathbuilds_odds_taus(tmp_path):
    d = work_dir(tmp_path, "run", [bc.golden("AMP_N.fa"), bc.golden("target-AMP_N.fa")])
    cli(d, ["--qformat", "fasta", "--arith", "odds", "--fs", "--hmmout", "odds.bhmm", "-o", "o.out", "AMP_N.fa", "target-AMP_N.fa"])
    assert bb.run(["--arith", "odds", str(d / "bathbuild.bhmm"), str(d / "AMP_N.fa")], stdout=io.StringIO()) == 0
    got, want = ba.HMM(str(d / "odds.bhmm")), ba.HMM(str(d / "bathbuild.bhmm"))
    assert np.array_equal(got.evparam.view(np.uint32), want.evparam.view(np.uint32)) and model_lines(d / "odds.bhmm") == model_lines(d / "bathbuild.bhmm")
    strict = bc.fresh_model("AMP_N", 0)
    ctx = ba.Context(0)
    try:
        ba.calibrate(ctx, strict, 1, ba.rng_state(42))
    finally:
        ctx.close()
    # the arithmetic reached the build: the taus are not the strict ones (a file holds four decimals), the standard fits are
    assert (np.abs(strict.evparam[6:8] - got.evparam[6:8]) > 1e-4).all() and (np.abs(strict.evparam[:6] - got.evparam[:6]) <= 5.1e-5).all()
    assert "\n>> " in (d / "o.out").read_text()
