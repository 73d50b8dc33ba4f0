"""GPU tier of `bathsearch --fs --fstblout`: the table of frameshift and stop locations, written from the GPU path's traces.

The recorded --fs search of AMP_N gives the recorded alignment's six rows and the tail of --tblout, and leaves the main output and
--tblout as they are without the option.  A synthetic search of two models holds every kind of row on both strands, agrees row by
row with the shifts / stops columns of --tblout and with the nucleotides of the FASTA file, and is the same file with --workers 2
and with --gpus 2 (two ranks sharing device 0, collectives over gloo).  Every search is a fresh child process under a time limit."""
import os
import shutil
import subprocess
import sys
from collections import Counter

import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import synth
from test_fstblout_cpu import recorded_table_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL_IGNORED = ("# Option settings:", "# Current dir:", "# Date:")
IGNORED = ("# CPU time:", "# Mc/sec:") + TAIL_IGNORED
SEED = 17


def cli(cwd, argv, timeout=300, multi=False):
    """bathsearch.run(argv) in a fresh child process."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT
    if multi:
        env.update(BATH_SEARCH_SHARE_DEVICE="1", BATH_SEARCH_BACKEND="gloo")
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "bath_amd.bathsearch"] + argv, cwd=str(cwd), env=env,
                       capture_output=True, text=True)
    if p.returncode in (124, 134, 137, 139):        # a time limit, an abort or a segmentation fault: nothing more is started on this GPU
        pytest.exit("bathsearch %s ended with status %d:\n%s" % (" ".join(argv), p.returncode, p.stderr[-3000:]), returncode=p.returncode)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return p


def keep(text, ignored=IGNORED):
    return [ln for ln in text.split("\n") if not ln.startswith(ignored)]


def data_rows(text):
    return [ln.split() for ln in text.split("\n") if ln and ln[0] != "#"]


def test_recorded_search(tmp_path):
    for f in ("AMP_N.bhmm", "target-AMP_N.fa"):
        shutil.copy(os.path.join(ol.GOLDEN, f), tmp_path / f)
    base = ["--fs", "--tblout", "t.tbl", "-o", "o.txt", "AMP_N.bhmm", "target-AMP_N.fa"]
    cli(tmp_path, base)
    t0, o0 = (tmp_path / "t.tbl").read_text(), (tmp_path / "o.txt").read_text()
    cli(tmp_path, ["--fs", "--fstblout", "f.tbl"] + base[1:])
    f, t, o = ((tmp_path / n).read_text() for n in ("f.tbl", "t.tbl", "o.txt"))
    table = recorded_table_text()
    assert f[:len(table)] == table
    recorded = open(os.path.join(ol.GOLDEN, "AMP_N-fs.tbl")).read()
    want_tail = recorded[recorded.index("#\n# Program:"):]
    got_tail = f[len(table):]
    assert keep(got_tail, TAIL_IGNORED) == keep(want_tail, TAIL_IGNORED)
    assert [ln.split(":")[0] for ln in got_tail.split("\n")] == [ln.split(":")[0] for ln in want_tail.split("\n")]
    assert "--fstblout f.tbl" in got_tail
    # the other two files: the option's header line and nothing else
    line = "# frameshift tabular output:                     f.tbl"
    assert keep(t) == keep(t0)
    assert line in o.split("\n") and [ln for ln in keep(o) if ln != line] == keep(o0)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """Two models against a 60 000 nt target with six frameshifted genes of each planted, searched on one context:
    (directory, command line, --tblout text, --fstblout text)."""
    d = tmp_path_factory.mktemp("fstbl")
    files = [os.path.join(ol.GOLDEN, f) for f in ("AMP_N.bhmm", "PTH2.bhmm")]
    with open(d / "db.bhmm", "wb") as out:
        for f in files:
            out.write(open(f, "rb").read())
    g, _ = synth.genome(60_000, SEED, [ba.HMM(f, 0) for f in files], genes_per_model=6, frameshift=True)
    s = "".join("ACGT"[c] for c in g)
    with open(d / "genome.fa", "w") as fh:
        fh.write(">chrS a synthetic target\n")
        for k in range(0, len(s), 70):
            fh.write(s[k:k + 70] + "\n")
    argv = ["--fs", "-o", "out.txt", "--tblout", "hits.tbl", "--fstblout", "fs.tbl", "db.bhmm", "genome.fa"]
    one = d / "one"
    one.mkdir()
    for f in ("db.bhmm", "genome.fa"):
        shutil.copy(d / f, one / f)
    cli(one, argv)
    return d, argv, (one / "hits.tbl").read_text(), (one / "fs.tbl").read_text()


COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def test_synthetic_search_has_every_row_kind(synthetic):
    """The target is synth.genome(60 000 nt, seed 17, genes_per_model=6, frameshift=True).  The seed was chosen with the oracle's
    --fs pipeline on the CPU (the whole target as one window, the rows from the oracle's traces): it reports 10 hits, 5 of them of
    the frameshift branch, with 17 rows -- 2 'I' of length 1, 10 'D' of length 1, 3 'D' of length 2, 2 'S' (both TAA) -- 15 of
    them on the minus strand, and both queries have hits of the frameshift branch."""
    d, argv, tbl, fstbl = synthetic
    (_, seq), = ol.read_fasta(str(d / "genome.fa"))
    hits = data_rows(tbl)
    rows = data_rows(fstbl)
    assert len(hits) >= 2 and len(rows) >= 4
    by_key = {}
    for r in rows:                                   # target, accession, query, accession, E-value, ali from, ali to, type, length, seq start, ali start
        assert len(r) == 11 and r[7] in "DIS"
        by_key.setdefault((r[0], r[2], r[5], r[6]), []).append(r)
    keys = [(h[1], h[3], h[9], h[10]) for h in hits]
    assert len(set(keys)) == len(keys) and set(by_key) <= set(keys)
    for h, key in zip(hits, keys):
        kinds = Counter(r[7] for r in by_key.get(key, []))
        assert kinds["D"] + kinds["I"] == int(h[15]), (key, kinds, h[15])          # the 'shifts' column
        assert kinds["S"] <= int(h[16]), (key, kinds, h[16])                       # 'stops' counts the insert columns' stops too
        assert all(r[4] == h[11] for r in by_key.get(key, []))                     # --tblout's E-value
    for r in rows:
        typ, length, seq_start, ali_start, ali_from, ali_to = r[7], int(r[8]), int(r[9]), int(r[10]), int(r[5]), int(r[6])
        assert abs(seq_start - ali_from) + 1 == ali_start
        assert (typ, length) in (("D", 1), ("D", 2), ("I", 1), ("I", 2), ("S", 0))
        if typ == "S":
            if ali_from < ali_to:
                codon = seq[seq_start - 1:seq_start + 2]
            else:
                codon = "".join(COMPLEMENT[x] for x in reversed(seq[seq_start - 3:seq_start]))
            assert codon.upper() in ("TAA", "TAG", "TGA"), (r, codon)
    kinds = Counter((r[7], int(r[8])) for r in rows)
    print("rows:", dict(kinds), "minus strand:", sum(int(r[5]) > int(r[6]) for r in rows))
    assert kinds[("I", 1)] + kinds[("I", 2)] >= 1
    assert kinds[("D", 2)] >= 1
    assert kinds[("S", 0)] >= 1
    assert any(int(r[5]) > int(r[6]) for r in rows)
    # the header: once, at the top; the second query adds none
    lines = fstbl.split("\n")
    assert lines[0].startswith("# target name") and lines[1].startswith("#----")
    assert fstbl.count(" target name") == 1 and sum(ln.startswith("#----") for ln in lines) == 1
    queries = [r[2] for r in rows]
    assert set(queries) == {"AMP_N", "PTH2"} and queries == sorted(queries)
    assert lines[2 + len(rows)] == "#" and lines[-2] == "# [ok]"


@pytest.mark.parametrize("mode", [["--workers", "2"], ["--gpus", "2"]], ids=["workers2", "gpus2"])
def test_same_bytes_in_every_mode(synthetic, tmp_path, mode):
    d, argv, tbl, fstbl = synthetic
    for f in ("db.bhmm", "genome.fa"):
        shutil.copy(d / f, tmp_path / f)
    cli(tmp_path, mode + argv, multi=(mode[0] == "--gpus"))
    got = (tmp_path / "fs.tbl").read_text()
    assert keep(got, TAIL_IGNORED) == keep(fstbl, TAIL_IGNORED)
    assert len(data_rows(got)) == len(data_rows(fstbl)) >= 4
    assert keep((tmp_path / "hits.tbl").read_text(), TAIL_IGNORED) == keep(tbl, TAIL_IGNORED)
