"""CPU tier of the bathsearch driver (bath_amd/bathsearch.py): option parsing, refusals, and the parts of its output that need no
search -- the banner with its option lines and the --tblout tail -- against the recorded runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from bath_amd import bathsearch as bs

RECORDED = [  # main output, its command line (as recorded in the files' headers and the --tblout tail)
    ("PTH2.out", ["-o", "PTH2.out", "--tblout", "PTH2.tbl", "--cigar", "PTH2.bhmm", "target-PTH2.fa"]),
    ("AMP_N-fs.out", ["--fs", "-o", "AMP_N-fs.out", "--tblout", "AMP_N-fs.tbl", "--cigar", "AMP_N.bhmm", "target-AMP_N.fa"]),
    ("AMP_N-frameline.out", ["--fs", "--frameline", "-o", "AMP_N-frameline.out", "AMP_N.bhmm", "target-AMP_N.fa"]),
    ("MET-ct4.out", ["--ct", "4", "-o", "MET-ct4.out", "MET-ct4.bhmm", "target-MET.fa"]),
]


def recorded_header(outfile):
    text = open(os.path.join(ol.GOLDEN, outfile)).read()
    return text[:text.index("Query:")]


def test_parse_recorded_command_lines():
    opts, h, s = bs.parse_args(RECORDED[0][1])
    assert (h, s) == ("PTH2.bhmm", "target-PTH2.fa")
    assert opts == {"-o": "PTH2.out", "--tblout": "PTH2.tbl", "--cigar": True}
    opts, h, s = bs.parse_args(RECORDED[3][1])
    assert opts == {"--ct": 4, "-o": "MET-ct4.out"}
    opts, _, _ = bs.parse_args(["-E", "1e-3", "--F1=0.5", "--strand", "minus", "-l", "30", "--seed", "7", "-Z", "12.5",
                                "--block_length", "60000", "-m", "--nonull2", "x.bhmm", "y.fa"])
    assert opts == {"-E": 1e-3, "--F1": 0.5, "--strand": "minus", "-l": 30, "--seed": 7, "-Z": 12.5, "--block_length": 60000,
                    "-m": True, "--nonull2": True}


@pytest.mark.parametrize("outfile,argv", RECORDED)
def test_banner_equals_recorded(outfile, argv):
    opts, h, s = bs.parse_args(argv)
    assert bs.output_header(opts, h, s) == recorded_header(outfile)


@pytest.mark.parametrize("tblfile,argv", [("PTH2.tbl", RECORDED[0][1]), ("AMP_N-fs.tbl", RECORDED[1][1])])
def test_tblout_tail_equals_recorded(tblfile, argv):
    text = open(os.path.join(ol.GOLDEN, tblfile)).read()
    want = text[text.index("#\n# Program:"):]
    opts, h, s = bs.parse_args(argv)
    got = bs.tabular_tail(h, s, argv)
    skip = ("# Option settings:", "# Current dir:", "# Date:")
    keep = lambda t: [ln for ln in t.split("\n") if not ln.startswith(skip)]
    assert keep(got) == keep(want)
    assert [ln.split(":")[0] for ln in got.split("\n")] == [ln.split(":")[0] for ln in want.split("\n")]


REFUSED_CASES = [["--splice"], ["--noali"], ["--acc"], ["--cpu", "4"], ["--incE", "0.1"], ["--tformat", "fasta"], ["--exontblout", "x"],
                 ["--w_length", "100"], ["--notanoption"], ["--frameline"], ["--cigar"], ["-m", "-M"], ["--max", "--F1", "0.1"],
                 ["--textw", "100"], ["--strand", "sideways"], ["--block_length", "1000"]]


@pytest.mark.parametrize("extra", REFUSED_CASES)
def test_refused_options_exit_1_naming_them(extra, capsys):
    argv = extra + [os.path.join(ol.GOLDEN, "PTH2.bhmm"), os.path.join(ol.GOLDEN, "target-PTH2.fa")]
    assert bs.run(argv) == 1
    err = capsys.readouterr().err
    assert extra[0] in err or extra[-2 if len(extra) > 1 else 0] in err, err


def test_refusal_from_the_command_line(tmp_path):
    """A child process: the exit status and the message as a user sees them (no GPU is touched before the refusal)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    p = subprocess.run([sys.executable, "-m", "bath_amd.bathsearch", "--hmmout", "x.hmm", os.path.join(ol.GOLDEN, "PTH2.bhmm"),
                        os.path.join(ol.GOLDEN, "target-PTH2.fa")], capture_output=True, text=True, env=env, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 1 and "--hmmout" in p.stderr and p.stdout == ""


def test_refused_inputs(tmp_path, capsys):
    hmm = os.path.join(ol.GOLDEN, "PTH2.bhmm")
    # a sequence query (the recorded AMP_N.out was made from one)
    q = tmp_path / "q.fa"
    q.write_text(">q\nMKVLAAGIVG\n")
    assert bs.run([str(q), os.path.join(ol.GOLDEN, "target-PTH2.fa")]) == 1
    assert "q.fa" in capsys.readouterr().err
    # compressed and non-FASTA targets
    gz = tmp_path / "t.fa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    assert bs.run([hmm, str(gz)]) == 1
    assert "compressed" in capsys.readouterr().err
    gb = tmp_path / "t.gb"
    gb.write_text("LOCUS       X 10 bp\nORIGIN\n        1 acgtacgtac\n//\n")
    assert bs.run([hmm, str(gb)]) == 1
    assert "FASTA" in capsys.readouterr().err


def test_complement_table_equals_oracle():
    want = np.array([ol.lib().bo_dna_complement(i) for i in range(18)], dtype=np.uint8)
    assert np.array_equal(bs.COMPLEMENT, want)
    codes = np.arange(18, dtype=np.uint8)
    assert np.array_equal(bs.revcomp(bs.revcomp(codes)), codes)


def test_model_descriptions():
    assert bs.model_descriptions(os.path.join(ol.GOLDEN, "MET-ct4.bhmm")) == ["Cystathionine beta-lyase", "Methionine--tRNA ligase"]
