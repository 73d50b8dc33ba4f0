"""CPU tier of bathsearch --qformat fasta (bath_amd/bathsearch.py): the new options' rules, the refusals of a sequence query that
happen before any GPU work, the header lines against the recorded AMP_N.out, the model text of a calibration without the frameshift
taus (bath_hmm_write_ascii, read back by ba.HMM), and the build loop bathsearch shares with bathbuild, on a calibrator stub."""
import io
import os

import numpy as np
import pytest

import bath_amd as ba
import bathbuild_common as bc
from bath_amd import bathbuild as bb
from bath_amd import bathsearch as bs

TARGET = bc.golden("target-AMP_N.fa")
QFMT_LINE = "# query format asserted:                         fasta\n"
BUILD_ARGS = [["--hmmout", "x.bhmm"], ["--popen", "0.1"], ["--pextend", "0.3"], ["--mx", "BLOSUM62"], ["--mxfile", "m.mat"], ["--w_beta", "1e-5"],
              ["--w_length", "100"]]


@pytest.mark.parametrize("extra", BUILD_ARGS, ids=lambda e: e[0])
def test_build_options_require_qformat(extra):
    with pytest.raises(bs.UsageError, match="option %s requires --qformat" % extra[0]):
        bs.parse_args(extra + ["q.fa", "t.fa"])
    opts, q, t = bs.parse_args(["--qformat", "fasta"] + extra + ["q.fa", "t.fa"])
    assert extra[0] in opts and opts["--qformat"] == "fasta" and (q, t) == ("q.fa", "t.fa")


@pytest.mark.parametrize("fmt", ["stockholm", "afa", "nonsense"])
def test_other_query_formats_are_refused_by_name(fmt):
    with pytest.raises(bs.UsageError, match="--qformat") as e:
        bs.parse_args(["--qformat", fmt, "q.fa", "t.fa"])
    assert fmt in str(e.value) and ("alignment queries are not supported" in str(e.value)) == (fmt != "nonsense")


@pytest.mark.parametrize("argv,word", [
    (["--mx", "BLOSUM62", "--mxfile", "m.mat"], "--mx and --mxfile are incompatible"),
    (["--fsonly"], "--fsonly"),
    (["--hmmout", "q.fa"], "--hmmout"), (["--hmmout", "./t.fa"], "--hmmout"),
    (["--popen", "0.5"], "--popen"), (["--pextend", "1"], "--pextend"), (["--w_beta", "1.5"], "--w_beta"), (["--w_length", "0"], "--w_length")])
def test_option_rules_under_qformat(argv, word):
    with pytest.raises(bs.UsageError, match=word):
        bs.parse_args(["--qformat", "fasta"] + argv + ["q.fa", "t.fa"])


def test_fsonly_is_taken_with_fs_or_hmmout():
    for more in (["--fs"], ["--hmmout", "x.bhmm"]):
        assert "--fsonly" in bs.parse_args(["--qformat", "fasta", "--fsonly"] + more + ["q.fa", "t.fa"])[0]


def no_gpu(monkeypatch):
    monkeypatch.setattr(ba, "Context", lambda *a, **k: pytest.fail("a GPU context was opened"))
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    monkeypatch.setattr(bs, "build_in_child", lambda *a, **k: pytest.fail("a build child was started"))


REFUSED_QUERIES = [(">q1\nMKVLAAGIWD\n>bad one\nMKVXLAAG\n", ["bad", "X"]), (">q1\nMKVLAAGIWD\n>hollow\n>q3\nMKV\n", ["hollow"]),
                   (">dna\nACGTACGTTGCAACGTTGCA\n", ["nucleotide"]), (">" + "n" * 128 + "\nMKVLAAGIWD\n", ["n" * 128, "127"])]


@pytest.mark.parametrize("gpus", [[], ["--gpus", "2"]], ids=["one", "gpus2"])
def test_refused_queries_exit_1_before_any_gpu_work(tmp_path, capsys, monkeypatch, gpus):
    no_gpu(monkeypatch)
    out, kept = tmp_path / "o.txt", tmp_path / "kept.bhmm"
    base = gpus + ["--qformat", "fasta", "-o", str(out), "--hmmout", str(kept)]
    assert bs.run(base + [bc.golden("AMP_N.bhmm"), TARGET]) == 1                   # a model file where a sequence file is asserted
    err = capsys.readouterr().err
    assert "AMP_N.bhmm" in err and "profile HMM file" in err
    for text, words in REFUSED_QUERIES:
        q = tmp_path / "query.fa"
        q.write_text(text)
        assert bs.run(base + [str(q), TARGET]) == 1
        err = capsys.readouterr().err
        assert "query.fa" in err and all(w in err for w in words), err
    assert not out.exists() and not kept.exists() and sorted(os.listdir(tmp_path)) == ["query.fa"]


def test_a_fasta_query_without_qformat_names_the_option(capsys, monkeypatch):
    no_gpu(monkeypatch)
    assert bs.run([bc.golden("AMP_N.fa"), TARGET], stdout=io.StringIO()) == 1
    err = capsys.readouterr().err
    assert "AMP_N.fa" in err and "--qformat fasta" in err


def test_header_of_the_tutorial_command_is_the_recorded_plus_one_line():
    argv = ["--qformat", "fasta", "--hmmout", "AMP_N.bhmm", "-o", "AMP_N.out", "AMP_N.fa", "target-AMP_N.fa"]
    opts, q, t = bs.parse_args(argv)
    text = open(bc.golden("AMP_N.out")).read()
    want = text[:text.index("Query:")]
    at = want.index(bs.RULE)                                      # bathsearch.c:311: behind --seed's line, before -l's
    assert bs.output_header(opts, q, t) == want[:at] + QFMT_LINE + want[at:]


def test_header_lines_in_the_reference_order():
    argv = ["--qformat", "fasta", "--w_length", "300", "--w_beta", "1e-5", "--mxfile", "m.mat", "--pextend", "0.3", "--popen", "0.1", "--hmmout", "h.bhmm",
            "--fstblout", "f.tbl", "--fs", "--notrans", "-E", "0.1", "--seed", "7", "-l", "30", "q.fa", "t.fa"]
    lines = bs.output_header(*bs.parse_args(argv)).split("\n")
    want = ["# frameshift tabular output:                     f.tbl", "# hmm output:                                    h.bhmm",
            "# show translated DNA sequence:                  no",                 # bathsearch.c:277, 285-288
            "# gap open probability:                          0.100000", "# gap extend probability:                        0.300000",
            "# subst score matrix (file):                     m.mat", "# sequence reporting threshold:       E-value <= 0.1",
            "# Use the frameshift aware algorithms", "# random number seed set to:                     7",
            "# query format asserted:                         fasta",              # bathsearch.c:311, 313-314
            "# window length beta value:                      1e-05", "# window length :                                300",
            "# minimum ORF length:                            30"]
    at = lines.index(want[0])
    assert lines[at:at + len(want)] == want
    mx = bs.output_header(*bs.parse_args(["--qformat", "fasta", "--mx", "BLOSUM62", "q.fa", "t.fa"]))
    assert "# subst score matrix (built-in):                 BLOSUM62\n" + QFMT_LINE in mx


def test_tabular_tail_names_the_kept_model_file(tmp_path):
    """bathsearch.c:728: the query file becomes the file the models were written to; without --hmmout it stays the file given."""
    for more, want in ((["--hmmout", str(tmp_path / "kept.bhmm")], str(tmp_path / "kept.bhmm")), ([], "q.fa")):
        argv = ["--qformat", "fasta", "--tblout", str(tmp_path / "t.tbl")] + more + ["q.fa", "t.fa"]
        opts, q, t = bs.parse_args(argv)
        with bs.Output(argv, opts, q, t, io.StringIO()) as out:
            out.finish()
            assert "# query HMM file:                                q.fa\n" in out.header
        tail = open(tmp_path / "t.tbl").read()
        assert "# Query file:      %s\n# Target file:     t.fa\n" % want in tail


SMALL_Q = ">q1 a small protein\nMKVLAAGIWDERT\nYHPSQNCF\n>q2\nMSTNPKPQRKTKRNTNRRPQDVKFPGG\n>q3 third\nWWHHCCMMKK\n"
STD_EV = np.array([-7.5, 0.71, -8.25, 0.71, -3.125, 0.71], np.float32)


def test_model_text_without_the_taus(tmp_path):
    """A model with the standard parameters set and the taus unset is written as the reference writes hmm->fs == FALSE
    (p7_hmmfile.c:620-623): the text with the taus set minus exactly the FS3, FS5 and FRAMESHIFT PROB lines; read back, the taus
    are unset.  The parameters are the bathbuild tests' CPU calibrator's."""
    opts = bb.parse_options(["--EmL", "30", "--EmN", "6", "--EvL", "30", "--EvN", "6", "--EfL", "12", "--EfN", "6", "out", "in"])[0]
    hmm = bb.build_model(bc.score_system(), "q1", "MKVLAAGIWDERTYHPSQNCF", opts)
    bc.OracleCalibrator(opts, None).calibrate(hmm, ba.rng_state(42))
    ev = hmm.evparam.copy()
    assert (ev != np.float32(ba.FS_UNSET)).all()
    full = ba.hmm_text(hmm, date="D").split(b"\n")
    ev[6:8] = ba.FS_UNSET
    ba.hmm_set_evparam(hmm, ev)
    std = ba.hmm_text(hmm, date="D").split(b"\n")
    left_out = [ln for ln in full if ln.startswith((b"STATS LOCAL FS3 FORWARD", b"STATS LOCAL FS5 FORWARD", b"FRAMESHIFT PROB"))]
    assert len(left_out) == 3 and std == [ln for ln in full if ln not in left_out] and len(std) == len(full) - 3
    assert sum(ln.startswith(b"STATS LOCAL") for ln in std) == 3 and b"CODON TABLE  1" in std
    path = tmp_path / "std.bhmm"
    path.write_bytes(b"\n".join(std))
    back = ba.HMM(str(path))
    assert (back.evparam[6:8] == np.float32(ba.FS_UNSET)).all() and back.ct == 1 and back.M == hmm.M
    assert ["%.4f" % v for v in back.evparam[:6]] == ["%.4f" % v for v in ev[:6]]
    ev[6:8] = (-4.5, -5.5)                                         # with its taus set a model is written as before
    ba.hmm_set_evparam(hmm, ev)
    assert len(ba.hmm_text(hmm, date="D").split(b"\n")) == len(full)


class StubCalibrator:
    """Fixed parameters in place of a calibration: what the build loop hands to its calibrator, and in what order."""
    calls = []

    def __init__(self, opts, state):
        self.opts = opts
        StubCalibrator.calls.append(("open", opts["--batch"], opts["--seed"], opts["--arith"], state))

    def calibrate_many(self, hmms, state, fs=True):
        StubCalibrator.calls.append(("many", [h.name for h in hmms], state, fs))
        for k, h in enumerate(hmms):
            ba.hmm_set_evparam(h, np.concatenate([STD_EV + k, [-4.0, -5.0] if fs else [ba.FS_UNSET] * 2]))

    def calibrate(self, hmm, state, fs=True):
        StubCalibrator.calls.append(("one", hmm.name, state, fs))
        ba.hmm_set_evparam(hmm, np.concatenate([STD_EV, [-4.0, -5.0] if fs else [ba.FS_UNSET] * 2]))
        return state + 1

    def close(self):
        StubCalibrator.calls.append(("close",))


@pytest.mark.parametrize("more,fs,batch", [([], False, 16), (["--fs"], True, 16), (["--hmmout", "h.bhmm"], True, 16),
                                           (["--fs", "--arith", "odds"], True, 1)], ids=["plain", "fs", "hmmout", "odds"])
def test_the_build_goes_through_bathbuilds_loop(tmp_path, more, fs, batch):
    """SeqQuery.build: bathbuild.build_models with seed 42 whatever --seed says, batches of 16 in strict arithmetic and model by
    model otherwise, the taus only with --fs or --hmmout; the file holds the records' models in order and appears whole."""
    q = tmp_path / "q.fa"
    q.write_text(SMALL_Q)
    opts, qfile, _ = bs.parse_args(["--qformat", "fasta", "--seed", "7", "--ct", "4", "--w_length", "55"] + more + [str(q), TARGET])
    sq = bs.SeqQuery(opts, qfile)
    assert sq.fs == fs and [r[0] for r in sq.queries] == ["q1", "q2", "q3"]
    StubCalibrator.calls = []
    out = tmp_path / "built.bhmm"
    sq.build(str(out), calibrator=StubCalibrator)
    s42 = ba.rng_state(42)
    arith = "odds" if "--arith" in more else "strict"
    if batch > 1:
        want = [("open", 16, 42, arith, s42), ("many", ["q1", "q2", "q3"], s42, fs), ("close",)]
    else:
        want = [("open", 1, 42, arith, s42)] + [("one", n, s42, fs) for n in ("q1", "q2", "q3")] + [("close",)]
    assert StubCalibrator.calls == want
    assert sorted(os.listdir(tmp_path)) == ["built.bhmm", "q.fa"]
    models = [ba.HMM(str(out), k) for k in range(ba.HMM.count(str(out)))]
    assert [(m.name, m.M, m.ct, m.max_length) for m in models] == [("q1", 21, 4, 55), ("q2", 27, 4, 55), ("q3", 10, 4, 55)]
    assert all((m.evparam[6:8] == np.float32(ba.FS_UNSET)).all() != fs for m in models)
    assert open(out, "rb").read().count(b"STATS LOCAL FS3 FORWARD") == (3 if fs else 0)


def test_a_failed_build_leaves_no_file(tmp_path):
    class Failing(StubCalibrator):
        def calibrate_many(self, hmms, state, fs=True):
            raise ba.BathError("model at position 1 of the batch: no")

    q = tmp_path / "q.fa"
    q.write_text(SMALL_Q)
    opts, qfile, _ = bs.parse_args(["--qformat", "fasta", str(q), TARGET])
    with pytest.raises(ba.BathError, match=r"records 1 to 3 of .*q\.fa, calibrated as one batch: model at position 1"):
        bs.SeqQuery(opts, qfile).build(str(tmp_path / "built.bhmm"), calibrator=Failing)
    assert os.listdir(tmp_path) == ["q.fa"]
