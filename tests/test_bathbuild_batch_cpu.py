"""CPU tier of bathbuild --batch N: the option's rules, and run() with the CPU calibrator of tests/bathbuild_common.py -- driven
through the calibrate fallback loop and through a wrapper that offers calibrate_many -- against --batch 1, byte for byte."""
import io
import os

import pytest

import bath_amd as ba
import bathbuild_common as bc
from bath_amd import bathbuild as bb

SMALL = ["--EmL", "30", "--EmN", "6", "--EvL", "30", "--EvN", "6", "--EfL", "12", "--EfN", "6"]     # a CPU calibration of about a second
# five records of 20 to 40 residues: batches of 2, 2 and 1 at --batch 2
RECORDS = [("q1", "first one", "MKVLAAGIVGLLLAQWERTY"), ("q2", "", "ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMN"), ("q3", "third", "MSTNPKPQRKTKRNTNRRPQDVKFPGG"),
           ("q4", "", "GSHMLEDPVDAFKLNWSTRQYCIHGEAMKVLAAGIVGLLL"), ("q5", "last", "WYVTSRQPNMLKIHGFEDCAWYV")]


def write_fasta(path):
    with open(path, "w") as fh:
        for name, desc, seq in RECORDS:
            fh.write(">%s %s\n%s\n" % (name, desc, seq))
    return str(path)


class ManyCalibrator(bc.OracleCalibrator):
    """The CPU calibrator with calibrate_many; .batches records the sizes run() hands it."""
    batches = None

    def calibrate_many(self, hmms, state):
        type(self).batches.append(len(hmms))
        after = state
        for hmm in hmms:
            after = self.calibrate(hmm, state)
        return after


class LoopCalibrator(bc.OracleCalibrator):
    """Without calibrate_many: run() drives a batch through calibrate; .calls records the models it sees."""
    calls = None

    def calibrate(self, hmm, state):
        type(self).calls.append(hmm.name)
        return super().calibrate(hmm, state)


class FailingCalibrator(ManyCalibrator):
    """Its second batch fails as the library's does."""

    def calibrate_many(self, hmms, state):
        if len(type(self).batches) == 1:
            type(self).batches.append(len(hmms))
            raise ba.BathError("calibrate_batch: model at position 1 of the batch: the Gumbel fit did not converge")
        return super().calibrate_many(hmms, state)


def run(argv, calibrator):
    out = io.StringIO()
    st = bb.run(argv, stdout=out, date="D", calibrator=calibrator)
    return st, out.getvalue()


def without_timing(text, *paths):
    """stdout without its CPU-time line and without the lines that name the output file."""
    return [ln for ln in text.splitlines() if not ln.startswith("# CPU time:") and not any(p in ln for p in paths)]


@pytest.mark.parametrize("value", ["1", "2", "64"])
def test_batch_values_are_accepted(value):
    opts, used, _, _ = bb.parse_options(["--batch", value, "out", "in"])
    assert opts["--batch"] == int(value) and "--batch" in used
    assert bb.parse_options(["out", "in"])[0]["--batch"] == 1


@pytest.mark.parametrize("value", ["0", "65", "many"])
def test_batch_values_out_of_range_are_refused_by_name(value):
    with pytest.raises(bb.UsageError, match="--batch"):
        bb.parse_options(["--batch", value, "out", "in"])


def test_batch_needs_a_seed_and_the_strict_arithmetic():
    with pytest.raises(bb.UsageError, match=r"--batch 2 with --seed 0"):
        bb.parse_options(["--batch", "2", "--seed", "0", "out", "in"])
    with pytest.raises(bb.UsageError, match=r"--batch 2 with --arith odds"):
        bb.parse_options(["--batch", "2", "--arith", "odds", "out", "in"])
    with pytest.raises(bb.UsageError, match=r"--batch 2 with --arith odds3"):
        bb.parse_options(["--arith", "odds3", "--batch", "2", "out", "in"])
    assert bb.parse_options(["--batch", "1", "--seed", "0", "out", "in"])[0]["--seed"] == 0
    assert bb.parse_options(["--batch", "1", "--arith", "odds", "out", "in"])[0]["--arith"] == "odds"


def test_batch_adds_no_header_line():
    a = bb.parse_options(["--seed", "7", "--EmL", "30", "out", "in"])
    b = bb.parse_options(["--batch", "16", "--seed", "7", "--EmL", "30", "out", "in"])
    assert bb.output_header(b[0], b[1], "in", "out") == bb.output_header(a[0], a[1], "in", "out")


def test_batches_write_the_bytes_of_batch_one(tmp_path):
    """--batch 2 over five records runs as batches of 2, 2 and 1, --batch 64 as one batch; the model file and stdout (minus its
    timing line and the lines that name the output file) are those of --batch 1, through calibrate_many and through the fallback loop."""
    fa = write_fasta(tmp_path / "five.fa")
    one = str(tmp_path / "one.bhmm")
    st, text1 = run(SMALL + ["--batch", "1", one, fa], bc.OracleCalibrator)
    assert st == 0
    want, names = open(one, "rb").read(), [r[0] for r in RECORDS]
    assert want.count(b"NAME  ") == len(names) and [ln.split()[1] for ln in text1.splitlines() if ln.startswith("  ")] == names
    plain = str(tmp_path / "plain.bhmm")
    st, text0 = run(SMALL + [plain, fa], bc.OracleCalibrator)                  # --batch 1 is the run without the option
    assert st == 0 and open(plain, "rb").read() == want and without_timing(text0, plain) == without_timing(text1, one)
    for nb, sizes in (("2", [2, 2, 1]), ("64", [5])):
        ManyCalibrator.batches, LoopCalibrator.calls = [], []
        for tag, cal in (("many", ManyCalibrator), ("loop", LoopCalibrator)):
            out = str(tmp_path / ("%s_%s.bhmm" % (tag, nb)))
            st, text = run(SMALL + ["--batch", nb, out, fa], cal)
            assert st == 0 and open(out, "rb").read() == want, (nb, tag)
            assert without_timing(text, out) == without_timing(text1, one), (nb, tag)
        assert ManyCalibrator.batches == sizes and LoopCalibrator.calls == names
    assert sorted(os.listdir(str(tmp_path))) == sorted(["five.fa", "one.bhmm", "plain.bhmm", "many_2.bhmm", "loop_2.bhmm", "many_64.bhmm", "loop_64.bhmm"])


def test_a_failing_batch_leaves_nothing_behind(tmp_path, capsys):
    fa = write_fasta(tmp_path / "five.fa")
    out = str(tmp_path / "o.bhmm")
    FailingCalibrator.batches = []
    st, text = run(SMALL + ["--batch", "2", out, fa], FailingCalibrator)
    err = capsys.readouterr().err
    assert st == 1 and FailingCalibrator.batches == [2, 2]
    assert err.count("Error:") == 1 and len(err.strip().splitlines()) == 1 and "records 3 to 4" in err and "position 1 of the batch" in err
    assert os.listdir(str(tmp_path)) == ["five.fa"]                            # no output file, no temporary file
    rows = [ln.split()[1] for ln in text.splitlines() if ln.startswith("  ")]
    assert rows == ["q1", "q2"] and "# CPU time:" not in text                  # the first batch's result lines, nothing later
