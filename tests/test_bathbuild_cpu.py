"""CPU tier of bathbuild: the single-sequence model's text against the reference's recorded files, the calibration stream and fits
(library sampler and fits around the oracle's scorers, tests/bathbuild_common.py) against the recorded STATS lines, and the tool's
options and input rules with that CPU calibrator in place of the GPU's."""
import io
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import bathbuild_common as bc
from bath_amd import bathbuild as bb

PIN_JSON = os.path.join(ba._ROOT, "profiles", "bathbuild_vs_recorded.json")
MODELS = [("AMP_N", 0), ("three_seqs", 0), ("three_seqs", 1), ("three_seqs", 2)]
# The one field of the recorded files that is not reproduced in its last digit: -ln of AMP_N's composition of P is 3.005615, on the
# boundary between the prints 3.00561 and 3.00562 (bathbuild).  Line 17 of the model with DATE and STATS left out; field 13.
KNIFE_EDGE = {"AMP_N": {(17, 13)}}
SMALL = ["--EmL", "30", "--EmN", "6", "--EvL", "30", "--EvN", "6", "--EfL", "12", "--EfN", "6"]     # a quick CPU calibration for the option tests


def run(argv, **kw):
    out = io.StringIO()
    st = bb.run(argv, stdout=out, calibrator=bc.OracleCalibrator, **kw)
    return st, out.getvalue()


def write(path, text):
    with open(str(path), "w") as fh:
        fh.write(text)
    return str(path)


# ---- 1: the score system and the model text
def test_blosum62_lambda_and_symmetry():
    s = ba.ScoreSystem()
    assert abs(s.lambda_ - 0.3179513) < 5e-8                       # the root the issue measured
    q = s.conditionals()
    assert np.allclose(q.sum(axis=1), 1.0, atol=1e-15)
    rows = [ln.split() for ln in ba.scorematrix_builtin().splitlines() if ln and not ln.startswith("#")]
    cols = rows[0]
    sc = {(r[0], c): int(v) for r in rows[1:] for c, v in zip(cols, r[1:])}
    assert all(sc[a, b] == sc[b, a] for a in cols for b in cols) and sc["W", "W"] == 11 and sc["A", "A"] == 4 and sc["*", "*"] == 1
    assert q.shape == (20, 20) and q.argmax(axis=1)[18] == 18      # W most likely stays W


def uncalibrated_text(fixture, index):
    hmm = bc.fresh_model(fixture, index)
    ba.hmm_set_evparam(hmm, np.zeros(8))                           # calibrated (the STATS block is written), values left out or replaced below
    return ba.hmm_text(hmm, date="-")


def test_model_text_equals_the_recorded_amp_n():
    """Every line except DATE and the five STATS lines, byte for byte; the one knife-edge field to 1e-5."""
    text = uncalibrated_text("AMP_N", 0)
    want = bc.stable_lines(open(bc.golden("AMP_N.bhmm"), "rb").read())
    got = bc.stable_lines(text)
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        gt, wt = g.split(), w.split()
        assert len(gt) == len(wt) and len(g) == len(w), (n, g, w)
        bad = [j for j, (a, b) in enumerate(zip(gt, wt)) if a != b]
        assert all((n, j) in KNIFE_EDGE["AMP_N"] for j in bad), (n, bad, g, w)
        assert all(abs(float(gt[j]) - float(wt[j])) <= 1.0000001e-5 for j in bad)
    assert b"FRAMESHIFT PROB    0.0100\nCODON TABLE  1\n" in text and b"COM   [1] [HMM created from a query sequence]\nNSEQ  1\nEFFN  1.000000\n" in text


def test_model_text_equals_the_recorded_three_seqs():
    """With the recorded DATE and STATS lines put in, the three models are the recorded file: its size and SHA-256, whole and per model
    (every other byte is the library's)."""
    rec = bc.recorded_lines("three_seqs")
    assert len(rec) == 3 and all(len(m) == 6 for m in rec)
    parts = [bc.with_recorded_lines(uncalibrated_text("three_seqs", i), rec[i]) for i in range(3)]
    for i, (part, (size, sha)) in enumerate(zip(parts, bc.THREE_SEQS["models"])):
        assert (len(part), bc.sha256(part)) == (size, sha), i
    whole = b"".join(parts)
    assert bc.first_differing_chunk(whole) is None, "lines %d-%d differ from the recorded file" % bc.first_differing_chunk(whole)
    assert (len(whole), bc.sha256(whole)) == (bc.THREE_SEQS["bytes"], bc.THREE_SEQS["sha256"])
    assert bc.first_differing_chunk(whole.replace(b"\nLENG  245\n", b"\nLENG  246\n")) == (1281, 1344)      # (the locator locates)


def test_summary_rows_equal_the_tutorial():
    """documentation/userguide/tutorial.md, Practice 3."""
    rows = []
    for i, (name, desc, seq) in enumerate(bc.queries("three_seqs")):
        hmm = bc.fresh_model("three_seqs", i)
        rows.append(bb.result_line(i + 1, name, len(seq), hmm.M, 1, ba.hmm_relent(hmm), desc))
    assert rows == ["  1      AT1G01010.1              1   429   429    1     1.00  0.591 \n",
                    "  2      AT1G01020.1              1   245   245    1     1.00  0.552 \n",
                    "  3      AT1G01030.1              1   358   358    1     1.00  0.600 \n"]
    assert bb.result_header() == ("# idx    name                  nseq   len  mlen ctbl eff_nseq re/pos description\n"
                                  "# ------ -------------------- ----- ----- ----- ---- -------- ------ -----------\n")


@pytest.mark.parametrize("fixture,index", MODELS)
def test_lambda_and_maxl_equal_the_recorded(fixture, index):
    hmm = bc.fresh_model(fixture, index)
    rec = bc.recorded_stats(fixture)[index]
    assert "%8.5f" % np.float32(ba.hmm_lambda(hmm)) == " " + rec["MSV"][1]
    if fixture == "AMP_N":
        assert "\nMAXL  %d\n" % hmm.max_length in open(bc.golden("AMP_N.bhmm")).read()
    else:
        assert hmm.max_length == bc.THREE_SEQS["maxl"][index]
    if (fixture, index) == ("three_seqs", 0):
        assert abs(ba.hmm_lambda(hmm) - (np.log(2) + 1.44 / (429 * ba.hmm_relent(hmm)))) < 1e-15 and hmm.max_length == 479


# ---- 2: calibration against the recorded files
@pytest.mark.parametrize("fixture,index", MODELS)
def test_calibration_against_the_recorded_stats(fixture, index):
    """Measured first (tools/bathbuild_pin.py -> profiles/bathbuild_vs_recorded.json): with the generator seeded with 42 for each model
    and the sets drawn in the order MSV, Viterbi, Forward, the MSV mu and the Viterbi mu of all four recorded models equal the
    recorded digits -- the stream is the reference's -- and so does the Forward tau (worst deviation from the 4-decimal record
    3.6e-5); it is held to four times that.  The frameshift taus of the strict (table log-sum) path sit 4.9e-3 .. 7.4e-3 above the
    recorded ones, the offset bathconvert's pin measured for that arithmetic (profiles/bathconvert_vs_recorded.json: 3.8e-3 .. 6.7e-3);
    they are held as that pin holds them, against 4 standard deviations of a tau over reseeded runs, the smallest that file has for
    these fit sizes (N = 200, L = 100)."""
    pin = json.load(open(PIN_JSON))
    m = next(m for m in pin["models"] if (m["fixture"], m["record"]) == (fixture, index))
    hmm, _ = bc.oracle_fixture(fixture, index)
    rec = bc.recorded_stats(fixture)[index]
    ev = hmm.evparam
    for key, tag, j in (("msv", "MSV", 0), ("vit", "VITERBI", 2), ("fwd", "FORWARD", 4), ("fs3", "FS3 FORWARD", 6), ("fs5", "FS5 FORWARD", 7)):
        print("%-12s %s recorded %s here %9.5f" % (hmm.name, key, rec[tag][0], ev[j]))
        assert m[key]["recorded"] == rec[tag][0] and abs(m[key]["cpu_path"] - float(ev[j])) < 1e-9      # the stored measurement is this path's
    assert pin["mus_equal_the_recorded_digits"]
    assert ("%8.4f" % ev[0]).strip() == rec["MSV"][0] and ("%8.4f" % ev[2]).strip() == rec["VITERBI"][0]
    assert pin["margin"] == 4.0 and pin["fwd_tau_bound"] == 4.0 * pin["fwd_tau_max_abs_dev"] <= 2e-4
    assert abs(float(ev[4]) - float(rec["FORWARD"][0])) <= pin["fwd_tau_bound"]
    conv = json.load(open(os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")))
    sd = min(c[k]["reseeded_sd"] for c in conv["models"] for k in ("fs3", "fs5"))
    assert (conv["L"], conv["N"], conv["tailp"]) == (100, 200, 0.04)
    for j, tag in ((6, "FS3 FORWARD"), (7, "FS5 FORWARD")):
        assert abs(float(ev[j]) - float(rec[tag][0])) <= 4.0 * sd
    assert all("%8.5f" % ev[j] == " " + rec["MSV"][1] for j in (1, 3, 5))


def test_calibrated_text_has_the_recorded_stats_block():
    """The writer's STATS block with the CPU path's parameters: the three standard lines are the recorded file's bytes."""
    hmm, _ = bc.oracle_fixture("AMP_N", 0)
    got = ba.hmm_text(hmm, date="Fri May  1 18:25:35 2026").split(b"\n")
    want = open(bc.golden("AMP_N.bhmm"), "rb").read().split(b"\n")
    assert got[:17] == want[:17] and got[19:21] == want[19:21]     # through STATS LOCAL FORWARD; FRAMESHIFT PROB and CODON TABLE
    assert got[17].startswith(b"STATS LOCAL FS3 FORWARD ") and got[17].endswith(b" 0.71189") and len(got[17]) == len(want[17])


def test_sample_order_and_fits():
    """The MSV set is drawn first, then Viterbi's, then Forward's, then the codon sets, from one stream; FitCompleteLoc is Lawless 4.1.5."""
    s0 = ba.rng_state(42)
    a, s1 = ba.calib_sample_amino(s0, 7, 5)
    b, s2 = ba.calib_sample_amino(s1, 3, 4)
    both, s3 = ba.calib_sample_amino(s0, 1, 47)
    assert s3 == s2 and np.array_equal(np.concatenate([a.ravel(), b.ravel()]), both.ravel()) and a.max() < 20
    assert any(s1 == ba.rng_jump(42, n) for n in range(35, 40))    # one step per residue, one more for a roll beyond the frequencies' sum
    x = np.array([1.0, 2.5, -0.3, 4.0])
    assert abs(ba.gumbel_fit_complete_loc(x, 0.7) - (-np.log(np.mean(np.exp(-0.7 * x))) / 0.7)) < 1e-14


# ---- 3: options and input rules
QUERY = ">q1 a small protein\nMKVLAAGIWDERT\nYHPSQNCF\n"


def test_tool_on_a_small_query(tmp_path):
    fa = write(tmp_path / "q.fa", QUERY)
    out = str(tmp_path / "q.bhmm")
    st, text = run(SMALL + [out, fa], date="D")
    assert st == 0
    lines = text.splitlines()
    assert text.startswith(bb.BANNER + "# input file:                       %s\n# output HMM file:                  %s\n# seq length for MSV Gumbel mu fit: 30\n" % (fa, out))
    assert "  1      q1                       1    21    21    1     1.00" in text
    assert [ln for ln in lines if ln.startswith("  1 ")][0].endswith(" a small protein") and lines[-1].startswith("# CPU time:")
    hmm = ba.HMM(out)                                              # the library's reader takes what the writer wrote
    assert (hmm.M, hmm.name, hmm.ct, hmm.consensus[1:4].lower()) == (21, "q1", 1, "mkv") and hmm.evparam[0] != ba.FS_UNSET
    assert hmm.max_length == ba.hmm_max_length(hmm, 1e-7)


def test_popen_pextend_mxfile(tmp_path):
    fa = write(tmp_path / "q.fa", QUERY)
    a, b, c = (str(tmp_path / n) for n in ("a.bhmm", "b.bhmm", "c.bhmm"))
    assert run(SMALL + [a, fa], date="D")[0] == 0
    st, text = run(SMALL + ["--popen", "0.05", "--pextend", "0.25", b, fa], date="D")
    assert st == 0 and "# gap open probability:             0.050000\n# gap extend probability:           0.250000\n" in text
    tl = open(b).read().splitlines()
    t = [ln.split() for ln in tl if len(ln.split()) == 7 and ln.startswith("          ") and "m->m" not in ln]
    want = ["%.5f" % -np.log(np.float32(v)) for v in (1 - 2 * 0.05, 0.05, 0.05, 0.75, 0.25, 0.75, 0.25)]
    assert t[0] == want and t[-1] == ["%.5f" % -np.log(np.float32(0.95)), want[1], "*", want[3], want[4], "0.00000", "*"]
    # a file holding BLOSUM62, its columns and rows in another order and with comments: the built-in's bytes
    rows = [ln.split() for ln in ba.scorematrix_builtin().splitlines() if ln and not ln.startswith("#")]
    cols, order = rows[0], list(range(len(rows[0])))[::-1]
    by = {r[0]: r[1:] for r in rows[1:]}
    mx = "# BLOSUM62, reversed\n\n   " + "  ".join(cols[j] for j in order) + "\n" + "".join(
        "%s %s # row\n" % (cols[i], " ".join(by[cols[i]][j] for j in order)) for i in order)
    st, text = run(SMALL + ["--mxfile", write(tmp_path / "b62.mat", mx), c, fa], date="D")
    assert st == 0 and "# subst score matrix (file): " in text
    assert open(c, "rb").read() == open(a, "rb").read()


def test_seed(tmp_path):
    two = QUERY + QUERY.replace(">q1", ">q2")
    fa = write(tmp_path / "two.fa", two)
    a, b, z = (str(tmp_path / n) for n in ("a.bhmm", "b.bhmm", "z.bhmm"))
    assert run(SMALL + ["--seed", "42", a, fa], date="D")[0] == 0 and run(SMALL + ["--seed", "42", b, fa], date="D")[0] == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    first, second = open(a).read().split("//\n")[:2]
    assert first.replace("q1", "q2") == second                     # reseeded per model: identical records give identical models
    st, text = run(SMALL + ["--seed", "0", z, fa], date="D")
    assert st == 0 and "# random number seed:               one-time arbitrary\n" in text
    first, second = (m.replace("NAME  q2", "NAME  q1").splitlines() for m in open(z).read().split("//\n")[:2])
    diff = [(x, y) for x, y in zip(first, second) if x != y]
    assert diff and all(x.startswith("STATS LOCAL") for x, _ in diff) and len(first) == len(second)


def test_n_w_length_ct_and_o(tmp_path):
    fa = write(tmp_path / "q.fa", QUERY)
    out, log = str(tmp_path / "n.bhmm"), str(tmp_path / "log.txt")
    st, text = run(SMALL + ["-n", "renamed", "--w_length", "77", "--ct", "4", "-o", log, out, fa], date="D")
    assert st == 0 and text == ""
    model, summary = open(out).read(), open(log).read()
    assert "NAME  renamed\n" in model and "\nMAXL  77\n" in model and "\nCODON TABLE  4\n" in model
    assert "# name (the single) HMM:            renamed\n# output directed to file:          %s\n" % log in summary
    assert "# window length :                   77\n" in summary and "  1      renamed " in summary
    st, text = run(SMALL + ["--w_beta", "1e-3", out, fa], date="D")
    assert st == 0 and "# window length tail mass:          0.001 bits\n" in text
    assert "\nMAXL  %d\n" % ba.hmm_max_length(ba.HMM(out), 1e-3) in open(out).read()


REFUSED = [
    (["-n", "x"], QUERY + QUERY.replace(">q1", ">q2"), "-n"),
    ([], "# STOCKHOLM 1.0\nq1 MKV\n//\n", "Stockholm"),
    ([], ">a\nMKV-LA\n>b\nMKVALA\n", "gap characters"),
    ([], ">a\nACGTACGTTTGACCAGT\n", "nucleotide"),
    ([], "", "empty"),
    ([], ">a\nMKVXLA\n", "X"),
    ([], ">a\nMKBLZA\n", "B, Z"),
    (["--mx", "PAM30"], QUERY, "PAM30"),
    (["--cpu", "4"], QUERY, "--cpu"),
    (["--hand"], QUERY, "--hand"),
    (["--eset", "3"], QUERY, "--eset"),
    (["-O", "x.sto"], QUERY, "-O"),
    (["--popen", "0.6"], QUERY, "--popen"),
    (["--arith", "fast"], QUERY, "--arith"),
    (["--bogus"], QUERY, "--bogus"),
]


@pytest.mark.parametrize("argv,content,names", REFUSED)
def test_refusals_name_what_they_refuse(tmp_path, capsys, argv, content, names):
    fa = write(tmp_path / "in.fa", content)
    out = str(tmp_path / "out.bhmm")
    st, text = run(argv + [out, fa])
    err = capsys.readouterr().err
    assert st == 1 and names in err and err.startswith("Error: "), err
    assert text == "" and not os.path.exists(out)


def test_a_matrix_without_a_root_is_refused(tmp_path, capsys):
    rows = [ln.split() for ln in ba.scorematrix_builtin().splitlines() if ln and not ln.startswith("#")]
    mx = "   " + "  ".join(rows[0]) + "\n" + "".join("%s %s\n" % (r[0], " ".join("-1" for _ in r[1:])) for r in rows[1:])
    path = write(tmp_path / "neg.mat", mx)
    st, _ = run([str(tmp_path / "o.bhmm"), write(tmp_path / "q.fa", QUERY), "--mxfile", path])
    err = capsys.readouterr().err
    assert st == 1 and "input score matrix %s has no valid solution for lambda" % path in err
    st, _ = run(["--mxfile", write(tmp_path / "bad.mat", "A C\nA 1\n"), str(tmp_path / "o.bhmm"), str(tmp_path / "q.fa")])
    assert st == 1 and "error parsing score matrix file" in capsys.readouterr().err


def test_a_name_the_model_cannot_hold_is_refused(tmp_path, capsys):
    fa = write(tmp_path / "long.fa", ">" + "n" * 128 + " d\nMKVLA\n")
    st, _ = run(SMALL + [str(tmp_path / "o.bhmm"), fa])
    assert st == 1 and "127 bytes" in capsys.readouterr().err and os.listdir(str(tmp_path)) == ["long.fa"]
    ok = write(tmp_path / "ok.fa", ">" + "n" * 127 + "\nMKVLA\n")
    assert run(SMALL + [str(tmp_path / "o.bhmm"), ok])[0] == 0 and ("NAME  " + "n" * 127 + "\n") in open(str(tmp_path / "o.bhmm")).read()


def test_non_residues_are_stripped():
    """p7_SingleBuilder:513-524: '*' is dropped before the model is made."""
    assert np.array_equal(ba.strip_query("MK*V"), ba.strip_query("MKV")) and len(ba.strip_query("MK*V")) == 3
    with pytest.raises(ba.BathError, match="U"):
        ba.strip_query("MKUV")


def test_bathsearch_still_refuses_a_sequence_query(capsys):
    from bath_amd import bathsearch as bs
    assert bs.run([bc.golden("AMP_N.fa"), bc.golden("target-AMP_N.fa")], stdout=io.StringIO()) != 0
