"""GPU tier of bathbuild: bath_hip_calibrate against the CPU path of tests/bathbuild_common.py (the library's sampler and fits around
the oracle's scorers), with and without resident sample sets, the smallest model with an interior node, the frameshift taus against
the recorded ones, and the tool end to end into bathsearch."""
import io
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import bathbuild_common as bc
from bath_amd import bathbuild as bb
from bath_amd import bathsearch as bs

pytestmark = pytest.mark.gpu

PIN_JSON = os.path.join(ba._ROOT, "profiles", "bathbuild_vs_recorded.json")
LN2 = bc.LN2
E_NAMES = ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN", "Eft")
# AMP_N (M = 134), three_seqs' 245- and 429-node models at the reference's defaults; one run whose counts differ between the sets and
# are no multiple of a wave
CASES = [("AMP_N", 0, bc.DEFAULT_E), ("three_seqs", 1, bc.DEFAULT_E), ("three_seqs", 0, bc.DEFAULT_E), ("AMP_N", 0, bc.ODD_E)]


def null1(L):
    """p7_bg_SetLength + p7_bg_NullOne."""
    p1 = np.float32(L) / np.float32(L + 1)
    return np.float32(np.float32(L) * np.log(np.float64(p1)) + np.log(1.0 - np.float64(p1)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("fixture,index,E", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_calibrate_equals_the_cpu_path(gpu_ctx, fixture, index, E):
    """The MSV and Viterbi bit scores equal the oracle-scored ones bit for bit, so the mus are equal; the Forward bit scores are within
    the bar tests/test_filters_gpu.py holds the Forward parser to (1e-4 relative, 2e-4 absolute nats); the Forward tau is within four
    times the deviation measured against the CPU path (profiles/bathbuild_vs_recorded.json, gpu: the Forward bit scores differ by up to
    3.4e-6 bits, which moved no tau by a unit of the float the model stores, so the measured deviation is 0; the bound has a floor of
    one unit in the last place of that float, the precision of the format); the frameshift bit scores (after
    the three standard fits have advanced the stream) equal the CPU path's bit for bit and the taus agree to 1e-6; the generator ends
    where the CPU path's does.  Resident sample sets give the same numbers as sets drawn for the call."""
    want, wxv = bc.oracle_fixture(fixture, index, E)
    kw = dict(zip(E_NAMES, E))
    s0 = ba.rng_state(42)
    hmm = bc.fresh_model(fixture, index)
    s1, xv = ba.calibrate(gpu_ctx, hmm, 1, s0, None, want_xv=True, **kw)
    ev, wev = hmm.evparam, want.evparam
    d = np.abs(xv["fwd"] - wxv["fwd"])
    bar = (2e-4 + 1e-4 * np.abs(wxv["fwd"] * LN2 + null1(E[4]))) / LN2
    pin = json.load(open(PIN_JSON))["gpu"]
    print("%s[%d] %r: fwd xv worst dev %.3e bits (bar %.3e), tau gpu %.6f cpu %.6f dev %.3e bound %.3e" %
          (fixture, index, E, d.max(), bar.min(), ev[4], wev[4], abs(float(ev[4]) - float(wev[4])), pin["fwd_tau_bound"]))
    assert same_bits(xv["msv"], wxv["msv"]) and same_bits(xv["vit"], wxv["vit"])
    assert ev[0] == wev[0] and ev[2] == wev[2] and ev[1] == ev[3] == ev[5] == wev[5]
    assert np.all(d <= bar), d.max()
    assert pin["margin"] == 4.0 and pin["fwd_tau_bound"] == 4.0 * pin["fwd_tau_max_abs_dev"]
    floor = float(np.spacing(np.float32(abs(wev[4]))))             # the stored tau is a float: one unit of it (the pin file says so)
    assert pin["fwd_tau_floor"] == "one float32 unit in the last place of the tau"
    assert abs(float(ev[4]) - float(wev[4])) <= max(pin["fwd_tau_bound"], floor)
    assert same_bits(xv["fs3"], wxv["fs3"]) and same_bits(xv["fs5"], wxv["fs5"])
    assert abs(float(ev[6]) - float(wev[6])) <= 1e-6 and abs(float(ev[7]) - float(wev[7])) <= 1e-6
    s = s0
    for L, N in ((E[0], E[1]), (E[2], E[3]), (E[4], E[5])):
        _, s = ba.calib_sample_amino(s, L, N)
    after_std = s
    for _ in range(2):
        _, s = ba.calib_sample(s, E[4], E[5], 1)
    assert s1 == s
    # resident sets: the same eight parameters, twice (nothing a model's fits leave behind reaches the next model's)
    sets = ba.CalibSamples(gpu_ctx, s0, *E[:6])
    try:
        assert sets.state_after == after_std
        for _ in range(2):
            again = bc.fresh_model(fixture, index)
            assert ba.calibrate(gpu_ctx, again, 1, s0, sets, **kw) == s1
            assert np.array_equal(again.evparam.view(np.uint32), ev.view(np.uint32))
        with pytest.raises(ba.BathError):                          # sets drawn from another state are refused
            ba.calibrate(gpu_ctx, bc.fresh_model(fixture, index), 1, s1, sets, **kw)
    finally:
        sets.close()


def test_three_residue_query(gpu_ctx, tmp_path):
    """The smallest model with an interior node is calibrated and written without error, and read back."""
    hmm = ba.seq_model(bc.score_system(), "MKV", "tiny")
    ba.hmm_set_max_length(hmm, ba.hmm_max_length(hmm, 1e-7))
    ba.calibrate(gpu_ctx, hmm, 1, ba.rng_state(42))
    assert hmm.M == 3 and np.all(np.isfinite(hmm.evparam)) and np.all(hmm.evparam != ba.FS_UNSET)
    path = str(tmp_path / "tiny.bhmm")
    with open(path, "wb") as fh:
        fh.write(ba.hmm_text(hmm, date="-"))
    back = ba.HMM(path)
    assert (back.M, back.name, back.consensus[1:4].lower(), back.max_length) == (3, "tiny", "mkv", hmm.max_length)
    assert np.allclose(back.evparam, hmm.evparam, atol=5.1e-5)     # the file's four and five decimals
    want, _ = bc.oracle_calibrate_cached("MKV")
    assert hmm.evparam[0] == want.evparam[0] and hmm.evparam[2] == want.evparam[2] and abs(float(hmm.evparam[6]) - float(want.evparam[6])) <= 1e-6


@pytest.mark.parametrize("fixture,index", [("AMP_N", 0), ("three_seqs", 1)])
def test_frameshift_taus_against_the_recorded(gpu_ctx, fixture, index):
    """As bathconvert's are held: the strict taus are the CPU path's, which the CPU tier holds against the record; in the
    reference's arithmetic (--arith odds) each tau lands closer to the record than the strict one does."""
    pin = json.load(open(PIN_JSON))
    m = next(m for m in pin["models"] if (m["fixture"], m["record"]) == (fixture, index))
    hmm = bc.fresh_model(fixture, index)
    ba.calibrate(gpu_ctx, hmm, 1, ba.rng_state(42), arith="odds")
    want, _ = bc.oracle_fixture(fixture, index)
    assert hmm.evparam[0] == want.evparam[0] and hmm.evparam[2] == want.evparam[2]      # the standard fits do not depend on --arith
    for key, j in (("fs3", 6), ("fs5", 7)):
        d = float(hmm.evparam[j]) - float(m[key]["recorded"])
        print("%s %s: odds minus recorded %+.2e, strict minus recorded %+.2e" % (hmm.name, key, d, m[key]["diff"]))
        assert abs(d) < abs(m[key]["diff"])


def search_output(model, fs, tmp_path, tag):
    out = str(tmp_path / (tag + ".out"))
    argv = (["--fs"] if fs else []) + ["-o", out, model, bc.golden("target-AMP_N.fa")]
    assert bs.run(argv, stdout=io.StringIO()) == 0
    return [ln for ln in open(out).read().splitlines() if not ln.startswith(("# CPU time:", "# Mc/sec:")) and model not in ln and out not in ln]


def evalue_tokens(lines):
    """{(line, token)} of the E-values of a main output: token 0 of the rows under "Scores for complete hits", the Evalue field (token 3,
    after the mark, score and bias) of a hit's '!' / '?' row."""
    at, in_scores = set(), False
    for n, ln in enumerate(lines):
        t = ln.split()
        if ln.startswith("Scores for complete hits"):
            in_scores = True
        elif in_scores and not t:
            in_scores = False
        elif in_scores and t[0] not in ("E-value", "-------") and not ln.lstrip().startswith(("-", "[")):
            at.add((n, 0))
        elif t and t[0] in ("!", "?") and len(t) > 3:
            at.add((n, 3))
    return at


@pytest.mark.parametrize("fs", [False, True], ids=["plain", "fs"])
def test_build_then_search(tmp_path, fs):
    """bathbuild on AMP_N.fa, then bathsearch of the written file against target-AMP_N.fa: every token of the main output -- hit
    coordinates, scores, alignment blocks, pipeline counts -- EQUALS that of the search with the recorded AMP_N.bhmm.  Only an
    E-value may differ: within exp(lambda |delta tau|) for the largest difference between a written and a recorded parameter, and
    on top of that the two-significant-digit print of either side (half a unit of the second digit: 5 % each)."""
    built = str(tmp_path / "AMP_N.bhmm")
    assert bb.run([built, bc.golden("AMP_N.fa")], stdout=io.StringIO()) == 0
    rec = bc.golden("AMP_N.bhmm")
    got_text, rec_text = open(built, "rb").read(), open(rec, "rb").read()
    assert bc.stable_lines(got_text)[:17] == bc.stable_lines(rec_text)[:17] and len(got_text) == len(rec_text)
    a, b = ba.HMM(built), ba.HMM(rec)
    dtau = float(np.abs(a.evparam.astype(np.float64) - b.evparam).max())
    from_tau, print_rounding = np.exp(float(b.evparam[5]) * dtau), 1.05 * 1.05
    got, want = search_output(built, fs, tmp_path, "built"), search_output(rec, fs, tmp_path, "recorded")
    assert len(got) == len(want) and any(ln.startswith(">> ") for ln in want)          # there is a hit to compare
    evalues = evalue_tokens(want)
    assert len(evalues) >= 2 and evalues == evalue_tokens(got)
    moved = 0
    for n, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        gt, wt = g.split(), w.split()
        assert len(gt) == len(wt), (g, w)
        for j, (x, y) in enumerate(zip(gt, wt)):
            if x != y:
                assert (n, j) in evalues, (n, j, g, w)               # anything but an E-value is equal
                assert abs(float(x) - float(y)) <= (from_tau * print_rounding - 1.0) * float(y), (g, w)
                moved += 1
    print("delta tau %.2e: E-values within %.4f relative from the taus, x %.4f for the print; %d printed E-values differ" %
          (dtau, from_tau - 1.0, print_rounding, moved))
