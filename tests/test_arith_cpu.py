"""CPU tier of --arith (the reference's odds-ratio arithmetic through bathsearch and bathconvert): the redraw loop of calibration
(bath_calib_fit_scores) against a serial restatement of evalues.c:633-649, the two command lines' option handling, and the
committed pin of the GPU's odds taus against the reference's recorded conversion.  No GPU."""
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import calib_common as cc
from bath_amd import bathconvert as bc
from bath_amd import bathsearch as bs

STRICT_JSON = os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")
ODDS_JSON = os.path.join(ba._ROOT, "profiles", "bathconvert_odds_vs_recorded.json")
NULLSC = np.float32(-3.25)


def read(path):
    with open(path, "rb") as fh:
        return fh.read().decode("latin-1")


# ---- the redraw driver
def fake_score(dna):
    """A deterministic score per sequence from its bytes alone."""
    d = np.asarray(dna, dtype=np.int64)
    w = np.arange(1, d.shape[1] + 1, dtype=np.int64)
    return ((d * w).sum(axis=1) % 1009).astype(np.float32) / np.float32(7.0) - np.float32(40.0)


def stream(state, L, n, table):
    """The first n sequences of the serial loop's stream (whatever their scores), as bytes."""
    out = []
    for _ in range(n):
        dna, state = ba.calib_sample(state, L, 1, table)
        out.append(dna[0].tobytes())
    return out


def scorer(fail):
    """fake_score with -inf for the sequences <fail> (a set of byte strings, or a predicate on a row) names."""
    def score(dna):
        sc = fake_score(dna)
        for j, row in enumerate(np.asarray(dna)):
            if (row.tobytes() in fail) if isinstance(fail, (set, frozenset)) else fail(row):
                sc[j] = -np.inf
        return sc
    return score


def serial_loop(state, score, L, N, table):
    """evalues.c:633-649 with its `i--; continue`, one sequence at a time."""
    xv, redrawn = [], 0
    while len(xv) < N:
        dna, state = ba.calib_sample(state, L, 1, table)
        sc = np.float32(score(dna)[0])
        if not np.isfinite(sc):
            redrawn += 1
            assert redrawn <= N
            continue
        xv.append(float(sc - NULLSC) / cc.LN2)
    return np.array(xv, np.float64), state, redrawn


@pytest.mark.parametrize("table", [1, 11])
@pytest.mark.parametrize("L,N", [(10, 8), (100, 200)])
def test_fit_scores_equals_the_serial_loop(L, N, table):
    s0 = ba.rng_state(7)
    seqs = stream(s0, L, N + 8, table)
    cases = {"none": set(), "first": {seqs[0]}, "last": {seqs[N - 1]}, "two in a row": {seqs[3], seqs[4]},
             "first, two in a row, and the redrawn last": {seqs[0], seqs[3], seqs[4], seqs[N + 2]},
             "sum mod 7": lambda row: int(row.sum()) % 7 == 0}
    for name, fail in cases.items():
        sc = scorer(fail)
        want_xv, want_state, want_re = serial_loop(s0, sc, L, N, table)
        xv, state, redrawn = ba.calib_fit_scores(s0, sc, NULLSC, L, N, table)
        assert redrawn == want_re, name
        assert state == want_state, name
        assert xv.tobytes() == want_xv.tobytes(), name
        if isinstance(fail, set):
            assert redrawn == len(fail), name
    assert serial_loop(s0, scorer(cases["sum mod 7"]), L, N, table)[2] > 0          # the predicate does discard at these sizes
    # nothing discarded: the generator ends where one calib_sample call of N ends
    assert ba.calib_fit_scores(s0, fake_score, NULLSC, L, N, table)[1] == ba.calib_sample(s0, L, N, table)[1]


def test_fit_scores_gives_up_after_n_discards():
    calls = []

    def never(dna):
        calls.append(len(dna))
        return np.full(len(dna), -np.inf, np.float32)
    with pytest.raises(ba.BathError) as e:
        ba.calib_fit_scores(ba.rng_state(7), never, NULLSC, 10, 8, 1)
    assert e.value.status == ba.ERANGE and e.value.redrawn == 9 and calls == [8, 8]
    with pytest.raises(ba.BathError) as e:                                             # NaN and +inf are discarded as -inf is
        ba.calib_fit_scores(ba.rng_state(7), lambda d: np.where(np.arange(len(d)) % 2 == 0, np.nan, np.inf).astype(np.float32), NULLSC, 10, 8, 1)
    assert e.value.status == ba.ERANGE


def test_fit_scores_passes_a_scorer_exception_on():
    def broken(dna):
        raise KeyError("scorer")
    with pytest.raises(KeyError):
        ba.calib_fit_scores(ba.rng_state(7), broken, NULLSC, 10, 8, 1)


def test_arith_modes():
    assert ba.ARITH_MODES == {"strict": 0, "odds3": 1, "odds": 2}
    assert (ba.ARITH_STRICT, ba.ARITH_ODDS3, ba.ARITH_ODDS) == (0, 1, 2)
    with pytest.raises(ValueError):
        ba.calibrate_fs(None, None, 1, 0, arith="fast")


# ---- bathsearch
def test_bathsearch_arith_option():
    for v in ("strict", "odds3", "odds"):
        assert bs.parse_args(["--fs", "--arith", v, "a.bhmm", "t.fa"])[0]["--arith"] == v
        assert bs.parse_args(["--arith=" + v, "--fs", "a.bhmm", "t.fa"])[0]["--arith"] == v
    for bad in ("fast", "ODDS", "odds5", ""):
        with pytest.raises(bs.UsageError, match="--arith"):
            bs.parse_args(["--fs", "--arith", bad, "a.bhmm", "t.fa"])
    with pytest.raises(bs.UsageError, match="--arith"):
        bs.parse_args(["--fs", "a.bhmm", "t.fa", "--arith"])
    with pytest.raises(bs.UsageError, match="--arith requires --fs"):
        bs.parse_args(["--arith", "odds", "a.bhmm", "t.fa"])
    assert bs.REQUIRES["--arith"] == "--fs"
    # with the other extensions, untouched
    o = bs.parse_args(["--fs", "--arith", "odds", "--ensemble", "device", "--ensemble-std", "streams", "--workers", "2", "--gpus", "2", "a", "b"])[0]
    assert (o["--arith"], o["--ensemble"], o["--ensemble-std"], o["--workers"], o["--gpus"]) == ("odds", "device", "streams", 2, 2)


def test_bathsearch_arith_writes_no_header_line():
    base = ["--fs", "--cigar", "--tblout", "x.tbl", "-o", "x.out"]
    want = bs.output_header(bs.parse_args(base + ["a.bhmm", "t.fa"])[0], "a.bhmm", "t.fa")
    for v in ("strict", "odds3", "odds"):
        assert bs.output_header(bs.parse_args(base + ["--arith", v, "a.bhmm", "t.fa"])[0], "a.bhmm", "t.fa") == want


def test_new_context_is_the_one_place_that_applies_arith(monkeypatch):
    class Ctx:
        def __init__(self, device):
            self.calls = {}

        def __getattr__(self, name):
            if not name.startswith("set_"):
                raise AttributeError(name)
            return lambda v=True: self.calls.__setitem__(name, v)
    monkeypatch.setattr(ba, "Context", Ctx)
    want = {None: (False, False), "strict": (False, False), "odds3": (True, False), "odds": (True, True)}
    for v, (o3, o5) in want.items():
        opts = {"--fs": True, "--ensemble": "device"}
        if v is not None:
            opts["--arith"] = v
        c = bs.new_context(0, opts).calls
        assert c["set_fs_strict"] is True, v                               # in every mode
        assert (bool(c["set_fs_odds"]), bool(c["set_fs5_odds"])) == (o3, o5), v
        assert c["set_fs_ensemble"] == "device" and c["set_std_ensemble"] == "serial", v


# ---- bathconvert
def test_bathconvert_arith_option():
    assert bc.parse_options(["out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm", {"arith": "strict"})
    for v in ("strict", "odds3", "odds"):
        assert bc.parse_options(["--arith", v, "out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm", {"arith": v})
        assert bc.parse_options(["--ct", "11", "out.bhmm", "--arith=" + v, "in.hmm"]) == (11, "out.bhmm", "in.hmm", {"arith": v})
        assert bc.parse_args(["--arith", v, "--ct=4", "out.bhmm", "in.hmm"]) == (4, "out.bhmm", "in.hmm")
    for bad in (["--arith", "fast", "a", "b"], ["--arith", "ODDS", "a", "b"], ["--arith=", "a", "b"]):
        with pytest.raises(bc.UsageError, match="--arith"):
            bc.parse_options(bad)
    with pytest.raises(bc.UsageError, match="--arith needs an argument"):
        bc.parse_options(["a", "b", "--arith"])
    # the forms tests/test_bathconvert_cpu.py::test_parse_args pins
    assert bc.parse_args(["out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm")
    assert bc.parse_args(["--ct", "11", "out.bhmm", "in.hmm"]) == (11, "out.bhmm", "in.hmm")
    assert bc.parse_args(["out.bhmm", "--ct=4", "in.hmm"]) == (4, "out.bhmm", "in.hmm")
    for bad in (["--ct", "0", "a", "b"], ["--ct", "7", "a", "b"], ["--ct", "x", "a", "b"], ["--ct"], ["a", "b", "--ct"], ["a"], ["a", "b", "c"], [],
                ["--gpus", "2", "a", "b"], ["--workers", "2", "a", "b"], ["-x", "a", "b"], ["-h"]):
        for parse in (bc.parse_args, bc.parse_options):
            with pytest.raises(bc.UsageError):
                parse(bad)


def test_bathconvert_arith_keeps_a_bath_files_taus_without_a_gpu(tmp_path, monkeypatch):
    want = read(cc.BHMM_OUT)
    ct_opt, _, _, opts = bc.parse_options(["--arith", "odds", "out.bhmm", cc.BHMM_OUT])
    assert opts["arith"] == "odds" and not any(bc.model_plan(m, ct_opt)["fit"] for m in bc.split_models(want))

    def no_gpu(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(ba, "Context", no_gpu)
    out = tmp_path / "out.bhmm"
    import io
    text = io.StringIO()
    assert bc.run(["--arith", "odds", str(out), cc.BHMM_OUT], stdout=text) == 0
    assert read(str(out)) == want and len([ln for ln in text.getvalue().splitlines() if ln.startswith("  ")]) == 12


# ---- the pin: the GPU's odds taus against the reference's recorded conversion
def test_pin_file_of_the_odds_taus():
    pin, strict = json.load(open(ODDS_JSON)), json.load(open(STRICT_JSON))
    rec = cc.recorded(cc.BHMM_OUT)
    assert len(pin["models"]) == 12 == len(strict["models"]) == len(rec)
    assert (pin["L"], pin["N"], pin["tailp"]) == (ba.CALIB_L, ba.CALIB_N, ba.CALIB_TAILP)
    for i, (m, s, r) in enumerate(zip(pin["models"], strict["models"], rec)):
        assert m["index"] == i and m["name"] == s["name"]
        for key, tau in (("fs3", r[1]), ("fs5", r[2])):
            e = m[key]
            assert e["recorded"] == tau == s[key]["recorded"], (i, key)
            assert e["strict_diff"] == s[key]["diff"] and e["exact_logsum_diff"] == s[key]["diff_exact_logsum"], (i, key)
            assert e["diff"] == pytest.approx(e["gpu_odds"] - e["recorded"], abs=1e-12), (i, key)
            assert isinstance(e["redrawn"], int) and e["redrawn"] >= 0, (i, key)
            # the condition: the reference's arithmetic lands closer to the reference's record than the strict arithmetic does
            assert abs(e["diff"]) < abs(e["strict_diff"]), (i, m["name"], key, e["diff"], e["strict_diff"])
