"""CPU tier of bathconvert (bath_amd/bathconvert.py, bath_amd/csrc/bath_calibrate.hip): MAXL, the text rewrite, the sample stream, the
Gumbel fit, the pin against the reference's recorded conversion of tutorial/tRNA-proteins.hmm, bathsearch's refusal of a model file
without frameshift taus, and the command line.  No GPU: where scores are needed the oracle's Forward recursions give them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import calib_common as cc
import oracle_lib as ol
from bath_amd import bathconvert as bc
from bath_amd import bathsearch as bs
from bath_amd import synth

PIN_JSON = os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")


def read(path):
    with open(path, "rb") as fh:
        return fh.read().decode("latin-1")


# ---- 1: MAXL
def test_max_length_equals_the_recorded_maxl():
    rec = cc.recorded(cc.BHMM_OUT)
    assert len(rec) == 12 == ba.HMM.count(cc.HMM_IN)
    for i, r in enumerate(rec):
        hmm = ba.HMM(cc.HMM_IN, i)
        assert hmm.max_length == 0                               # the HMMER3 file has none
        assert ba.hmm_max_length(hmm, 1e-7) == r[0], i


# ---- 2: the rewrite
def test_rewrite_with_the_recorded_taus_is_the_recorded_file():
    rec = cc.recorded(cc.BHMM_OUT)
    got = bc.rewrite(read(cc.HMM_IN), [(r[1], r[2]) for r in rec], [r[0] for r in rec])
    assert got == read(cc.BHMM_OUT)


def test_rewrite_of_a_bath_file_changes_nothing():
    want = read(cc.BHMM_OUT)
    assert bc.rewrite(want, None) == want
    plans = [bc.model_plan(m, None) for m in bc.split_models(want)]
    assert not any(p["fit"] or p["need_maxl"] for p in plans) and all(p["ct"] == 1 for p in plans)
    assert all(bc.model_plan(m, 11)["fit"] for m in bc.split_models(want))              # --ct with another table: fitted again
    assert not any(bc.model_plan(m, 1)["fit"] for m in bc.split_models(want))            # --ct with the file's: kept
    assert all(p["fit"] and p["need_maxl"] and p["ct"] == 1 for p in (bc.model_plan(m, None) for m in bc.split_models(read(cc.HMM_IN))))
    with pytest.raises(ValueError):
        bc.rewrite(read(cc.HMM_IN), None, None)                                          # taus to fit, none given


# ---- 3: the sample stream, against a restatement in plain Python
def py_seed(seed):
    m = 0xffffffff
    a, b, c = seed & m, 87654321, 12345678
    for s1, s2, s3 in ((13, 8, 13), (12, 16, 5), (3, 10, 15)):
        a = (a - b - c) & m; a ^= c >> s1
        b = (b - c - a) & m; b ^= (a << s2) & m
        c = (c - a - b) & m; c ^= b >> s3
    return c if c else 42


def py_sample(state, f, ncbi_table, L, N):
    basic = ba.gencode_basic(ncbi_table)
    codons = [[c for c in range(64) if basic[c] == a] for a in range(20)]             # x, y, z order over ACGT: ascending 16x + 4y + z
    f = [np.float32(v) for v in f]

    def rnd():
        nonlocal state
        state = (state * 69069 + 1) & 0xffffffff
        return state / 4294967296.0

    out = np.zeros((N, 3 * L), np.uint8)
    for s in range(N):
        aa = []
        for _ in range(L):
            while True:                                                               # esl_rnd_FChoose: a roll beyond the sum is drawn again
                roll, acc, hit = np.float32(rnd()), np.float32(0.0), -1
                for q in range(20):
                    acc = np.float32(acc + f[q])
                    if roll < acc:
                        hit = q
                        break
                if hit >= 0:
                    break
            aa.append(hit)
        for i, a in enumerate(aa):
            c = codons[a][int(rnd() * len(codons[a]))]                                # esl_rnd_Roll
            out[s, 3 * i:3 * i + 3] = (c >> 4, (c >> 2) & 3, c & 3)
    return out, state


@pytest.mark.parametrize("L,N", [(1, 1), (5, 3), (100, 200)])
@pytest.mark.parametrize("table", [1, 4])
def test_sample_stream_equals_the_restatement(L, N, table):
    assert ba.rng_state(42) == py_seed(42) and ba.rng_state(7) == py_seed(7)
    f = ol.Bg()
    ol.lib().bo_bg_create(C.byref(f))
    freqs = np.array(f.f[:20], np.float32)
    assert (freqs == synth.BG.astype(np.float32)).all()
    want, wstate = py_sample(py_seed(42), freqs, table, L, N)
    got, gstate = ba.calib_sample(ba.rng_state(42), L, N, table)
    assert (got == want).all() and gstate == wstate
    got2, gstate2 = ba.calib_sample(ba.rng_state(42), L, N, table, f=freqs)           # the default frequencies are the background
    assert (got2 == want).all() and gstate2 == wstate
    nxt, nstate = ba.calib_sample(gstate, L, N, table)                                # the state goes in and out: a second call goes on
    want2, wstate2 = py_sample(wstate, freqs, table, L, N)
    assert (nxt == want2).all() and nstate == wstate2


def test_sample_stream_rerolls_beyond_the_frequencies_sum():
    freqs = (synth.BG * 0.9).astype(np.float32)
    want, wstate = py_sample(py_seed(42), freqs, 1, 100, 20)
    plain, pstate = py_sample(py_seed(42), synth.BG.astype(np.float32), 1, 100, 20)
    got, gstate = ba.calib_sample(ba.rng_state(42), 100, 20, 1, f=freqs)
    assert (got == want).all() and gstate == wstate
    assert wstate != pstate                                       # re-rolls happened: more numbers were drawn than 2 x L x N
    with pytest.raises(ba.BathError):
        ba.calib_sample(ba.rng_state(42), 5, 3, 7)                # no such table


# ---- 4: the Gumbel fit, against a bisection on the same likelihood equation
def lawless(x, lam):
    e = np.exp(-lam * x)
    return 1.0 / lam - x.mean() + (x * e).sum() / e.sum()


def bisect_fit(x):
    lo, hi = 1e-6, 1.0
    while lawless(x, hi) > 0:
        hi *= 2
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if lawless(x, mid) > 0:
            lo = mid
        else:
            hi = mid
    lam = 0.5 * (lo + hi)
    return -np.log(np.exp(-lam * x).mean()) / lam, lam


def gumbel_samples():
    rng = np.random.default_rng(11)
    known = -5.0 - np.log(-np.log(rng.random(200))) / 0.71                          # mu = -5, lambda = 0.71
    model = ol.Model(cc.HMM_IN, 0)
    dna, _ = ba.calib_sample(ba.rng_state(42), 100, 200, 1)
    real = cc.oracle_bits(model, model.basic, 3, dna, 100)                          # the bit scores the first FS3 fit of the file sees
    small = -3.0 - np.log(-np.log(rng.random(8))) / 0.7
    return {"known": known, "real": real, "n8": small}


@pytest.mark.parametrize("which", ["known", "real", "n8"])
def test_gumbel_fit_equals_bisection(which):
    x = gumbel_samples()[which]
    mu, lam = ba.gumbel_fit_complete(x)
    bmu, blam = bisect_fit(np.asarray(x, np.float64))
    print(which, mu, lam, bmu, blam)
    assert abs(lam - blam) <= 1e-6 * abs(blam) and abs(mu - bmu) <= 1e-6 * abs(bmu)
    if which == "known":
        assert abs(lam - 0.71) < 0.1 and abs(mu + 5.0) < 0.3                        # (the sample's own spread at n = 200)
    p = 0.96
    assert abs(ba.gumbel_invcdf(p, mu, lam) - (mu - np.log(-np.log(p)) / lam)) < 1e-12
    assert abs(ba.calib_tau(x, 0.7, 0.04) - (ba.gumbel_invcdf(0.96, mu, lam) + np.log(0.04) / 0.7)) < 1e-12


# ---- 5: the pin against the reference's recorded run
def test_taus_against_the_recorded_conversion():
    """OUTCOME B, measured before any GPU work (tools/bathconvert_pin.py -> profiles/bathconvert_vs_recorded.json): the 24 taus of the
    CPU path (library sampler and fit, oracle Forward with the table log-sums the strict kernels reproduce, one generator carried
    through the file) are all 3.8e-3 .. 6.7e-3 ABOVE the recorded ones, not within 1.5e-4.  The offset has one sign and nearly one size
    on every model, first to last, FS3 (4.5e-3) and FS5 (5.8e-3) alike, where a wrong sample stream would scatter by the taus' own
    spread of ~0.1: the stream is the reference's, the arithmetic is not -- the recorded file was made by the odds-ratio SSE parsers
    (exact sums), the path here uses p7_FLogsum's table.  The JSON also holds the same path with exact log-sums.  So, as the issue
    sets for this outcome, each difference is held against 4 standard deviations of that tau over the 50 reseeded runs of this same
    path stored in the JSON; the stored values are held against this run's."""
    pin = json.load(open(PIN_JSON))
    rec = cc.recorded(cc.BHMM_OUT)
    got = cc.oracle_file(cc.HMM_IN)
    assert len(pin["models"]) == len(rec) == len(got) == 12
    for i, (m, r, g) in enumerate(zip(pin["models"], rec, got)):
        for j, key in enumerate(("fs3", "fs5")):
            d = g[j] - r[1 + j]
            print("%-12s %s recorded %8.4f here %9.5f diff %+.2e sd(50 reseeded) %.3f" % (m["name"], key, r[1 + j], g[j], d, m[key]["reseeded_sd"]))
            assert m[key]["recorded"] == r[1 + j]
            assert abs(m[key]["cpu_path"] - g[j]) < 1e-9, (i, key)               # the stored measurement is this path's
            assert abs(d) <= 4.0 * m[key]["reseeded_sd"], (i, key, d)
    assert pin["max_abs_diff"] > pin["bound_outcome_A"] == 1.5e-4                    # outcome B is what was measured


# ---- 6: bathsearch refuses what it cannot score
def test_bathsearch_refuses_a_model_file_without_frameshift_taus(capsys, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the refusal")
    monkeypatch.setattr(ba, "Context", no_gpu)
    monkeypatch.setattr(bs, "new_context", no_gpu)
    monkeypatch.setattr(bs, "launch_ranks", no_gpu)
    target = os.path.join(ol.GOLDEN, "target-PTH2.fa")
    for extra in ([], ["--fs"], ["--gpus", "2"], ["--workers", "2"]):
        assert bs.run(extra + [cc.HMM_IN, target]) == 1
        err = capsys.readouterr().err
        assert ("HMM file %s not formated for this version bathsearch. Please run 'bathconvert new_file.bhmm old_file.bhmm'." % cc.HMM_IN) in err


def test_bathsearch_refusal_from_the_command_line():
    r = subprocess.run([sys.executable, "-m", "bath_amd.bathsearch", cc.HMM_IN, os.path.join(ol.GOLDEN, "target-PTH2.fa")],
                       cwd=ba._ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "not formated for this version bathsearch" in r.stderr and r.stdout == ""


# ---- 7: the command line
def test_parse_args():
    assert bc.parse_args(["out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm")
    assert bc.parse_args(["--ct", "11", "out.bhmm", "in.hmm"]) == (11, "out.bhmm", "in.hmm")
    assert bc.parse_args(["out.bhmm", "--ct=4", "in.hmm"]) == (4, "out.bhmm", "in.hmm")
    for bad in (["--ct", "0", "a", "b"], ["--ct", "7", "a", "b"], ["--ct", "26", "a", "b"], ["--ct", "x", "a", "b"], ["--ct"], ["a", "b", "--ct"],
                ["a"], ["a", "b", "c"], [], ["--gpus", "2", "a", "b"], ["--workers", "2", "a", "b"], ["-x", "a", "b"], ["-h"]):
        with pytest.raises(bc.UsageError):
            bc.parse_args(bad)


def test_refused_inputs_exit_1_naming_them(tmp_path, capsys):
    out = str(tmp_path / "out.bhmm")
    text = read(cc.HMM_IN)
    one = bc.split_models(text)[0]
    cases = {"older.hmm": (one.replace("HMMER3/f", "HMMER3/b", 1), "HMMER3/b"),
             "binary.h3m": (b"\xe8\xed\xed\xb3" + b"\0" * 64, "binary"),
             "dna.hmm": (one.replace("ALPH  amino", "ALPH  DNA", 1), "Invalid alphabet type"),
             "fasta.fa": (">seq\nACGT\n", "not a profile HMM file"),
             "cut.hmm": (one[:len(one) // 2], "//")}
    for name, (body, word) in cases.items():
        p = tmp_path / name
        p.write_bytes(body if isinstance(body, bytes) else body.encode("latin-1"))
        assert bc.run([out, str(p)]) == 1
        assert word in capsys.readouterr().err, name
        assert not os.path.exists(out)
    same = tmp_path / "same.hmm"
    same.write_text(one)
    assert bc.run([str(same), str(same)]) == 1 and "is the input file" in capsys.readouterr().err
    assert same.read_text() == one
    assert bc.run([out, str(tmp_path / "missing.hmm")]) == 1 and "missing.hmm" in capsys.readouterr().err
    assert bc.run(["--ct", "99", out, cc.HMM_IN]) == 1 and "--ct" in capsys.readouterr().err


def test_keeping_the_taus_needs_no_gpu(tmp_path, capsys, monkeypatch):
    """--ct equal to the file's table, or none, on a BATH file: nothing is fitted, no context is created, the text comes back."""
    def no_gpu(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(ba, "Context", no_gpu)
    src = os.path.join(ol.GOLDEN, "PTH2.bhmm")
    for extra in ([], ["--ct", "1"]):
        out = str(tmp_path / "o.bhmm")
        assert bc.run(extra + [out, src]) == 0
        assert read(out) == read(src)
        text = capsys.readouterr().out
        assert text.startswith(bc.BANNER) and "# CPU time:" in text.splitlines()[-1]
        assert len([ln for ln in text.splitlines() if ln and not ln.startswith("#")]) == 1


def test_summary_line_equals_the_tutorial():
    """documentation/userguide/tutorial.md, Practice 5: the first result line of the recorded conversion."""
    p = bc.model_plan(bc.split_models(read(cc.HMM_IN))[0], None)
    assert bc.result_line(1, p, bc.mean_match_relative_entropy(ba.HMM(cc.HMM_IN, 0))) == \
        "  1      ATE_N                   30    78         1     1.11  0.726 Arginine-tRNA-protein transferase, N terminus\n"
