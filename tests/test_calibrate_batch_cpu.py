"""CPU tier of bathconvert --batch: the batch sampler against successive calib_sample calls, the option and its refusals, the
library's refusal of a null context, and that the oracle scores every input of tests/test_calibrate_batch_gpu.py finitely -- the GPU
tests leave no case out for want of a reference."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
import calib_batch_common as cb
from bath_amd import bathconvert as bc


def serial_samples(state, tables, L, N):
    parts = []
    for t in tables:
        for _ in range(2):                                            # a model's 3-codon set, then its 5-codon set
            dna, state = ba.calib_sample(state, L, N, t)
            parts.append(dna)
    return np.array(parts, np.uint8).reshape(len(tables), 2, N, 3 * L), state


@pytest.mark.parametrize("tables", [(1,), (4,), (1, 4, 1), (4, 1, 4)])
def test_sample_batch_is_the_serial_stream(tables):
    L, N = 10, 7
    want, wstate = serial_samples(cb.S0, tables, L, N)
    got, gstate = ba.calib_sample_batch(cb.S0, tables, L, N)
    assert got.shape == (len(tables), 2, N, 3 * L) and got.dtype == np.uint8
    assert np.array_equal(got, want) and gstate == wstate
    again, astate = ba.calib_sample_batch(gstate, tables[:1], L, N)    # the state goes in and out
    assert np.array_equal(again, serial_samples(wstate, tables[:1], L, N)[0]) and astate != gstate
    if len(tables) > 1:                                                # tables 1 and 4 differ (UGA), so the sets are the tables' own
        assert not np.array_equal(got, ba.calib_sample_batch(cb.S0, (1,) * len(tables), L, N)[0])


def raw_sample_batch(state, tables, L, N):
    st = C.c_uint32(state)
    tabs = np.array(tables, np.int32)
    dna = np.full((len(tables), 2, N, 3 * L), 255, np.uint8)
    rc = ba.lib().bath_calib_sample_batch(C.byref(st), None, tabs.ctypes.data_as(C.POINTER(C.c_int)), len(tables), L, N,
                                          dna.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, st.value


def test_sample_batch_refuses_and_keeps_the_state():
    """An unknown table anywhere in the batch: an error, and the caller's state is what it was although the models before it were
    drawn.  (A table without a codon for a background residue returns the same error from bath_calib_sample; none of the tables
    this build knows lacks one, which is held here, so that case cannot be built from real tables.)"""
    for tables in ((7,), (1, 7), (1, 4, 99)):
        rc, state = raw_sample_batch(cb.S0, tables, 10, 7)
        assert rc == ba.EINVAL and state == cb.S0, tables
        with pytest.raises(ba.BathError, match="translation table"):
            ba.calib_sample_batch(cb.S0, tables, 10, 7)
    assert raw_sample_batch(cb.S0, (1, 4), 10, 7) == (ba.OK, serial_samples(cb.S0, (1, 4), 10, 7)[1])
    for t in bc.NCBI_TABLES:
        basic = np.zeros(64, np.uint8)
        assert ba.lib().bath_gencode_basic(t, basic.ctypes.data_as(C.POINTER(C.c_uint8))) == ba.OK
        assert set(range(20)) <= set(basic.tolist()), t


def test_batch_option():
    assert bc.parse_options(["out.bhmm", "in.hmm"])[3].get("batch", 1) == 1            # the default: today's path
    for n in (1, 2, 12, 64):
        assert bc.parse_options(["--batch", str(n), "out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm", {"arith": "strict", "batch": n})
        assert bc.parse_options(["--ct", "4", "out.bhmm", "--batch=%d" % n, "in.hmm"]) == (4, "out.bhmm", "in.hmm", {"arith": "strict", "batch": n})
        assert bc.parse_args(["--batch", str(n), "out.bhmm", "in.hmm"]) == (None, "out.bhmm", "in.hmm")
    assert bc.parse_options(["--batch", "1", "--arith", "odds", "a", "b"])[3] == {"arith": "odds", "batch": 1}   # one model per call: today's path
    for bad in (["--batch", "0", "a", "b"], ["--batch", "65", "a", "b"], ["--batch=-3", "a", "b"],              # outside 1..64
                ["--batch", "x", "a", "b"], ["--batch=", "a", "b"], ["--batch", "2.5", "a", "b"],               # not a number
                ["--batch", "2", "--arith", "odds", "a", "b"], ["--arith=odds3", "--batch=64", "a", "b"]):      # strict arithmetic only
        with pytest.raises(bc.UsageError, match="--batch"):
            bc.parse_options(bad)
    with pytest.raises(bc.UsageError, match="--batch needs an argument"):
        bc.parse_options(["a", "b", "--batch"])


@pytest.mark.parametrize("argv", [["--batch", "2", "--arith", "odds"], ["--batch", "0"], ["--batch", "65"], ["--batch", "many"]])
def test_batch_refusals_exit_with_status_1(argv, tmp_path, capsys):
    """Refused before the input is opened or a context made: status 1, the option named, no output file."""
    import calib_common as cc
    out = tmp_path / "out.bhmm"
    assert bc.run(argv + [str(out), cc.HMM_IN]) == 1
    err = capsys.readouterr().err
    assert err.startswith("Error: ") and "--batch" in err and not out.exists()


def test_null_context_is_einval():
    st = C.c_uint32(cb.S0)
    t = np.zeros(1, np.float64)
    tabs = np.array([1], np.int32)
    hmm = cb.hmms(((1, 11),))
    ptrs = (C.POINTER(ba._Hmm) * 1)(hmm[0]._p)
    p = t.ctypes.data_as(C.POINTER(C.c_double))
    rc = ba.lib().bath_hip_calibrate_fs_batch(None, ptrs, tabs.ctypes.data_as(C.POINTER(C.c_int)), 1, C.byref(st), 10, 9, 0.04, p, p, None, None)
    assert rc == ba.EINVAL and st.value == cb.S0 and t[0] == 0.0


def all_finite(rows):
    return all(np.isfinite(r[3]).all() and np.isfinite(r[4]).all() and np.isfinite(r[0]) and np.isfinite(r[1]) for r in rows)


@pytest.mark.parametrize("case", cb.tiling_batches(), ids=lambda c: "C%d" % c[0])
def test_oracle_scores_of_the_tiling_batches_are_finite(case):
    _, specs, tables = case
    rows = cb.oracle_batch(specs, tables, cb.SMALL_L, cb.SMALL_N)
    assert len(rows) == len(specs) and all_finite(rows)
    assert rows[-1][2] == cb.sampler_state(tables, cb.SMALL_L, cb.SMALL_N)


def test_oracle_scores_of_the_other_batches_are_finite():
    assert all_finite(cb.oracle_batch(cb.ORDER_SPECS, cb.ORDER_TABLES, cb.SMALL_L, cb.SMALL_N))
    assert all_finite(cb.oracle_batch(cb.SINGLE_SPECS, cb.SINGLE_TABLES, cb.SMALL_L, cb.SMALL_N))
    full = cb.oracle_batch(cb.FULL_SPECS, cb.FULL_TABLES, cb.FULL_L, cb.FULL_N, limit=cb.FULL_ORACLE)
    assert len(full) == 2 and all_finite(full)
