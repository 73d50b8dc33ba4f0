"""GPU tier of bathconvert --batch: bath_hip_calibrate_fs_batch (fs3_fwd_batch_kernel, fs5_fwd_parser_batch_kernel: several models
per launch) at every per-lane tiling, in mixed order and at the full shape, against the CPU path of tests/calib_common.py (the
library's sampler and fit around the oracle's recursions) bit for bit and against the serial bath_amd.calibrate_fs loop exactly; its
refusals; and the command line, whose output with --batch N is the bytes of --batch 1."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import calib_batch_common as cb
import calib_common as cc
from bath_amd import bathconvert as bc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def serial_loop(ctx, hmms, tables, state, L, N):
    """[(tau3, tau5, state afterwards, xv3, xv5)] of successive calibrate_fs calls with the state carried."""
    out = []
    for h, t in zip(hmms, tables):
        r = ba.calibrate_fs(ctx, h, t, state, L, N, want_xv=True)
        state = r[2]
        out.append(r)
    return out


def check_batch(ctx, specs, tables, L, N, n_oracle=None, state=cb.S0):
    """One batch against the oracle path (the first n_oracle models; None: all) and the serial loop (all); returns the batch's result."""
    hmms = cb.hmms(specs)
    t3, t5, s1, x3, x5 = ba.calibrate_fs_batch(ctx, hmms, tables, state, L, N, want_xv=True)
    assert t3.shape == t5.shape == (len(specs),) and x3.shape == x5.shape == (len(specs), N)
    want = cb.oracle_batch(tuple(specs), tuple(tables), L, N, state, n_oracle)
    for k, w in enumerate(want):
        assert np.isfinite(w[3]).all() and np.isfinite(w[4]).all(), (k, "the reference must score every input")
        assert np.array_equal(bits(x3[k]), bits(w[3])), (k, specs[k], "xv3")
        assert np.array_equal(bits(x5[k]), bits(w[4])), (k, specs[k], "xv5")
        assert abs(t3[k] - w[0]) <= 1e-6 and abs(t5[k] - w[1]) <= 1e-6, (k, specs[k])      # (the fit is the library's in both)
    ser = serial_loop(ctx, hmms, tables, state, L, N)
    for k, r in enumerate(ser):
        assert (t3[k], t5[k]) == (r[0], r[1]), (k, specs[k])
        assert np.array_equal(bits(x3[k]), bits(r[3])) and np.array_equal(bits(x5[k]), bits(r[4])), (k, specs[k])
    assert s1 == ser[-1][2] == cb.sampler_state(tables, L, N, state)
    if n_oracle is None:
        assert s1 == want[-1][2]
    assert ba.calibrate_fs_batch(ctx, hmms, tables, state, L, N)[2] == s1                    # without xv: the same call
    return t3, t5, s1, x3, x5


@pytest.mark.parametrize("case", cb.tiling_batches(), ids=lambda c: "C%d" % c[0])
def test_every_tiling(gpu_ctx, case):
    """Per entry of BATH_FS_COLUMNS one batch of its smallest and its largest M (and M = 2 beside M = 1): two or three models in one
    launch of each parser, 9 windows of 30 nt each."""
    c, specs, tables = case
    check_batch(gpu_ctx, specs, tables, cb.SMALL_L, cb.SMALL_N)
    # the spans of the last call on the context, a batch: one tiling, one launch of each parser, and none of the single-model parsers
    # (the session's context may also report spans of its auxiliary contexts from earlier tests: other names, not looked at)
    kt = ba.kernel_times(gpu_ctx)
    assert kt["fs3_fwd_batch_kernel"][1] == 1 and kt["fs5_fwd_parser_batch_kernel"][1] == 1, (c, kt)
    assert "fs3_fwd_kernel" not in kt and "fs5_fwd_parser_kernel" not in kt, (c, kt)


def test_results_stand_in_input_order(gpu_ctx):
    """M = 1, 1280, 64, 65, 129, 65: the tilings alternate (the launches group them), one length comes twice with other parameters
    and another table; and a batch of one model."""
    t3, t5, _, x3, x5 = check_batch(gpu_ctx, cb.ORDER_SPECS, cb.ORDER_TABLES, cb.SMALL_L, cb.SMALL_N)
    assert not np.array_equal(bits(x3[3]), bits(x3[5])) and t3[3] != t3[5]                  # the two models of 65 nodes are not one
    kt = ba.kernel_times(gpu_ctx)
    fs = cb.fs_options()
    n_launch = len({min(c for c in fs if 64 * c >= m) for m, _ in cb.ORDER_SPECS})            # the tilings present: four
    assert kt["fs3_fwd_batch_kernel"][1] == n_launch and kt["fs5_fwd_parser_batch_kernel"][1] == n_launch, kt
    check_batch(gpu_ctx, cb.SINGLE_SPECS, cb.SINGLE_TABLES, cb.SMALL_L, cb.SMALL_N)


def test_full_shape(gpu_ctx):
    """What bathconvert runs: L = 100, N = 200.  ATE_N (M = 78), synthetic 129 and 459 with tables 1, 4, 1: the oracle path for the
    first two (the third's cost on the CPU is the reason), the serial loop for all three."""
    check_batch(gpu_ctx, cb.FULL_SPECS, cb.FULL_TABLES, cb.FULL_L, cb.FULL_N, n_oracle=cb.FULL_ORACLE)


def test_state_is_carried_between_batches(gpu_ctx):
    specs, tables = ((1, 11), (64, 13), (65, 14)), (4, 1, 4)
    L, N = cb.SMALL_L, cb.SMALL_N
    hmms = cb.hmms(specs)
    whole = ba.calibrate_fs_batch(gpu_ctx, hmms, tables, cb.S0, L, N, want_xv=True)
    a = ba.calibrate_fs_batch(gpu_ctx, hmms[:2], tables[:2], cb.S0, L, N, want_xv=True)
    b = ba.calibrate_fs_batch(gpu_ctx, hmms[2:], tables[2:], a[2], L, N, want_xv=True)
    assert b[2] == whole[2] and a[2] != cb.S0
    for i in (0, 1, 3, 4):
        assert np.array_equal(bits(np.concatenate([a[i], b[i]])), bits(whole[i])), i


def raw_batch(ctx, hmms, tables, state, L, N):
    """The C call with outputs the test owns: (status, state afterwards, tau3, tau5, xv3, xv5), the arrays filled with -7 before."""
    n = len(hmms)
    st = C.c_uint32(state)
    ptrs = (C.POINTER(ba._Hmm) * max(n, 1))(*[h._p for h in hmms])
    tabs = np.array(list(tables) + [1], np.int32)
    arrs = [np.full(max(n, 1), -7.0), np.full(max(n, 1), -7.0), np.full(max(n, 1) * N, -7.0), np.full(max(n, 1) * N, -7.0)]
    p = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
    rc = ba.lib().bath_hip_calibrate_fs_batch(ctx._h, ptrs, tabs.ctypes.data_as(C.POINTER(C.c_int)), n, C.byref(st), L, N, 0.04, *p)
    return (rc, st.value) + tuple(arrs)


def test_refusals_leave_everything_as_it_was(gpu_ctx):
    ctx = gpu_ctx
    L, N = cb.SMALL_L, cb.SMALL_N
    good = cb.hmms(((64, 13), (65, 14)))
    long_ = cb.hmms(((1281, 3),))[0]
    want = ba.calibrate_fs_batch(ctx, good, (1, 4), cb.S0, L, N, want_xv=True)

    def untouched(r):
        return r[1] == cb.S0 and all((a == -7.0).all() for a in r[2:])

    r = raw_batch(ctx, [good[0], long_, good[1]], (1, 1, 4), cb.S0, L, N)                    # a model beyond the kernels' 1280 nodes
    assert r[0] == ba.EINVAL and untouched(r)
    with pytest.raises(ba.BathError, match=r"position 1 .*1280 nodes \(this one has 1281\)"):
        ba.calibrate_fs_batch(ctx, [good[0], long_, good[1]], (1, 1, 4), cb.S0, L, N)
    with pytest.raises(ba.BathError, match=r"position 2 .*translation table 7"):
        ba.calibrate_fs_batch(ctx, [good[0], good[1], good[0]], (1, 4, 7), cb.S0, L, N)
    r = raw_batch(ctx, [good[0], good[1], good[0]], (1, 4, 7), cb.S0, L, N)
    assert r[0] == ba.EINVAL and untouched(r)
    for hm, tb in (([], ()), ([good[0]] * 65, (1,) * 65)):                                    # 0 and 65 models
        r = raw_batch(ctx, hm, tb, cb.S0, L, N)
        assert r[0] == ba.EINVAL and untouched(r), len(hm)
        with pytest.raises(ba.BathError, match="1 to 64 models"):
            ba.calibrate_fs_batch(ctx, hm, tb, cb.S0, L, N)
    for L_, N_ in ((1, N), (L, 1)):                                                           # L = 1: no codon pair; N = 1: nothing to fit
        r = raw_batch(ctx, good, (1, 4), cb.S0, L_, N_)
        assert r[0] == ba.EINVAL and untouched(r), (L_, N_)
    with pytest.raises(ba.BathError):
        ba.calibrate_fs_batch(ctx, good, (1, 4), cb.S0, L, N, tailp=1.0)
    with pytest.raises(ValueError):
        ba.calibrate_fs_batch(ctx, good, (1,), cb.S0, L, N)
    # the context is as usable as before: the same call, the same bits
    again = ba.calibrate_fs_batch(ctx, good, (1, 4), cb.S0, L, N, want_xv=True)
    assert again[2] == want[2] and all(np.array_equal(bits(again[i]), bits(want[i])) for i in (0, 1, 3, 4))


# ---- the command line
def run_convert(cwd, argv):
    """The command line in a fresh child process: (stdout, the output file's bytes)."""
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "bath_amd.bathconvert"] + argv, cwd=str(cwd),
                       env=dict(os.environ, PYTHONPATH=ba._ROOT), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    with open(argv[-2], "rb") as fh:
        return p.stdout, fh.read()


def summary(stdout):
    """stdout without the time line and the line that names the output file."""
    lines = stdout.splitlines()
    assert lines[-1].startswith("# CPU time:")
    return [ln for ln in lines[:-1] if not ln.startswith("# output HMM file:")]


@pytest.mark.parametrize("ct", [None, 4])
def test_cli_batch_writes_the_bytes_of_batch_1(tmp_path, ct):
    """--batch 5 on the 12-model file is batches of 5, 5 and 2; the file and the summary are those of --batch 1 and of no option."""
    pre = [] if ct is None else ["--ct", str(ct)]
    one, f1 = run_convert(tmp_path, pre + ["--batch", "1", str(tmp_path / "b1.bhmm"), cc.HMM_IN])
    five, f5 = run_convert(tmp_path, pre + ["--batch=5", str(tmp_path / "b5.bhmm"), cc.HMM_IN])
    assert f5 == f1 and summary(five) == summary(one)
    rows = [ln for ln in summary(five) if ln and not ln.startswith("#")]
    assert [int(r.split()[0]) for r in rows] == list(range(1, 13))
    assert [r[3] for r in cc.recorded(str(tmp_path / "b5.bhmm"))] == [ct or 1] * 12
    if ct is None:
        plain, f0 = run_convert(tmp_path, [str(tmp_path / "b0.bhmm"), cc.HMM_IN])
        assert f0 == f1 and summary(plain) == summary(one)


def test_cli_batch_passes_kept_taus_through(tmp_path):
    """A HMMER3 model, a converted BATH model (its taus are kept: no fit), another HMMER3 model: --batch 4 fits the first and the third
    in one call with the second between them in the output, as --batch 1 writes it."""
    h3 = bc.split_models(open(cc.HMM_IN, "rb").read().decode(bc.ENC))
    b3 = bc.split_models(open(cc.BHMM_OUT, "rb").read().decode(bc.ENC))
    src = tmp_path / "mixed.hmm"
    src.write_bytes((h3[0] + b3[1] + h3[2]).encode(bc.ENC))
    assert [bc.model_plan(m, None)["fit"] for m in bc.split_models(src.read_text(encoding=bc.ENC))] == [True, False, True]
    one, f1 = run_convert(tmp_path, ["--batch", "1", str(tmp_path / "m1.bhmm"), str(src)])
    four, f4 = run_convert(tmp_path, ["--batch", "4", str(tmp_path / "m4.bhmm"), str(src)])
    assert f4 == f1 and summary(four) == summary(one)
    got = bc.split_models(f4.decode(bc.ENC))
    assert len(got) == 3 and got[1] == b3[1]                                                 # the kept model: byte for byte


def test_cli_batch_failure_writes_no_file(tmp_path):
    """A failure in a batch: status 1, the error on stderr, no output file (as a failure does without --batch)."""
    long_path, _ = cb.model_file((1281, 3))
    text = open(long_path).read()
    src = tmp_path / "long.hmm"
    src.write_text(re.sub(r"^STATS LOCAL FS[35] FORWARD.*\n", "", text, flags=re.M))         # without its taus: it needs a fit
    out = tmp_path / "long.bhmm"
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "bath_amd.bathconvert", "--batch", "3", str(out), str(src)],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ba._ROOT), capture_output=True, text=True)
    assert p.returncode == 1 and "position 0" in p.stderr and "1281" in p.stderr and not out.exists()
