"""GPU tier of bathbuild --batch: bath_hip_calibrate_batch (msv_wave_batch_kernel, vit_wave_batch_kernel, fwd_wave_batch_kernel: one
standard sample set against several models per launch; the two frameshift batch kernels on one shared pair of sets) at every wave
tiling, in mixed order and at the full shape, against the serial bath_amd.calibrate loop from the same state bit for bit and against
the CPU path of tests/bathbuild_common.py; its refusals; and the tool, whose output with --batch N is the bytes of --batch 1."""
import ctypes as C
import io

import numpy as np
import pytest

import bath_amd as ba
import bathbuild_common as bc
import calib_batch_common as cb
from bath_amd import bathbuild as bb
from test_tiling_coverage_cpu import lengths_per_column, tiling

pytestmark = pytest.mark.gpu

E_NAMES = ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN")
SMALL_E = (30, 9, 25, 7, 10, 9)             # sets that are no multiple of a wave and differ from each other
EFT = 0.04
KEYS = ("msv", "vit", "fwd", "fs3", "fs5")
FS_MAX = 1280                               # kFsMaxNodes: the frameshift kernels' limit bounds a calibration
NEW_KERNELS = ("msv_wave_batch_kernel", "vit_wave_batch_kernel", "fwd_wave_batch_kernel", "fs3_fwd_batch_kernel", "fs5_fwd_parser_batch_kernel")
SINGLE_SPANS = ("calib_msv", "calib_vit", "calib_fwd", "fs3_fwd_kernel", "fs5_fwd_parser_kernel")
S0 = ba.rng_state(42)


def wave_tilings():
    """(C, smallest M, largest M capped at 1280) of every entry of BATH_WAVE_COLUMNS a calibration can reach."""
    return [(c, lo, min(hi, FS_MAX)) for c, lo, hi in lengths_per_column(tiling("BATH_WAVE_COLUMNS")) if lo <= FS_MAX]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def null1(L):
    """p7_bg_SetLength + p7_bg_NullOne."""
    p1 = np.float32(L) / np.float32(L + 1)
    return np.float32(np.float32(L) * np.log(np.float64(p1)) + np.log(1.0 - np.float64(p1)))


def check_batch(ctx, make_models, E, ct=1, n_oracle=0):
    """One batch against the serial calibrate loop from the same state and the same CalibSamples (every model), and against the CPU
    path (the first n_oracle models).  make_models() gives fresh, uncalibrated-or-not models; returns the batch's models and xv."""
    kw = dict(zip(E_NAMES, E))
    sets = ba.CalibSamples(ctx, S0, *E)
    try:
        serial = make_models()
        want = [ba.calibrate(ctx, h, ct, S0, sets, Eft=EFT, want_xv=True, **kw) for h in serial]
        assert len({w[0] for w in want}) == 1                        # every serial call leaves the same state
        hmms = make_models()
        s1, xv = ba.calibrate_batch(ctx, hmms, ct, S0, sets, Eft=EFT, want_xv=True, **kw)
        kt = ba.kernel_times(ctx)                                    # the spans of the batch call
        assert s1 == want[0][0] and len(xv) == len(hmms)
        for k, (h, w, (_, wxv)) in enumerate(zip(hmms, serial, want)):
            assert np.array_equal(h.evparam.view(np.uint32), w.evparam.view(np.uint32)), (k, h.M, h.evparam, w.evparam)
            for key in KEYS:
                assert np.array_equal(bits(xv[k][key]), bits(wxv[key])), (k, h.M, key)
        again = make_models()
        assert ba.calibrate_batch(ctx, again, ct, S0, sets, Eft=EFT, **kw) == s1          # without xv: the same call
        assert all(np.array_equal(a.evparam.view(np.uint32), h.evparam.view(np.uint32)) for a, h in zip(again, hmms))
    finally:
        sets.close()
    for k, h in enumerate(make_models()[:n_oracle]):
        s_cpu, oxv = bc.oracle_calibrate(h, S0, tuple(E) + (EFT,), ct)
        assert s_cpu == s1
        for key in ("msv", "vit", "fs3", "fs5"):
            assert np.array_equal(bits(xv[k][key]), bits(oxv[key])), (k, h.M, key)
        d = np.abs(xv[k]["fwd"] - oxv["fwd"])                       # the bar tests/test_bathbuild_gpu.py holds the Forward bit scores to
        bar = (2e-4 + 1e-4 * np.abs(oxv["fwd"] * bc.LN2 + null1(E[4]))) / bc.LN2
        print("M %d: fwd xv worst dev %.3e bits (bar %.3e)" % (h.M, d.max(), bar.min()))
        assert np.all(d <= bar), (k, h.M, d.max())
        assert hmms[k].evparam[0] == h.evparam[0] and hmms[k].evparam[2] == h.evparam[2]
    return hmms, xv, kt


@pytest.mark.parametrize("case", wave_tilings(), ids=lambda c: "C%d" % c[0])
def test_every_tiling(gpu_ctx, case):
    """Per entry of BATH_WAVE_COLUMNS one batch of its smallest and its largest model: two models in one launch of each filter."""
    c, lo, hi = case
    specs = ((lo, 100 + lo), (hi, 100 + hi))
    first_two = [t[0] for t in wave_tilings()[:2]]
    _, _, kt = check_batch(gpu_ctx, lambda: cb.hmms(specs), SMALL_E, n_oracle=2 if c in first_two else 0)
    fs = cb.fs_options()
    n_fs = len({min(f for f in fs if 64 * f >= m) for m, _ in specs})              # the frameshift tilings of the two models
    for name in NEW_KERNELS:
        assert kt[name][1] == (n_fs if name.startswith("fs") else 1), (c, name, kt)
    assert not any(name in kt for name in SINGLE_SPANS), (c, kt)


def test_results_stand_in_input_order(gpu_ctx):
    """M = 1, 1280, 64, 65, 129, 65: the tilings alternate (the launches group them) and one length comes twice with other
    parameters; and a batch of one model."""
    hmms, xv, kt = check_batch(gpu_ctx, lambda: cb.hmms(cb.ORDER_SPECS), SMALL_E)
    assert [h.M for h in hmms] == [m for m, _ in cb.ORDER_SPECS]
    assert not np.array_equal(bits(xv[3]["fwd"]), bits(xv[5]["fwd"])) and not np.array_equal(hmms[3].evparam, hmms[5].evparam)
    wave = tiling("BATH_WAVE_COLUMNS")
    n_launch = len({min(c for c in wave if 64 * c >= m) for m, _ in cb.ORDER_SPECS})   # the wave tilings present: four
    assert n_launch == 4 and all(kt[name][1] == n_launch for name in NEW_KERNELS[:3]), kt
    hmms, _, kt = check_batch(gpu_ctx, lambda: cb.hmms(cb.SINGLE_SPECS), SMALL_E, ct=4)
    assert len(hmms) == 1 and all(kt[name][1] == 1 for name in NEW_KERNELS), kt


def test_full_shape(gpu_ctx, tmp_path):
    """What bathbuild runs: the three models of three_seqs.fa (429, 245 and 358 nodes) at the default sizes, batch against serial;
    and the tool, whose model file and stdout with --batch 2 (batches of 2 and 1) and --batch 64 (one batch) are those of --batch 1."""
    hmms, _, _ = check_batch(gpu_ctx, lambda: [bc.fresh_model("three_seqs", i) for i in range(3)], bc.DEFAULT_E[:6])
    assert [h.M for h in hmms] == [429, 245, 358]
    fa, out = bc.golden("three_seqs.fa"), {}
    for nb in ("1", "2", "64"):
        path, log = str(tmp_path / ("b%s.bhmm" % nb)), io.StringIO()
        assert bb.run(["--batch", nb, path, fa], stdout=log, date="D") == 0
        out[nb] = (open(path, "rb").read(), [ln for ln in log.getvalue().splitlines() if not ln.startswith("# CPU time:") and path not in ln])
    assert out["2"] == out["1"] and out["64"] == out["1"]
    assert out["1"][0].count(b"STATS LOCAL FS5 FORWARD") == 3 and len([ln for ln in out["1"][1] if ln.startswith("  ")]) == 3


def raw_batch(ctx, hmms, ct, state, sets, E, n=None):
    """The C call with an xv the test owns, filled with -7 before: (status, state afterwards, xv)."""
    n = len(hmms) if n is None else n
    st = C.c_uint32(state)
    ptrs = (C.POINTER(ba._Hmm) * max(len(hmms), 1))(*[h._p for h in hmms])
    xv = np.full(max(n, 1) * (E[1] + E[3] + 3 * E[5]), -7.0)
    rc = ba.lib().bath_hip_calibrate_batch(ctx._h, ptrs, n, ct, C.byref(st), sets._h, *E, EFT, xv.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, st.value, xv


def test_refusals_leave_everything_as_it_was(gpu_ctx):
    ctx, E = gpu_ctx, SMALL_E
    kw = dict(zip(E_NAMES, E))
    good_specs = ((64, 13), (65, 14))
    sets = ba.CalibSamples(ctx, S0, *E)
    other = ba.CalibSamples(ctx, sets.state_after, *E)                                # drawn from another state
    try:
        want = cb.hmms(good_specs)
        s1, wxv = ba.calibrate_batch(ctx, want, 1, S0, sets, Eft=EFT, want_xv=True, **kw)
        good = cb.hmms(good_specs)
        long_ = cb.hmms(((1281, 3),))[0]
        before = [np.array(h._p.contents.evparam[:], np.float32) for h in good + [long_]]

        def untouched(r):
            now = [np.array(h._p.contents.evparam[:], np.float32) for h in good + [long_]]
            return r[0] == ba.EINVAL and r[1] == S0 and (r[2] == -7.0).all() and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(now, before))

        assert untouched(raw_batch(ctx, [good[0], long_, good[1]], 1, S0, sets, E))   # a model beyond the frameshift kernels' 1280 nodes
        with pytest.raises(ba.BathError, match=r"position 1 .*1280 nodes \(this one has 1281\)"):
            ba.calibrate_batch(ctx, [good[0], long_, good[1]], 1, S0, sets, Eft=EFT, **kw)
        assert untouched(raw_batch(ctx, good, 1, S0, sets, E, n=0))                   # 0 and 65 models
        assert untouched(raw_batch(ctx, [good[0]] * 65, 1, S0, sets, E))
        for hm in ([], [good[0]] * 65):
            with pytest.raises(ba.BathError, match="1 to 64 models"):
                ba.calibrate_batch(ctx, hm, 1, S0, sets, Eft=EFT, **kw)
        assert untouched(raw_batch(ctx, good, 1, S0, other, E))                       # samples drawn from another state
        assert untouched(raw_batch(ctx, good, 7, S0, sets, E))                        # an unknown table
        with pytest.raises(ba.BathError, match="sample sets"):
            ba.calibrate_batch(ctx, good, 1, S0, None, Eft=EFT, **kw)
        # the context is as usable as before: the good call, the good result
        s2, xv = ba.calibrate_batch(ctx, good, 1, S0, sets, Eft=EFT, want_xv=True, **kw)
        assert s2 == s1 and all(np.array_equal(g.evparam.view(np.uint32), w.evparam.view(np.uint32)) for g, w in zip(good, want))
        assert all(np.array_equal(bits(xv[k][key]), bits(wxv[k][key])) for k in range(2) for key in KEYS)
    finally:
        other.close()
        sets.close()
