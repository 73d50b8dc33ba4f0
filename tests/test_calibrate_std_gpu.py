"""GPU tier of the standard-only calibration (bath_hip_calibrate_std, bath_hip_calibrate_std_batch; bath_amd.calibrate and
calibrate_batch with fs=False): lambda, the MSV and Viterbi mus and the Forward tau bit for bit those of the full calls, the two
frameshift taus unset, the generator where the three standard draws end, and no frameshift parser among the launches."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
import calib_batch_common as cb
from test_tiling_coverage_cpu import tiling

pytestmark = pytest.mark.gpu

E_NAMES = ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN")
SMALL_E = (30, 9, 25, 7, 10, 9)             # sets that are no multiple of a wave and differ from each other
EFT = 0.04
KW = dict(zip(E_NAMES, SMALL_E))
S0 = ba.rng_state(42)
STD_SPANS = {"calib_msv", "calib_vit", "calib_fwd"}
STD_BATCH = {"msv_wave_batch_kernel", "vit_wave_batch_kernel", "fwd_wave_batch_kernel"}
SPECS = ((8, 108), (65, 165), (300, 400), (8, 208))      # the batch: two models of one tiling, three tilings
CASCADE_MAX = 2048                                        # kCascadeMaxNodes


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: kernel_times also reports what the auxiliary contexts of a context that has run the
    pipeline still hold, and the tests below ask for the launches of one calibration call and nothing else."""
    c = ba.Context(0)
    yield c
    c.close()


def u32(ev):
    return np.asarray(ev, np.float32).view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def unset(ev):
    return (np.asarray(ev[6:8]) == np.float32(ba.FS_UNSET)).all()


@pytest.mark.parametrize("spec", SPECS[:3], ids=lambda s: "M%d" % s[0])
@pytest.mark.parametrize("resident", [True, False], ids=["samples", "drawn"])
def test_serial(ctx, spec, resident):
    sets = ba.CalibSamples(ctx, S0, *SMALL_E)
    try:
        after_std = sets.state_after
        full, std = cb.hmms((spec, spec))
        s_full, xv_full = ba.calibrate(ctx, full, 1, S0, sets if resident else None, Eft=EFT, want_xv=True, **KW)
        s_std, xv_std = ba.calibrate(ctx, std, 1, S0, sets if resident else None, Eft=EFT, want_xv=True, fs=False, **KW)
        kt = ba.kernel_times(ctx)
    finally:
        sets.close()
    assert np.array_equal(u32(std.evparam[:6]), u32(full.evparam[:6])), (std.evparam, full.evparam)
    assert unset(std.evparam) and not unset(full.evparam) and unset(std._p.contents.evparam[:])
    assert s_std == after_std and s_full != after_std
    assert sorted(xv_std) == ["fwd", "msv", "vit"] and all(np.array_equal(bits(xv_std[k]), bits(xv_full[k])) for k in xv_std)
    assert set(kt) == STD_SPANS and not any("fs" in name for name in kt), kt
    again = cb.hmms((spec,))[0]                                    # without xv: the same call
    assert ba.calibrate(ctx, again, 1, S0, None, Eft=EFT, fs=False, **KW) == after_std
    assert np.array_equal(u32(again.evparam), u32(std.evparam))


def test_batch_equals_the_serial_calls(ctx):
    sets = ba.CalibSamples(ctx, S0, *SMALL_E)
    try:
        serial = cb.hmms(SPECS)
        want = [ba.calibrate(ctx, h, 1, S0, sets, Eft=EFT, want_xv=True, fs=False, **KW) for h in serial]
        hmms = cb.hmms(SPECS)
        s1, xv = ba.calibrate_batch(ctx, hmms, 1, S0, sets, Eft=EFT, want_xv=True, fs=False, **KW)
        kt = ba.kernel_times(ctx)
        again = cb.hmms(SPECS)
        assert ba.calibrate_batch(ctx, again, 1, S0, sets, Eft=EFT, fs=False, **KW) == s1
        full = cb.hmms(SPECS)
        ba.calibrate_batch(ctx, full, 1, S0, sets, Eft=EFT, **KW)
        after_std = sets.state_after
    finally:
        sets.close()
    assert s1 == after_std and all(w[0] == after_std for w in want) and len(xv) == len(SPECS)
    for k, (h, w, (_, wxv)) in enumerate(zip(hmms, serial, want)):
        assert np.array_equal(u32(h.evparam), u32(w.evparam)) and unset(h.evparam), (k, h.M, h.evparam, w.evparam)
        assert np.array_equal(u32(again[k].evparam), u32(h.evparam)) and np.array_equal(u32(full[k].evparam[:6]), u32(h.evparam[:6]))
        assert sorted(xv[k]) == ["fwd", "msv", "vit"]
        for key in ("msv", "vit", "fwd"):
            assert np.array_equal(bits(xv[k][key]), bits(wxv[key])), (k, h.M, key)
    assert not np.array_equal(u32(hmms[0].evparam), u32(hmms[3].evparam))      # the two 8-node models differ
    wave = tiling("BATH_WAVE_COLUMNS")
    n_tilings = len({min(c for c in wave if 64 * c >= m) for m, _ in SPECS})
    assert n_tilings == 3 and set(kt) == STD_BATCH and all(kt[name][1] == n_tilings for name in STD_BATCH), kt


def raw_batch(ctx, hmms, state, sets):
    """The C call with an xv the test owns, filled with -7 before: (status, state afterwards, xv)."""
    st = C.c_uint32(state)
    ptrs = (C.POINTER(ba._Hmm) * len(hmms))(*[h._p for h in hmms])
    xv = np.full(len(hmms) * (SMALL_E[1] + SMALL_E[3] + SMALL_E[5]), -7.0)
    rc = ba.lib().bath_hip_calibrate_std_batch(ctx._h, ptrs, len(hmms), C.byref(st), sets._h, *SMALL_E, EFT, xv.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, st.value, xv


def test_failure_and_limits(ctx):
    """A model beyond the filter cascade's 2048 nodes fails the whole batch, named by its position, and nothing is changed; the
    frameshift kernels' 1280-node limit does not apply: a 1281-node model is calibrated, in the batch as alone."""
    sets = ba.CalibSamples(ctx, S0, *SMALL_E)
    try:
        good = cb.hmms(SPECS[:2])
        too_long = cb.hmms(((CASCADE_MAX + 1, 5),))[0]
        batch = [good[0], too_long, good[1]]
        before = [np.array(h._p.contents.evparam[:], np.float32) for h in batch]
        rc, state, xv = raw_batch(ctx, batch, S0, sets)
        now = [np.array(h._p.contents.evparam[:], np.float32) for h in batch]
        assert rc == ba.EINVAL and state == S0 and (xv == -7.0).all() and all(np.array_equal(u32(a), u32(b)) for a, b in zip(now, before))
        with pytest.raises(ba.BathError, match=r"position 1 .*2048 nodes \(this one has 2049\)"):
            ba.calibrate_batch(ctx, batch, 1, S0, sets, Eft=EFT, fs=False, **KW)
        with pytest.raises(ba.BathError, match="2048 nodes"):
            ba.calibrate(ctx, too_long, 1, S0, sets, Eft=EFT, fs=False, **KW)
        assert np.array_equal(u32(too_long._p.contents.evparam[:]), u32(before[1]))
        specs = (SPECS[0], (1281, 3))                                # beyond the frameshift kernels, within the cascade
        with pytest.raises(ba.BathError, match=r"position 1 .*1280 nodes \(this one has 1281\)"):
            ba.calibrate_batch(ctx, cb.hmms(specs), 1, S0, sets, Eft=EFT, **KW)
        serial, hmms = cb.hmms(specs), cb.hmms(specs)
        for h in serial:
            assert ba.calibrate(ctx, h, 1, S0, sets, Eft=EFT, fs=False, **KW) == sets.state_after
        assert ba.calibrate_batch(ctx, hmms, 1, S0, sets, Eft=EFT, fs=False, **KW) == sets.state_after
        for h, w in zip(hmms, serial):
            assert np.array_equal(u32(h.evparam), u32(w.evparam)) and unset(h.evparam) and (h.evparam[:6] != np.float32(ba.FS_UNSET)).all()
    finally:
        sets.close()
