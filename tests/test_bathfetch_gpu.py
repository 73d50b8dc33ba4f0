"""GPU tier of bathfetch: bath_hip_calibrate_fs_batch_at (the batch kernels fs3_fwd_batch_kernel and fs5_fwd_parser_batch_kernel with
a generator state per model, shared sample sets) against bath_amd.calibrate_fs model by model, bit for bit; and the command -- the
tutorial's fetch from the HMMER3 file, --ct 11 from the BATH file, and fetches through an index -- against bathconvert's output of
the same input byte for byte and against the reference's recorded files (tests/bathfetch_common.py) within the bars bathconvert's
own tests apply."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import bathfetch_common as fc
import calib_batch_common as cb
import calib_common as cc
import oracle_lib as ol
from bath_amd import bathconvert as bc
from bath_amd import bathfetch as bf

pytestmark = pytest.mark.gpu

KEYS = os.path.join(ol.GOLDEN, "tRNA-synthetases-key.txt")
STRICT_PIN = json.load(open(os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")))["models"]
SEL = fc.SEL                                      # the models the tutorial's key file names, by position in the 12-model file
TAU_LINES = ("STATS LOCAL FS3 FORWARD", "STATS LOCAL FS5 FORWARD")

# M = 1, 64, 65, 129 and 65 again: the tilings alternate (the launches group them), one length twice with other parameters
SPECS = tuple(s for s in cb.ORDER_SPECS if s[0] != 1280)
L, N = cb.SMALL_L, cb.SMALL_N


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def walk(n, tables):
    """n generator states, each two sample sets behind the one before."""
    out = [cb.S0]
    for t in list(tables)[:n - 1]:
        out.append(ba.calib_skip(out[-1], 2, L=L, N=N, ncbi_table=t))
    return out


def check_at(ctx, specs, tables, states):
    hmms = cb.hmms(specs)
    t3, t5, s1, x3, x5 = ba.calibrate_fs_batch_at(ctx, hmms, tables, states, L, N, want_xv=True)
    kt = ba.kernel_times(ctx)
    assert t3.shape == t5.shape == (len(specs),) and x3.shape == x5.shape == (len(specs), N) and len(s1) == len(specs)
    for k, (h, t, s) in enumerate(zip(hmms, tables, states)):
        w = ba.calibrate_fs(ctx, h, t, s, L, N, want_xv=True)
        assert (t3[k], t5[k], s1[k]) == (w[0], w[1], w[2]), (k, specs[k])
        assert np.array_equal(bits(x3[k]), bits(w[3])) and np.array_equal(bits(x5[k]), bits(w[4])), (k, specs[k])
    again = ba.calibrate_fs_batch_at(ctx, hmms, tables, states, L, N)                      # without xv: the same call
    assert np.array_equal(bits(again[0]), bits(t3)) and np.array_equal(bits(again[1]), bits(t5)) and again[2] == s1
    return kt


@pytest.mark.parametrize("case", ["distinct", "equal", "two_groups"])
def test_batch_at_equals_the_single_calls(gpu_ctx, case):
    n = len(SPECS)
    tables, states = {"distinct": ((1, 4, 1, 4, 4), None), "equal": ((1,) * n, [cb.S0] * n), "two_groups": ((1, 4, 1, 4, 1), [cb.S0] * n)}[case]
    states = states or walk(n, tables)
    assert len(set(zip(states, tables))) == {"distinct": n, "equal": 1, "two_groups": 2}[case]
    kt = check_at(gpu_ctx, SPECS, tables, states)
    fs = cb.fs_options()
    n_launch = len({min(c for c in fs if 64 * c >= m) for m, _ in SPECS})                     # the tilings present
    assert kt["fs3_fwd_batch_kernel"][1] == n_launch and kt["fs5_fwd_parser_batch_kernel"][1] == n_launch, kt
    assert "fs3_fwd_kernel" not in kt and "fs5_fwd_parser_kernel" not in kt, kt


def test_batch_at_of_one_model(gpu_ctx):
    check_at(gpu_ctx, cb.SINGLE_SPECS, cb.SINGLE_TABLES, [walk(3, (1, 1))[2]])


def test_a_refusal_names_the_position_and_writes_nothing(gpu_ctx):
    ctx = gpu_ctx
    good = cb.hmms(((64, 13), (65, 14)))
    long_ = cb.hmms(((1281, 3),))[0]
    want = ba.calibrate_fs_batch_at(ctx, good, (1, 4), [cb.S0, cb.S0], L, N, want_xv=True)
    hmms = [good[0], long_, good[1]]
    with pytest.raises(ba.BathError, match=r"position 1 .*1280 nodes \(this one has 1281\)"):
        ba.calibrate_fs_batch_at(ctx, hmms, (1, 1, 4), [cb.S0] * 3, L, N)
    # the C call with outputs the test owns
    ptrs = (C.POINTER(ba._Hmm) * 3)(*[h._p for h in hmms])
    tabs, s_in, s_out = np.array([1, 1, 4], np.int32), np.full(3, cb.S0, np.uint32), np.full(3, 77, np.uint32)
    arrs = [np.full(3, -7.0), np.full(3, -7.0), np.full(3 * N, -7.0), np.full(3 * N, -7.0)]
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    call = lambda n, L_, N_: ba.lib().bath_hip_calibrate_fs_batch_at(ctx._h, ptrs, tabs.ctypes.data_as(C.POINTER(C.c_int)), n, s_in.ctypes.data_as(u32p),
                                                                     s_out.ctypes.data_as(u32p), L_, N_, 0.04, *[a.ctypes.data_as(f64p) for a in arrs])
    for n, L_, N_ in ((3, L, N), (0, L, N), (65, L, N), (1, 1, N), (1, L, 1)):                # the long model; 0 and 65 models; L = 1; N = 1
        assert call(n, L_, N_) == ba.EINVAL, (n, L_, N_)
        assert (s_out == 77).all() and all((a == -7.0).all() for a in arrs), (n, L_, N_)
    with pytest.raises(ba.BathError, match=r"position 2 .*translation table 7"):
        ba.calibrate_fs_batch_at(ctx, [good[0], good[1], good[0]], (1, 4, 7), [cb.S0] * 3, L, N)
    with pytest.raises(ba.BathError, match="1 to 64 models"):
        ba.calibrate_fs_batch_at(ctx, [good[0]] * 65, (1,) * 65, [cb.S0] * 65, L, N)
    with pytest.raises(ValueError):
        ba.calibrate_fs_batch_at(ctx, good, (1, 4), [cb.S0], L, N)
    again = ba.calibrate_fs_batch_at(ctx, good, (1, 4), [cb.S0, cb.S0], L, N, want_xv=True)  # the context is as usable as before
    assert again[2] == want[2] and all(np.array_equal(bits(again[i]), bits(want[i])) for i in (0, 1, 3, 4))


# ---- the command
def read(path):
    with open(path, "rb") as fh:
        return fh.read().decode(bc.ENC)


def convert(tmp, argv, src):
    """bathconvert's output of <src> as its models' texts."""
    out = str(tmp / ("conv%d.bhmm" % len(os.listdir(tmp))))
    assert bc.run(argv + [out, src], stdout=io.StringIO()) == 0
    return bc.split_models(read(out))


def fetched(tmp, argv, stats=None):
    out = str(tmp / ("fetch%d.bhmm" % len(os.listdir(tmp))))
    text = io.StringIO()
    assert bf.run(argv[:-2] + ["-o", out] + argv[-2:], stdout=text, stats=stats) == 0
    return bc.split_models(read(out)), text.getvalue()


def without_maxl(model):
    return "".join(ln for ln in model.splitlines(keepends=True) if not ln.startswith("MAXL "))


def taus_of(model):
    return [float(ln.split()[-2]) for ln in model.splitlines() if ln.startswith(TAU_LINES)]


def outside_the_taus(model):
    return [ln if not ln.startswith(TAU_LINES) else ln[:len(TAU_LINES[0])] + ln[len(TAU_LINES[0]) + 9:] for ln in model.splitlines(keepends=True)]


def check_against_recorded(got, recorded, arith):
    """Every byte outside the tau fields is the recorded file's; each tau within the bar bathconvert's tests hold that arithmetic to
    against the recorded conversion: strict, 4 standard deviations of that tau over the pin's reseeded runs (test_bathconvert_cpu);
    odds, closer to the record than the strict path's measured difference (test_arith_gpu)."""
    assert len(got) == len(recorded) == len(SEL)
    for g, r, i in zip(got, recorded, SEL):
        assert outside_the_taus(g) == outside_the_taus(r), STRICT_PIN[i]["name"]
        for key, tau, want in zip(("fs3", "fs5"), taus_of(g), taus_of(r)):
            d = tau - want
            print("%-14s %s %-6s recorded %8.4f here %8.4f diff %+.1e" % (STRICT_PIN[i]["name"], key, arith, want, tau, d))
            assert want == STRICT_PIN[i][key]["recorded"]
            if arith == "strict":
                assert abs(d) <= 4.0 * STRICT_PIN[i][key]["reseeded_sd"], (i, key, d)
            else:
                assert abs(d) < abs(STRICT_PIN[i][key]["diff"]), (i, key, d)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("bathfetch")


@pytest.fixture(scope="module")
def converted(work):
    """bathconvert --batch 16 of the HMMER3 input: the road the selected models' blocks are defined by."""
    return convert(work, ["--batch", "16"], cc.HMM_IN)


def test_the_tutorial_command(work, converted):
    """bathfetch -f -o out tRNA-proteins.hmm tRNA-synthetases-key.txt without an index."""
    want = [without_maxl(converted[i]) for i in SEL]
    stats = {}
    got, text = fetched(work, ["-f", cc.HMM_IN, KEYS], stats)
    assert got == want and text == "\nRetrieved 3 HMMs.\n"                                   # (a)
    assert stats["fitted"] == 3 and stats["skipped"] == 9                                    # (b): three models scored, not twelve
    for batch in ("1", "2"):                                                                 # (a): more models than --batch
        stats = {}
        assert fetched(work, ["--batch", batch, "-f", cc.HMM_IN, KEYS], stats)[0] == want and stats["fitted"] == 3, batch
    check_against_recorded(got, fc.recorded_fetch(), "strict")                  # (c)
    one, text = fetched(work, [cc.HMM_IN, "PF03950.13"])                                     # the single-key form walks the same generator
    assert one == [want[1]] and text == "\n\nRetrieved HMM PF03950.13.\n"


def test_the_tutorial_command_in_odds_arithmetic(work):
    conv = convert(work, ["--arith", "odds"], cc.HMM_IN)
    stats = {}
    got, _ = fetched(work, ["--arith", "odds", "-f", cc.HMM_IN, KEYS], stats)
    assert got == [without_maxl(conv[i]) for i in SEL]                                       # (d)
    assert stats["fitted"] == 10 and stats["skipped"] == 0                                   # the redraw feeds the generator: every model up to the last selected
    check_against_recorded(got, fc.recorded_fetch(), "odds")                    # (c)


def test_ct_11_from_the_bath_file(work):
    """Every model of the BATH file carries table 1: --ct 11 refits each, so the walk is the file's.  MAXL is in the input and stays.
    (A copy of the file: beside the fixture lies the recorded index, and this fetch is the one without.)"""
    src = str(work / "tRNA-proteins.bhmm")
    with open(src, "wb") as fh:
        fh.write(open(cc.BHMM_OUT, "rb").read())
    conv = convert(work, ["--ct", "11", "--batch", "16"], src)
    stats = {}
    got, _ = fetched(work, ["--ct", "11", "-f", src, KEYS], stats)
    assert got == [conv[i] for i in SEL] and stats["fitted"] == 3 and stats["skipped"] == 9
    assert all("\nCODON TABLE  11\n" in m and "\nMAXL  " in m for m in got)
    check_against_recorded(got, [fc.recorded_ct11()[i] for i in SEL], "strict")


def test_with_an_index(gpu_ctx, work):
    """Every key starts from a fresh generator: each model's taus are calibrate_fs from the seed state; the order is the key file's."""
    src = work / "indexed.hmm"
    src.write_bytes(open(cc.HMM_IN, "rb").read())
    assert bf.run(["--index", str(src)], stdout=io.StringIO()) == 0
    keys = work / "keys.txt"
    keys.write_text("tRNA-synt_2d\nPF04376.8\ntRNA-synt_1_2\n")
    order = (9, 0, 7)
    stats = {}
    got, text = fetched(work, ["-f", str(src), str(keys)], stats)
    assert text == "\nRetrieved 3 HMMs.\n" and stats["fitted"] == 3 and stats["skipped"] == 0
    blocks = bc.split_models(read(cc.HMM_IN))
    for g, i in zip(got, order):
        t3, t5, _ = ba.calibrate_fs(gpu_ctx, ba.HMM(cc.HMM_IN, i), 1, ba.rng_state())
        assert g == bc.rewrite_model(blocks[i], 1, t3, t5, add_maxl=False), i
    one, _ = fetched(work, [str(src), "PF13603.1"])                                          # tRNA-synt_1_2 by its accession
    assert one == [got[2]]
    assert fetched(work, ["--batch", "1", "-f", str(src), str(keys)])[0] == got
