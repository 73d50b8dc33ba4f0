"""GPU tier of bathconvert: the score-only 5-codon Forward parser (fs5_fwd_chain_kernel<C, 256, false>) at every per-lane tiling,
bath_hip_calibrate_fs against the CPU path of tests/calib_common.py, the command line on the 12-model fixture, and a search with the
converted file."""
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
from bath_amd import synth

pytestmark = pytest.mark.gpu

FS_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16, 20]                      # BATH_FS_COLUMNS (bath_tilings.hpp), held equal below
# per entry its largest M, and the smallest M of the next entry; plus M = 1 and M = 2
PARSER_M = sorted({1, 2} | {64 * c for c in FS_COLUMNS} | {64 * c + 1 for c in FS_COLUMNS[:-1]})
LENGTHS = [0, 4, 5, 6, 299, 300, 301]
PIN_JSON = os.path.join(ba._ROOT, "profiles", "bathconvert_vs_recorded.json")


def identical(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_parser_lengths_cover_the_tiling_list():
    from test_tiling_coverage_cpu import fs_options, lengths_per_column
    fs = fs_options()
    assert FS_COLUMNS == fs
    assert all(lo in PARSER_M and hi in PARSER_M for _, lo, hi in lengths_per_column(fs))
    assert "fs5_fwd_chain_kernel<CC, 256, false>" in open(ba._ROOT + "/bath_amd/csrc/bath_fs_chain.hip").read()


def oracle_fs5(model, wins):
    """bo_gforward_fs on the multihit length-100 profile; a window too short for the recursion (L < 5) has no path: -inf."""
    L_ = ol.lib()
    gm5 = model.fs(5, 100)
    f = C.c_float()
    out = np.zeros(len(wins), np.float32)
    for e, w in enumerate(wins):
        L = len(w)
        if L < 5:
            out[e] = -np.inf
            continue
        g8 = L_.bo_gmx_create(model.M, L + 1, L, 8)
        assert L_.bo_gforward_fs(ol.u8(ol.dsq_from(w)), L, gm5, g8, 0, C.byref(f)) == 0
        L_.bo_gmx_free(g8)
        out[e] = f.value
    return out


@pytest.mark.parametrize("M", PARSER_M)
def test_parser_is_bit_identical_to_the_full_forward(gpu_ctx, tmp_path, M):
    """bath_hip_fs5_forward_parser against bo_gforward_fs (strict, the library's default), one launch of 0, 4, 5, 6, 299, 300 and 301 nt
    (one window with N codes) as a block of 1 window and as a block of 201; 0 and 4 nt score -inf."""
    ctx = gpu_ctx
    path = synth.write_synthetic_bhmm(str(tmp_path / "s.bhmm"), M, seed=M)
    hmm = ba.HMM(path)
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, 100))
    model = ol.Model(path)
    rng = np.random.default_rng(M)
    distinct = [rng.integers(0, 4, n).astype(np.uint8) for n in LENGTHS]
    distinct[4][[7, 8, 150]] = 15                                 # N
    distinct += [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(5, 302, 5)]
    want = oracle_fs5(model, distinct)
    assert np.isneginf(want[:2]).all() and np.isfinite(want[2:]).all()
    pick = list(range(len(LENGTHS))) + [int(v) for v in rng.integers(0, len(distinct), 201 - len(LENGTHS))]
    got = ba.FS5ForwardParser(ctx, om5, ba.SeqBlock(ctx, [distinct[p] for p in pick]), 100)
    assert len(got) == 201 and identical(got, want[pick]), (M, got[:7], want[:7])
    for p in (5, 0, 1):                                           # blocks of one window: 300 nt, and the two without a path
        one = ba.FS5ForwardParser(ctx, om5, ba.SeqBlock(ctx, [distinct[p]]), 100)
        assert identical(one, want[p:p + 1]), (M, p)
    full, _, _ = ba.FS5ForwardFull(ctx, om5, ba.SeqBlock(ctx, distinct[2:6]), 100)        # ... and the kernel it is an instantiation of
    assert identical(full, want[2:6])


def test_parser_ignores_the_arithmetic_switches(gpu_ctx, tmp_path):
    """The header's promise: strict arithmetic whatever set_fs_strict / set_fs5_odds say."""
    ctx = gpu_ctx
    hmm = ba.HMM(os.path.join(ol.GOLDEN, "PTH2.bhmm"))
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, 100))
    rng = np.random.default_rng(3)
    blk = ba.SeqBlock(ctx, [rng.integers(0, 4, 300).astype(np.uint8) for _ in range(5)])
    base = ba.FS5ForwardParser(ctx, om5, blk, 100)
    try:
        ctx.set_fs_strict(False); ctx.set_fs5_odds(True)
        assert identical(ba.FS5ForwardParser(ctx, om5, blk, 100), base)
    finally:
        ctx.set_fs5_odds(False); ctx.set_fs_strict(True)
    om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, 100))
    with pytest.raises(ba.BathError):
        ba.FS5ForwardParser(ctx, om3, blk, 100)


def check_calibrate(ctx, path, index, L, N):
    hmm = ba.HMM(path, index)
    s0 = ba.rng_state(42)
    t3, t5, s1, x3, x5 = ba.calibrate_fs(ctx, hmm, 1, s0, L, N, want_xv=True)
    w3, w5, ws, wx3, wx5 = cc.oracle_model(path, index, 1, s0, L, N)
    assert np.array_equal(x3.view(np.uint64), wx3.view(np.uint64)) and np.array_equal(x5.view(np.uint64), wx5.view(np.uint64))
    assert abs(t3 - w3) <= 1e-6 and abs(t5 - w5) <= 1e-6
    _, s = ba.calib_sample(s0, L, N, 1)
    _, s = ba.calib_sample(s, L, N, 1)
    assert s1 == ws == s
    assert ba.calibrate_fs(ctx, hmm, 1, s0, L, N) == (t3, t5, s1)
    return t3, t5


def test_calibrate_equals_the_cpu_path(gpu_ctx, tmp_path):
    """ATE_N (M = 78) and a synthetic model at a tiling boundary (M = 129: the first of three nodes per lane): the bit scores equal
    the oracle-scored ones bit for bit, the taus agree to 1e-6, the generator ends where the sampler's does."""
    t3, t5 = check_calibrate(gpu_ctx, cc.HMM_IN, 0, 100, 200)
    pin = json.load(open(PIN_JSON))["models"][0]
    assert abs(t3 - pin["fs3"]["cpu_path"]) <= 1e-6 and abs(t5 - pin["fs5"]["cpu_path"]) <= 1e-6
    check_calibrate(gpu_ctx, cc.HMM_IN, 0, 10, 8)
    check_calibrate(gpu_ctx, synth.write_synthetic_bhmm(str(tmp_path / "s129.bhmm"), 129, seed=5), 0, 100, 200)


def test_calibrate_refuses_by_name(gpu_ctx):
    hmm = ba.HMM(cc.HMM_IN, 0)
    for kw in (dict(ncbi_table=7), dict(L=1), dict(N=1), dict(tailp=0.0)):
        a = dict(ncbi_table=1, L=100, N=200, tailp=0.04); a.update(kw)
        with pytest.raises(ba.BathError):
            ba.calibrate_fs(gpu_ctx, hmm, a["ncbi_table"], ba.rng_state(42), a["L"], a["N"], a["tailp"])


def run_convert(cwd, argv):
    """The command line in a fresh child process."""
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "bath_amd.bathconvert"] + argv, cwd=str(cwd),
                       env=dict(os.environ, PYTHONPATH=ba._ROOT), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.fixture(scope="module")
def converted(tmp_path_factory):
    d = tmp_path_factory.mktemp("bathconvert")
    out = str(d / "tRNA-proteins.bhmm")
    return out, run_convert(d, [out, cc.HMM_IN])


def read(path):
    with open(path, "rb") as fh:
        return fh.read().decode("latin-1")


def test_cli_converts_the_twelve_model_file(converted):
    """Outcome B of the pin (tests/test_bathconvert_cpu.py): the output is, byte for byte, the rewrite fed with the CPU path's 24
    taus (stored in profiles/bathconvert_vs_recorded.json, which the CPU tier holds against that path); the summary lists 12 models."""
    out, text = converted
    pin = json.load(open(PIN_JSON))["models"]
    rec = cc.recorded(cc.BHMM_OUT)
    want = bc.rewrite(read(cc.HMM_IN), [(m["fs3"]["cpu_path"], m["fs5"]["cpu_path"]) for m in pin], [r[0] for r in rec])
    assert read(out) == want
    lines = text.splitlines()
    assert text.startswith(bc.BANNER) and lines[-1].startswith("# CPU time:") and " Elapsed: " in lines[-1]
    rows = [ln for ln in lines if ln and not ln.startswith("#")]
    assert [int(r.split()[0]) for r in rows] == list(range(1, 13))
    assert [r.split()[1] for r in rows] == [m["name"] for m in pin]
    assert rows[0] == "  1      ATE_N                   30    78         1     1.11  0.726 Arginine-tRNA-protein transferase, N terminus"


def test_cli_ct(tmp_path):
    """--ct 11 on a table-1 file: CODON TABLE 11 and the taus of the CPU path with table 11; --ct 1: the taus stay."""
    src = os.path.join(ol.GOLDEN, "PTH2.bhmm")
    out11, out1 = str(tmp_path / "ct11.bhmm"), str(tmp_path / "ct1.bhmm")
    run_convert(tmp_path, ["--ct", "11", out11, src])
    w3, w5 = cc.oracle_file(src, 11)[0][:2]
    assert read(out11) == bc.rewrite(read(src), [(w3, w5)], None, ct_opt=11)
    assert cc.recorded(out11)[0][3] == 11 and "\nCODON TABLE  11\n" in read(out11)
    run_convert(tmp_path, ["--ct", "1", out1, src])
    assert read(out1) == read(src)


def tbl_rows(path):
    text = open(path).read()
    return text[:text.index("#\n# Program:")].split("\n")          # up to the trailer: program, files, options, directory, date


def test_search_with_the_converted_file(converted, tmp_path):
    """bathsearch --fs with the converted file against the recorded target: the --tblout of the same search with the golden file."""
    from bath_amd import bathsearch as bs
    out, _ = converted
    target = os.path.join(ol.GOLDEN, "target-PTH2.fa")
    a, b = str(tmp_path / "a.tbl"), str(tmp_path / "b.tbl")
    null = open(os.devnull, "w")
    assert bs.run(["--fs", "--tblout", a, out, target], stdout=null) == 0
    assert bs.run(["--fs", "--tblout", b, cc.BHMM_OUT, target], stdout=null) == 0
    assert tbl_rows(a) == tbl_rows(b)
    assert any(not ln.startswith("#") and ln.strip() for ln in tbl_rows(a))            # there are hits to compare
