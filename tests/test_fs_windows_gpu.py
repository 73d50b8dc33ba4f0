"""The DNA-window kernels of the frameshift stage (bath_fs_windows.hip: merge, counting rank, scatter, slot, the two hit-window passes,
per-ORF window, group rank, fuse, scan, summary, layout, decide) and the host build that takes the blocks they hand back, on blocks of
thousands of surviving ORFs, through bath_selftest_fs_windows / bath_selftest_fs_decide.

Every case of tests/fs_windows_inputs.py (tests/test_fs_windows_cpu.py shows that each reaches what it names) goes through both drivers
and is held to the oracle's bo_fs_build_windows, run (sequence, strand) by (sequence, strand): ordered ORFs, windows, summaries and group
bounds equal, tot_orfsc and P_min bitwise (same table, same order), P_tot bitwise from the host build (libm on both sides, the same
expression) and within 2 ulp of a double from the kernels (one ulp of documented error for either library's exp); pool offsets, lengths and
totals recomputed in numpy from the window lengths.  The lists go to the device driver shuffled, as the select kernels leave them, under
two shuffles whose results must be identical.  A block the kernels do not take comes back as BATH_ENORESULT without an error, the host
driver builds it, and the next accepted block on the same context is right."""
import numpy as np
import pytest

import bath_amd as ba
import fs_windows_inputs as I
import oracle_lib as ol

pytestmark = pytest.mark.gpu

_worst = {"P_tot": 0, "P_fs": 0, "P_null": 0}          # ulps, over the device driver's runs of this session


@pytest.fixture(scope="module")
def models(gpu_ctx):
    out = {}
    for key in ("pth2", "m12"):
        path, m = I.model(key)
        hmm = ba.HMM(path, 0)
        out[key] = (ba.OProfile(gpu_ctx, ba.Profile(hmm)), ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct)))
    return out


_blocks = {}


def block(ctx, c):
    if c.name not in _blocks:
        _blocks.clear()                                   # one case's sequences on the device at a time
        _blocks[c.name] = ba.SeqBlock(ctx, c.seqs)
    return _blocks[c.name]


def ulps(a, b):
    """Distance in representable doubles (same sign, finite)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def check_build(c, got, driver, dna_off):
    E, W = c.orfs, c.windows
    assert (got["n_orfs"], got["nw"]) == (c.n, c.nw)
    o = got["orfs"]
    for f in ("w", "strand", "start", "end", "n", "cand", "aa_off", "g0", "g1", "dw_n", "dw_len", "dw_k", "kmin", "kmax"):
        assert np.array_equal(o[f], E[f]), (c.name, driver, f, np.flatnonzero(o[f] != E[f])[:8])
    assert np.array_equal(o["we"] > o["wb"], c.found), (c.name, driver, "hit window found")
    assert np.array_equal(o["P"].view(np.uint64), E["P"].view(np.uint64)) and np.array_equal(o["fwd_null"].view(np.uint32), E["fwd_null"].view(np.uint32))
    w = got["windows"]
    for f in ("window", "strand", "n", "length", "orf_cnt", "k_min", "k_max"):
        assert np.array_equal(w[f], W[f]), (c.name, driver, f, np.flatnonzero(w[f] != W[f])[:8])
    assert np.array_equal(got["grp"], c.grp), (c.name, driver, "grp")
    assert np.array_equal(w["tot_orfsc"].view(np.uint32), W["tot_orfsc"].view(np.uint32)), (c.name, driver, "tot_orfsc")
    assert np.array_equal(w["P_min"].view(np.uint64), W["P_min"].view(np.uint64)), (c.name, driver, "P_min")
    d = ulps(w["P_tot"], W["P_tot"])
    if driver == 1:
        assert d.max(initial=0) == 0, (c.name, "P_tot, host build", int(d.max()))
    else:
        _worst["P_tot"] = max(_worst["P_tot"], int(d.max(initial=0)))
        print("%s: device P_tot within %d ulp of the oracle's" % (c.name, int(d.max(initial=0))))
        assert d.max(initial=0) <= 2, (c.name, "P_tot, kernels", int(d.max()))
    # ---- the layout, from the lengths alone
    pitch = I.pool_pitch(W["length"])
    voff = np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.int64)
    assert np.array_equal(got["voff"], voff) and np.array_equal(got["vlen"], W["length"])
    assert (got["maxlen"], got["pool_bytes"], got["total"]) == (int(W["length"].max()), int(pitch.sum()), int(W["length"].astype(np.int64).sum()))
    desc = got["desc"]
    n_seq = np.array([len(s) for s in c.seqs], np.int64)
    assert np.array_equal(desc["dst_off"], voff) and np.array_equal(desc["src_off"], dna_off[W["window"]])
    for f, want in (("seq_n", n_seq[W["window"]]), ("start", W["n"]), ("len", W["length"]), ("strand", W["strand"]), ("kmin", W["k_min"]), ("kmax", W["k_max"])):
        assert np.array_equal(desc[f], want), (c.name, driver, "desc." + f)


def run_case(ctx, models, c):
    om, om3 = models[c.mkey]
    dna = block(ctx, c)
    dna_off = dna.read()[1]
    # the host driver: always the oracle's, whatever order the lists come in
    st, got = ba.fs_windows_selftest(ctx, om, om3, dna, c.lanes(shuffle=3), c.nc_total, F3=I.F3, std_pipe=c.std_pipe, driver=1)
    assert st == ba.OK
    check_build(c, got, 1, dna_off)
    # the device driver, under two shuffles
    outs = []
    for seed in (1, 2):
        st, got = ba.fs_windows_selftest(ctx, om, om3, dna, c.lanes(shuffle=seed), c.nc_total, F3=I.F3, std_pipe=c.std_pipe, driver=0)
        if not c.accepts:
            assert st == ba.ENORESULT and got is None, (c.name, st)
            continue
        assert st == ba.OK, (c.name, st)
        check_build(c, got, 0, dna_off)
        outs.append(got)
    if outs:
        a, b = outs
        for f in ("orfs", "windows", "grp", "voff", "vlen", "desc"):
            fa, fb = a[f], b[f]
            if f == "orfs":                                # (wb, we: the winner's index in a shuffled list)
                for n in fa.dtype.names:
                    assert n in ("wb", "we") or fa[n].tobytes() == fb[n].tobytes(), (c.name, "two shuffles", f, n)
            else:
                assert fa.tobytes() == fb.tobytes(), (c.name, "two shuffles", f)


REFUSED = [n for n in I.CASES if n in ("n32769", "group1025", "hitwins65537", "lanes17", "far_start")]
ACCEPTED = [n for n in I.CASES if n not in REFUSED]


@pytest.mark.parametrize("name", ACCEPTED)
def test_both_drivers_against_the_oracle(gpu_ctx, models, name):
    c = I.case(name)
    assert c.accepts
    run_case(gpu_ctx, models, c)


@pytest.mark.parametrize("name", REFUSED)
def test_blocks_the_kernels_hand_back(gpu_ctx, models, name):
    """BATH_ENORESULT without an error from the kernels' driver, the oracle's windows from the host build, and the next accepted block on
    the same context still right."""
    c = I.case(name)
    assert not c.accepts
    run_case(gpu_ctx, models, c)
    run_case(gpu_ctx, models, I.case("density"))


def test_rank_grid_of_this_device(gpu_ctx, models):
    """fsw_rank_kernel's grid is (tiles of 256 keys, column ranges), about four blocks per compute unit: the first n at which the column
    ranges are fewer than the tiles and do not divide them evenly, computed for the device the test runs on."""
    cus = ba.lib().bath_selftest_compute_units(gpu_ctx._h)
    n = I.first_split_n(cus)
    gn = (n + 255) // 256
    cols = max(1, min(gn, (cus * 4) // gn))
    assert cols < gn and gn % cols != 0
    print("%d compute units: n = %d, %d tiles over %d column ranges" % (cus, n, gn, cols))
    if n > 32768:
        pytest.fail("the device has so many compute units that the rank grid never splits unevenly below the ORF cap")
    run_case(gpu_ctx, models, I.case("n%d" % n) if n in I.SIZES else I.size_case(n))


@pytest.mark.parametrize("do_biasfilter,std_pipe", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("driver", [0, 1])
def test_decide(gpu_ctx, models, do_biasfilter, std_pipe, driver):
    """fsw_decide_kernel and the host loop of fs_decide against bo_fs_decide_window: L3 = 0, 1, 2 and typical lengths, windows without a
    hit window (no local pass), the bias filter off, --fsonly; every decision clear or exactly tied."""
    rec, bias, fsc, kinds, want = I.decide_cases(do_biasfilter, std_pipe)
    got = ba.fs_decide_selftest(gpu_ctx, models["pth2"][1], rec, bias, fsc, do_biasfilter, std_pipe, I.F3, driver)
    wn = np.array(want, np.float64)
    assert np.array_equal(got["branch"], wn[:, 4].astype(np.int32)), np.flatnonzero(got["branch"] != wn[:, 4])[:8]
    for f in ("window", "strand", "n", "length", "orf_cnt", "k_min", "k_max", "P_tot", "P_min", "tot_orfsc"):
        assert np.array_equal(got[f], rec[f])
    assert np.array_equal(got["fwdsc"].view(np.uint32), fsc.view(np.uint32))
    nan = np.isnan(wn[:, 0])
    assert nan.sum() == 3 and np.array_equal(np.isnan(got["nullsc"]), nan) and np.array_equal(np.isnan(got["P_fs"]), nan) and np.array_equal(np.isnan(got["P_null"]), nan)
    ok = ~nan
    assert (np.abs(got["nullsc"][ok] - wn[ok, 0]) <= 1e-5 * np.maximum(1.0, np.abs(wn[ok, 0]))).all()
    assert (np.abs(got["filtersc"][ok] - wn[ok, 1]) <= 1e-4 * np.maximum(1.0, np.abs(wn[ok, 1]))).all()
    # (an ulp bound on a P-value asks that the fp32 scores entering it are the oracle's bits: the figures say whether they were)
    for f, col in (("nullsc", 0), ("filtersc", 1)):
        print("driver %d: %s differs from the oracle's bits in %d of %d records" % (driver, f, int((got[f][ok].view(np.uint32) != wn[ok, col].astype(np.float32).view(np.uint32)).sum()), int(ok.sum())))
    for f, col in (("P_fs", 2), ("P_null", 3)):
        d = ulps(got[f][ok], wn[ok, col])
        if driver == 1:
            assert d.max(initial=0) == 0, (f, "host loop", int(d.max()))
        else:
            _worst[f] = max(_worst[f], int(d.max(initial=0)))
            print("device %s within %d ulp of the oracle's" % (f, int(d.max(initial=0))))
            assert d.max(initial=0) <= 2, (f, "kernel", int(d.max()))


_planted = {}


@pytest.mark.parametrize("lanes", ["1", "3"])
def test_pipeline_with_hundreds_of_survivors_on_a_strand(gpu_ctx, monkeypatch, lanes):
    """End to end through Pipeline.run_frameshift with one and with three cascade lanes: a 285 kb sequence carrying 900 planted PTH2 genes
    on both strands, most with insertions or deletions, plus a few short sequences.  The only case in which fs_select_*_kernel, the
    fetch and the merge feed the window kernels a (sequence, strand) group of more than 256 survivors.  Held to model.run_pipeline_fs by
    test_fs_pipeline_gpu.compare, plus the windows' coordinates and the Forward scores' bits as test_fs_strict_gpu.check_exact has them.
    (The gene count is what puts more than 256 survivors on each strand: about 0.3 per gene pass F4.  The oracle leg takes 3 s on the CPU
    machine and is shared by both runs.)"""
    import test_fs_pipeline_gpu as P
    path, model = I.model("pth2")
    if not _planted:
        wins = I.planted_block(900)
        _planted["wins"], _planted["oracle"] = wins, model.run_pipeline_fs(wins)
    wins = _planted["wins"]
    pli, ores, per_seq, ofw, per_seq_w = _planted["oracle"]
    per_group = {}
    for w, (a, b) in enumerate(per_seq):
        for r in ores[a:b]:
            if r.stage == 4:
                per_group[(w, r.strand)] = per_group.get((w, r.strand), 0) + 1
    assert max(per_group.values()) > 256 and sorted(per_group.values())[-2] > 256       # both strands of the long sequence
    monkeypatch.setenv("BATH_HIP_LANES", lanes)
    gpu_ctx.set_fs_strict(True)
    hmm = ba.HMM(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    stats, res, fw = ba.Pipeline(gpu_ctx, om, fs_pipe=True, ncbi_table=hmm.ct).run_frameshift(om3, ba.SeqBlock(gpu_ctx, wins))
    assert P.compare(model, stats, fw, pli, ofw, per_seq_w) == len(ofw) >= 300
    want = sorted(((w, o) for w, (a, b) in enumerate(per_seq_w) for o in ofw[a:b]), key=lambda t: (t[0], t[1].strand, t[1].n))
    got = sorted(fw, key=lambda g: (g.window, g.strand, g.n))
    for g, (w, o) in zip(got, want):
        assert (g.window, g.strand, g.n, g.length, g.orf_cnt, g.k_min, g.k_max) == (w, o.strand, o.n, o.length, o.orf_cnt, o.k_min, o.k_max)
        assert np.float32(g.fwdsc).view(np.uint32) == np.float32(o.fwdsc).view(np.uint32), (w, g.fwdsc, o.fwdsc)
    assert {g.branch for g in got} == {1, 2} and any(g.orf_cnt > 2 for g in got)


def test_worst_device_deviation_is_reported(gpu_ctx):
    """Runs last in this module: the largest deviation of the kernels' P-values from the oracle's seen above, in ulps of a double (DESIGN.md 4.5d states it)."""
    print("worst device deviation, ulps: %r" % (_worst,))
    assert max(_worst.values()) <= 2
