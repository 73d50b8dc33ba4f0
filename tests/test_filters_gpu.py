"""GPU parity: the batched HIP filters (through the C ABI) against the oracle, per target.

Integer filters (SSV/MSV, Viterbi) must be BIT-EXACT in score and status (the reference's own tests
demand 0.001 against the exact-emulation identity, msvfilter.c:648, vitfilter.c:680; integers give 0).
Forward and the bias filter are fp32: tolerance 1e-4 relative / 2e-4 absolute nats, written below.
"""
import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol

pytestmark = pytest.mark.gpu

MODELS = [("Caudal_act.bhmm", 0), ("PTH2.bhmm", 0), ("2OG-FeII_Oxy_3.bhmm", 0), ("MET-ct4.bhmm", 0), ("MET-ct4.bhmm", 1),
          ("synthetic:1024", 0), ("synthetic:700", 0), ("synthetic:7", 0),   # M=458: 2 lanes/target; M=1024: 4 lanes/target
          ("synthetic:256", 0), ("synthetic:300", 0), ("synthetic:1025", 0), ("synthetic:2048", 0)]   # wave filters at 4, 6, 24 and 32 nodes per lane (C > 16: tables in global memory)


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] + "#" + str(m[1]) for m in MODELS])
def setup(request, gpu_ctx, tmp_path_factory):
    name, idx = request.param
    if name.startswith("synthetic:"):
        M = int(name.split(":")[1])
        path = common.write_synthetic_bhmm(str(tmp_path_factory.mktemp("hmm") / ("s%d.bhmm" % M)), M, seed=M)
    else:
        path = ol.GOLDEN + "/" + name
    model = ol.Model(path, idx)
    hmm = ba.HMM(path, idx)
    gm = ba.Profile(hmm)
    om = ba.OProfile(gpu_ctx, gm)
    rng = np.random.default_rng(42)
    seqs = common.random_aa(rng, 600, 20, 400)
    seqs += common.emit_from_model(rng, model, 200)
    seqs += common.emit_from_model(rng, model, 60, sharpen=3.0)          # strong hits: overflow / J-state branches
    seqs += [np.zeros(1, np.uint8), np.full(3, 19, np.uint8), seqs[0][:1]]  # L=1 edge cases (msvfilter.c:722)
    seqs += common.random_aa(rng, 20, 1500, 3000)
    sq = ba.SeqBlock(gpu_ctx, seqs)
    return gpu_ctx, model, om, seqs, sq


def _same_scores(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ssv_bit_exact(setup):
    ctx, model, om, seqs, sq = setup
    sc, st = ba.SSVFilter(ctx, om, sq)
    osc, ost = common.oracle_scores(model, seqs, "bo_ssvfilter")
    assert np.array_equal(st, ost)
    ok = ost == 0
    assert _same_scores(sc[ok], osc[ok])
    assert set(np.unique(ost)) >= {0}, "test set must exercise the OK branch"


@pytest.mark.parametrize("M", [16, 33, 64, 100, 152, 153, 200, 260, 304, 305, 416, 417, 600, 830, 1024, 1300, 1664])
def test_ssv_every_register_tiling(gpu_ctx, tmp_path, M):
    """The lane-per-target SSV kernels are instantiated per register count (NR = 16 .. 208 in steps of 4 / 16) and lanes per
    target (G = 1, 2, 4, 8), with hand-pipelined LDS reads and a VGPR bound that depends on NR: a sweep over model lengths
    that lands on the shapes' boundaries (152 | 153: one | two lanes with narrow tiles; 304 | 305: back to one lane with a wide
    tile; 416 | 417: one | two lanes per target; 1024: four).  A target's lanes are 64/G apart in the wave (SsvGroups).
    Both entry points: the standalone filter (ssv_lane_kernel) and the cascade (ssv_orf_kernel, through the survivors'
    MSV scores and the counters)."""
    path = common.write_synthetic_bhmm(str(tmp_path / ("s%d.bhmm" % M)), M, seed=M)
    model = ol.Model(path, 0)
    hmm = ba.HMM(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    rng = np.random.default_rng(M)
    seqs = common.random_aa(rng, 150, 20, 300) + common.emit_from_model(rng, model, 60) + common.emit_from_model(rng, model, 20, sharpen=3.0)
    sc, st = ba.SSVFilter(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs))
    osc, ost = common.oracle_scores(model, seqs, "bo_ssvfilter")
    assert np.array_equal(st, ost)
    ok = ost == 0
    assert ok.sum() > 0 and _same_scores(sc[ok], osc[ok])
    wins = [np.array(common.revtranslate(rng, aa, model.basic), dtype=np.uint8) for aa in common.emit_from_model(rng, model, 12, flank=10)]
    wins += common.random_dna(rng, 24, 900)
    stats, res = ba.Pipeline(gpu_ctx, om, fs_pipe=False).run(ba.SeqBlock(gpu_ctx, wins))
    pli, ores, _ = model.run_pipeline(wins)
    for f in ("n_orfs", "n_past_msv", "pos_past_msv", "pos_past_bias", "pos_past_vit", "pos_past_fwd"):
        assert getattr(stats, f) == getattr(pli, f), f
    want = sorted(np.float32(r.usc).view(np.uint32) for r in ores if r.stage >= 1)
    got = sorted(np.float32(u).view(np.uint32) for u in res["usc"])
    assert want == got
    if M == 1300:
        # above ~1100 nodes the Forward / Backward tables no longer fit the LDS and are read from global memory; above 1024 the
        # envelope kernels take the lane-per-envelope path: the hits must still be the oracle's
        _, dm, _ = ba.Pipeline(gpu_ctx, om, fs_pipe=False).run_hits(ba.SeqBlock(gpu_ctx, wins[:12]))
        _, odm, per_d, _ = model.run_pipeline_hits(wins[:12])
        key = lambda w, d: (w, d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm)
        assert len(odm) >= 6 and sorted(key(d.window, d) for d in dm) == sorted(key(w, o) for w, (a, b) in enumerate(per_d) for o in odm[a:b])


@pytest.mark.parametrize("M", [40, 46, 54, 62, 70, 78, 86, 94, 102, 110, 118, 126, 134, 142, 150])
def test_msv_lane_every_register_tiling(gpu_ctx, tmp_path, M):
    """msv_lane_kernel<NR> (bath_msv_lane.hip: the J-state recurrence with a lane per target, models up to 152 nodes) is instantiated
    per register count NR = 16 .. 76 in steps of 4: every NR the other tests' models do not land on, score and status bit-exact,
    with targets that reach the J state, targets that overflow, single residues and lengths that are no multiple of the 8-residue
    reads."""
    path = common.write_synthetic_bhmm(str(tmp_path / ("s%d.bhmm" % M)), M, seed=M)
    model = ol.Model(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))
    rng = np.random.default_rng(1000 + M)
    seqs = common.random_aa(rng, 120, 1, 97) + common.emit_from_model(rng, model, 80) + common.emit_from_model(rng, model, 40, sharpen=3.0)
    seqs += [np.concatenate(common.emit_from_model(rng, model, 3, sharpen=3.0)) for _ in range(6)]       # several domains in a row: J state, overflow
    sc, st = ba.MSVFilter(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs))
    osc, ost = common.oracle_scores(model, seqs, "bo_msvfilter")
    assert np.array_equal(st, ost)
    assert _same_scores(sc, osc)
    _, sst = common.oracle_scores(model, seqs, "bo_ssvfilter")
    assert (sst != 0).sum() >= 5                             # targets SSV could not decide: they went through the lane kernel


VIT_LANE_NR = [16, 32, 48, 64, 68, 72, 76, 80, 96, 112]
# per instantiation the smallest and the largest model that selects it; 16 | 17: the high half of every register is padding | holds
# one node (M <= NR | M = NR + 1); 31: an odd M, the last slot padded; 32, 64, ...: M = 2 NR, no padding; 225: the wave kernel
VIT_LANE_M = [1, 16, 17, 31, 32, 33, 64, 65, 96, 97, 128, 129, 136, 137, 144, 145, 152, 153, 160, 161, 192, 193, 224, 225]
ESL_ERANGE = 16


def vit_lane_nr(M):
    """Node pairs per lane of vit_lane_kernel<NR> for a model of M nodes, None beyond its range (bath_profile.hip: NRv)."""
    nr = ((M + 1) // 2 + 15) // 16 * 16
    if nr == 80:
        nr = max(68, ((M + 1) // 2 + 3) // 4 * 4)
    return nr if nr <= 112 else None


def vit_lane_targets(model, M):
    """The targets of the lane-per-target Viterbi sweeps, seeded by M: every length from 1 to 9 and either side of multiples of 4
    (the kernel reads residues four to a word and pads the last word with code 29) and of 128 (the cascade's long-ORF split),
    background with degenerate residues, homologs plain and sharpened, several sharpened domains in a row (overflow, the J state),
    and targets of '*' residues (the lowest scores a target can get).  325 targets: the second block of 256 lanes has one full wave,
    one partly live wave (5 lanes) and two idle ones."""
    rng = np.random.default_rng(2000 + M)
    seqs = []
    for L in list(range(1, 10)) + [11, 12, 13, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130]:
        seqs += common.random_aa(rng, 2, L, L)
    seqs += common.random_aa(rng, 99, 20, 300)
    seqs += common.emit_from_model(rng, model, 100) + common.emit_from_model(rng, model, 50, sharpen=3.0)
    seqs += [np.concatenate(common.emit_from_model(rng, model, int(rng.integers(2, 6)), sharpen=3.0)) for _ in range(24)]
    seqs += common.random_aa(rng, 6, 400, 900)
    seqs += [np.full(1, 27, np.uint8), np.full(5, 27, np.uint8)]
    assert len(seqs) == 325
    return seqs


@pytest.mark.parametrize("M", VIT_LANE_M, ids=["NR%s-M%d" % (vit_lane_nr(m) or "wave", m) for m in VIT_LANE_M])
def test_vit_lane_every_register_tiling(gpu_ctx, tmp_path, M):
    """vit_lane_kernel<NR> (bath_viterbi.hip: a lane per target, node pairs r+1 | NR+r+1 packed per register, models up to 224 nodes)
    at every instantiation, at the smallest and the largest model each serves, and the first model beyond them (225: vit_wave_kernel):
    score and status of every target bit-exact against the oracle.  The conditions on the target set are the oracle's results
    alone.  The oracle scores no target -inf at any M of the list, '*' residues included (they score about -50 nats): the
    special states start at base 12000 of the 16-bit range, and neither B->M of a model this short nor any emission the profile holds
    takes xE down to -32768.  The count is printed; the branch stays compiled in and unreached here, as it is in the oracle."""
    path = common.write_synthetic_bhmm(str(tmp_path / ("s%d.bhmm" % M)), M, seed=M)
    model = ol.Model(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))
    seqs = vit_lane_targets(model, M)
    osc, ost = common.oracle_scores(model, seqs, "bo_vitfilter")
    n_erange, n_ok, n_neginf = int((ost == ESL_ERANGE).sum()), int((ost == 0).sum()), int(np.isneginf(osc).sum())
    print("M=%d NR=%s targets=%d ERANGE=%d OK=%d -inf=%d" % (M, vit_lane_nr(M), len(seqs), n_erange, n_ok, n_neginf))
    assert len(seqs) % 64 != 0 and 0 < len(seqs) % 256 <= 192          # a partly live wave and an idle one in the last block
    if M >= 65:
        assert n_erange >= 5 and n_ok >= 100
    sc, st = ba.ViterbiFilter(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs))
    assert np.array_equal(st, ost)
    assert _same_scores(sc, osc)
    for t in (0, len(seqs) // 2):                                       # one target per call: one live lane in the grid
        sc1, st1 = ba.ViterbiFilter(gpu_ctx, om, ba.SeqBlock(gpu_ctx, seqs[t:t + 1]))
        assert st1[0] == ost[t] and _same_scores(sc1, osc[t:t + 1])


VIT_WINDOWS_P = 1e-3
LONG_VIT_TARGET = 128          # bath_viterbi.hip, kVitLongTarget: longer targets of a sorted list go to the wave-per-target kernel


def vit_window_targets(model, M):
    """Targets for the window sweeps, seeded by M: homologs plain and sharpened, homologs cut off inside the domain (a window that
    runs into the target's end), several domains in a row (several windows per target: skip_until; the long side of the split),
    background, and the short lengths of vit_lane_targets."""
    rng = np.random.default_rng(3000 + M)
    seqs = []
    for L in list(range(1, 10)) + [11, 12, 13, 127, 128, 129]:
        seqs += common.random_aa(rng, 1, L, L)
    seqs += common.random_aa(rng, 40, 20, 300)
    seqs += common.emit_from_model(rng, model, 40, flank=12) + common.emit_from_model(rng, model, 40, flank=12, sharpen=2.0)
    cut = common.emit_from_model(rng, model, 20, flank=6, sharpen=2.0)
    seqs += [s[:max(1, len(s) - int(rng.integers(1, max(2, len(s) // 2))))] for s in cut]
    seqs += [np.concatenate([d if rng.random() < 0.5 else np.concatenate([d, common.random_aa(rng, 1, 10, 40)[0]])
                             for d in common.emit_from_model(rng, model, int(rng.integers(2, 5)), flank=8, sharpen=1.5)]) for _ in range(20)]
    seqs += common.random_aa(rng, 4, 300, 600)
    # the model's last nodes, most probable residue each, behind a random flank: a window whose extension runs to node M
    h = model.hmm.contents
    mat = np.ctypeslib.as_array(h.mat, shape=((M + 1) * 20,)).reshape(M + 1, 20)
    for _ in range(6):
        a = int(rng.integers(max(1, M - 60), max(2, M - 8)))
        seqs.append(np.concatenate([common.random_aa(rng, 1, 5, 30, with_degenerate=False)[0], mat[a:M + 1].argmax(axis=1).astype(np.uint8)]))
    return seqs


def oracle_vit_windows(model, seqs, filtersc, P):
    """bo_vitfilter_bath per target: (scores, statuses, [(target, n, k, length, score)])."""
    import ctypes as C
    L_ = ol.lib()
    sc, st, wins = np.zeros(len(seqs), np.float32), np.zeros(len(seqs), np.int32), []
    out = C.c_float()
    for t, s_ in enumerate(seqs):
        L_.bo_oprofile_reconfig_length(model.om, len(s_))
        owl = ol.WindowList(); L_.bo_windowlist_init(C.byref(owl))
        st[t] = L_.bo_vitfilter_bath(ol.u8(ol.dsq_from(s_)), len(s_), model.om, model.sd, C.c_float(filtersc[t]), C.c_double(P), C.byref(owl), C.byref(out))
        sc[t] = out.value
        wins += [(t, owl.w[i].n, owl.w[i].k, owl.w[i].length, owl.w[i].score) for i in range(owl.count)]
        L_.bo_windowlist_free(C.byref(owl))
    return sc, st, wins


def gpu_vit_windows(ctx, om, seqs, filtersc, P):
    """bath_hip_vitfilter_bath: (scores, statuses, [(target, n, k, length, score)], name of the Viterbi kernel that ran)."""
    import ctypes as C
    blk = ba.SeqBlock(ctx, seqs)                     # (held: the block must outlive the call)
    sc, st = np.zeros(len(seqs), np.float32), np.zeros(len(seqs), np.int32)
    fsc = np.ascontiguousarray(filtersc, np.float32)
    w, nw = C.POINTER(ba.HmmWindow)(), C.c_int64(0)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ctx._check(ba.lib().bath_hip_vitfilter_bath(ctx._h, om._h, blk._h, fsc.ctypes.data_as(f32p), C.c_double(P), sc.ctypes.data_as(f32p), st.ctypes.data_as(i32p),
                                                C.byref(w), C.byref(nw)), "vitfilter_bath")
    wins = [(int(w[i].target), w[i].n, w[i].k, w[i].length, w[i].score) for i in range(nw.value)]
    arr = (ba.KernelTime * 32)()
    names = [arr[i].name.decode() for i in range(ba.lib().bath_hip_kernel_times(ctx._h, 32, arr))]
    vit = [n for n in names if n.startswith("vit_")]        # (the call also lists what the domain stage's own contexts last ran)
    assert len(vit) == 1, names
    return sc, st, wins, vit[0]


@pytest.fixture(scope="module")
def lane_forced_windows(tmp_path_factory):
    """The window sweep again in a fresh process with BATH_HIP_LANE_MIN_NT=0 (read once per process): bath_hip_vitfilter_bath then takes
    the lane-per-target kernel with the length sort and the long-target split, as the cascade does on blocks of 150 M nt.  The
    child asserts the oracle comparison and the kernel's name itself and leaves its arrays per M in the directory returned."""
    import os, subprocess, sys
    if os.environ.get("BATH_TEST_VIT_WINDOWS_DUMP"):
        return None                                  # this is the child
    out = str(tmp_path_factory.mktemp("vit_lane_windows"))
    env = dict(os.environ, BATH_HIP_LANE_MIN_NT="0", BATH_TEST_VIT_WINDOWS_DUMP=out)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_vit_lane_windows_every_register_tiling"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "%d passed" % len(VIT_LANE_WINDOWS_M) in p.stdout and "failed" not in p.stdout, p.stdout[-3000:]
    return out


VIT_LANE_WINDOWS_M = [m for m in VIT_LANE_M if vit_lane_nr(m) is not None]


@pytest.mark.parametrize("M", VIT_LANE_WINDOWS_M, ids=["NR%d-M%d" % (vit_lane_nr(m), m) for m in VIT_LANE_WINDOWS_M])
def test_vit_lane_windows_every_register_tiling(gpu_ctx, tmp_path, lane_forced_windows, M):
    """p7_ViterbiFilter_BATH's hit windows (vitfilter.c:386-424) from vit_lane_kernel<NR> at every instantiation: the visiting-rank
    table, k_start, the diagonal extension, skip_until.  bath_hip_vitfilter_bath runs the cascade's own Viterbi step
    (launch_vit_sorted: length sort, targets beyond 128 residues to the wave kernel on the side stream, the rest to the lane kernel)
    when the batch is large enough or BATH_HIP_LANE_MIN_NT=0.  This test runs twice: here, where the small batch takes
    vit_wave_kernel, and in a child process with the variable set, where it must take vit_lane_kernel<NR> with the NR the rule of
    bath_profile.hip gives (the kernel's name is read back: a forced run that took the wave kernel fails).  Both runs hold status,
    score bits and every target's windows (n, k, length exactly; the score is 0.0 on both sides: only p7_SSVFilter_BATH scores its
    windows, hmmer.h:998) against the oracle, and the two runs' arrays must be identical.
    The oracle's records tell how an extension ended: k == M means it ran to the model's last node (kk == M), n + length - 1 == L
    that it ran to the target's last residue (nn == L); both are required of the set from M = 33 on."""
    import os
    dump = os.environ.get("BATH_TEST_VIT_WINDOWS_DUMP")
    forced = os.environ.get("BATH_HIP_LANE_MIN_NT") == "0"
    assert bool(dump) == forced
    path = common.write_synthetic_bhmm(str(tmp_path / ("s%d.bhmm" % M)), M, seed=M)
    model = ol.Model(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))
    seqs = vit_window_targets(model, M)
    _, filtersc = common.oracle_bias(model, seqs)
    osc, ost, owins = oracle_vit_windows(model, seqs, filtersc, VIT_WINDOWS_P)
    # the input set, judged on the oracle's results alone
    per_target = np.bincount([w[0] for w in owins], minlength=len(seqs))
    lens = np.array([len(s) for s in seqs])
    to_model_end = sum(1 for w in owins if w[2] == M)
    to_target_end = sum(1 for w in owins if w[1] + w[3] - 1 == lens[w[0]])
    print("M=%d NR=%d targets=%d long=%d ERANGE=%d windows=%d multi-window targets=%d to-model-end=%d to-target-end=%d" %
          (M, vit_lane_nr(M), len(seqs), (lens > LONG_VIT_TARGET).sum(), (ost == ESL_ERANGE).sum(), len(owins), (per_target >= 2).sum(), to_model_end, to_target_end))
    assert (lens > LONG_VIT_TARGET).sum() >= 5 and (lens <= LONG_VIT_TARGET).sum() >= 50
    if M >= 33:
        assert len(owins) >= 20 and (per_target >= 2).sum() >= 3
        assert to_model_end >= 1 and to_target_end >= 1
    sc, st, wins, kernel = gpu_vit_windows(gpu_ctx, om, seqs, filtersc, VIT_WINDOWS_P)
    print("M=%d kernel=%s" % (M, kernel))
    assert kernel == ("vit_lane_kernel<%d>" % vit_lane_nr(M) if forced else "vit_wave_kernel")
    assert np.array_equal(st, ost)
    assert _same_scores(sc, osc)
    assert [w[:4] for w in wins] == [w[:4] for w in owins]
    assert all(a[4] == b[4] == 0.0 for a, b in zip(wins, owins))
    flat = np.array(wins, np.float64).reshape(-1, 5)
    if dump:
        np.savez(os.path.join(dump, "M%d.npz" % M), sc=sc, st=st, wins=flat)
    else:
        lane = np.load(os.path.join(lane_forced_windows, "M%d.npz" % M))
        assert np.array_equal(lane["st"], st) and _same_scores(lane["sc"], sc) and np.array_equal(lane["wins"], flat)


def test_msv_bit_exact(setup):
    ctx, model, om, seqs, sq = setup
    sc, st = ba.MSVFilter(ctx, om, sq)
    osc, ost = common.oracle_scores(model, seqs, "bo_msvfilter")
    assert np.array_equal(st, ost)
    assert _same_scores(sc, osc)
    # the set has to reach the J-state re-run and the overflow branch, or this test proves little
    _, sst = common.oracle_scores(model, seqs, "bo_ssvfilter")
    if model.M >= 50:
        assert (sst == 19).sum() > 0 and (ost == 16).sum() > 0


def test_viterbi_bit_exact(setup):
    ctx, model, om, seqs, sq = setup
    sc, st = ba.ViterbiFilter(ctx, om, sq)
    osc, ost = common.oracle_scores(model, seqs, "bo_vitfilter")
    assert np.array_equal(st, ost)
    assert _same_scores(sc, osc)


def test_forward_parser(setup):
    ctx, model, om, seqs, sq = setup
    sc, st = ba.ForwardParser(ctx, om, sq)
    osc, ost = common.oracle_scores(model, seqs, "bo_forward_parser")
    assert np.array_equal(st, ost)
    assert np.allclose(sc, osc, rtol=1e-4, atol=2e-4)


def test_backward_parser(setup):
    """p7_BackwardParser on the GPU against the oracle (oracle/filters.c, fwdback.c:468-740): score, and every
    special-state row {E,N,J,B,C} of both passes with the same per-row SCALE.  Backward is rescaled by Forward's row
    factors, which are exactly 1 except on the sparse rows where xE passed 1e4, so the SCALE columns must be identical
    unless a row's xE sits within rounding of that threshold.  Forward == Backward per target (the reference's own
    utest, fwdback.c:1015-1085, demands 0.001)."""
    ctx, model, om, seqs, sq = setup
    fsc, bsc, fst, bst, fx, bx = ba.FwdBackParser(ctx, om, sq)
    L_ = ol.lib()
    import ctypes as C
    out = C.c_float(0)
    checked = 0
    for i, s_ in enumerate(seqs):
        n = len(s_)
        d = ol.dsq_from(s_)
        L_.bo_oprofile_reconfig_length(model.om, n)
        ofx = np.zeros((n + 1) * 6, np.float32); obx = np.zeros((n + 1) * 6, np.float32)
        st_f = L_.bo_forward_parser(ol.u8(d), n, model.om, ofx.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)); of = out.value
        st_b = L_.bo_backward_parser(ol.u8(d), n, model.om, ofx.ctypes.data_as(C.POINTER(C.c_float)), obx.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)); ob = out.value
        assert (fst[i], bst[i]) == (st_f, st_b)
        if st_f != 0 or st_b != 0:
            continue
        assert abs(fsc[i] - of) <= 2e-4 + 1e-4 * abs(of)
        assert abs(bsc[i] - ob) <= 2e-4 + 1e-4 * abs(ob)
        assert abs(fsc[i] - bsc[i]) <= 1e-3 + 1e-4 * abs(of)
        ofx, obx = ofx.reshape(-1, 6), obx.reshape(-1, 6)
        if i % 7 == 0 or n > 1000:                        # row-level comparison on a sample (and on every long target)
            same_scale = np.array_equal(fx[i][:, 5], ofx[:, 5])
            if same_scale:
                assert np.allclose(fx[i][:, :5], ofx[:, :5], rtol=2e-4, atol=1e-30)
                assert np.array_equal(bx[i][:, 5], obx[:, 5])
                assert np.allclose(bx[i][:, :5], obx[:, :5], rtol=5e-4, atol=1e-30)
                checked += 1
    assert checked > 50


def test_bias_filter(setup):
    ctx, model, om, seqs, sq = setup
    nullsc, fsc = ba.BiasFilter(ctx, om, sq)
    onull, ofsc = common.oracle_bias(model, seqs)
    assert _same_scores(nullsc, onull)
    assert np.allclose(fsc, ofsc, rtol=1e-5, atol=1e-4)


def test_empty_block(gpu_ctx, setup):
    ctx, model, om, seqs, sq = setup
    empty = ba.SeqBlock(ctx, [])
    sc, st = ba.MSVFilter(ctx, om, empty)
    assert sc.shape == (0,) and st.shape == (0,)


SSV_BATH_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 52]
SSV_BATH_M = [1, 65, 129, 193, 300, 512, 768, 1024, 1025, 2048, 2049, 3328]


@pytest.mark.parametrize("M", SSV_BATH_M, ids=["C%d-M%d" % (next(c for c in SSV_BATH_COLUMNS if (m + 63) // 64 <= c), m) for m in SSV_BATH_M])
def test_ssv_bath_windows_every_tiling(gpu_ctx, tmp_path, M):
    """p7_SSVFilter_BATH (bath_hip_ssvfilter_bath: ssv_bath_kernel<C>, C = ceil(M / 64) rounded up to the next instantiation) at
    every tiling, up to the 3328 nodes an OProfile holds (C = 52: beyond the cascade's 2048, only this entry point reaches it): every
    hit window (position, node, length) and its score against the oracle's, target by target."""
    import ctypes as C
    path = common.write_synthetic_bhmm(str(tmp_path / ("s%d.bhmm" % M)), M, seed=M)
    model = ol.Model(path, 0)
    om = ba.OProfile(gpu_ctx, ba.Profile(ba.HMM(path, 0)))
    rng = np.random.default_rng(M)
    seqs = common.random_aa(rng, 40, 20, 400) + common.emit_from_model(rng, model, 12, sharpen=2.0) + common.emit_from_model(rng, model, 4, flank=5)
    seqs += [np.concatenate(common.emit_from_model(rng, model, 2, sharpen=3.0)), seqs[0][:1]]
    P = 0.02
    w = C.POINTER(ba.HmmWindow)()
    nw = C.c_int64(0)
    blk = ba.SeqBlock(gpu_ctx, seqs)                 # (held: the block must outlive the call)
    gpu_ctx._check(ba.lib().bath_hip_ssvfilter_bath(gpu_ctx._h, om._h, blk._h, C.c_double(P), C.byref(w), C.byref(nw)), "ssvfilter_bath")
    got = {}
    for i in range(nw.value):
        got.setdefault(int(w[i].target), []).append((w[i].n, w[i].k, w[i].length, w[i].score))
    L_ = ol.lib()
    n_windows = 0
    for t, s_ in enumerate(seqs):
        L = len(s_)
        L_.bo_oprofile_reconfig_length(model.om, L)
        owl = ol.WindowList(); L_.bo_windowlist_init(C.byref(owl))
        L_.bo_ssvfilter_bath(ol.u8(ol.dsq_from(s_)), L, model.om, model.sd, C.byref(model.bg), C.c_double(P), C.byref(owl))
        want = [(owl.w[i].n, owl.w[i].k, owl.w[i].length, owl.w[i].score) for i in range(owl.count)]
        L_.bo_windowlist_free(C.byref(owl))
        g = got.get(t, [])
        assert [x[:3] for x in g] == [x[:3] for x in want], t
        assert all(abs(a[3] - b[3]) <= 1e-5 * max(1.0, abs(b[3])) for a, b in zip(g, want)), t
        n_windows += len(want)
    assert n_windows >= 10
