"""CPU tier: the per-trace-stream ensemble modes of the frameshift branch (bath_hip_set_fs_ensemble), host side.

ENSEMBLE_STREAMS_HOST is the twin of the GPU kernel: the same source (bath_fs_ens_walk.hpp) walks a region's 200 stochastic
tracebacks, trace t from the state the region's generator has after t * 2^20 steps.  Here: the jump-ahead against the stepped
stream, the walk on fabricated matrices whose whole mass lies on one path (every exit of the state switch, the segment
bookkeeping), the "no valid traces" outcome, and the stream mode against the serial mode on the oracle's multihit Forward matrix
-- where the two can only agree the way two seeds of the serial mode agree, which the test checks first."""
import ctypes as C
import math

import numpy as np
import pytest

import bath_amd as ba
from bath_amd import synth
import oracle_lib as ol

NEG = -np.inf
XNL, XNM, XE = ba.fs_ensemble_loop_scores(100)
gD, gI, gM = 0, 1, 2
xE_, xN_, xJ_, xB_, xC_ = 0, 1, 2, 3, 4


@pytest.mark.parametrize("seed", [42, 1, 0xffffffff])
def test_jump_ahead_equals_the_stepped_stream(seed):
    """State after t * 2^20 steps, t = 0..3: value number n of the stream is state(n) / 2^32, so state(t 2^20 + 1) is behind element t 2^20."""
    n = 3 * (1 << 20) + 1
    out = np.zeros(n, np.float64)
    assert ba.lib().bath_selftest_rng_stream(seed, n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    for t in range(4):
        k = t << 20
        assert ba.rng_jump(seed, k + 1) / 4294967296.0 == out[k], (seed, t)
        if k:
            assert ba.rng_jump(seed, k) / 4294967296.0 == out[k - 1], (seed, t)      # the start state of trace t itself
    assert ba.rng_jump(seed, 0) == ba.rng_jump(seed, 1 << 32)                         # the generator's period


def forced(M, Lr, domains, last_codon=None):
    """A Forward matrix with one path of finite cells.  domains: [(iB, kstart, [codon lengths])] left to right; N before the first B, J
    between an E and the next B, C after the last E.  Returns fwd, fx and the segments (i, j, k, m) in region coordinates."""
    fwd = np.full((Lr + 1, M + 1, 8), NEG, np.float32)
    fx = np.full((Lr + 1, 5), NEG, np.float32)
    segs = []
    prev_e = None
    for d, (iB, k0, cs) in enumerate(domains):
        fx[iB, xB_] = 0.0
        if d == 0:
            fx[: iB + 1, xN_] = 0.0
        else:
            fx[prev_e: iB + 1, xJ_] = 0.0
        r = iB
        for q, c in enumerate(cs):
            r += c
            fwd[r, k0 + q, gM] = 0.0
            fwd[r, k0 + q, gM + c] = 0.0
        fx[r, xE_] = 0.0
        segs.append((iB + 1, r, k0, k0 + len(cs) - 1))
        prev_e = r
    fx[prev_e:, xC_] = 0.0
    return fwd.reshape(-1), fx.reshape(-1), segs


def expected_envelopes(segs, ireg):
    """cluster_segments on 200 copies of the path's segments (it is tested against the oracle in test_ensemble_cpu.py)."""
    idx, i, j, k, m = [], [], [], [], []
    for t in range(200):
        for s in segs:
            idx.append(t); i.append(s[0] + ireg - 1); j.append(s[1] + ireg - 1); k.append(s[2]); m.append(s[3])
    a = lambda v: np.ascontiguousarray(v, np.int32)
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    idx, i, j, k, m = a(idx), a(i), a(j), a(k), a(m)
    env = np.zeros(128, np.int32); n = C.c_int32(0)
    assert ba.lib().bath_selftest_cluster_segments(len(idx), p(idx), p(i), p(j), p(k), p(m), 200, 1, p(env), 64, C.byref(n)) == 0
    return [(int(env[2 * e]), int(env[2 * e + 1])) for e in range(n.value)]


def forced_cases():
    cases = []
    for Lr in range(5, 15):
        # M = 1: the C state runs down to i = 3 and leaves through its i < 4 exit; one codon of 3 ends at row 0
        cases.append(("M1-c-exit", 1, Lr, [(0, 1, [3])]))
        if Lr >= 6:        # two domains: the second one's B goes to J, which leaves through ITS i < 4 exit
            cases.append(("M1-j-exit", 1, Lr, [(0, 1, [3]), (Lr - 3, 1, [3])]))
        if Lr >= 8:        # codons of 1, 2, 4 and 5 nucleotides; E above row 3 is chosen by the draw, not by the exit
            cases.append(("M1-c5", 1, Lr, [(Lr - 7, 1, [5])]))
            cases.append(("M1-c1", 1, Lr, [(Lr - 5, 1, [1])]))
        # M = 7: as many nodes as the region holds, ending at node 7 (a local entry at node kstart > 1 below 21 nt)
        nk = min(7, (Lr - 1) // 3)
        cases.append(("M7-tail", 7, Lr, [(1, 7 - nk + 1, [3] * nk)]))
        nk = min(7, Lr // 3)
        cases.append(("M7-head", 7, Lr, [(0, 1, [3] * nk)]))             # nodes 1..nk from row 0: leaves at node nk < 7
        if Lr >= 12:
            cases.append(("M7-mixed", 7, Lr, [(1, 2, [2, 4, 3, 1][: 4])]))
    cases.append(("M7-full", 7, 30, [(4, 1, [3] * 7)]))
    cases.append(("M7-two", 7, 60, [(2, 1, [3, 3, 2, 3, 4, 3, 3]), (30, 1, [3] * 7)]))
    return cases


@pytest.mark.parametrize("name,M,Lr,domains", forced_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_forced_path_gives_its_segment_in_every_trace(name, M, Lr, domains):
    fwd, fx, segs = forced(M, Lr, domains)
    tsc = np.zeros((M, 8), np.float32)
    ireg = 17
    r = ba.fs_ensemble_streams(M, tsc, XNL, XNM, XE, ireg, Lr, fwd, fx, seed=42)
    assert r["status"] == ba.ENS_REGION_OK and not r["trace_status"].any()
    want = np.array([(t,) + s for t in range(200) for s in segs], np.int32)
    assert np.array_equal(r["segments"], want), (r["segments"][:4], want[:4])
    env = expected_envelopes(segs, ireg)
    assert r["envelopes"] == env
    if name == "M7-full":
        assert env == [(4 + ireg, 25 + ireg - 1)]            # sqfrom = iB + 1 = 5, sqto = 25, shifted by ireg - 1
    if name == "M7-two":
        assert len(env) == 2
    if M == 1:
        assert env == []                                     # a one-node segment is not linked to its own copies (p7_spensemble.c:207)
    # the serial mode walks the same only path
    assert ba.fs_ensemble_serial(M, tsc, XNL, XNM, XE, ireg, Lr, fwd, fx, seed=42) == env


@pytest.mark.parametrize("Lr", [5, 9, 14])
@pytest.mark.parametrize("c", [4, 5])
def test_codon_longer_than_the_rows_left_ends_the_ensemble(Lr, c):
    """i - c < 0 turns the M state into B and the walk then stands before row 0: the serial function returns with no envelopes, and so
    does the stream mode, with status "no valid traces"."""
    fwd, fx, _ = forced(1, Lr, [(0, 1, [3])])
    f = fwd.reshape(Lr + 1, 2, 8)
    f[3, 1, gM + 3] = NEG; f[3, 1, gM + c] = 0.0
    tsc = np.zeros((1, 8), np.float32)
    r = ba.fs_ensemble_streams(1, tsc, XNL, XNM, XE, 1, Lr, fwd, fx)
    assert r["status"] == ba.ENS_REGION_NO_TRACES and r["envelopes"] == [] and len(r["segments"]) == 0
    assert (r["trace_status"] == ba.ENS_IMPOSSIBLE).all()
    assert ba.fs_ensemble_serial(1, tsc, XNL, XNM, XE, 1, Lr, fwd, fx) == []


@pytest.mark.parametrize("M,Lr", [(1, 9), (7, 30)])
def test_impossible_start_gives_no_traces(M, Lr):
    fwd, fx, _ = forced(M, Lr, [(1, 1, [3] * min(M, 2))])
    fx.reshape(Lr + 1, 5)[Lr, xC_] = NEG                     # X(Lr, C) = -inf: the first state of every trace is impossible
    tsc = np.zeros((M, 8), np.float32)
    r = ba.fs_ensemble_streams(M, tsc, XNL, XNM, XE, 1, Lr, fwd, fx)
    assert r["status"] == ba.ENS_REGION_NO_TRACES and r["envelopes"] == [] and len(r["segments"]) == 0
    assert (r["trace_status"] == ba.ENS_IMPOSSIBLE).all()
    assert ba.fs_ensemble_serial(M, tsc, XNL, XNM, XE, 1, Lr, fwd, fx) == []


def test_region_outside_the_stream_rule_is_refused():
    """4 (4 (Lr + M) + 64) >= 2^20: a trace could run into the next trace's slice.  The twin answers ERANGE (the pipeline then runs
    the serial ensemble and counts it); nothing is read from the matrices."""
    M, Lr = 1, 65520
    z = np.zeros(8, np.float32)
    rs, ns, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    st = ba.lib().bath_selftest_fs_ensemble_streams(M, ba._f32(z), XNL, XNM, XE, 1, Lr, ba._f32(z), ba._f32(z), 42, C.byref(rs), None, None, 0, C.byref(ns), None, 0, C.byref(ne))
    assert st == ba.ERANGE


def test_own_expf_logf_are_correctly_rounded_where_sampled():
    """The walk's expf / logf are IEEE double arithmetic rounded once to float (so that host and device give the same float); the issue
    asks for 1 ulp.  Bound: 0.5 ulp of rounding + the double evaluation's error, far below 0.01 ulp of fp32."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-87, 88.7, 200000), rng.uniform(-1, 1, 100000)]).astype(np.float32)
    e = np.zeros_like(x)
    assert ba.lib().bath_selftest_ens_explog(len(x), ba._f32(x), ba._f32(e), None) == 0
    ref = np.exp(x.astype(np.float64))
    assert (np.abs(e - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)).max() <= 0.51
    y = np.concatenate([rng.uniform(0.5, 2, 100000), rng.uniform(1, 2100, 100000), np.exp(rng.uniform(-87, 88, 100000))]).astype(np.float32)
    lg = np.zeros_like(y)
    assert ba.lib().bath_selftest_ens_explog(len(y), ba._f32(y), None, ba._f32(lg)) == 0
    ref = np.log(y.astype(np.float64))
    nz = ref != 0
    assert (np.abs(lg - ref)[nz] / np.spacing(np.abs(ref[nz]).astype(np.float32)).astype(np.float64)).max() <= 0.51
    sp = np.array([-np.inf, -104.5, 0.0, 89.0, np.inf], np.float32)
    e = np.zeros_like(sp); lg = np.zeros_like(sp)
    assert ba.lib().bath_selftest_ens_explog(len(sp), ba._f32(sp), ba._f32(e), ba._f32(lg)) == 0
    assert list(e) == [0.0, 0.0, 1.0, np.inf, np.inf] and lg[2] == -np.inf and lg[4] == np.inf and np.isnan(lg[0])


# ---- stream mode against serial mode on the oracle's matrix

def consensus_two_copy_window(hmm, seed, spacer):
    """flank + gene + <spacer> random nt + gene + flank, the gene being the model's consensus (the likeliest residue of every match
    state) reverse-translated with a codon choice of its own per copy."""
    rng = np.random.default_rng(seed)
    mat = synth.hmm_match_emissions(hmm)
    aa = mat[1:].argmax(axis=1).astype(np.uint8)
    basic = ba.gencode_basic(hmm.ct)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    return np.concatenate([rnd(30), synth.reverse_translate(rng, aa, basic), rnd(spacer), synth.reverse_translate(rng, aa, basic), rnd(30)])


def overlap_ok(a, b):
    """The project's own link criterion (cluster_segments: min_overlap): shared nucleotides >= 0.8 of the shorter envelope."""
    nov = min(a[1], b[1]) - max(a[0], b[0]) + 1
    return nov / min(a[1] - a[0] + 1, b[1] - b[0] + 1) >= 0.8


# (model, window seed, spacer): fixed after checking on the CPU that the SERIAL mode meets the condition between seeds 42 and 43
ORACLE_WINDOWS = [("PTH2.bhmm", 11, 300), ("PTH2.bhmm", 12, 345), ("Caudal_act.bhmm", 21, 300), ("Caudal_act.bhmm", 22, 411)]


@pytest.fixture(scope="module")
def oracle_matrices():
    out = []
    L_ = ol.lib()
    for name, wseed, spacer in ORACLE_WINDOWS:
        path = ol.GOLDEN + "/" + name
        model = ol.Model(path, 0)
        hmm = ba.HMM(path, 0)
        tsc = ba.FSProfile(hmm, 5, ncbi_table=hmm.ct).arrays()[0].astype(np.float32)
        gm5 = model.fs(5)
        L_.bo_fs_profile_reconfig_multihit(gm5, 100)
        w = consensus_two_copy_window(hmm, wseed, spacer)
        L, M = len(w), model.M
        g8 = L_.bo_gmx_create(M, L + 1, L, 8)
        f = C.c_float()
        assert L_.bo_gforward_fs(ol.u8(ol.dsq_from(w)), L, gm5, g8, 0, C.byref(f)) == 0
        fwd = np.ctypeslib.as_array(g8.contents.dp, shape=((L + 1) * (M + 1) * 8,)).astype(np.float32).copy()
        fx = np.ctypeslib.as_array(g8.contents.xmx, shape=((L + 1) * 5,)).astype(np.float32).copy()
        L_.bo_gmx_free(g8)
        out.append((name, M, L, tsc, fwd, fx, model))       # (the model owns gm5)
    return out


def test_streams_agree_with_serial_as_two_serial_seeds_agree(oracle_matrices):
    for name, M, L, tsc, fwd, fx, _ in oracle_matrices:
        s42 = ba.fs_ensemble_serial(M, tsc, XNL, XNM, XE, 1, L, fwd, fx, seed=42)
        s43 = ba.fs_ensemble_serial(M, tsc, XNL, XNM, XE, 1, L, fwd, fx, seed=43)
        assert len(s42) == 2, (name, s42)                    # the two copies
        assert len(s43) == len(s42) and all(overlap_ok(a, b) for a, b in zip(s42, s43)), (name, s42, s43)     # the premise
        r = ba.fs_ensemble_streams(M, tsc, XNL, XNM, XE, 1, L, fwd, fx, seed=42)
        assert r["status"] == ba.ENS_REGION_OK and not r["trace_status"].any()
        got = r["envelopes"]
        print(name, L, "serial(42)", s42, "serial(43)", s43, "streams(42)", got)
        assert len(got) == len(s42), (name, got, s42)
        assert all(overlap_ok(a, b) for a, b in zip(got, s42)), (name, got, s42)
        # trace 0 starts where the serial stream starts, but its expf / logf are the walk's own: no bit-for-bit claim, only sanity --
        # every trace has at least one segment inside the window and nodes inside the model
        seg = r["segments"]
        assert set(seg[:, 0]) == set(range(200))
        assert (seg[:, 1] >= 1).all() and (seg[:, 2] <= L).all() and (seg[:, 1] <= seg[:, 2]).all()
        assert (seg[:, 3] >= 1).all() and (seg[:, 4] <= M).all() and (seg[:, 3] <= seg[:, 4]).all()
