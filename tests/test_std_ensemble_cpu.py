"""CPU tier: the ensemble modes of the standard branch's multi-domain regions (bath_hip_set_std_ensemble), host side.

Mode 0 (serial) is the code path the pipeline has always run: here it is held against the oracle's restatement of
region_trace_ensemble / p7_StochasticTrace (oracle/stotrace.c) on the oracle's own multihit Forward matrix of the region --
envelopes and per-residue null2 scores.  Mode 1 (a stream per trace) is the host twin of std_ensemble_kernel: its trace t must be
the walk started from the generator stepped t * 2^20 times one step at a time, and its envelopes can agree with mode 0's only the
way two seeds of mode 0 agree, which the test checks first (the criterion of tests/test_fs_ensemble_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import bath_amd as ba
from bath_amd import synth
import oracle_lib as ol

f32p = C.POINTER(C.c_float)


def consensus_region(hmm, seed, copies, spacer):
    """flank + consensus + (<spacer> random residues + consensus) * (copies - 1) + flank, in amino-acid codes."""
    rng = np.random.default_rng(seed)
    aa = synth.hmm_match_emissions(hmm)[1:].argmax(axis=1).astype(np.uint8)
    rnd = lambda n: rng.integers(0, 20, size=n, dtype=np.uint8)
    parts = [rnd(12), aa]
    for _ in range(copies - 1):
        parts += [rnd(spacer), aa]
    return np.concatenate(parts + [rnd(12)])


# (model, region seed, copies, spacer)
REGIONS = [("PTH2.bhmm", 11, 2, 40), ("PTH2.bhmm", 12, 3, 25), ("Caudal_act.bhmm", 21, 2, 30), ("Caudal_act.bhmm", 22, 3, 18)]


@pytest.fixture(scope="module")
def cases():
    """Per region: the oracle's tables and its p7_Forward of the region (multihit, configured for the region's length), computed once."""
    L_ = ol.lib()
    L_.bo_forward_full.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.POINTER(ol.OProfile), f32p, f32p, f32p]
    L_.bo_forward_full.restype = C.c_int
    L_.bo_oprofile_reconfig_multihit.argtypes = [C.POINTER(ol.OProfile), C.c_int]
    out = []
    for name, rseed, copies, spacer in REGIONS:
        path = ol.GOLDEN + "/" + name
        model = ol.Model(path, 0)
        hmm = ba.HMM(path, 0)
        M = model.M
        res = consensus_region(hmm, rseed, copies, spacer)
        n = len(res)
        L_.bo_oprofile_reconfig_multihit(model.om, n)
        om = model.om.contents
        fwd = np.zeros((n + 1) * (M + 1) * 3, np.float32); fx = np.zeros((n + 1) * 6, np.float32)
        sc = C.c_float()
        dsq = ol.dsq_from(res)
        assert L_.bo_forward_full(ol.u8(dsq), n, model.om, fwd.ctypes.data_as(f32p), fx.ctypes.data_as(f32p), C.byref(sc)) == 0
        tf = np.ctypeslib.as_array(om.tf, shape=((M + 1) * 8,)).astype(np.float32).copy()
        rf = np.ctypeslib.as_array(om.rf, shape=(20 * (M + 1),)).astype(np.float32).copy()
        tabs = dict(M=M, tf=tf, rf=rf, pmove=float(om.xf[1][1]), tEL=float(om.xf[0][0]), tEM=float(om.xf[0][1]))
        out.append(dict(name=name, copies=copies, model=model, dsq=dsq, res=res, fwd=fwd, fx=fx, tabs=tabs))
    return out


def run(mode, c, seed=42):
    t = c["tabs"]
    return ba.std_ensemble_host(mode, t["M"], t["tf"], t["rf"], t["pmove"], t["tEL"], t["tEM"], c["res"], c["fwd"], c["fx"], seed=seed)


def overlap_ok(a, b):
    """The project's own link criterion (cluster_segments: min_overlap): shared residues >= 0.8 of the shorter envelope."""
    nov = min(a[1], b[1]) - max(a[0], b[0]) + 1
    return nov / min(a[1] - a[0] + 1, b[1] - b[0] + 1) >= 0.8


@pytest.mark.parametrize("seed", [42, 7])
def test_serial_mode_equals_the_oracles_ensemble(cases, seed):
    """Mode 0 on the oracle's matrix: the oracle's envelopes, and its null2 scores.  Both sum a domain's null2 over the nodes in
    ascending order (the product skips the nodes whose count is zero, which adds nothing), so the scores are the same floats."""
    L_ = ol.lib()
    L_.bo_region_trace_ensemble.restype = C.c_int
    L_.bo_region_trace_ensemble.argtypes = [C.POINTER(ol.OProfile), C.POINTER(C.c_uint8), C.c_int, C.c_int, f32p, f32p, f32p, C.POINTER(C.c_int), C.c_int]
    L_.bo_set_seed(seed)
    try:
        for c in cases:
            n = len(c["res"])
            n2 = np.zeros(n + 2, np.float32)
            oenv = (C.c_int * 64)()
            nc = L_.bo_region_trace_ensemble(c["model"].om, ol.u8(c["dsq"]), 1, n, c["fwd"].ctypes.data_as(f32p), c["fx"].ctypes.data_as(f32p),
                                             n2.ctypes.data_as(f32p), oenv, 32)
            assert nc == c["copies"], (c["name"], nc)                 # the planted copies come out as that many envelopes
            r = run("serial", c, seed)
            assert r["status"] == ba.ENS_REGION_OK
            assert r["envelopes"] == [(oenv[2 * e], oenv[2 * e + 1]) for e in range(nc)], c["name"]
            assert np.array_equal(r["n2sc"], n2[1:n + 1]), (c["name"], np.abs(r["n2sc"] - n2[1:n + 1]).max())
            assert len(r["segments"]) == 0 and not r["trace_status"].any()      # the serial walk keeps neither
    finally:
        L_.bo_set_seed(42)


@pytest.mark.parametrize("seed", [42, 1])
def test_stream_mode_trace_t_is_the_walk_from_the_stepped_generator(cases, seed):
    """Trace t of mode 1 starts t * 2^20 steps into the region's generator.  The states come from stepping the generator one draw at a
    time (value n of the stream is state(n) / 2^32), not from the jump-ahead the mode itself uses."""
    T = 4
    n = (T - 1) * (1 << 20) + 1
    out = np.zeros(n, np.float64)
    assert ba.lib().bath_selftest_rng_stream(seed, n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    states = [ba.rng_jump(seed, 0)] + [int(out[(t << 20) - 1] * 4294967296.0) for t in range(1, T)]
    for c in cases:
        r = run("streams", c, seed)
        assert r["status"] == ba.ENS_REGION_OK and not r["trace_status"].any()
        seg = r["segments"]
        t_ = c["tabs"]
        for t in range(T):
            st, segs = ba.std_ens_walk(t_["M"], t_["tf"], t_["pmove"], t_["tEL"], t_["tEM"], len(c["res"]), c["fwd"], c["fx"], states[t])
            assert st == ba.ENS_OK
            assert [tuple(int(v) for v in g[1:]) for g in seg[seg[:, 0] == t]] == segs, (c["name"], t)
        assert len({tuple(map(tuple, seg[seg[:, 0] == t][:, 1:])) for t in range(T)}) > 1 or c["tabs"]["M"] < 3    # the slices do differ


def test_stream_mode_agrees_with_serial_as_two_serial_seeds_agree(cases):
    for c in cases:
        s42, s43 = run("serial", c, 42)["envelopes"], run("serial", c, 43)["envelopes"]
        assert len(s42) == c["copies"], (c["name"], s42)
        assert len(s43) == len(s42) and all(overlap_ok(a, b) for a, b in zip(s42, s43)), (c["name"], s42, s43)     # the premise
        r = run("streams", c, 42)
        got = r["envelopes"]
        print(c["name"], len(c["res"]), "serial(42)", s42, "serial(43)", s43, "streams(42)", got)
        assert len(got) == len(s42), (c["name"], got, s42)
        assert all(overlap_ok(a, b) for a, b in zip(got, s42)), (c["name"], got, s42)
        seg, L, M = r["segments"], len(c["res"]), c["tabs"]["M"]
        assert set(seg[:, 0]) == set(range(200))
        assert (seg[:, 1] >= 1).all() and (seg[:, 2] <= L).all() and (seg[:, 1] <= seg[:, 2]).all()
        assert (seg[:, 3] >= 1).all() and (seg[:, 4] <= M).all() and (seg[:, 3] <= seg[:, 4]).all()
        assert np.isfinite(r["n2sc"]).all()


def test_region_outside_the_stream_rule_is_refused():
    """4 (4 (Lr + M) + 64) >= 2^20: a trace could run into the next trace's slice.  The twin answers ERANGE before it reads anything
    (the pipeline then runs the serial ensemble and counts the region)."""
    M, Lr = 1, 65520
    z = np.zeros(40, np.float32)
    rs, ns, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    res = np.zeros(Lr, np.uint8)
    st = ba.lib().bath_selftest_std_ensemble(1, M, ba._f32(z), ba._f32(z), 0.5, 0.5, 0.5, ba._u8(res), Lr, ba._f32(z), ba._f32(z), 42, C.byref(rs), None, None, 0,
                                             C.byref(ns), None, None, 0, C.byref(ne))
    assert st == ba.ERANGE


def test_cli_refuses_an_unknown_mode(tmp_path, monkeypatch, capsys):
    """--ensemble-std takes serial, streams or device; anything else is a usage error that says so, before any GPU is opened."""
    import io
    import shutil
    from bath_amd import bathsearch
    monkeypatch.chdir(tmp_path)
    for f in ("AMP_N.bhmm", "target-AMP_N.fa"):
        shutil.copy(ol.GOLDEN + "/" + f, tmp_path / f)
    assert bathsearch.run(["--ensemble-std", "sideways", "AMP_N.bhmm", "target-AMP_N.fa"], stdout=io.StringIO()) == 1
    assert "option --ensemble-std: expected serial, streams or device" in capsys.readouterr().err
    opts, _, _ = bathsearch.parse_args(["--ensemble-std", "device", "AMP_N.bhmm", "target-AMP_N.fa"])
    assert opts["--ensemble-std"] == "device"
