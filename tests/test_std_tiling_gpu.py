"""The standard branch's envelope kernels (bath_amd/csrc/bath_std_domains.hip) at every instantiation, matrix by matrix.

std_envelope_fill_kernel<C> (a wave per envelope, C = 1, 2, 3, 4, 6, 8, 12, 16 nodes per lane), std_envelope_fill_mw_kernel<C> (a block
of four waves, C = 1, 2, 4) and the lane-per-envelope std_envelope_kernel each do p7_Decoding, p7_OptimalAccuracy and
p7_Null2_ByExpectation on an envelope.  bath_hip_std_envelopes_fill runs any of the three on the same envelopes and returns what the
stage's traceback reads: the posteriors, the optimal-accuracy matrix and their special-state rows.  Every cell is held against the
oracle's restatement (oracle/domaindef.c, bo_std_envelope_matrices), and the three paths against each other bit for bit.

STD_M holds the smallest and the largest model of every instantiation of both fill kernels; tests/test_tiling_coverage_cpu.py reads
the instantiations from the source and fails when one has no model here.  tests/test_std_tiling_cpu.py checks, with the oracle alone,
that the inputs do what they are meant to (traces with M, D and I states, deletions at the holes, a domain in every long ORF).

Bounds, from the suite's own rules and not from what the kernels return:
  * Forward and Backward scores: 1e-4 relative (tests/test_filters_gpu.py);
  * a posterior is a product of a Forward value, a Backward value (1e-4 each) and a scale: 3e-4 pp + 1e-6;
  * an optimal-accuracy cell and oasc are sums of posteriors: 2e-3 + 1e-3 |value| (tests/test_hits_gpu.py); -inf where the oracle has it;
  * null2: the same 2e-3 + 1e-3 |value|;
  * across the paths: everything identical but null2, whose sum over the M nodes associates by lane and wave: 2 M 2^-24 relative.
The largest discrepancy per model and path goes to std_tiling_ledger.json, beside the ledger of tests/test_hits_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bath_amd as ba
import common
import oracle_lib as ol

pytestmark = pytest.mark.gpu

STD_FILL_COLUMNS = [1, 2, 3, 4, 6, 8, 12, 16]          # std_envelope_fill_kernel<C>
STD_FILL_MW_COLUMNS = [1, 2, 4]                        # std_envelope_fill_mw_kernel<C>
STD_M = [1, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1024]
STD_FILL_MAX_NODES = 1024
ENV_LENGTHS = [1, 2, 63, 64, 65, 128, 129]             # the fill kernels fetch the special-state rows 64 at a time
# (c) the paths through the pipeline: M -> the BATH_HIP_STD_FILL_MW settings to run besides the default
PIPELINE_M = {64: [], 256: ["0"], 768: ["0"], 1025: [], 2048: []}
# (b) M -> (nodes without m->d and d->d, nodes without m->i and i->i)
HOLE_MODELS = {70: ([5, 31, 32, 33, 34, 64], [20, 48]),
               200: ([4, 5, 128, 129, 199], [60, 150]),
               520: ([12, 13, 256, 257, 260, 519], [100, 400])}
# (d) residues of the one ORF of a window: std_regions_wave_kernel in 64 KiB of LDS, beyond 64 KiB, and std_regions_kernel
REGION_RESIDUES = [1000, 4200, 8300]
REGION_MODEL = "PTH2.bhmm"

T_M, T_D, T_I = 3, 4, 5                                # BO_T_M / D / I of the oracle's traces
_f32p, _i32p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
fp = lambda a: a.ctypes.data_as(_f32p)
ip = lambda a: a.ctypes.data_as(_i32p)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the oracle's side (no GPU: tests/test_std_tiling_cpu.py uses these too)
# ---------------------------------------------------------------------------------------------------------------------------------
def background(rng, n):
    return rng.choice(20, size=n, p=common.BG / common.BG.sum()).astype(np.uint8)


def fit(rng, s, n):
    """<s> cut (its middle) or padded with background (both sides) to n residues."""
    if len(s) >= n:
        a = (len(s) - n) // 2
        return s[a:a + n].copy()
    left = (n - len(s)) // 2
    return np.concatenate([background(rng, left), s, background(rng, n - len(s) - left)]).astype(np.uint8)


def tiling_envelopes(model, M):
    """The nine envelopes of a model: homologs cut or padded to ENV_LENGTHS, one of about M + 20 residues (at most 400 from 385 nodes
    on, for the oracle's time) and 100 residues of background."""
    rng = np.random.default_rng(1000 + M)
    genes = common.emit_from_model(rng, model, len(ENV_LENGTHS) + 1, flank=5, sharpen=2.0)
    envs = [fit(rng, g, n) for g, n in zip(genes, ENV_LENGTHS)]
    envs.append(fit(rng, genes[-1], min(M + 20, 400) if M >= 385 else M + 20))
    envs.append(background(rng, 100))
    return envs


def punch_holes(src, dst, d_nodes, i_nodes):
    """A copy of the model file <src> in which the nodes d_nodes have no m->d and no d->d (d->m = 1) and the nodes i_nodes no m->i
    and no i->i (i->m = 1); the other match transitions are renormalised.  Lines of a node: emissions, insert emissions, transitions
    m->m m->i m->d i->m i->i d->m d->d."""
    lines = open(src).read().split("\n")
    base = next(i for i, l in enumerate(lines) if l.startswith("HMM ")) + 2      # COMPO, insert, transitions of node 0; then 3 per node
    for k in sorted(set(d_nodes) | set(i_nodes)):
        f = lines[base + 3 * k + 2].split()
        assert len(f) == 7
        p = [0.0 if x == "*" else float(np.exp(-float(x))) for x in f]
        if k in d_nodes:
            p[2], p[5], p[6] = 0.0, 1.0, 0.0
        if k in i_nodes:
            p[1], p[3], p[4] = 0.0, 1.0, 0.0
        tot = p[0] + p[1] + p[2]
        p[0], p[1], p[2] = p[0] / tot, p[1] / tot, p[2] / tot
        lines[base + 3 * k + 2] = "          " + "  ".join("%.5f" % (-np.log(v) + 0.0) if v > 0 else "      *" for v in p)
    with open(dst, "w") as fh:
        fh.write("\n".join(lines))
    return dst


def hole_envelopes(model, M, d_nodes):
    """Homologs of the whole model that lack the nodes just before and at a hole: the alignment has to run D ... D(hole) -> M, the
    only way out of a node without d->d.  The run of skipped nodes starts after the previous hole (no m->d there) and is at most
    three nodes long; a hole right behind another one cannot be deleted at all.  Plus 100 residues of background."""
    rng = np.random.default_rng(2000 + M)
    h = model.hmm.contents
    mat = np.ctypeslib.as_array(h.mat, shape=((M + 1) * 20,)).reshape(M + 1, 20)
    runs = []
    for d in d_nodes:
        if d - 1 in d_nodes or d < 2:
            continue
        start = d
        while d - start < 2 and start - 1 >= 2 and start - 2 not in d_nodes:
            start -= 1
        runs.append(set(range(start, d + 1)))
    envs = []
    for q in range(8):
        skip = set().union(*[r for z, r in enumerate(runs) if (z + q) % 2 == 0 or len(runs) < 3])
        core = []
        for k in range(1, M + 1):
            if k in skip:
                continue
            p = mat[k].astype(np.float64) ** 2.0
            core.append(rng.choice(20, p=p / p.sum()))
        envs.append(np.concatenate([background(rng, int(rng.integers(0, 8))), np.array(core, np.uint8), background(rng, int(rng.integers(0, 8)))]).astype(np.uint8))
    envs.append(background(rng, 100))
    return envs


def oracle_envelope(model, s):
    """bo_std_envelope_matrices and bo_std_envelope_trace on one envelope: a dict of the hook's arrays, ok (decoding in range and a
    trace) and trace [(state, node, residue)] from the last column to the first."""
    L_ = ol.lib()
    M, L = model.M, len(s)
    d = ol.dsq_from(s)
    L_.bo_std_envelope_matrices.argtypes = [C.POINTER(ol.OProfile), _u8p, C.c_int] + [_f32p] * 10
    L_.bo_std_envelope_matrices.restype = C.c_int
    L_.bo_std_envelope_trace.argtypes = [C.POINTER(ol.OProfile), _u8p, C.c_int, _i32p, _i32p, _i32p, _f32p]
    o = {"sc": np.zeros(3, np.float32), "pp": np.zeros((L + 1, M + 1, 3), np.float32), "ppx": np.zeros((L + 1, 5), np.float32),
         "oa": np.zeros((L + 1, M + 1, 3), np.float32), "ox": np.zeros((L + 1, 5), np.float32), "null2": np.zeros(ol.KP, np.float32),
         "fwd": np.zeros((L + 1, M + 1, 3), np.float32), "bck": np.zeros((L + 1, M + 1, 3), np.float32),
         "fx": np.zeros((L + 1, 6), np.float32), "bx": np.zeros((L + 1, 6), np.float32)}
    st = L_.bo_std_envelope_matrices(model.om, ol.u8(d), L, fp(o["sc"]), fp(o["pp"]), fp(o["ppx"]), fp(o["oa"]), fp(o["ox"]), fp(o["null2"]),
                                     fp(o["fwd"]), fp(o["bck"]), fp(o["fx"]), fp(o["bx"]))
    pst, pk, pi_ = (np.zeros(L + M + 8, np.int32) for _ in range(3))
    oasc = np.zeros(1, np.float32)
    pn = L_.bo_std_envelope_trace(model.om, ol.u8(d), L, ip(pst), ip(pk), ip(pi_), fp(oasc))
    o["trace"] = [(int(pst[z]), int(pk[z]), int(pi_[z])) for z in range(max(pn, 0))]
    o["ok"] = st == 0 and pn > 0 and any(t[0] == T_M for t in o["trace"])
    assert st != 0 or pn < 0 or bits(oasc)[0] == bits(o["sc"][2:])[0]                    # the two hooks are the same passes
    return o


_ORACLE = {}


def oracle_envelopes(key, model, envs):
    """The oracle's side of a model's envelopes, computed once per session and left unchanged."""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle_envelope(model, s) for s in envs]
    return _ORACLE[key]


def assert_tiling_inputs(M, ref):
    """Non-vacuity of (a): at least seven of the nine envelopes give a domain, and from 64 nodes on their traces hold M, D and I."""
    good = [o for o in ref if o["ok"] and np.isfinite(o["pp"]).all()]                  # (see check_paths on envelopes that overflow)
    assert len(good) >= 7, [o["ok"] for o in ref]
    kinds = {t[0] for o in good for t in o["trace"]}
    assert T_M in kinds and (M < 64 or kinds >= {T_M, T_D, T_I}), (M, kinds)


def assert_hole_inputs(M, ref):
    """Non-vacuity of (b): some trace deletes a hole node (it entered D behind the hole's predecessor and leaves through d->m = 1),
    and most envelopes give a domain."""
    d_nodes = HOLE_MODELS[M][0]
    deleted = {k for o in ref if np.isfinite(o["pp"]).all() for st, k, _ in o["trace"] if st == T_D and k in d_nodes}
    assert deleted, "no trace has a delete state at a hole of the %d-node model" % M
    assert sum(o["ok"] and bool(np.isfinite(o["pp"]).all()) for o in ref) >= 7
    return deleted


def synthetic(tmp, M, holes=None):
    path = common.write_synthetic_bhmm(os.path.join(str(tmp), "std%d.bhmm" % M), M, seed=M)
    if holes:
        path = punch_holes(path, os.path.join(str(tmp), "std%d_holes.bhmm" % M), *holes)
    return path


def pipeline_windows(model, M):
    """8 planted genes, on either strand, and 4 windows of background.  Beyond the fill kernels' range one lane fills an envelope
    cell by cell: the genes are cut to 250 residues there to keep the case to a few seconds."""
    rng = np.random.default_rng(3000 + M)
    wins = []
    for i, aa in enumerate(common.emit_from_model(rng, model, 8, flank=4, sharpen=2.0)):
        if M > STD_FILL_MAX_NODES:
            aa = fit(rng, aa, min(len(aa), 250))
        nt = np.array(common.revtranslate(rng, aa, model.basic), dtype=np.uint8)
        w = np.concatenate([rng.integers(0, 4, size=45).astype(np.uint8), nt, rng.integers(0, 4, size=30).astype(np.uint8)])
        wins.append((3 - w[::-1]).astype(np.uint8) if i % 2 else w)
    return wins + common.random_dna(rng, 4, 900)


def region_window(model, residues):
    """One stop-free reading frame of <residues> codons on the top strand: background with two genes planted in it."""
    rng = np.random.default_rng(4000 + residues)
    g = common.emit_from_model(rng, model, 2, flank=1, sharpen=2.0)
    rest = residues - len(g[0]) - len(g[1])
    a, b = rest // 4, rest // 2
    aa = np.concatenate([background(rng, a), g[0], background(rng, b), g[1], background(rng, rest - a - b)])
    assert len(aa) == residues
    return np.array(common.revtranslate(rng, aa, model.basic), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU's side
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    return ba.Context(0)


LEDGER = {}
PATHS = {ba.STD_FILL_SERIAL: "serial", ba.STD_FILL_WAVE: "wave", ba.STD_FILL_BLOCK: "block"}


def _write_ledger():
    """std_tiling_ledger.json, beside the standard branch's other ledger (test_hits_gpu)."""
    import test_hits_gpu
    test_hits_gpu._write_ledger("std_tiling_ledger.json", LEDGER)


def worst(got, want, rel, abs_):
    """Largest |got - want| over the finite cells, and the largest ratio of a difference to its bound rel |want| + abs_."""
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(got[~fin], want[~fin], equal_nan=True), "-inf (or another non-finite value) on one side only"
    if not fin.any():
        return 0.0, 0.0
    diff = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    return float(diff.max()), float((diff / (rel * np.abs(want[fin].astype(np.float64)) + abs_)).max())


def check_paths(ctx, path, model, envs, ref, label):
    """Every fill path on <envs> against the oracle's <ref>, then the paths against each other."""
    M = model.M
    hmm = ba.HMM(path)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    blk = ba.SeqBlock(ctx, envs)
    runs = {}
    for fill, name in PATHS.items():
        res, pp, oa, ppx, oax = ba.StdEnvelopes(ctx, om, blk, fill)
        runs[fill] = (res, pp, oa, ppx, oax)
        led = {"pp": 0.0, "pp_over_bound": 0.0, "oa": 0.0, "oa_over_bound": 0.0, "null2": 0.0, "null2_over_bound": 0.0, "score_rel": 0.0, "envelopes_ok": 0, "envelopes_overflowed": 0}
        fails = []
        for e, o in enumerate(ref):
            r = res[e]
            assert bool(r.ok) == bool(o["ok"]), (label, name, e, r.ok, o["ok"])
            for g, w in ((r.fwdsc, o["sc"][0]), (r.bcksc, o["sc"][1])):
                rel = abs(g - float(w)) / max(1.0, abs(float(w)))
                led["score_rel"] = max(led["score_rel"], rel)
                if rel > 1e-4:
                    fails.append((e, "score", g, float(w)))
            if not o["ok"]:
                continue
            led["envelopes_ok"] += 1
            # An envelope on which the reference's own arithmetic leaves its range -- Backward's N row down in the denormals, so that
            # Forward and Backward no longer agree and posteriors overflow to inf and 0 * inf -- has no optimal-accuracy matrix to
            # speak of: a maximum over NaN is whatever the instruction makes of it (maxps, a C comparison, v_max_f32).  Its posteriors
            # are still cell-wise products and must agree, non-finite cells included; the rest is held across the paths only, below.
            overflowed = not np.isfinite(o["pp"]).all()
            led["envelopes_overflowed"] += int(overflowed)
            null2 = np.array(r.null2[:], np.float32)
            cells = (("pp", np.concatenate([pp[e][1:, 1:, :].ravel(), ppx[e].ravel()]), np.concatenate([o["pp"][1:, 1:, :].ravel(), o["ppx"].ravel()]), 3e-4, 1e-6),
                     ("oa", np.concatenate([oa[e].ravel(), oax[e].ravel(), np.float32([r.oasc])]), np.concatenate([o["oa"].ravel(), o["ox"].ravel(), o["sc"][2:]]), 1e-3, 2e-3),
                     ("null2", null2, o["null2"], 1e-3, 2e-3))
            for what, g, w, rel, abs_ in cells[:1] if overflowed else cells:
                d, ratio = worst(g, w, rel, abs_)
                led[what] = max(led[what], d)
                led[what + "_over_bound"] = max(led[what + "_over_bound"], ratio)
                if ratio > 1.0:
                    fails.append((e, what, d, ratio))
        LEDGER.setdefault(label, {})[name] = led
        _write_ledger()
        print("std tiling %s %-6s %s" % (label, name, json.dumps(led)))
        assert not fails, (label, name, fails)
    base = runs[ba.STD_FILL_SERIAL]
    for fill in (ba.STD_FILL_WAVE, ba.STD_FILL_BLOCK):
        res, pp, oa, ppx, oax = runs[fill]
        for e in range(len(envs)):
            a, b = base[0][e], res[e]
            assert (a.ok, a.fwd_status, a.bck_status) == (b.ok, b.fwd_status, b.bck_status)
            assert np.array_equal(bits([a.fwdsc, a.bcksc]), bits([b.fwdsc, b.bcksc])), (label, PATHS[fill], e)
            if not a.ok:
                continue
            cells = (("pp", base[1][e][1:, 1:, :], pp[e][1:, 1:, :]), ("ppx", base[3][e], ppx[e]), ("oa", base[2][e], oa[e]), ("oax", base[4][e], oax[e]))
            if not np.isfinite(base[1][e][1:, 1:, :]).all():
                # posteriors out of range (see above): the lane kernel's fmaxf and the fill kernels' v_max_f32 / v_min_f32 and bit
                # masks do not treat a NaN operand alike, so only the posteriors, products by one expression, are held to the bit
                cells = cells[:2]
            else:
                assert bits([a.oasc])[0] == bits([b.oasc])[0], (label, PATHS[fill], e, a.oasc, b.oasc)
            for what, x, y in cells:
                same = bits(x) == bits(y)
                assert same.all(), (label, PATHS[fill], e, what, "first differing cell", tuple(int(v[0]) for v in np.nonzero(~same)))
            if len(cells) == 2:
                continue
            na, nb = np.array(a.null2[:], np.float64), np.array(b.null2[:], np.float64)
            fin = np.isfinite(na)
            assert np.array_equal(fin, np.isfinite(nb)) and np.array_equal(na[~fin], nb[~fin], equal_nan=True), (label, PATHS[fill], e, na, nb)
            assert (np.abs(na[fin] - nb[fin]) <= 2.0 * M * 2.0 ** -24 * np.abs(na[fin])).all(), (label, PATHS[fill], e, na, nb)


@pytest.mark.parametrize("M", STD_M)
def test_every_fill_tiling_against_the_oracle(ctx, tmp_path, M):
    """(a) Both ends of every instantiation of both fill kernels, and the lane kernel, on nine envelopes whose lengths sit on the edges
    of the 64-row chunks of the special-state rows; nine envelopes are more than the four waves of a block, so the one-wave kernel's
    packing and grid stride run too."""
    path = synthetic(tmp_path, M)
    model = ol.Model(path, 0)
    envs = tiling_envelopes(model, M)
    ref = oracle_envelopes(("tiling", M), model, envs)
    assert_tiling_inputs(M, ref)
    check_paths(ctx, path, model, envs, ref, "M=%d" % M)


@pytest.mark.parametrize("M", sorted(HOLE_MODELS))
def test_interior_zero_transitions(ctx, tmp_path, M):
    """(b) Nodes inside the model without d->d and m->d -- the D chain's non-pass branch (npz, plim, fpass) at a lane's last node, the
    next lane's first, mid-lane, and either side of a wave of the block kernel -- and nodes without m->i and i->i."""
    path = synthetic(tmp_path, M, HOLE_MODELS[M])
    model = ol.Model(path, 0)
    envs = hole_envelopes(model, M, HOLE_MODELS[M][0])
    ref = oracle_envelopes(("holes", M), model, envs)
    assert_hole_inputs(M, ref)
    check_paths(ctx, path, model, envs, ref, "holes M=%d" % M)


def test_fill_entry_refuses_what_it_cannot_run(ctx, tmp_path):
    """Beyond 1024 nodes there is no fill kernel: BATH_ERANGE with a message for fill 1 and 2 (the lane kernel runs), BATH_EINVAL for
    a fill that does not exist."""
    path = synthetic(tmp_path, 1025)
    om = ba.OProfile(ctx, ba.Profile(ba.HMM(path)))
    blk = ba.SeqBlock(ctx, [background(np.random.default_rng(0), 12)])
    res = ba.StdEnvelopes(ctx, om, blk, ba.STD_FILL_SERIAL)[0]
    assert res[0].ok in (0, 1)
    for fill in (ba.STD_FILL_WAVE, ba.STD_FILL_BLOCK):
        with pytest.raises(ba.BathError, match="1024 nodes"):
            ba.StdEnvelopes(ctx, om, blk, fill)
    r = (ba.StdResult * 1)()
    assert ba.lib().bath_hip_std_envelopes_fill(ctx._h, om._h, blk._h, r, None, None, None, None, 3) == ba.EINVAL


def hit_fields(dm):
    return sorted((d.window, d.ienv, d.jenv, d.iali, d.jali, d.ihmm, d.jhmm, d.envsc, d.oasc, d.ali_columns, d.pid, d.cigar, d.domcorrection) for d in dm)


def assert_same_hits(a, b):
    """test_hits_gpu.test_wave_and_lane_envelope_kernels_agree's comparison: every field identical, the null2 correction to the
    association of one sum."""
    assert a[0] == b[0] and len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x[:12] == y[:12]
        assert abs(x[12] - y[12]) <= 1e-4 * max(1.0, abs(y[12]))


@pytest.mark.parametrize("M", sorted(PIPELINE_M))
def test_fill_paths_through_the_pipeline(ctx, monkeypatch, tmp_path, M):
    """(c) std_domains' own choice of kernel at 64 (one wave), 256 and 768 (the block kernel; BATH_HIP_STD_FILL_MW=0: one wave, 4 and
    12 nodes per lane), and the lane kernel doing everything at 1025 and at the cascade's last model, 2048: hits against the
    oracle, and each choice against BATH_HIP_STD_SERIAL=1."""
    from test_hits_gpu import compare_hits
    path = synthetic(tmp_path, M)
    model = ol.Model(path, 0)
    wins = pipeline_windows(model, M)
    pli, odm, per_d, onskip = model.run_pipeline_hits(wins)
    hmm = ba.HMM(path)
    om = ba.OProfile(ctx, ba.Profile(hmm))

    def run(serial, mw, lane=None):
        monkeypatch.setenv("BATH_HIP_STD_SERIAL", serial)
        for name, v in (("BATH_HIP_STD_FILL_MW", mw), ("BATH_HIP_STD_TRACE_LANE", lane)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        pipe = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct)
        stats, dm, nskip = pipe.run_hits(ba.SeqBlock(ctx, wins))
        return stats, dm, nskip, pipe.traces()

    stats, dm, nskip, tr = run("0", None)
    assert (stats.n_past_fwd, stats.pos_past_fwd) == (pli.n_past_fwd, pli.pos_past_fwd)
    assert compare_hits(dm, odm, per_d, nskip, onskip) >= 3
    serial = run("1", None)
    assert_same_hits((nskip, hit_fields(dm)), (serial[2], hit_fields(serial[1])))
    for mw in PIPELINE_M[M]:
        _, dm2, nskip2, _ = run("0", mw)
        assert compare_hits(dm2, odm, per_d, nskip2, onskip) >= 3
        assert_same_hits((nskip2, hit_fields(dm2)), (serial[2], hit_fields(serial[1])))
    if M > STD_FILL_MAX_NODES:
        # no fill kernel: the wave traceback needs one, so both settings of BATH_HIP_STD_TRACE_LANE must take the lane kernel
        for lane in ("0", "1"):
            _, dm3, nskip3, tr3 = run("0", None, lane)
            assert nskip3 == nskip and hit_fields(dm3) == hit_fields(dm) and len(tr3) == len(tr) >= 3
            for (t1, st1, k1, i1, c1, pp1), (t2, st2, k2, i2, c2, pp2) in zip(tr, tr3):
                assert (t1.N, t1.win_start, t1.orf_start) == (t2.N, t2.win_start, t2.orf_start)
                assert np.array_equal(st1, st2) and np.array_equal(k1, k2) and np.array_equal(i1, i2) and np.array_equal(bits(pp1), bits(pp2))


@pytest.mark.parametrize("residues", REGION_RESIDUES)
def test_region_kernel_lds_tiers(ctx, monkeypatch, residues):
    """(d) std_regions_wave_kernel keeps four rows of an ORF in LDS: 16 (L + 1) bytes.  1000 residues fit the default 64 KiB, 4200
    need the raised limit, 8300 are beyond 128 KiB and go to std_regions_kernel.  Each is a window of its own (the longest ORF of a
    block decides for all of it); hits and clustered regions against the oracle, and the same from BATH_HIP_STD_SERIAL=1."""
    from test_hits_gpu import compare_hits
    path = ol.GOLDEN + "/" + REGION_MODEL
    model = ol.Model(path, 0)
    wins = [region_window(model, residues)]
    pli, odm, per_d, onskip = model.run_pipeline_hits(wins)
    assert len(odm) >= 1
    hmm = ba.HMM(path)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    out = []
    for serial in ("0", "1"):
        monkeypatch.setenv("BATH_HIP_STD_SERIAL", serial)
        stats, dm, nskip = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct).run_hits(ba.SeqBlock(ctx, wins))
        assert (stats.n_past_fwd, stats.pos_past_fwd) == (pli.n_past_fwd, pli.pos_past_fwd)
        assert compare_hits(dm, odm, per_d, nskip, onskip) >= 1
        out.append((nskip, hit_fields(dm)))
    assert_same_hits(out[0], out[1])
    assert [h[:3] for h in out[0][1]] == [h[:3] for h in out[1][1]]                   # identical regions: the same envelopes
