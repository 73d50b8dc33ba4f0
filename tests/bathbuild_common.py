"""The CPU path of single-sequence model calibration that the bathbuild tests share: the library's sampler and fits around the ORACLE's
MSV filter, Viterbi filter and Forward parser (bo_msvfilter, bo_vitfilter, bo_forward_parser on the profile reconfigured to the
sample length) and, for the frameshift taus, calib_common's two Forward recursions -- p7_Calibrate (evalues.c:64-199) with the
generator seeded per model (evalues.c:94-95).  The model goes to the oracle as it lies in memory: bath_hmm and bo_hmm share their
leading fields.  Results are cached per (fixture, record, calibration sizes): computed once, shared by the CPU and the GPU tests,
never changed."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

import bath_amd as ba
import oracle_lib as ol
from bath_amd import bathbuild as bb

LN2 = 0.69314718055994529
DEFAULT_E = (200, 200, 200, 200, 100, 200, 0.04)                  # EmL EmN EvL EvN EfL EfN Eft
ODD_E = (50, 70, 33, 65, 20, 129, 0.04)                           # counts that differ between sets and are no multiple of a wave
FIXTURES = {"AMP_N": ("AMP_N.fa", "AMP_N.bhmm"), "three_seqs": ("three_seqs.fa", "three_seqs.bhmm.lines")}
# The reference's tutorial/three_seqs.bhmm (three models, 483 384 bytes) is not committed whole: apart from its DATE and STATS lines
# it is what the library writes, so tests/golden/three_seqs.bhmm.lines holds those 18 lines, and the text the library writes with them
# put in is held to the original's size and SHA-256, whole and per model.  A mismatch is located by the SHA-256 prefixes of the original's
# consecutive 64-line chunks (first_differing_chunk).  Its MAXL lines, read off the original.
THREE_SEQS = {"bytes": 483384, "sha256": "109acb9e6c638b52f309b50d164b47545a1e03fe4e920ec65322d84ff8711011",
              "models": [(200653, "6d6a75bbf3a736b7cb45a7b8dcd221d8b57def37dd77c1344b1cf2524c25944c"),
                         (115093, "422a907cf51d9bf11b50ac707c55237d5648bd46afdf29567b16aa9942436670"),
                         (167638, "87c4d03d70c2f152d1bb4509a351e8986e1ea5c17385cc2a985ba53b3475dc6a")],
              "maxl": [479, 285, 404],
              "chunk_lines": 64, "chunks": (
                  "9c05903a 254b4edd a5fe5b8e c2cf732a 83017151 7e1ab4f0 087f064f 04c5d755 648e7805 a629d664 b7ad1d93 f54bb92c "
                  "d413484a 761bb0a2 e149dd1b f2910377 2f88f4e7 3b207f9f e083f992 1264d852 8fa2e88c 944980b9 bfb2895c eb32ad04 "
                  "2b2592bf ecdbdbc3 8121989e e3e208a3 740f36b5 269427f3 d3caaa00 3ad6d3b7 e3d7cc10 81c8d192 533738de 66b1e1b0 "
                  "d85e172e d93179b1 0fcf6749 faea33de 5b775ca9 37076416 738422dd 3f501320 f69c5331 dc6a1254 05e6bdc5 9cef33d2 "
                  "ab340810 34753824 ").split()}
VOLATILE = (b"DATE ", b"STATS LOCAL")                             # lines a comparison with a recorded file leaves out


def golden(name):
    return os.path.join(ol.GOLDEN, name)


@functools.lru_cache(maxsize=None)
def score_system():
    return ba.ScoreSystem()


@functools.lru_cache(maxsize=None)
def queries(fixture):
    return tuple(bb.read_queries(golden(FIXTURES[fixture][0])))


def fresh_model(fixture, index, argv=()):
    """Record <index> of a fixture as an uncalibrated model with MAXL set, as bathbuild makes it."""
    name, _, seq = queries(fixture)[index]
    opts = bb.parse_options(list(argv) + ["out", "in"])[0]
    return bb.build_model(score_system(), name, seq, opts)


def recorded_lines(fixture):
    """Per model of a fixture's recorded file: its DATE and STATS lines, as text."""
    out = []
    for ln in open(golden(FIXTURES[fixture][1])).read().splitlines():
        if ln.startswith("DATE "):
            out.append([])
        if ln.startswith(("DATE ", "STATS LOCAL")) and out:
            out[-1].append(ln)
    return out


def recorded_stats(fixture):
    """Per model of a fixture's recorded file: the five STATS lines as text fields, {kind: (mu or tau, lambda)}."""
    return [{" ".join(t[2:-2]): (t[-2], t[-1]) for t in (ln.split() for ln in m if ln.startswith("STATS LOCAL"))} for m in recorded_lines(fixture)]


def with_recorded_lines(text, lines):
    """One model's text (bytes, calibrated so that its STATS block is there) with its DATE and STATS lines replaced by the recorded ones."""
    it = iter(lines)
    out = [next(it).encode() if ln.startswith(VOLATILE) else ln for ln in text.split(b"\n")]
    assert next(it, None) is None
    return b"\n".join(out)


def sha256(data):
    return hashlib.sha256(data).hexdigest()


def first_differing_chunk(text):
    """The 1-based line range of the first 64-line chunk of <text> whose digest is not the recorded three_seqs.bhmm's; None: all equal."""
    n = THREE_SEQS["chunk_lines"]
    lines = text.split(b"\n")[:-1]
    for c, want in enumerate(THREE_SEQS["chunks"]):
        if sha256(b"\n".join(lines[c * n:(c + 1) * n]))[:8] != want:
            return (c * n + 1, min((c + 1) * n, len(lines)))
    return None if len(lines) <= n * len(THREE_SEQS["chunks"]) else (n * len(THREE_SEQS["chunks"]) + 1, len(lines))


def stable_lines(text):
    """A model file's lines without DATE and STATS."""
    return [ln for ln in text.split(b"\n") if not ln.startswith(VOLATILE)]


class OracleModel:
    """What the oracle derives from a model in memory."""

    def __init__(self, hmm, L=100):
        L_ = ol.lib()
        self.keep = hmm
        self.hmm = C.cast(hmm._p, C.POINTER(ol.Hmm))
        self.M = hmm.M
        self.bg = ol.Bg()
        L_.bo_bg_create(C.byref(self.bg))
        self.gm = L_.bo_profile_config(self.hmm, C.byref(self.bg), L)
        self.om = L_.bo_oprofile_convert(self.gm)

    def __del__(self):
        L_ = ol.lib()
        L_.bo_oprofile_free(self.om)
        L_.bo_profile_free(self.gm)


def oracle_std_bits(model, kind, aa, L):
    """xv[i] = (score - null1) / ln 2 of the rows of <aa> [N, L] under one of the three standard scorers, as evalues.c:315-325,
    :384-394 and :554-560 have it: the overflow score for an MSV or Viterbi eslERANGE, an error for any other status."""
    L_ = ol.lib()
    om = model.om
    L_.bo_oprofile_reconfig_length(om, L)
    bg = ol.Bg()
    L_.bo_bg_create(C.byref(bg))
    L_.bo_bg_setlength(C.byref(bg), L)
    nullsc = np.float32(L_.bo_bg_nullone(C.byref(bg), L))
    o = om.contents
    maxsc = {"msv": np.float32((255 - o.base_b) / np.float32(o.scale_b)), "vit": np.float32((32767.0 - o.base_w) / float(o.scale_w))}
    f = C.c_float()
    xv = np.zeros(len(aa), np.float64)
    for i, row in enumerate(aa):
        d = ol.u8(ol.dsq_from(row))
        if kind == "msv":
            st = L_.bo_msvfilter(d, L, om, C.byref(f))
        elif kind == "vit":
            st = L_.bo_vitfilter(d, L, om, C.byref(f))
        else:
            st = L_.bo_forward_parser(d, L, om, None, C.byref(f))
        sc = np.float32(f.value)
        if st == ba.ERANGE and kind in maxsc:
            sc = maxsc[kind]
        else:
            assert st == 0, (kind, i, st)
        xv[i] = float(sc - nullsc) / LN2
    return xv


def oracle_calibrate(hmm, state, E=DEFAULT_E, ct=1):
    """p7_Calibrate of a model in memory on the CPU path: stores the eight parameters in the model and returns (the generator's
    state afterwards, the bit scores of the five fits)."""
    import calib_common as cc
    EmL, EmN, EvL, EvN, EfL, EfN, Eft = E
    model = OracleModel(hmm)
    lam = ba.hmm_lambda(hmm)
    xv = {}
    aa, state = ba.calib_sample_amino(state, EmL, EmN)
    xv["msv"] = oracle_std_bits(model, "msv", aa, EmL)
    aa, state = ba.calib_sample_amino(state, EvL, EvN)
    xv["vit"] = oracle_std_bits(model, "vit", aa, EvL)
    aa, state = ba.calib_sample_amino(state, EfL, EfN)
    xv["fwd"] = oracle_std_bits(model, "fwd", aa, EfL)
    ev = np.full(8, ba.FS_UNSET, np.float32)
    ev[[1, 3, 5]] = lam
    ev[0] = ba.gumbel_fit_complete_loc(xv["msv"], lam)
    ev[2] = ba.gumbel_fit_complete_loc(xv["vit"], lam)
    ev[4] = ba.calib_tau(xv["fwd"], lam, Eft)
    ba.hmm_set_evparam(hmm, ev)
    basic = np.zeros(64, np.uint8)
    assert ol.lib().bo_gencode_basic(ct, ol.u8(basic)) == 0
    for j, cl in ((6, 3), (7, 5)):
        dna, state = ba.calib_sample(state, EfL, EfN, ct)
        xv["fs%d" % cl] = cc.oracle_bits(model, basic, cl, dna, EfL)
        ev[j] = ba.calib_tau(xv["fs%d" % cl], lam, Eft)        # p7_Calibrate hands its double lambda on (evalues.c:142-143)
    ba.hmm_set_evparam(hmm, ev)
    return state, xv


@functools.lru_cache(maxsize=None)
def oracle_fixture(fixture, index, E=DEFAULT_E):
    """(calibrated model, bit scores of the five fits) of one record of a fixture, seeded with 42."""
    hmm = fresh_model(fixture, index)
    _, xv = oracle_calibrate(hmm, ba.rng_state(42), E)
    return hmm, xv


@functools.lru_cache(maxsize=None)
def oracle_calibrate_cached(seq, name="tiny"):
    """(calibrated model, bit scores) of a query given as text, MAXL at the default beta, seeded with 42, the default sizes."""
    hmm = ba.seq_model(score_system(), seq, name)
    ba.hmm_set_max_length(hmm, ba.hmm_max_length(hmm, 1e-7))
    _, xv = oracle_calibrate(hmm, ba.rng_state(42))
    return hmm, xv


class OracleCalibrator:
    """bathbuild's calibrator on the CPU path (bathbuild.run(..., calibrator=OracleCalibrator)): the tool's option and input rules
    are tested without a GPU.  Small sample sets by default keep a run at a second or two."""

    def __init__(self, opts, state):
        self.E = tuple(opts["--" + k] for k in ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN", "Eft"))
        self.ct = opts["--ct"]

    def calibrate(self, hmm, state):
        return oracle_calibrate(hmm, state, self.E, self.ct)[0]

    def close(self):
        pass
