"""The CPU path of frameshift calibration that the bathconvert tests share: the library's sampler and Gumbel fit around the
ORACLE's two Forward recursions (bo_gforward_parser_fs3, bo_gforward_fs on the multihit length-L profile) and its null score.
One generator is carried through a file's models, the 3-codon fit before the 5-codon fit (bathconvert.c:128-161).  Results are
cached per (file, table, seed, L, N): computed once, shared by the CPU and the GPU tests, never changed."""
import atexit
import ctypes as C
import functools
import hashlib
import os
import re
import shutil
import tempfile

import numpy as np

import bath_amd as ba
import oracle_lib as ol

BHMM_OUT = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")
HMM_LINES = os.path.join(ol.GOLDEN, "tRNA-proteins.hmm.lines")
HMM_BYTES, HMM_SHA256 = 995188, "a91b9ca8a92c938281a4abe36112020efb74e4fa4db4dfaea01bac2d6e8e131c"


def hmmer3_input():
    """The reference's tutorial/tRNA-proteins.hmm (HMMER3/f, 12 models, 995 188 bytes), the recorded INPUT of the conversion whose
    recorded output is tests/golden/tRNA-proteins.bhmm.  The two differ in 13 lines per model and in nothing else, so the input is
    not committed a second time: it is put together from the output and the 4 lines per model that the conversion rewrote (the header
    line and the three STATS lines as the input spells them, tests/golden/tRNA-proteins.hmm.lines), MAXL and the four frameshift lines
    left out, and held to the original's size and SHA-256.  Returns the path of the file, made once per process."""
    theirs = iter(open(HMM_LINES).read().splitlines())
    out = []
    for ln in open(BHMM_OUT, "rb").read().decode("latin-1").splitlines(keepends=True):
        if ln.startswith("BATH3/f") or ln.startswith(("STATS LOCAL MSV", "STATS LOCAL VITERBI", "STATS LOCAL FORWARD")):
            out.append(next(theirs) + "\n")
        elif not ln.startswith(("MAXL ", "STATS LOCAL FS", "FRAMESHIFT PROB", "CODON TABLE")):
            out.append(ln)
    data = "".join(out).encode("latin-1")
    assert next(theirs, None) is None and len(data) == HMM_BYTES and hashlib.sha256(data).hexdigest() == HMM_SHA256
    d = tempfile.mkdtemp(prefix="bath_hmm_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "tRNA-proteins.hmm")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


HMM_IN = hmmer3_input()
LN2 = 0.69314718055994529


def recorded(path):
    """Per model of a BATH3/f file: (MAXL, FS3 tau, FS5 tau, codon table) as its text states them."""
    txt = open(path).read()
    return [(int(re.search(r"^MAXL\s+(\d+)", m, re.M).group(1)), float(re.search(r"^STATS LOCAL FS3 FORWARD\s+(\S+)", m, re.M).group(1)),
             float(re.search(r"^STATS LOCAL FS5 FORWARD\s+(\S+)", m, re.M).group(1)), int(re.search(r"^CODON TABLE\s+(\d+)", m, re.M).group(1)))
            for m in txt.split("\n//\n") if m.strip()]


def oracle_bits(model, basic, codon_lengths, dna, L):
    """xv[i] = (Forward score - null score) / ln 2 of the rows of <dna> [N, 3L], every float operation as evalues.c:645-649 has it."""
    L_ = ol.lib()
    gm = L_.bo_fs_profile_config(model.hmm, C.byref(model.bg), ol.u8(basic), codon_lengths, L)
    bg = ol.Bg()
    L_.bo_bg_create(C.byref(bg))
    L_.bo_bg_setlength(C.byref(bg), L)
    nullsc = np.float32(L_.bo_bg_fs_nullone(C.byref(bg), L))
    n = 3 * L
    gx = L_.bo_gmx_create(model.M, n + 1, n, 8 if codon_lengths == 5 else 3)
    f = C.c_float()
    xv = np.zeros(len(dna), np.float64)
    for i, w in enumerate(dna):
        d = ol.u8(ol.dsq_from(w))
        st = L_.bo_gforward_fs(d, n, gm, gx, 0, C.byref(f)) if codon_lengths == 5 else L_.bo_gforward_parser_fs3(d, n, gm, gx, C.byref(f))
        assert st == 0, st
        xv[i] = float(np.float32(f.value) - nullsc) / LN2
    L_.bo_gmx_free(gx)
    L_.bo_fs_profile_free(gm)
    return xv


def oracle_model(path, index, ncbi_table, state, L=ba.CALIB_L, N=ba.CALIB_N, tailp=ba.CALIB_TAILP):
    """One model's (tau3, tau5, state afterwards, xv3, xv5) on the CPU path."""
    model = ol.Model(path, index)
    basic = np.zeros(64, np.uint8)
    assert ol.lib().bo_gencode_basic(ncbi_table, ol.u8(basic)) == 0
    lam = float(ba.HMM(path, index).evparam[5])
    out = []
    for cl in (3, 5):
        dna, state = ba.calib_sample(state, L, N, ncbi_table)
        xv = oracle_bits(model, basic, cl, dna, L)
        out.append((ba.calib_tau(xv, lam, tailp), xv))
    return out[0][0], out[1][0], state, out[0][1], out[1][1]


@functools.lru_cache(maxsize=None)
def oracle_file(path, ncbi_table=None, seed=ba.CALIB_SEED, L=ba.CALIB_L, N=ba.CALIB_N):
    """Every model of a file, one generator carried through it: [(tau3, tau5, state afterwards, xv3, xv5)].  ncbi_table None: 1."""
    state = ba.rng_state(seed)
    out = []
    for i in range(ba.HMM.count(path)):
        r = oracle_model(path, i, 1 if ncbi_table is None else ncbi_table, state, L, N)
        state = r[2]
        out.append(r)
    return out
