"""What the CPU and the GPU tests of bath_amd.calibrate_fs_batch share: the batches they run (models, tables, L, N) and the
expected values of each from the CPU path of tests/calib_common.py -- the library's sampler and fit around the oracle's two
Forward recursions -- computed once per process and never changed.  A batch is a tuple of (M or "fixture index", seed) specs; the
synthetic models are written once into a directory of the process's own."""
import atexit
import functools
import shutil
import tempfile

import bath_amd as ba
import calib_common as cc
from bath_amd import synth
from test_tiling_coverage_cpu import fs_options, lengths_per_column

DIR = tempfile.mkdtemp(prefix="bath_calib_batch_")
atexit.register(shutil.rmtree, DIR, True)

SMALL_L, SMALL_N = 10, 9                # 30 nt windows; an odd N, no multiple of any windows-per-block choice
FULL_L, FULL_N = ba.CALIB_L, ba.CALIB_N
S0 = ba.rng_state(ba.CALIB_SEED)


def fixture(index):
    return ("fixture", index)


@functools.lru_cache(maxsize=None)
def model_file(spec):
    """(path, index in the file) of a spec: ("fixture", i) is model i of the 12-model HMMER3 file, (M, seed) a synthetic model."""
    if spec[0] == "fixture":
        return cc.HMM_IN, spec[1]
    M, seed = spec
    return synth.write_synthetic_bhmm("%s/s%d_%d.bhmm" % (DIR, M, seed), M, seed=seed), 0


def hmms(specs):
    return [ba.HMM(*model_file(s)) for s in specs]


def tiling_batches():
    """Per entry C of BATH_FS_COLUMNS: (C, specs, tables) -- the tiling's smallest and largest M in one batch, so two models share a
    launch; the first entry also holds M = 2 (its smallest is M = 1)."""
    out = []
    for c, lo, hi in lengths_per_column(fs_options()):
        ms = [lo, hi] + ([2] if lo == 1 else [])
        out.append((c, tuple((m, 100 + m) for m in ms), tuple((1, 4, 1)[:len(ms)])))
    return out


# alternating tilings, a repeated length with other parameters; and a batch of one
ORDER_SPECS = ((1, 11), (1280, 12), (64, 13), (65, 14), (129, 15), (65, 16))
ORDER_TABLES = (1, 4, 1, 1, 4, 4)
SINGLE_SPECS, SINGLE_TABLES = ((65, 14),), (4,)
# the full shape: ATE_N (M = 78), synthetic 129 and 459; the oracle's cost allows the first two on the CPU
FULL_SPECS = (fixture(0), (129, 5), (459, 7))
FULL_TABLES = (1, 4, 1)
FULL_ORACLE = 2


@functools.lru_cache(maxsize=None)
def oracle_batch(specs, tables, L, N, state=S0, limit=None):
    """[(tau3, tau5, state afterwards, xv3, xv5)] of the first <limit> models (None: all) on the CPU path, one generator carried."""
    out = []
    for spec, table in list(zip(specs, tables))[:limit]:
        path, index = model_file(spec)
        r = cc.oracle_model(path, index, table, state, L, N)
        state = r[2]
        out.append(r)
    return out


def sampler_state(tables, L, N, state=S0):
    """Where the generator stands after the samples of the models with <tables>: the library's sampler alone."""
    for t in tables:
        for _ in range(2):
            _, state = ba.calib_sample(state, L, N, t)
    return state
