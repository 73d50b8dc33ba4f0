"""orf_tile_kernel with a quarter wave per tile (16 lanes x 24 nt, 8 codons per stream and lane) against the oracle's
bo_translate_orfs, ORF by ORF, on the inputs of tests/translate_quarter_inputs.py: every window length around the lane and tile
seams, stops at each of the 24 in-lane positions of a tile's first, middle and last lane on either strand, two stops inside one
lane, min_orf_len on both sides of the kernel's first-stop shortcut, blocks that leave quarter waves idle, a degenerate
nucleotide among canonical tiles of one wave, other genetic codes.  tests/test_translate_quarter_cpu.py checks the inputs."""
import numpy as np
import pytest

import translate_quarter_inputs as tq

pytestmark = pytest.mark.gpu

CASES = tq.cases()


def compare(gpu_ctx, windows, ct, minlen):
    import bath_amd as ba
    dna = ba.SeqBlock(gpu_ctx, [np.asarray(w, np.uint8) for w in windows])
    got = ba.translate_orfs(gpu_ctx, dna, ct, minlen)
    want = tq.oracle_orfs(windows, ct, minlen)
    gk = [tuple(int(v) for v in g[:5]) for g in got]
    wk = [tuple(int(v) for v in o[:5]) for o in want]
    missing, extra = sorted(set(wk) - set(gk)), sorted(set(gk) - set(wk))
    assert not missing and not extra, ("missing", missing[:5], "extra", extra[:5], len(got), len(want))
    assert gk == wk, "same ORFs in another order, or repeated"
    for g, o in zip(got, want):
        assert np.array_equal(g[5], o[5]), (g[:5], g[5][:16], o[5][:16])
    return len(got)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_quarter_wave_tiles(gpu_ctx, case):
    name, windows, ct, minlen = CASES[case]
    n = compare(gpu_ctx, windows, ct, minlen)
    assert n > 0, name


@pytest.mark.parametrize("wave", ["1", "0"])
def test_both_stitch_kernels_on_every_case(wave):
    """The tile summaries feed orf_stitch_wave_kernel (BATH_HIP_STITCH_WAVE=1) and orf_stitch_kernel (=0); the switch is read once
    per process, so every case above runs again in a fresh child process under each."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BATH_HIP_STITCH_WAVE=wave)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_quarter_wave_tiles"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=os.path.dirname(here))
    assert p.returncode == 0 and "%d passed" % len(CASES) in p.stdout and "failed" not in p.stdout, p.stdout[-3000:]
