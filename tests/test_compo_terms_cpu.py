"""The local-composition filter's term table, terms[x][s] = bg_f[x] * expf((base_b - s) / scale_b) for a residue x and a byte
score s (p7_pli_ComputeLocalCompo; compo_term in bath_pipeline.hip).  A profile builds it once, with the kernel that every
pipeline call used to launch.  bath_selftest_compo_terms evaluates the host build of the same function, held here against the
formula in numpy float32 -- with the model's constants (base_b = 190, scale_b = 3 / ln 2: arguments from -15 to +44) and with
constants that drive expf to both ends of the float range, where the table must underflow to zero and overflow to infinity as
the formula does.

Tolerance: the division and the product are single IEEE operations, equal in both; the two expf (the C library's and numpy's) are
each within 1 ulp of the true value, so their rounded results differ by at most 2 ulp, and the product with bg_f (one more
rounding of either) by at most 3."""
import numpy as np

import bath_amd as ba

# p7_bg.c's amino acid background, the table's bg_f (bath_amd.synth carries the same twenty floats)
from bath_amd.synth import BG


def numpy_terms(base_b, scale_b):
    s = np.arange(256, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        lo = (np.float32(base_b) - s) / np.float32(scale_b)
        return (BG.astype(np.float32)[:, None] * np.exp(lo, dtype=np.float32)[None, :]).astype(np.float32)


def ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)       # non-negative floats: ordered as their bits
    return np.abs(ia - ib)


def library_terms(base_b, scale_b):
    out = np.full((20, 256), np.nan, dtype=np.float32)
    assert ba.lib().bath_selftest_compo_terms(base_b, np.float32(scale_b), ba._f32(out)) == 0
    return out


def check(base_b, scale_b):
    got, want = library_terms(base_b, scale_b), numpy_terms(base_b, scale_b)
    assert not np.isnan(got).any() and (got >= 0).all()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert ulp_distance(got[fin], want[fin]).max() <= 3
    return got


def test_term_table_of_a_profile():
    got = check(190, np.float32(3.0 / np.log(2.0)))
    assert np.isfinite(got).all() and (got > 0).all()
    assert (np.diff(got, axis=1) < 0).all()                 # a higher byte score is a lower odds ratio


def test_term_table_at_the_ends_of_expf():
    lo = check(0, np.float32(0.5))                          # arguments 0 .. -510: subnormal results, then zero
    assert lo[:, 255].max() == 0.0 and (lo[:, 0] > 0).all()
    assert ((lo > 0) & (lo < np.finfo(np.float32).tiny)).any()
    hi = check(255, np.float32(0.5))                        # arguments +510 .. 0: infinity, then the largest finite values
    assert np.isinf(hi[:, 0]).all() and np.isfinite(hi[:, 255]).all()
    assert (hi[np.isfinite(hi)] > 1e37).any()


def test_rejects_a_scale_of_zero():
    out = np.zeros((20, 256), dtype=np.float32)
    assert ba.lib().bath_selftest_compo_terms(190, np.float32(0.0), ba._f32(out)) != 0
