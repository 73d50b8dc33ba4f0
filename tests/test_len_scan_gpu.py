"""The Viterbi stage's counting sort of a work list by target length (len_hist_kernel, len_scan_kernel, len_scatter_kernel;
bath_viterbi.hip) through bath_selftest_len_sort: the list longest first and the count of targets longer than T, against numpy.
len_scan_kernel scans the 2048 length bins with 256 threads of 8 bins each; the length sets put targets on both sides of every
seam between two threads' bins (and so between two waves'), into the last bin, which also takes every longer target, and
nowhere at all."""
import numpy as np
import pytest

import bath_amd as ba

pytestmark = pytest.mark.gpu

BINS = 2048


def _i32(a):
    return a.ctypes.data_as(ba._i32p)


def seams():
    """Lengths 8k - 1 and 8k for every k, in unequal numbers, shuffled."""
    rng = np.random.default_rng(3)
    k = np.arange(1, BINS // 8)
    lens = np.concatenate([np.repeat(8 * k - 1, 1 + k % 3), np.repeat(8 * k, 1 + k % 2)])
    return rng.permutation(lens)


SETS = {
    "all_equal": np.full(1000, 57),
    "one_target": np.array([300]),
    "seams": seams(),
    "last_bin": np.array([2046, 2047, 2047, 2048, 5000, 2046, 100000, 1, 0]),
    "empty": np.zeros(0, dtype=np.int64),
}
THRESHOLDS = (0, 6, 7, 8, 56, 57, 128, 1023, 1024, 2045, 2046, 2047, 4000)


@pytest.mark.parametrize("name", list(SETS))
def test_length_sort_against_numpy(gpu_ctx, name):
    lens = np.ascontiguousarray(SETS[name], dtype=np.int32)
    n = len(lens)
    bins = np.minimum(lens, BINS - 1)
    for T in THRESHOLDS:
        out = np.full(max(n, 1), -1, dtype=np.int32)
        longer = np.full(1, -1, dtype=np.int32)
        st = ba.lib().bath_selftest_len_sort(gpu_ctx._h, n, _i32(lens), T, _i32(out), _i32(longer))
        assert st == 0, ba.lib().bath_hip_last_error(gpu_ctx._h).decode()
        out = out[:n]
        assert np.array_equal(np.sort(out), np.arange(n)), (name, T)                  # a permutation of the list: no hole, no duplicate
        assert (np.diff(bins[out]) <= 0).all(), (name, T)                              # longest first; targets of one bin in any order
        # the targets ahead of bin min(T + 1, 2047)'s end: those longer than T, while T + 1 is a bin of its own
        assert int(longer[0]) == int((bins >= min(T + 1, BINS - 1)).sum()), (name, T)
