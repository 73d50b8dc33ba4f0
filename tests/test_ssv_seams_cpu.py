"""CPU tier: the inputs of test_ssv_shapes_gpu meet their seam condition, judged by the oracle and a plain numpy Kadane alone.

The GPU tests assert the condition for every model before they compare anything; here it is held for one model of each lane count
and for the models at the ends of the range, together with the restatement it rests on."""
import numpy as np
import pytest

import test_ssv_shapes_gpu as t


def test_diagonal_max_is_kadane_along_the_diagonals():
    S = np.zeros((5, 20))
    S[1:, 0] = [2.0, -1.0, 3.0, 1.5]                   # residue 0 over nodes 1..4; every other residue scores 0
    S[1:, 1] = -5.0
    x = [0, 0, 0, 0]
    assert t.diagonal_max(S, x) == 2.0 - 1.0 + 3.0 + 1.5
    assert t.diagonal_max(S, x, cut=2) == 3.0 + 1.5    # no step from node 2 to node 3
    assert t.diagonal_max(S, x, cut=3) == 2.0 - 1.0 + 3.0
    assert t.diagonal_max(S, x, cut=1) == 3.0 + 1.5
    assert t.diagonal_max(S, [0, 1, 0, 0]) == 3.0 + 1.5
    assert t.diagonal_max(S, [1, 1]) == 0.0            # the begin score
    assert t.diagonal_max(np.array([[0.0] * 20, [2.5] * 20]), [3], cut=0) == 0.0 and t.seam_cut(1, 1) == 0
    assert t.seam_cut(100, 1) == 1 and t.seam_cut(100, 52) == 52 and t.seam_cut(100, 100) == 99


@pytest.mark.parametrize("M", [1, 57, 152, 153, 417, 1024, 2560], ids=lambda M: "%d-False" % M)     # the ids these cases have always had
def test_seam_condition_holds_from_the_oracle_alone(M):
    I = t.inputs(M)
    counts = t.seam_condition(I)                         # asserts at least 2 targets per seam
    assert sorted(counts) == [s for s, _ in I.seams] == [s for s, _ in t.ssv_seams(M, *t.ssv_shape(M))]
    assert len(I.seqs) % 64 != 0 and {len(s) for s in I.seqs} >= set(range(1, 10)) | {n + d for n in range(4, 41, 4) for d in (-1, 0, 1)}
    assert (I.ssv[1] != 0).sum() > 0 or M < 16           # statuses that are not OK are there too
    print("M=%d (NR=%d, G=%d): targets per seam that meet the condition: %s" % (M, I.NR, I.G, counts))
