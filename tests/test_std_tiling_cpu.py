"""CPU tier: the inputs of tests/test_std_tiling_gpu.py do what they are there for, checked with the oracle alone (the GPU tests
assert the same on the same cached results), and the oracle's matrices hook is the pass the domain stage's oracle makes."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import test_std_tiling_gpu as t


@pytest.mark.parametrize("M", t.STD_M)
def test_tiling_envelopes_exercise_the_kernels(tmp_path, M):
    """(a) nine envelopes on the edges of the 64-row chunks; at least seven give a domain; from 64 nodes on the traces hold M, D, I."""
    model = ol.Model(t.synthetic(tmp_path, M), 0)
    envs = t.tiling_envelopes(model, M)
    assert [len(s) for s in envs[:7]] == t.ENV_LENGTHS and len(envs) == 9 and len(envs[8]) == 100
    assert len(envs[7]) == (M + 20 if M < 385 else min(M + 20, 400))
    t.assert_tiling_inputs(M, t.oracle_envelopes(("tiling", M), model, envs))


@pytest.mark.parametrize("M", sorted(t.HOLE_MODELS))
def test_hole_models_load_and_delete_at_the_holes(tmp_path, M):
    """(b) the rewritten file has the zero transitions where they were asked for and nowhere else inside the model, and the oracle's
    traces run a delete state into a hole."""
    d_nodes, i_nodes = t.HOLE_MODELS[M]
    plain = ol.Model(t.synthetic(tmp_path, M), 0)
    model = ol.Model(t.synthetic(tmp_path, M, t.HOLE_MODELS[M]), 0)
    tr = lambda m: np.ctypeslib.as_array(m.hmm.contents.t, shape=((M + 1) * 7,)).reshape(M + 1, 7)      # MM MI MD IM II DM DD
    a, b = tr(plain), tr(model)
    for k in range(1, M):
        if k in d_nodes:
            assert b[k][2] == 0.0 and b[k][6] == 0.0 and b[k][5] == 1.0
        if k in i_nodes:
            assert b[k][1] == 0.0 and b[k][4] == 0.0 and b[k][3] == 1.0
        if k not in d_nodes and k not in i_nodes:
            assert np.array_equal(a[k], b[k]) and (a[k] > 0).all()
        assert abs(b[k][:3].sum() - 1.0) < 1e-4
    # in the optimized profile the fill kernels read: a zero DD or MD inside the model exactly at the holes
    tf = np.ctypeslib.as_array(model.om.contents.tf, shape=((M + 1) * 8,)).reshape(M + 1, 8)            # MM IM DM BM MD DD MI II
    assert sorted(k for k in range(1, M) if tf[k][5] == 0.0) == sorted(k for k in d_nodes if k < M)
    envs = t.hole_envelopes(model, M, d_nodes)
    t.assert_hole_inputs(M, t.oracle_envelopes(("holes", M), model, envs))


def test_hole_nodes_sit_on_the_lane_and_wave_boundaries():
    """Where the holes of (b) fall in the kernels' node layout: lane l of the one-wave kernel owns nodes l C + 1 .. l C + C, wave w of the
    block kernel nodes 64 w C + 1 .. 64 (w + 1) C."""
    import test_tiling_coverage_cpu as cov
    for M, (d_nodes, _) in t.HOLE_MODELS.items():
        c = cov.columns(M, t.STD_FILL_COLUMNS)
        assert any(k % c == 0 for k in d_nodes) and any(k % c == 1 for k in d_nodes) and (c < 3 or any(k % c not in (0, 1) for k in d_nodes))
    assert cov.columns(70, t.STD_FILL_COLUMNS) == 2 and cov.columns(200, t.STD_FILL_COLUMNS) == 4 and cov.columns(520, t.STD_FILL_COLUMNS) == 12
    c4 = lambda M: next(c for c in t.STD_FILL_MW_COLUMNS if (M + 255) // 256 <= c)
    assert c4(200) == 1 and c4(520) == 4
    assert {128, 129} <= set(t.HOLE_MODELS[200][0])          # <1>: wave 1 ends at node 128
    assert {256, 257} <= set(t.HOLE_MODELS[520][0])          # <4>: wave 0 ends at node 256


def test_matrices_hook_is_the_domain_stage_oracle(tmp_path):
    """bo_std_envelope_matrices against rescore_envelope through bo_std_envelope_trace (same oasc, asserted in oracle_envelope) and
    against its own definition: posteriors from the Forward and Backward matrices it hands out, in float64."""
    M = 65
    model = ol.Model(t.synthetic(tmp_path, M), 0)
    for s in t.tiling_envelopes(model, M)[2:8]:
        o = t.oracle_envelope(model, s)
        assert o["ok"] and abs(o["sc"][0] - o["sc"][1]) <= 1e-3 * max(1.0, abs(o["sc"][0]))
        L = len(s)
        fx, bx = o["fx"].astype(np.float64), o["bx"].astype(np.float64)
        sp = 1.0 / bx[0][1]
        for i in range(1, L + 1):
            want = o["fwd"][i].astype(np.float64) * o["bck"][i].astype(np.float64) * sp * fx[i][5]
            want[:, 1] = 0.0
            assert np.allclose(o["pp"][i][1:], want[1:], rtol=1e-5, atol=1e-9)
            sp *= fx[i][5] / bx[i][5]
        # every residue is emitted by a match, an insert or N / J / C: the posteriors of a row add up to 1
        rows = o["pp"][1:, 1:, :].sum(axis=(1, 2)) + o["ppx"][1:, 1] + o["ppx"][1:, 2] + o["ppx"][1:, 4]
        assert np.allclose(rows, 1.0, atol=2e-3)
        assert np.isneginf(o["oa"][0]).all() and o["sc"][2] == o["ox"][L][4]


@pytest.mark.parametrize("M", sorted(t.PIPELINE_M))
def test_pipeline_windows_give_hits(tmp_path, M):
    model = ol.Model(t.synthetic(tmp_path, M), 0)
    wins = t.pipeline_windows(model, M)
    assert len(wins) == 12
    _, odm, per_d, _ = model.run_pipeline_hits(wins)
    assert len(odm) >= 3


@pytest.mark.parametrize("residues", t.REGION_RESIDUES)
def test_region_windows_are_one_long_orf_with_a_domain(residues):
    """(d) the window's first frame has no stop, so its ORF has <residues> residues: 16 (L + 1) bytes of LDS on either side of 64 KiB
    and of 128 KiB; the oracle finds a domain in it."""
    model = ol.Model(ol.GOLDEN + "/" + t.REGION_MODEL, 0)
    w = t.region_window(model, residues)
    assert len(w) == 3 * residues
    codons = w.reshape(-1, 3)
    assert all(model.basic[int(c[0]) * 16 + int(c[1]) * 4 + int(c[2])] < 20 for c in codons)
    lds = 16 * (residues + 1)
    assert {1000: lds <= 65536, 4200: 65536 < lds <= 131072, 8300: lds > 131072}[residues]
    pli, odm, per_d, _ = model.run_pipeline_hits([w])
    assert len(odm) >= 1
