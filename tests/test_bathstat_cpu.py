"""CPU tier of bath_amd.bathstat: the tutorial's rows (practice 4) for the recorded two-model file, the twelve-model file with its
accessions, a HMMER3 file, and the statistic itself against a restatement of modelstats.c:163-198 in numpy."""
import io
import os

import numpy as np
import pytest

import bath_amd as ba
import calib_common as cc
import oracle_lib as ol
from bath_amd import bathstat as bst
from bath_amd import synth

HEADER = ("#\n"
          "# idx    name                 accession        nseq eff_nseq   mlen codon_tbl re/pos\n"
          "# ------ -------------------- ------------ -------- -------- ------ --------- ------\n")


def stat(path):
    out = io.StringIO()
    assert bst.run([path], stdout=out) == 0
    return out.getvalue()


def test_the_tutorial_rows():
    """practice 4 prints these two rows for MET.bhmm with table 1; MET-ct4.bhmm is the same pair of models with table 4."""
    text = stat(os.path.join(ol.GOLDEN, "MET-ct4.bhmm"))
    assert text == bst.BANNER + HEADER + (
        "  1      metC                 -                  11     0.60    409         4   0.53\n"
        "  2      metG                 -                  24     0.62    458         4   0.53\n")
    assert text.startswith("# bathstat :: display summary statistics for a profile file\n# BATH 2.0 (May 2026); ")


def test_twelve_rows_with_accessions():
    rows = stat(cc.BHMM_OUT)[len(bst.BANNER + HEADER):].splitlines()
    assert len(rows) == 12 and [int(r.split()[0]) for r in rows] == list(range(1, 13))
    assert rows[0] == "  1      ATE_N                PF04376.8          30     1.11     78         1 %6.2f" % position_relent(ba.HMM(cc.BHMM_OUT, 0))
    assert rows[2].split() == ["3", "PTH2", "PF01981.11", "10", "0.74", "116", "1"] + rows[2].split()[-1:]
    assert [r.split()[2][:2] for r in rows] == ["PF"] * 12


def test_a_hmmer3_file_prints_the_table_the_reader_gives():
    rows = stat(cc.HMM_IN)[len(bst.BANNER + HEADER):].splitlines()
    brows = stat(cc.BHMM_OUT)[len(bst.BANNER + HEADER):].splitlines()
    assert len(rows) == 12
    for i, (r, b) in enumerate(zip(rows, brows)):
        t, tb = r.split(), b.split()
        assert t[:6] == tb[:6] and t[7] == tb[7] and int(t[6]) == ba.HMM(cc.HMM_IN, i).ct


def position_relent(hmm):
    """modelstats.c:163-198 and p7_hmm.c:1348-1356 in double precision."""
    M = hmm.M
    t = np.ctypeslib.as_array(hmm._p.contents.t, shape=((M + 1) * 7,)).reshape(M + 1, 7).astype(np.float64)     # MM MI MD IM II DM DD
    mat = synth.hmm_match_emissions(hmm).astype(np.float64)
    p1 = 350. / 351.
    mocc = np.zeros(M + 1)
    mocc[1] = t[0][1] + t[0][0]
    for k in range(2, M + 1):
        mocc[k] = mocc[k - 1] * (t[k - 1][0] + t[k - 1][1]) + (1. - mocc[k - 1]) * t[k - 1][5]
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(mat > 0, mat * np.log2(mat / synth.BG), 0.0).sum(axis=1)
    mre = (mocc[1:] * kl[1:]).sum() / mocc[1:].sum()
    tre = 0.
    for k in range(2, M + 1):
        mm, mi, im, dm = t[k - 1][0], t[k - 1][1], t[k - 1][3], t[k - 1][5]
        tre += (mocc[k - 1] * mm * np.log(mm / p1) + mocc[k - 1] * mi * (np.log(mm / p1) + np.log(im / p1)) + (1. - mocc[k - 1]) * dm * np.log(dm / p1)) / np.log(2.)
    return mre + tre / mocc[2:].sum()


@pytest.mark.parametrize("name,index", [("MET-ct4.bhmm", 0), ("MET-ct4.bhmm", 1), ("PTH2.bhmm", 0), ("Caudal_act.bhmm", 0)])
def test_the_statistic_against_a_double_precision_restatement(name, index):
    """The library keeps the reference's float steps (occupancy, the relative entropy of a node, the occupancy sums); in double the
    figure moves by float rounding of sums over M <= 458 nodes of terms below 5 bits: 1e-4 is a hundred times that."""
    hmm = ba.HMM(os.path.join(ol.GOLDEN, name), index)
    got = ba.hmm_position_relent(hmm)
    assert abs(got - position_relent(hmm)) < 1e-4, (got, position_relent(hmm))
    assert got != ba.hmm_relent(hmm)                                                   # not bathbuild's re/pos


def test_refusals(capsys, tmp_path):
    out = io.StringIO()
    assert bst.run([], stdout=out) == 1 and "Incorrect number of command line arguments." in out.getvalue()
    assert bst.run([str(tmp_path / "absent.bhmm")], stdout=io.StringIO()) == 1
    assert "absent.bhmm" in capsys.readouterr().err
    out = io.StringIO()
    assert bst.run(["-h"], stdout=out) == 0 and "Usage: bathstat [-options] <hmmfile>" in out.getvalue()
