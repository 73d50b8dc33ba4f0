"""CPU tier of bath_amd.ssi: the writer reproduces the recorded index of the reference's tutorial byte for byte, the reader finds
every name and accession at the offset where the model stands in the file, and a truncated or foreign file is refused by name."""
import os

import pytest

import oracle_lib as ol
from bath_amd import bathconvert as bc
from bath_amd import bathfetch as bf
from bath_amd import ssi

BHMM = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")
SSI = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm.ssi")


def models_and_offsets():
    models = bc.split_models(open(BHMM, "rb").read().decode(bc.ENC))
    offs, at = [], 0
    for m in models:
        offs.append(at)
        at += len(m.encode(bc.ENC))
    return models, offs


def test_the_recorded_index_is_what_the_layout_predicts():
    """12 names and 12 accessions: header 78, one file record 19 + 16, 12 x (15 + 2 + 8 + 8 + 8), 12 x (11 + 15) = 917 bytes."""
    data = open(SSI, "rb").read()
    assert len(data) == 78 + 35 + 12 * 41 + 12 * 26 == 917
    ix = ssi.Index(SSI)
    assert (ix.nprimary, ix.nsecondary, ix.flen, ix.plen, ix.slen, ix.files) == (12, 12, 19, 15, 11, ["tRNA-proteins.bhmm"])
    keys = ix.primary_keys()
    assert keys == sorted(keys, key=lambda k: k.encode()) and keys[0] == "ATE_N" and keys[-1] == "tRNA-synt_2d"    # strcmp order


def test_writer_reproduces_the_recorded_index():
    models, offs = models_and_offsets()
    names = [bc.model_plan(m, None)["name"] for m in models]
    accs = [bf.model_acc(m) for m in models]
    assert len(names) == 12 and all(accs)
    data = ssi.build("tRNA-proteins.bhmm", zip(names, offs), zip(accs, names))
    assert data == open(SSI, "rb").read()
    with pytest.raises(ValueError, match="more than once"):
        ssi.build("x", [("a", 0), ("a", 5)])


def test_reader_finds_every_name_and_accession():
    models, offs = models_and_offsets()
    ix = ssi.Index(SSI)
    data = open(BHMM, "rb").read()
    for m, off in zip(models, offs):
        name, acc = bc.model_plan(m, None)["name"], bf.model_acc(m)
        assert ix.find(name) == ("tRNA-proteins.bhmm", off) and ix.find(acc) == ("tRNA-proteins.bhmm", off), name
        assert data[off:off + 8] == b"BATH3/f\n"                                       # the model's format line
    for absent in ("", "A", "ATE", "ATE_NN", "PF01981", "zzz", "tRNA-synt_2e"):
        assert ix.find(absent) is None, absent


@pytest.mark.parametrize("keep", [0, 10, 53, 77, 100, 400, 604, 916])
def test_reader_refuses_a_truncated_copy(tmp_path, keep):
    p = tmp_path / "cut.ssi"
    p.write_bytes(open(SSI, "rb").read()[:keep])
    with pytest.raises(ssi.SSIFormatError, match="cut.ssi"):
        ssi.Index(str(p))


def test_reader_refuses_a_foreign_file(tmp_path):
    p = tmp_path / "model.ssi"
    p.write_bytes(open(BHMM, "rb").read()[:4096])
    with pytest.raises(ssi.SSIFormatError, match="model.ssi"):
        ssi.Index(str(p))

