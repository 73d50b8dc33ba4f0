"""The reference's two recorded bathfetch / bathconvert outputs that the bathfetch tests compare with, put together from
tests/golden/tRNA-proteins.bhmm and held to the originals' size and SHA-256, as tests/calib_common.py does for the HMMER3 input.
Neither is committed a second time: checked against the reference's tutorial directory, each differs from the recorded conversion
in nothing but the lines named here.

tutorial/tRNA-synthetases.bhmm (`bathfetch -f -o tRNA-synthetases.bhmm tRNA-proteins.hmm tRNA-synthetases-key.txt`, 293 927 bytes):
models 8, 9 and 10 of tRNA-proteins.bhmm without their MAXL lines (the HMMER3 input has none and bathfetch computes none).
tutorial/tRNA-proteins-ct11.bhmm (`bathconvert --ct 11`, 996 687 bytes): tRNA-proteins.bhmm with CODON TABLE 11 in its 12 models
(tables 1 and 11 translate alike, so the sampled codons and the taus are the same)."""
import functools
import hashlib
import os

import oracle_lib as ol
from bath_amd import bathconvert as bc

BHMM = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")
SEL = (7, 8, 9)                                   # the models tests/golden/tRNA-synthetases-key.txt names, by position in the file
FETCH = {"bytes": 293927, "sha256": "658c4386b9ff128f8dfbf700899cec582b0b55cc06507b6d20b2a42d64d71883"}
CT11 = {"bytes": 996687, "sha256": "05064668d23e4c49c98c51e1842c66e461d72bd93279f745f0c0b2d111ee8704"}


def _held(text, want, what):
    data = text.encode(bc.ENC)
    assert len(data) == want["bytes"] and hashlib.sha256(data).hexdigest() == want["sha256"], what
    return text


@functools.lru_cache(maxsize=None)
def _conversion():
    with open(BHMM, "rb") as fh:
        return bc.split_models(fh.read().decode(bc.ENC))


@functools.lru_cache(maxsize=None)
def recorded_fetch():
    """The models of tutorial/tRNA-synthetases.bhmm, as texts."""
    models = ["".join(ln for ln in _conversion()[i].splitlines(keepends=True) if not ln.startswith("MAXL ")) for i in SEL]
    _held("".join(models), FETCH, "tRNA-synthetases.bhmm")
    return models


@functools.lru_cache(maxsize=None)
def recorded_ct11():
    """The models of tutorial/tRNA-proteins-ct11.bhmm, as texts."""
    models = [m.replace("\nCODON TABLE  1\n", "\nCODON TABLE  11\n") for m in _conversion()]
    _held("".join(models), CT11, "tRNA-proteins-ct11.bhmm")
    return models
