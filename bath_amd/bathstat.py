"""bathstat: one line of summary statistics per model of a HMMER3/f or BATH3/f model file.  Host code, no GPU.

    python -m bath_amd.bathstat [-h] <hmmfile>

What bathstat.c prints (:74-130): the banner, a header and per model its index, name, accession ("-" without one), NSEQ, EFFN, length,
codon table and p7_MeanPositionRelativeEntropy (bath_amd.hmm_position_relent: match emissions weighted by match occupancy plus the
cost of the transitions into each node -- not the unweighted match relative entropy bathbuild and bathconvert print as re/pos).  The
codon table is what the library's reader gives the model: a HMMER3 model states none.
"""
import os
import sys
import tempfile

import bath_amd as ba
from bath_amd.bathconvert import ENC, UsageError, check_format, split_models
from bath_amd.bathfetch import model_acc

BANNER = ("# bathstat :: display summary statistics for a profile file\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
USAGE = "Usage: bathstat [-options] <hmmfile>\n"
HEAD = "# %-6s %-20s %-12s %8s %8s %6s %9s %6s\n"
ROW = "  %-6d %-20s %-12s %8d %8.2f %6d %9d %6.2f\n"


def header_fields(model):
    """NAME, NSEQ and EFFN of a model's text as the reference's model record holds them (-1, -1.0 where the text has none).  Not
    bathconvert.model_plan: an uncalibrated model has statistics too."""
    f = {"name": "", "nseq": -1, "eff_nseq": -1.0}
    for ln in model.splitlines():
        t = ln.split(None, 1)
        if ln.startswith("HMM "):
            break
        if len(t) == 2 and t[0] == "NAME":
            f["name"] = t[1].strip()
        elif len(t) == 2 and t[0] == "NSEQ":
            f["nseq"] = int(t[1])
        elif len(t) == 2 and t[0] == "EFFN":
            f["eff_nseq"] = float(t[1])
    return f


def run(argv, stdout=None):
    stdout = stdout or sys.stdout
    opts = [a for a in argv if a.startswith("-") and len(a) > 1]
    args = [a for a in argv if a not in opts]
    if "-h" in opts:
        stdout.write(BANNER + USAGE + "\nOptions:\n  -h : show brief help on version and usage\n")
        return 0
    if opts or len(args) != 1:
        stdout.write(("Failed to parse command line: unknown option %s\n" % opts[0] if opts else "Incorrect number of command line arguments.\n") + USAGE +
                     "\nTo see more help on available options, do bathstat -h\n\n")
        return 1
    path = args[0]
    stdout.write(BANNER)
    scratch = tempfile.TemporaryDirectory()
    try:
        if not os.path.isfile(path):
            raise UsageError("File existence/permissions problem in trying to open HMM file %s." % path)
        with open(path, "rb") as fh:
            data = fh.read()
        check_format(data, path)
        models = split_models(data.decode(ENC))
        stdout.write("#\n" + HEAD % ("idx", "name", "accession", "nseq", "eff_nseq", "mlen", "codon_tbl", "re/pos") +
                     HEAD % ("------", "--------------------", "------------", "--------", "--------", "------", "---------", "------"))
        one = os.path.join(scratch.name, "model.hmm")
        for i, m in enumerate(models):
            p = header_fields(m)
            with open(one, "wb") as fh:                              # the library reads model <index> of a file from the file's start:
                fh.write(m.encode(ENC))                              # one model at a time keeps a Pfam-sized file linear
            try:
                hmm = ba.HMM(one, 0)
            except ba.BathError:
                raise UsageError("bad file format in HMM file %s (model %d, %s)" % (path, i + 1, p["name"]))
            stdout.write(ROW % (i + 1, p["name"], model_acc(m) or "-", p["nseq"], p["eff_nseq"], hmm.M, hmm.ct, ba.hmm_position_relent(hmm)))
    except (UsageError, OSError) as e:
        sys.stderr.write("\nError: %s\n" % e)
        return 1
    finally:
        scratch.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
