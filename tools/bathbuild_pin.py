"""Pins bathbuild's calibration against the reference's recorded runs: profiles/bathbuild_vs_recorded.json.

    python tools/bathbuild_pin.py            the CPU path (library sampler and fits around the oracle's MSV filter, Viterbi filter and
                                             Forward parser, tests/bathbuild_common.py) against the STATS lines of the four recorded
                                             single-sequence models (tests/golden/AMP_N.bhmm, three_seqs.bhmm.lines)
    python tools/bathbuild_pin.py --gpu      the same, and bath_hip_calibrate on one GPU against that CPU path: kept under "gpu"

A run without --gpu keeps the "gpu" section the file already has.  The tests read the bounds from the file and hold the stored
figures against what they compute."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np

import bath_amd as ba
import bathbuild_common as bc
from compact_json import dump

OUT = os.path.join(ROOT, "profiles", "bathbuild_vs_recorded.json")
KINDS = (("msv", "MSV", 0), ("vit", "VITERBI", 2), ("fwd", "FORWARD", 4), ("fs3", "FS3 FORWARD", 6), ("fs5", "FS5 FORWARD", 7))
MODELS = (("AMP_N", 0), ("three_seqs", 0), ("three_seqs", 1), ("three_seqs", 2))
GPU_CASES = (("AMP_N", 0, bc.DEFAULT_E), ("three_seqs", 1, bc.DEFAULT_E), ("three_seqs", 0, bc.DEFAULT_E), ("AMP_N", 0, bc.ODD_E))
MARGIN = 4.0


def cpu_section():
    models = []
    for fx, i in MODELS:
        hmm, _ = bc.oracle_fixture(fx, i)
        rec = bc.recorded_stats(fx)[i]
        m = {"fixture": fx, "record": i, "name": hmm.name, "M": hmm.M, "lambda": {"recorded": rec["MSV"][1], "cpu_path": "%8.5f" % hmm.evparam[1]}}
        for key, tag, j in KINDS:
            v = float(hmm.evparam[j])
            m[key] = {"recorded": rec[tag][0], "cpu_path": v, "printed": ("%8.4f" % v).strip(), "diff": v - float(rec[tag][0])}
        models.append(m)
    digits = all(m[k]["printed"] == m[k]["recorded"] for m in models for k in ("msv", "vit"))
    fwd = max(abs(m["fwd"]["diff"]) for m in models)
    return {"models": models, "mus_equal_the_recorded_digits": digits, "lambda_equals_the_recorded_digits": all(m["lambda"]["cpu_path"].strip() == m["lambda"]["recorded"] for m in models),
            "fwd_tau_max_abs_dev": fwd, "fwd_tau_bound": MARGIN * fwd, "margin": MARGIN,
            "fs_tau_max_abs_dev": max(abs(m[k]["diff"]) for m in models for k in ("fs3", "fs5"))}


def gpu_section():
    ctx = ba.Context(0)
    cases = []
    for fx, i, E in GPU_CASES:
        want, wxv = bc.oracle_fixture(fx, i, E)
        hmm = bc.fresh_model(fx, i)
        kw = dict(zip(("EmL", "EmN", "EvL", "EvN", "EfL", "EfN", "Eft"), E))
        _, xv = ba.calibrate(ctx, hmm, 1, ba.rng_state(42), None, want_xv=True, **kw)
        c = {"fixture": fx, "record": i, "E": list(E), "M": hmm.M}
        for key, _, j in KINDS:
            c[key] = {"gpu": float(hmm.evparam[j]), "cpu_path": float(want.evparam[j]), "abs_dev": abs(float(hmm.evparam[j]) - float(want.evparam[j])),
                      "xv_bit_identical": bool(np.array_equal(xv[key].view(np.uint64), wxv[key].view(np.uint64))),
                      "xv_max_abs_dev_bits": float(np.abs(xv[key] - wxv[key]).max())}
        cases.append(c)
    ctx.close()
    worst = max(c["fwd"]["abs_dev"] for c in cases)
    return {"cases": cases, "fwd_tau_max_abs_dev": worst, "fwd_tau_bound": MARGIN * worst, "margin": MARGIN,
            "fwd_tau_floor": "one float32 unit in the last place of the tau"}



def main(argv):
    old = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc = {"what": "calibration of the four recorded single-sequence models (seed 42 per model, the reference's defaults): the CPU path "
                   "(library sampler and fits, oracle MSV / Viterbi filters and Forward parser, oracle frameshift Forward with table log-sums) "
                   "minus the STATS values recorded in tests/golden/AMP_N.bhmm and three_seqs.bhmm.lines; under gpu, bath_hip_calibrate minus that CPU path"}
    doc.update(cpu_section())
    out = OUT
    if "--gpu" in argv:
        doc["gpu"] = gpu_section()
        if "--out" in argv:
            out = argv[argv.index("--out") + 1]
    elif "gpu" in old:
        doc["gpu"] = old["gpu"]
    with open(out, "w") as fh:
        fh.write(dump(doc))
    print(json.dumps({k: v for k, v in doc.items() if k not in ("models", "what")}, indent=1)[:4000])


if __name__ == "__main__":
    main(sys.argv[1:])
