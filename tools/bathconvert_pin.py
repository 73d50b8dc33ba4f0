#!/usr/bin/env python
"""Measures profiles/bathconvert_vs_recorded.json: the 24 frameshift taus of the reference's tutorial/tRNA-proteins.hmm (tests/calib_common.py puts it together) on the CPU path of
tests/calib_common.py (the library's sampler and Gumbel fit around the oracle's Forward recursions) against the values recorded in
tests/golden/tRNA-proteins.bhmm, the same path with the oracle's exact log-sums in place of the table, and each tau's spread over 50
reseeded runs.  No GPU.  usage: tools/bathconvert_pin.py [processes]"""
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEEDS = list(range(1, 51))


def taus(arg):
    seed, exact = arg
    import calib_common as cc
    import oracle_lib as ol
    ol.lib().bo_flogsum_set_exact(1 if exact else 0)
    r = cc.oracle_file(cc.HMM_IN, None, seed)
    return [(a[0], a[1]) for a in r]


def main():
    import numpy as np
    import bath_amd as ba
    import calib_common as cc
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    with mp.Pool(nproc) as pool:
        runs = pool.map(taus, [(42, False), (42, True)] + [(s, False) for s in SEEDS], chunksize=1)
    table, exact, reseeded = runs[0], runs[1], np.array(runs[2:])          # [50][12][2]
    rec = cc.recorded(cc.BHMM_OUT)
    models = []
    for i, r in enumerate(rec):
        m = {"index": i, "name": ba.HMM(cc.HMM_IN, i).name}
        for j, key in enumerate(("fs3", "fs5")):
            m[key] = {"recorded": r[1 + j], "cpu_path": table[i][j], "diff": table[i][j] - r[1 + j],
                      "cpu_path_exact_logsum": exact[i][j], "diff_exact_logsum": exact[i][j] - r[1 + j],
                      "reseeded_mean": float(reseeded[:, i, j].mean()), "reseeded_sd": float(reseeded[:, i, j].std(ddof=1))}
        models.append(m)
    out = {"what": "frameshift taus of tutorial/tRNA-proteins.hmm: CPU path (library sampler and fit, oracle Forward with table log-sums, seed 42 carried "
                   "through the file) minus the values recorded in tests/golden/tRNA-proteins.bhmm; the same with exact log-sums; sd over reseeded runs",
           "bound_outcome_A": 1.5e-4, "reseeded_seeds": SEEDS, "L": ba.CALIB_L, "N": ba.CALIB_N, "tailp": ba.CALIB_TAILP,
           "max_abs_diff": max(abs(m[k]["diff"]) for m in models for k in ("fs3", "fs5")),
           "max_abs_diff_exact_logsum": max(abs(m[k]["diff_exact_logsum"]) for m in models for k in ("fs3", "fs5")),
           "models": models}
    with open(os.path.join(ROOT, "profiles", "bathconvert_vs_recorded.json"), "w") as fh:
        models = out.pop("models")                            # one line per model
        head = json.dumps(out, indent=1)[:-2]
        fh.write(head + ',\n "models": [\n  ' + ",\n  ".join(json.dumps(m) for m in models) + "\n ]\n}\n")
        out["models"] = models
    print(json.dumps({k: out[k] for k in ("max_abs_diff", "max_abs_diff_exact_logsum")}))


if __name__ == "__main__":
    main()
