#!/usr/bin/env python
"""Writes profiles/bathconvert_odds_vs_recorded.json on one GPU: the 24 frameshift taus of the reference's tutorial/tRNA-proteins.hmm
fitted in the reference's odds-ratio arithmetic (bath_amd.calibrate_fs(arith="odds"), seed 42 carried through the file) minus the
values recorded in tests/golden/tRNA-proteins.bhmm, beside the strict path's and the exact-log-sum CPU path's differences copied from
profiles/bathconvert_vs_recorded.json, and the sequences each fit redrew.  The condition tests/test_arith_cpu.py holds the file to:
every |diff| is smaller than that tau's |strict_diff|.  usage: tools/bathconvert_pin_odds.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import bath_amd as ba
    import calib_common as cc
    out_json = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bathconvert_odds_vs_recorded.json")
    strict = json.load(open(os.path.join(ROOT, "profiles", "bathconvert_vs_recorded.json")))
    rec = cc.recorded(cc.BHMM_OUT)
    ctx = ba.Context(0)
    state, models = ba.rng_state(ba.CALIB_SEED), []
    for i, (s, r) in enumerate(zip(strict["models"], rec)):
        hmm = ba.HMM(cc.HMM_IN, i)
        t3, t5, state, _, _, redrawn = ba.calibrate_fs(ctx, hmm, 1, state, want_xv=True, arith="odds")
        m = {"index": i, "name": hmm.name}
        for key, tau, want, nre in (("fs3", t3, r[1], redrawn[0]), ("fs5", t5, r[2], redrawn[1])):
            m[key] = {"recorded": want, "gpu_odds": tau, "diff": tau - want, "strict_diff": s[key]["diff"],
                      "exact_logsum_diff": s[key]["diff_exact_logsum"], "redrawn": nre}
        models.append(m)
    ctx.close()
    diffs = {k: [abs(m[k]["diff"]) for m in models] for k in ("fs3", "fs5")}
    res = {"what": "frameshift taus of tutorial/tRNA-proteins.hmm fitted on the GPU in odds-ratio arithmetic (calibrate_fs arith=odds: fs3_fwd_odds_kernel, "
                   "fs5_fwd_odds_kernel without its stores; seed 42 carried through the file) minus the values recorded in tests/golden/tRNA-proteins.bhmm; "
                   "strict_diff and exact_logsum_diff are profiles/bathconvert_vs_recorded.json's diff and diff_exact_logsum",
           "condition": "every |diff| < that tau's |strict_diff|",
           "L": ba.CALIB_L, "N": ba.CALIB_N, "tailp": ba.CALIB_TAILP,
           "max_abs_diff_fs3": max(diffs["fs3"]), "max_abs_diff_fs5": max(diffs["fs5"]),
           "min_factor_under_strict": min(abs(m[k]["strict_diff"]) / max(abs(m[k]["diff"]), 1e-300) for m in models for k in ("fs3", "fs5")),
           "condition_met": all(abs(m[k]["diff"]) < abs(m[k]["strict_diff"]) for m in models for k in ("fs3", "fs5")),
           "models": models}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "models"}))


if __name__ == "__main__":
    main()
