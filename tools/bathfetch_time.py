#!/usr/bin/env python
"""Measures profiles/bathfetch_time.json on one GPU: what fetching a few models costs beside converting the whole file.

Workload: the 96-model HMMER3 file of tools/bathconvert_batch_time.py -- the 12-model fixture of tests/calib_common.py (the
reference's tutorial/tRNA-proteins.hmm) eight times -- with the copies' names and accessions made distinct (copy c > 0: NAME_c,
ACC_c).  No model of it has taus, so every fetched model is fitted and, without an index, the file's generator is walked.

Legs, every run in a fresh process, five counted after one uncounted, the legs alternating; seconds inside run() and process wall
time, medians with the raw values; for the fetches also the seconds run() spent in the host's generator walk and in the fits:
  convert16        bathconvert --batch 16 of the whole file: the only road to a fetched model before bathfetch (a lower bound of
                   it: the cut of the wanted models out of the output comes on top)
  scan3, scan24    bathfetch -f without an index: 3 keys (models 8 of copy 0, 9 of copy 4, 10 of copy 7: the walk covers 94 of the 96
                   models) and 24 keys (models 8, 9, 10 of every copy)
  index3, index24  the same key files with <file>.ssi present

Every step is a child process under a time limit of its own; the first that fails, is killed by a signal or runs into its limit ends
the script with its status, and nothing is started after it.
usage: tools/bathfetch_time.py [out.json]"""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHILD = ("import sys, time, io; from bath_amd import %s as b; s = {}; t = time.perf_counter(); "
         "rc = b.run(sys.argv[1:], stdout=io.StringIO()%s); "
         "print('INSIDE %%.6f WALK %%.6f FIT %%.6f FITTED %%d' %% (time.perf_counter() - t, s.get('walk_seconds', 0), s.get('fit_seconds', 0), s.get('fitted', -1))); sys.exit(rc)")
ROUNDS = 6                                                  # the first is not counted
SEL = (7, 8, 9)


def step(argv, limit):
    """One child process under its own time limit; a failure ends the script."""
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    w = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("step %s ended with status %d: nothing further is started" % (" ".join(argv[-4:]), p.returncode))
    return p.stdout, w


def main():
    out_json = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bathfetch_time.json")
    import calib_common as cc
    from bath_amd import bathconvert as bc
    one = bc.split_models(open(cc.HMM_IN, "rb").read().decode(bc.ENC))
    names = [bc.model_plan(m, None)["name"] for m in one]
    legs = ("convert16", "scan3", "scan24", "index3", "index24")
    rows = {m: [] for m in legs}
    with tempfile.TemporaryDirectory() as d:
        plain, indexed = os.path.join(d, "plain"), os.path.join(d, "indexed")
        os.mkdir(plain), os.mkdir(indexed)
        text = "".join(m if c == 0 else re.sub(r"^(NAME|ACC)(\s+)(\S+)", r"\1\2\3_%d" % c, m, flags=re.M) for c in range(8) for m in one)
        for sub in (plain, indexed):
            with open(os.path.join(sub, "x8.hmm"), "wb") as fh:
                fh.write(text.encode(bc.ENC))
        name = lambda c, i: names[i] if c == 0 else "%s_%d" % (names[i], c)
        keys = {"3": [name(0, 7), name(4, 8), name(7, 9)], "24": [name(c, i) for c in range(8) for i in SEL]}
        for n, ks in keys.items():
            with open(os.path.join(d, "keys%s.txt" % n), "w") as fh:
                fh.write("\n".join(ks) + "\n")
        step([sys.executable, "-m", "bath_amd.bathfetch", "--index", os.path.join(indexed, "x8.hmm")], 120)
        digest = {}
        for r in range(ROUNDS):
            for m in legs:
                out = os.path.join(d, "o%d%s.bhmm" % (r, m))
                if m == "convert16":
                    argv = [sys.executable, "-c", CHILD % ("bathconvert", ""), "--batch", "16", out, os.path.join(plain, "x8.hmm")]
                else:
                    sub, n = (plain, m[4:]) if m.startswith("scan") else (indexed, m[5:])
                    argv = [sys.executable, "-c", CHILD % ("bathfetch", ", stats=s"), "--batch", "16", "-f", "-o", out, os.path.join(sub, "x8.hmm"), os.path.join(d, "keys%s.txt" % n)]
                stdout, w = step(argv, 300)
                with open(out, "rb") as fh:
                    digest.setdefault(m, set()).add(fh.read())
                os.remove(out)
                t = stdout.split()
                if r:
                    rows[m].append({"inside_process_s": float(t[1]), "process_wall_s": w, "walk_s": float(t[3]), "fit_s": float(t[5]), "fitted": int(t[7])})
        if any(len(v) != 1 for v in digest.values()):
            raise SystemExit("a leg wrote different files in different runs")
        # a scan's models are the conversion's blocks without MAXL: the roads give the same models
        conv = bc.split_models(next(iter(digest["convert16"])).decode(bc.ENC))
        got = bc.split_models(next(iter(digest["scan24"])).decode(bc.ENC))
        want = ["".join(ln for ln in conv[12 * c + i].splitlines(keepends=True) if not ln.startswith("MAXL ")) for c in range(8) for i in SEL]
        if got != want:
            raise SystemExit("scan24's models are not the conversion's")
    med = lambda m, k: statistics.median(r[k] for r in rows[m])
    res = {"what": "bathfetch -f --batch 16 of 3 and of 24 keys from a 96-model HMMER3 file (tests/calib_common.HMM_IN eight times, names and accessions made "
                   "distinct; every model needs a fit), without an index (scan) and with one, beside bathconvert --batch 16 of the whole file, on one MI355X; "
                   "per leg 5 runs in fresh processes after one uncounted, the legs alternating; walk_s: the host's generator walk (calib_skip), fit_s: context, "
                   "model reads and calibrate_fs_batch_at",
           "legs": {m: {"runs": rows[m], **{k + "_median": med(m, k) for k in ("inside_process_s", "process_wall_s", "walk_s", "fit_s")},
                        "models_fitted": rows[m][0]["fitted"]} for m in legs},
           "scan24_equals_the_conversions_blocks_without_MAXL": True}
    for m in ("scan3", "scan24"):
        res["legs"][m]["walk_share_of_inside"] = res["legs"][m]["walk_s_median"] / res["legs"][m]["inside_process_s_median"]
    c = res["legs"]["convert16"]["inside_process_s_median"]
    res["inside_process_vs_convert16"] = {m: c / res["legs"][m]["inside_process_s_median"] for m in legs}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({m: {k: v for k, v in leg.items() if k != "runs"} for m, leg in res["legs"].items()}))


if __name__ == "__main__":
    main()
