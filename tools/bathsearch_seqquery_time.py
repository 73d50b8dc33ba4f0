#!/usr/bin/env python
"""Measures profiles/bathsearch_seqquery_time.json on one GPU: what bathsearch --qformat fasta costs against building first.

Workload: a 96-record query file, the three records of tests/golden/three_seqs.fa (429, 245 and 358 residues) 32 times under
distinct names, against the synthetic genome of tools/bathsearch_workers_ab.py (bench.py's c4_genome, seed 4300, --mb million
nucleotides, one record).

1. Four legs, every run in a fresh process, five counted after one uncounted, the legs alternating; process wall time and the
   seconds inside run(), medians with the raw values:
     a_plain  bathbuild --batch 16, then bathsearch of the written file: the two processes' times summed (what the parent commit can do)
     a_fs     the same with bathsearch --fs
     b_plain  bathsearch --qformat fasta (the models calibrated without the frameshift taus, in a temporary file)
     b_fs     bathsearch --qformat fasta --fs --hmmout
   The main outputs of a_plain and b_plain, and of a_fs and b_fs, must be equal from the first Query: on.
2. In one process: the 96 models calibrated with and without the frameshift fits, model by model (calibrate) and in batches of 16
   (calibrate_batch), five counted after one uncounted, alternating: device ms per model from the library's kernel timers, and host
   ms per model.

Every step is a child process under a time limit of its own; the first that fails, is killed by a signal or runs into its limit ends
the script with its status, and nothing is started after it.
usage: tools/bathsearch_seqquery_time.py [--mb X] [out.json]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILD = ("import sys, time; from bath_amd import bathbuild as b; t = time.perf_counter(); rc = b.run(sys.argv[1:], stdout=open(sys.argv[-2] + '.txt', 'w')); "
         "print('INSIDE %.6f' % (time.perf_counter() - t)); sys.exit(rc)")
SEARCH = ("import sys, time; from bath_amd import bathsearch as b; t = time.perf_counter(); rc = b.run(sys.argv[1:]); "
          "print('INSIDE %.6f' % (time.perf_counter() - t)); sys.exit(rc)")
COPIES = 32
ROUNDS = 6                                                  # the first is not counted
BATCH = 16
IGNORED = ("# CPU time:", "# Mc/sec:")


def step(code, argv, limit, cwd):
    """One child process under its own time limit: (seconds inside run(), wall seconds); a failure ends the script."""
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", code] + argv, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True)
    w = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("step %s ended with status %d: nothing further is started" % (" ".join(argv[-4:]), p.returncode))
    return float(p.stdout.split("INSIDE")[1]), w


def records():
    from bath_amd import bathbuild as bb
    three = bb.read_queries(os.path.join(ROOT, "tests", "golden", "three_seqs.fa"))
    return [("%s_%02d" % (name, c), desc, seq) for c in range(COPIES) for name, desc, seq in three]


def from_query(path):
    text = open(path).read()
    return [ln for ln in text[text.index("Query:"):].split("\n") if not ln.startswith(IGNORED)]


def inprocess():
    """Step 2: prints one JSON line."""
    import bath_amd as ba
    from bath_amd import bathbuild as bb
    opts = bb.parse_options(["out", "in"])[0]
    score = ba.ScoreSystem()
    recs = records()
    E = {k: opts["--" + k] for k in ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN")}
    ctx = ba.Context(0)
    s0 = ba.rng_state(42)
    sets = ba.CalibSamples(ctx, s0, **E)
    legs = [(b, fs) for b in (1, BATCH) for fs in (True, False)]
    rows = {leg: [] for leg in legs}
    for r in range(ROUNDS):
        for b, fs in legs:
            hmms = [bb.build_model(score, name, seq, opts) for name, _, seq in recs]
            dev = host = 0.0
            for i0 in range(0, len(hmms), b):
                part = hmms[i0:i0 + b]
                t = time.perf_counter()
                if b == 1:
                    ba.calibrate(ctx, part[0], 1, s0, sets, Eft=opts["--Eft"], fs=fs, **E)
                else:
                    ba.calibrate_batch(ctx, part, 1, s0, sets, Eft=opts["--Eft"], fs=fs, **E)
                host += time.perf_counter() - t
                dev += sum(v[0] for v in ba.kernel_times(ctx).values())
            if r:
                rows[(b, fs)].append({"device_ms_per_model": dev / len(hmms), "host_ms_per_model": host * 1e3 / len(hmms)})
    sets.close()
    ctx.close()
    med = lambda leg, k: statistics.median(x[k] for x in rows[leg])
    print("RESULT " + json.dumps({"models": len(recs), "legs": {
        "%s_%s" % ("serial" if b == 1 else "batch%d" % b, "with_fs_fits" if fs else "standard_only"):
            {"runs": rows[(b, fs)], "device_ms_per_model_median": med((b, fs), "device_ms_per_model"), "host_ms_per_model_median": med((b, fs), "host_ms_per_model")}
        for b, fs in legs}}))


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--inprocess"]:
        return inprocess()
    mb = 12.5
    if argv[:1] == ["--mb"]:
        mb, argv = float(argv[1]), argv[2:]
    out_json = argv[0] if argv else os.path.join(ROOT, "profiles", "bathsearch_seqquery_time.json")
    from tools.bathsearch_workers_ab import write_genome
    legs = ("a_plain", "a_fs", "b_plain", "b_fs")
    inside, wall = {m: [] for m in legs}, {m: [] for m in legs}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "q.fa"), "w") as fh:
            for name, desc, seq in records():
                fh.write(">%s %s\n%s\n" % (name, desc, seq))
        planted = write_genome(os.path.join(d, "genome.fa"), int(mb * 1e6))
        for r in range(ROUNDS):
            for m in legs:
                fs = ["--fs"] if m.endswith("_fs") else []
                if m.startswith("a_"):
                    i0, w0 = step(BUILD, ["--batch", str(BATCH), "built.bhmm", "q.fa"], 300, d)
                    i1, w1 = step(SEARCH, fs + ["-o", m + ".out", "built.bhmm", "genome.fa"], 600, d)
                    i, w = i0 + i1, w0 + w1
                    os.remove(os.path.join(d, "built.bhmm"))
                else:
                    i, w = step(SEARCH, ["--qformat", "fasta"] + (fs + ["--hmmout", "kept.bhmm"] if fs else []) + ["-o", m + ".out", "q.fa", "genome.fa"], 600, d)
                sys.stderr.write("round %d %s: %.2f s wall, %.2f s inside run()\n" % (r, m, w, i))
                sys.stderr.flush()
                if r:
                    wall[m].append(w)
                    inside[m].append(i)
            for kind in ("plain", "fs"):
                if from_query(os.path.join(d, "a_%s.out" % kind)) != from_query(os.path.join(d, "b_%s.out" % kind)):
                    raise SystemExit("round %d: the main outputs of a_%s and b_%s differ" % (r, kind, kind))
    stdout = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--inprocess"], cwd=ROOT,
                            env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    if stdout.returncode != 0:
        sys.stderr.write(stdout.stderr[-3000:])
        raise SystemExit("the in-process step ended with status %d" % stdout.returncode)
    res = {"what": "bathsearch with a 96-record protein query file (tests/golden/three_seqs.fa, 3 records, 32 times) against c4_genome (%.1f Mb, %d planted "
                   "genes) on one MI355X; per leg 5 runs in fresh processes after one uncounted, the legs alternating.  a_*: bathbuild --batch 16 then "
                   "bathsearch, two processes, times summed; b_*: bathsearch --qformat fasta, one process (b_fs with --hmmout)" % (mb, planted),
           "legs": {m: {"inside_run_s": inside[m], "process_wall_s": wall[m], "inside_run_s_median": statistics.median(inside[m]),
                        "inside_run_s_range": [min(inside[m]), max(inside[m])], "process_wall_s_median": statistics.median(wall[m]),
                        "process_wall_s_range": [min(wall[m]), max(wall[m])]} for m in legs},
           "outputs_equal_from_the_first_query_on": True,
           "calibration_one_process_96_models": json.loads(stdout.stdout.split("RESULT ")[1])}
    res["b_over_a_process_wall"] = {k: res["legs"]["b_" + k]["process_wall_s_median"] / res["legs"]["a_" + k]["process_wall_s_median"] for k in ("plain", "fs")}
    res["b_over_a_inside_run"] = {k: res["legs"]["b_" + k]["inside_run_s_median"] / res["legs"]["a_" + k]["inside_run_s_median"] for k in ("plain", "fs")}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "calibration_one_process_96_models"}))
    print(json.dumps({k: {x: y for x, y in v.items() if x != "runs"} for k, v in res["calibration_one_process_96_models"]["legs"].items()}))


if __name__ == "__main__":
    main()
