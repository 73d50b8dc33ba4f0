"""A/B of `bathsearch --workers N` on one GPU: the CLI in fresh child processes with --workers 1 and --workers 2 / 3 / 4 / 6,
alternating after a warm-up round, on two inputs:

  genome  tests/golden/tRNA-proteins.bhmm (12 models) against the synthetic genome of bench.py's configs[3] leg (c4_genome: seed
          4300, --mb million nucleotides, one record);
  small   the same model file against tests/golden/target-MET.fa (36 kb): launch latency and the fixed costs dominate.

--parent TREE adds the same searches (no --workers option) run from another checkout of the project whose library is built -- the
parent commit's serial time from the same box, the same script and the same inputs.  Every run is a child under its own `timeout`;
the script stops at the first non-zero status.  Per run: the child's wall time, and the seconds inside bathsearch.run (contexts,
ingest, search, rendering; without the interpreter's start and the imports).  The outputs of every configuration are compared with
the --workers 1 output (timing and trailer lines apart).

    python tools/bathsearch_workers_ab.py --parent ../parent-checkout --out profiles/bathsearch_workers_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DB = os.path.join(ROOT, "tests", "golden", "tRNA-proteins.bhmm")
SMALL = os.path.join(ROOT, "tests", "golden", "target-MET.fa")
IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")
CHILD = ("import sys, time; from bath_amd import bathsearch as b; t = time.perf_counter(); st = b.run(sys.argv[1:]); "
         "sys.stderr.write('RUN_S %.6f\\n' % (time.perf_counter() - t)); sys.exit(st)")


def write_genome(path, n_nt):
    """bench.py's c4_genome as a one-record FASTA file of 80-column lines."""
    import bath_amd as ba
    from bath_amd import synth
    hmms = [ba.HMM(DB, q) for q in range(ba.HMM.count(DB))]
    g, planted = synth.genome(n_nt, seed=4300, hmms=hmms, genes_per_model=max(4, n_nt // 400_000))
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[g]
    full = len(s) // 80 * 80
    with open(path, "wb") as fh:
        fh.write(b">c4_genome synthetic seed 4300\n")
        fh.write(np.hstack([s[:full].reshape(-1, 80), np.full((full // 80, 1), ord("\n"), np.uint8)]).tobytes())
        if len(s) > full:
            fh.write(s[full:].tobytes() + b"\n")
    return len(planted)


def search(tree, cwd, argv, timeout):
    """(wall seconds, seconds inside run) of one search run from the checkout <tree>."""
    env = dict(os.environ, PYTHONPATH=tree)
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-c", CHILD] + argv, cwd=cwd, env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("bathsearch %s (from %s): exit status %d" % (" ".join(argv), tree, p.returncode))
    inside = [float(ln.split()[1]) for ln in p.stderr.splitlines() if ln.startswith("RUN_S ")]
    return wall, inside[-1]


def text_of(path):
    with open(path) as fh:
        return [ln for ln in fh.read().split("\n") if not ln.startswith(IGNORED)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=12.5)
    ap.add_argument("--workers", default="2,3,4,6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = [("workers-1", ROOT, ["--workers", "1"])] + [("workers-%d" % int(n), ROOT, ["--workers", str(int(n))]) for n in args.workers.split(",") if n.strip()]
    if args.parent:
        configs.insert(0, ("parent", os.path.abspath(args.parent), []))
    result = {"rounds": args.rounds, "warmup": args.warmup, "model_file": "tests/golden/tRNA-proteins.bhmm", "inputs": {}}
    with tempfile.TemporaryDirectory() as d:
        genome = os.path.join(d, "c4_genome.fa")
        planted = write_genome(genome, int(args.mb * 1e6))
        inputs = [("genome", genome, "c4_genome, %.1f Mb, %d planted genes" % (args.mb, planted)), ("small", SMALL, "tests/golden/target-MET.fa")]
        for key, target, what in inputs:
            runs = {name: [] for name, _, _ in configs}
            want = None
            for rnd in range(args.warmup + args.rounds):
                for name, tree, extra in configs:                       # the configurations alternate within a round
                    out = os.path.join(d, "%s-%s.out" % (key, name))
                    tbl = os.path.join(d, "%s-%s.tbl" % (key, name))
                    wall, inside = search(tree, d, extra + ["-o", "out.txt", "--tblout", "hits.tbl", DB, target], args.timeout)
                    os.replace(os.path.join(d, "out.txt"), out)
                    os.replace(os.path.join(d, "hits.tbl"), tbl)
                    if rnd >= args.warmup:
                        runs[name].append((wall, inside))
                    if name == "workers-1" and want is None:
                        want = (text_of(out), text_of(tbl))
                    elif want is not None and (text_of(out), text_of(tbl)) != want:
                        raise SystemExit("%s on %s: output differs from --workers 1" % (name, key))
            rows = {}
            for name, r in runs.items():
                rows[name] = {"wall_s_median": statistics.median(w for w, _ in r), "wall_s_min": min(w for w, _ in r), "wall_s_max": max(w for w, _ in r),
                              "run_s_median": statistics.median(x for _, x in r), "run_s_min": min(x for _, x in r), "run_s_max": max(x for _, x in r)}
                print("%-7s %-10s wall %.3f s (%.3f..%.3f)  inside run() %.3f s (%.3f..%.3f)" % (
                    key, name, rows[name]["wall_s_median"], rows[name]["wall_s_min"], rows[name]["wall_s_max"],
                    rows[name]["run_s_median"], rows[name]["run_s_min"], rows[name]["run_s_max"]), flush=True)
            result["inputs"][key] = {"target": what, "hit_rows": sum(1 for ln in want[1] if ln and not ln.startswith("#")), "configurations": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
