"""A/B of `bathsearch --fs --arith strict|odds3|odds` on one GPU: the CLI in fresh child processes, the three modes alternating
after a warm-up round, on two inputs:

  genome  tests/golden/tRNA-proteins.bhmm (12 models) against the synthetic genome of bench.py's configs[3] leg (c4_genome: seed
          4300, --mb million nucleotides, one record), as tools/bathsearch_workers_ab.py searches it;
  long    one synthetic model of --long-m nodes (synth.write_synthetic_bhmm, seed 1024) against a genome of --mb million
          nucleotides with frameshifted genes of it planted (synth.genome, seed 4400).

--parent TREE adds the same --fs searches (no --arith option) run from another checkout of the project whose library is built:
the parent commit's time from the same box, the same script and the same inputs, beside which the strict leg shows that nothing
else moved.  Every run is a child under its own `timeout`; the script stops at the first non-zero status.  Per run: the child's
wall time, and the seconds inside bathsearch.run.  Per mode: the hit rows, and how many differ from strict's.

    python tools/bathsearch_arith_ab.py --parent ../parent-checkout --out profiles/bathsearch_arith_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bathsearch_workers_ab import DB, search, text_of, write_genome   # noqa: E402


def write_long(d, M, n_nt):
    import bath_amd as ba
    from bath_amd import synth
    path = synth.write_synthetic_bhmm(os.path.join(d, "synth%d.bhmm" % M), M, seed=1024, name="synth%d" % M)
    g, planted = synth.genome(n_nt, seed=4400, hmms=[ba.HMM(path)], genes_per_model=max(4, n_nt // 400_000), frameshift=True)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[g]
    fa = os.path.join(d, "long_genome.fa")
    with open(fa, "wb") as fh:
        fh.write(b">long_genome synthetic seed 4400\n")
        full = len(s) // 80 * 80
        fh.write(np.hstack([s[:full].reshape(-1, 80), np.full((full // 80, 1), ord("\n"), np.uint8)]).tobytes())
        if len(s) > full:
            fh.write(s[full:].tobytes() + b"\n")
    return path, fa, len(planted)


def hit_rows(lines):
    return [ln for ln in lines if ln and not ln.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=12.5)
    ap.add_argument("--long-m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = [(m, ROOT, ["--arith", m]) for m in ("strict", "odds3", "odds")]
    if args.parent:
        configs.insert(0, ("parent", os.path.abspath(args.parent), []))
    result = {"rounds": args.rounds, "warmup": args.warmup, "inputs": {}}
    with tempfile.TemporaryDirectory() as d:
        genome = os.path.join(d, "c4_genome.fa")
        planted = write_genome(genome, int(args.mb * 1e6))
        long_hmm, long_fa, long_planted = write_long(d, args.long_m, int(args.mb * 1e6))
        inputs = [("genome", DB, genome, "tests/golden/tRNA-proteins.bhmm (12 models) against c4_genome, %.1f Mb, %d planted genes" % (args.mb, planted)),
                  ("long", long_hmm, long_fa, "synthetic model of %d nodes against a %.1f Mb genome, %d frameshifted genes planted" % (args.long_m, args.mb, long_planted))]
        for key, db, target, what in inputs:
            runs = {name: [] for name, _, _ in configs}
            tables = {}
            for rnd in range(args.warmup + args.rounds):
                for name, tree, extra in configs:                       # the configurations alternate within a round
                    wall, inside = search(tree, d, extra + ["--fs", "--cigar", "-o", "out.txt", "--tblout", "hits.tbl", db, target], args.timeout)
                    got = hit_rows(text_of(os.path.join(d, "hits.tbl")))
                    if name in tables and tables[name] != got:
                        raise SystemExit("%s on %s: the table differs between two runs" % (name, key))
                    tables[name] = got
                    if rnd >= args.warmup:
                        runs[name].append((wall, inside))
            if "parent" in tables and tables["parent"] != tables["strict"]:
                raise SystemExit("--arith strict on %s: the table differs from the parent's" % key)
            rows = {}
            for name, r in runs.items():
                rows[name] = {"wall_s_median": statistics.median(w for w, _ in r), "wall_s_min": min(w for w, _ in r), "wall_s_max": max(w for w, _ in r),
                              "run_s_median": statistics.median(x for _, x in r), "run_s_min": min(x for _, x in r), "run_s_max": max(x for _, x in r),
                              "hit_rows": len(tables[name]), "hit_rows_not_in_strict": len(set(tables[name]) - set(tables["strict"]))}
                print("%-7s %-7s wall %.3f s (%.3f..%.3f)  inside run() %.3f s (%.3f..%.3f)  %d hit rows, %d not in strict's" % (
                    key, name, rows[name]["wall_s_median"], rows[name]["wall_s_min"], rows[name]["wall_s_max"],
                    rows[name]["run_s_median"], rows[name]["run_s_min"], rows[name]["run_s_max"], rows[name]["hit_rows"], rows[name]["hit_rows_not_in_strict"]), flush=True)
            result["inputs"][key] = {"what": what, "configurations": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
