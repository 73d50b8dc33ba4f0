"""Wall time of `bathsearch --gpus N` on one box: tRNA-proteins.bhmm (12 models) against a seeded synthetic genome, searched by the
CLI with no --gpus option, with --gpus 1 and with --gpus N whose ranks share device 0 over gloo (BATH_SEARCH_SHARE_DEVICE=1,
BATH_SEARCH_BACKEND=gloo).  The N-rank runs report every rank's phases (BATH_SEARCH_LAPS): launch and rendezvous (from the parent's
start to the process group), ingest, search (the rank's busy time on its items), merge and write, and the items it searched.

On a shared device the ranks take turns on one GPU, so this shows the fixed cost of N ranks and the cost of the merge, not a speed-up.

    python tools/bathsearch_multi_profile.py --mb 100 --gpus 2 --out profiles/bathsearch_multi_one_gpu.json
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DB = os.path.join(ROOT, "tests", "golden", "tRNA-proteins.bhmm")


def write_genome(path, n_nt, seed, records=10):
    import bath_amd as ba
    from bath_amd import synth
    hmms = [ba.HMM(DB, q) for q in range(ba.HMM.count(DB))]
    g, planted = synth.genome(n_nt, seed=seed, hmms=hmms, genes_per_model=max(4, n_nt // 400_000))
    syms = np.frombuffer(b"ACGT", dtype=np.uint8)[g]
    cut = np.linspace(0, n_nt, records + 1).astype(np.int64)
    with open(path, "wb") as fh:
        for r in range(records):
            s = syms[cut[r]:cut[r + 1]]
            fh.write(b">chr%d synthetic seed %d\n" % (r, seed))
            full = len(s) // 80 * 80
            fh.write(np.hstack([s[:full].reshape(-1, 80), np.full((full // 80, 1), ord("\n"), np.uint8)]).tobytes())
            if len(s) > full:
                fh.write(s[full:].tobytes() + b"\n")
    return len(planted)


def run(cwd, argv, env_extra, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "bath_amd.bathsearch"] + argv, cwd=cwd, env=env,
                       capture_output=True, text=True)
    dt = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("bathsearch %s: exit status %d" % (" ".join(argv), p.returncode))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=4300)
    ap.add_argument("--gpus", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="bathsearch_multi_")
    try:
        shutil.copy(DB, os.path.join(work, "db.bhmm"))
        t = time.perf_counter()
        n_planted = write_genome(os.path.join(work, "genome.fa"), int(args.mb * 1e6), args.seed)
        out = {"workload": "tRNA-proteins.bhmm (12 models) vs a %.0f Mb synthetic genome (10 records, %d planted genes), "
                           "bathsearch -o --tblout --cigar" % (args.mb, n_planted),
               "genome_write_s": time.perf_counter() - t, "runs": {}}
        base = ["-o", "out.txt", "--tblout", "hits.tbl", "--cigar", "db.bhmm", "genome.fa"]
        outputs = {}
        for name, extra, env in [("no_option", [], {}), ("gpus_1", ["--gpus", "1"], {}),
                                 ("gpus_%d_shared_device" % args.gpus, ["--gpus", str(args.gpus)],
                                  {"BATH_SEARCH_SHARE_DEVICE": "1", "BATH_SEARCH_BACKEND": "gloo", "BATH_SEARCH_LAPS": os.path.join(work, "laps")})]:
            for f in glob.glob(os.path.join(work, "laps*.json")):
                os.remove(f)
            wall = run(work, extra + base, env, args.timeout)
            rec = {"wall_s": wall}
            laps = sorted(glob.glob(os.path.join(work, "laps.rank*.json")))
            if laps:
                rec["ranks"] = [json.load(open(f)) for f in laps]
            out["runs"][name] = rec
            keep = lambda t: [ln for ln in t.split("\n") if not ln.startswith(("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:"))]
            outputs[name] = (keep(open(os.path.join(work, "out.txt")).read()), keep(open(os.path.join(work, "hits.tbl")).read()))
            out["runs"][name]["hits"] = sum(1 for ln in outputs[name][1] if ln and not ln.startswith("#"))
        first = outputs["no_option"]
        out["outputs_equal_to_no_option_run"] = {k: v == first for k, v in outputs.items()}
        out["note"] = ("ranks share ONE device: no speed-up can show. launch_s: the parent's start to the rank's process group "
                       "(interpreter, imports of torch and bath_amd, rendezvous); context_s: the rank's device context; ingest_s: the FASTA "
                       "file to the device; search_s: the rank's busy time on its items; merge_write_s: the exchange, the owners' finish "
                       "and rendering, rank 0's writes; rank_main_s: the rank's whole run after its imports")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
