"""A/B of the 3-codon parsers' modes on the --fs pass: strict (the default, log-space, bit-identical to the generic reference)
against odds ratios (Context.set_fs_odds, what the reference's bathsearch --fs runs).

Runs run_frameshift_domains alternately in the two modes on
  * bench.py's --fs block: synth.dna_windows(1_000_000, 1000, seed=4242, hmm=Caudal_act, frameshift=True), and
  * bench.py's configs[4] leg: the synthetic 1024-node model against a 125 Mb synthetic genome (--c5-mb; 0 skips it),
<passes> timed passes per mode after a warm-up of each, and prints per pass the wall time (host clock around a call that ends
in a device synchronize), the per-kernel device times of kernel_times(), the domain count, and the domains that differ between
the two modes.  --only odds|strict runs one mode (for a profiler run of its own).

--fs5: three modes instead of two -- strict; "odds" (the 3-codon parsers in odds ratios); "odds5" (Context.set_fs_odds and
Context.set_fs5_odds: the 5-codon envelope Forward / Backward and the regions' Forward in odds ratios too) -- and the domains of
each odds mode against strict's.  --only odds5 runs that mode alone."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bath_amd as ba                     # noqa: E402
from bath_amd import dist as bdist, synth  # noqa: E402


def records(dm):
    return sorted((int(r["window"]), int(r["strand"]), int(r["ienv"]), int(r["jenv"]), int(r["iali"]), int(r["jali"]), int(r["ihmm"]), int(r["jhmm"]),
                   round(float(r["bitscore"]), 2)) for r in dm)


def leg(name, ctx, hmm, block, passes, only, fs5=False):
    om = ba.OProfile(ctx, ba.Profile(hmm))
    om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
    om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
    pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
    modes = [only] if only else (["strict", "odds", "odds5"] if fs5 else ["strict", "odds"])
    last = {}

    def one(mode):
        ctx.set_fs_odds(mode in ("odds", "odds5"))
        ctx.set_fs5_odds(mode == "odds5")
        ctx.synchronize()
        t0 = time.perf_counter()
        stats, fw, dm, nskip = pipe.run_frameshift_domains(om3, om5, block, arrays=True)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kt = {k: round(v[0], 3) for k, v in sorted(pipe.kernel_times().items(), key=lambda kv: -kv[1][0])}
        last[mode] = records(dm)
        return ms, kt, len(dm)

    for mode in modes:
        one(mode)                                    # warm-up: code objects, tables, lanes
    out = {m: [] for m in modes}
    for p in range(passes):
        for mode in modes:
            ms, kt, nd = one(mode)
            out[mode].append(ms)
            print(json.dumps({"leg": name, "mode": mode, "pass": p, "pass_ms": round(ms, 2), "domains": nd, "kernel_ms": kt}))
            sys.stdout.flush()
    ctx.set_fs_odds(False)
    ctx.set_fs5_odds(False)
    summary = {"leg": name, "pass_ms_median": {m: round(float(np.median(v)), 2) for m, v in out.items()},
               "pass_ms_range": {m: [round(min(v), 2), round(max(v), 2)] for m, v in out.items()}}
    if len(modes) == 2:
        a, b = set(last["strict"]), set(last["odds"])
        summary["domains"] = {"strict": len(last["strict"]), "odds": len(last["odds"]), "only_strict": sorted(a - b), "only_odds": sorted(b - a)}
    elif len(modes) == 3:
        a = set(last["strict"])
        summary["domains"] = {m: len(last[m]) for m in modes}
        for m in ("odds", "odds5"):
            b = set(last[m])
            summary["domains"]["differ_" + m] = {"only_strict": len(a - b), "only_" + m: len(b - a)}
        summary["domains"]["only_odds5_vs_odds"] = sorted(set(last["odds5"]) - set(last["odds"]))[:40]
    print(json.dumps(summary))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fs-windows", type=int, default=1_000_000)
    ap.add_argument("--c5-mb", type=float, default=125.0)
    ap.add_argument("--only", choices=["strict", "odds", "odds5"], default=None)
    ap.add_argument("--fs5", action="store_true", help="three modes: strict, 3-codon odds, 3- and 5-codon odds")
    args = ap.parse_args()
    ctx = ba.Context(0)
    hmm = ba.HMM(os.path.join(ROOT, "tests", "golden", "Caudal_act.bhmm"))
    flat, offsets, _ = synth.dna_windows(args.fs_windows, 1000, seed=4242, hmm=hmm, frameshift=True)
    leg("fs_block", ctx, hmm, ba.SeqBlock(ctx, flat, offsets), args.passes, args.only, args.fs5)
    del flat, offsets
    if args.c5_mb > 0:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "synth1024.bhmm")
            synth.write_synthetic_bhmm(path, 1024, seed=1024, name="synth1024")          # bench.py's configs[4] model
            h5 = ba.HMM(path)
            n_nt = int(args.c5_mb * 1e6)
            g, _ = synth.genome(n_nt, seed=4400, hmms=[h5], genes_per_model=max(8, n_nt // 400_000), frameshift=True)
            wins = bdist.split_targets([len(g)], h5.max_length)
            block = ba.SeqBlock(ctx, [g[s:s + n] for _, s, n, _ in wins])
            block.set_context([c for _, _, _, c in wins])
            leg("c5_%gmb" % args.c5_mb, ctx, h5, block, args.passes, args.only, args.fs5)
    ctx.close()


if __name__ == "__main__":
    main()
