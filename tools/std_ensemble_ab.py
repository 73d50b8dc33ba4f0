#!/usr/bin/env python3
"""A/B of the standard branch's ensemble modes: serial host ensemble (mode 0) against the device ensemble (mode 2).

Two inputs.  "plain": a search without --fs (Pipeline.run_hits) over a block dense in multi-copy genes -- --genes windows whose ORF
holds two or three copies of a domain sampled from tests/golden/PTH2.bhmm, among three random windows each -- so that a pass resolves a
few hundred regions by clustering (the count is printed).  "fs": bench.py's --fs block through Pipeline.run_frameshift_domains with
BOTH switches (set_fs_ensemble, set_std_ensemble) serial or device.  Passes of the two modes alternate after a warm-up, at
BATH_HIP_HOST_THREADS = 2 and 16; per combination the wall time per pass (median and range), std_ensemble_kernel's device time from
kernel_times() (which covers the context the standard branch of an --fs pass runs on), the regions it walked and the fallback
counters.  On a build without set_std_ensemble (the parent of the commit that added it) only mode 0 runs: that is the yardstick.
bench.py is imported for its inputs only and is not changed.

    python tools/std_ensemble_ab.py [--genes N] [--passes K] [--fs-windows N | --no-fs]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def multi_copy_block(ba, synth, hmm, genes, seed=7):
    rng = np.random.default_rng(seed)
    mat = synth.hmm_match_emissions(hmm)
    basic = ba.gencode_basic(hmm.ct)
    rnd_aa = lambda n: rng.integers(0, 20, size=n, dtype=np.uint8)
    rnd_nt = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    wins = []
    for g in range(genes):
        copies = 2 + (g % 4 == 0)
        aa = np.concatenate([rnd_aa(6)] + [np.concatenate([synth.sample_domain(rng, mat), rnd_aa(int(rng.integers(8, 25)))]) for _ in range(copies)])
        wins.append(np.concatenate([rnd_nt(60), synth.reverse_translate(rng, aa, basic), rnd_nt(60)]))
        wins += [rnd_nt(900) for _ in range(3)]
    return wins


def ab(ctx, run, set_mode, modes, passes, label):
    for threads in (2, 16):
        os.environ["BATH_HIP_HOST_THREADS"] = str(threads)
        t = {m: [] for m in modes}
        kms, info = [], {}
        for mode in modes:                                        # warm-up: buffers, side contexts
            set_mode(mode)
            run()
        c0 = ctx.std_ensemble_counters() if hasattr(ctx, "std_ensemble_counters") else None
        for _ in range(passes):
            for mode in modes:
                set_mode(mode)
                ctx.synchronize()
                t0 = time.perf_counter()
                ndm, nclust, ktimes = run()
                t[mode].append((time.perf_counter() - t0) * 1e3)
                info[mode] = (ndm, nclust)
                if mode == 2:
                    kms.append(ktimes.get("std_ensemble_kernel", (0.0,))[0])
        c1 = ctx.std_ensemble_counters() if c0 is not None else None
        for mode in modes:
            extra = ""
            if mode == 2:
                extra = "  std_ensemble_kernel %.3f ms  regions walked per pass %.0f  fallbacks: serial %d twin %d" % (
                    statistics.median(kms), (c1["kernel_regions"] - c0["kernel_regions"]) / passes, c1["serial_fallbacks"] - c0["serial_fallbacks"],
                    c1["twin_fallbacks"] - c0["twin_fallbacks"])
            print("%-6s threads %2d  mode %d  pass %8.2f ms (min %8.2f max %8.2f, %d passes)  domains %d  clustered regions %d%s" % (
                label, threads, mode, statistics.median(t[mode]), min(t[mode]), max(t[mode]), passes, info[mode][0], info[mode][1], extra), flush=True)
    os.environ.pop("BATH_HIP_HOST_THREADS", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=400)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fs-windows", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--no-fs", action="store_true")
    ap.add_argument("--no-plain", action="store_true")
    args = ap.parse_args()
    import bath_amd as ba
    from bath_amd import synth
    import bench
    ctx = ba.Context(0)
    ctx.set_fs_strict(True)
    has = hasattr(ctx, "set_std_ensemble")
    modes = (0, 2) if has else (0,)
    if not args.no_plain:
        hmm = ba.HMM(os.path.join(ROOT, "tests", "golden", "PTH2.bhmm"))
        om = ba.OProfile(ctx, ba.Profile(hmm))
        wins = multi_copy_block(ba, synth, hmm, args.genes)
        dna = ba.SeqBlock(ctx, wins)
        pipe = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct)
        print("# plain block: %d windows, %d of them with a two- or three-copy ORF, PTH2.bhmm (M = %d)" % (len(wins), args.genes, hmm.M), flush=True)

        def run():
            _, dm, nclust = pipe.run_hits(dna, arrays=True)
            return len(dm), nclust, pipe.kernel_times()
        ab(ctx, run, (lambda m: ctx.set_std_ensemble(m)) if has else (lambda m: None), modes, args.passes, "plain")
        del dna
    if not args.no_fs:
        hmm = ba.HMM(bench.MODEL)
        om = ba.OProfile(ctx, ba.Profile(hmm))
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
        flat, offsets, _ = synth.dna_windows(args.fs_windows, args.length, seed=4242, hmm=hmm, frameshift=True)
        dna = ba.SeqBlock(ctx, flat, offsets)
        pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
        print("# --fs block: %d windows of %d nt, %s (M = %d); both ensemble switches" % (args.fs_windows, args.length, os.path.basename(bench.MODEL), hmm.M), flush=True)

        def run_fs():
            _, _, dm, nclust = pipe.run_frameshift_domains(om3, om5, dna, arrays=True)
            return len(dm), nclust, pipe.kernel_times()

        def set_both(m):
            ctx.set_fs_ensemble(m)
            if has:
                ctx.set_std_ensemble(m)
        ab(ctx, run_fs, set_both, modes, args.passes, "fs")
    ctx.close()


if __name__ == "__main__":
    main()
