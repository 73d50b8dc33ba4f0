#!/usr/bin/env python3
"""A/B of the frameshift branch's ensemble modes: serial host ensemble (mode 0) against the device ensemble (mode 2).

bench.py's --fs block (synth.dna_windows(fs_windows, length, seed=4242, frameshift=True) of tests/golden/Caudal_act.bhmm) through
Pipeline.run_frameshift_domains, passes of the two modes alternating after a warm-up, at BATH_HIP_HOST_THREADS = 2 and 16, strict
and with both odds switches; then configs[4]'s 1024-node model against --c5-mb Mb of genome.  Per combination: wall time per pass
(median and range), fs_ensemble_kernel's device time from kernel_times(), the bytes of Forward matrices that did not go to the
host, the fallback counters.  bench.py is imported for its inputs only and is not changed.

    python tools/fs_ensemble_ab.py [--fs-windows N] [--passes K] [--c5-mb MB | --no-c5] > profiles/r10_fs_ensemble_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ab(ba, ctx, pipe, om3, om5, dna, passes, label):
    rows = []
    for threads in (2, 16):
        os.environ["BATH_HIP_HOST_THREADS"] = str(threads)
        for odds in (False, True):
            ctx.set_fs_odds(odds); ctx.set_fs5_odds(odds)
            t = {0: [], 2: []}
            kms, nclust, ndm = [], {}, {}
            for mode in (0, 2):                                   # warm-up: buffers, side contexts, odds tables
                ctx.set_fs_ensemble(mode)
                pipe.run_frameshift_domains(om3, om5, dna, arrays=True)
            c0 = ctx.fs_ensemble_counters()
            for _ in range(passes):
                for mode in (0, 2):
                    ctx.set_fs_ensemble(mode)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    _, _, dm, nc = pipe.run_frameshift_domains(om3, om5, dna, arrays=True)
                    t[mode].append((time.perf_counter() - t0) * 1e3)
                    nclust[mode], ndm[mode] = nc, len(dm)
                    if mode == 2:
                        kms.append(pipe.kernel_times().get("fs_ensemble_kernel", (0.0,))[0])
            c1 = ctx.fs_ensemble_counters()
            kept = (c1["matrix_bytes_kept"] - c0["matrix_bytes_kept"]) / passes
            for mode in (0, 2):
                rows.append((threads, odds, mode, statistics.median(t[mode]), min(t[mode]), max(t[mode])))
                print("%-6s threads %2d  %-6s  mode %d  pass %8.2f ms (min %8.2f max %8.2f, %d passes)  domains %d  clustered regions %d%s" % (
                    label, threads, "odds" if odds else "strict", mode, statistics.median(t[mode]), min(t[mode]), max(t[mode]), passes, ndm[mode], nclust[mode],
                    "  fs_ensemble_kernel %.3f ms  matrices kept on the device %.1f MB/pass  fallbacks: bound %d overflow %d" % (
                        statistics.median(kms), kept / 1e6, c1["bound_fallbacks"] - c0["bound_fallbacks"], c1["overflow_fallbacks"] - c0["overflow_fallbacks"]) if mode == 2 else ""),
                      flush=True)
    ctx.set_fs_odds(False); ctx.set_fs5_odds(False); ctx.set_fs_ensemble(0)
    os.environ.pop("BATH_HIP_HOST_THREADS", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs-windows", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--c5-mb", type=float, default=125.0)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--no-fs", action="store_true")
    args = ap.parse_args()
    import bath_amd as ba
    from bath_amd import dist as bdist, synth
    import bench
    ctx = ba.Context(0)
    ctx.set_fs_strict(True)
    if not args.no_fs:
        hmm = ba.HMM(bench.MODEL)
        om = ba.OProfile(ctx, ba.Profile(hmm))
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
        flat, offsets, _ = synth.dna_windows(args.fs_windows, args.length, seed=4242, hmm=hmm, frameshift=True)
        dna = ba.SeqBlock(ctx, flat, offsets)
        pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
        print("# --fs block: %d windows of %d nt, %s (M = %d)" % (args.fs_windows, args.length, os.path.basename(bench.MODEL), hmm.M), flush=True)
        ab(ba, ctx, pipe, om3, om5, dna, args.passes, "fs")
        del dna
    if not args.no_c5:
        hmm, g, planted = bench.c5_genome(ba, synth, int(args.c5_mb * 1e6))
        om = ba.OProfile(ctx, ba.Profile(hmm))
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=hmm.ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=hmm.ct))
        wins = bdist.split_targets([len(g)], hmm.max_length)
        blk = ba.SeqBlock(ctx, [g[s:s + n] for _, s, n, _ in wins]); blk.set_context([c for _, _, _, c in wins])
        pipe = ba.Pipeline(ctx, om, fs_pipe=True, ncbi_table=hmm.ct)
        print("# configs[4]: %d-node model against %.0f Mb (%d genome windows)" % (hmm.M, args.c5_mb, len(wins)), flush=True)
        ab(ba, ctx, pipe, om3, om5, blk, max(2, args.passes // 2), "c5")
    ctx.close()


if __name__ == "__main__":
    main()
