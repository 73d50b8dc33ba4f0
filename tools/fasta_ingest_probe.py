"""FASTA ingest measured: a seeded synthetic genome (bath_amd.synth.genome, several targets, one longer than block_length,
60-column lines) written as FASTA, then

  read_s      host read() of the file into page-locked memory, chunk by chunk
  feed_s      FastaTargets.feed of those chunks: H2D of the raw bytes + the ingest kernels (wall, synchronous per chunk)
  h2d_s       the raw bytes' H2D alone, from the same page-locked buffer, one chunk at a time
  cli_s       `python -m bath_amd.bathsearch q.bhmm genome.fa` (plain pipeline) as a child process
  cascade_s   the resident cascade (Pipeline.run) over the same windows, built once on the device

The ingest kernels' device times come from a separate run under rocprofv3 (--kernel: only the parse, no CLI):

  python tools/fasta_ingest_probe.py --mb 1000 --out profiles/fasta_ingest_probe.json
  rocprofv3 --kernel-trace --stats -d <dir> -o ingest -- python tools/fasta_ingest_probe.py --mb 1000 --kernel
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bath_amd as ba  # noqa: E402
from bath_amd import dist, synth  # noqa: E402


def write_genome(path, n_nt, hmm, seed=1234):
    g, _ = synth.genome(n_nt, seed=seed, hmms=[hmm], genes_per_model=max(4, n_nt // 2_000_000))
    cuts = [0, n_nt // 2, n_nt // 2 + 30_000, n_nt // 2 + 400_000, n_nt]     # one target far longer than block_length
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as fh:
        for i in range(len(cuts) - 1):
            s = lut[g[cuts[i]:cuts[i + 1]]]
            fh.write(b">chr%d synthetic\n" % i)
            full = len(s) // 60 * 60
            body = np.concatenate([s[:full].reshape(-1, 60), np.full((full // 60, 1), ord("\n"), np.uint8)], axis=1).tobytes()
            fh.write(body)
            if len(s) > full:
                fh.write(s[full:].tobytes() + b"\n")


def parse(ctx, path, chunk):
    pinned = ba.PinnedBuffer(chunk)
    ft = ba.FastaTargets(ctx)
    t_read = t_feed = 0.0
    with open(path, "rb", buffering=0) as fh:
        while True:
            t0 = time.perf_counter()
            n = fh.readinto(memoryview(pinned.array)[:chunk])
            t1 = time.perf_counter()
            if not n:
                break
            ft.feed(pinned, n)
            t2 = time.perf_counter()
            t_read += t1 - t0
            t_feed += t2 - t1
    ft.finish()
    ctx.synchronize()
    return ft, t_read, t_feed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=1000.0)
    ap.add_argument("--chunk_mb", type=int, default=256)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--kernel", action="store_true", help="only parse the file (for a rocprofv3 run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", action="store_true", help="keep the generated FASTA file")
    a = ap.parse_args()
    hmmfile = os.path.join(ROOT, "tests", "golden", "Caudal_act.bhmm")
    hmm = ba.HMM(hmmfile)
    path = os.path.join(a.dir, "bath_ingest_probe_%d.fa" % int(a.mb))
    n_nt = int(a.mb * 1e6)
    if not os.path.exists(path):
        write_genome(path, n_nt, hmm)
    size = os.path.getsize(path)
    chunk = a.chunk_mb << 20
    ctx = ba.Context(0)
    ft, t_read, t_feed = parse(ctx, path, chunk)
    res = {"file_bytes": size, "nucleotides": int(ft.records()["length"].sum()), "records": len(ft), "chunk_bytes": chunk,
           "read_s": t_read, "feed_s": t_feed}
    if a.kernel:
        print(json.dumps(res))
        return
    # H2D of the raw bytes alone, from the same page-locked buffer
    import torch
    pinned = ba.PinnedBuffer(chunk)
    host = torch.frombuffer(pinned.array, dtype=torch.uint8)
    dev = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    left = size
    while left > 0:
        k = min(chunk, left)
        dev[:k].copy_(host[:k], non_blocking=True)
        left -= k
    torch.cuda.synchronize()
    res["h2d_s"] = time.perf_counter() - t0
    # the resident cascade over the same windows
    wins = ft.windows(hmm.max_length, dist.BLOCK_LENGTH)
    blk = ft.seqs(wins)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    pipe = ba.Pipeline(ctx, om)
    pipe.run(blk, want_results=False)
    ctx.synchronize()
    t0 = time.perf_counter()
    stats, _ = pipe.run(blk, want_results=False)
    ctx.synchronize()
    res["cascade_s"] = time.perf_counter() - t0
    res["windows"] = len(wins)
    del blk, ft
    ctx.close()
    # the whole CLI, plain pipeline, in a child process
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-m", "bath_amd.bathsearch", "-o", os.devnull, hmmfile, path],
                       env=env, capture_output=True, text=True)
    res["cli_s"] = time.perf_counter() - t0
    res["cli_rc"] = p.returncode
    res["ingest_GBps_wall"] = size / t_feed / 1e9 if t_feed else None
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if not a.keep:
        os.remove(path)


if __name__ == "__main__":
    main()
