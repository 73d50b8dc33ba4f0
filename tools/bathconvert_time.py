#!/usr/bin/env python
"""Measures profiles/bathconvert_time.json on one GPU: bathconvert on the reference's tutorial/tRNA-proteins.hmm (12 models; tests/calib_common.py puts it together), five runs in fresh
processes -- the conversion inside the process (bathconvert.run: context, 12 x 2 fits, rewrite) and the process wall time, medians --
and, from the library's kernel timers, the two parsers' device time per launch for M = 78 and M = 459, with the host time of the
calibration call around them.  usage: tools/bathconvert_time.py [out.json]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHILD = ("import sys, time; from bath_amd import bathconvert as b; t = time.perf_counter(); rc = b.run(sys.argv[1:], stdout=open(sys.argv[1] + '.txt', 'w')); "
         "print('INSIDE %.6f' % (time.perf_counter() - t)); sys.exit(rc)")


def main():
    import bath_amd as ba
    import calib_common as cc
    HMM_IN = cc.HMM_IN                                      # the reference's tutorial/tRNA-proteins.hmm, put together from tests/golden
    out_json = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bathconvert_time.json")
    inside, wall = [], []
    with tempfile.TemporaryDirectory() as d:
        for r in range(6):                                  # the first run warms the file cache and the code-object cache: not counted
            out = os.path.join(d, "o%d.bhmm" % r)
            t = time.perf_counter()
            p = subprocess.run([sys.executable, "-c", CHILD, out, HMM_IN], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
            w = time.perf_counter() - t
            assert p.returncode == 0, p.stderr[-2000:]
            if r:
                wall.append(w)
                inside.append(float(p.stdout.split("INSIDE")[1]))
    ctx = ba.Context(0)
    kernels = {}
    for idx in range(ba.HMM.count(HMM_IN)):
        hmm = ba.HMM(HMM_IN, idx)
        if hmm.M not in (78, 459):
            continue
        runs = []
        for r in range(6):
            t = time.perf_counter()
            ba.calibrate_fs(ctx, hmm, 1, ba.rng_state(42))
            host = time.perf_counter() - t
            kt = ba.kernel_times(ctx)
            if r:
                runs.append((host * 1e3, kt["fs3_fwd_kernel"][0] / kt["fs3_fwd_kernel"][1], kt["fs5_fwd_parser_kernel"][0] / kt["fs5_fwd_parser_kernel"][1]))
        kernels["M=%d (%s)" % (hmm.M, hmm.name)] = {"calibrate_fs_host_ms_median": statistics.median(r[0] for r in runs),
                                                    "fs3_fwd_kernel_ms_per_launch_median": statistics.median(r[1] for r in runs),
                                                    "fs5_fwd_parser_kernel_ms_per_launch_median": statistics.median(r[2] for r in runs)}
    ctx.close()
    res = {"what": "bathconvert tRNA-proteins.bhmm tRNA-proteins.hmm (12 models, 2 x 200 sequences of 300 nt each) on one MI355X; 5 runs in fresh processes after one uncounted",
           "inside_process_s": inside, "process_wall_s": wall, "inside_process_s_median": statistics.median(inside), "process_wall_s_median": statistics.median(wall),
           "parsers": kernels,
           "reference_recorded": "7.86u 0.01s, elapsed 7.90 s: the tutorial's recorded run of the same command, on its authors' CPU, another machine"}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
