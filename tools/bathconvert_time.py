#!/usr/bin/env python
"""Measures profiles/bathconvert_time.json on one GPU: bathconvert on the reference's tutorial/tRNA-proteins.hmm (12 models; tests/calib_common.py puts it together), five runs in fresh
processes -- the conversion inside the process (bathconvert.run: context, 12 x 2 fits, rewrite) and the process wall time, medians --
and, from the library's kernel timers, the two parsers' device time per launch for M = 78 and M = 459, with the host time of the
calibration call around them.  usage: tools/bathconvert_time.py [out.json]

--arith odds3|odds measures that arithmetic (bathconvert --arith, calibrate_fs(arith=)) AND strict again, alternating in the same
session on the same box, into profiles/bathconvert_time_<arith>.json: compare the two legs of that file with each other, not with
the figures of another session.  usage: tools/bathconvert_time.py --arith odds [out.json]"""
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


SPANS = {"strict": ("fs3_fwd_kernel", "fs5_fwd_parser_kernel"), "odds3": ("fs3_fwd_odds_kernel", "fs5_fwd_parser_kernel"),
         "odds": ("fs3_fwd_odds_kernel", "fs5_fwd_odds_parser_kernel")}


def main_arith(arith, argv):
    """The strict leg and the <arith> leg, alternating."""
    import bath_amd as ba
    import calib_common as cc
    out_json = argv[0] if argv else os.path.join(ROOT, "profiles", "bathconvert_time_%s.json" % arith)
    legs = ("strict", arith)
    inside, wall = {m: [] for m in legs}, {m: [] for m in legs}
    with tempfile.TemporaryDirectory() as d:
        for r in range(6):                                  # the first round is not counted
            for m in legs:
                out = os.path.join(d, "o%d%s.bhmm" % (r, m))
                t = time.perf_counter()
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, out, "--arith", m, cc.HMM_IN], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                                   capture_output=True, text=True)
                w = time.perf_counter() - t
                if p.returncode != 0:
                    raise SystemExit("bathconvert --arith %s: exit status %d\n%s" % (m, p.returncode, p.stderr[-2000:]))
                if r:
                    wall[m].append(w)
                    inside[m].append(float(p.stdout.split("INSIDE")[1]))
    ctx = ba.Context(0)
    kernels = {}
    for idx in range(ba.HMM.count(cc.HMM_IN)):
        hmm = ba.HMM(cc.HMM_IN, idx)
        if hmm.M not in (78, 459):
            continue
        runs = {m: [] for m in legs}
        for r in range(6):
            for m in legs:
                t = time.perf_counter()
                ba.calibrate_fs(ctx, hmm, 1, ba.rng_state(42), arith=m)
                host = time.perf_counter() - t
                kt = ba.kernel_times(ctx)
                if r:
                    runs[m].append((host * 1e3,) + tuple(kt[k][0] / kt[k][1] for k in SPANS[m]))
        kernels["M=%d (%s)" % (hmm.M, hmm.name)] = {m: {"calibrate_fs_host_ms_median": statistics.median(r[0] for r in runs[m]),
                                                        SPANS[m][0] + "_ms_per_launch_median": statistics.median(r[1] for r in runs[m]),
                                                        SPANS[m][1] + "_ms_per_launch_median": statistics.median(r[2] for r in runs[m])} for m in legs}
    ctx.close()
    res = {"what": "bathconvert [--arith MODE] tRNA-proteins.bhmm tRNA-proteins.hmm (12 models, 2 x 200 sequences of 300 nt each) on one MI355X; per mode 5 runs in "
                   "fresh processes after one uncounted, the modes alternating; then calibrate_fs(arith=MODE) of two models in one process, 5 calls after one uncounted",
           "modes": {m: {"inside_process_s": inside[m], "process_wall_s": wall[m], "inside_process_s_median": statistics.median(inside[m]),
                         "process_wall_s_median": statistics.median(wall[m])} for m in legs},
           "parsers": kernels}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--arith":
        if sys.argv[2] not in ("odds3", "odds"):
            raise SystemExit("--arith: odds3 or odds")
        return main_arith(sys.argv[2], sys.argv[3:])
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
