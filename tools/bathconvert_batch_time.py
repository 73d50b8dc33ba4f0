#!/usr/bin/env python
"""Measures profiles/bathconvert_batch_time.json on one GPU: what bathconvert --batch N buys.

Workload: a 96-model file, the 12-model fixture of tests/calib_common.py (the reference's tutorial/tRNA-proteins.hmm) eight times.

1. bathconvert --batch 1 against --batch 4, 12 and 32 (and, with --parent DIR, the bathconvert of another checkout of this project --
   the parent commit, built -- without the option): every run in a fresh process, five counted after one uncounted, the legs
   alternating; seconds inside run() and process wall time, medians with the raw values.  The legs' output files must be the same bytes.
2. In one process: calibrate_fs_batch over the fixture's 12 models against the 12 serial calibrate_fs calls, five counted after one
   uncounted, alternating: host time of the call(s), device time per launch from the library's kernel timers.  The two batch
   kernels' launches run beside each other on two streams, so their device times overlap; the serial calls' do not.
3. The same batch call under the launch-shape switches of bath_fs_chain.hip (BATH_HIP_CALIB_BATCH_W: windows per block capped;
   BATH_HIP_CALIB_BATCH_SOLO=1: a block has its CU to itself), each in a process of its own: what the builder's choice was measured against.

Every step is a child process under a time limit of its own; the first that fails, is killed by a signal or runs into its limit ends
the script with its status, and nothing is started after it.
usage: tools/bathconvert_batch_time.py [--parent DIR] [out.json]"""
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
CHILD = ("import sys, time; from bath_amd import bathconvert as b; t = time.perf_counter(); rc = b.run(sys.argv[1:], stdout=open(sys.argv[-2] + '.txt', 'w')); "
         "print('INSIDE %.6f' % (time.perf_counter() - t)); sys.exit(rc)")
BATCHES = (1, 4, 12, 32)
SHAPES = ({}, {"BATH_HIP_CALIB_BATCH_W": "8"}, {"BATH_HIP_CALIB_BATCH_W": "2"}, {"BATH_HIP_CALIB_BATCH_W": "1"},
          {"BATH_HIP_CALIB_BATCH_SOLO": "1"}, {"BATH_HIP_CALIB_BATCH_SOLO": "1", "BATH_HIP_CALIB_BATCH_W": "2"})
ROUNDS = 6                                                  # the first is not counted


def step(argv, limit, env=None, root=ROOT):
    """One child process under its own time limit; a failure ends the script."""
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=root, env=dict(os.environ, PYTHONPATH=root, **(env or {})), capture_output=True, text=True)
    w = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("step %s ended with status %d: nothing further is started" % (" ".join(argv[-4:]), p.returncode))
    return p.stdout, w


def inprocess():
    """Step 2 (and 3, under the environment it is started with): prints one JSON line."""
    import bath_amd as ba
    import calib_common as cc
    hmms = [ba.HMM(cc.HMM_IN, i) for i in range(ba.HMM.count(cc.HMM_IN))]
    tables = [1] * len(hmms)
    ctx = ba.Context(0)
    s0 = ba.rng_state(ba.CALIB_SEED)
    serial, batch = [], []
    want = None
    for r in range(ROUNDS):
        t = time.perf_counter()
        state, k3, k5, taus = s0, 0.0, 0.0, []
        for h in hmms:
            t3, t5, state = ba.calibrate_fs(ctx, h, 1, state)
            taus.append((t3, t5))
            kt = ba.kernel_times(ctx)
            k3 += kt["fs3_fwd_kernel"][0]
            k5 += kt["fs5_fwd_parser_kernel"][0]
        host = time.perf_counter() - t
        if r:
            serial.append({"host_ms": host * 1e3, "fs3_fwd_kernel_ms": k3, "fs5_fwd_parser_kernel_ms": k5})
        t = time.perf_counter()
        b3, b5, bstate = ba.calibrate_fs_batch(ctx, hmms, tables, s0)
        host = time.perf_counter() - t
        kt = ba.kernel_times(ctx)
        if (state, taus) != (bstate, list(zip(b3.tolist(), b5.tolist()))):
            raise SystemExit("the batch's taus or state differ from the serial calls'")
        want = taus
        if r:
            batch.append({"host_ms": host * 1e3, "fs3_fwd_batch_kernel_ms": kt["fs3_fwd_batch_kernel"][0], "fs3_launches": kt["fs3_fwd_batch_kernel"][1],
                          "fs5_fwd_parser_batch_kernel_ms": kt["fs5_fwd_parser_batch_kernel"][0], "fs5_launches": kt["fs5_fwd_parser_batch_kernel"][1]})
    ctx.close()
    med = lambda rows, k: statistics.median(r[k] for r in rows)
    print("RESULT " + json.dumps({"models": [(h.name, h.M) for h in hmms], "serial_12_calls": serial, "batch_1_call": batch,
                                  "serial_host_ms_median": med(serial, "host_ms"), "batch_host_ms_median": med(batch, "host_ms"),
                                  "serial_kernels_ms_median": med(serial, "fs3_fwd_kernel_ms") + med(serial, "fs5_fwd_parser_kernel_ms"),
                                  "batch_fs3_ms_median": med(batch, "fs3_fwd_batch_kernel_ms"), "batch_fs5_ms_median": med(batch, "fs5_fwd_parser_batch_kernel_ms"),
                                  "n_taus_equal": len(want)}))


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--inprocess"]:
        return inprocess()
    parent = None
    if argv[:1] == ["--parent"]:
        parent, argv = os.path.abspath(argv[1]), argv[2:]
    out_json = argv[0] if argv else os.path.join(ROOT, "profiles", "bathconvert_batch_time.json")
    import calib_common as cc
    legs = (["parent"] if parent else []) + ["batch%d" % b for b in BATCHES]
    inside, wall, digest = {m: [] for m in legs}, {m: [] for m in legs}, set()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "x8.hmm")
        with open(cc.HMM_IN, "rb") as fh:
            one = fh.read()
        with open(src, "wb") as fh:
            fh.write(one * 8)
        for r in range(ROUNDS):
            for m in legs:
                out = os.path.join(d, "o%d%s.bhmm" % (r, m))
                opts = [] if m == "parent" else ["--batch", m[5:]]
                stdout, w = step([sys.executable, "-c", CHILD] + opts + [out, src], 300, root=parent if m == "parent" else ROOT)
                with open(out, "rb") as fh:
                    digest.add(fh.read())
                os.remove(out)
                if r:
                    wall[m].append(w)
                    inside[m].append(float(stdout.split("INSIDE")[1]))
    if len(digest) != 1:
        raise SystemExit("the legs wrote different files")
    shapes = []
    for env in SHAPES:
        stdout, _ = step([sys.executable, os.path.abspath(__file__), "--inprocess"], 300, env=env)
        shapes.append({"env": env, **json.loads(stdout.split("RESULT ")[1])})
    one_process = shapes[0]
    res = {"what": "bathconvert --batch N on a 96-model file (tests/calib_common.HMM_IN, 12 models, eight times; 2 x 200 sequences of 300 nt per model) on one MI355X; "
                   "per leg 5 runs in fresh processes after one uncounted, the legs alternating; 'parent': the parent commit's bathconvert, no option, same session",
           "legs": {m: {"inside_process_s": inside[m], "process_wall_s": wall[m], "inside_process_s_median": statistics.median(inside[m]),
                        "process_wall_s_median": statistics.median(wall[m])} for m in legs},
           "all_legs_wrote_the_same_bytes": True,
           "one_process_12_models": {k: v for k, v in one_process.items() if k != "env"},
           "launch_shapes": [{"env": s["env"], "batch_host_ms_median": s["batch_host_ms_median"], "batch_fs3_ms_median": s["batch_fs3_ms_median"],
                              "batch_fs5_ms_median": s["batch_fs5_ms_median"], "serial_host_ms_median": s["serial_host_ms_median"]} for s in shapes]}
    b1 = res["legs"]["batch1"]["inside_process_s_median"]
    res["speedup_inside_process_vs_batch1"] = {m: b1 / res["legs"][m]["inside_process_s_median"] for m in legs}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("one_process_12_models",)}))


if __name__ == "__main__":
    main()
