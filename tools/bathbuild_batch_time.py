#!/usr/bin/env python
"""Measures profiles/bathbuild_batch_time.json on one GPU: what bathbuild --batch N buys.

Workload: a 96-record FASTA file, the three records of tests/golden/three_seqs.fa (429, 245 and 358 residues) 32 times under
distinct names, at the default calibration sizes.

1. bathbuild --batch 1 against --batch 4, 16 and 64 (and, with --parent DIR, the bathbuild of another checkout of this project -- the
   parent commit, built -- without the option): every run in a fresh process, five counted after one uncounted, the legs alternating;
   seconds inside run() and process wall time, medians with the raw values.  The legs' model files must be the same bytes.
2. In one process: the 96 models calibrated model by model (calibrate) and in batches of 4, 16 and 64 (calibrate_batch), five counted
   after one uncounted, alternating: host ms per model, and per batch the device ms of the three standard launches and of the two
   parser launches from the library's kernel timers.  The two parsers run beside each other on two streams, so their device times
   overlap; the serial calls' do not.

Every step is a child process under a time limit of its own; the first that fails, is killed by a signal or runs into its limit ends
the script with its status, and nothing is started after it.
usage: tools/bathbuild_batch_time.py [--parent DIR] [out.json]"""
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
CHILD = ("import sys, time; from bath_amd import bathbuild as b; t = time.perf_counter(); rc = b.run(sys.argv[1:], stdout=open(sys.argv[-2] + '.txt', 'w'), date='D'); "
         "print('INSIDE %.6f' % (time.perf_counter() - t)); sys.exit(rc)")
BATCHES = (1, 4, 16, 64)
COPIES = 32
ROUNDS = 6                                                  # the first is not counted
STD = ("msv_wave_batch_kernel", "vit_wave_batch_kernel", "fwd_wave_batch_kernel")
FS = ("fs3_fwd_batch_kernel", "fs5_fwd_parser_batch_kernel")
STD_1 = ("calib_msv", "calib_vit", "calib_fwd")
FS_1 = ("fs3_fwd_kernel", "fs5_fwd_parser_kernel")


def step(argv, limit, root=ROOT):
    """One child process under its own time limit; a failure ends the script."""
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True)
    w = time.perf_counter() - t
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit("step %s ended with status %d: nothing further is started" % (" ".join(argv[-4:]), p.returncode))
    return p.stdout, w


def records():
    from bath_amd import bathbuild as bb
    three = bb.read_queries(os.path.join(ROOT, "tests", "golden", "three_seqs.fa"))
    return [("%s_%02d" % (name, c), desc, seq) for c in range(COPIES) for name, desc, seq in three]


def inprocess():
    """Step 2: prints one JSON line."""
    import bath_amd as ba
    from bath_amd import bathbuild as bb
    opts = bb.parse_options(["out", "in"])[0]
    score = ba.ScoreSystem()
    recs = records()
    E = {k: opts["--" + k] for k in ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN")}
    ctx = ba.Context(0)
    s0 = ba.rng_state(42)
    sets = ba.CalibSamples(ctx, s0, **E)
    rows = {b: [] for b in BATCHES}
    want = None
    for r in range(ROUNDS):
        for b in BATCHES:
            hmms = [bb.build_model(score, name, seq, opts) for name, _, seq in recs]
            std = fs = host = 0.0
            for i0 in range(0, len(hmms), b):
                part = hmms[i0:i0 + b]
                t = time.perf_counter()
                if b == 1:
                    ba.calibrate(ctx, part[0], 1, s0, sets, Eft=opts["--Eft"], **E)
                else:
                    ba.calibrate_batch(ctx, part, 1, s0, sets, Eft=opts["--Eft"], **E)
                host += time.perf_counter() - t
                kt = ba.kernel_times(ctx)
                std += sum(kt[k][0] for k in (STD_1 if b == 1 else STD))
                fs += sum(kt[k][0] for k in (FS_1 if b == 1 else FS))
            ev = [h.evparam.tobytes() for h in hmms]
            if want is None:
                want = ev
            if ev != want:
                raise SystemExit("batch %d: the parameters differ from the first leg's" % b)
            if r:
                n_calls = (len(hmms) + b - 1) // b
                rows[b].append({"host_ms_per_model": host * 1e3 / len(hmms), "std_device_ms_per_call": std / n_calls, "fs_device_ms_per_call": fs / n_calls, "calls": n_calls})
    sets.close()
    ctx.close()
    med = lambda b, k: statistics.median(x[k] for x in rows[b])
    print("RESULT " + json.dumps({"models": len(recs), "all_legs_gave_the_same_parameters": True,
                                  "batch": {str(b): {"runs": rows[b], "host_ms_per_model_median": med(b, "host_ms_per_model"),
                                                     "std_device_ms_per_call_median": med(b, "std_device_ms_per_call"),
                                                     "fs_device_ms_per_call_median": med(b, "fs_device_ms_per_call")} for b in BATCHES}}))


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--inprocess"]:
        return inprocess()
    parent = None
    if argv[:1] == ["--parent"]:
        parent, argv = os.path.abspath(argv[1]), argv[2:]
    out_json = argv[0] if argv else os.path.join(ROOT, "profiles", "bathbuild_batch_time.json")
    legs = (["parent"] if parent else []) + ["batch%d" % b for b in BATCHES]
    inside, wall, digest = {m: [] for m in legs}, {m: [] for m in legs}, set()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "x%d.fa" % COPIES)
        with open(src, "w") as fh:
            for name, desc, seq in records():
                fh.write(">%s %s\n%s\n" % (name, desc, seq))
        for r in range(ROUNDS):
            for m in legs:
                out = os.path.join(d, "o.bhmm")                        # one name for every leg: the run's header names it
                opts = [] if m == "parent" else ["--batch", m[5:]]
                stdout, w = step([sys.executable, "-c", CHILD] + opts + [out, src], 300, root=parent if m == "parent" else ROOT)
                with open(out, "rb") as fh:
                    digest.add(fh.read())
                os.remove(out)
                sys.stderr.write("round %d %s: %.2f s\n" % (r, m, w))
                sys.stderr.flush()
                if r:
                    wall[m].append(w)
                    inside[m].append(float(stdout.split("INSIDE")[1]))
    if len(digest) != 1:
        raise SystemExit("the legs wrote different files")
    stdout, _ = step([sys.executable, os.path.abspath(__file__), "--inprocess"], 600)
    res = {"what": "bathbuild --batch N on a 96-record FASTA file (tests/golden/three_seqs.fa, 3 records, 32 times; default calibration sizes) on one MI355X; "
                   "per leg 5 runs in fresh processes after one uncounted, the legs alternating; 'parent': the parent commit's bathbuild, no option, same session",
           "legs": {m: {"inside_process_s": inside[m], "process_wall_s": wall[m], "inside_process_s_median": statistics.median(inside[m]),
                        "inside_process_s_range": [min(inside[m]), max(inside[m])], "process_wall_s_median": statistics.median(wall[m]),
                        "process_wall_s_range": [min(wall[m]), max(wall[m])]} for m in legs},
           "all_legs_wrote_the_same_bytes": True,
           "one_process_96_models": json.loads(stdout.split("RESULT ")[1])}
    b1 = res["legs"]["batch1"]["inside_process_s_median"]
    res["speedup_inside_process_vs_batch1"] = {m: b1 / res["legs"][m]["inside_process_s_median"] for m in legs}
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "one_process_96_models"}))
    print(json.dumps({b: {k: v for k, v in row.items() if k != "runs"} for b, row in res["one_process_96_models"]["batch"].items()}))


if __name__ == "__main__":
    main()
