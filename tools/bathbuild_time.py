"""Times bathbuild on tests/golden/three_seqs.fa on one MI355X: profiles/bathbuild_time.json.

    python tools/bathbuild_time.py [--runs 5] [--out profiles/bathbuild_time.json]

Five fresh processes, medians over them.  Per process: its wall time as the parent sees it (interpreter start, library load and
context creation included), the time inside bathbuild.run, and per model the host time of its calibration call and the device
spans of its kernels (HIP events on the context's stream: calib_msv, calib_vit, calib_fwd and the two frameshift parsers).  The first
model of a process pays the one-time costs (code-object load, the resident sample sets); it is reported on its own.  The
reference's tutorial records 4.58 s of CPU for the same three models on another machine's CPU: quoted, no ratio is stated."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from compact_json import dump
FASTA = os.path.join(ROOT, "tests", "golden", "three_seqs.fa")


def child(out_path):
    import io
    import bath_amd as ba
    from bath_amd import bathbuild as bb
    models = []

    class Timed(bb.GpuCalibrator):
        def calibrate(self, hmm, state):
            t = time.perf_counter()
            after = super().calibrate(hmm, state)
            host_ms = (time.perf_counter() - t) * 1e3
            models.append({"name": hmm.name, "M": hmm.M, "calibrate_host_ms": host_ms,
                           "kernel_ms": {k: v[0] for k, v in ba.kernel_times(self.ctx).items()}})
            return after

    t0 = time.perf_counter()
    st = bb.run([out_path, FASTA], stdout=io.StringIO(), calibrator=Timed)
    print(json.dumps({"status": st, "in_process_s": time.perf_counter() - t0, "models": models}))
    return st



def main(argv):
    if "--child" in argv:
        return child(argv[argv.index("--child") + 1])
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 5
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "bathbuild_time.json")
    import tempfile
    recs = []
    with tempfile.TemporaryDirectory() as d:
        for r in range(runs):
            t = time.perf_counter()
            p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", os.path.join(d, "m%d.bhmm" % r)],
                               capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
            wall = time.perf_counter() - t
            if p.returncode != 0:                                   # a failed run ends the measurement: nothing more is started
                sys.stderr.write(p.stderr[-2000:])
                return p.returncode
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["process_wall_s"] = wall
            recs.append(rec)
    med = statistics.median
    names = [m["name"] for m in recs[0]["models"]]
    per_model = []
    for i, name in enumerate(names):
        ks = sorted({k for r in recs for k in r["models"][i]["kernel_ms"]})
        per_model.append({"name": name, "M": recs[0]["models"][i]["M"], "calibrate_host_ms_median": med(r["models"][i]["calibrate_host_ms"] for r in recs),
                          "kernel_ms_median": {k: med(r["models"][i]["kernel_ms"].get(k, 0.0) for r in recs) for k in ks}})
    doc = {"what": "bathbuild three_seqs.bhmm three_seqs.fa (three models: 429, 245, 358 nodes), default options, one MI355X; medians of %d fresh processes" % runs,
           "runs": runs, "process_wall_s_median": med(r["process_wall_s"] for r in recs), "in_process_s_median": med(r["in_process_s"] for r in recs),
           "process_wall_s": [r["process_wall_s"] for r in recs], "in_process_s": [r["in_process_s"] for r in recs],
           "models": per_model,
           "reference_tutorial": "documentation/userguide/tutorial.md, Practice 3 records '# CPU time: 4.58u 0.01s' for the same command on another machine's CPU; no ratio is stated"}
    with open(out, "w") as fh:
        fh.write(dump(doc))
    print(json.dumps(doc, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
