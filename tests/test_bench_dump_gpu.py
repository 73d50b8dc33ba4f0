"""GPU tier: `bench.py --dump-outputs DIR` writes what the timed cascade computed -- the counters of the last timed step and the
surviving ORFs' records, every value finite -- the same arrays from run to run whatever --steps is, and the same as the cascade run
here on the bench's seeded block.  bench.py is started as a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "Caudal_act.bhmm")
WINDOWS, LENGTH = 20000, 1000


def bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--windows", str(WINDOWS),
           "--length", str(LENGTH), "--no-cpu-baseline", "--no-fs", "--no-c45", "--no-streamed", "--no-concurrent", "--no-one-part",
           "--dump-outputs", out_dir]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir) if f.endswith(".npy")}


def test_dump_outputs_are_the_cascade_outputs(gpu_ctx, tmp_path):
    import bath_amd as ba
    from bath_amd import synth
    line1, d1 = bench(str(tmp_path / "one"), 1)
    line3, d3 = bench(str(tmp_path / "three"), 3)
    assert line1["steps"] == 1 and line3["steps"] == 3 and line1["ms_per_step"] > 0 and line3["ms_per_step"] > 0
    assert sorted(d1) == sorted(d3) and sum(a.nbytes for a in d1.values()) <= 64 << 20
    for name, a in d1.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
        assert np.array_equal(a, d3[name]), name

    # the same seeded block through the cascade in this process: every counter, every record
    hmm = ba.HMM(MODEL)
    flat, _, _ = synth.dna_windows(WINDOWS, LENGTH, seed=42, hmm=hmm)
    dna = ba.SeqBlock(gpu_ctx, flat, np.arange(WINDOWS + 1, dtype=np.int64) * LENGTH)
    pipe = ba.Pipeline(gpu_ctx, ba.OProfile(gpu_ctx, ba.Profile(hmm)), fs_pipe=False, ncbi_table=hmm.ct)
    stats, res = pipe.run(dna)
    for f, _ in ba.PipelineStats._fields_:
        assert d1["counter_" + f][0] == getattr(stats, f), f
    assert d1["record_stride"][0] == 1 and len(d1["record_window"]) == len(res) == stats.n_past_msv > 0
    res = res[np.lexsort((res["start"], res["frame"], res["strand"], res["window"]))]
    for f in res.dtype.names:
        got, want = d1["record_" + f], res[f].astype(d1["record_" + f].dtype)
        if res.dtype[f].kind == "f":                     # scores: the finite values and the rows they belong to
            rows = np.flatnonzero(np.isfinite(want))
            assert np.array_equal(d1["record_%s_rows" % f], rows), f
            want = want[rows]
        assert np.array_equal(got, want), f
    # a row missing from record_<score>_rows is +inf where that filter overflowed (ERANGE) and -inf where it did not run
    for f, status in (("usc", "msv_status"), ("vfsc", "vit_status"), ("fwdsc", None)):
        gone = ~np.isfinite(res[f])
        over = (res[status] == ba.ERANGE) if status else np.zeros(len(res), bool)
        assert np.array_equal(np.isposinf(res[f]), gone & over) and np.array_equal(np.isneginf(res[f]), gone & ~over), f
