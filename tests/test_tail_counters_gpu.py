"""The cascade's decision kernels count and append per block (BlockTally, bath_pipeline.hip): a block adds up its counters in
LDS, ranks the ids it appends with LDS atomics, and touches each global counter and list length once.  Held here against the oracle
(oracle/pipeline.c through oracle_lib, as test_pipeline_gpu.py drives it): the pipeline counters and every ORF record, matched by
key, with that file's tolerances on the two float-arithmetic scores and bit equality on the rest.

Every block runs in child processes (the switches are read once per process): the fused MSV stage (BATH_HIP_LANE_MIN_NT=1) and the
three kernels it replaces (BATH_HIP_MSV_WAVE=1 beside it, as test_msv_stage_gpu.py forces them), each as one part and as two
(BATH_HIP_LANES).  The blocks:
  few          fewer candidates than one block of 256
  odd          F1 = 1.0, every ORF a candidate: more than one block, the last one partly filled
  iid          random DNA without a planted domain: blocks in which no lane passes, a flush with nothing to add
  grid_stride  F1 = 1.0 and enough windows that the candidates are more than twice the decision grid's 4 x CUs x 256 threads, so
               that a block of the one-part runs takes a third round of candidates.  A striding kernel parks up to 512 ids per
               list and writes its lists out inside the loop when a round begins with more than 256 parked: after two rounds
               that each parked nearly 256, at the earliest.  In the one-part three-kernel run classify_kernel (every ORF is
               undecided after SSV, in practice) and f1_bias_kernel (at F1 = 1.0 every ORF passes, and all but the ~F2 = 1e-3 of
               them with the best MSV scores go to todo_vit) do that in every block that has a third round.  The two-part runs
               halve the candidates per part, and the fused stage has no loop: those stay at one flush per block.  The other
               striding kernels (post_vit, post_vit_local, post_vit2) park a small share of their candidates and reach the
               write-out inside the loop in no test: it is the same function, on the same barriers.
  overflow     `odd` again with a candidate list of 300 (BATH_HIP_TEST_CANDCAP): the pass that overflows is repeated

The oracle is the slow side: it scores every ORF of the F1 = 1.0 blocks on a CPU core (~65 us each), so grid_stride is shared
out over a pool of processes while the GPU runs go on beside it.  Timed on the CPU tier, without a GPU, at the 256 CUs of an
MI355X: 17 477 windows, 627 465 ORFs (2.39 grids), 5.0 s for the oracle on 8 cores; the other three blocks together 0.7 s.

The work lists themselves stay on the device and no entry point returns them, so they are checked through what reads them: a
list with a hole leaves an ORF without the next stage's score or status, one with a duplicate counts its residues twice in
cells_vit / cells_fwd (res_vit, res_fwd) or its ORF twice in n_past_fwd / pos_past_fwd -- all compared below, ORF by ORF."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "golden", "Caudal_act.bhmm")
COUNTERS = ("nres", "n_orfs", "n_past_msv", "n_past_bias", "n_past_vit", "n_past_fwd",
            "pos_past_msv", "pos_past_bias", "pos_past_vit", "pos_past_fwd", "cells_msv", "cells_vit", "cells_fwd")
ORFS_PER_KB = 33          # ORFs of >= 20 codons in 1 kb of iid DNA, both strands: ~36; a low estimate, the test checks the count it got
ROUNDS = 2.2              # grid_stride's candidates, in decision grids: past 2, a block's third round, with a margin
RUNS = {"fused1": {"BATH_HIP_LANE_MIN_NT": "1", "BATH_HIP_LANES": "1"},
        "fused2": {"BATH_HIP_LANE_MIN_NT": "1", "BATH_HIP_LANES": "2"},
        "three1": {"BATH_HIP_LANE_MIN_NT": "1", "BATH_HIP_MSV_WAVE": "1", "BATH_HIP_LANES": "1"},
        "three2": {"BATH_HIP_LANE_MIN_NT": "1", "BATH_HIP_MSV_WAVE": "1", "BATH_HIP_LANES": "2"}}
OVERFLOW = {"BATH_HIP_LANE_MIN_NT": "1", "BATH_HIP_LANES": "1", "BATH_HIP_TEST_CANDCAP": "300"}
OPTS = {"few": {}, "odd": {"F1": 1.0}, "iid": {}, "grid_stride": {"F1": 1.0}}
OVERFLOW_CASES = ("odd",)                                  # (`few` has fewer ORFs than the list of 300 holds)


def grid_stride_windows(cus):
    """The number of 1 kb windows whose ORFs are more than twice the decision kernels' grid (4 blocks per CU, 256 threads each)."""
    return int(ROUNDS * 4 * cus * 256) // ORFS_PER_KB + 1


def build_blocks(cus):
    import bath_amd as ba
    import common
    import oracle_lib as ol
    from bath_amd import synth
    model = ol.Model(MODEL)
    rng = np.random.default_rng(31)

    def planted(n):
        return [common.revtranslate(rng, aa, model.basic) for aa in common.emit_from_model(rng, model, n, flank=10, sharpen=2.0)]
    blocks = {"few": common.random_dna(rng, 3, 600) + planted(5),
              "odd": common.random_dna(rng, 40, 900) + planted(10),
              "iid": common.random_dna(rng, 2000, 600)}
    n = grid_stride_windows(cus)
    flat, _, _ = synth.dna_windows(n, 1000, seed=32, hmm=ba.HMM(MODEL))
    blocks["grid_stride"] = list(flat.reshape(n, 1000))
    return blocks


def oracle_dtype():
    import ctypes as C
    import oracle_lib as ol
    dt = np.dtype([(f, np.dtype(t)) for f, t in ol.OrfResult._fields_], align=True)
    assert dt.itemsize == C.sizeof(ol.OrfResult)
    return dt


def oracle_chunk(job):
    """The oracle's pipeline over windows first..first+len(wins)-1 of a block: (counters, raw records past MSV, their windows)."""
    import oracle_lib as ol
    first, wins, opts = job
    pli, ores, per_seq = ol.Model(MODEL).run_pipeline(wins, opts=dict(opts))
    window = np.zeros(len(ores), dtype=np.int64)
    for w, (a, b) in enumerate(per_seq):
        window[a:b] = first + w
    keep = np.array([o.stage >= 1 for o in ores], dtype=bool)
    raw = b"".join(bytes(o) for o, k in zip(ores, keep) if k)
    return [int(getattr(pli, c)) for c in COUNTERS], raw, window[keep]


def oracle_run(pool, wins, opts, per_job=600):
    """(counters, records as a structured array sorted by (window, strand, frame, start), their windows) of the oracle's pipeline.
    The windows are independent and every counter is a sum over them: a large block is shared out over the pool's processes
    (the oracle scores every ORF of the F1 = 1.0 blocks on one CPU core each, ~75 us per ORF)."""
    jobs = [(a, wins[a:a + per_job], opts) for a in range(0, len(wins), per_job)]
    parts = pool.map(oracle_chunk, jobs) if len(jobs) > 1 else [oracle_chunk(j) for j in jobs]
    counters = {c: sum(p[0][i] for p in parts) for i, c in enumerate(COUNTERS)}
    rec = np.frombuffer(b"".join(p[1] for p in parts), dtype=oracle_dtype())
    window = np.concatenate([p[2] for p in parts])
    order = np.lexsort((rec["start"], rec["frame"], rec["strand"], window))
    return counters, rec[order], window[order]


def child(blocks_path, out_path, names):
    import bath_amd as ba
    z = np.load(blocks_path)
    ctx = ba.Context(0)
    hmm = ba.HMM(MODEL)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    out = {}
    for name in names:
        flat, off = z[name + ":flat"], z[name + ":off"]
        wins = [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        pipe = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct, **OPTS[name])
        stats, res = pipe.run(ba.SeqBlock(ctx, wins))
        launches = {n: k for n, _, k in pipe.timings()}
        out[name + ":launches"] = np.array([launches.get("classify_msv", -1), launches.get("f1_bias", -1)], dtype=np.int64)
        out[name + ":counters"] = np.array([getattr(stats, c) for c in COUNTERS], dtype=np.int64)
        out[name + ":records"] = np.frombuffer(res.tobytes(), dtype=np.uint8)
    np.savez(out_path, **out)
    ctx.close()


def start_child(tmp, blocks_path, tag, names, env_set):
    env = dict(os.environ)
    for k in ("BATH_HIP_LANE_MIN_NT", "BATH_HIP_LANES", "BATH_HIP_MSV_WAVE", "BATH_HIP_TEST_CANDCAP", "BATH_HIP_TEST_WINCAP"):
        env.pop(k, None)
    env.update(env_set)
    out = os.path.join(str(tmp), tag + ".npz")
    log = open(os.path.join(str(tmp), tag + ".log"), "w+")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), blocks_path, out, json.dumps(list(names))], env=env,
                         stdout=log, stderr=subprocess.STDOUT, cwd=ROOT)
    return p, log, out


def finish_child(started):
    p, log, out = started
    try:
        rc = p.wait(timeout=600)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        rc = "timeout"
    log.seek(0)
    text = log.read()
    log.close()
    assert rc == 0, (rc, text[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def world(tmp_path_factory, gpu_ctx):
    import bath_amd as ba
    cus = ba.lib().bath_selftest_compute_units(gpu_ctx._h)
    assert cus > 0
    tmp = tmp_path_factory.mktemp("tail_counters")
    blocks = build_blocks(cus)
    packed = {}
    for name, wins in blocks.items():
        packed[name + ":flat"] = np.concatenate(wins).astype(np.uint8)
        packed[name + ":off"] = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).astype(np.int64)
    blocks_path = os.path.join(str(tmp), "blocks.npz")
    np.savez(blocks_path, **packed)
    # the five GPU runs side by side, and the oracle on the CPUs meanwhile: once, shared by every comparison below
    started = {tag: start_child(tmp, blocks_path, tag, OPTS, env) for tag, env in RUNS.items()}
    started["overflow"] = start_child(tmp, blocks_path, "overflow", OVERFLOW_CASES, OVERFLOW)
    try:
        import multiprocessing
        with multiprocessing.get_context("spawn").Pool(12) as pool:         # (spawn: this process has the GPU open)
            oracle = {name: oracle_run(pool, blocks[name], OPTS[name]) for name in OPTS}
    finally:
        runs, errors = {}, []
        for tag, st in started.items():                                       # wait for every child, whatever happened
            try:
                runs[tag] = finish_child(st)
            except AssertionError as e:
                errors.append((tag, e))
    assert not errors, errors
    return {"cus": cus, "runs": runs, "oracle": oracle}


def assert_equals_oracle(run, oracle, name):
    import bath_amd as ba
    want_c, want, want_win = oracle[name]
    got_c = dict(zip(COUNTERS, (int(x) for x in run[name + ":counters"])))
    for c in COUNTERS:
        assert got_c[c] == want_c[c], (name, c, got_c[c], want_c[c])
    got = np.frombuffer(run[name + ":records"].tobytes(), dtype=ba.ORF_RESULT_DTYPE)
    got = got[np.lexsort((got["start"], got["frame"], got["strand"], got["window"]))]
    assert len(got) == len(want), (name, len(got), len(want))
    assert np.array_equal(got["window"], want_win), name
    for f in ("strand", "frame", "start", "end", "n", "stage", "msv_status"):
        assert np.array_equal(got[f], want[f]), (name, f)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for f in ("usc", "nullsc"):                                               # integer filters: bit exact
        assert np.array_equal(bits(got[f]), bits(want[f])), (name, f)
    assert (np.abs(got["filtersc"] - want["filtersc"]) <= 1e-4 + 1e-5 * np.abs(want["filtersc"])).all(), name
    vit = np.isfinite(want["vfsc"]) | np.isinf(got["vfsc"])
    assert np.array_equal(bits(got["vfsc"][vit]), bits(want["vfsc"][vit])), name
    assert np.array_equal(got["vit_status"][vit], want["vit_status"][vit]), name
    fwd = (want["stage"] >= 3) & np.isfinite(want["fwdsc"])
    assert (np.abs(got["fwdsc"][fwd] - want["fwdsc"][fwd]) <= 2e-4 + 1e-4 * np.abs(want["fwdsc"][fwd])).all(), name


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("tag", list(RUNS))
def test_counters_and_records_equal_the_oracles(world, tag, name):
    assert_equals_oracle(world["runs"][tag], world["oracle"], name)


@pytest.mark.parametrize("name", OVERFLOW_CASES)
def test_a_pass_repeated_after_candidate_overflow_equals_the_oracle(world, name):
    assert_equals_oracle(world["runs"]["overflow"], world["oracle"], name)
    assert world["oracle"][name][0]["n_orfs"] > 300                           # the first attempt's list of 300 did overflow


def test_the_runs_took_the_paths_they_are_named_for(world):
    """The stage "f1_bias" has launches only where f1_bias_kernel ran: none behind the fused stage (a block in two parts adds up
    its parts' launches, so only the one-part runs have the exact counts of test_msv_stage_gpu.py)."""
    for name in OPTS:
        assert tuple(world["runs"]["fused1"][name + ":launches"]) == (1, 0), name
        assert tuple(world["runs"]["three1"][name + ":launches"]) == (2, 1), name
        assert world["runs"]["fused2"][name + ":launches"][0] > 0 and world["runs"]["fused2"][name + ":launches"][1] == 0, name
        assert world["runs"]["three2"][name + ":launches"][1] > 0, name


def test_the_blocks_reach_the_cases_they_are_named_for(world):
    c = {name: world["oracle"][name][0] for name in OPTS}
    # F1 = 1.0: every ORF is a candidate and passes MSV, so n_orfs counts the candidates
    assert c["odd"]["n_past_msv"] == c["odd"]["n_orfs"] and c["grid_stride"]["n_past_msv"] == c["grid_stride"]["n_orfs"]
    assert 0 < c["few"]["n_past_msv"] < 256 and c["few"]["n_past_fwd"] > 0
    assert c["odd"]["n_orfs"] > 256 and c["odd"]["n_orfs"] % 256 != 0
    assert c["iid"]["n_past_msv"] > 0 and c["iid"]["n_past_fwd"] == 0         # candidates in a few blocks of the grid, and none at the end
    # more than two decision grids of candidates: blocks 0 .. (n_orfs - 2 grids) / 256 of the one-part runs begin a third round,
    # with two full rounds' ids parked; every one of them passed the bias filter too, so f1_bias_kernel parked one id for each
    grid = 4 * world["cus"] * 256
    assert c["grid_stride"]["n_orfs"] > 2 * grid + 256
    assert c["grid_stride"]["n_past_bias"] == c["grid_stride"]["n_orfs"]
    assert c["grid_stride"]["n_past_fwd"] > 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    child(sys.argv[1], sys.argv[2], json.loads(sys.argv[3]))
