"""The cascade's fused MSV stage (msv_stage_kernel: SSV status, MSV with the J state, F1 and the bias filter in one kernel, a lane
per candidate) against the three kernels it replaces on large blocks.

Blocks of test size take classify_kernel + the wave-per-ORF MSV + f1_bias_kernel; BATH_HIP_LANE_MIN_NT=1 (read once per process)
sends them through the fused stage.  Every case below runs once in a child process with the variable set and once in one without
it; the two must agree on the ten pipeline counters and on every field of every ORF record, floats by their bits.  A child with
BATH_HIP_MSV_WAVE=1 beside the first variable keeps the three kernels in front of the same Viterbi path as the fused run.  The blocks
with planted domains are also held against the oracle's counters.  A third child adds BATH_HIP_LANES=2, so that a block's parts
run the stage side by side and their records merge."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COUNTERS = ("nres", "n_orfs", "n_past_msv", "n_past_bias", "n_past_vit", "n_past_fwd",
            "pos_past_msv", "pos_past_bias", "pos_past_vit", "pos_past_fwd")
# (file, model index, M): NR = 76 (the bench's tile), the smallest tile, and the middle ones
MODELS = {"Caudal_act": ("Caudal_act.bhmm", 0, 145), "TruB_C": ("tRNA-proteins.bhmm", 11, 56), "Trm56": ("tRNA-proteins.bhmm", 6, 121),
          "Thg1": ("tRNA-proteins.bhmm", 5, 131), "tRNA-Thr_ED": ("tRNA-proteins.bhmm", 10, 136)}
STOP = np.array([3, 0, 0], dtype=np.uint8)          # TAA


def synth_block(name):
    import bath_amd as ba
    from bath_amd import synth
    f, idx, M = MODELS[name]
    hmm = ba.HMM(os.path.join(HERE, "golden", f), idx)
    assert hmm.M == M
    flat, offsets, _ = synth.dna_windows(3000, 600, seed=100 + M, hmm=hmm)
    return list(flat.reshape(3000, 600))


def planted(rng, n, sharpen=2.0):
    import common
    import oracle_lib as ol
    model = ol.Model(os.path.join(HERE, "golden", "Caudal_act.bhmm"), 0)
    return [common.revtranslate(rng, aa, model.basic) for aa in common.emit_from_model(rng, model, n, flank=1, sharpen=sharpen)]


def short_orfs():
    """ORFs of every length from 4 to 43 codons, each a piece of a planted domain between two stop codons: lengths 0-3 mod 4 and
    below 8 (the bias filter's dword reads and byte tail, the row loop's last partial group of eight residues)."""
    rng = np.random.default_rng(21)
    doms = planted(rng, 40)
    wins = []
    for rep in range(3):
        for n, d in zip(range(4, 44), doms):
            a = int(rng.integers(0, max(1, len(d) // 3 - n))) * 3
            wins.append(np.concatenate([STOP, d[a:a + 3 * n], STOP, rng.integers(0, 4, size=int(rng.integers(0, 3))).astype(np.uint8)]))
    return wins


def degenerate():
    import common
    rng = np.random.default_rng(22)
    wins = common.random_dna(rng, 40, 600, degenerate_frac=0.03)
    for d in planted(rng, 20):
        d = d.copy()
        d[rng.integers(0, len(d), size=4)] = rng.choice([5, 9, 15], size=4)      # ambiguous codons inside a domain: residue X
        wins.append(d)
    return wins


def overflowing():
    rng = np.random.default_rng(23)
    return [np.concatenate([d] * 4) for d in planted(rng, 6, sharpen=3.0)]


def no_survivors():
    import common
    return common.random_dna(np.random.default_rng(25), 8, 600)          # under an F1 no ORF of random DNA reaches


def mixed():
    import common
    rng = np.random.default_rng(24)
    return common.random_dna(rng, 300, 900) + planted(rng, 37)


# name -> (model, windows, pipeline options)
CASES = {
    "synth_Caudal_act": ("Caudal_act", lambda: synth_block("Caudal_act"), {}),
    "synth_TruB_C": ("TruB_C", lambda: synth_block("TruB_C"), {}),
    "synth_Trm56": ("Trm56", lambda: synth_block("Trm56"), {}),
    "synth_Thg1": ("Thg1", lambda: synth_block("Thg1"), {}),
    "synth_tRNA-Thr_ED": ("tRNA-Thr_ED", lambda: synth_block("tRNA-Thr_ED"), {}),
    "short_orfs": ("Caudal_act", short_orfs, {"min_orf_len": 4, "F1": 0.3}),
    "degenerate": ("Caudal_act", degenerate, {}),
    "overflowing": ("Caudal_act", overflowing, {}),
    "no_survivors": ("Caudal_act", no_survivors, {"F1": 1e-12}),
    "mixed": ("Caudal_act", mixed, {}),
    "mixed_nobias": ("Caudal_act", mixed, {"do_biasfilter": 0}),
    "mixed_top_strand": ("Caudal_act", mixed, {"strands": 1}),
    "mixed_bottom_strand": ("Caudal_act", mixed, {"strands": 2}),
}
MERGED = ("mixed", "synth_Caudal_act")          # the cases the BATH_HIP_LANES=2 child runs


def child(out_path, names):
    """Runs the named cases on the GPU; the counters and the records' raw bytes go to <out_path>."""
    import bath_amd as ba
    ctx = ba.Context(0)
    out = {}
    for name in names:
        model, build, opts = CASES[name]
        f, idx, _ = MODELS[model]
        hmm = ba.HMM(os.path.join(HERE, "golden", f), idx)
        om = ba.OProfile(ctx, ba.Profile(hmm))
        pipe = ba.Pipeline(ctx, om, fs_pipe=False, ncbi_table=hmm.ct, **opts)
        stats, res = pipe.run(ba.SeqBlock(ctx, build()))
        launches = {n: k for n, _, k in pipe.timings()}
        out[name + ":launches"] = np.array([launches.get("classify_msv", -1), launches.get("f1_bias", -1)], dtype=np.int64)
        out[name + ":counters"] = np.array([getattr(stats, c) for c in COUNTERS], dtype=np.int64)
        out[name + ":records"] = np.frombuffer(res.tobytes(), dtype=np.uint8)
    np.savez(out_path, **out)
    ctx.close()


def run_child(tmp, tag, names, **env_set):
    env = dict(os.environ)
    for k in ("BATH_HIP_LANE_MIN_NT", "BATH_HIP_LANES", "BATH_HIP_MSV_WAVE"):
        env.pop(k, None)
    env.update(env_set)
    out = os.path.join(str(tmp), tag + ".npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out, json.dumps(list(names))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("msv_stage")
    return {"wave": run_child(tmp, "wave", CASES),
            "three": run_child(tmp, "three", CASES, BATH_HIP_LANE_MIN_NT="1", BATH_HIP_MSV_WAVE="1"),
            "fused": run_child(tmp, "fused", CASES, BATH_HIP_LANE_MIN_NT="1"),
            "fused2": run_child(tmp, "fused2", MERGED, BATH_HIP_LANE_MIN_NT="1", BATH_HIP_LANES="2")}


def records(run, name):
    import bath_amd as ba
    return np.frombuffer(run[name + ":records"].tobytes(), dtype=ba.ORF_RESULT_DTYPE)


def assert_same(a, b, name):
    ca, cb = a[name + ":counters"], b[name + ":counters"]
    for c, x, y in zip(COUNTERS, ca, cb):
        assert x == y, (name, c, int(x), int(y))
    ra, rb = records(a, name), records(b, name)
    assert len(ra) == len(rb), name
    for f in ra.dtype.names:                              # field by field (the records carry padding bytes), floats by their bits
        assert ra[f].tobytes() == rb[f].tobytes(), (name, f)


@pytest.mark.parametrize("name", list(CASES))
def test_fused_stage_equals_three_kernels(runs, name):
    assert_same(runs["wave"], runs["fused"], name)


@pytest.mark.parametrize("name", list(CASES))
def test_fused_stage_equals_three_kernels_before_the_same_viterbi_path(runs, name):
    """BATH_HIP_LANE_MIN_NT=1 also sends the Viterbi stage down its lane path.  With BATH_HIP_MSV_WAVE=1 beside it the MSV stage
    keeps its three kernels and everything behind it is the fused run's: a difference here is the MSV stage's."""
    assert_same(runs["three"], runs["fused"], name)


def test_the_fused_run_is_the_fused_path(runs):
    """The stage names stay in the timings on both paths; their launch counts tell which one ran: msv_stage_kernel,
    then nothing, against classify_kernel + the MSV kernel, then f1_bias_kernel."""
    for name in CASES:
        assert tuple(runs["fused"][name + ":launches"]) == (1, 0), name
        assert tuple(runs["wave"][name + ":launches"]) == (2, 1), name
        assert tuple(runs["three"][name + ":launches"]) == (2, 1), name


@pytest.mark.parametrize("name", MERGED)
def test_fused_stage_in_two_parts(runs, name):
    assert_same(runs["wave"], runs["fused2"], name)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("synth_")])
def test_fused_stage_counters_equal_the_oracles(runs, name):
    import oracle_lib as ol
    f, idx, _ = MODELS[CASES[name][0]]
    pli, _, _ = ol.Model(os.path.join(HERE, "golden", f), idx).run_pipeline(CASES[name][1]())
    got = dict(zip(COUNTERS, runs["fused"][name + ":counters"]))
    for c in COUNTERS:
        assert int(got[c]) == getattr(pli, c), (name, c)
    assert got["n_past_msv"] > got["n_past_fwd"] > 0      # the block exercises every stage


def test_cases_reach_the_edges_they_are_named_for(runs):
    import bath_amd as ba
    r = records(runs["fused"], "short_orfs")
    lens = set(int(n) for n in r["n"])
    assert min(lens) < 8 and {0, 1, 2, 3} <= {n % 4 for n in lens} and {1, 2, 3} <= {n % 4 for n in lens if n >= 8}
    assert (r["stage"] >= 2).any()                                       # ... and some of them went through the bias filter
    r = records(runs["fused"], "overflowing")
    over = r[r["msv_status"] == ba.ERANGE]
    # (their P-value of 0 at this stage sends them on; the records hold the P of the last stage they reached: compared above, bit for bit)
    assert len(over) > 0 and np.isinf(over["usc"]).all() and (over["usc"] > 0).all() and (over["stage"] >= 2).all()
    assert len(records(runs["fused"], "no_survivors")) == 0 and runs["fused"]["no_survivors:counters"][COUNTERS.index("n_orfs")] > 0
    for name in ("mixed", "degenerate"):                                 # a last wave that is not full
        assert len(records(runs["fused"], name)) % 64 != 0
    nb, wb = records(runs["fused"], "mixed_nobias"), records(runs["fused"], "mixed")
    assert len(nb) > 0 and (nb["filtersc"][nb["stage"] >= 1] == nb["nullsc"][nb["stage"] >= 1]).all() and (wb["filtersc"] != wb["nullsc"]).any()
    top, bot = records(runs["fused"], "mixed_top_strand"), records(runs["fused"], "mixed_bottom_strand")
    assert len(top) > 0 and len(bot) > 0 and len(top) + len(bot) == len(wb) and len(set(top["strand"])) == 1 and len(set(bot["strand"])) == 1 and top["strand"][0] != bot["strand"][0]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    child(sys.argv[1], json.loads(sys.argv[2]))
