"""CPU tier of `bathsearch --gpus N` (bath_amd/bathsearch.py): the option's parsing, refusals that happen in the parent before any
rank starts, the plan every rank computes alone (items, owners, nres_before), and the split of the host threads among the ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import bathsearch as bs
from bath_amd import dist
from test_bathsearch_cpu import REFUSED_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMM = os.path.join(ol.GOLDEN, "PTH2.bhmm")
FA = os.path.join(ol.GOLDEN, "target-PTH2.fa")


@pytest.mark.parametrize("bad", [["--gpus", "0"], ["--gpus", "17"], ["--gpus", "x"], ["--gpus=-1"], ["--gpus=2.5"]])
def test_bad_gpus_values_exit_1_naming_the_option(bad, capsys, monkeypatch):
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    assert bs.run(bad + [HMM, FA]) == 1
    assert "--gpus" in capsys.readouterr().err


def test_missing_gpus_value_exits_1(capsys, monkeypatch):
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    assert bs.run([HMM, FA, "--gpus"]) == 1
    assert "--gpus" in capsys.readouterr().err


def test_gpus_parses_and_adds_no_header_line():
    opts, h, s = bs.parse_args(["--gpus", "4", "-o", "x.out", HMM, FA])
    assert opts["--gpus"] == 4 and (h, s) == (HMM, FA)
    without, _, _ = bs.parse_args(["-o", "x.out", HMM, FA])
    assert bs.output_header(opts, h, s) == bs.output_header(without, h, s)
    for n in (1, 16):
        assert bs.parse_args(["--gpus=%d" % n, HMM, FA])[0]["--gpus"] == n


@pytest.mark.parametrize("extra", REFUSED_CASES)
def test_refusals_happen_before_any_rank_starts(extra, capsys, monkeypatch):
    """Every refusal of the single-GPU driver is the same with --gpus 2, and no child process is started for it."""
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: pytest.fail("a child process was started"))
    argv = extra + [HMM, FA]
    assert bs.run(argv) == 1
    want = capsys.readouterr().err
    assert bs.run(["--gpus", "2"] + argv) == 1
    assert capsys.readouterr().err == want


def test_refused_inputs_before_any_rank_starts(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    q = tmp_path / "q.fa"
    q.write_text(">q\nMKVLAAGIVG\n")
    gz = tmp_path / "t.fa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00rest")
    for argv in ([str(q), FA], [HMM, str(gz)], [HMM, str(tmp_path / "missing.fa")]):
        assert bs.run(argv) == 1
        want = capsys.readouterr().err
        assert bs.run(["--gpus", "3"] + argv) == 1
        assert capsys.readouterr().err == want


def test_codon_table_mismatch_refused_in_the_parent(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(bs, "launch_ranks", lambda *a, **k: pytest.fail("a rank was launched"))
    out = tmp_path / "o.txt"
    argv = ["--gpus", "2", "--ct", "1", "-o", str(out), os.path.join(ol.GOLDEN, "MET-ct4.bhmm"), os.path.join(ol.GOLDEN, "target-MET.fa")]
    assert bs.run(argv) == 1
    assert "codon translation tabel ID 1" in capsys.readouterr().err
    opts, h, s = bs.parse_args(argv)
    assert out.read_text() == bs.output_header(opts, h, s)           # what the single-GPU driver leaves: the header, no [ok]


def test_no_gpu_visible_fails_cleanly_once(tmp_path):
    """On a machine without a GPU the ranks start and every one of them refuses: the message is printed once, status 1, no
    output file presented as complete and no child left behind."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(PYTHONPATH=ROOT, BATH_SEARCH_SHARE_DEVICE="1", BATH_SEARCH_BACKEND="gloo", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "bath_amd.bathsearch", "--gpus", "3", "-o", "out.txt", HMM, FA],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert p.returncode == 1, p.stderr
    assert p.stderr.count("Error:") == 1 and "--gpus 3" in p.stderr, p.stderr
    assert "[ok]" not in ((tmp_path / "out.txt").read_text() if (tmp_path / "out.txt").exists() else "")
    assert not _children_with(str(tmp_path))


def _children_with(marker):
    """Live processes whose command line or working directory names <marker>."""
    found = []
    for pid in os.listdir("/proc"):
        if not pid.isdigit() or int(pid) == os.getpid():
            continue
        try:
            if os.readlink("/proc/%s/cwd" % pid).startswith(marker):
                found.append(int(pid))
        except OSError:
            pass
    return found


def synthetic_windows(rng, n_records, max_length, block_length):
    """A FASTA window table (FASTA_WINDOW_DTYPE) laid out as the device ingest lays it out (dist.split_targets)."""
    lengths = [int(x) for x in rng.integers(1, 3 * block_length, size=n_records)]
    w = dist.split_targets(lengths, max_length, block_length)
    out = np.zeros(len(w), dtype=ba.FASTA_WINDOW_DTYPE)
    for i, (t, s, n, c) in enumerate(w):
        out[i] = (t, s, n, c)
    return out


def single_gpu_nres_before(wins, block_nt, strand_factor=2):
    """The block loop of _search_items: nres before every window, accumulated block by block (stats.nres of each block)."""
    before, acc = {}, 0
    cut = bs.block_cuts(wins["n"], block_nt)
    for a, b in zip(cut[:-1], cut[1:]):
        for i in range(a, b):
            before[i] = acc + strand_factor * int(sum(int(wins[j]["n"]) - int(wins[j]["context"]) for j in range(a, i)))
        acc += strand_factor * int(sum(int(x["n"]) - int(x["context"]) for x in wins[a:b]))
    return before


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("strand", ["both", "plus"])
def test_plan_covers_every_window_once(world, strand):
    rng = np.random.default_rng(7 + world)
    Ms = [56, 120, 459, 80, 300, 99, 200]
    wins = [synthetic_windows(rng, int(rng.integers(1, 9)), int(M * 1.3), 50_000) for M in Ms]
    plan = bs.search_plan(wins, Ms, world, strand)
    assert plan and all(0 <= it.owner < world for it in plan)
    for q, w in enumerate(wins):
        items = sorted((it for it in plan if it.query == q), key=lambda it: it.lo)
        assert items[0].lo == 0 and items[-1].hi == len(w)                          # every window in exactly one item, contiguous
        assert all(a.hi == b.lo for a, b in zip(items, items[1:])) and all(it.hi > it.lo for it in items)
        ref = single_gpu_nres_before(w, 256_000_000, 2 if strand == "both" else 1)
        assert [it.nres_before for it in items] == [ref[it.lo] for it in items]
        small = single_gpu_nres_before(w, 60_000, 2 if strand == "both" else 1)     # small blocks: the same counts
        assert [it.nres_before for it in items] == [small[it.lo] for it in items]
    again = bs.search_plan(wins, Ms, world, strand)
    assert [repr(x) for x in again] == [repr(x) for x in plan]
    if world > 1:
        assert len({it.owner for it in plan}) > 1


def test_plan_splits_the_large_query_across_ranks():
    rng = np.random.default_rng(3)
    Ms = [56, 459, 80]
    wins = [synthetic_windows(np.random.default_rng(11), 6, int(M * 1.3), 50_000) for M in Ms]
    plan = bs.search_plan(wins, Ms, 3)
    big = [it for it in plan if it.query == 1]
    assert len(big) > 1 and len({it.owner for it in big}) > 1


def test_host_threads_split_affinity_and_omp(monkeypatch):
    def boom():
        raise AssertionError("os.cpu_count() was read")
    monkeypatch.setattr(os, "cpu_count", boom)
    aff = set(range(40))
    assert bs.host_threads_per_rank(4, environ={}, affinity=aff) == 10
    assert bs.host_threads_per_rank(3, environ={}, affinity=aff) == 13
    assert bs.host_threads_per_rank(4, environ={"OMP_NUM_THREADS": "16"}, affinity=aff) == 4
    assert bs.host_threads_per_rank(4, environ={"OMP_NUM_THREADS": "400"}, affinity=aff) == 10
    assert bs.host_threads_per_rank(16, environ={"OMP_NUM_THREADS": "8"}, affinity=aff) == 1
    assert bs.host_threads_per_rank(2, environ={"OMP_NUM_THREADS": "junk"}, affinity=aff) == 20
    assert bs.host_threads_per_rank(2, environ={}) == max(1, len(os.sched_getaffinity(0)) // 2)
    assert bs.host_threads_per_rank(4, environ={"BATH_HIP_HOST_THREADS": "7"}, affinity=aff) is None


def test_rank_env_keeps_a_user_set_thread_count(monkeypatch):
    monkeypatch.setattr(os, "cpu_count", lambda: 10 ** 6)
    user = {"BATH_HIP_HOST_THREADS": "7", "RANK": "5"}
    env = bs.rank_env(3, 1, 1234, environ=user, threads=bs.host_threads_per_rank(3, environ=user))
    assert env["BATH_HIP_HOST_THREADS"] == "7"
    assert (env["RANK"], env["LOCAL_RANK"], env["WORLD_SIZE"], env["MASTER_PORT"]) == ("1", "1", "3", "1234")
    env = bs.rank_env(3, 2, 1234, environ={"OMP_NUM_THREADS": "12"}, threads=bs.host_threads_per_rank(3, environ={"OMP_NUM_THREADS": "12"},
                                                                                                     affinity=set(range(64))))
    assert env["BATH_HIP_HOST_THREADS"] == "4"
    assert env["PYTHONPATH"].split(os.pathsep)[0] == ROOT


def test_item_payload_round_trip():
    st = ba.PipelineStats()
    st.nres, st.n_orfs = 123, 45
    blob = bs._pack_item(2, 0, 17, st, [(5, 100), (7, 200)], b"STREAM") + bs._pack_item(3, 1, 0, ba.PipelineStats(), [], b"")
    got = list(bs._unpack_items(blob))
    assert [(q, piece, lo) for q, piece, lo, *_ in got] == [(2, 0, 17), (3, 1, 0)]
    assert got[0][3]["nres"] == 123 and got[0][3]["n_orfs"] == 45
    assert got[0][4].tolist() == [[5, 100], [7, 200]] and got[0][5] == b"STREAM"
    assert len(got[1][4]) == 0 and got[1][5] == b""


def test_hit_stream_carries_traces():
    """A hit stream written with traces reads back as the domains and the six trace arrays alidisplay_print takes."""
    doms = []
    for w in range(3):
        d = ba.FsDomain(); d.window = w; d.iali = 10 + w; d.jali = 40 + w; d.bitscore = 20.5 + w; d.cigar = "%dM" % (30 + w); d.reported = 1; d.lnP = -10.0 - w
        doms.append(d)
    traces = []
    for n in (4, 0, 6):
        t = ba.DomainTrace(0, n, 3 + n, 1, n % 2)
        traces.append((t, np.arange(n, dtype=np.int8), np.arange(n, dtype=np.int32) * 2, np.arange(n, dtype=np.int32) + 7,
                       np.full(n, 3, np.int8), np.linspace(0, 1, n, dtype=np.float32)))
    stream = ba.HitArray.from_domains(doms).to_bytes(traces=traces)
    back = ba.HitArray.traces_from_bytes(stream)
    assert len(back) == 3
    for (d, tr), want_d, want_t in zip(back, doms, traces):
        assert (d.window, d.iali, d.jali, d.bitscore) == (want_d.window, want_d.iali, want_d.jali, want_d.bitscore)
        assert (tr[0].N, tr[0].win_start, tr[0].orf_start, tr[0].frameshift) == (want_t[0].N, want_t[0].win_start, 1, want_t[0].frameshift)
        for a, b in zip(tr[1:], want_t[1:]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    th = ba.TopHits()
    th.add_serialized(stream, ["a", "b", "c"], [100, 100, 100], descs=["x", "", "z"])
    th.finalize(300, 100)
    assert sorted(idx for _, idx, _ in th.hits()) == [0, 1, 2]
    with pytest.raises(ba.BathError):
        ba.TopHits().add_serialized(stream, ["a", "b"], [100, 100])               # window 2 names no target
