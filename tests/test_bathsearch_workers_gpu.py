"""GPU tier of `bathsearch --workers N`: the queries of a model file searched side by side on N contexts of one GPU write the
N = 1 search's main output and --tblout byte for byte (but for the timing lines and the tail's option, directory and date lines),
resident or streamed targets, one rank or two; a failing query ends the search the same way with one worker and with two; and the
library rule underneath: one FastaTargets, its windows gathered for other contexts from several threads at once.  Every search is
a fresh child process under a time limit; only recorded fixtures are searched."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from test_bathsearch_gpu import env_free_heads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORED = ("# CPU time:", "# Mc/sec:", "# Option settings:", "# Current dir:", "# Date:")
DB = "tRNA-proteins.bhmm"
STAT_FIELDS = [f for f, _ in ba.PipelineStats._fields_]


def normalise(text):
    """The lines of a main output or a --tblout file without the timing lines and the trailer's option, directory and date lines."""
    return [ln for ln in text.split("\n") if not ln.startswith(IGNORED)]


def cli(cwd, argv, timeout=300, expect=0, run_kw=None, multi=False):
    """The driver in a fresh child process: `python -m bath_amd.bathsearch`, or bathsearch.run(argv, **run_kw)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT
    if multi:
        env.update(BATH_SEARCH_SHARE_DEVICE="1", BATH_SEARCH_BACKEND="gloo")
    if run_kw is None:
        cmd = [sys.executable, "-m", "bath_amd.bathsearch"]
    else:
        cmd = [sys.executable, "-c", "import sys; from bath_amd import bathsearch as b; sys.exit(b.run(sys.argv[1:], **%r))" % (run_kw,)]
    p = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd + argv, cwd=str(cwd), env=env, capture_output=True, text=True)
    if p.returncode in (124, 134, 137, 139):        # a time limit, an abort or a segmentation fault: nothing more is started on this GPU
        pytest.exit("bathsearch %s ended with status %d:\n%s" % (" ".join(argv), p.returncode, p.stderr[-3000:]), returncode=p.returncode)
    assert p.returncode == expect, (p.returncode, p.stderr[-3000:])
    return p


def fresh_dir(base, name, files):
    d = base / name
    d.mkdir()
    for f in files:                                 # a recorded fixture by name, or any file by its path
        shutil.copy(os.path.join(ol.GOLDEN, f), d / os.path.basename(f))
    return d


def search(base, name, argv, files, outs=("out.txt",), **kw):
    """One search in its own directory: the normalised text of every file of <outs>."""
    d = fresh_dir(base, name, files)
    cli(d, argv, **kw)
    return {f: normalise((d / f).read_text()) for f in outs}


MET = (["--ct", "4", "-o", "MET-ct4.out", "MET-ct4.bhmm", "target-MET.fa"], ["MET-ct4.bhmm", "target-MET.fa"])     # the recorded command
TWELVE = {"plain": ["--block_length", "50000", "-o", "out.txt", "--tblout", "hits.tbl", DB],
          "fs": ["--fs", "--cigar", "--block_length", "50000", "-o", "out.txt", "--tblout", "hits.tbl", DB]}
_serial = {}


def serial(tmp_path_factory, key, argv, files, outs=("out.txt",)):
    """The --workers 1 search of a command, run once per module."""
    if key not in _serial:
        _serial[key] = search(tmp_path_factory.mktemp("serial"), "run", ["--workers", "1"] + argv, files, outs)
    return _serial[key]


@pytest.mark.parametrize("n", [2, 3])            # two queries: a worker each, and more workers than queries
def test_two_queries_equal_one_worker_and_the_recorded_run(tmp_path, tmp_path_factory, n):
    argv, files = MET
    want = serial(tmp_path_factory, "met", argv, files, ("MET-ct4.out",))
    got = search(tmp_path, "w%d" % n, ["--workers", str(n)] + argv, files, ("MET-ct4.out",))["MET-ct4.out"]
    assert got == want["MET-ct4.out"]
    assert got[-2] == "[ok]" and sum(ln.startswith("Query:") for ln in got) == 2
    recorded = normalise(open(os.path.join(ol.GOLDEN, "MET-ct4.out")).read())
    assert env_free_heads(got) == env_free_heads(recorded)


def test_absent_option_is_one_worker(tmp_path, tmp_path_factory):
    argv, files = MET
    assert search(tmp_path, "none", argv, files, ("MET-ct4.out",)) == serial(tmp_path_factory, "met", argv, files, ("MET-ct4.out",))


@pytest.fixture(scope="module")
def planted_fa(tmp_path_factory):
    """What the existing twelve-model searches pair the database with: a seeded synthetic target with genes of the 12 models
    planted (bath_amd.synth), here 180 kb in four records, one of them three windows of --block_length 50000 long."""
    from bath_amd import synth
    db = os.path.join(ol.GOLDEN, DB)
    hmms = [ba.HMM(db, q) for q in range(ba.HMM.count(db))]
    lens = [120_000, 7_000, 51_000, 2_500]
    g, _ = synth.genome(sum(lens), seed=91, hmms=hmms, genes_per_model=2)
    path = tmp_path_factory.mktemp("planted") / "planted.fa"
    with open(path, "w") as fh:
        p = 0
        for i, n in enumerate(lens):
            text = "".join("ACGT"[c] for c in g[p:p + n])
            fh.write(">rec%d planted record %d\n" % (i, i))
            fh.writelines(text[k:k + 70] + "\n" for k in range(0, n, 70))
            p += n
    return str(path)


@pytest.mark.parametrize("target", ["target-MET.fa", "planted.fa"])
@pytest.mark.parametrize("mode", ["plain", "fs"])
def test_twelve_queries_on_four_workers(tmp_path, tmp_path_factory, planted_fa, mode, target):
    argv, files, outs = TWELVE[mode] + [target], [DB, planted_fa if target == "planted.fa" else target], ("out.txt", "hits.tbl")
    want = serial(tmp_path_factory, "db-%s-%s" % (mode, target), argv, files, outs)
    assert sum(ln.startswith("Query:") for ln in want["out.txt"]) == 12 and want["out.txt"][-2] == "[ok]"
    if target == "planted.fa":                      # the recorded MET target holds no gene of these models; the planted one does
        assert sum(1 for ln in want["hits.tbl"] if ln and not ln.startswith("#")) >= 6
    got = search(tmp_path, "w4", ["--workers", "4"] + argv, files, outs)
    assert got["hits.tbl"] == want["hits.tbl"]
    assert got["out.txt"] == want["out.txt"]


def concatenated(d, name, parts):
    with open(d / name, "wb") as out:
        for f in parts:
            out.write(open(os.path.join(ol.GOLDEN, f), "rb").read())


def test_streamed_targets_shared_and_released_under_two_workers(tmp_path):
    """Thirteen recorded records in one target file, three recorded models in one query file; a device budget of 8 kB and uploads
    of 4 kB cut the targets into several pieces that are parsed, searched by both workers and released, batch after batch."""
    d = tmp_path / "run"
    d.mkdir()
    concatenated(d, "targets.fa", ["target-PTH2.fa", "target-MET.fa", "2OG-FeII_Oxy_3-nt.fa", "target-AMP_N.fa"])
    concatenated(d, "q.bhmm", ["PTH2.bhmm", "2OG-FeII_Oxy_3.bhmm", "AMP_N.bhmm"])
    argv = ["-o", "out.txt", "--tblout", "hits.tbl", "--cigar", "q.bhmm", "targets.fa"]
    cli(d, ["--workers", "1"] + argv)
    want = {f: normalise((d / f).read_text()) for f in ("out.txt", "hits.tbl")}
    assert sum(1 for ln in want["hits.tbl"] if ln and not ln.startswith("#")) >= 3
    cli(d, ["--workers", "2"] + argv, run_kw=dict(resident_bytes=8000, chunk_bytes=4096))
    got = {f: normalise((d / f).read_text()) for f in ("out.txt", "hits.tbl")}
    assert got == want


def test_two_ranks_of_two_workers(tmp_path, tmp_path_factory, planted_fa):
    argv, files, outs = TWELVE["plain"] + ["planted.fa"], [DB, planted_fa], ("out.txt", "hits.tbl")
    want = serial(tmp_path_factory, "db-plain-planted.fa", argv, files, outs)
    got = search(tmp_path, "g2w2", ["--gpus", "2", "--workers", "2"] + argv, files, outs, timeout=600, multi=True)
    assert got == want


def test_a_model_of_another_codon_table_ends_the_search_there(tmp_path):
    """The second of three models carries codon table 4: the first query's block is written, nothing of the third, one message."""
    models = open(os.path.join(ol.GOLDEN, DB)).read().split("//\n")[:3]
    assert all("CODON TABLE  1\n" in m for m in models)
    models[1] = models[1].replace("CODON TABLE  1\n", "CODON TABLE  4\n")
    argv = ["-o", "out.txt", "--tblout", "hits.tbl", "q.bhmm", "target-MET.fa"]
    ends = []
    for name, extra in (("workers", ["--workers", "2"]), ("serial", [])):
        d = fresh_dir(tmp_path, name, ["target-MET.fa"])
        (d / "q.bhmm").write_text("//\n".join(models) + "//\n")
        p = cli(d, extra + argv, expect=1)
        ends.append((p.stderr, normalise((d / "out.txt").read_text()), normalise((d / "hits.tbl").read_text())))
    names = [ba.HMM(str(d / "q.bhmm"), q).name for q in range(3)]
    for err, out, tbl in ends:
        assert err.count("Error:") == 1 and "codon translation tabel ID 1 does not match" in err, err
        assert "--ct 4" in err and "Traceback" not in err
        assert [ln.split()[1] for ln in out if ln.startswith("Query:")] == names[:1] and out.count("//") == 1 and "[ok]" not in out
        assert "[ok]" not in tbl
    assert ends[0] == ends[1]                       # one worker ends the same way


def test_streamed_targets_a_failing_query_in_the_middle_of_a_batch(tmp_path):
    """Streamed targets in several pieces, three models in one batch, the second with another codon table: the first query still
    gets every piece and is written, with two workers and with one; nothing of the second and third."""
    models = [open(os.path.join(ol.GOLDEN, f)).read() for f in ("PTH2.bhmm", "2OG-FeII_Oxy_3.bhmm", "AMP_N.bhmm")]
    assert "CODON TABLE  1\n" in models[1]
    models[1] = models[1].replace("CODON TABLE  1\n", "CODON TABLE  4\n")
    argv = ["-o", "out.txt", "--tblout", "hits.tbl", "q.bhmm", "targets.fa"]
    ends = []
    for name, extra, kw in (("workers", ["--workers", "2"], dict(resident_bytes=8000, chunk_bytes=4096)), ("serial", [], {})):
        d = fresh_dir(tmp_path, name, [])
        concatenated(d, "targets.fa", ["2OG-FeII_Oxy_3-nt.fa", "target-MET.fa", "target-AMP_N.fa", "target-PTH2.fa"])
        (d / "q.bhmm").write_text("".join(models))
        p = cli(d, extra + argv, expect=1, run_kw=kw)
        ends.append((p.stderr, normalise((d / "out.txt").read_text()), normalise((d / "hits.tbl").read_text())))
    for err, out, tbl in ends:
        assert err.count("Error:") == 1 and "codon translation tabel ID 1 does not match" in err and "Traceback" not in err, err
        assert [ln.split()[1] for ln in out if ln.startswith("Query:")] == ["PTH2"] and any(ln.startswith(">> ") for ln in out)
    assert ends[0] == ends[1]


# ------------------------------------------------------------------------------------------------------------------------
# the library rule: one FastaTargets, blocks gathered for other contexts from their threads
# ------------------------------------------------------------------------------------------------------------------------

def same_block(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def side_by_side(jobs):
    """Runs the callables on a thread each, started together; their results in order (a raised exception is raised here)."""
    out, start = [None] * len(jobs), threading.Barrier(len(jobs))

    def call(i):
        try:
            start.wait(30)
            out[i] = ("ok", jobs[i]())
        except BaseException as e:                  # noqa: B036 -- handed to the caller below
            out[i] = ("raised", e)

    th = [threading.Thread(target=call, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
        assert not t.is_alive()
    for kind, v in out:
        if kind == "raised":
            raise v
    return [v for _, v in out]


def test_one_resident_target_gathered_for_two_other_contexts(gpu_ctx):
    hmm = ba.HMM(os.path.join(ol.GOLDEN, "MET-ct4.bhmm"), 1)
    ft = ba.FastaTargets(gpu_ctx)
    for f in ("target-PTH2.fa", "target-MET.fa", "2OG-FeII_Oxy_3-nt.fa", "target-AMP_N.fa"):
        data = open(os.path.join(ol.GOLDEN, f), "rb").read()
        for i in range(0, len(data), 5000):
            ft.feed(data[i:i + 5000])
    ft.finish()
    assert len(ft) == 13
    w = ft.windows(100, 7000)                       # the 35 kb record in six windows with context, the short ones whole
    assert len(w) > 13 and (w["context"] > 0).any() and (w["n"] % 16 != 0).any()
    own = ft.seqs(w)
    want = own.read()
    assert want[0].size >= int(w["n"].sum()) + 64 and np.array_equal(want[2], w["n"]) and np.array_equal(want[3], w["context"])

    def pass_on(ctx, blk):
        pipe = ba.Pipeline(ctx, ba.OProfile(ctx, ba.Profile(hmm)), fs_pipe=False, ncbi_table=4)
        stats, dm, _ = pipe.run_hits(blk)
        return [int(getattr(stats, f)) for f in STAT_FIELDS], [bytes(d) for d in dm]

    want_pass = pass_on(gpu_ctx, own)
    assert want_pass[0][STAT_FIELDS.index("nres")] > 0 and len(want_pass[1]) >= 1
    others = [ba.Context(0), ba.Context(0)]
    try:
        def gather_and_search(ctx, windows):
            def job():
                blocks = [ft.seqs(windows, ctx=ctx) for _ in range(3)]           # several gathers of each thread overlap the other's
                assert all(b.ctx is ctx for b in blocks)
                return [b.read() for b in blocks], pass_on(ctx, blocks[-1])
            return job

        for reads, got_pass in side_by_side([gather_and_search(c, w) for c in others]):
            assert all(same_block(r, want) for r in reads)
            assert got_pass == want_pass
        # an error is the consumer's; the targets stay usable
        bad = w[:1].copy()
        bad["n"] = 10 ** 9
        with pytest.raises(ba.BathError, match="outside its target"):
            ft.seqs(bad, ctx=others[0])
        assert same_block(ft.seqs(w, ctx=others[0]).read(), want)
        # release the first four records while both other contexts keep gathering windows of the records that stay: release waits for
        # the gathers in flight, and every block, gathered before the codes moved or after, holds what the owner's block held
        rest = w[w["target"] >= 4]
        first = int(np.flatnonzero(w["target"] >= 4)[0])
        a = int(want[1][first])
        kept = (want[0][a:], want[1][first:] - a, want[2][first:], want[3][first:])

        def keep_gathering(ctx):
            return lambda: [ft.seqs(rest, ctx=ctx).read() for _ in range(25)]

        reads_1, reads_2, _ = side_by_side([keep_gathering(others[0]), keep_gathering(others[1]), lambda: ft.release(4)])
        assert all(same_block(r, kept) for r in reads_1 + reads_2)
        want_rest = ft.seqs(rest).read()
        assert same_block(want_rest, kept)
        assert np.array_equal(want_rest[2], rest["n"]) and np.array_equal(want_rest[3], rest["context"])
        for x, off in zip(rest, want_rest[1]):
            assert np.array_equal(want_rest[0][off:off + x["n"]], ft.codes(int(x["target"]), int(x["start0"]), int(x["n"])))
        for reads, _ in side_by_side([gather_and_search(c, rest) for c in others]):
            assert all(same_block(r, want_rest) for r in reads)
        with pytest.raises(ba.BathError, match="released"):
            ft.seqs(w[:1], ctx=others[1])
    finally:
        own = None
        for c in others:
            c.close()
