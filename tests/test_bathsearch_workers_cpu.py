"""CPU tier of `bathsearch --workers N` (bath_amd/bathsearch.py): the option's parsing, the ordered writer that puts the queries'
texts back into query order and bounds how many queries are alive, the worker pool's behaviour when a query fails, and the split
of the host threads among the worker contexts.  Threads are ordered with events; nothing sleeps."""
import os
import threading

import pytest

import oracle_lib as ol
from bath_amd import bathsearch as bs

HMM = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")
FA = os.path.join(ol.GOLDEN, "target-MET.fa")
WAIT = 30.0                                     # an event that does not come within this fails the test instead of hanging it


@pytest.mark.parametrize("bad", [["--workers", "0"], ["--workers", "9"], ["--workers", "x"], ["--workers=-1"], ["--workers=2.5"]])
def test_bad_workers_values_exit_1_naming_the_option(bad, capsys, monkeypatch):
    monkeypatch.setattr(bs, "_workers_search", lambda *a, **k: pytest.fail("a search was started"))
    assert bs.run(bad + [HMM, FA]) == 1
    assert "--workers" in capsys.readouterr().err
    with pytest.raises(bs.UsageError, match="--workers"):
        bs.parse_args(bad + [HMM, FA])


def test_workers_parses_adds_no_header_line_and_shows_in_the_trailer():
    opts, h, s = bs.parse_args(["--workers", "3", "-o", "x.out", HMM, FA])
    assert opts["--workers"] == 3 and (h, s) == (HMM, FA)
    without, _, _ = bs.parse_args(["-o", "x.out", HMM, FA])
    assert bs.output_header(opts, h, s) == bs.output_header(without, h, s)
    for n in (1, bs.MAX_WORKERS):
        assert bs.parse_args(["--workers=%d" % n, HMM, FA])[0]["--workers"] == n
    assert bs.parse_args([HMM, FA])[0].get("--workers", 1) == 1
    argv = ["--workers", "3", "--tblout", "t.tbl", HMM, FA]
    assert "--workers 3" in bs.spoof_cmdline(argv)
    assert "# Option settings: bathsearch --workers 3 --tblout t.tbl" in bs.tabular_tail(HMM, FA, argv)
    assert bs.parse_args(["--gpus", "2", "--workers", "2", HMM, FA])[0] == {"--gpus": 2, "--workers": 2}


def test_ordered_writer_emits_in_query_order_whatever_order_they_finish_in():
    """Eight queries finish in a scrambled order, the last one first: a text is written once every earlier one is."""
    n, order = 8, [7, 3, 0, 5, 1, 2, 6, 4]
    written = []
    w = bs.OrderedWriter(lambda q, text: written.append((q, text)), bound=n)
    go = [threading.Event() for _ in range(n)]
    done = [threading.Event() for _ in range(n)]

    def render(q):
        w.admit()
        assert go[q].wait(WAIT)
        w.put(q, "text %d" % q)
        done[q].set()

    threads = [threading.Thread(target=render, args=(q,)) for q in range(n)]
    for t in threads:
        t.start()
    want_after = {7: [], 3: [], 0: [0], 5: [0], 1: [0, 1], 2: [0, 1, 2, 3], 6: [0, 1, 2, 3], 4: list(range(8))}
    for q in order:
        go[q].set()
        assert done[q].wait(WAIT)
        assert [x for x, _ in written] == want_after[q]
    for t in threads:
        t.join(WAIT)
        assert not t.is_alive()
    assert written == [(q, "text %d" % q) for q in range(n)]
    assert w.alive == 0 and not w.held and w.max_held <= n and w.max_alive <= n


@pytest.mark.parametrize("workers", [2, 3])
def test_no_more_than_2n_queries_are_alive(workers):
    """Query 0 does not finish until the test lets it: the workers finish the queries after it, and stop picking new ones up when
    2N are alive (picked up and not yet written).  The bound is checked by the test's own count at every pick-up, and by the
    writer's."""
    bound, nq = 2 * workers, 20
    lock = threading.Lock()
    started, written = [], []
    release0, full = threading.Event(), threading.Event()
    w = bs.OrderedWriter(lambda q, text: written.append(q), bound=bound)

    def work(wk, rnd, q):
        with lock:
            started.append(q)
            alive = len(started) - len(written)
            assert alive <= bound, (started, written)
            if alive == bound:
                full.set()
        if q == 0:
            assert release0.wait(WAIT)
        w.put(q, "t")

    pool = bs.WorkerPool(workers, work, w)
    try:
        pool.submit(bs.Round(range(nq), admit=True))
        assert full.wait(WAIT)                      # 2N picked up, none written: query 0 holds them all back
        with w.cv:
            assert w.cv.wait_for(lambda: len(w.held) == bound - 1, WAIT)      # every other one has finished and is held
            assert sorted(started) == list(range(bound)) and written == [] and w.alive == bound
        release0.set()
        pool.wait()
    finally:
        release0.set()
        pool.close()
    assert written == list(range(nq))
    assert w.max_alive <= bound and w.max_held <= bound
    assert not any(t.is_alive() for t in pool.threads)


def test_rounds_run_in_order_and_jobs_in_the_order_given():
    seen = []
    lock = threading.Lock()

    def work(wk, rnd, q):
        with lock:
            seen.append((rnd.payload, q))

    pool = bs.WorkerPool(1, work)
    try:
        pool.submit(bs.Round([2, 0, 1], "a"))
        pool.submit(bs.Round([5, 4], "b"))
        pool.wait()
    finally:
        pool.close()
    assert seen == [("a", 2), ("a", 0), ("a", 1), ("b", 5), ("b", 4)]


@pytest.mark.parametrize("k", [0, 4, 9])
def test_a_failure_at_query_k_writes_the_queries_before_it_and_nothing_after(k):
    """Query k raises while query k - 2 is still running and later queries have finished or are running: the queries before k are
    all written, nothing from k on, the failure comes out of wait() once, and every thread ends."""
    workers, nq = 3, 10
    written, ran = [], []
    lock = threading.Lock()
    failed = threading.Event()
    w = bs.OrderedWriter(lambda q, text: written.append(q), bound=2 * workers)

    def work(wk, rnd, q):
        with lock:
            ran.append(q)
        if q == k:
            failed.set()
            raise RuntimeError("query %d failed" % q)
        if q == k - 2:
            assert failed.wait(WAIT)                # still in flight when k fails: it is finished all the same
        if pool.cancelled(q):
            raise bs.Cancelled()
        w.put(q, "t")

    before = threading.active_count()
    pool = bs.WorkerPool(workers, work, w)
    try:
        pool.submit(bs.Round(range(nq), admit=True))
        with pytest.raises(RuntimeError, match="query %d failed" % k):
            pool.wait()
        pool.fail(k + 3, RuntimeError("a later failure"))           # does not replace the first
        with pytest.raises(RuntimeError, match="query %d failed" % k):
            pool.wait()
    finally:
        pool.close()
    assert written == list(range(k))
    assert set(range(k + 1)) <= set(ran)
    assert not any(t.is_alive() for t in pool.threads) and threading.active_count() == before
    assert not w.held


def test_a_failure_of_the_coordinator_stops_the_jobs_not_yet_started():
    ran = []
    gate = threading.Event()

    def work(wk, rnd, q):
        assert gate.wait(WAIT)
        ran.append(q)

    pool = bs.WorkerPool(1, work)
    try:
        pool.submit(bs.Round(range(6)))
        pool.fail(2, ValueError("stop"))
        gate.set()
        with pytest.raises(ValueError):
            pool.wait()
    finally:
        gate.set()
        pool.close()
    assert ran == [0, 1] and pool.cancelled(3) and not pool.cancelled(2) and not pool.cancelled(1)


@pytest.mark.parametrize("option", [["--workers", "2"], ["--workers", "1"], []])
@pytest.mark.parametrize("exc,text", [(bs.CtMismatch(bs.CT_MISMATCH % (1, "q.bhmm", 4, 1)), "codon translation tabel ID 1 does not match")])
def test_run_reports_a_workers_failure_once_with_status_1(exc, text, option, tmp_path, capsys, monkeypatch):
    """With --workers 2, --workers 1 and without the option: one search, whose failure after the first query is reported once."""
    during = []

    def search(opts, hmmfile, seqfile, nq, write, *a):
        during.append(os.environ.get("BATH_HIP_HOST_THREADS"))
        write(0, ("Query:       first\n//\n", ""))
        raise exc

    monkeypatch.setattr(bs, "_workers_search", search)
    monkeypatch.delenv("BATH_HIP_HOST_THREADS", raising=False)
    out = tmp_path / "o.txt"
    assert bs.run(option + ["-o", str(out), HMM, FA]) == 1
    err = capsys.readouterr().err
    assert err.count("Error:") == 1 and text in err
    got = out.read_text()
    assert "Query:       first" in got and "[ok]" not in got
    assert "BATH_HIP_HOST_THREADS" not in os.environ           # the workers' share does not outlive the search
    assert len(during) == 1 and (during[0] is None) == (option != ["--workers", "2"])      # ... and one worker is given none


def test_host_threads_split_among_worker_contexts(monkeypatch):
    def boom():
        raise AssertionError("os.cpu_count() was read")
    monkeypatch.setattr(os, "cpu_count", boom)
    aff = set(range(40))
    assert bs.host_threads_per_worker(4, environ={}, affinity=aff) == 10
    assert bs.host_threads_per_worker(3, environ={}, affinity=aff) == 13
    assert bs.host_threads_per_worker(4, ranks=2, environ={}, affinity=aff) == 5
    assert bs.host_threads_per_worker(4, environ={"OMP_NUM_THREADS": "16"}, affinity=aff) == 4
    assert bs.host_threads_per_worker(8, environ={"OMP_NUM_THREADS": "4"}, affinity=aff) == 1             # at least one each
    assert bs.host_threads_per_worker(8, ranks=16, environ={}, affinity=aff) == 1
    assert bs.host_threads_per_worker(4, environ={"BATH_HIP_HOST_THREADS": "7"}, affinity=aff) is None    # the user's value stays
    assert bs.host_threads_per_worker(1, environ={}, affinity=aff) == bs.host_threads_per_rank(1, environ={}, affinity=aff) == 40
    assert bs.host_threads_per_worker(2, environ={}) == max(1, len(os.sched_getaffinity(0)) // 2)


def test_ranks_get_the_share_of_all_their_workers(monkeypatch):
    """launch_ranks hands every rank BATH_HIP_HOST_THREADS = budget / (ranks x workers)."""
    seen = {}

    class Stop(Exception):
        pass

    def fake_env(n, rank, port, environ=None, threads=None):
        seen["threads"] = threads
        raise Stop()

    monkeypatch.setattr(bs, "rank_env", fake_env)
    monkeypatch.delenv("BATH_HIP_HOST_THREADS", raising=False)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(48)))
    with pytest.raises(Stop):
        bs.launch_ranks(2, ["--gpus", "2", "--workers", "3", HMM, FA], None, {})
    assert seen["threads"] == 8
    with pytest.raises(Stop):
        bs.launch_ranks(2, ["--gpus", "2", HMM, FA], None, {})
    assert seen["threads"] == 24


@pytest.mark.parametrize("workers", [1, 3])
def test_the_coordinator_prepares_one_batch_ahead_and_no_more(workers):
    """Sixty queries in batches of 2N; query 0 is held back.  While it is, the coordinator prepares the batch the workers are on
    and the next one and then waits, however many queries follow; released, it prepares the rest, each batch only after every
    query before the previous batch is written."""
    size, nq = 2 * workers, 60
    prepared, written = [], []
    release0, second = threading.Event(), threading.Event()
    w = bs.OrderedWriter(lambda q, text: written.append(q), bound=size)

    def work(wk, rnd, q):
        if q == 0:
            assert release0.wait(WAIT)
        w.put(q, "t")

    def prepare(b0, b1):
        assert len(written) >= b0 - size, (b0, written)         # every query before the previous batch is written
        prepared.append((b0, b1))
        pool.submit(bs.Round(range(b0, b1), admit=True))
        if len(prepared) == 2:
            second.set()

    pool = bs.WorkerPool(workers, work, w)
    feeder = threading.Thread(target=bs.feed_batches, args=(pool, nq, size, prepare))
    try:
        feeder.start()
        assert second.wait(WAIT)
        held = size - 1 if workers > 1 else 0       # the first batch's other queries are done and held (one worker: it is on query 0)
        with w.cv:                                  # ... and nothing moves any more
            assert w.cv.wait_for(lambda: len(w.held) == held and pool.pending == 2 * size - held, WAIT)
        assert prepared == [(0, size), (size, 2 * size)] and written == [] and feeder.is_alive()
        release0.set()
        feeder.join(WAIT)
        assert not feeder.is_alive()
    finally:
        release0.set()
        pool.close()
    assert prepared == [(b0, min(nq, b0 + size)) for b0 in range(0, nq, size)]
    assert written == list(range(nq)) and w.max_alive <= size


def test_after_a_failure_the_queries_before_it_still_get_their_later_rounds():
    """Streamed targets: a round per piece with a barrier behind it, the texts in a last round.  Query 3 fails in the first
    piece; queries 0-2 are searched in the second piece too and written, nothing from 3 on, and the failure is raised at the end."""
    ran, written = [], []
    lock = threading.Lock()
    w = bs.OrderedWriter(lambda q, text: written.append(q), bound=6)

    def work(wk, rnd, q):
        with lock:
            ran.append((rnd.payload, q))
        if rnd.payload == "piece 0" and q == 3:
            raise RuntimeError("query 3 failed")
        if rnd.payload == "render":
            w.put(q, "t")

    pool = bs.WorkerPool(2, work, w)
    try:
        for name in ("piece 0", "piece 1", "render"):
            pool.submit(bs.Round(range(6), name, admit=(name == "piece 0")))
            pool.barrier()                          # does not raise: the coordinator goes on to the next piece
        with pytest.raises(RuntimeError, match="query 3 failed"):
            pool.wait()
    finally:
        pool.close()
    assert written == [0, 1, 2]
    assert {(p, q) for p, q in ran if p != "piece 0"} == {(p, q) for p in ("piece 1", "render") for q in range(3)}


def test_close_after_the_coordinator_raised_searches_nothing_still_queued():
    ran, written = [], []
    gate = threading.Event()
    w = bs.OrderedWriter(lambda q, text: written.append(q), bound=4)

    started = threading.Event()

    def work(wk, rnd, q):
        started.set()
        assert gate.wait(WAIT)
        ran.append(q)
        w.put(q, "t")

    pool = bs.WorkerPool(1, work, w)
    pool.submit(bs.Round(range(4), admit=True))
    pool.submit(bs.Round(range(4, 8), admit=True))
    assert started.wait(WAIT)                       # query 0 is with the worker
    closer = threading.Thread(target=pool.close, args=(KeyboardInterrupt(),))
    closer.start()
    with w.cv:
        assert w.cv.wait_for(lambda: pool.closing, WAIT)
    gate.set()
    closer.join(WAIT)
    assert not closer.is_alive() and not any(t.is_alive() for t in pool.threads)
    assert ran == [0] and written == [0] and pool.failure[0] == 1


def test_every_worker_thread_runs_the_start_hook_first():
    seen = []
    lock = threading.Lock()

    def work(wk, rnd, q):
        with lock:
            assert ("start", wk, threading.get_ident()) in seen
            seen.append(("work", q))

    def start(wk):
        with lock:
            seen.append(("start", wk, threading.get_ident()))

    pool = bs.WorkerPool(3, work, start=start)
    try:
        pool.submit(bs.Round(range(9)))
        pool.wait()
    finally:
        pool.close()
    assert sorted(x[1] for x in seen if x[0] == "start") == [0, 1, 2] and sum(x[0] == "work" for x in seen) == 9
