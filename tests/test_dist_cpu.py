"""CPU tier: the N>1 path (one process per GPU, model broadcast, sharded targets, counters reduced and hits
gathered on rank 0) exercised with two gloo processes.  No GPU compute: each rank fabricates the records
a shard would produce, so the collectives, shard arithmetic and record packing are what is under test."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import bath_amd as ba
    from bath_amd import dist as bd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blob = open(os.path.join(ROOT, "tests", "golden", "PTH2.bhmm"), "rb").read() if rank == 0 else b""
    blob = bd.broadcast_bytes(blob, 0)
    n_total = 11
    lo, hi = bd.shard_range(n_total, rank, world)
    stats = ba.PipelineStats()
    stats.nres = 2000 * (hi - lo)
    stats.n_past_msv = hi - lo
    res = np.zeros(hi - lo, dtype=ba.ORF_RESULT_DTYPE)
    res["window"] = np.arange(hi - lo)
    res["usc"] = 10.0 * rank + np.arange(hi - lo)
    merged = bd.reduce_stats(stats)
    hits = bd.gather_results(res, lo, 0)
    doms = []
    for w in range(hi - lo):                                    # one hit per local sequence, CIGAR of rank-dependent length
        d = ba.FsDomain()
        d.window, d.iali, d.jali, d.ihmm, d.jhmm, d.bitscore, d.lnP, d.reported = w, 10 + w, 300 + w, 1, 100, 50.0 + lo + w, -30.0 - (lo + w), 1
        d.cigar = "%dM" % (3 * (lo + w + 1)) * (rank + 1)
        doms.append(d)
    gd = bd.gather_domains(doms, lo, 0)
    table = None
    if gd is not None:                                          # rank 0 finishes the search: hit list + table
        th = ba.TopHits()
        th.add(gd, ["s%d" % i for i in range(n_total)], [5000] * n_total)
        th.finalize(merged["nres"], 100)
        table = [l.split() for l in th.tblout("q", "", 100, show_cigar=True, show_header=False).split("\n") if l]
    t = bd.max_over_ranks(1.0 + rank)
    q.put((rank, len(blob), (lo, hi), merged["nres"], merged["n_past_msv"], None if hits is None else hits["window"].tolist(), t,
           None if gd is None else [(d.window, d.cigar) for d in gd], table))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_and_reduce():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "PTH2.bhmm"))
    assert [o[1] for o in outs] == [size, size]                     # the model reached every rank
    assert [o[2] for o in outs] == [(0, 6), (6, 11)]                # contiguous shards cover all targets once
    assert all(o[3] == 2000 * 11 and o[4] == 11 for o in outs)      # p7_pipeline_Merge
    assert outs[0][5] == list(range(11)) and outs[1][5] is None     # p7_tophits_Merge on rank 0, global window ids
    assert all(o[6] == 2.0 for o in outs)                           # max-over-ranks timing
    # the hits themselves: records and CIGAR strings of both ranks on rank 0, global sequence indices, then one table
    assert outs[1][7] is None and [w for w, _ in outs[0][7]] == list(range(11))
    assert all(c == "%dM" % (3 * (w + 1)) * (1 if w < 6 else 2) for w, c in outs[0][7])
    table = outs[0][8]
    assert [r[1] for r in table] == ["s%d" % i for i in range(10, -1, -1)]          # best E-value (last sequence) first
    assert table[0][-1] == "33M33M" and table[-1][-1] == "3M"


def test_shard_range_partitions():
    from bath_amd.dist import shard_range
    for n in (0, 1, 7, 8, 1000003):
        for world in (1, 2, 4, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            assert max(b - a for a, b in spans) - min(b - a for a, b in spans) <= 1


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_launcher_starts_the_ranks(scaling):
    """`python bench.py --gpus 2` outside torch.distributed.run starts two ranks itself (a fresh child process) and relays rank
    0's JSON line; --plumbing-only runs the launcher, the model broadcast, the counter reduction and the gather to rank 0
    over gloo with fabricated counters (the kernels need the GPU)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plumbing-only", "--full", "--windows", "1001", "--fs-windows", "1001", "--scaling", scaling,
                        "--c4-total-mb", "3", "--c5-total-mb", "3"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                           # one JSON line, from rank 0
    # stdout ends with the compact line the driver records (its tail holds 2000 characters): the contract's keys and every leg's numbers
    line = json.loads(lines[0])
    assert len(lines[0]) < 2000 and p.stdout.rstrip().endswith(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "fs", "c4", "c5"):
        assert key in line, key
    assert line["n_gpus"] == 2 and line["scaling"] == scaling and line["plumbing_only"] is True and line["fs"]["n_gpus"] == 2 and line["c4"]["n_gpus"] == 2
    # ... and the full record goes to stderr
    full = [l for l in p.stderr.splitlines() if l.startswith("{") and '"residues_per_step"' in l]
    assert len(full) == 1
    out = json.loads(full[0])
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["plumbing_only"] is True
    total = 1001 if scaling == "strong" else 2002                    # strong: one block sharded; weak: a block per rank
    assert out["residues_per_step"] == 2 * 1000 * total              # counters reduced over both ranks
    assert out["survivors"]["n_past_msv"] == total
    # the --fs leg stays under --gpus N: one block sharded over the ranks, counters reduced, domains gathered on rank 0
    fs = out["fs"]
    assert fs["n_gpus"] == 2 and fs["scaling"] == "strong" and fs["domains_gathered"] == 6 and fs["windows_of_gathered_domains_are_global"]
    # configs[3] under --gpus N: the 12-model database broadcast once, (query, window group) pairs dealt to the ranks, hits gathered
    # per query on rank 0 and every query finished there; configs[4]: window shards, domains gathered
    c4 = out["c4"]
    # 13 items: the 459-node model's windows are cut in two (dist.query_items_weighted); one fabricated hit per item
    assert c4["n_gpus"] == 2 and c4["items"] == 13 and sorted(c4["items_per_rank"]) == [6, 7] and len(c4["rank_busy_ms"]) == 2
    assert c4["hits_per_query"] == [1, 1, 1, 2] + [1] * 8 and c4["hits"] == 13
    c5 = out["c5"]
    assert c5["n_gpus"] == 2 and c5["domains_gathered"] == 4 and c5["windows_of_gathered_domains_are_global"]


def test_bench_plain_run_is_the_headline_alone():
    """Without --full a run does only what the headline needs: the same contract keys and counters as under --full, and none of the
    other legs (fs, c4, c5), the records copy-out or its gather to rank 0."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plumbing-only", "--windows", "1001", "--fs-windows", "1001",
                        "--c4-total-mb", "3", "--c5-total-mb", "3"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and p.stdout.rstrip().endswith(lines[0])
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in line, key
    assert line["n_gpus"] == 2 and line["plumbing_only"] is True
    full = [l for l in p.stderr.splitlines() if l.startswith("{") and '"residues_per_step"' in l]
    assert len(full) == 1
    out = json.loads(full[0])
    assert out["residues_per_step"] == 2 * 1000 * 2002 and out["survivors"]["n_past_msv"] == 2002
    for key in ("fs", "c4", "c5", "cpu_baseline", "hits_gathered", "ms_per_step_with_records", "strong_scaling_check"):
        assert key not in out and key not in line, key


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the counters and the records the cascade leg gathered, one finite float32 / float64 .npy per array; --steps is
    the number of timed steps the line reports (the arrays themselves are the GPU tier's test_bench_dump_gpu.py)."""
    import json
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--plumbing-only", "--windows", "1001", "--no-fs", "--no-c45",
                        "--steps", "3", "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and "ms_per_step" in line
    d = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in d.values())
    assert d["counter_nres"][0] == 2 * 1001 * 1000 and d["counter_n_past_msv"][0] == 1001
    assert list(d["record_window"]) == list(range(64)) and d["record_stride"][0] == 1 and d["record_usc"].dtype == np.float32


def _query_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import bath_amd as ba
    from bath_amd import dist as bd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nwin = [5, 3, 8]                                            # three queries, their windows
    items = bd.query_items(nwin, world, items_per_rank=3)       # G = 2 groups per query
    owner = bd.deal([(hi - lo) * (q + 1.0) for q, lo, hi in items], world)
    by_q, st_q = {}, {}
    for (qq, lo, hi), o in zip(items, owner):
        if o != rank:
            continue
        for w in range(lo, hi):                                 # one hit per window, tagged with its query and global window
            d = ba.FsDomain()
            d.window, d.iali, d.jali, d.reported = w, 100 * qq + w, 100 * qq + w + 50, 1
            d.cigar = "%dM" % (10 * qq + w + 1)
            by_q.setdefault(qq, []).append(d)
        acc = st_q.setdefault(qq, dict.fromkeys(bd.STAT_FIELDS, 0))
        acc["nres"] += 1000 * (hi - lo); acc["n_orfs"] += hi - lo
    got = bd.gather_query_domains(by_q, 0)
    # the same exchange on record arrays + CIGAR pools (no Python object per hit): what bench.py's configs[3] leg ships
    arr = bd.gather_query_hits({k: ba.HitArray.from_domains(v) for k, v in by_q.items()}, 0)
    arr_view = None
    if arr is not None:
        arr_view = {}
        for k, h in arr.items():
            cig = [h.pool[int(o):h.pool.index(b"\0", int(o))].decode() for o in h.rec["cigar_off"]]
            arr_view[k] = sorted(zip([int(x) for x in h.rec["window"]], [int(x) for x in h.rec["iali"]], cig))
    merged = bd.reduce_query_stats(st_q, len(nwin))
    busy = bd.gather_floats(1.0 + rank, 0)
    q.put((rank, items, owner, None if got is None else {k: sorted((d.window, d.iali, d.cigar) for d in v) for k, v in got.items()},
           [(m["nres"], m["n_orfs"]) for m in merged], busy, arr_view))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_query_deal_and_gather():
    """configs[3]'s exchange: (query, window group) items dealt identically on every rank, each rank's hits tagged by query arrive
    on rank 0 in one gather, the per-query counters in one all-reduce."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_query_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nwin = [5, 3, 8]
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]                   # the same deal on both ranks
    items, owner = outs[0][1], outs[0][2]
    assert len(items) == 6 and set(owner) == {0, 1}
    for qq, n in enumerate(nwin):                                                   # every query's windows covered exactly once
        spans = sorted((lo, hi) for q_, lo, hi in items if q_ == qq)
        assert spans[0][0] == 0 and spans[-1][1] == n and all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    got = outs[0][3]
    assert outs[1][3] is None
    for qq, n in enumerate(nwin):
        assert got[qq] == [(w, 100 * qq + w, "%dM" % (10 * qq + w + 1)) for w in range(n)]
    assert outs[0][4] == outs[1][4] == [(1000 * n, n) for n in nwin]               # p7_pipeline_Merge per query
    assert outs[0][5] == [1.0, 2.0] and outs[1][5] is None
    assert outs[1][6] is None and outs[0][6] == got                                   # the array path delivers the same hits and CIGAR strings


def test_deal_is_balanced_and_deterministic():
    from bath_amd.dist import deal, query_items
    costs = [459, 247, 238, 192, 185, 136, 131, 121, 100, 90, 78, 56]
    for world in (1, 2, 4, 8):
        owner = deal(costs, world)
        assert owner == deal(list(costs), world)
        load = [sum(c for c, o in zip(costs, owner) if o == r) for r in range(world)]
        assert max(load) <= sum(costs) / world + max(costs)                         # LPT bound
        items = query_items([382] * 12, world)
        assert len(items) >= min(2 * world, 12) and all(hi > lo for _, lo, hi in items)


def test_weighted_items_cut_the_heavy_queries_and_cover_every_window():
    from bath_amd.dist import query_items_weighted
    M = [78, 152, 116, 459, 238, 131, 121, 185, 192, 247, 136, 56]
    nwin = [382] * 12
    costs = [n * (m + 150.0) for n, m in zip(nwin, M)]
    for world in (1, 2, 4, 8):
        items = query_items_weighted(nwin, costs, world)
        assert items == query_items_weighted(list(nwin), list(costs), world)          # every rank computes the same list
        for q in range(12):                                                           # a query's groups tile its windows, in order
            mine = [(lo, hi) for qq, lo, hi in items if qq == q]
            assert mine[0][0] == 0 and mine[-1][1] == nwin[q] and all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
        groups = [sum(1 for qq, _, _ in items if qq == q) for q in range(12)]
        assert groups[3] == max(groups) and groups[3] >= 2 and groups[11] == 1        # the 459-node model is cut, the 56-node one never
        assert len(items) <= max(12, 3 * world) + 6
    assert query_items_weighted([1, 1], [5.0, 1.0], 8) == [(0, 0, 1), (1, 0, 1)]      # never more groups than windows


def _fabricated_hits(ba, items, owner, rank=None):
    """{query: [FsDomain]} of the items <rank> owns (all items when rank is None): one hit per window, a duplicate pair at every
    group boundary (the overlap of two windows finds a hit twice: p7_tophits_RemoveDuplicates must drop one copy whoever found it)."""
    by_q = {}
    for (qq, lo, hi), o in zip(items, owner):
        if rank is not None and o != rank:
            continue
        for w in range(lo, hi):
            d = ba.FsDomain()
            d.window, d.reported = 0, 1
            d.iali = d.ienv = 1000 * w + 17 * qq + 1
            d.jali = d.jenv = d.iali + 299
            d.ihmm, d.jhmm = 1, 100
            d.lnP, d.bitscore = -30.0 - 0.25 * w - qq, 40.0 + 0.5 * w + qq
            d.cigar = "%dM" % (100 + w)
            by_q.setdefault(qq, []).append(d)
        if lo > 0:                                              # the copy of the previous group's last hit
            d = ba.FsDomain()
            w = lo - 1
            d.window, d.reported = 0, 1
            d.iali = d.ienv = 1000 * w + 17 * qq + 1
            d.jali = d.jenv = d.iali + 299
            d.ihmm, d.jhmm = 1, 100
            d.lnP, d.bitscore = -30.0 - 0.25 * w - qq, 40.0 + 0.5 * w + qq
            d.cigar = "%dM" % (100 + w)
            by_q.setdefault(qq, []).append(d)
    return by_q


def _finish(ba, hits, nres):
    th = ba.TopHits()
    th.add_arrays(hits if hits is not None else ba.HitArray(np.zeros(0, dtype=ba.FS_DOMAIN_DTYPE), b""), ["genome"], [10 ** 6])
    th.finalize(int(nres), 300)
    return th.reported(), th.tblout("q", "", 100, show_cigar=True, show_header=False)


def _owner_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import bath_amd as ba
    from bath_amd import dist as bd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nwin = [7, 2, 9, 4, 5]
    items = bd.query_items(nwin, world, items_per_rank=3)
    owner = bd.deal([(hi - lo) * (qq + 1.0) for qq, lo, hi in items], world)
    mine = {k: ba.HitArray.from_domains(v) for k, v in _fabricated_hits(ba, items, owner, rank).items()}
    st_q = {}
    for (qq, lo, hi), o in zip(items, owner):
        if o == rank:
            st_q.setdefault(qq, dict.fromkeys(bd.STAT_FIELDS, 0))["nres"] += 2000 * (hi - lo)
    owned = bd.exchange_query_hits(mine)                        # a query's hits on its owner (q mod N) ...
    merged = bd.reduce_query_stats(st_q, len(nwin))
    my_q = [qq for qq in range(len(nwin)) if bd.query_owner(qq, world) == rank]
    assert sorted(owned) == [qq for qq in my_q if qq in owned] and all(qq in my_q for qq in owned)
    done = {qq: _finish(ba, owned.get(qq), merged[qq]["nres"]) for qq in my_q}          # ... finished there ...
    tables = bd.gather_query_tables(done, 0)                    # ... and only the tables travel to rank 0
    # exchange_bytes on its own: every rank sends rank-dependent payloads to every other rank (and nothing to itself)
    got = bd.exchange_bytes({d: bytes([rank]) * (3 * d + rank + 1) for d in range(world) if d != rank})
    q.put((rank, items, owner, tables, {s: (len(b), set(b)) for s, b in got.items()}, [m["nres"] for m in merged]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_queries_finished_on_their_owner_give_the_single_process_tables(world):
    """configs[3]'s end of a job with the serial tail spread: per query the hits of all ranks meet on the owner rank (q mod N), the
    owner finishes the query (bath_tophits_finalize: E-values, duplicates of window overlaps, order, thresholds) and ships the
    table; rank 0's tables must be those of ONE process finishing every query from all hits (bathsearch.c:868-921)."""
    import bath_amd as ba
    from bath_amd import dist as bd
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_owner_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    items, owner = outs[0][1], outs[0][2]
    assert all(o[1] == items and o[2] == owner for o in outs)
    assert all(o[3] is None for o in outs[1:])
    tables = outs[0][3]
    nwin = [7, 2, 9, 4, 5]
    nres = [2000 * n for n in nwin]
    assert outs[0][5] == nres
    everything = _fabricated_hits(ba, items, owner)
    for qq in range(len(nwin)):
        want = _finish(ba, ba.HitArray.from_domains(everything[qq]), nres[qq])
        assert tables[qq] == want, qq
        assert want[0] == nwin[qq]                              # the duplicates at the group boundaries are gone, whoever found them
    for o in outs:                                              # the raw exchange: from every other rank, the right length and content
        rank = o[0]
        assert o[4] == {s_: (3 * rank + s_ + 1, {s_}) for s_ in range(world) if s_ != rank}


def test_item_cost_orders_the_database_as_measured():
    """dist.item_cost (the longest-first deal's estimate) against the item times measured alone on an MI355X for the 100 Mb x 12-model
    job (profiles/r05_c4_items.txt: model length, share of the genome, milliseconds): every pair of items whose measured times differ
    by more than 15 % is ordered the same way by the estimate, the estimate is within 15 % of every measured time but one, and the
    deal it leads to is balanced."""
    from bath_amd.dist import item_cost, deal
    measured = [(78, 1.0, 3.80), (152, 1.0, 4.02), (116, 1.0, 3.16), (459, 0.5, 7.69), (459, 0.5, 7.52), (238, 1.0, 5.58), (131, 1.0, 3.70),
                (121, 1.0, 3.29), (185, 1.0, 4.10), (192, 1.0, 4.32), (247, 1.0, 4.93), (136, 1.0, 3.53), (56, 1.0, 2.75)]
    n_nt = 100_000_000
    est = [item_cost(m, int(share * n_nt)) for m, share, _ in measured]
    for a in range(len(measured)):
        for b in range(len(measured)):
            if 0 not in (a, b) and measured[a][2] > 1.15 * measured[b][2]:      # (item 0 is the measurement's outlier, below)
                assert est[a] > est[b], (measured[a], measured[b], est[a], est[b])
    off = [abs(e - t) / t for e, (_, _, t) in zip(est, measured)]
    assert sorted(off)[-2] < 0.15, off                          # (the 78-node model's 3.80 ms is the outlier of the measurement)
    assert est.index(max(est)) in (3, 4)                        # the halves of the 459-node model lead the longest-first deal
    for world in (2, 4, 8):
        own = deal(est, world)
        assert own == deal(list(est), world)
        load = [sum(c for c, o in zip(est, own) if o == r) for r in range(world)]
        assert max(load) <= sum(est) / world + max(est) and max(load) - min(load) <= max(est)
