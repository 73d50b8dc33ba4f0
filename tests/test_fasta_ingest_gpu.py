"""FASTA ingest on the device (bath_hip_fasta_*, bath_amd.FastaTargets) against the host readers: records, names, descriptions,
lengths and every code equal oracle_lib.read_fasta + bath_amd.digitize; the same at every chunk boundary; format errors name their
record and line and leave the context usable; windows equal dist.split_targets; the pipeline reads the device-built windows
exactly as it reads the same codes uploaded from the host."""
import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import dist

pytestmark = pytest.mark.gpu

SYMS = "ACGT-RYMKSWHBVDN*~" + "acgt-rymkswhbvdn*~" + "UuXx"


def write_fasta(rng, recs, crlf=False, blank_lines=False, ragged=False, width=60, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    out = bytearray()
    for header, seq in recs:
        out += b">" + header.encode() + nl
        i = 0
        while i < len(seq):
            w = int(rng.integers(1, 2 * width + 1)) if ragged else width
            out += seq[i:i + w].encode() + nl
            i += w
            if blank_lines and rng.random() < 0.1:
                out += (b"  \t" if rng.random() < 0.5 else b"") + nl
    if not final_newline and out.endswith(nl):
        out = out[:-len(nl)]
    return bytes(out)


def random_seq(rng, n, alphabet="ACGT"):
    a = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    return a[rng.integers(0, len(a), size=n)].tobytes().decode()


def parse(ctx, data, chunk=None):
    ft = ba.FastaTargets(ctx)
    chunk = chunk or max(1, len(data))
    for i in range(0, len(data), chunk):
        ft.feed(data[i:i + chunk])
    ft.finish()
    return ft


def check(ctx, tmp_path, data, chunk=None):
    p = tmp_path / "t.fa"
    p.write_bytes(data)
    want = ol.read_fasta(str(p))
    ft = parse(ctx, data, chunk)
    recs = ft.records()
    assert len(recs) == len(want)
    heads = ba.fasta_headers(str(p), recs)
    raw_heads = [ln[1:].strip() for ln in data.decode().replace("\r", "").split("\n") if ln.strip().startswith(">")]
    for r, (name, seq), (gname, gdesc), raw in zip(recs, want, heads, raw_heads):
        assert gname == name
        parts = raw.split(None, 1)
        assert gdesc == (parts[1].strip() if len(parts) > 1 else "")
        codes = ba.digitize(seq, ba.DNA_SYMS) if seq else np.zeros(0, np.uint8)
        assert int(r["length"]) == len(codes)
    allc = [ba.digitize(s, ba.DNA_SYMS) for _, s in want if s]
    flat = np.concatenate(allc) if allc else np.zeros(0, np.uint8)
    got = np.concatenate([ft.codes(i) for i in range(len(recs))]) if len(recs) else np.zeros(0, np.uint8)
    assert np.array_equal(got, flat)
    return ft


@pytest.mark.parametrize("case", ["widths", "ragged", "crlf_blank", "symbols", "empty_records", "gt_in_header", "no_final_newline"])
def test_parse_equals_host_reader(gpu_ctx, tmp_path, case):
    rng = np.random.default_rng(hash(case) % 1000)
    if case == "widths":
        for width in (1, 2, 59, 60, 61, 128, 200):
            recs = [("s%d desc %d" % (i, i), random_seq(rng, int(rng.integers(0, 700)))) for i in range(5)]
            check(gpu_ctx, tmp_path, write_fasta(rng, recs, width=width))
        return
    if case == "ragged":
        recs = [("r%d" % i, random_seq(rng, int(rng.integers(1, 3000)))) for i in range(12)]
        data = write_fasta(rng, recs, ragged=True)
    elif case == "crlf_blank":
        recs = [("c%d some words here" % i, random_seq(rng, int(rng.integers(1, 2000)))) for i in range(8)]
        data = b"\n  \n\r\n" + write_fasta(rng, recs, crlf=True, blank_lines=True)
    elif case == "symbols":
        recs = [("x%d" % i, random_seq(rng, int(rng.integers(100, 900)), SYMS)) for i in range(6)]
        data = write_fasta(rng, recs, width=77)
    elif case == "empty_records":
        recs = [("e0", ""), ("e1", random_seq(rng, 100)), ("e2", ""), ("e3", "")]
        data = write_fasta(rng, recs)
        check(gpu_ctx, tmp_path, b">only a header\n")
        check(gpu_ctx, tmp_path, b">only a header, no newline")
        check(gpu_ctx, tmp_path, b"")
    elif case == "gt_in_header":
        recs = [("g%d a>b >c >" % i, random_seq(rng, 300)) for i in range(4)]
        data = write_fasta(rng, recs, width=50)
    else:
        recs = [("n%d" % i, random_seq(rng, 333)) for i in range(3)]
        data = write_fasta(rng, recs, width=60, final_newline=False)
    check(gpu_ctx, tmp_path, data)


def test_long_record(gpu_ctx, tmp_path):
    rng = np.random.default_rng(5)
    recs = [("short", random_seq(rng, 1000)), ("chr1 a long one", random_seq(rng, 3_000_000)), ("tail", random_seq(rng, 10))]
    check(gpu_ctx, tmp_path, write_fasta(rng, recs, width=60))
    check(gpu_ctx, tmp_path, write_fasta(rng, recs, width=60), chunk=1 << 20)


def test_chunk_boundaries(gpu_ctx, tmp_path):
    rng = np.random.default_rng(11)
    recs = [("a desc", random_seq(rng, 70, SYMS)), ("b", ""), ("c x>y", random_seq(rng, 130))]
    data = b"\r\n" + write_fasta(rng, recs, crlf=True, width=17)
    for chunk in (1, 2, 3, 5, 7, 16, 31):                     # with 1: a boundary after every byte
        check(gpu_ctx, tmp_path, data, chunk=chunk)
    # tile edges (4096 bytes): a long multi-record file cut at and around multiples of the tile
    big = write_fasta(rng, [("t%d" % i, random_seq(rng, int(rng.integers(1, 9000)))) for i in range(40)], ragged=True, crlf=True)
    for chunk in (4095, 4096, 4097, 8192 + 13, 65536):
        check(gpu_ctx, tmp_path, big, chunk=chunk)


@pytest.mark.parametrize("chunk", [None, 3, 4096])
def test_format_errors_name_record_and_line(gpu_ctx, tmp_path, chunk):
    good = b">a\nACGT\nACGT\n>b desc\nAC\n"
    with pytest.raises(ba.FastaFormatError) as e:
        parse(gpu_ctx, good + b"ACGJT\n", chunk)
    assert (e.value.record, e.value.line, e.value.byte) == (1, 6, ord("J"))
    with pytest.raises(ba.FastaFormatError) as e:
        parse(gpu_ctx, b"\n\nACGT\n>a\nAC\n", chunk)
    assert (e.value.record, e.value.line) == (-1, 3)
    with pytest.raises(ba.FastaFormatError) as e:
        parse(gpu_ctx, b">a\nAC>GT\n", chunk)
    assert (e.value.record, e.value.line, e.value.byte) == (0, 2, ord(">"))
    # the context runs a clean search afterwards
    rng = np.random.default_rng(1)
    ft = check(gpu_ctx, tmp_path, write_fasta(rng, [("ok", random_seq(rng, 5000))]))
    hmm = ba.HMM(ol.GOLDEN + "/PTH2.bhmm")
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    stats, dm, _ = ba.Pipeline(gpu_ctx, om).run_hits(ft.seqs(ft.windows(hmm.max_length, dist.BLOCK_LENGTH)))
    assert stats.nres == 2 * 5000


def test_windows_equal_split_targets(gpu_ctx, tmp_path):
    rng = np.random.default_rng(3)
    lens = [0, 5, 14, 15, 1000, 60000, 250000, 123457]
    data = write_fasta(rng, [("w%d" % i, random_seq(rng, n)) for i, n in enumerate(lens)])
    ft = check(gpu_ctx, tmp_path, data)
    for max_length, block_length in [(100, 50000), (470, 50000), (250, 100000), (1000, dist.BLOCK_LENGTH)]:
        w = ft.windows(max_length, block_length)
        want = dist.split_targets(lens, max_length, block_length)
        assert [tuple(int(x) for x in r) for r in w] == want
        assert [tuple(int(x) for x in r) for r in ft.windows(max_length, block_length, 4, 7)] == [x for x in want if 4 <= x[0] < 7]
        # the block holds exactly those codes, contexts set
        blk = ft.seqs(w)
        assert blk.n == len(w) and list(blk.lengths) == [r[2] for r in want]


def test_pipeline_on_device_windows_equals_host_block(gpu_ctx, tmp_path):
    from bath_amd import synth
    hmm = ba.HMM(ol.GOLDEN + "/PTH2.bhmm")
    rng = np.random.default_rng(9)
    g, _ = synth.genome(400_000, seed=77, hmms=[hmm], genes_per_model=6)
    lens = [250_000, 1200, 90_000, 58_800]
    seqs, p = [], 0
    for n in lens:
        seqs.append(g[p:p + n]); p += n
    text = [("t%d" % i, "".join("ACGT"[c] for c in s)) for i, s in enumerate(seqs)]
    data = write_fasta(rng, text, width=60)
    ft = parse(gpu_ctx, data, chunk=100_000)
    wins = ft.windows(hmm.max_length, 50_000)
    want = dist.split_targets(lens, hmm.max_length, 50_000)
    host = ba.SeqBlock(gpu_ctx, [seqs[t][s:s + n] for t, s, n, c in want])
    host.set_context([c for _, _, _, c in want])
    dev = ft.seqs(wins)
    om = ba.OProfile(gpu_ctx, ba.Profile(hmm))
    for fs in (False, True):
        res = []
        for blk in (host, dev):
            pipe = ba.Pipeline(gpu_ctx, om, fs_pipe=fs)
            if fs:
                om3 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 3)); om5 = ba.FSOProfile(gpu_ctx, ba.FSProfile(hmm, 5))
                stats, _, dm, _ = pipe.run_frameshift_domains(om3, om5, blk)
            else:
                stats, dm, _ = pipe.run_hits(blk)
            res.append(([getattr(stats, f) for f, _ in ba.PipelineStats._fields_], [bytes(d) for d in dm], [d.cigar for d in dm]))
        assert res[0] == res[1]
        assert len(res[0][1]) >= 3
