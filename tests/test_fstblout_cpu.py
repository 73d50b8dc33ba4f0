"""bathsearch --fstblout without a GPU: the rows of p7_tophits_TabularFrameshifts (bath_trace_frameshift_rows), the table text
(bath_tophits_tabular_frameshifts), their Python wrappers and the driver's option handling.

The recorded --fs hit of AMP_N (tests/golden/AMP_N-fs.out, AMP_N-fs.tbl) is rendered from the ORACLE's trace; the row rules are
restated here (expected_rows) and applied to hand-made traces on both strands; the table's widths, header and reporting rules are
checked on made-up hits against a rendering written here with Python's % operator from the reference's formats."""
import os

import numpy as np
import pytest

import bath_amd as ba
import oracle_lib as ol
from bath_amd import bathsearch as bs
from test_tophits_cpu import from_oracle, mk

HEAD1 = "#%-*s %-*s %-*s %-*s %-9s %-*s %-*s  %5s %6s %-*s %9s\n"                    # p7_tophits.c:1467
HEAD2 = "#%*s %*s %*s %*s %9s %-*s %-*s  %5s  %6s  %-*s  %9s\n"                       # :1470
ROW = " %-*s %-*s %-*s %-*s %9.2g %-*d %-*d  %5c  %6d  %-*d  %9d\n"                   # :1562

# the recorded alignment's quasi-codons (AMP_N-fs.out): TCaA at 43, AG- at 83, C-- at 232, G-A at 251 and 295, --G at 336;
# the TGA at 300 is in an insert column and gets no row
RECORDED_ROWS = [("I", 1, 43, 43), ("D", 1, 83, 83), ("D", 2, 232, 232), ("D", 1, 251, 251), ("D", 1, 295, 295), ("D", 2, 336, 336)]


def want_table(hits, qname, qacc, tnamew, taccw, posw, header=True):
    """hits: [(target name, target accession or None, E-value, iali, jali, rows)] of the reported hits in order."""
    qnamew, qaccw = max(20, len(qname)), max(10, len(qacc or ""))
    s = ""
    if header:
        s += HEAD1 % (tnamew - 1, " target name", taccw, " accession", qnamew, " query name", qaccw, " accession", " E-value", posw, " ali from", posw,
                      " ali to", " I D S", " length", posw, " seq start", " ali start")
        s += HEAD2 % (tnamew - 1, "-------------------", taccw, "-----------", qnamew, "--------------------", qaccw, "----------", "---------", posw,
                      "---------", posw, "---------", "-----", "------", posw, "---------", "---------")
    for name, acc, E, iali, jali, rows in hits:
        for typ, length, seq_start, ali_start in rows:
            s += ROW % (tnamew, name, taccw, acc or "-", qnamew, qname, qaccw, qacc or "-", E, posw, iali, posw, jali, typ, length, posw, seq_start, ali_start)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# 1. options
# ---------------------------------------------------------------------------------------------------------------------------

FILES = [os.path.join(ol.GOLDEN, "AMP_N.bhmm"), os.path.join(ol.GOLDEN, "target-AMP_N.fa")]


def test_options_are_accepted():
    opts, h, s = bs.parse_args(["--fs", "--fstblout", "x", "--notrans"] + FILES)
    assert opts["--fstblout"] == "x" and opts["--notrans"] is True and opts["--fs"] is True and [h, s] == FILES
    assert "--fstblout" not in bs.REFUSED and "--notrans" not in bs.REFUSED


def test_fstblout_needs_fs(capsys, tmp_path):
    f = tmp_path / "x"
    assert bs.run(["--fstblout", str(f)] + FILES) == 1
    assert "--fstblout" in capsys.readouterr().err
    assert not f.exists()                                    # refused before any file is opened


def recorded_header():
    text = open(os.path.join(ol.GOLDEN, "AMP_N-fs.out")).read()
    return text[:text.index("Query:")]


def test_header_lines_at_the_reference_positions():
    lines = recorded_header().split("\n")
    at = lines.index("# per-seq hits tabular output:                   AMP_N-fs.tbl")
    assert lines[at + 1] == "# Use the frameshift aware algorithms"
    new = ["# frameshift tabular output:                     AMP_N-fs.fstbl", "# show translated DNA sequence:                  no"]
    want = "\n".join(lines[:at + 1] + new + lines[at + 1:])
    argv = ["--fs", "-o", "AMP_N-fs.out", "--tblout", "AMP_N-fs.tbl", "--cigar", "--fstblout", "AMP_N-fs.fstbl", "--notrans", "AMP_N.bhmm", "target-AMP_N.fa"]
    opts, h, s = bs.parse_args(argv)
    assert bs.output_header(opts, h, s) == want
    # ... with a --textw line between them, as bathsearch.c:276-283 orders them
    opts, h, s = bs.parse_args(["--textw", "130"] + argv)
    want = "\n".join(lines[:at + 1] + new[:1] + ["# max ASCII text line length:                    130"] + new[1:] + lines[at + 1:])
    assert bs.output_header(opts, h, s) == want
    opts, h, s = bs.parse_args(["--notextw"] + argv)
    want = "\n".join(lines[:at + 1] + new[:1] + ["# max ASCII text line length:                    unlimited"] + new[1:] + lines[at + 1:])
    assert bs.output_header(opts, h, s) == want


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the recorded hit, from the oracle's trace
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def amp_n():
    """The oracle's --fs hit of AMP_N.bhmm on target-AMP_N.fa: (hmm, 5-codon profile, oracle domain, trace, window codes, nres)."""
    model = ol.Model(FILES[0], 0)
    hmm = ba.HMM(FILES[0], 0)
    recs = ol.read_fasta(FILES[1])
    seqs = [ol.digitize_dna(s) for _, s in recs]
    ol.lib().bo_traces_reset()
    pli, _, _, odm, per_d, _ = model.run_pipeline_fsdom(seqs)
    (w, o), = [(w, o) for w, (a, b) in enumerate(per_d) for o in odm[a:b] if o.reported]
    t, *arrays = ol.trace_arrays(o.trace_idx)
    trace = (ba.DomainTrace(0, t.N, t.win_start, t.orf_start, t.frameshift),) + tuple(arrays)      # a copy: the oracle's store is reused
    return dict(hmm=hmm, gm5=ba.FSProfile(hmm, 5, ncbi_table=hmm.ct), o=o, trace=trace, window=seqs[w][trace[0].win_start - 1:].astype(np.uint8),
                nres=pli.nres, name=recs[w][0].split()[0], length=len(seqs[w]))


def recorded_tbl_row():
    return [ln for ln in open(os.path.join(ol.GOLDEN, "AMP_N-fs.tbl")) if ln[0] != "#"][0].split()


def recorded_table_text():
    """The --fstblout text of the recorded run, built from the recorded rows and the recorded --tblout row."""
    r = recorded_tbl_row()
    assert (r[1], r[2], r[3], r[4], r[9], r[10]) == ("seq1", "-", "AMP_N", "-", "1", "402")
    return want_table([("seq1", None, float(r[11]), 1, 402, RECORDED_ROWS)], "AMP_N", None, 20, 10, 9)


def test_recorded_hit_rows(amp_n):
    a = amp_n
    assert a["trace"][0].frameshift == 1 and (a["o"].iali, a["o"].jali) == (1, 402)
    rows = ba.frameshift_rows(a["trace"], a["window"], a["gm5"], a["o"].iali, a["o"].jali)
    assert rows == RECORDED_ROWS
    r = recorded_tbl_row()
    assert len(rows) == int(r[15]) == 6                      # the 'shifts' column
    assert int(r[16]) == 1 and not [x for x in rows if x[0] == "S"]          # 'stops' is 1: that stop is in an insert column


def test_recorded_hit_table_text(amp_n):
    a = amp_n
    th = ba.TopHits()
    th.add([from_oracle(a["o"], 0)], [a["name"]], [a["length"]])
    th.finalize(a["nres"], a["hmm"].max_length)
    rows = ba.frameshift_rows(a["trace"], a["window"], a["gm5"], a["o"].iali, a["o"].jali)
    assert th.fstblout(a["hmm"].name, a["hmm"].acc, [rows]) == recorded_table_text()
    with pytest.raises(ba.BathError):
        th.fstblout(a["hmm"].name, a["hmm"].acc, [])         # one row list per reported hit


# ---------------------------------------------------------------------------------------------------------------------------
# 3. hand-made traces
# ---------------------------------------------------------------------------------------------------------------------------

M, D, I = ba.T_M, ba.T_D, ba.T_I
STOPS = ("TAA", "TAG", "TGA")
# (state, codon): a match state on every codon length, a stop codon in a match state and in an insert state, delete states
COLUMNS = [(M, "GCT"), (M, "A"), (D, ""), (M, "CG"), (M, "TAA"), (I, "TAG"), (M, "ACGT"), (D, ""), (D, ""), (M, "ACGTA"), (I, "GGC"), (M, "TGA"),
           (M, "TAG"), (M, "GCA")]


def expected_rows(columns, iali, jali):
    """The table of the issue, restated: ali_pos starts at 1; a row carries ali_pos before the advance."""
    rows, ali_pos = [], 1
    for st, codon in columns:
        if st == M:
            kind = {1: ("D", 2), 2: ("D", 1), 4: ("I", 1), 5: ("I", 2)}.get(len(codon))
            if kind is None and codon in STOPS:
                kind = ("S", 0)
            if kind is not None:
                rows.append((kind[0], kind[1], iali + ali_pos - 1 if iali < jali else iali - ali_pos + 1, ali_pos))
            ali_pos += len(codon)
        elif st == I:
            ali_pos += 3
    return rows


def handmade_trace(columns, lead=7, frameshift=1):
    """(trace, window codes): the codons back to back behind <lead> nucleotides of the window; k advances on M and D."""
    st, k, i, c, nts = [], [], [], [], "ACGTACG"[:lead]
    node = 0
    for s, codon in columns:
        node += 0 if s == I else 1
        nts += codon
        st.append(s); k.append(node); i.append(len(nts)); c.append(len(codon) if s == M else 0)
    t = ba.DomainTrace(0, len(columns), 1, 0, frameshift)
    trace = (t, np.array(st, np.int8), np.array(k, np.int32), np.array(i, np.int32), np.array(c, np.int8), np.full(len(columns), 0.9, np.float32))
    return trace, ol.digitize_dna(nts + "ACGT").astype(np.uint8)


@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_handmade_trace_rows(amp_n, strand):
    trace, window = handmade_trace(COLUMNS)
    n = sum(len(codon) for _, codon in COLUMNS)
    iali, jali = (101, 100 + n) if strand == "plus" else (5000, 5001 - n)
    want = expected_rows(COLUMNS, iali, jali)
    assert [(r[0], r[1]) for r in want] == [("D", 2), ("D", 1), ("S", 0), ("I", 1), ("I", 2), ("S", 0), ("S", 0)]
    assert want[2][3] == 7 and want[3][3] == 13              # the insert state's TAG: no row, three positions
    assert ba.frameshift_rows(trace, window, amp_n["gm5"], iali, jali) == want


def test_standard_branch_trace_has_no_rows(amp_n):
    trace, window = handmade_trace([(s, "TAA" if s == M else codon) for s, codon in COLUMNS if len(codon) in (0, 3)], frameshift=0)
    assert ba.frameshift_rows(trace, window, amp_n["gm5"], 101, 400) == []
    trace, window = handmade_trace([(s, "TAA" if s == M else codon) for s, codon in COLUMNS if len(codon) in (0, 3)], frameshift=1)
    assert [r[0] for r in ba.frameshift_rows(trace, window, amp_n["gm5"], 101, 400)] == ["S"] * 5


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the table's rules, on made-up hits
# ---------------------------------------------------------------------------------------------------------------------------

LONG = "a_target_name_of_25_chars"


def made_up_list():
    doms = [mk(0, 100, 400, 1, 100, -40.0),                       # reported
            mk(1, 9000, 8700, 1, 100, -35.0),                     # reported, other strand, the 25-character name
            mk(2, 1234567890, 1234568190, 1, 100, -1.0),          # E-value above the threshold: not reported, a 10-digit coordinate
            mk(0, 7000, 7300, 1, 100, -45.0)]                     # not reported by the pipeline: never becomes a hit
    doms[-1].reported = 0
    th = ba.TopHits()
    th.add(doms, ["short", LONG, "far"], [10000, 10000, 2_000_000_000], accs=[None, "ACC12345678901", None])
    th.finalize(nres=3000 * 100, max_length=100)
    return th


def test_table_widths_header_and_reporting():
    assert len(LONG) == 25
    th = made_up_list()
    hits = th.hits()
    assert [fl & 1 for _, _, fl in hits] == [1, 1, 0]
    rows = [[("D", 1, 105, 6), ("S", 0, 130, 31)], [("I", 2, 8990, 11)]]
    E = [float(np.exp(d.lnP)) for d, _, _ in hits]
    want = want_table([("short", None, E[0], 100, 400, rows[0]), (LONG, "ACC12345678901", E[1], 9000, 8700, rows[1])], "query", "QACC000000012", 25, 14, 10)
    got = th.fstblout("query", "QACC000000012", rows)
    assert got == want
    lines = got.split("\n")
    assert len(lines) == 6 and lines[0][0] == lines[1][0] == "#" and "far" not in got           # the unreported hit: no rows, but its widths
    assert lines[2].startswith(" short" + " " * 21 + "-" + " " * 14 + "query") and " 100        400         " in lines[2]
    assert th.fstblout("query", "QACC000000012", rows, show_header=False) == "".join(ln + "\n" for ln in lines[2:5])
    # a hit without rows prints nothing; the header stays
    assert th.fstblout("query", None, [[], []]).count("\n") == 2


def test_empty_list_has_no_header():
    th = ba.TopHits()
    th.finalize(1000, 100)
    assert th.fstblout("query", "ACC1", [], show_header=True) == ""


def test_header_needs_a_hit_of_any_kind_not_a_reported_one():
    th = ba.TopHits()
    th.add([mk(0, 100, 400, 1, 100, -1.0)], ["t"], [1000])
    th.finalize(3000 * 100, 100)
    assert [fl & 1 for _, _, fl in th.hits()] == [0]
    assert th.fstblout("query", None, []) == want_table([], "query", None, 20, 10, 9)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the hit stream carries what the rows need
# ---------------------------------------------------------------------------------------------------------------------------

def test_rows_survive_the_hit_stream(amp_n):
    a = amp_n
    hand, window = handmade_trace(COLUMNS)
    n = sum(len(codon) for _, codon in COLUMNS)
    doms = [from_oracle(a["o"], 0), mk(0, 5000, 5001 - n, 1, 11, -30.0)]
    traces = [a["trace"], hand]
    windows = [a["window"], window]
    before = [ba.frameshift_rows(t, w, a["gm5"], d.iali, d.jali) for t, w, d in zip(traces, windows, doms)]
    assert before[0] == RECORDED_ROWS and len(before[1]) == 7
    stream = ba.HitArray.from_domains(doms).to_bytes(traces=traces)
    back = ba.HitArray.traces_from_bytes(stream)
    assert len(back) == 2
    after = [ba.frameshift_rows(t, w, a["gm5"], d.iali, d.jali) for (d, t), w in zip(back, windows)]
    assert after == before
