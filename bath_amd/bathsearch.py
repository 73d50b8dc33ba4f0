"""bathsearch on one GPU or several: search the profile HMMs of a model file against the DNA targets of a FASTA file.

    python -m bath_amd.bathsearch [--gpus N] [--workers N] [--arith strict|odds3|odds] [options] <hmmfile> <seqfile>

The FASTA file's bytes go to the device as they are (bath_amd.FastaTargets: records, digitising and the windows of
esl_sqio_ReadWindow are found there); per query the windows run through the pipeline in blocks of at most <block_nt>
nucleotides, and the hits are finished, sorted and printed as bathsearch.c does (main output, --tblout and --fstblout).

--fstblout <f> (needs --fs) writes the table of frameshift and stop-codon locations (p7_tophits_TabularFrameshifts): a row per
quasi-codon and per stop codon in a match state of every reported hit of the frameshift branch, from the same trace and the same
window codes its alignment block is rendered from (main_output_query); the file is opened, filled per query and closed with the
same tail as the --tblout file, in every run mode.  Its header lines come with the first query only, and only when that query's hit
list is not empty (the reference's rule).  --notrans adds its header line and changes nothing else: the reference sets
pli->show_translated_sequence and never reads it, so the translation line of the alignment blocks is printed regardless.

Every option the library implements is mapped; every other bathsearch option, an alignment query and a target file that is not
plain FASTA are refused (exit status 1, a message naming it).

--qformat fasta takes an unaligned protein FASTA file as the query (the tutorial's bathsearch --hmmout AMP_N.bhmm -o AMP_N.out
AMP_N.fa target-AMP_N.fa): one single-sequence model per record, built by bathbuild's builder (bathbuild.build_models: --mx /
--mxfile / --popen / --pextend, --ct, --w_beta / --w_length with bathbuild's meaning; the builder's seed is 42 with reseeding,
whatever --seed says; the default calibration sizes), calibrated on the GPU in batches of 16 (one by one with --arith odds3|odds),
written to --hmmout's file or to a temporary file that is removed on every exit path, and searched as read back from that text.
The two frameshift taus are fitted only with --fs or --hmmout (bath_amd.calibrate fs=False otherwise: the standard filters alone);
--fsonly without either is refused.  Every record is checked before any file is opened or the GPU touched.  The header names the
query file as given; the tabular tails name --hmmout's file when given (the reference prints the name of the /tmp file it leaves
behind there; this driver leaves none and names the query file).  Unlike the reference, which detects a single-record FASTA query
by itself, the format must be asserted: a sequence file without --qformat is refused, and so is a model file with it.  With
--gpus N the parent starts one child that builds the file and ends, then the ranks.

--gpus N (1..16) runs one search over N ranks, one process per GPU (rank r on device r): the parent checks the command line and the
inputs, opens no GPU and starts N fresh children (launch_ranks).  Every rank ingests the whole target file, the (query, window group)
items of every query are cut and dealt the same way on every rank (search_plan), each query's hits with their traces travel to its
owner rank, which merges them in item order and renders the query, and rank 0 writes the queries in order; the output does not
depend on N.  BATH_SEARCH_SHARE_DEVICE=1 puts every rank on device 0 and BATH_SEARCH_BACKEND=gloo runs the collectives on CPU
tensors (default nccl); each rank gets an equal share of the parent's CPUs as BATH_HIP_HOST_THREADS unless that is set.

--workers N (1..8, default 1; an extension like --ensemble: no header line) searches the queries of the model file side by side on
one GPU: N contexts on the device, one host thread each, all reading the one device copy of the targets (FastaTargets.seqs(ctx=)).
There is one search loop: without the option, or with N = 1, it runs on one context and one worker thread (_workers_search), and
a rank of --gpus runs its share of the items through the same pool (_rank_search); plan_pieces walks the targets for both,
_search_items is the only loop over the blocks of windows, _render_query finishes and renders every query, Output writes the files.
Within a piece of the targets the queries of a batch are drawn from a shared counter, longest first (dist.item_cost); every query
is finished and rendered by the worker that searched its last piece, and an ordered writer (OrderedWriter) holds its text until
every earlier query's text is written, so the output is the N = 1 output byte for byte but for the timing lines.  At most 2N
queries' hits are alive at once, and the models and plans of at most two batches of 2N (feed_batches).  A failure at query k
writes the queries before k, nothing from k on, one message, status 1.
With --gpus G every rank runs its items on N contexts of its device; BATH_HIP_HOST_THREADS is then the CPU share / (G x N).

--arith strict|odds3|odds (default strict; an extension like --ensemble: no header line; needs --fs) chooses the arithmetic of the
frameshift Forward / Backward recursions: strict, the log-space kernels bit-identical to the generic reference; odds3, the 3-codon
parsers in fp32 odds ratios (Context.set_fs_odds); odds, the 5-codon Forward / Backward of envelopes and regions too
(Context.set_fs5_odds) -- what the reference binary's --fs runs.  new_context applies it, so every context of --workers and every
rank of --gpus runs the same arithmetic.  Search a file converted with the same bathconvert --arith.
"""
import codecs
import contextlib
import os
import socket
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

import bath_amd as ba
from bath_amd import bathbuild as bb
from bath_amd import dist

BANNER = ("# bathsearch :: search protein profile(s) against DNA sequence database\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
RULE = "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n\n"

# option -> kind ('flag', int, float, str)
OPTIONS = {"-o": str, "--tblout": str, "--fstblout": str, "--fs": "flag", "--cigar": "flag", "--frameline": "flag", "--textw": int, "--notextw": "flag",
           "--notrans": "flag",    # accepted as the reference accepts it: a header line, nothing else
           "--ct": int, "-l": int, "-m": "flag", "-M": "flag", "--strand": str,
           "-E": float, "-T": float, "--incT": float, "-Z": float, "--seed": int,
           "--F1": float, "--F2": float, "--F3": float, "--F4": float, "--max": "flag", "--nobias": "flag", "--nonull2": "flag", "--fsonly": "flag",
           "--block_length": int, "--gpus": int,
           "--workers": int,       # an extension (no header line): queries searched side by side on N contexts of one GPU
           "--arith": str,         # an extension (no header line): the arithmetic of the --fs Forward / Backward recursions (ba.ARITH_MODES)
           "--ensemble": str,      # an extension, not a reference option (no header line): how --fs samples a multi-domain region's traces
           "--ensemble-std": str,  # ... and how the standard branch does (a search without --fs; the --fs windows that take that branch)
           # a sequence query (--qformat fasta) and how its models are built; all but --qformat itself require it
           "--qformat": str, "--hmmout": str, "--popen": float, "--pextend": float, "--mx": str, "--mxfile": str, "--w_beta": float,
           "--w_length": int}
MAX_GPUS = 16
MAX_WORKERS = 8
# bathsearch options this driver does not implement: refused, never ignored (--crick and --watson too: the reference declares them
# and never reads them)
REFUSED = ["-h", "--splice", "--exontblout", "--acc", "--noali", "--min_intron", "--max_intron",
           "--incE", "--tformat", "--singlemx", "--cpu",
           "--restrictdb_stkey", "--restrictdb_n", "--ssifile", "--domZ", "--domE", "--domT", "--incdomE", "--incdomT", "--crick", "--watson",
           "--nodeinfo"]
EXCLUSIVE = [("-m", "-M"), ("--textw", "--notextw"), ("-E", "-T"), ("--max", "--F1"), ("--max", "--F2"), ("--max", "--F3"), ("--max", "--F4"),
             ("--max", "--nobias"), ("--mx", "--mxfile")]
BUILD_OPTIONS = ("--hmmout", "--popen", "--pextend", "--mx", "--mxfile", "--w_beta", "--w_length")     # how a sequence query's models are built
REQUIRES = {"--frameline": "--fs", "--cigar": "--tblout", "--F4": "--fs", "--arith": "--fs", "--fstblout": "--fs",
            **{o: "--qformat" for o in BUILD_OPTIONS}}
BUILD_BATCH = 16            # a sequence query's models calibrated per bath_amd.calibrate_batch call (strict arithmetic)
BUILD_SEED = 42             # p7_search_builder creates its builder without options (p7_builder.c:67-73): seed 42, reseeded per model


# bathsearch.c:748-750 (the reference's spelling): a model without the frameshift taus, such as a plain HMMER3 file's
NOT_FORMATED = "HMM file %s not formated for this version bathsearch. Please run 'bathconvert new_file.bhmm old_file.bhmm'."

CT_MISMATCH = ("Error: Requested codon translation tabel ID %d does not match the codon translation tabel ID of the HMM file %s. "
               "Please either run bathsearch with option '--ct %d' or run bathconvert with option '--ct %d'.\n")


class UsageError(Exception):
    pass


def parse_args(argv):
    """(options dict in command-line order, hmmfile, seqfile); raises UsageError naming the offending option."""
    opts, pos, i = {}, [], 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("-") and len(a) > 1:
            name, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") and "=" in a else (a, None)
            if name in REFUSED:
                raise UsageError("option %s is not supported by this bathsearch" % name)
            kind = OPTIONS.get(name)
            if kind is None:
                raise UsageError("unknown option %s" % name)
            if kind == "flag":
                if val is not None:
                    raise UsageError("option %s takes no argument" % name)
                opts[name] = True
            else:
                if val is None:
                    i += 1
                    if i >= len(argv):
                        raise UsageError("option %s needs an argument" % name)
                    val = argv[i]
                try:
                    opts[name] = kind(val)
                except ValueError:
                    raise UsageError("option %s: bad argument %r" % (name, val))
        else:
            pos.append(a)
        i += 1
    if len(pos) != 2:
        raise UsageError("Incorrect number of command line arguments: bathsearch [options] <hmmfile> <seqfile>")
    for a, b in EXCLUSIVE:
        if a in opts and b in opts:
            raise UsageError("options %s and %s are incompatible" % (a, b))
    for a, b in REQUIRES.items():
        if a in opts and b not in opts:
            raise UsageError("option %s requires %s" % (a, b))
    if "--qformat" in opts:
        if opts["--qformat"] in ("afa", "stockholm"):
            raise UsageError("option --qformat %s: alignment queries are not supported; --qformat fasta searches with unaligned protein "
                             "sequences" % opts["--qformat"])
        if opts["--qformat"] != "fasta":
            raise UsageError("option --qformat: %r is not a query format this bathsearch takes (fasta)" % opts["--qformat"])
        if "--fsonly" in opts and "--fs" not in opts and "--hmmout" not in opts:
            raise UsageError("option --fsonly with a sequence query needs --fs or --hmmout: the frameshift taus are fitted only then")
        for o in BUILD_OPTIONS[1:]:                      # bathbuild's ranges
            if o in opts and bb.OPTIONS[o][2] is not None and not bb.OPTIONS[o][2](opts[o]):
                raise UsageError("option %s: %s is out of range" % (o, opts[o]))
        if "--hmmout" in opts and any(os.path.abspath(opts["--hmmout"]) == os.path.abspath(f) for f in pos):
            raise UsageError("option --hmmout: %s is an input of this search" % opts["--hmmout"])
    if "--strand" in opts and opts["--strand"] not in ("plus", "minus", "both"):
        raise UsageError("option --strand: expected plus, minus or both")
    for o in ("--ensemble", "--ensemble-std"):
        if o in opts and opts[o] not in ba.ENSEMBLE_MODES:
            raise UsageError("option %s: expected serial, streams or device" % o)
    if "--arith" in opts and opts["--arith"] not in ba.ARITH_MODES:
        raise UsageError("option --arith: expected %s" % ", ".join(ba.ARITH_MODES))
    if opts.get("--textw", 150) < 120:
        raise UsageError("option --textw: n >= 120")
    if opts.get("--block_length", 50000) < 50000:
        raise UsageError("option --block_length: n >= 50000")
    if not 1 <= opts.get("--gpus", 1) <= MAX_GPUS:
        raise UsageError("option --gpus: 1 <= n <= %d" % MAX_GPUS)
    if not 1 <= opts.get("--workers", 1) <= MAX_WORKERS:
        raise UsageError("option --workers: 1 <= n <= %d" % MAX_WORKERS)
    if opts.get("-E", 1.0) <= 0:
        raise UsageError("option -E: x > 0")
    if opts.get("-Z", 0.0) < 0 or opts.get("--seed", 0) < 0:
        raise UsageError("option %s: must not be negative" % ("-Z" if opts.get("-Z", 0.0) < 0 else "--seed"))
    return opts, pos[0], pos[1]


def output_header(opts, hmmfile, seqfile):
    """The banner and option lines of the main output (bathsearch.c output_header); <hmmfile>: the query file as given on the
    command line, a model file or (--qformat fasta) a sequence file."""
    o = opts
    s = BANNER
    s += "# query HMM file:                                %s\n" % hmmfile
    s += "# target sequence database:                      %s\n" % seqfile
    s += "# codon translation table:                       %d\n" % o.get("--ct", 1)
    lines = [("-o", "# output directed to file:                       %s\n"), ("--tblout", "# per-seq hits tabular output:                   %s\n"),
             ("--fstblout", "# frameshift tabular output:                     %s\n")]
    for k, f in lines:
        if k in o:
            s += f % o[k]
    if "--hmmout" in o:
        s += "# hmm output:                                    %s\n" % o["--hmmout"]
    if "--notextw" in o:
        s += "# max ASCII text line length:                    unlimited\n"
    if "--textw" in o:
        s += "# max ASCII text line length:                    %d\n" % o["--textw"]
    if "--notrans" in o:
        s += "# show translated DNA sequence:                  no\n"
    for k, f in [("--popen", "# gap open probability:                          %f\n"), ("--pextend", "# gap extend probability:                        %f\n"),
                 ("--mx", "# subst score matrix (built-in):                 %s\n"), ("--mxfile", "# subst score matrix (file):                     %s\n")]:
        if k in o:
            s += f % o[k]
    for k, f in [("-E", "# sequence reporting threshold:       E-value <= %g\n"), ("-T", "# sequence reporting threshold:         score >= %g\n"),
                 ("--incT", "# sequence inclusion threshold:         score >= %g\n")]:
        if k in o:
            s += f % o[k]
    if "--max" in o:
        s += "# Max sensitivity mode:                          on [all heuristic filters off]\n"
    for k, f in [("--F1", "# MSV filter P threshold:                     <= %g\n"), ("--F2", "# Vit filter P threshold:                     <= %g\n"),
                 ("--F3", "# Fwd filter P threshold:                     <= %g\n"), ("--F4", "# ORF P threshold for FS FWD:                 <= %g\n")]:
        if k in o:
            s += f % o[k]
    if "--nobias" in o:
        s += "# biased composition HMM filter:                 off\n"
    if "--nonull2" in o:
        s += "# null2 bias corrections:                        off\n"
    if "--fs" in o:
        s += "# Use the frameshift aware algorithms\n"
    if "--fsonly" in o:
        s += "# Use only the frameshift aware pipeline\n"
    if "-Z" in o:
        s += "# database size is set to:                       %.1f Mb\n" % o["-Z"]
    if "--seed" in o:
        s += ("# random number seed:                            one-time arbitrary\n" if o["--seed"] == 0 else
              "# random number seed set to:                     %d\n" % o["--seed"])
    for k, f in [("--qformat", "# query format asserted:                         %s\n"), ("--w_beta", "# window length beta value:                      %g\n"),
                 ("--w_length", "# window length :                                %d\n")]:
        if k in o:
            s += f % o[k]
    if "-l" in o:
        s += "# minimum ORF length:                            %d\n" % o["-l"]
    if "-m" in o:
        s += "# ORFs must initiate with AUG only:              yes\n"
    if "-M" in o:
        s += "# ORFs must start with allowed initiation codon: yes\n"
    if "--strand" in o:
        s += {"plus": "# only translate the forward strand:             yes\n",
              "minus": "# only translate the reverse complement strand:  yes\n",
              "both": "# translate both strands:                        yes\n"}[o["--strand"]]
    return s + RULE


def spoof_cmdline(argv):
    return "bathsearch " + " ".join(argv) + " "


def tabular_tail(hmmfile, seqfile, argv, cwd=None, date=None):
    """p7_tophits_TabularTail for bathsearch."""
    return ("#\n# Program:         bathsearch\n# Query file:      %s\n# Target file:     %s\n# Option settings: %s\n"
            "# Current dir:     %s\n# Date:            %s\n# [ok]\n") % (hmmfile, seqfile, spoof_cmdline(argv), cwd or os.getcwd(),
                                                                          date or time.strftime("%a %b %e %H:%M:%S %Y"))


def _hms(t):
    h, r = divmod(t, 3600)
    m, s = divmod(r, 60)
    return "%02d:%02d:%05.2f" % (h, m, s)


def timing_lines(cpu_user, cpu_sys, elapsed, nres, M):
    mcs = (nres * M / elapsed / 1e6) if elapsed > 0 else 0.0
    return "# CPU time: %.2fu %.2fs %s Elapsed: %s\n# Mc/sec: %.2f\n" % (cpu_user, cpu_sys, _hms(cpu_user + cpu_sys), _hms(elapsed), mcs)


def model_descriptions(path):
    """DESC of every model of a model file, in order (the library's model record has no description)."""
    out, cur = [], None
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b"HMMER") or line.startswith(b"BATH"):
                cur = None
            elif line.startswith(b"DESC ") and cur is None:
                cur = line[5:].decode("latin-1").strip()
            elif line.startswith(b"//"):
                out.append(cur)
                cur = None
    return out


# complement of every DNA code (DNA_SYMS = ACGT-RYMKSWHBVDN*~: IUPAC pairs; gap, N, * and ~ are their own)
COMPLEMENT = np.array([3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 14, 13, 12, 11, 15, 16, 17], dtype=np.uint8)


def revcomp(codes):
    return COMPLEMENT[np.asarray(codes, dtype=np.uint8)][::-1].copy()


def check_target_file(path):
    """Refuse what is not plain FASTA (compressed, or another format) before any byte goes to the device."""
    with open(path, "rb") as fh:
        head = fh.read(1 << 16)
    if path.endswith(".gz") or head[:2] == b"\x1f\x8b":
        raise UsageError("target file %s is compressed: only plain FASTA targets are supported" % path)
    first = head.lstrip(b" \t\r\n\v\f")[:1]
    if first and first != b">":
        raise UsageError("target file %s is not in FASTA format" % path)


class Targets:
    """The target file on the device: parsed once and kept when its codes fit <resident_bytes>, else parsed again per query in
    pieces of at most that many codes (records completed so far; a single record is kept whole)."""

    def __init__(self, ctx, path, chunk_bytes, resident_bytes):
        self.ctx, self.path, self.chunk_bytes, self.resident_bytes = ctx, path, int(chunk_bytes), int(resident_bytes)
        self.size = os.path.getsize(path)
        self.resident = self.size <= self.resident_bytes
        self.pinned = ba.PinnedBuffer(max(1, min(self.chunk_bytes, self.size)))
        self.ft = None

    def _parse(self):
        """Yields (FastaTargets, lo, hi) for every piece of complete records, then closes the handle."""
        ft = ba.FastaTargets(self.ctx)
        lo = 0
        with open(self.path, "rb", buffering=0) as fh:
            while True:
                n = fh.readinto(memoryview(self.pinned.array)[:self.chunk_bytes])
                if not n:
                    break
                ft.feed(self.pinned, n)
                if not self.resident and ba.lib().bath_hip_fasta_symbols(ft._h) - (ft.records()["sym_start"][lo] if len(ft) > lo else 0) >= self.resident_bytes:
                    hi = max(lo, len(ft) - 1)               # the last record may be open
                    if hi > lo:
                        yield ft, lo, hi
                        ft.release(hi)
                        lo = hi
        ft.finish()
        yield ft, lo, len(ft)

    def pieces(self):
        if not self.resident:
            yield from self._parse()
            return
        if self.ft is None:
            for ft, lo, hi in self._parse():
                pass
            self.ft, self.lo, self.hi = ft, lo, hi
        yield self.ft, self.lo, self.hi


class Hit:
    __slots__ = ("trace", "target", "start0", "n")


def block_cuts(ns, block_nt):
    """Boundaries of the blocks of at most <block_nt> nucleotides that windows of lengths <ns> run in (a window is never cut)."""
    cut = [0]
    acc = 0
    for i, n in enumerate(ns):
        if acc and acc + int(n) > block_nt:
            cut.append(i); acc = 0
        acc += int(n)
    cut.append(len(ns))
    return cut


def pipeline_overrides(opts):
    """The Pipeline parameters the options set (every rank of a --gpus N search sets the same)."""
    over = {}
    if "--max" in opts:
        over.update(F1=1.0, F2=1.0, F3=1.0, F4=1.0, do_biasfilter=0)
    for k in ("F1", "F2", "F3", "F4"):
        if "--" + k in opts:
            over[k] = opts["--" + k]
    if "--nobias" in opts:
        over["do_biasfilter"] = 0
    if "--nonull2" in opts:
        over["do_null2"] = 0
    if "--fsonly" in opts:
        over["std_pipe"] = 0
    if "-l" in opts:
        over["min_orf_len"] = opts["-l"]
    over["strands"] = {"both": ba.STRAND_BOTH, "plus": ba.STRAND_TOPONLY, "minus": ba.STRAND_BOTTOMONLY}[opts.get("--strand", "both")]
    if "-m" in opts:
        over["initiator"] = ba.INIT_AUG
    if "-M" in opts:
        over["initiator"] = ba.INIT_TABLE
    if "--incT" in opts:
        over["inc_by_E"] = 0
    if "-T" in opts:
        over["T"] = opts["-T"]
    if "--seed" in opts:
        over["seed"] = opts["--seed"]
    return over


def finish_tophits(th, opts, nres, max_length, E):
    """The end of a query's search: -T / --incT thresholds, E-values over the whole search's residues (or -Z), duplicates, sorting."""
    if "--incT" in opts or "-T" in opts:
        th.set_score_thresholds(by_E="-T" not in opts, T=opts.get("-T", 0.0), inc_by_E="--incT" not in opts, incT=opts.get("--incT", 0.0))
    if "-Z" in opts:
        search_nres = int(1e6 * opts["-Z"]) * (2 if opts.get("--strand", "both") == "both" else 1)
    else:
        search_nres = nres
    th.finalize(search_nres, max_length, E)


def _key(d):
    return (int(d.window), int(d.iali), int(d.jali), int(d.ihmm), int(d.jhmm), float(d.bitscore))


def main_output_query(hmm, desc, r, opts, targets, elapsed, cpu, fs_rows=None):
    """The query's block of the main output.  fs_rows: a list that receives, per reported hit in the order of the block, the hit's
    --fstblout rows (ba.frameshift_rows), made from the window codes its alignment block is rendered from."""
    fs = "--fs" in opts
    textw = 0 if "--notextw" in opts else opts.get("--textw", 150)
    th = r["th"]
    s = "Query:       %s  [M=%d]\n" % (hmm.name, hmm.M)
    if hmm.acc:
        s += "Accession:   %s\n" % hmm.acc
    if desc:
        s += "Description: %s\n" % desc
    s += th.targets(fs_pipe=fs, textw=textw) + "\n\n"
    s += "Annotation for each hit (and alignments):\n"
    heads = th.annotations(hmm.M, fs_pipe=fs)
    reported = [(d, idx) for d, idx, fl in th.hits() if fl & 1]
    for head, (d, idx) in zip(heads, reported):
        h = r["traces"][_key(d)]
        codes = targets.codes_of(h.target, h.start0, h.n)
        bottom = d.iali > d.jali
        strand = revcomp(codes) if bottom else codes
        win = strand[h.trace[0].win_start - 1:]
        if fs_rows is not None:
            fs_rows.append(ba.frameshift_rows(h.trace, win, r["gm5"], d.iali, d.jali))
        ali = ba.alidisplay_print(h.trace, win, hmm, d.iali, d.jali, r["names"][idx], gm_fs5=r["gm5"], gm=r["gm"], ncbi_table=opts.get("--ct", 1),
                                  textw=textw, frameline="--frameline" in opts,
                                  initiator=ba.INIT_AUG if "-m" in opts else (ba.INIT_TABLE if "-M" in opts else ba.INIT_ANY))
        s += head + "\n  Alignment:\n" + "  score: %.1f bits\n" % d.bitscore + ali + "\n"
    if not reported:
        s += "\n   [No hits detected that satisfy reporting thresholds]\n"
    s += "\n\n"
    s += th.statistics(r["stats"], r["pipe"].params, 1, hmm.M, r["nseqs"])
    s += timing_lines(cpu[0], cpu[1], elapsed, r["nres"], hmm.M)
    s += "//\n"
    return s


def tabular_query(hmm, th, opts, q, fs_rows):
    """(--tblout rows, --fstblout rows) of query <q>, '' for a file not asked for; the header lines go with the first query."""
    tbl = th.tblout(hmm.name, hmm.acc, hmm.M, fs_pipe="--fs" in opts, show_cigar="--cigar" in opts, show_header=(q == 0)) if "--tblout" in opts else ""
    fstbl = th.fstblout(hmm.name, hmm.acc, fs_rows, show_header=(q == 0)) if "--fstblout" in opts else ""
    return tbl, fstbl


class Output:
    """The files a search writes: the main output (-o, or the stream given), --tblout and --fstblout.  A context manager: the
    banner is written on entry, and on every exit the files it opened are closed and a stream it was given is flushed."""

    def __init__(self, argv, opts, hmmfile, seqfile, stdout):
        # <hmmfile>: the query file as given.  The tails name the file the models were read from when the run keeps it
        # (bathsearch.c:728 replaces cfg->queryfile with the file it built; that is --hmmout's, or a temporary one this run removes)
        self.header, self.tail_args, self.stdout = output_header(opts, hmmfile, seqfile), (opts.get("--hmmout", hmmfile), seqfile, argv), stdout
        self.ofp = open(opts["-o"], "w") if "-o" in opts else stdout
        self.tblfp = open(opts["--tblout"], "w") if "--tblout" in opts else None
        self.fstblfp = open(opts["--fstblout"], "w") if "--fstblout" in opts else None

    def __enter__(self):
        self.ofp.write(self.header)
        self.ofp.flush()
        return self

    def write_query(self, q, text):
        """Query <q>'s (main-output block, --tblout rows, --fstblout rows), as _render_query returns them."""
        self.ofp.write(text[0])
        if self.tblfp:
            self.tblfp.write(text[1])
        if self.fstblfp:
            self.fstblfp.write(text[2])
        self.ofp.flush()

    def finish(self):
        """The end of a search that succeeded: the tails of the tabular files and the [ok] line."""
        for fp in (self.tblfp, self.fstblfp):
            if fp:
                fp.write(tabular_tail(*self.tail_args))
        self.ofp.write("[ok]\n")

    def __exit__(self, *exc):
        if self.ofp is self.stdout:
            self.ofp.flush()
        else:
            self.ofp.close()
        for fp in (self.tblfp, self.fstblfp):
            if fp:
                fp.close()


class _CodesSource:
    """Window codes of reported hits, from the device copy of the targets (parsed again when they were not kept resident)."""

    def __init__(self, targets):
        self.t = targets
        self._ft = None
        self._lock = threading.Lock()            # worker threads render side by side (--workers)

    def codes_of(self, target, start0, n):
        if self.t.resident:
            return self.t.ft.codes(target, start0, n)
        with self._lock:
            self._parse_again()
        return self._ft.codes(target, start0, n)

    def _parse_again(self):
        if self._ft is None:                     # a streamed file: the hits' records, parsed once more
            ft = ba.FastaTargets(self.t.ctx)
            with open(self.t.path, "rb", buffering=0) as fh:
                while True:
                    k = fh.readinto(memoryview(self.t.pinned.array)[:self.t.chunk_bytes])
                    if not k:
                        break
                    ft.feed(self.t.pinned, k)
            ft.finish()
            self._ft = ft


# ---------------------------------------------------------------------------------------------------------------------------
# --gpus N: one search over N ranks, one process per GPU.  The parent checks the command line and the inputs, opens no GPU and
# starts N fresh children (rank_main).  Every rank ingests the whole target file, cuts every query's windows into (query, window
# group) items the same way (search_plan), searches the items dealt to it, and ships each item's hits -- with their CIGARs and
# traces, in the library's hit stream -- and counters to the query's owner (dist.query_owner), which merges them in item order,
# finishes the query over the whole search's residues and renders its main-output block and its --tblout and --fstblout rows.
# Rank 0 writes the blocks in query order and the [ok] line last.
# ---------------------------------------------------------------------------------------------------------------------------

BATCH_QUERIES = 256         # queries planned and merged together: what a rank holds of the hits at once
STOP_GRACE_S = 5.0          # a failed search: SIGTERM to the other ranks, SIGKILL after this long
STAT_FIELDS = [f for f, _ in ba.PipelineStats._fields_]


class Item:
    __slots__ = ("query", "lo", "hi", "owner", "nres_before")

    def __init__(self, query, lo, hi, owner, nres_before):
        self.query, self.lo, self.hi, self.owner, self.nres_before = query, lo, hi, owner, nres_before

    def __repr__(self):
        return "Item(%d, %d, %d, owner=%d, nres_before=%d)" % (self.query, self.lo, self.hi, self.owner, self.nres_before)


def window_nres(windows, strand="both"):
    """stats.nres of every window (FASTA_WINDOW_DTYPE): its new nucleotides (length minus context), once per strand searched."""
    w = np.asarray(windows)
    return (w["n"].astype(np.int64) - w["context"].astype(np.int64)) * (2 if strand == "both" else 1)


def search_plan(windows_by_query, M_by_query, world, strand="both"):
    """[Item] of one batch of queries, the same on every rank without communication: query q's windows cut into consecutive groups
    in proportion to its share of the work (dist.query_items_weighted, cost windows' nucleotides x (M + 150)), dealt to the ranks
    longest first (dist.deal, dist.item_cost).  nres_before: the residues counted before the item's first window when the query's
    windows are searched in order (the summed stats.nres of its earlier windows)."""
    ns = [np.asarray(w)["n"].astype(np.int64) for w in windows_by_query]
    items = dist.query_items_weighted([len(n) for n in ns], [float(n.sum()) * (M + 150.0) for n, M in zip(ns, M_by_query)], world)
    owner = dist.deal([dist.item_cost(M_by_query[q], int(ns[q][lo:hi].sum())) for q, lo, hi in items], world)
    before = [np.concatenate([[0], np.cumsum(window_nres(w, strand))]) for w in windows_by_query]
    return [Item(q, lo, hi, o, int(before[q][lo])) for (q, lo, hi), o in zip(items, owner)]


def plan_pieces(targets, hmms, opts, world, heads):
    """The loop over the targets for one batch of models, the same for every coordinator: yields (piece, FastaTargets, the window
    table of every model, search_plan's items for <world>) for every piece of targets.pieces(), an item's nres_before counted over
    the whole search (the residues of the query's earlier pieces added).  heads: the (names, descriptions, lengths) lists that
    receive the piece's targets before it is yielded; None for a caller that has them already.  A streamed piece is released when
    the generator resumes."""
    strand = opts.get("--strand", "both")
    block_length = opts.get("--block_length", dist.BLOCK_LENGTH)
    base = [0] * len(hmms)                               # residues of the earlier pieces, per query
    for piece, (ft, lo, hi) in enumerate(targets.pieces()):
        if heads is not None:
            names, descs, lengths = heads
            recs = ft.records()[lo:hi]
            for name, desc in ba.fasta_headers(targets.path, recs):
                names.append(name); descs.append(desc)
            lengths.extend(int(x) for x in recs["length"])
        wins = [ft.windows(h.max_length, block_length, lo, hi) for h in hmms]
        plan = search_plan(wins, [h.M for h in hmms], world, strand)
        for it in plan:
            it.nres_before += base[it.query]
        for k in range(len(hmms)):
            base[k] += int(window_nres(wins[k], strand).sum())
        yield piece, ft, wins, plan


def host_threads_per_rank(n, environ=None, affinity=None):
    """BATH_HIP_HOST_THREADS for each of <n> ranks: the CPUs this process may run on (its affinity set, lowered to OMP_NUM_THREADS
    when that is set) split evenly, at least one each; None when the user has set it (it is then left as it is)."""
    env = os.environ if environ is None else environ
    if env.get("BATH_HIP_HOST_THREADS"):
        return None
    budget = len(os.sched_getaffinity(0) if affinity is None else affinity)
    try:
        omp = int(env.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        omp = 0
    if omp > 0:
        budget = min(budget, omp)
    return max(1, budget // int(n))


def host_threads_per_worker(workers, ranks=1, environ=None, affinity=None):
    """BATH_HIP_HOST_THREADS for each of <workers> contexts in each of <ranks> processes: host_threads_per_rank's budget split
    over all of them, at least one each; None when the user has set it."""
    return host_threads_per_rank(int(ranks) * int(workers), environ=environ, affinity=affinity)


def rank_env(n, rank, port, environ=None, threads=None):
    """The environment of rank <rank> of <n>: torch.distributed's rendezvous variables and the host-thread share."""
    env = {k: v for k, v in (os.environ if environ is None else environ).items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE")}
    env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if threads is not None:
        env["BATH_HIP_HOST_THREADS"] = str(threads)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _drain(pipe, sink):
    """Copies a child's pipe into <sink> (a list of bytes, or a text stream) until it closes."""
    dec = codecs.getincrementaldecoder("utf-8")("replace")
    for chunk in iter(lambda: pipe.read1(1 << 16), b""):
        if isinstance(sink, list):
            sink.append(chunk)
        else:
            sink.write(dec.decode(chunk))
            sink.flush()
    pipe.close()


def _stop(procs, grace=STOP_GRACE_S):
    for p in procs:
        if p.poll() is None:
            p.terminate()
    end = time.time() + grace
    for p in procs:
        try:
            p.wait(max(0.0, end - time.time()))
        except subprocess.TimeoutExpired:
            pass
    for p in procs:
        if p.poll() is None:
            p.kill()
    for p in procs:
        p.wait()


def launch_ranks(n, argv, stdout, run_kw):
    """Starts the <n> ranks as fresh child processes, relays rank 0's standard output, and waits for them.  When a rank fails the
    others are stopped, its error message is printed once and the status is 1.  No child outlives this call."""
    code = "import sys; from bath_amd import bathsearch as b; sys.exit(b.rank_main(sys.argv[1:], **%r))" % (run_kw,)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code] + list(argv)
    port, threads = _free_port(), host_threads_per_worker(parse_args(list(argv))[0].get("--workers", 1), n)
    procs, errs, readers = [], [], []
    t0 = "%.6f" % time.time()
    try:
        for r in range(n):
            env = rank_env(n, r, port, threads=threads)
            env["BATH_SEARCH_T0"] = t0
            p = subprocess.Popen(cmd, env=env, stdin=subprocess.DEVNULL,
                                 stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE)
            procs.append(p)
            errs.append([])
            readers.append(threading.Thread(target=_drain, args=(p.stderr, errs[-1]), daemon=True))
            readers[-1].start()
            if r == 0:
                readers.append(threading.Thread(target=_drain, args=(p.stdout, stdout), daemon=True))
                readers[-1].start()
        failed = None
        while failed is None:
            codes = [p.poll() for p in procs]
            bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                failed = bad[0]
            elif all(c == 0 for c in codes):
                break
            else:
                time.sleep(0.02)
    finally:
        _stop(procs)
        for t in readers:
            t.join()
    if failed is None:
        sys.stderr.write("".join(ln for ln in b"".join(errs[0]).decode("utf-8", "replace").splitlines(True) if not ln.startswith("[Gloo] ")))
        return 0
    msg = b"".join(errs[failed]).decode("utf-8", "replace")
    sys.stderr.write(msg if msg.strip() else "Error: rank %d of the --gpus %d search exited with status %d\n" % (failed, n, procs[failed].returncode))
    return 1


def _pack_item(q, piece, lo, stats, geometry, stream):
    """One item's result as it travels to the query's owner: ids, counters, each hit's window (start, length), the hit stream."""
    head = np.array([q, piece, lo] + [int(getattr(stats, f)) for f in STAT_FIELDS] + [len(geometry), len(stream)], dtype="<i8")
    return head.tobytes() + np.asarray(geometry, dtype="<i8").reshape(-1, 2).tobytes() + stream


def _unpack_items(buf):
    p, nh = 0, 3 + len(STAT_FIELDS) + 2
    while p < len(buf):
        head = np.frombuffer(buf, dtype="<i8", count=nh, offset=p); p += 8 * nh
        nhit, nstream = int(head[-2]), int(head[-1])
        geometry = np.frombuffer(buf, dtype="<i8", count=2 * nhit, offset=p).reshape(-1, 2); p += 16 * nhit
        yield int(head[0]), int(head[1]), int(head[2]), dict(zip(STAT_FIELDS, (int(x) for x in head[3:3 + len(STAT_FIELDS)]))), geometry, buf[p:p + nstream]
        p += nstream


def _send_text(text, dst, dev):
    import torch
    import torch.distributed as tdist
    b = text.encode()
    tdist.send(torch.tensor([len(b)], dtype=torch.int64, device=dev), dst)
    if b:
        tdist.send(torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev), dst)


def _recv_text(src, dev):
    import torch
    import torch.distributed as tdist
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    tdist.recv(n, src)
    if not int(n.item()):
        return ""
    buf = torch.empty(int(n.item()), dtype=torch.uint8, device=dev)
    tdist.recv(buf, src)
    return bytes(buf.cpu().numpy().tobytes()).decode()


def _search_items(ctx, hmm, ft, wins, items, opts, block_nt, cancelled=None):
    """This rank's items of one query in one piece of the targets: [(item, stats, hit window geometry, hit stream)].  <ctx> is the
    targets' own context or a worker context beside it (the blocks are then gathered for it); cancelled(): asked before every
    pipeline call, True ends the search with Cancelled."""
    gather_for = None if ctx is ft.ctx else ctx
    fs = "--fs" in opts
    ct = opts.get("--ct", 1)
    om = ba.OProfile(ctx, ba.Profile(hmm))
    pipe = ba.Pipeline(ctx, om, fs_pipe=fs, ncbi_table=ct, **pipeline_overrides(opts))
    if fs:
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=ct))
        om5 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 5, ncbi_table=ct))
    E = opts.get("-E", 10.0)
    out = []
    for it in items:
        iw = wins[it.lo:it.hi]
        total, nres = ba.PipelineStats(), it.nres_before
        doms, trs, geometry = [], [], []
        cut = block_cuts(iw["n"], block_nt)
        for a, b in zip(cut[:-1], cut[1:]):
            w = iw[a:b]
            if cancelled is not None and cancelled():
                raise Cancelled()
            blk = ft.seqs(w, ctx=gather_for)
            if fs:
                stats, _, dm, _ = pipe.run_frameshift_domains(om3, om5, blk, E_report=E, nres_before=nres)
            else:
                stats, dm, _ = pipe.run_hits(blk, E_report=E, nres_before=nres)
            for f in STAT_FIELDS:
                setattr(total, f, getattr(total, f) + getattr(stats, f))
            nres += stats.nres
            for d in dm:                                 # window -> target coordinates
                win = w[d.window]
                off = int(win["start0"])
                d.ienv += off; d.jenv += off; d.iali += off; d.jali += off
                d.window = int(win["target"])
                geometry.append((off, int(win["n"])))
            doms.extend(dm)
            trs.extend(pipe.traces())
            del blk
        stream = ba.HitArray.from_domains(doms).to_bytes(traces=trs)
        out.append((it, total, geometry, stream))
    return out


def _render_query(q, hmm, desc, parts, opts, names, descs, lengths, src, t0, c0):
    """The owner's end of query <q>: its items' hits added in item order, counters summed, the query finished (finish_tophits), and
    its (main-output block, --tblout rows, --fstblout rows) rendered, '' for a file not asked for."""
    fs = "--fs" in opts
    ct = opts.get("--ct", 1)
    th = ba.TopHits()
    total = ba.PipelineStats()
    traces = {}
    for _key_, stats, geometry, stream in sorted(parts, key=lambda x: x[0]):
        for f in STAT_FIELDS:
            setattr(total, f, getattr(total, f) + stats[f])
        if len(geometry) == 0:
            continue
        th.add_serialized(stream, names, lengths, descs=descs)
        for (d, tr), (off, n) in zip(ba.HitArray.traces_from_bytes(stream), geometry):
            h = Hit()
            h.trace, h.target, h.start0, h.n = tr, int(d.window), int(off), int(n)
            traces.setdefault(_key(d), h)
    finish_tophits(th, opts, total.nres, hmm.max_length, opts.get("-E", 10.0))
    r = dict(th=th, stats=total, pipe=ba.Pipeline(None, None, fs_pipe=fs, ncbi_table=ct, **pipeline_overrides(opts)), traces=traces,
             nseqs=len(names), gm=ba.Profile(hmm), gm5=ba.FSProfile(hmm, 5, ncbi_table=ct), names=names, nres=total.nres)
    c1 = os.times()
    fs_rows = [] if "--fstblout" in opts else None
    block = main_output_query(hmm, desc, r, opts, src, time.time() - t0, (c1.user - c0.user, c1.system - c0.system), fs_rows)
    return (block,) + tabular_query(hmm, th, opts, q, fs_rows)


# ---------------------------------------------------------------------------------------------------------------------------
# The search in one process, --workers N or none (N = 1): queries side by side on N contexts of one GPU, one host thread per
# context (WorkerPool), all of them reading the one device copy of the targets; the finished queries' texts are written in query
# order (OrderedWriter).
# ---------------------------------------------------------------------------------------------------------------------------

class Cancelled(Exception):
    """A worker's search ended early: a query before its own has failed."""


class CtMismatch(Exception):
    """A model whose codon table is not the --ct one (the message is CT_MISMATCH, filled in)."""


class OrderedWriter:
    """write(q, text) for q = 0, 1, 2, ... in that order, whatever order the queries finish in.  A query is alive from its
    admission (WorkerPool admits a query when a worker picks its first job up; admit() does so for a caller without a pool) until
    its text is written; at most <bound> are alive at once, so a worker waits instead of running ahead and what is held does not
    grow with the number of queries.  put() hands a finished query's text over: it is held until every earlier one is written.
    fail_at(k): nothing from query k on is written any more; the queries before k still are (a query from k on that was admitted
    and hands no text over keeps its place: no query from k on is started any more, and the queries before k fit beside them)."""

    def __init__(self, write, bound):
        self.write, self.bound = write, int(bound)
        self.cv = threading.Condition()
        self.next, self.alive, self.limit, self.held = 0, 0, None, {}
        self.max_alive = self.max_held = 0

    def try_admit(self):
        with self.cv:
            if self.alive >= self.bound:
                return False
            self.alive += 1
            self.max_alive = max(self.max_alive, self.alive)
            return True

    def admit(self):
        with self.cv:
            while not self.try_admit():
                self.cv.wait()

    def put(self, q, text):
        with self.cv:
            if self.limit is not None and q >= self.limit:
                self.alive -= 1
            else:
                self.held[q] = text
                self.max_held = max(self.max_held, len(self.held))
                while self.next in self.held:
                    self.write(self.next, self.held.pop(self.next))
                    self.next += 1
                    self.alive -= 1
            self.cv.notify_all()

    def fail_at(self, k):
        with self.cv:
            self.limit = k if self.limit is None else min(self.limit, k)
            for q in [q for q in self.held if q >= self.limit]:
                del self.held[q]
                self.alive -= 1
            self.cv.notify_all()


class Round:
    """Jobs the workers draw from a shared counter: <queries> in the order they are handed out, <payload> what work() needs for
    them; admit: a job of this round is its query's first, and takes one of the writer's places."""

    def __init__(self, queries, payload=None, admit=False):
        self.queries, self.payload, self.admit, self.taken = list(queries), payload, admit, 0


class WorkerPool:
    """<n> host threads, thread w serving worker context w: work(w, round, query) for every job of every round submitted, rounds in
    the order of submit(), a round's jobs from a shared counter.  When work raises, or fail() is called, at query k: jobs of
    queries after k are not started, cancelled(q) turns True for them (a running search asks it before every pipeline call and
    ends), the writer writes nothing from k on, and the queries before k are still finished and written, as a search query after
    query leaves them.  wait() returns when every submitted job is done and raises the failure of the lowest query; close() joins
    the threads; close(exc), after the coordinating thread itself raised <exc>, first fails the pool at the lowest query not yet
    handed out, so that the workers do not search what is still queued.  start(w), when given, runs first on thread w (the driver
    binds the thread to its context's device there)."""

    def __init__(self, n, work, writer=None, start=None):
        self.work, self.writer, self.start = work, writer, start
        self.cv = writer.cv if writer is not None else threading.Condition()
        self.rounds, self.pending, self.closing, self.failure = [], 0, False, None
        self.threads = [threading.Thread(target=self._serve, args=(w,), name="bathsearch-worker-%d" % w) for w in range(n)]
        for t in self.threads:
            t.start()

    def submit(self, rnd):
        with self.cv:
            self.rounds.append(rnd)
            self.pending += len(rnd.queries)
            self.cv.notify_all()

    def cancelled(self, q):
        f = self.failure
        return f is not None and q > f[0]

    def fail(self, q, exc):
        with self.cv:
            if self.failure is None or q < self.failure[0]:
                self.failure = (q, exc)
            if self.writer is not None:
                self.writer.fail_at(self.failure[0])
            self.cv.notify_all()

    def _next(self):
        with self.cv:
            while True:
                while self.rounds and self.rounds[0].taken == len(self.rounds[0].queries):
                    self.rounds.pop(0)
                if self.rounds:
                    r = self.rounds[0]
                    q = r.queries[r.taken]
                    skip = self.failure is not None and q >= self.failure[0]
                    if skip or not (r.admit and self.writer is not None) or self.writer.try_admit():
                        r.taken += 1
                        return r, q, skip
                elif self.closing:
                    return None
                self.cv.wait()

    def _serve(self, w):
        if self.start is not None:
            try:
                self.start(w)
            except BaseException as e:
                self.fail(-1, e)
        for r, q, skip in iter(self._next, None):
            try:
                if not skip:
                    self.work(w, r, q)
            except Cancelled:
                pass
            except BaseException as e:
                self.fail(q, e)
            with self.cv:
                self.pending -= 1
                self.cv.notify_all()

    def barrier(self):
        """Returns when every submitted job is done or skipped."""
        with self.cv:
            while self.pending:
                self.cv.wait()

    def wait(self):
        self.barrier()
        if self.failure is not None:
            raise self.failure[1]

    def wait_written(self, k):
        """Returns True when the writer has written every query before <k>, False when a query has failed before that."""
        with self.cv:
            while self.writer.next < k and self.failure is None:
                self.cv.wait()
            return self.failure is None

    def close(self, exc=None):
        with self.cv:
            untaken = [r.queries[i] for r in self.rounds for i in range(r.taken, len(r.queries))]
            if exc is not None and untaken:
                self.fail(min(untaken), exc)
            self.closing = True
            self.cv.notify_all()
        for t in self.threads:
            t.join()


def new_context(device, opts):
    ctx = ba.Context(device)
    ctx.set_fs_strict(True)                              # in every --arith mode: the stages the odds switches do not cover
    arith = ba.ARITH_MODES[opts.get("--arith", "strict")]
    ctx.set_fs_odds(arith >= ba.ARITH_ODDS3)
    ctx.set_fs5_odds(arith >= ba.ARITH_ODDS)
    ctx.set_fs_ensemble(opts.get("--ensemble", "serial"))
    ctx.set_std_ensemble(opts.get("--ensemble-std", "serial"))
    return ctx


def longest_first(items_by_query, M_by_query, wins_by_query):
    """The queries (keys of <items_by_query>) by the estimated cost of their items (dist.item_cost), longest first."""
    cost = {k: sum(dist.item_cost(M_by_query[k], int(wins_by_query[k]["n"][it.lo:it.hi].sum())) for it in items) for k, items in items_by_query.items()}
    return sorted(cost, key=lambda k: (-cost[k], k))


class _Batch:
    """The queries [b0, b0 + len(hmms)) of a --workers search while they are alive."""

    def __init__(self, b0, hmms):
        self.b0, self.hmms = b0, hmms
        self.names, self.descs, self.lengths = [], [], []
        self.parts = [[] for _ in hmms]
        self.t0 = [None] * len(hmms)
        self.c0 = [None] * len(hmms)


def _workers_search(opts, hmmfile, seqfile, nq, write, device, chunk_bytes, block_nt, resident_bytes):
    """The single-process search, with --workers N or without (N = 1): the pieces of the targets outermost (plan_pieces with one
    rank), a query's items of a piece searched by _search_items, the query merged and rendered by _render_query, the queries of a
    batch of 2N spread over N contexts.  Resident targets are one piece: a query is rendered by the worker that searched it, and the
    next batch is prepared and handed out while the last one's queries are still running (feed_batches: never more than that one).
    Streamed targets: a piece is released when the generator resumes, so every worker is done with it first; the batch is rendered
    after its last piece.  write(q, text) gets every query's text in query order.  Raises what the search of the lowest failing
    query raised (CtMismatch, ba.FastaFormatError, ...), the queries before it written."""
    n = opts.get("--workers", 1)
    ct = opts.get("--ct", 1)
    qdescs = model_descriptions(hmmfile)
    ctxs = [new_context(device, opts) for _ in range(n)]
    targets = Targets(ctxs[0], seqfile, chunk_bytes, resident_bytes)
    src = _CodesSource(targets)
    writer = OrderedWriter(write, 2 * n)

    def render(b, k):
        q = b.b0 + k
        parts, b.parts[k] = b.parts[k], None
        writer.put(q, _render_query(q, b.hmms[k], qdescs[q] if q < len(qdescs) else None, parts, opts, b.names, b.descs, b.lengths, src,
                                    b.t0[k], b.c0[k]))

    def work(w, rnd, q):
        b, piece, ft, wins, items, last = rnd.payload
        k = q - b.b0
        if ft is not None:
            if b.t0[k] is None:
                b.t0[k], b.c0[k] = time.time(), os.times()
            for it, stats, geometry, stream in _search_items(ctxs[w], b.hmms[k], ft, wins[k], items[k], opts, block_nt, lambda: pool.cancelled(q)):
                b.parts[k].append(((piece, it.lo), {f: int(getattr(stats, f)) for f in STAT_FIELDS}, geometry, stream))
        if last:
            render(b, k)

    pool = WorkerPool(n, work, writer, start=lambda w: ctxs[w].synchronize())    # binds thread w to its context's device
    shared = None                                        # names, descriptions, lengths of resident targets: one list for every batch

    def prepare(b0, b1):
        """Loads the models [b0, b1) and hands their jobs to the pool, piece after piece."""
        nonlocal shared
        hmms = []
        for q in range(b0, b1):
            hmm = ba.HMM(hmmfile, q)
            if hmm.ct != ct:
                pool.fail(q, CtMismatch(CT_MISMATCH % (ct, hmmfile, hmm.ct, ct)))
                break
            hmms.append(hmm)
        if not hmms:
            return
        b = _Batch(b0, hmms)
        if shared is not None:
            b.names, b.descs, b.lengths = shared
        heads = (b.names, b.descs, b.lengths)
        try:
            for piece, ft, wins, plan in plan_pieces(targets, hmms, opts, 1, heads if shared is None else None):
                if targets.resident:
                    shared = heads
                items = {k: [it for it in plan if it.query == k] for k in range(len(hmms))}
                order = longest_first(items, [h.M for h in hmms], wins)
                pool.submit(Round([b0 + k for k in order], (b, piece, ft, wins, items, targets.resident), admit=(piece == 0)))
                if not targets.resident:
                    pool.barrier()                       # the piece is released next.  After a failure at query k the queries before k
        except ba.FastaFormatError as e:                 # still get their later pieces and are rendered; the jobs from k on are skipped
            pool.fail(b0, e)
        if not targets.resident:
            pool.submit(Round(range(b0, b0 + len(hmms)), (b, None, None, None, None, True)))
            pool.barrier()

    try:
        feed_batches(pool, nq, 2 * n, prepare)
    finally:
        pool.close(sys.exc_info()[1] if pool.failure is None else None)     # the coordinator itself raised: nothing queued is searched


def feed_batches(pool, nq, size, prepare):
    """prepare(b0, b1) for the batches of <size> queries one after the other, each only once every query before the previous batch
    is written: beside the batch the workers are on, one more is prepared and queued, never more, so what the coordinator holds
    (models, window tables, items) does not grow with the number of queries.  Ends at the first failure; raises it after the
    queries before it are written."""
    for b0 in range(0, nq, size):
        if not pool.wait_written(b0 - size):
            break
        prepare(b0, min(nq, b0 + size))
        if pool.failure is not None:
            break
    pool.wait()


def _rank_search(argv, opts, hmmfile, seqfile, rank, world, device, dev, chunk_bytes, block_nt, resident_bytes, laps, queryfile=None):
    """One rank's share of the search: per batch of queries and piece of the targets (plan_pieces, the same on every rank) its own
    items go through its pool of --workers contexts (one by default), a query per worker, longest first; the batch's results
    travel to the queries' owners, which render them, and rank 0 writes the texts in query order.  <hmmfile>: the model file;
    <queryfile>: the query file as given when it is another (a sequence query, whose models the parent had built)."""
    nq = ba.HMM.count(hmmfile)
    qdescs = model_descriptions(hmmfile)
    with contextlib.ExitStack() as stack:                # leaves in reverse order: the pool's threads joined, then the files closed
        out = stack.enter_context(Output(argv, opts, queryfile or hmmfile, seqfile, sys.stdout)) if rank == 0 else None
        t = time.perf_counter()
        ctxs = [new_context(device, opts) for _ in range(opts.get("--workers", 1))]
        laps["context_s"] = time.perf_counter() - t
        found = {}                                       # what the workers found in the piece at hand, per query of the batch

        def work(w, rnd, q):
            k, h, ft, wk, mine = rnd.payload[q]
            found[k] = _search_items(ctxs[w], h, ft, wk, mine, opts, block_nt, lambda: pool.cancelled(q))
        pool = WorkerPool(len(ctxs), work, start=lambda w: ctxs[w].synchronize())     # binds thread w to this rank's device
        stack.push(lambda et, exc, tb: pool.close(exc))
        targets = Targets(ctxs[0], seqfile, chunk_bytes, resident_bytes)
        src = _CodesSource(targets)
        for b0 in range(0, nq, BATCH_QUERIES):
            qs = list(range(b0, min(nq, b0 + BATCH_QUERIES)))
            t0, c0 = time.time(), os.times()
            hmms = [ba.HMM(hmmfile, q) for q in qs]
            names, descs, lengths = [], [], []
            n_items = [0] * len(qs)
            by_dest = {}
            tb = time.perf_counter()
            for piece, ft, wins, plan in plan_pieces(targets, hmms, opts, world, (names, descs, lengths)):
                ts = time.perf_counter()
                laps["ingest_s"] += ts - tb              # the piece parsed, its windows cut and planned
                mine_by = {}
                for it in plan:
                    n_items[it.query] += 1
                    if it.owner == rank:
                        mine_by.setdefault(it.query, []).append(it)
                found.clear()                            # this rank's items of the piece, a query per worker, longest first
                order = longest_first(mine_by, [h.M for h in hmms], wins)
                pool.submit(Round([qs[k] for k in order], {qs[k]: (k, hmms[k], ft, wins[k], mine_by[k]) for k in order}))
                pool.wait()                              # every worker is done with the piece before it is released
                for k in sorted(found):
                    for it, stats, geometry, stream in found[k]:
                        by_dest.setdefault(dist.query_owner(qs[k], world), bytearray()).extend(
                            _pack_item(k, piece, it.lo, stats, geometry, stream))
                laps["items"] += sum(len(m) for m in mine_by.values())
                laps["search_s"] += time.perf_counter() - ts
                tb = time.perf_counter()
            tm = time.perf_counter()
            got = dist.exchange_bytes({d: bytes(b) for d, b in by_dest.items()}, dev)
            parts = {}
            for srank in sorted(got):
                for k, piece, lo, stats, geometry, stream in _unpack_items(got[srank]):
                    parts.setdefault(k, []).append(((piece, lo), stats, geometry, stream))
            for k, q in enumerate(qs):
                owner = dist.query_owner(q, world)
                if owner == rank:
                    if len(parts.get(k, ())) != n_items[k]:
                        raise RuntimeError("query %d: %d of its %d items arrived" % (q, len(parts.get(k, ())), n_items[k]))
                    text = _render_query(q, hmms[k], qdescs[q] if q < len(qdescs) else None, parts.pop(k, []), opts, names, descs, lengths,
                                         src, t0, c0)
                    if rank != 0:
                        _send_text("%d %d\n%s%s%s" % ((len(text[0]), len(text[1])) + text), 0, dev)
                elif rank == 0:
                    msg = _recv_text(owner, dev)
                    head, rest = msg.split("\n", 1)
                    n0, n1 = (int(x) for x in head.split())
                    text = (rest[:n0], rest[n0:n0 + n1], rest[n0 + n1:])
                if rank == 0:
                    out.write_query(q, text)
            laps["merge_write_s"] += time.perf_counter() - tm
        if rank == 0:
            out.finish()
    return 0


def rank_main(argv, chunk_bytes=64 << 20, block_nt=256_000_000, resident_bytes=8 << 30, models=None):
    """One rank of a --gpus N search (a child of launch_ranks: RANK, WORLD_SIZE and the rendezvous address in its environment).
    BATH_SEARCH_SHARE_DEVICE=1: every rank on device 0; BATH_SEARCH_BACKEND: nccl (default) or gloo (collectives on CPU tensors).
    models: the model file the parent built from a sequence query (--qformat fasta); the ranks search it."""
    t_main = time.perf_counter()
    laps = dict(launch_s=0.0, context_s=0.0, ingest_s=0.0, search_s=0.0, merge_write_s=0.0, items=0)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    opts, hmmfile, seqfile = parse_args(argv)
    share = os.environ.get("BATH_SEARCH_SHARE_DEVICE") == "1"
    backend = os.environ.get("BATH_SEARCH_BACKEND") or "nccl"
    if backend not in ("nccl", "gloo"):
        sys.stderr.write("Error: BATH_SEARCH_BACKEND must be nccl or gloo\n")
        return 1
    if share and backend == "nccl":
        sys.stderr.write("Error: BATH_SEARCH_SHARE_DEVICE=1 needs BATH_SEARCH_BACKEND=gloo (RCCL does not run two ranks on one device)\n")
        return 1
    sys.stdout.flush()
    sys.stdout = os.fdopen(os.dup(1), "w")              # the main output's own stream: what libraries print to fd 1 (gloo's
    os.dup2(2, 1)                                       # connection notes) goes to stderr instead of into the output
    import torch
    import torch.distributed as tdist
    device = 0 if share else int(os.environ.get("LOCAL_RANK", rank))
    ndev = torch.cuda.device_count()
    if (not share and world > ndev) or ndev < 1:
        sys.stderr.write("Error: option --gpus %d: %d GPU(s) visible\n" % (world, ndev))
        return 1
    t = time.perf_counter()
    if backend == "nccl":
        torch.cuda.set_device(device)
        dev = torch.device("cuda", device)
        tdist.init_process_group("nccl", device_id=dev)
    else:
        dev = torch.device("cpu")
        tdist.init_process_group("gloo")
    laps["rendezvous_s"] = time.perf_counter() - t
    t_start = float(os.environ.get("BATH_SEARCH_T0", "0") or 0)
    if t_start:
        laps["launch_s"] = time.time() - t_start
    try:
        status = _rank_search(argv, opts, models or hmmfile, seqfile, rank, world, device, dev, chunk_bytes, block_nt, resident_bytes, laps,
                              queryfile=hmmfile)
    except ba.FastaFormatError as e:
        sys.stderr.write("Error: %s: %s\n" % (seqfile, e))
        status = 1
    if status == 0:
        tdist.barrier()
        tdist.destroy_process_group()
    laps["rank_main_s"] = time.perf_counter() - t_main
    if os.environ.get("BATH_SEARCH_LAPS"):                 # tools/bathsearch_multi_profile.py: every rank's phase times
        import json
        with open("%s.rank%d.json" % (os.environ["BATH_SEARCH_LAPS"], rank), "w") as fh:
            json.dump(dict(laps, rank=rank, world=world, status=status), fh)
    return status


# ---------------------------------------------------------------------------------------------------------------------------
# --qformat fasta: a protein sequence file as the query.  What p7_search_builder does with an unaligned file
# (p7_search_builder.c:97-308): one single-sequence model per record, built and calibrated by bathbuild's builder
# (bathbuild.build_models), written to --hmmout's file or to a temporary one, and searched as read back from that text
# (bathsearch.c:727-731), so the search sees the five-decimal probabilities of a model file.  The two frameshift taus are fitted
# only when --fs or --hmmout is given (p7_search_builder.c:182).
# ---------------------------------------------------------------------------------------------------------------------------

class SeqQuery:
    """A checked sequence query: its records, the score system and the options of bathbuild's builder, fs (whether the taus are fitted)."""

    def __init__(self, opts, path):
        if not os.path.isfile(path):
            raise UsageError("query file %s not found" % path)
        if ba.HMM.count(path) > 0:
            raise UsageError("query file %s is a profile HMM file: --qformat fasta asserts a protein sequence file" % path)
        try:
            self.queries = bb.read_queries(path)
        except bb.UsageError as e:
            raise UsageError(str(e))
        try:
            self.score = ba.ScoreSystem(opts.get("--mx") or "BLOSUM62", opts.get("--mxfile"), opts.get("--popen", 0.02), opts.get("--pextend", 0.4))
        except ba.BathError as e:
            raise UsageError("Failed to set single query seq score system:\n%s" % e)
        for name, _, seq in self.queries:
            if len(name.encode("latin-1")) > 127:
                raise UsageError("%s: record %s: a model's name holds at most 127 bytes" % (path, name))
            try:
                ba.strip_query(seq)
            except ba.BathError as e:
                raise UsageError("%s: record %s: %s" % (path, name, e))
        self.path, self.fs = path, "--fs" in opts or "--hmmout" in opts
        arith = opts.get("--arith", "strict")
        self.opts = {k: v[1] for k, v in bb.OPTIONS.items()}             # the builder's defaults; bathsearch's own --seed stays out
        self.opts.update({"--ct": opts.get("--ct", 1), "--w_beta": opts.get("--w_beta"), "--w_length": opts.get("--w_length"), "--seed": BUILD_SEED,
                          "--arith": arith, "--batch": BUILD_BATCH if arith == "strict" else 1})

    def build(self, path_out, device=0, calibrator=None):
        """The models' text in <path_out>, whole or not at all (a temporary name beside it, then a rename)."""
        state = ba.rng_state(BUILD_SEED)
        cal, tmp = None, path_out + ".tmp%d" % os.getpid()
        try:
            with open(tmp, "wb") as fh:
                cal = calibrator(self.opts, state) if calibrator is not None else bb.GpuCalibrator(self.opts, state, device)
                bb.build_models(self.queries, self.score, self.opts, cal, state, fh, self.path, fs=self.fs)
            os.replace(tmp, path_out)
        finally:
            if cal is not None:
                cal.close()
            if os.path.exists(tmp):
                os.remove(tmp)


BUILD_TIMEOUT_S = (600.0, 1.0)      # the build child of a --gpus search: this long, and this much more per record


def build_main(argv, path_out):
    """The build of a --gpus N search with a sequence query, in a child process of its own (the parent opens no GPU)."""
    try:
        opts, qfile, _ = parse_args(argv)
        SeqQuery(opts, qfile).build(path_out)
    except (UsageError, ba.BathError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    return 0


def build_in_child(argv, path_out, n_records):
    """build_main in one fresh child process, under a time limit; returns its exit status (1 with a message when the limit ran out)."""
    code = "import sys; from bath_amd import bathsearch as b; sys.exit(b.build_main(sys.argv[2:], sys.argv[1]))"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code, path_out] + list(argv)
    limit = BUILD_TIMEOUT_S[0] + BUILD_TIMEOUT_S[1] * n_records
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    p = subprocess.Popen(cmd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
    try:
        return 1 if p.wait(limit) else 0
    except subprocess.TimeoutExpired:
        _stop([p])
        sys.stderr.write("Error: building the models of the sequence query took more than %d s\n" % limit)
        return 1


def run(argv, stdout=None, chunk_bytes=64 << 20, block_nt=256_000_000, resident_bytes=8 << 30, device=0):
    """The whole search; returns the exit status.  chunk_bytes: FASTA bytes per upload; block_nt: nucleotides per pipeline call;
    resident_bytes: the device-memory budget for the digitised targets kept across queries.  With --workers N > 1 and no
    BATH_HIP_HOST_THREADS in the environment, the variable is set in os.environ (process-wide: the library reads it at every
    ensemble) for the time of the search and removed afterwards; a caller with threads of its own that read or set it sees that."""
    stdout = stdout or sys.stdout
    seqquery = None
    try:
        opts, hmmfile, seqfile = parse_args(argv)
        if "--qformat" in opts:
            seqquery = SeqQuery(opts, hmmfile)
        else:
            nq = ba.HMM.count(hmmfile) if os.path.exists(hmmfile) else -1
            if nq <= 0:
                raise UsageError("query file %s is not a profile HMM file; give --qformat fasta to search with sequence queries "
                                 "(alignment queries are not supported)" % hmmfile)
        if not os.path.exists(seqfile):
            raise UsageError("target file %s not found" % seqfile)
        check_target_file(seqfile)
        for q in range(0 if seqquery else nq):       # before any GPU work: P-values from an unset tau mean nothing
            if (ba.HMM(hmmfile, q).evparam[6:8] == np.float32(ba.FS_UNSET)).any():
                raise UsageError(NOT_FORMATED % hmmfile)
    except UsageError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    if seqquery is None:
        return _search(argv, opts, hmmfile, hmmfile, seqfile, nq, stdout, chunk_bytes, block_nt, resident_bytes, device)
    # a sequence query: its models into --hmmout's file, or into a temporary one that no exit path leaves behind
    keep = "--hmmout" in opts
    try:
        if keep:
            built = opts["--hmmout"]
        else:
            fd, built = tempfile.mkstemp(prefix="bathsearch_", suffix=".bhmm")
            os.close(fd)
    except OSError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    try:
        if opts.get("--gpus", 1) > 1:                # the parent opens no GPU: one child builds, and has ended before the ranks start
            if build_in_child(argv, built, len(seqquery.queries)):
                return 1
        else:
            try:
                seqquery.build(built, device)
            except (ba.BathError, OSError) as e:
                sys.stderr.write("Error: %s\n" % e)
                return 1
        return _search(argv, opts, hmmfile, built, seqfile, len(seqquery.queries), stdout, chunk_bytes, block_nt, resident_bytes, device)
    finally:
        if not keep and os.path.exists(built):
            os.remove(built)


def _search(argv, opts, queryfile, hmmfile, seqfile, nq, stdout, chunk_bytes, block_nt, resident_bytes, device):
    """The search of the <nq> models of <hmmfile>, in the run mode the options ask for; <queryfile>: the query file as given (the
    model file itself, or the sequence file the models were built from)."""
    ct = opts.get("--ct", 1)
    if opts.get("--gpus", 1) > 1:
        for q in range(nq):                      # the ranks start only on inputs the single-GPU search would not refuse
            hmm = ba.HMM(hmmfile, q)
            if hmm.ct != ct:
                if "-o" in opts:
                    with open(opts["-o"], "w") as fh:
                        fh.write(output_header(opts, queryfile, seqfile))
                else:
                    stdout.write(output_header(opts, queryfile, seqfile))
                sys.stderr.write(CT_MISMATCH % (ct, hmmfile, hmm.ct, ct))
                return 1
        run_kw = dict(chunk_bytes=chunk_bytes, block_nt=block_nt, resident_bytes=resident_bytes)
        if hmmfile != queryfile:
            run_kw["models"] = hmmfile
        return launch_ranks(opts["--gpus"], argv, stdout, run_kw)
    workers = opts.get("--workers", 1)
    threads = host_threads_per_worker(workers) if workers > 1 else None
    try:
        with Output(argv, opts, queryfile, seqfile, stdout) as out:
            if threads is not None:                  # the library reads it at every ensemble: each worker context's share
                os.environ["BATH_HIP_HOST_THREADS"] = str(threads)
            _workers_search(opts, hmmfile, seqfile, nq, out.write_query, device, chunk_bytes, block_nt, resident_bytes)
            out.finish()
    except ba.FastaFormatError as e:
        sys.stderr.write("Error: %s: %s\n" % (seqfile, e))
        return 1
    except CtMismatch as e:
        sys.stderr.write(str(e))
        return 1
    finally:
        if threads is not None:
            os.environ.pop("BATH_HIP_HOST_THREADS", None)
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
