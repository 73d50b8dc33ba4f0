"""bathsearch on one GPU: search the profile HMMs of a model file against the DNA targets of a FASTA file.

    python -m bath_amd.bathsearch [options] <hmmfile> <seqfile>

The FASTA file's bytes go to the device as they are (bath_amd.FastaTargets: records, digitising and the windows of
esl_sqio_ReadWindow are found there); per query the windows run through the pipeline in blocks of at most <block_nt>
nucleotides, and the hits are finished, sorted and printed as bathsearch.c does (main output and --tblout).

Every option the library implements is mapped; every other bathsearch option, a sequence or alignment query and a target file that
is not plain FASTA are refused (exit status 1, a message naming it).  Multi-GPU sharding is not here (bath_amd.dist has the pieces).
"""
import os
import sys
import time

import numpy as np

import bath_amd as ba
from bath_amd import dist

BANNER = ("# bathsearch :: search protein profile(s) against DNA sequence database\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
RULE = "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n\n"

# option -> kind ('flag', int, float, str)
OPTIONS = {"-o": str, "--tblout": str, "--fs": "flag", "--cigar": "flag", "--frameline": "flag", "--textw": int, "--notextw": "flag",
           "--ct": int, "-l": int, "-m": "flag", "-M": "flag", "--strand": str,
           "-E": float, "-T": float, "--incT": float, "-Z": float, "--seed": int,
           "--F1": float, "--F2": float, "--F3": float, "--F4": float, "--max": "flag", "--nobias": "flag", "--nonull2": "flag", "--fsonly": "flag",
           "--block_length": int}
# bathsearch options this driver does not implement: refused, never ignored
REFUSED = ["-h", "--splice", "--exontblout", "--fstblout", "--hmmout", "--acc", "--noali", "--notrans", "--min_intron", "--max_intron",
           "--incE", "--qformat", "--tformat", "--singlemx", "--popen", "--pextend", "--mx", "--mxfile", "--w_beta", "--w_length", "--cpu",
           "--restrictdb_stkey", "--restrictdb_n", "--ssifile", "--domZ", "--domE", "--domT", "--incdomE", "--incdomT", "--crick", "--watson",
           "--nodeinfo"]
EXCLUSIVE = [("-m", "-M"), ("--textw", "--notextw"), ("-E", "-T"), ("--max", "--F1"), ("--max", "--F2"), ("--max", "--F3"), ("--max", "--F4"),
             ("--max", "--nobias")]
REQUIRES = {"--frameline": "--fs", "--cigar": "--tblout", "--F4": "--fs"}


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
    if "--strand" in opts and opts["--strand"] not in ("plus", "minus", "both"):
        raise UsageError("option --strand: expected plus, minus or both")
    if opts.get("--textw", 150) < 120:
        raise UsageError("option --textw: n >= 120")
    if opts.get("--block_length", 50000) < 50000:
        raise UsageError("option --block_length: n >= 50000")
    if opts.get("-E", 1.0) <= 0:
        raise UsageError("option -E: x > 0")
    if opts.get("-Z", 0.0) < 0 or opts.get("--seed", 0) < 0:
        raise UsageError("option %s: must not be negative" % ("-Z" if opts.get("-Z", 0.0) < 0 else "--seed"))
    return opts, pos[0], pos[1]


def output_header(opts, hmmfile, seqfile):
    """The banner and option lines of the main output (bathsearch.c output_header)."""
    o = opts
    s = BANNER
    s += "# query HMM file:                                %s\n" % hmmfile
    s += "# target sequence database:                      %s\n" % seqfile
    s += "# codon translation table:                       %d\n" % o.get("--ct", 1)
    lines = [("-o", "# output directed to file:                       %s\n"), ("--tblout", "# per-seq hits tabular output:                   %s\n")]
    for k, f in lines:
        if k in o:
            s += f % o[k]
    if "--notextw" in o:
        s += "# max ASCII text line length:                    unlimited\n"
    if "--textw" in o:
        s += "# max ASCII text line length:                    %d\n" % o["--textw"]
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


def search_query(ctx, hmm, targets, opts, block_nt, names_out):
    """One query: (TopHits, summed PipelineStats, Pipeline, trace map, number of targets, target names, ...)."""
    fs = "--fs" in opts
    ct = opts.get("--ct", 1)
    gm = ba.Profile(hmm)
    om = ba.OProfile(ctx, gm)
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
    pipe = ba.Pipeline(ctx, om, fs_pipe=fs, ncbi_table=ct, **over)
    if fs:
        om3 = ba.FSOProfile(ctx, ba.FSProfile(hmm, 3, ncbi_table=ct))
        gm5 = ba.FSProfile(hmm, 5, ncbi_table=ct)
        om5 = ba.FSOProfile(ctx, gm5)
    else:
        gm5 = ba.FSProfile(hmm, 5, ncbi_table=ct)          # the renderer's translation of the codons
    E = opts.get("-E", 10.0)
    th = ba.TopHits()
    total = ba.PipelineStats()
    traces = {}
    names, descs, lengths = [], [], []
    nres = 0
    block_length = opts.get("--block_length", dist.BLOCK_LENGTH)
    for ft, lo, hi in targets.pieces():
        recs = ft.records()[lo:hi]
        for name, desc in ba.fasta_headers(targets.path, recs):
            names.append(name); descs.append(desc)
        lengths.extend(int(x) for x in recs["length"])
        wins = ft.windows(hmm.max_length, block_length, lo, hi)
        # blocks of at most block_nt nucleotides (a window is never cut)
        cut = [0]
        acc = 0
        for i, n in enumerate(wins["n"]):
            if acc and acc + int(n) > block_nt:
                cut.append(i); acc = 0
            acc += int(n)
        cut.append(len(wins))
        for a, b in zip(cut[:-1], cut[1:]):
            if a == b:
                continue
            w = wins[a:b]
            blk = ft.seqs(w)
            if fs:
                stats, _, dm, _ = pipe.run_frameshift_domains(om3, om5, blk, E_report=E, nres_before=nres)
            else:
                stats, dm, _ = pipe.run_hits(blk, E_report=E, nres_before=nres)
            trs = pipe.traces()
            for f, _t in ba.PipelineStats._fields_:
                setattr(total, f, getattr(total, f) + getattr(stats, f))
            nres += stats.nres
            for d, tr in zip(dm, trs):
                win = w[d.window]
                off = int(win["start0"])
                d.ienv += off; d.jenv += off; d.iali += off; d.jali += off
                d.window = int(win["target"])
                h = Hit()
                h.trace, h.target, h.start0, h.n = tr, int(win["target"]), off, int(win["n"])
                traces.setdefault(_key(d), h)
            th.add(dm, names, lengths, descs=descs) if dm else None
            del blk
    if "--incT" in opts or "-T" in opts:
        th.set_score_thresholds(by_E="-T" not in opts, T=opts.get("-T", 0.0), inc_by_E="--incT" not in opts, incT=opts.get("--incT", 0.0))
    if "-Z" in opts:
        search_nres = int(1e6 * opts["-Z"]) * (2 if opts.get("--strand", "both") == "both" else 1)
    else:
        search_nres = nres
    th.finalize(search_nres, hmm.max_length, E)
    return dict(th=th, stats=total, pipe=pipe, traces=traces, nseqs=len(names), gm=gm, gm5=gm5, names=names, nres=nres)


def _key(d):
    return (int(d.window), int(d.iali), int(d.jali), int(d.ihmm), int(d.jhmm), float(d.bitscore))


def main_output_query(hmm, desc, r, opts, targets, elapsed, cpu):
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


class _CodesSource:
    """Window codes of reported hits, from the device copy of the targets (parsed again when they were not kept resident)."""

    def __init__(self, targets):
        self.t = targets
        self._ft = None

    def codes_of(self, target, start0, n):
        if self.t.resident:
            return self.t.ft.codes(target, start0, n)
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
        return self._ft.codes(target, start0, n)


def run(argv, stdout=None, chunk_bytes=64 << 20, block_nt=256_000_000, resident_bytes=8 << 30, device=0):
    """The whole search; returns the exit status.  chunk_bytes: FASTA bytes per upload; block_nt: nucleotides per pipeline call;
    resident_bytes: the device-memory budget for the digitised targets kept across queries."""
    stdout = stdout or sys.stdout
    try:
        opts, hmmfile, seqfile = parse_args(argv)
        nq = ba.HMM.count(hmmfile) if os.path.exists(hmmfile) else -1
        if nq <= 0:
            raise UsageError("query file %s is not a profile HMM file (sequence and alignment queries are not supported)" % hmmfile)
        if not os.path.exists(seqfile):
            raise UsageError("target file %s not found" % seqfile)
        check_target_file(seqfile)
    except UsageError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    ct = opts.get("--ct", 1)
    descs = model_descriptions(hmmfile)
    ofp = open(opts["-o"], "w") if "-o" in opts else stdout
    tblfp = open(opts["--tblout"], "w") if "--tblout" in opts else None
    try:
        ofp.write(output_header(opts, hmmfile, seqfile))
        ctx = ba.Context(device)
        ctx.set_fs_strict(True)
        targets = Targets(ctx, seqfile, chunk_bytes, resident_bytes)
        src = _CodesSource(targets)
        for q in range(nq):
            hmm = ba.HMM(hmmfile, q)
            if hmm.ct != ct:
                sys.stderr.write("Error: Requested codon translation tabel ID %d does not match the codon translation tabel ID of the HMM file %s. "
                                 "Please either run bathsearch with option '--ct %d' or run bathconvert with option '--ct %d'.\n" % (ct, hmmfile, hmm.ct, ct))
                return 1
            t0, c0 = time.time(), os.times()
            r = search_query(ctx, hmm, targets, opts, block_nt, None)
            c1 = os.times()
            ofp.write(main_output_query(hmm, descs[q] if q < len(descs) else None, r, opts, src, time.time() - t0,
                                        (c1.user - c0.user, c1.system - c0.system)))
            if tblfp:
                tblfp.write(r["th"].tblout(hmm.name, hmm.acc, hmm.M, fs_pipe="--fs" in opts, show_cigar="--cigar" in opts, show_header=(q == 0)))
            ofp.flush()
        if tblfp:
            tblfp.write(tabular_tail(hmmfile, seqfile, argv))
        ofp.write("[ok]\n")
    except ba.FastaFormatError as e:
        sys.stderr.write("Error: %s: %s\n" % (seqfile, e))
        return 1
    finally:
        if ofp is not stdout:
            ofp.close()
        if tblfp:
            tblfp.close()
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
