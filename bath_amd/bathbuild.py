"""bathbuild: single-sequence profile HMMs from an unaligned protein FASTA file, calibrated on the GPU.

    python -m bath_amd.bathbuild [options] <hmmfile_out> <seqfile_in>

What bathbuild.c does with an unaligned sequence file (serial_loop, :720-735): one model per record.  The model is p7_SingleBuilder's
(bath_amd.seq_model: a substitution matrix turned into match emissions, fixed gap transitions), named by the record's first word;
MAXL is --w_length if given, else p7_Builder_MaxLength at --w_beta (1e-7); the E-value parameters are p7_Calibrate's
(bath_amd.calibrate: the MSV and Viterbi mus, the Forward tau and the two frameshift taus from simulated sequences scored by the
GPU's filters and parsers).  With --seed other than 0 the generator is reseeded for every model, so the three standard sample
sets are the same for every model: they are drawn once and stay on the device.  With --seed 0 an arbitrary seed is chosen and the
generator runs on from model to model.  The model is written from memory (bath_amd.hmm_text), not through text.

Options: -n -o --ct --mx --mxfile --popen --pextend --seed --EmL --EmN --EvL --EvN --EfL --EfN --Eft --w_beta --w_length, and
--arith strict|odds3|odds with bathconvert's meaning (the arithmetic of the two frameshift Forward parsers; odds is the reference's).
--batch N (1..64, default 1; an extension like --arith, no header line): N models are built, calibrated in one call with the sample
sets scored against all of them in each kernel launch (bath_amd.calibrate_batch), then written in record order; at most N models are
alive at once, and the output is the bytes of --batch 1.  It needs the generator reseeded per model and the strict arithmetic:
--batch above 1 with --seed 0 or with --arith odds3|odds is refused by name.
Refused by name, status 1: an alignment (Stockholm, or FASTA with gap characters), a nucleotide file, an empty file, a degenerate
residue code in a query, a built-in matrix other than BLOSUM62, the alignment-only options and --cpu.
"""
import os
import sys
import time

import bath_amd as ba
from bath_amd.bathconvert import NCBI_TABLES, RULE, UsageError, _hms

BANNER = ("# bathbuild :: profile HMM construction from MSAs or unaligned sequences\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
USAGE = "bathbuild [-options] <hmmfile_out> <seqfile_in>"
W_BETA = 1e-7                                                                        # p7_DEFAULT_WINDOW_BETA
# option -> (type, default, range check, header line of output_header (bathbuild.c:262-316))
OPTIONS = {
    "-n": (str, None, None, "# name (the single) HMM:            %s\n"),
    "-o": (str, None, None, "# output directed to file:          %s\n"),
    "--ct": (int, 1, lambda v: v in NCBI_TABLES, None),
    "--EmL": (int, 200, lambda v: v > 0, "# seq length for MSV Gumbel mu fit: %d\n"),
    "--EmN": (int, 200, lambda v: v > 0, "# seq number for MSV Gumbel mu fit: %d\n"),
    "--EvL": (int, 200, lambda v: v > 0, "# seq length for Vit Gumbel mu fit: %d\n"),
    "--EvN": (int, 200, lambda v: v > 0, "# seq number for Vit Gumbel mu fit: %d\n"),
    "--EfL": (int, 100, lambda v: v > 0, "# seq length for Fwd exp tau fit:   %d\n"),
    "--EfN": (int, 200, lambda v: v > 0, "# seq number for Fwd exp tau fit:   %d\n"),
    "--Eft": (float, 0.04, lambda v: 0 < v < 1, "# tail mass for Fwd exp tau fit:    %f\n"),
    "--popen": (float, None, lambda v: 0 <= v < 0.5, "# gap open probability:             %f\n"),
    "--pextend": (float, None, lambda v: 0 <= v < 1, "# gap extend probability:           %f\n"),
    "--mx": (str, None, None, "# subst score matrix (built-in):    %s\n"),
    "--mxfile": (str, None, None, "# subst score matrix (file):        %s\n"),
    "--seed": (int, 42, lambda v: v >= 0, None),
    "--w_beta": (float, None, lambda v: 0 <= v <= 1, "# window length tail mass:          %g bits\n"),
    "--w_length": (int, None, lambda v: v > 0, "# window length :                   %d\n"),
    "--arith": (str, "strict", lambda v: v in ba.ARITH_MODES, None),
    "--batch": (int, 1, lambda v: 1 <= v <= ba.CALIB_BATCH_MAX, None),
}
HEADER_ORDER = ("-n", "-o", "--EmL", "--EmN", "--EvL", "--EvN", "--EfL", "--EfN", "--Eft", "--popen", "--pextend", "--mx", "--mxfile",
                "--seed", "--w_beta", "--w_length")
ALIGNMENT_ONLY = ("-O", "--fast", "--hand", "--symfrac", "--fragthresh", "--wpb", "--wgsc", "--wblosum", "--wnone", "--wgiven", "--wid",
                  "--eent", "--eentexp", "--eclust", "--enone", "--eset", "--ere", "--esigma", "--eid", "--pnone", "--plaplace",
                  "--singlemx", "--maxinsertlen", "--informat")
NUCLEOTIDE = set("ACGTUNacgtun")


def parse_options(argv):
    """(options by name with their defaults, the set of options given, hmmfile_out, seqfile_in); UsageError names what is wrong."""
    opts = {k: v[1] for k, v in OPTIONS.items()}
    used, pos, i = [], [], 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("-") and len(a) > 1:
            name, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") and "=" in a else (a, None)
            if name in ALIGNMENT_ONLY:
                raise UsageError("option %s applies to alignment input, which this bathbuild does not take: unaligned protein FASTA only" % name)
            if name == "--cpu":
                raise UsageError("option --cpu is not supported by this bathbuild: calibration runs on the GPU")
            if name == "-h":
                raise UsageError("option -h is not supported by this bathbuild: %s" % USAGE)
            if name not in OPTIONS:
                raise UsageError("unknown option %s" % name)
            if val is None:
                i += 1
                if i >= len(argv):
                    raise UsageError("option %s needs an argument" % name)
                val = argv[i]
            typ, _, ok, _ = OPTIONS[name]
            try:
                v = typ(val)
            except ValueError:
                raise UsageError("option %s: bad argument %r" % (name, val))
            if ok is not None and not ok(v):
                if name == "--ct":
                    raise UsageError("option --ct: %d is not an NCBI translation table this build knows (%s)" % (v, ", ".join(map(str, NCBI_TABLES))))
                if name == "--arith":
                    raise UsageError("option --arith: %r is not one of %s" % (v, ", ".join(ba.ARITH_MODES)))
                raise UsageError("option %s: %s is out of range" % (name, val))
            opts[name] = v
            used.append(name)
        else:
            pos.append(a)
        i += 1
    if len(pos) != 2:
        raise UsageError("Incorrect number of command line arguments: %s" % USAGE)
    if "--mx" in used and "--mxfile" in used:
        raise UsageError("options --mx and --mxfile are incompatible")
    if pos[0] == "-":
        raise UsageError("Can't write <hmmfile_out> to stdout: don't use '-'")
    if opts["--batch"] > 1:
        if opts["--seed"] == 0:
            raise UsageError("option --batch %d with --seed 0: the generator then runs on from model to model, so every model's sample "
                             "sets differ and there is nothing to share; use --batch 1 or a seed" % opts["--batch"])
        if opts["--arith"] != "strict":
            raise UsageError("option --batch %d with --arith %s: a redrawn sequence makes a model's samples depend on its scores; "
                             "use --batch 1 or --arith strict" % (opts["--batch"], opts["--arith"]))
    return opts, used, pos[0], pos[1]


def read_queries(path):
    """The records of an unaligned protein FASTA file: [(name, description, sequence text)].  Refuses, by name, what bathbuild's
    sequence mode does not take here: an empty file, a Stockholm alignment, FASTA with gap characters, a nucleotide file."""
    if not os.path.isfile(path):
        raise UsageError("Failed to open input sequence file %s for reading" % path)
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:2] == b"\x1f\x8b":
        raise UsageError("%s is compressed: unaligned protein FASTA text only" % path)
    text = data.decode("latin-1")
    if not text.strip():
        raise UsageError("Input sequence file %s is empty or misformatted" % path)
    if text.lstrip().startswith("# STOCKHOLM"):
        raise UsageError("%s is a Stockholm alignment: this bathbuild takes unaligned protein FASTA only" % path)
    if not text.lstrip().startswith(">"):
        raise UsageError("%s is not a FASTA file: this bathbuild takes unaligned protein FASTA only" % path)
    recs, head, buf = [], None, []
    for ln in text.splitlines():
        if ln.startswith(">"):
            if head is not None:
                recs.append((head, "".join(buf)))
            head, buf = ln[1:], []
        else:
            buf.append("".join(ln.split()))
    recs.append((head, "".join(buf)))
    out = []
    for head, seq in recs:
        words = head.split(None, 1)
        name = words[0] if words else ""
        if not name:
            raise UsageError("%s: a record has no name" % path)
        if any(c in seq for c in "-."):
            raise UsageError("%s: record %s holds gap characters: an aligned FASTA file is an alignment, and this bathbuild takes unaligned "
                             "protein FASTA only" % (path, name))
        if not seq:
            raise UsageError("%s: record %s holds no sequence" % (path, name))
        out.append((name, words[1].strip() if len(words) > 1 else "", seq))
    residues = "".join(s for _, _, s in out)
    if len(residues) >= 10 and sum(c in NUCLEOTIDE for c in residues) >= 0.9 * len(residues):
        raise UsageError("%s is a nucleotide file: bathbuild requires an amino acid MSA or sequence file as input" % path)
    return out


def output_header(opts, used, path_in, path_out):
    out = ["# input file:                       %s\n" % path_in, "# output HMM file:                  %s\n" % path_out]
    for name in HEADER_ORDER:
        if name not in used:
            continue
        if name == "--seed":
            out.append("# random number seed:               one-time arbitrary\n" if opts["--seed"] == 0 else
                       "# random number seed set to:        %d\n" % opts["--seed"])
        else:
            out.append(OPTIONS[name][3] % opts[name])
    return "".join(out) + RULE


def result_header():
    row = "# %-6s %-20s %5s %5s %5s %4s %8s %6s %s\n"
    return (row % ("idx", "name", "nseq", "len", "mlen", "ctbl", "eff_nseq", "re/pos", "description") +
            row % ("------", "--------------------", "-----", "-----", "-----", "----", "--------", "------", "-----------"))


def result_line(idx, name, n, M, ct, entropy, desc):
    return "  %-6d %-20s %5d %5d %5d %4d %8.2f %6.3f %s\n" % (idx, name, 1, n, M, ct, 1.0, entropy, desc)


def arbitrary_seed():
    """esl_randomness_CreateFast(0): a one-time seed from the clock and the process."""
    return (int(time.time() * 1e6) ^ (os.getpid() << 16)) % (2 ** 32 - 1) + 1


def build_model(score, name, seq, opts):
    """One record's uncalibrated model with its MAXL set.  The reference calibrates first and sets MAXL afterwards
    (p7_builder.c:534-538); the order is swapped here on purpose, so that no profile is ever configured with an unset length.
    Nothing calibration reads depends on MAXL."""
    hmm = ba.seq_model(score, seq, name, opts["--ct"])
    if opts["--w_length"] is not None:                                   # p7_builder.c:536-538
        maxl = opts["--w_length"]
    else:
        beta = W_BETA if opts["--w_beta"] is None else opts["--w_beta"]
        maxl = hmm.M * 4 if beta == 0.0 else ba.hmm_max_length(hmm, beta)
    ba.hmm_set_max_length(hmm, maxl)
    return hmm


class GpuCalibrator:
    """p7_Calibrate on one GPU context.  With a seed the three standard sample sets are drawn once and stay on the device."""

    def __init__(self, opts, state, device=0):
        self.E = {k: opts["--" + k] for k in ("EmL", "EmN", "EvL", "EvN", "EfL", "EfN")}
        self.opts, self.samples = opts, None
        self.ctx = ba.Context(device)
        if opts["--seed"]:                                               # reseeded per model: the same three sets for every model
            self.samples = ba.CalibSamples(self.ctx, state, **self.E)

    def calibrate(self, hmm, state, fs=True):
        """Stores the eight E-value parameters in the model (fs=False: the six standard ones, the two taus unset); returns the
        generator's state afterwards."""
        return ba.calibrate(self.ctx, hmm, self.opts["--ct"], state, self.samples, Eft=self.opts["--Eft"], arith=self.opts["--arith"], fs=fs, **self.E)

    def calibrate_many(self, hmms, state, fs=True):
        """calibrate of every model of a batch (--batch above 1: a seed, strict arithmetic) in one call; the state one call leaves."""
        return ba.calibrate_batch(self.ctx, hmms, self.opts["--ct"], state, self.samples, Eft=self.opts["--Eft"], fs=fs, **self.E)

    def close(self):
        if self.samples is not None:
            self.samples.close()
        self.ctx.close()


def build_models(queries, score, opts, cal, state, fh, path_in, fs=True, date=None, report=None):
    """The build loop bathbuild and bathsearch --qformat fasta share: the models of <queries> (read_queries' records) built
    (build_model), calibrated by <cal> in batches of opts["--batch"] from <state> (a seed: every model from <state>; --seed 0: the
    generator runs on), and their text written to the open binary file <fh> in record order; at most a batch's models are alive
    at once.  fs=False: the standard fits only (calibrate's fs), handed to the calibrator only then, so a calibrator without the
    argument serves every fs=True caller.  report(index from 0, record, model), when given, is called after a model is written."""
    nb, seed = opts["--batch"], opts["--seed"]
    kw = {} if fs else {"fs": False}
    for i0 in range(0, len(queries), nb):                                # --batch 1: a model at a time, call for call as without the option
        part = queries[i0:i0 + nb]
        hmms = [build_model(score, opts["-n"] or name, seq, opts) for name, _, seq in part]
        if nb == 1:
            after = cal.calibrate(hmms[0], state, **kw)
            if not seed:                                                 # p7_builder.c:131: no reseeding, the generator runs on
                state = after
        else:                                                            # a seed: every model starts from <state> (parse_options)
            try:
                if hasattr(cal, "calibrate_many"):
                    cal.calibrate_many(hmms, state, **kw)
                else:
                    for hmm in hmms:
                        cal.calibrate(hmm, state, **kw)
            except ba.BathError as e:
                raise ba.BathError("records %d to %d of %s, calibrated as one batch: %s" % (i0 + 1, i0 + len(part), path_in, e))
        for j, (hmm, rec) in enumerate(zip(hmms, part)):
            fh.write(ba.hmm_text(hmm, date=date or time.strftime("%a %b %e %H:%M:%S %Y")))
            if report is not None:
                report(i0 + j, rec, hmm)
        del hmms                                                         # at most a batch's models are alive at once


def run(argv, stdout=None, device=0, date=None, calibrator=None):
    """The whole build; returns the exit status.  calibrator: a callable (options, generator state) -> an object with
    calibrate(hmm, state) and close(), and for --batch above 1 calibrate_many(hmms, state), which calibrates every model from <state>
    (without it the batch goes through calibrate, model by model); None: GpuCalibrator on <device>."""
    t0, c0 = time.time(), os.times()
    ofh = None
    try:
        opts, used, path_out, path_in = parse_options(argv)
        queries = read_queries(path_in)
        if opts["-n"] is not None and len(queries) > 1:
            raise UsageError("option -n names one model, and %s holds %d sequences" % (path_in, len(queries)))
        try:
            score = ba.ScoreSystem(opts["--mx"] or "BLOSUM62", opts["--mxfile"], 0.02 if opts["--popen"] is None else opts["--popen"],
                                   0.4 if opts["--pextend"] is None else opts["--pextend"])
        except ba.BathError as e:
            raise UsageError("Failed to set single query seq score system:\n%s" % e)
        for name, _, seq in queries:
            try:
                ba.strip_query(seq)
            except ba.BathError as e:
                raise UsageError("%s: record %s: %s" % (path_in, name, e))
        if opts["-o"] is not None:
            ofh = open(opts["-o"], "w")
    except (UsageError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    stdout = ofh or stdout or sys.stdout
    stdout.write(BANNER + output_header(opts, used, path_in, path_out) + result_header())
    seed = opts["--seed"]
    state = ba.rng_state(seed if seed else arbitrary_seed())             # p7_builder.c:130: esl_randomness_CreateFast(seed)
    cal, fh, tmp_out = None, None, path_out + ".tmp%d" % os.getpid()
    try:
        fh = open(tmp_out, "wb")                                         # models go out one by one: a proteome's text is never held whole
        cal = calibrator(opts, state) if calibrator is not None else GpuCalibrator(opts, state, device)
        build_models(queries, score, opts, cal, state, fh, path_in, date=date, report=lambda i, rec, hmm: stdout.write(
            result_line(i + 1, opts["-n"] or rec[0], len(rec[2]), hmm.M, opts["--ct"], ba.hmm_relent(hmm), rec[1])))
        fh.close()
        os.replace(tmp_out, path_out)                                    # the output appears only when it is whole
    except (ba.BathError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        if fh is not None:
            fh.close()
        if os.path.exists(tmp_out):
            os.remove(tmp_out)
        if ofh:
            ofh.close()
        return 1
    finally:
        if cal is not None:
            cal.close()
    c1 = os.times()
    u, s = c1.user - c0.user, c1.system - c0.system
    stdout.write("\n# CPU time: %.2fu %.2fs %s Elapsed: %s\n" % (u, s, _hms(u + s), _hms(time.time() - t0)))
    if ofh:
        ofh.close()
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
