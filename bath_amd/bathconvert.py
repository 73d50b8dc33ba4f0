"""bathconvert: HMMER3 or BATH model files to the BATH format bathsearch takes, the frameshift taus fitted on the GPU.

    python -m bath_amd.bathconvert [--ct N] [--arith strict|odds3|odds] [--batch N] <hmmfile_out> <hmmfile_in>

What bathconvert.c does: per model of a HMMER3/f or BATH3/f file, the codon table is --ct if given, else the file's, else 1; the
FS3 and FS5 Forward taus are fitted by simulation (bath_amd.calibrate_fs: p7_fs_Tau_3codons then p7_fs_Tau_5codons, one generator
seeded with 42 carried through the file) when the file lacks either or --ct names another table than the file's, and kept otherwise;
MAXL is computed (p7_Builder_MaxLength) only when the file has none; FRAMESHIFT PROB is 0.0100.  The output is the input's text with
the header line, MAXL, the STATS lines and the four frameshift lines rewritten (rewrite_model), every other byte kept: the model's
parameters never pass through a number.  Anything else -- older format letters, binary files, a non-amino alphabet, an output path
that is the input -- is refused by name, status 1.  One context on one device, created only if a model needs a fit.

--arith (an extension) chooses the arithmetic of the two Forward parsers a fit runs (bath_amd.ARITH_MODES): strict, the default,
today's output byte for byte; odds3, the 3-codon parser in fp32 odds ratios; odds, both parsers, which is what the reference's own
bathconvert runs (with its redraw of a sequence whose parser overflows).  A file whose taus are kept is not touched by it.

--batch N (an extension, 1..64, default 1: today's path call for call) fits up to N models with one bath_amd.calibrate_fs_batch:
the models that need a fit are collected in file order, the windows of all of them go into each parser launch, and models whose
taus are kept pass through between them.  The generator is carried in file order as always, so the output file and the summary
lines are the bytes of --batch 1; one batch of models is alive at a time.  Strict arithmetic only: with --arith odds3 or odds it
is refused by name.
"""
import os
import re
import sys
import tempfile
import time

import numpy as np

import bath_amd as ba

BANNER = ("# bathconvert :: convert HMMER or older BATH formatted HMM to current BATH format\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
RULE = "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n\n"
USAGE = "bathconvert [-options] <hmmfile_out> <hmmfile_in>"
NCBI_TABLES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 16, 21, 22, 23, 24, 25)      # the tables bath_gencode_basic knows
FSPROB = 0.01                                                                        # p7P_FSPROB
W_BETA = 1e-7                                                                        # p7_DEFAULT_WINDOW_BETA
ENC = "latin-1"                                                                      # bytes in, the same bytes out


class UsageError(Exception):
    pass


def parse_args(argv):
    """(--ct or None, hmmfile_out, hmmfile_in); raises UsageError naming what is wrong."""
    return parse_options(argv)[:3]


def parse_options(argv):
    """(--ct or None, hmmfile_out, hmmfile_in, {"arith": "strict" | "odds3" | "odds"}): what run() reads.  The dictionary has
    "batch": N only when --batch was given (absent: 1)."""
    ct, pos, i, opts = None, [], 0, {"arith": "strict"}
    while i < len(argv):
        a = argv[i]
        if a.startswith("-") and len(a) > 1:
            name, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") and "=" in a else (a, None)
            if name == "-h":
                raise UsageError("option -h is not supported by this bathconvert: %s" % USAGE)
            if name not in ("--ct", "--arith", "--batch"):
                raise UsageError("unknown option %s" % name)
            if val is None:
                i += 1
                if i >= len(argv):
                    raise UsageError("option %s needs an argument" % name)
                val = argv[i]
            if name == "--arith":
                if val not in ba.ARITH_MODES:
                    raise UsageError("option --arith: %r is not one of %s" % (val, ", ".join(ba.ARITH_MODES)))
                opts["arith"] = val
                i += 1
                continue
            if name == "--batch":
                try:
                    batch = int(val)
                except ValueError:
                    raise UsageError("option --batch: bad argument %r" % (val,))
                if not 1 <= batch <= ba.CALIB_BATCH_MAX:
                    raise UsageError("option --batch: %d is not in 1..%d" % (batch, ba.CALIB_BATCH_MAX))
                opts["batch"] = batch
                i += 1
                continue
            try:
                ct = int(val)
            except ValueError:
                raise UsageError("option --ct: bad argument %r" % (val,))
            if ct not in NCBI_TABLES:
                raise UsageError("option --ct: %d is not an NCBI translation table this build knows (%s)" % (ct, ", ".join(map(str, NCBI_TABLES))))
        else:
            pos.append(a)
        i += 1
    if opts.get("batch", 1) > 1 and opts["arith"] != "strict":
        raise UsageError("option --batch: several models per launch are fitted in strict arithmetic only, not with --arith %s "
                         "(its redraw makes a model's samples depend on the scores of the model before it)" % opts["arith"])
    if len(pos) != 2:
        raise UsageError("Incorrect number of command line arguments: %s" % USAGE)
    return ct, pos[0], pos[1], opts


def split_models(text):
    """The models of a model file's text, each up to and including its '//' line."""
    out, cur = [], []
    for line in text.splitlines(keepends=True):
        cur.append(line)
        if line.startswith("//"):
            out.append("".join(cur))
            cur = []
    if "".join(cur).strip():
        raise UsageError("the last model has no closing // line")
    return out


def check_format(data, path):
    """Refuses what is not a HMMER3/f or BATH3/f text file, by name."""
    if data[:4] in (b"\xe8\xed\xed\xb3", b"\xb3\xed\xed\xe8") or b"\0" in data[:4096] or (data[:1] and data[0] >= 0x80):
        raise UsageError("%s is a binary model file: only the HMMER3/f and BATH3/f text formats are converted" % path)
    first = data.split(b"\n", 1)[0].decode(ENC)
    m = re.match(r"(HMMER3|BATH3)/([a-z])\b", first)
    if not m:
        raise UsageError("%s is not a profile HMM file in HMMER3/f or BATH3/f format" % path)
    if m.group(2) != "f":
        raise UsageError("%s is in format %s/%s: only HMMER3/f and BATH3/f are converted" % (path, m.group(1), m.group(2)))


def model_plan(model, ct_opt, path="the input"):
    """What bathconvert.c:130-169 decides for one model's text: its name and summary fields, the table to write, whether the taus are
    to be fitted (else the file's, kept) and whether MAXL is to be computed."""
    lines = model.splitlines()
    if not re.match(r"(HMMER3|BATH3)/f\b", lines[0]):
        raise UsageError("%s: a model begins with %r: only HMMER3/f and BATH3/f are converted" % (path, lines[0][:24]))
    f = {}
    for ln in lines:
        if ln.startswith("HMM "):
            break
        tag = ln.split(None, 1)
        if not tag:
            continue
        if tag[0] == "STATS":
            t = ln.split()
            f["STATS " + " ".join(t[2:-2])] = (t[-2], t[-1])
        elif tag[0] in ("FRAMESHIFT", "CODON"):
            f[tag[0]] = ln.split()[2]
        elif tag[0] not in f:
            f[tag[0]] = tag[1].strip() if len(tag) > 1 else ""
    if f.get("ALPH", "").lower() != "amino":
        raise UsageError("Invalid alphabet type in the pHMM input file %s. Expect Amino Acid" % path)
    for s in ("STATS MSV", "STATS VITERBI", "STATS FORWARD"):
        if s not in f:
            raise UsageError("%s: model %s has no %s line: it cannot be calibrated" % (path, f.get("NAME", "?"), s.replace("STATS ", "STATS LOCAL ")))
    file_ct = int(f.get("CODON", 0))
    ct = ct_opt if ct_opt is not None else (file_ct if file_ct > 0 else 1)
    tau3 = float(f["STATS FS3 FORWARD"][0]) if "STATS FS3 FORWARD" in f else None
    tau5 = float(f["STATS FS5 FORWARD"][0]) if "STATS FS5 FORWARD" in f else None
    fit = (ct_opt is not None and ct != file_ct) or tau3 is None or tau5 is None or tau3 == ba.FS_UNSET or tau5 == ba.FS_UNSET
    return {"name": f.get("NAME", ""), "desc": f.get("DESC"), "nseq": int(f["NSEQ"]) if "NSEQ" in f else -1,
            "eff_nseq": float(f["EFFN"]) if "EFFN" in f else -1.0, "M": int(f["LENG"]), "ct": ct, "fit": fit,
            "tau3": tau3, "tau5": tau5, "need_maxl": "MAXL" not in f}


def rewrite_model(model, ct, tau3, tau5, maxl=None, add_maxl=True):
    """One model's text as p7_hmmfile_WriteASCII(fp, p7_BATH_3f, hmm) writes it after bathconvert: the header line BATH3/f, MAXL <maxl>
    after LENG when the text has none, the three STATS lines in the writer's spacing, then FS3, FS5, FRAMESHIFT PROB and CODON TABLE
    (p7_hmmfile.c:617-623; taus as the floats the model record holds).  Every other line is the input's, byte for byte.
    add_maxl=False (bathfetch, which computes no MAXL): a text without a MAXL line stays without one."""
    f32 = lambda s: float(np.float32(float(s)))
    lines = model.splitlines(keepends=True)
    has_maxl = any(ln.startswith("MAXL ") for ln in lines)
    lam, out, head = None, [], True
    for i, ln in enumerate(lines):
        eol = "\r\n" if ln.endswith("\r\n") else "\n"
        if i == 0:
            out.append("BATH3/f" + eol)
        elif not head:
            out.append(ln)
        elif ln.startswith("HMM "):
            head = False
            out.append(ln)
        elif ln.startswith("LENG ") and not has_maxl and add_maxl:
            out.append(ln)
            if maxl is None:
                raise ValueError("the model has no MAXL line and none was given")
            out.append("MAXL  %d%s" % (maxl, eol))
        elif ln.startswith("STATS LOCAL"):
            t = ln.split()
            kind = " ".join(t[2:-2])
            if kind in ("MSV", "VITERBI"):
                out.append("STATS LOCAL %-11s %8.4f %8.5f%s" % (kind, f32(t[-2]), f32(t[-1]), eol))
            elif kind == "FORWARD":
                lam = f32(t[-1])
                out.append("STATS LOCAL FORWARD     %8.4f %8.5f%s" % (f32(t[-2]), lam, eol))
                out.append("STATS LOCAL FS3 FORWARD %8.4f %8.5f%s" % (float(np.float32(tau3)), lam, eol))
                out.append("STATS LOCAL FS5 FORWARD %8.4f %8.5f%s" % (float(np.float32(tau5)), lam, eol))
                out.append("FRAMESHIFT PROB  %8.4f%s" % (float(np.float32(FSPROB)), eol))
                out.append("CODON TABLE  %d%s" % (ct, eol))
            elif kind not in ("FS3 FORWARD", "FS5 FORWARD"):
                out.append(ln)
        elif ln.startswith("FRAMESHIFT PROB") or ln.startswith("CODON TABLE"):
            pass
        else:
            out.append(ln)
    if lam is None:
        raise ValueError("the model has no STATS LOCAL FORWARD line")
    return "".join(out)


def rewrite(text, taus, maxls=None, ct_opt=None):
    """The whole file's text.  taus[i]: (tau3, tau5) for model i, or None to keep the file's (a model whose taus are to be fitted
    needs them given); maxls[i]: MAXL for a model whose text has none.  No GPU, no file."""
    out = []
    for i, model in enumerate(split_models(text)):
        p = model_plan(model, ct_opt)
        t = taus[i] if taus is not None and taus[i] is not None else None
        if t is None:
            if p["fit"]:
                raise ValueError("model %d (%s) needs fitted taus" % (i, p["name"]))
            t = (p["tau3"], p["tau5"])
        out.append(rewrite_model(model, p["ct"], t[0], t[1], maxls[i] if maxls is not None and p["need_maxl"] else None))
    return "".join(out)


def result_header():
    row = "# %-6s %-20s %5s %5s %9s %8s %6s %s\n"
    return (row % ("idx", "name", "nseq", "mlen", "codon_tbl", "eff_nseq", "re/pos", "description") +
            row % ("------", "--------------------", "-----", "-----", "---------", "--------", "------", "-----------"))


def result_line(idx, p, entropy):
    return "  %-6d %-20s %5d %5d %9d %8.2f %6.3f %s\n" % (idx, p["name"], p["nseq"], p["M"], p["ct"], p["eff_nseq"], entropy, p["desc"] or "")


def mean_match_relative_entropy(hmm):
    """p7_MeanMatchRelativeEntropy: bits per match state against the background."""
    from bath_amd import synth
    mat = synth.hmm_match_emissions(hmm)[1:].astype(np.float64)
    bg = synth.BG
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(mat > 0, mat * np.log(mat / bg), 0.0).sum(axis=1)
    return float(1.44269504 * kl.mean())


def _hms(t):
    h, r = divmod(t, 3600)
    m, s = divmod(r, 60)
    return "%02d:%02d:%05.2f" % (h, m, s)


def run(argv, stdout=None, device=0):
    """The whole conversion; returns the exit status."""
    stdout = stdout or sys.stdout
    t0, c0 = time.time(), os.times()
    try:
        ct_opt, path_out, path_in, opts = parse_options(argv)
        if not os.path.isfile(path_in):
            raise UsageError("File existence/permissions problem in trying to open HMM file %s." % path_in)
        if os.path.exists(path_out) and os.path.samefile(path_out, path_in):
            raise UsageError("the output file %s is the input file" % path_out)
        with open(path_in, "rb") as fh:
            data = fh.read()
        check_format(data, path_in)
        models = split_models(data.decode(ENC))
        if not models:
            raise UsageError("%s holds no model" % path_in)
        plans = [model_plan(m, ct_opt, path_in) for m in models]
    except UsageError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    stdout.write(BANNER)
    stdout.write("# input HMM file:                   %s\n# output HMM file:                  %s\n" % (path_in, path_out))
    stdout.write(RULE + result_header())
    ctx, state, out = None, ba.rng_state(ba.CALIB_SEED), []          # one generator per file (bathconvert.c:128)
    scratch = tempfile.TemporaryDirectory()
    one = os.path.join(scratch.name, "model.hmm")
    batch = opts.get("batch", 1)
    # --batch N > 1: the models read since the last fit, in file order -- [index, text, plan, MAXL, entropy, the model if it awaits
    # a fit].  A model whose taus are kept waits here only as text, for its place in the output.
    waiting = []

    def fit_waiting():
        nonlocal ctx, state
        fits = [w for w in waiting if w[5] is not None]
        taus = {}
        if fits:
            if ctx is None:
                ctx = ba.Context(device)
            t3, t5, state = ba.calibrate_fs_batch(ctx, [w[5] for w in fits], [w[2]["ct"] for w in fits], state)
            taus = {w[0]: (float(a), float(b)) for w, a, b in zip(fits, t3, t5)}
        for i, model, p, maxl, entropy, _ in waiting:
            tau3, tau5 = taus.get(i, (p["tau3"], p["tau5"]))
            out.append(rewrite_model(model, p["ct"], tau3, tau5, maxl))
            stdout.write(result_line(i + 1, p, entropy))
        del waiting[:]

    try:
        for i, (model, p) in enumerate(zip(models, plans)):
            with open(one, "wb") as fh:                              # the library reads model <index> of a file from the file's start:
                fh.write(model.encode(ENC))                          # one model at a time keeps a Pfam-sized file linear
            try:
                hmm = ba.HMM(one, 0)
            except ba.BathError:
                raise ba.BathError("model %d (%s) of %s cannot be read" % (i + 1, p["name"], path_in))
            if batch > 1:
                maxl = ba.hmm_max_length(hmm, W_BETA) if p["need_maxl"] else None
                waiting.append([i, model, p, maxl, mean_match_relative_entropy(hmm), hmm if p["fit"] else None])
                if sum(w[5] is not None for w in waiting) in (0, batch):     # nothing to wait for, or a full batch
                    fit_waiting()
                continue
            tau3, tau5 = p["tau3"], p["tau5"]
            if p["fit"]:
                if ctx is None:
                    ctx = ba.Context(device)
                tau3, tau5, state = ba.calibrate_fs(ctx, hmm, p["ct"], state, arith=opts["arith"])
            maxl = ba.hmm_max_length(hmm, W_BETA) if p["need_maxl"] else None
            out.append(rewrite_model(model, p["ct"], tau3, tau5, maxl))
            stdout.write(result_line(i + 1, p, mean_match_relative_entropy(hmm)))
        fit_waiting()
        with open(path_out, "wb") as fh:
            fh.write("".join(out).encode(ENC))
    except (ba.BathError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    finally:
        if ctx is not None:
            ctx.close()
        scratch.cleanup()
    c1 = os.times()
    u, s = c1.user - c0.user, c1.system - c0.system
    stdout.write("# CPU time: %.2fu %.2fs %s Elapsed: %s\n" % (u, s, _hms(u + s), _hms(time.time() - t0)))
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
