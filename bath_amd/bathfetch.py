"""bathfetch: copy selected models out of a HMMER3/f or BATH3/f model file as BATH models, the frameshift taus fitted on the GPU where
the file lacks them; or index the file.

    python -m bath_amd.bathfetch [options] <hmmfile_in> <key>         (retrieves the model named <key>)
    python -m bath_amd.bathfetch [options] -f <hmmfile_in> <keyfile>  (retrieves all the models in <keyfile>)
    python -m bath_amd.bathfetch [options] --index <hmmfile_in>       (indexes <hmmfile_in>, creating <hmmfile_in>.ssi)

Options, the reference's (bathfetch.c:54-63): -h; -f; -o <f> (incompatible with -O, --index); -O: the output file is named after the
key (incompatible with -o, -f, --index); --ct <n>; --index (incompatible with -f).  Two extensions, which print no header line:
--arith strict|odds3|odds and --batch N (1..64, default 16).  <hmmfile_in> and <keyfile> are files: "-" is refused by name.

--index writes <hmmfile_in>.ssi (bath_amd.ssi): the names as primary keys, the accessions as aliases, the offset of each model's
format line, the file's name as the argument gives it.  No GPU.

A key is a name or an accession.  In a key file '#' starts a comment line, the first token of a line counts, a repeated key is an
error.  With <hmmfile_in>.ssi present every key is found by seeking and the models come out in the key file's order; a key the index
does not hold is an error.  Without an index the file is scanned once and the models come out in the file's order; with -f a key no
model has is silently absent, as in the reference; the single-key form takes the first model with that name or accession.

What is written per model is bathconvert.rewrite_model's text: the format line, the STATS lines, FRAMESHIFT PROB and CODON TABLE
rewritten, every other byte kept.  bathfetch computes no MAXL: a MAXL line of the input stays, none is added.

When a model is fitted (bathfetch.c:297-326, :422-451; L = 100, N = 200, tail 0.04, seed 42): when it lacks either tau, or when --ct is
given and differs from the model's table.  One departure: the reference then writes --ct's DEFAULT, table 1, into every fetched model,
also into a table-4 model whose taus it did not refit (bathfetch.c:328, :453); here a model keeps its own table when --ct is not given,
because a wrong label would make bathsearch translate with the wrong table without a word.

The generators are the reference's.  With an index every key starts from a fresh seed-42 generator: all fits of a run start from one
state, and one bath_amd.calibrate_fs_batch_at per --batch models shares one pair of sample sets per codon table.  Without an index
one seed-42 generator is carried through every model of the file that meets the fitting rule, in file order, in both forms (the
reference stops at the key in the single-key form; nothing written depends on what comes after).  In strict arithmetic nothing a
kernel computes feeds the generator, so a model that meets the rule but is not selected only advances it (bath_amd.calib_skip: host
code, no GPU); a selected one is noted with the state it starts from, the generator is stepped over it the same way unless it is the
last, and the noted models are fitted --batch at a time.  The GPU is not touched when no selected model needs a fit.  --batch never
changes a byte.

--arith odds3 | odds: a sequence whose parser overflows is redrawn, so the scores feed the generator.  Without an index every model
that meets the rule, up to the last selected one, is then fitted one by one with bath_amd.calibrate_fs(arith=); with an index the
selected ones are, each from the fresh state.  --batch is accepted and has no effect there.

Every input is checked before a file is written or the GPU touched; a failure leaves no partial file (the output is written under a
temporary name and renamed); refusals exit with status 1 and a message that starts "Error: ".
"""
import os
import sys
import tempfile
import time

import bath_amd as ba
from bath_amd import ssi
from bath_amd.bathconvert import ENC, NCBI_TABLES, UsageError, check_format, model_plan, rewrite_model, split_models

BANNER = ("# bathfetch :: retrieve profile HMM(s) from a file\n"
          "# BATH 2.0 (May 2026); https://github.com/TravisWheelerLab/BATH\n"
          "# Freely distributed under the BSD open source license.\n"
          "# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -\n")
USAGE = ("Usage: bathfetch [options] <hmmfile_in> <key>         (retrieves HMM named <key>)\n"
         "Usage: bathfetch [options] -f <hmmfile_in> <keyfile>  (retrieves all HMMs in <keyfile>)\n"
         "Usage: bathfetch [options] --index <hmmfile_in>       (indexes <hmmfile>)\n")
HELP = ("\nOptions:\n"
        "  -h       : help; show brief info on version and usage\n"
        "  -f       : second cmdline arg is a file of names to retrieve\n"
        "  -o <f>   : output HMM to file <f> instead of stdout\n"
        "  -O       : output HMM to file named <key>\n"
        "  --ct <n> : use alt genetic code of NCBI transl table <n>  [1]\n"
        "  --index  : index the <hmmfile>, creating <hmmfile>.ssi\n"
        "  --arith <s> : arithmetic of a fit's two Forward parsers: strict, odds3 or odds  [strict]\n"
        "  --batch <n> : fit up to <n> models per kernel launch (1..%d)  [16]\n" % ba.CALIB_BATCH_MAX)
INCOMPATIBLE = (("-f", "--index"), ("-o", "-O"), ("-o", "--index"), ("-O", "-f"), ("-O", "--index"))   # bathfetch.c:57-59
DEFAULT_BATCH = 16


def parse_options(argv):
    """{"-h", "-f", "-O", "--index": bool, "-o": path or None, "ct": N or None, "arith", "batch", "args": [...]}; raises UsageError."""
    o = {"-h": False, "-f": False, "-O": False, "--index": False, "-o": None, "ct": None, "arith": "strict", "batch": DEFAULT_BATCH, "args": []}
    i = 0
    while i < len(argv):
        a = argv[i]
        i += 1
        if not (a.startswith("-") and len(a) > 1):
            o["args"].append(a)
            continue
        name, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") and "=" in a else (a, None)
        if name in ("-h", "-f", "-O", "--index"):
            if val is not None:
                raise UsageError("option %s takes no argument" % name)
            o[name] = True
            continue
        if name not in ("-o", "--ct", "--arith", "--batch"):
            raise UsageError("unknown option %s" % name)
        if val is None:
            if i >= len(argv):
                raise UsageError("option %s needs an argument" % name)
            val = argv[i]
            i += 1
        if name == "-o":
            o["-o"] = val
        elif name == "--arith":
            if val not in ba.ARITH_MODES:
                raise UsageError("option --arith: %r is not one of %s" % (val, ", ".join(ba.ARITH_MODES)))
            o["arith"] = val
        else:
            try:
                n = int(val)
            except ValueError:
                raise UsageError("option %s: bad argument %r" % (name, val))
            if name == "--batch":
                if not 1 <= n <= ba.CALIB_BATCH_MAX:
                    raise UsageError("option --batch: %d is not in 1..%d" % (n, ba.CALIB_BATCH_MAX))
                o["batch"] = n
            else:
                if n not in NCBI_TABLES:
                    raise UsageError("option --ct: %d is not an NCBI translation table this build knows (%s)" % (n, ", ".join(map(str, NCBI_TABLES))))
                o["ct"] = n
    if o["-h"]:
        return o
    for a, b in INCOMPATIBLE:
        if (o[a] if a != "-o" else o[a] is not None) and (o[b] if b != "-o" else o[b] is not None):
            raise UsageError("Option %s is incompatible with option %s" % (a, b))
    if len(o["args"]) != (1 if o["--index"] else 2):
        raise UsageError("Incorrect number of command line arguments.")
    return o


def read_keys(path):
    """The keys of a key file in its order (esl_fileparser with '#' comments: the first token of each line that has one)."""
    keys, seen = [], set()
    with open(path, "rb") as fh:
        for ln in fh.read().decode(ENC).splitlines():
            tok = ln.split()
            if not tok or tok[0].startswith("#"):
                continue
            if tok[0] in seen:
                raise UsageError("HMM key %s occurs more than once in file %s" % (tok[0], path))
            seen.add(tok[0])
            keys.append(tok[0])
    return keys


def model_acc(model):
    """The ACC field of a model's text, or None."""
    for ln in model.splitlines():
        if ln.startswith("HMM "):
            return None
        if ln.startswith("ACC ") or ln.startswith("ACC\t"):
            return ln.split(None, 1)[1].strip() if len(ln.split(None, 1)) > 1 else None
    return None


def read_models(path):
    with open(path, "rb") as fh:
        data = fh.read()
    check_format(data, path)
    models = split_models(data.decode(ENC))
    if not models:
        raise UsageError("%s holds no model" % path)
    return models


def write_atomically(path, data):
    """<data> under <path>, or nothing: a temporary name beside it, then a rename."""
    d = os.path.dirname(path) or "."
    fd, tmp = tempfile.mkstemp(prefix=".bathfetch_", dir=d)
    try:
        with os.fdopen(fd, "wb") as fh:
            fh.write(data)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def create_index(path, stdout):
    """bathfetch.c:165-223."""
    if path == "-":
        raise UsageError("Can't use - with --index, can't index <stdin>.")
    ssifile = path + ".ssi"
    if not os.path.isfile(path):
        raise UsageError("File existence/permissions problem in trying to open HMM file %s." % path)
    if os.path.exists(ssifile):
        raise UsageError("SSI index %s already exists; delete or rename it" % ssifile)
    models = read_models(path)
    stdout.write("Working...    ")
    stdout.flush()
    primary, secondary, off = [], [], 0
    for i, m in enumerate(models):
        p = model_plan(m, None, path)
        if not p["name"]:
            raise UsageError("Every HMM must have a name to be indexed. Failed to find name of HMM #%d" % (i + 1))
        primary.append((p["name"], off))
        acc = model_acc(m)
        if acc:
            secondary.append((acc, p["name"]))
        off += len(m.encode(ENC))
    try:
        data = ssi.build(path, primary, secondary)
    except ValueError as e:
        raise UsageError("Failed to write keys to ssi file %s: %s" % (ssifile, e))
    write_atomically(ssifile, data)
    stdout.write("done.\n")
    if secondary:
        stdout.write("Indexed %d HMMs (%d names and %d accessions).\n" % (len(models), len(primary), len(secondary)))
    else:
        stdout.write("Indexed %d HMMs (%d names).\n" % (len(models), len(primary)))
    stdout.write("SSI index written to file %s\n" % ssifile)


def fetch_by_index(path, index, keys):
    """The texts of the models <keys> name, in that order, each found by seeking."""
    with open(path, "rb") as fh:
        check_format(fh.read(4096), path)
        out = []
        for key in keys:
            try:
                hit = index.find(key)
            except ssi.SSIFormatError:
                raise UsageError("Failed to parse SSI index for %s" % path)
            if hit is None:
                raise UsageError("HMM %s not found in SSI index for file %s" % (key, path))
            fh.seek(hit[1])
            lines = []
            for ln in fh:
                lines.append(ln)
                if ln.startswith(b"//"):
                    break
            else:
                raise UsageError("read failed, HMM file %s may be truncated?" % path)
            out.append(b"".join(lines).decode(ENC))
    return out


def load_hmm(model, scratch, what):
    one = os.path.join(scratch, "model.hmm")
    with open(one, "wb") as fh:
        fh.write(model.encode(ENC))
    try:
        return ba.HMM(one, 0)
    except ba.BathError:
        raise ba.BathError("%s cannot be read" % what)


def run(argv, stdout=None, device=0, stats=None):
    """The whole command; returns the exit status.  stats (a dict, or None): filled with the run's own counts and times -- "fitted",
    the models scored on the GPU; "skipped", the calib_skip calls of the generator walk; "walk_seconds"; "fit_seconds"."""
    stdout = stdout or sys.stdout
    stats = stats if stats is not None else {}
    stats.update(fitted=0, skipped=0, walk_seconds=0.0, fit_seconds=0.0)
    try:
        o = parse_options(argv)
        if o["-h"]:
            stdout.write(BANNER + USAGE + HELP)
            return 0
        if o["--index"]:
            create_index(o["args"][0], stdout)
            return 0
        # ---- every input, before a file is written or the GPU touched
        path, second = o["args"]
        if path == "-" or (o["-f"] and second == "-"):
            raise UsageError("- : reading %s from standard input is not supported" % ("<hmmfile_in>" if path == "-" else "<keyfile>"))
        if not os.path.isfile(path):
            raise UsageError("File existence/permissions problem in trying to open HMM file %s." % path)
        if o["-f"]:
            if not os.path.isfile(second):
                raise UsageError("Failed to open key file %s" % second)
            keys = read_keys(second)
        else:
            keys = [second]
        dest = second if o["-O"] else o["-o"]
        if dest is not None and os.path.exists(dest) and os.path.samefile(dest, path):
            raise UsageError("the output file %s is the input file" % dest)
        if dest is not None and not os.path.isdir(os.path.dirname(dest) or "."):
            raise UsageError("Failed to open output file %s" % dest)
        strict = o["arith"] == "strict"
        S0 = ba.rng_state(ba.CALIB_SEED)
        # ---- the selected models' texts and plans, in output order; jobs: what is to be fitted -- [position in the output or None
        # (fitted for the generator alone: odds arithmetic without an index), text, plan, state]
        jobs = []
        indexed = os.path.exists(path + ".ssi")
        if indexed:
            try:
                index = ssi.Index(path + ".ssi")
            except ssi.SSIFormatError as e:
                raise UsageError(str(e))
            texts = fetch_by_index(path, index, keys)
            plans = [model_plan(m, o["ct"], path) for m in texts]
            jobs = [[j, m, p, S0] for j, (m, p) in enumerate(zip(texts, plans)) if p["fit"]]     # bathfetch.c:420: a fresh generator per key
        else:
            models = read_models(path)
            all_plans = [model_plan(m, o["ct"], path) for m in models]
            want = set(keys)
            sel = [i for i, (m, p) in enumerate(zip(models, all_plans)) if p["name"] in want or model_acc(m) in want]
            if not o["-f"]:
                if not sel:
                    raise UsageError("HMM %s not found in file %s" % (second, path))
                sel = sel[:1]
            texts, plans = [models[i] for i in sel], [all_plans[i] for i in sel]
            # the file's one generator (bathfetch.c:295): it moves over every model that meets the rule, up to the last selected one
            last_fit = max([i for i in sel if all_plans[i]["fit"]], default=-1)
            state, pos = S0, {i: j for j, i in enumerate(sel)}
            t0 = time.time()
            for i in range(last_fit + 1):
                p = all_plans[i]
                if not p["fit"]:
                    continue
                if i in pos or not strict:
                    jobs.append([pos.get(i), models[i], p, state])
                if strict and i != last_fit:
                    state = ba.calib_skip(state, 2, ncbi_table=p["ct"])
                    stats["skipped"] += 1
            stats["walk_seconds"] = time.time() - t0
    except (UsageError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    ctx, scratch = None, tempfile.TemporaryDirectory()
    taus = {}
    try:
        t0 = time.time()
        if jobs:
            ctx = ba.Context(device)
        if strict:
            for b in range(0, len(jobs), o["batch"]):
                part = jobs[b:b + o["batch"]]
                hmms = [load_hmm(m, scratch.name, "model %s of %s" % (p["name"], path)) for _, m, p, _ in part]
                try:
                    t3, t5, _ = ba.calibrate_fs_batch_at(ctx, hmms, [p["ct"] for _, _, p, _ in part], [s for _, _, _, s in part])
                except ba.BathError as e:
                    raise ba.BathError("%s (the batch starts at model %s)" % (e, part[0][2]["name"]))
                for (j, _, _, _), a, c in zip(part, t3, t5):
                    taus[j] = (float(a), float(c))
                stats["fitted"] += len(part)
        else:
            state = S0
            for j, m, p, _ in jobs:                                   # with an index every fit from the fresh state; without, one carried
                hmm = load_hmm(m, scratch.name, "model %s of %s" % (p["name"], path))
                a, c, state = ba.calibrate_fs(ctx, hmm, p["ct"], S0 if indexed else state, arith=o["arith"])
                if j is not None:
                    taus[j] = (float(a), float(c))
                stats["fitted"] += 1
        stats["fit_seconds"] = time.time() - t0
        out = []
        for j, (m, p) in enumerate(zip(texts, plans)):
            tau3, tau5 = taus.get(j, (p["tau3"], p["tau5"]))
            out.append(rewrite_model(m, p["ct"], tau3, tau5, add_maxl=False))
        data = "".join(out).encode(ENC)
        if dest is None:
            if hasattr(stdout, "buffer"):                             # the input's bytes, whatever the stream's encoding
                stdout.flush()
                stdout.buffer.write(data)
            else:
                stdout.write("".join(out))
        else:
            write_atomically(dest, data)
    except (ba.BathError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    finally:
        if ctx is not None:
            ctx.close()
        scratch.cleanup()
    if dest is not None:
        stdout.write("\nRetrieved %d HMMs.\n" % len(texts) if o["-f"] else "\n\nRetrieved HMM %s.\n" % second)
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
