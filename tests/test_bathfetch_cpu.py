"""CPU tier of bath_amd.bathfetch: the index it writes against the recorded one, fetches of models whose taus are kept (no GPU: the
context raises) against the blocks of the input byte for byte, the order of the output, the messages, the refusals, the table label,
and the generator walk -- calib_skip against the sampler, and which models a fetch without an index skips and which it fits."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import bath_amd as ba
import bathfetch_common as fc
import calib_common as cc
import oracle_lib as ol
from bath_amd import bathconvert as bc
from bath_amd import bathfetch as bf

BHMM = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm")
SSI = os.path.join(ol.GOLDEN, "tRNA-proteins.bhmm.ssi")
KEYS = os.path.join(ol.GOLDEN, "tRNA-synthetases-key.txt")
MET4 = os.path.join(ol.GOLDEN, "MET-ct4.bhmm")
BLOCKS = bc.split_models(open(BHMM, "rb").read().decode(bc.ENC))
NAMES = [bc.model_plan(m, None)["name"] for m in BLOCKS]
ACCS = [bf.model_acc(m) for m in BLOCKS]
INDEX_STDOUT = "Working...    done.\nIndexed 12 HMMs (12 names and 12 accessions).\nSSI index written to file tRNA-proteins.bhmm.ssi\n"


@pytest.fixture(autouse=True)
def no_gpu(monkeypatch):
    """These models keep their taus: a context would be a GPU call nothing asked for."""
    def refuse(*a, **k):
        raise AssertionError("bathfetch touched the GPU")
    monkeypatch.setattr(ba, "Context", refuse)


@pytest.fixture
def work(tmp_path, monkeypatch):
    """A directory with a copy of the 12-model BATH file, and the process in it."""
    (tmp_path / "tRNA-proteins.bhmm").write_bytes(open(BHMM, "rb").read())
    monkeypatch.chdir(tmp_path)
    return tmp_path


def fetch(argv):
    """(status, stdout) of one run in this process."""
    out = io.StringIO()
    return bf.run(argv, stdout=out), out.getvalue()


def block(i):
    return BLOCKS[i].encode(bc.ENC)


# ---- the index
def test_index_bytes_and_stdout(work, capsys):
    st, out = fetch(["--index", "tRNA-proteins.bhmm"])
    assert st == 0 and out == INDEX_STDOUT
    assert (work / "tRNA-proteins.bhmm.ssi").read_bytes() == open(SSI, "rb").read()
    st, out = fetch(["--index", "tRNA-proteins.bhmm"])                                   # a second run
    assert st == 1 and "already exists" in capsys.readouterr().err
    assert (work / "tRNA-proteins.bhmm.ssi").read_bytes() == open(SSI, "rb").read()
    assert sorted(os.listdir(work)) == ["tRNA-proteins.bhmm", "tRNA-proteins.bhmm.ssi"]


def test_index_refusals(work, capsys):
    assert fetch(["--index", "-"])[0] == 1 and "can't index <stdin>" in capsys.readouterr().err
    nameless = BLOCKS[0] + BLOCKS[1].replace("NAME  GlutR_N\n", "")
    (work / "n.bhmm").write_text(nameless, encoding=bc.ENC)
    assert fetch(["--index", "n.bhmm"])[0] == 1
    assert "Every HMM must have a name to be indexed. Failed to find name of HMM #2" in capsys.readouterr().err
    assert not (work / "n.bhmm.ssi").exists()
    (work / "plain.bhmm").write_text(BLOCKS[0].replace("ACC   PF04376.8\n", ""), encoding=bc.ENC)
    st, out = fetch(["--index", "plain.bhmm"])
    assert st == 0 and "Indexed 1 HMMs (1 names).\n" in out


# ---- fetches of models whose taus are kept
@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "index"])
def test_fetch_by_name_accession_and_key_file(work, indexed, capfd):
    if indexed:
        assert fetch(["--index", "tRNA-proteins.bhmm"])[0] == 0
    for i in (0, 7, 11):
        for key in (NAMES[i], ACCS[i]):
            st, out = fetch(["-o", "one.bhmm", "tRNA-proteins.bhmm", key])
            assert st == 0 and out == "\n\nRetrieved HMM %s.\n" % key
            assert (work / "one.bhmm").read_bytes() == block(i), (i, key)
    # a key file in another order than the file's, a name and accessions mixed, comments and a second token
    (work / "keys.txt").write_text("# three models\n%s  ignored\n\n   %s\n#%s\n%s # the first\n" % (NAMES[9], ACCS[2], NAMES[5], NAMES[0]))
    st, out = fetch(["-f", "-o", "some.bhmm", "tRNA-proteins.bhmm", "keys.txt"])
    assert st == 0 and out == "\nRetrieved 3 HMMs.\n"
    order = (9, 2, 0) if indexed else (0, 2, 9)                                          # the key file's order; the file's
    assert (work / "some.bhmm").read_bytes() == b"".join(block(i) for i in order)
    # the tutorial's key file
    assert fetch(["-f", "-o", "syn.bhmm", "tRNA-proteins.bhmm", KEYS])[0] == 0
    assert (work / "syn.bhmm").read_bytes() == block(7) + block(8) + block(9)
    # -O: the file is named after the key; nothing is said on stdout for a fetch to stdout
    st, out = fetch(["-O", "tRNA-proteins.bhmm", ACCS[3]])
    assert st == 0 and out == "\n\nRetrieved HMM %s.\n" % ACCS[3] and (work / ACCS[3]).read_bytes() == block(3)
    st, out = fetch(["tRNA-proteins.bhmm", NAMES[4]])
    assert st == 0 and out.encode(bc.ENC) == block(4)
    # an unknown key
    capfd.readouterr()
    assert fetch(["-o", "no.bhmm", "tRNA-proteins.bhmm", "PF00000.1"])[0] == 1
    err = capfd.readouterr().err
    assert err.startswith("Error: ") and "PF00000.1" in err and ("not found in SSI index" if indexed else "not found in file") in err
    (work / "k2.txt").write_text("%s\nnobody\n" % NAMES[1])
    st, out = fetch(["-f", "-o", "k2.bhmm", "tRNA-proteins.bhmm", "k2.txt"])
    if indexed:
        assert st == 1 and "nobody" in capfd.readouterr().err and not (work / "k2.bhmm").exists()
    else:                                                                                # silently absent, as in the reference
        assert st == 0 and out == "\nRetrieved 1 HMMs.\n" and (work / "k2.bhmm").read_bytes() == block(1)
    assert not [f for f in os.listdir(work) if f.startswith(".bathfetch_") or f == "no.bhmm"]


def test_stdout_of_the_command_line_is_the_block(work):
    """A child process: the bytes on its stdout are the model's, and nothing else."""
    p = subprocess.run([sys.executable, "-m", "bath_amd.bathfetch", "tRNA-proteins.bhmm", "PTH2"], cwd=str(work),
                       env=dict(os.environ, PYTHONPATH=ba._ROOT, HIP_VISIBLE_DEVICES="-1"), capture_output=True)
    assert p.returncode == 0 and p.stdout == block(2) == open(os.path.join(ol.GOLDEN, "PTH2.bhmm"), "rb").read() and p.stderr == b""


def test_refusals(work, capsys):
    def refused(argv, *words):
        before = sorted(os.listdir(work))
        assert fetch(argv)[0] == 1
        err = capsys.readouterr().err
        assert err.startswith("Error: ") and all(w in err for w in words), (argv, err)
        assert sorted(os.listdir(work)) == before                                        # nothing is left behind
    (work / "twice.txt").write_text("PTH2\nTGT\nPTH2\n")
    refused(["-f", "-o", "x.bhmm", "tRNA-proteins.bhmm", "twice.txt"], "HMM key PTH2 occurs more than once in file twice.txt")
    refused(["-f", "--index", "tRNA-proteins.bhmm"], "-f", "--index")
    refused(["-o", "x.bhmm", "-O", "tRNA-proteins.bhmm", "PTH2"], "-o", "-O")
    refused(["-O", "-f", "tRNA-proteins.bhmm", KEYS], "-O", "-f")
    refused(["-o", "x.bhmm", "--index", "tRNA-proteins.bhmm"], "-o", "--index")
    refused(["-o", "x.bhmm", "tRNA-proteins.bhmm"], "Incorrect number of command line arguments")
    refused(["-o", "x.bhmm", "absent.bhmm", "PTH2"], "absent.bhmm")
    refused(["-f", "-o", "x.bhmm", "tRNA-proteins.bhmm", "absent.txt"], "absent.txt")
    refused(["--ct", "7", "tRNA-proteins.bhmm", "PTH2"], "--ct")
    refused(["--batch", "65", "tRNA-proteins.bhmm", "PTH2"], "--batch")
    refused(["--batch", "0", "tRNA-proteins.bhmm", "PTH2"], "--batch")
    refused(["--arith", "exact", "tRNA-proteins.bhmm", "PTH2"], "--arith")
    refused(["-o", "tRNA-proteins.bhmm", "tRNA-proteins.bhmm", "PTH2"], "is the input file")
    refused(["-o", "x.bhmm", "-", "PTH2"], "standard input")
    (work / "tRNA-proteins.bhmm.ssi").write_bytes(open(SSI, "rb").read()[:300])          # a truncated index is not passed over
    refused(["-o", "x.bhmm", "tRNA-proteins.bhmm", "PTH2"], "tRNA-proteins.bhmm.ssi")


def test_options_that_change_nothing_here(work):
    """--batch and --arith are accepted and, with nothing to fit, change no byte; --ct 1 is the file's own table."""
    for extra in (["--batch", "1"], ["--batch=64"], ["--arith", "odds"], ["--ct", "1"]):
        assert fetch(extra + ["-f", "-o", "o.bhmm", "tRNA-proteins.bhmm", KEYS])[0] == 0, extra
        assert (work / "o.bhmm").read_bytes() == block(7) + block(8) + block(9), extra
    st, out = fetch(["-h"])
    assert st == 0 and "--index" in out and "--batch" in out


def test_a_model_keeps_its_own_table_label(work):
    """The stated departure from bathfetch.c:328, :453: without --ct a table-4 model is not relabelled with --ct's default 1."""
    src = open(MET4, "rb").read()
    met = bc.split_models(src.decode(bc.ENC))
    assert fetch(["-o", "metG.bhmm", MET4, "metG"])[0] == 0
    got = (work / "metG.bhmm").read_bytes()
    assert got == met[1].encode(bc.ENC) and b"\nCODON TABLE  4\n" in got
    assert fetch(["--ct", "4", "-o", "metC.bhmm", MET4, "metC"])[0] == 0                  # the model's own table: its taus stay
    assert (work / "metC.bhmm").read_bytes() == met[0].encode(bc.ENC)


def test_the_recorded_outputs_are_the_conversions_blocks():
    """tutorial/tRNA-synthetases.bhmm and tutorial/tRNA-proteins-ct11.bhmm, rebuilt from the recorded conversion and held to their
    size and SHA-256: the recorded fetch is models 8, 9 and 10 without MAXL, so the file's one generator was carried through all twelve."""
    assert fc.recorded_fetch() == ["".join(ln for ln in BLOCKS[i].splitlines(keepends=True) if not ln.startswith("MAXL ")) for i in fc.SEL]
    assert [bc.model_plan(m, None)["name"] for m in fc.recorded_fetch()] == open(KEYS).read().split()
    assert [bc.model_plan(m, None)["ct"] for m in fc.recorded_ct11()] == [11] * 12


# ---- the generator walk
@pytest.mark.parametrize("table", [1, 4, 11])
def test_calib_skip_is_two_sample_calls(table):
    after_models = ba.calib_skip(ba.calib_skip(ba.rng_state(), 2, ncbi_table=1), 2, ncbi_table=4)      # a state several sets in
    for state in (ba.rng_state(), after_models):
        for L, N in ((ba.CALIB_L, ba.CALIB_N), (10, 9)):
            s = state
            for n in range(1, 3):
                s = ba.calib_sample(s, L, N, table)[1]
                assert ba.calib_skip(state, n, L=L, N=N, ncbi_table=table) == s, (table, L, N, n)
            assert s != state
        assert ba.calib_skip(state, 0, ncbi_table=table) == state
    f = np.full(20, 0.04, np.float32)                                                      # frequencies that sum to 0.8: rolls are drawn again
    assert ba.calib_skip(ba.rng_state(), 1, 10, 9, table, f) == ba.calib_sample(ba.rng_state(), 10, 9, table, f)[1]


def test_calib_skip_refuses_what_the_sampler_refuses():
    with pytest.raises(ba.BathError, match="table 7"):
        ba.calib_skip(ba.rng_state(), 2, ncbi_table=7)
    import ctypes as C
    st = C.c_uint32(5)
    assert ba.lib().bath_calib_skip(None, None, 1, 10, 9, 2) == ba.EINVAL
    for L, N, n in ((-1, 9, 2), (10, -1, 2), (10, 9, -1)):
        assert ba.lib().bath_calib_skip(C.byref(st), None, 1, L, N, n) == ba.EINVAL and st.value == 5


def test_which_models_a_scan_skips_and_which_it_fits(tmp_path, monkeypatch):
    """The tutorial's command on the 12-model HMMER3 input, a stub in the calibrator's place: the key file names models 8, 9 and 10.
    The seven models before them are skipped; the generator is stepped over models 8 and 9 as well (their fits wait for the batch),
    so nine calib_skip calls in all; the three fits start from the states after 7, 8 and 9 models; models 11 and 12 cost nothing."""
    skips, fits = [], []
    real_skip = ba.calib_skip

    def skip(state, n_sets=2, **kw):
        assert n_sets == 2 and kw == {"ncbi_table": 1}
        skips.append(state)
        return real_skip(state, n_sets, **kw)

    class Ctx:
        def close(self):
            pass

    def fit(ctx, hmms, tables, states, **kw):
        assert isinstance(ctx, Ctx) and not kw                                             # L = 100, N = 200, tail 0.04: the defaults
        fits.append(([h.M for h in hmms], list(tables), list(states)))
        n = len(hmms)
        return np.full(n, -5.25), np.full(n, -4.5), [0] * n

    monkeypatch.setattr(ba, "calib_skip", skip)
    monkeypatch.setattr(ba, "Context", lambda device: Ctx())
    monkeypatch.setattr(ba, "calibrate_fs_batch_at", fit)
    stats = {}
    out = tmp_path / "syn.bhmm"
    assert bf.run(["-f", "-o", str(out), cc.HMM_IN, KEYS], stdout=io.StringIO(), stats=stats) == 0
    walk = [ba.rng_state()]
    for _ in range(9):
        walk.append(real_skip(walk[-1], 2, ncbi_table=1))
    assert skips == walk[:9] and stats["skipped"] == 9 and stats["fitted"] == 3
    assert fits == [([ba.HMM(cc.HMM_IN, i).M for i in (7, 8, 9)], [1, 1, 1], walk[7:10])]
    assert len(set(walk[7:10])) == 3
    got = bc.split_models(out.read_text(encoding=bc.ENC))
    assert [bc.model_plan(m, None)["name"] for m in got] == NAMES[7:10]
    assert all("STATS LOCAL FS3 FORWARD  -5.2500" in m and "STATS LOCAL FS5 FORWARD  -4.5000" in m and "MAXL" not in m for m in got)
    # --batch 2: the same states, two calls
    del skips[:], fits[:]
    assert bf.run(["--batch", "2", "-f", "-o", str(out), cc.HMM_IN, KEYS], stdout=io.StringIO()) == 0
    assert [f[2] for f in fits] == [walk[7:9], walk[9:10]] and len(skips) == 9
    # the single-key form: the same generator, so the same state for model 9; nothing after it
    del skips[:], fits[:]
    assert bf.run(["-o", str(out), cc.HMM_IN, NAMES[8]], stdout=io.StringIO()) == 0
    assert [f[2] for f in fits] == [[walk[8]]] and len(skips) == 8
    # with an index every key starts from the fresh generator and nothing is skipped
    del skips[:], fits[:]
    src = tmp_path / "in.hmm"
    src.write_bytes(open(cc.HMM_IN, "rb").read())
    assert bf.run(["--index", str(src)], stdout=io.StringIO()) == 0
    assert bf.run(["-f", "-o", str(out), str(src), KEYS], stdout=io.StringIO()) == 0
    assert [f[2] for f in fits] == [[walk[0]] * 3] and not skips
