"""CPU tier of the 5-codon odds-ratio mode (bath_hip_set_fs5_odds, bath_fs5_odds.hip): the switch is exported with the signature
the ABI table binds and refuses a null context, and the GPU module's model lengths reach every per-lane tiling the new kernels are
instantiated for, at its smallest and its largest M (the rule of tests/test_tiling_coverage_cpu.py)."""
import ctypes as C
import re

import bath_amd as ba

from test_tiling_coverage_cpu import body, columns, const_nodes, fs_options, lengths_per_column, src


def test_set_fs5_odds_is_exported():
    assert re.search(r"int\s+bath_hip_set_fs5_odds\s*\(\s*bath_hip_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)", open(ba._ROOT + "/include/bath_hip.h").read())
    assert ba.ABI["bath_hip_set_fs5_odds"] == (C.c_int, [C.c_void_p, C.c_int])
    fn = ba.lib().bath_hip_set_fs5_odds
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    assert fn(None, 1) != 0 and fn(None, 0) != 0     # a null context is refused, not dereferenced
    assert callable(getattr(ba.Context, "set_fs5_odds", None)) and ba.Context.set_fs5_odds.__doc__


def test_fs5_odds_kernels_are_instantiated_for_every_tiling():
    fs_options()                       # BATH_FS_SWITCH, the one in bath_fs_device.hpp, goes over every entry of BATH_FS_COLUMNS
    text = src("bath_fs5_odds.hip")
    assert "#define" not in body(text, "int launch_fs5_odds(") and "BATH_FS_SWITCH" not in text.split("int launch_fs5_odds(")[0]
    launch = body(text, "int launch_fs5_odds(")
    assert "BATH_FS_SWITCH(Cv" in launch
    for k in ("fs5_fwd_odds_kernel<CC, false>", "fs5_fwd_odds_kernel<CC, true>", "fs5_bwd_odds_kernel<CC>"):
        assert k in launch, k


def test_fs5_odds_tests_reach_every_tiling_at_both_ends():
    import test_fs5_odds_gpu as t
    fs = fs_options()
    assert t.FS_COLUMNS == fs
    missing = [(c, m) for c, lo, hi in lengths_per_column(fs) for m in (lo, hi) if m not in t.FS_M]
    assert not missing, "5-codon odds tilings without a test at this model length: %s" % missing
    assert all(columns(m, fs) is not None for m in t.FS_M)
    assert t.FS_MAX_NODES == const_nodes("kFsMaxNodes", "BATH_FS_COLUMNS") == 64 * fs[-1]
