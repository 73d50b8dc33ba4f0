"""CPU tier of the odds-ratio mode (BATH_LOGSUM_ODDS): the Python constant mirrors the header's, and the switch is exported with
the signature the ABI table binds."""
import ctypes as C
import re

import bath_amd as ba


def test_logsum_odds_matches_header():
    hdr = open(ba._ROOT + "/include/bath_hip.h").read()
    m = re.search(r"#define\s+BATH_LOGSUM_ODDS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == ba.LOGSUM_ODDS == 4
    others = {int(v) for v in re.findall(r"#define\s+BATH_LOGSUM_(?:TABLE|EXACT|TABLE_SERIAL|CONTEXT)\s+(\d+)", hdr)}
    assert ba.LOGSUM_ODDS not in others


def test_set_fs_odds_is_exported():
    assert re.search(r"int\s+bath_hip_set_fs_odds\s*\(\s*bath_hip_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)", open(ba._ROOT + "/include/bath_hip.h").read())
    assert ba.ABI["bath_hip_set_fs_odds"] == (C.c_int, [C.c_void_p, C.c_int])
    fn = ba.lib().bath_hip_set_fs_odds
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    assert fn(None, 1) != 0                          # a null context is refused, not dereferenced
    assert hasattr(ba.Context, "set_fs_odds")
