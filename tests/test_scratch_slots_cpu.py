"""CPU tier: a context's scratch and staging buffers are named, never numbered.

bath_slots.hpp holds the two enums (Scratch for bath_hip_ctx::scratch, Pinned for bath_hip_ctx::stage) and the array type that
takes nothing else as an index -- the compiler refuses an integer (the static_assert beside SlotArray).  What the compiler cannot
see is read here from bath_amd/csrc: comments that quote a number, enumerators no unit uses, two roles in one allocation without
the line that says what keeps them apart."""
import glob
import os
import re

import pytest

import bath_amd as ba

CSRC = ba._ROOT + "/bath_amd/csrc/"
FILES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(CSRC + "*.hip") + glob.glob(CSRC + "*.hpp") + glob.glob(CSRC + "*.cpp"))}
ENUMS = ("Scratch", "Pinned")


def enumerators(enum):
    """[(name, the enumerator it is defined equal to or None, its comment)] of <enum>, in order, kCount left out (it must be the last)."""
    m = re.search(r"enum class %s : int \{\n(.*?)\n\};" % enum, FILES["bath_slots.hpp"], re.S)
    assert m, enum
    out = []
    for line in m.group(1).split("\n"):
        line = line.strip()
        if not line or line.startswith("//"):
            continue
        q = re.fullmatch(r"(k\w+)(?:\s*=\s*(k\w+))?,?\s*(//.*)?", line)
        assert q, (enum, line)                    # one enumerator per line, equal to nothing or to another enumerator: no literal values
        out.append((q.group(1), q.group(2), q.group(3) or ""))
    assert out and out[-1][:2] == ("kCount", None) and [n for n, _, _ in out].count("kCount") == 1, enum
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names), enum
    return out[:-1]


def occurrences(pattern):
    """(file, line number, line) of every line of bath_amd/csrc that matches, code and comments alike."""
    return [(f, i + 1, line) for f, text in FILES.items() for i, line in enumerate(text.split("\n")) if re.search(pattern, line)]


def test_scratch_is_indexed_by_name_only():
    assert occurrences(r"(?:->|\.)scratch\[(?!Scratch::k\w+\])") == []
    assert len(occurrences(r"->scratch\[Scratch::")) > 50          # (the pattern still finds the sites)


def test_stage_is_indexed_by_name_only():
    # cand.stage[c] (a candidate's filter stage) and s_stage[...] (LDS) are other things: neither is reached through "->"
    assert occurrences(r"->stage\[(?!Pinned::k\w+\])") == []
    # stage_upload: an enumerator at the call, chain_batches' own Pinned parameter, or the declaration -- never a digit
    assert occurrences(r"\bstage_upload\((?!Pinned::k\w+,|stage_slot,|bath::Pinned slot,)") == []
    assert occurrences(r"\bstage_upload\(\s*\d") == []
    assert len(occurrences(r"\bPinned stage_slot\b")) == 1
    assert len(occurrences(r"->stage\[Pinned::")) > 10 and len(occurrences(r"\bstage_upload\(Pinned::")) >= 4
    assert occurrences(r"->pinned\[") == []                        # no numbered page-locked array beside it


def test_no_number_names_a_slot():
    assert occurrences(r"\b(?:scratch|stage)\[\d") == []
    assert occurrences(r"\bint stage_slot\b") == []                # chain_batches takes a Pinned


def test_arrays_are_sized_by_their_enums():
    common, slots = FILES["bath_common.hpp"], FILES["bath_slots.hpp"]
    assert len(re.findall(r"^\s*bath::SlotArray<bath::Scratch, bath::DevBuf> scratch;", common, re.M)) == 1
    assert len(re.findall(r"^\s*bath::SlotArray<bath::Pinned, bath::HostBuf> stage;", common, re.M)) == 1
    assert re.findall(r"\b(?:DevBuf|HostBuf)\s+(?:scratch|stage)\b", common) == []
    assert "B b[(int)E::kCount];" in slots and "B &operator[](E e)" in slots
    assert re.findall(r"operator\[\]\((?!E e\))", slots) == []     # one index type
    assert "static_assert(!std::is_invocable_v<decltype(&SlotArray<Scratch, int>::operator[]), SlotArray<Scratch, int> &, int>" in slots


@pytest.mark.parametrize("enum", ENUMS)
def test_every_enumerator_is_used(enum):
    used = {n for f, text in FILES.items() if f.endswith(".hip") for n in re.findall(r"\b%s::(k\w+)" % enum, text)}
    assert [n for n, _, _ in enumerators(enum) if n not in used] == []
    known = {n for n, _, _ in enumerators(enum)}
    for f, text in FILES.items():                                  # ... and every name the code uses is an enumerator (the compiler's check, restated for comments)
        for n in re.findall(r"\b%s::(k\w+)" % enum, text):
            assert n in known or (n == "kCount" and f == "bath_slots.hpp"), (f, n)


@pytest.mark.parametrize("enum", ENUMS)
def test_shared_allocations_say_why(enum):
    es = enumerators(enum)
    value, nxt = {}, 0
    for i, (name, same_as, comment) in enumerate(es):
        if same_as is None:
            value[name] = nxt
        else:
            assert same_as in value, (name, same_as)               # defined above it
            assert len(comment) > len("// ") + 20, (name, "an enumerator equal to another says what keeps the two roles apart")
            # directly behind its first role (or behind that role's other aliases): the values stay sequential
            assert value[es[i - 1][0]] == value[same_as], (name, "belongs directly behind %s" % same_as)
            value[name] = value[same_as]
        nxt = value[name] + 1
    assert sorted(set(value.values())) == list(range(nxt))          # kCount == the number of allocations: no gap, no dead slot
