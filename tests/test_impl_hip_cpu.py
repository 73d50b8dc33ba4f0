"""impl_hip/ -- the drop-in for the reference's impl_sse/ directory -- checked on the CPU tier:

* every function impl_hip.h declares has EXACTLY the prototype impl_sse.h declares (name, return type, argument types and
  names), against the digests of the reference's prototypes stored in tests/golden/impl_sse_interface.json;
* every impl_sse symbol that the bathsearch path's generic code references (p7_pipeline.c, p7_domaindef.c, bathsearch.c,
  p7_scoredata.c, p7_alidisplay.c; listed in the same file) is declared by impl_hip.h;
* impl_hip/ *.c compile warning-free against the test harness header and define every declared function (no stubs left
  undefined: the shared object exports each one)."""
import hashlib
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPL_HIP_H = os.path.join(ROOT, "impl_hip", "impl_hip.h")
# the reference's impl_sse interface, recorded from its src/impl_sse/impl_sse.h and the five files named above (see "what" inside)
IMPL_SSE = os.path.join(ROOT, "tests", "golden", "impl_sse_interface.json")


def prototypes(path):
    """name -> normalised 'extern' prototype text"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"extern\s+([^;{}]*?\))\s*;", text, flags=re.S):
        proto = re.sub(r"\s+", " ", m.group(1)).strip()
        proto = re.sub(r"\s*([(),*])\s*", r"\1", proto)
        name = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\(", proto).group(1)
        out[name] = proto
    return out


def test_declared_functions_are_defined():
    import impl_hip_build
    so = impl_hip_build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    declared = {n for n in prototypes(IMPL_HIP_H)}
    assert len(declared) >= 55
    assert declared <= defined, sorted(declared - defined)


def test_prototypes_equal_impl_sse():
    want = json.load(open(IMPL_SSE))["prototype_sha256"]
    got = prototypes(IMPL_HIP_H)
    ours = {"impl_hip_init", "impl_hip_context"}
    for name, proto in got.items():
        if name in ours:
            continue
        assert name in want, name + " is not an impl_sse function"
        assert hashlib.sha256(proto.encode()).hexdigest() == want[name], (name, proto)


def test_every_symbol_the_path_references_is_declared():
    sse = json.load(open(IMPL_SSE))
    hip = open(IMPL_HIP_H).read()
    declared = set(prototypes(IMPL_HIP_H)) | set(re.findall(r"^(p7_[A-Za-z0-9_]+|impl_Init)\(", hip, flags=re.M))
    needed = set(sse["referenced_by_path"])
    assert len(needed) >= 50
    assert needed <= declared, sorted(needed - declared)
    # ... and the four types hmmer.h embeds by name
    for t in ("P7_OPROFILE", "P7_FS_OPROFILE", "P7_OIVX", "P7_OMX"):
        assert re.search(r"}\s*" + t + r"\s*;", hip) and t in sse["typedefs"]
