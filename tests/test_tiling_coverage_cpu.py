"""CPU tier: the GPU tests reach every per-lane model tiling the kernels are instantiated for.

The option lists are read from the sources (fs_columns / odds_columns / BATH_CHAIN_SWITCH, columns_per_lane / BATH_C_SWITCH, the
ssv_bath_kernel dispatch, fs_wf_waves) and held against the M lists the GPU modules import: a new instantiation without a test
fails here, on any machine."""
import re

import pytest

import bath_amd as ba

CSRC = ba._ROOT + "/bath_amd/csrc/"


def src(name):
    return open(CSRC + name).read()


def body(text, start):
    """The text of the function or macro that begins at <start>, up to the next blank line."""
    i = text.index(start)
    j = text.find("\n\n", i)
    return text[i:j if j >= 0 else len(text)]


def opt_list(text, start):
    m = re.search(r"for \(int opt : \{([0-9, ]+)\}\)", body(text, start))
    assert m, start
    return [int(x) for x in m.group(1).split(",")]


def cases(text, start):
    return [int(x) for x in re.findall(r"case (\d+):", body(text, start))]


def const_nodes(name):
    m = re.search(r"constexpr int %s = 64 \* (\d+);" % name, src("bath_common.hpp"))
    assert m, name
    return 64 * int(m.group(1))


def columns(M, opts):
    return next((c for c in opts if (M + 63) // 64 <= c), None)


def lengths_per_column(opts):
    """(C, smallest M, largest M) of every instantiation."""
    out, prev = [], 0
    for c in opts:
        out.append((c, 64 * prev + 1, 64 * c))
        prev = c
    return out


def fs_options():
    fs = opt_list(src("bath_frameshift.hip"), "static int fs_columns(int M)")
    assert opt_list(src("bath_fs_odds.hip"), "static int odds_columns(int M)") == fs
    assert cases(src("bath_frameshift.hip"), "#define BATH_FS_SWITCH") == fs
    assert cases(src("bath_fs_chain.hip"), "#define BATH_CHAIN_SWITCH") == fs
    return fs


def test_frameshift_tests_reach_every_tiling_at_both_ends():
    import test_fs_tiling_gpu as t
    fs = fs_options()
    assert t.FS_COLUMNS == fs
    assert const_nodes("kFsMaxNodes") == t.FS_MAX_NODES == 64 * fs[-1]
    missing = [(c, m) for c, lo, hi in lengths_per_column(fs) for m in (lo, hi) if m not in t.FS_M]
    assert not missing, "frameshift tilings without a test at this model length: %s" % missing
    assert all(columns(m, fs) is not None for m in t.FS_M)
    # the fs5 wavefront: every forced wave count at M below and above its 64 W rows in flight
    waves = [int(x) for x in re.findall(r"forced == (\d+)", body(src("bath_fs_wavefront.hip"), "static int fs_wf_waves("))]
    assert sorted(t.WF_WAVES) == sorted(waves)
    assert any(m < 64 for m in t.WF_M) or min(t.WF_M) <= 64 * min(waves) + 1
    assert max(t.WF_M) >= 64 * max(waves) and t.FS_MAX_NODES in t.WF_M


def test_standard_filter_tests_reach_every_tiling():
    import test_filters_gpu as t
    import oracle_lib as ol
    opts = opt_list(src("bath_filters.hip"), "static int columns_per_lane(int M)")
    assert cases(src("bath_filters.hip"), "#define BATH_C_SWITCH") == opts
    assert const_nodes("kCascadeMaxNodes") == 64 * opts[-1]
    ms = set()
    for name, idx in t.MODELS:
        ms.add(int(name.split(":")[1]) if name.startswith("synthetic:") else ba.HMM(ol.GOLDEN + "/" + name, idx).M)
    reached = {columns(m, opts) for m in ms}
    assert None not in reached, "a filter test model is longer than the wave kernels take"
    assert reached == set(opts), "wave-filter tilings without a test: %s" % sorted(set(opts) - reached)


def test_cascade_and_ssv_window_tests_reach_every_tiling():
    import test_filters_gpu as tf
    import test_pipeline_gpu as tp
    pipe = src("bath_pipeline.hip")
    lists = re.findall(r"for \(int opt : \{([0-9, ]+)\}\) if \(Cc <= opt\)", pipe)
    assert len(lists) == 2 and lists[0] == lists[1]                      # the cascade's and bath_hip_ssvfilter_bath's dispatch
    ssvb = [int(x) for x in lists[0].split(",")]
    insts = sorted({int(x) for x in re.findall(r"BATH_SSVB_CASE\((\d+)\)\s", pipe)})
    assert insts == sorted(ssvb)
    assert tf.SSV_BATH_COLUMNS == ssvb
    reached = {columns(m, ssvb) for m in tf.SSV_BATH_M}
    assert reached == set(ssvb), "ssv_bath_kernel tilings without a test: %s" % sorted(set(ssvb) - reached)
    # the OProfile's own limit (bath_profile.hip: 416 nodes per lane, at most 8 lanes per target) is where the list ends
    assert re.search(r"model longer than (\d+) nodes", src("bath_profile.hip")).group(1) == str(64 * ssvb[-1]) == str(max(tf.SSV_BATH_M))
    # the cascade end to end: 6, 12 and every tiling beyond 16 nodes per lane here (the golden-model and 1024-node cascade tests
    # run the others), and the refusal just past its limit
    wave = opt_list(src("bath_filters.hip"), "static int columns_per_lane(int M)")
    assert tp.CASCADE_MAX_NODES == const_nodes("kCascadeMaxNodes") == max(tp.CASCADE_M)
    assert {columns(m, wave) for m in tp.CASCADE_M} >= {c for c in wave if c > 16 or c in (6, 12)}
