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


def test_vit_lane_tests_reach_every_instantiation():
    """vit_lane_kernel<NR> (BATH_VITL_CASE) and msv_lane_kernel<NR> (BATH_MSV_CASE): every instantiation has a test model, the Viterbi
    ones at the smallest and the largest model that selects them, and the first model beyond the kernel's range is there too."""
    import test_filters_gpu as t
    vit = src("bath_viterbi.hip")
    nrs = [int(x) for x in re.findall(r"BATH_VITL_CASE\((\d+)\)", vit)]
    assert nrs and nrs == sorted(set(nrs)) and t.VIT_LANE_NR == nrs
    assert [int(x) for x in re.findall(r"BATH_VITL_NAME\((\d+)\)", vit)] == nrs            # the names the window sweep reads back
    # the rule that picks NR for a model (bath_profile.hip), restated by t.vit_lane_nr: tied to the source's text here, and on the GPU
    # by the window sweep, which holds the name of the kernel that ran against it
    prof = src("bath_profile.hip")
    assert "int NRv = ((M + 1) / 2 + 15) / 16 * 16;" in prof
    assert "if (NRv == 80) NRv = std::max(68, ((M + 1) / 2 + 3) / 4 * 4);" in prof
    assert "if (NRv <= 112) {" in prof and max(nrs) == 112
    limit = 2 * max(nrs)
    by_nr = {}
    for m in range(1, limit + 1):
        by_nr.setdefault(t.vit_lane_nr(m), []).append(m)
    assert sorted(by_nr) == nrs, "the rule selects an NR that is not instantiated, or never selects one that is"
    missing = [(nr, m) for nr, ms in by_nr.items() for m in (ms[0], ms[-1]) if m not in t.VIT_LANE_M]
    assert not missing, "vit_lane_kernel instantiations without a test at this model length: %s" % missing
    assert t.vit_lane_nr(limit + 1) is None and limit + 1 in t.VIT_LANE_M
    assert t.VIT_LANE_WINDOWS_M == [m for m in t.VIT_LANE_M if m <= limit]
    # M <= NR (an empty high half), M = NR + 1 (one node in the high chain), an odd M (a padded last slot)
    assert any(m <= t.vit_lane_nr(m) for m in t.VIT_LANE_WINDOWS_M) and any(m == t.vit_lane_nr(m) + 1 for m in t.VIT_LANE_WINDOWS_M)
    assert any(m % 2 and m < 2 * t.vit_lane_nr(m) for m in t.VIT_LANE_WINDOWS_M)
    # msv_lane_kernel: NR is the SSV tile's -- ceil(M / 2) pairs in steps of 4, one lane per target, at most 76 pairs (152 nodes)
    import oracle_lib as ol
    msv = [int(x) for x in re.findall(r"BATH_MSV_CASE\((\d+)\)", src("bath_msv_lane.hip"))]
    assert msv and msv == sorted(set(msv)) and msv[-1] == 76
    assert "int NR = ((M + G - 1) / G + 1) / 2;" in prof and "if (G == 1 && NR <= 112) NR = (NR + 3) / 4 * 4;" in prof and "NR = std::max(NR, 16);" in prof
    assert "om->G != 1 || om->NR > 76" in src("bath_msv_lane.hip")
    ms = set(int(x) for x in re.search(r'parametrize\("M", \[([0-9, ]+)\]\)\ndef test_msv_lane_every_register_tiling', open(t.__file__).read()).group(1).split(","))
    ms |= {int(n.split(":")[1]) if n.startswith("synthetic:") else ba.HMM(ol.GOLDEN + "/" + n, i).M for n, i in t.MODELS}     # test_msv_bit_exact
    reached = {max(16, ((m + 1) // 2 + 3) // 4 * 4) for m in ms if m <= 152}
    assert reached == set(msv), "msv_lane_kernel instantiations without a test: %s" % sorted(set(msv) - reached)


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
