"""CPU tier: the GPU tests reach every per-lane model tiling the kernels are instantiated for.

Every family's list of instantiations is read from its one definition in bath_tilings.hpp (BATH_FS_COLUMNS, BATH_WAVE_COLUMNS,
BATH_SSVB_COLUMNS, BATH_VIT_LANE_NR, BATH_MSV_LANE_NR; the wavefront's wave counts from fs_wf_waves) and held against the M lists
the GPU modules import: a new instantiation without a test fails here, on any machine.  The launchers take their pick, dispatch
and limits from the same definitions, and no copy of a list is left beside them."""
import glob
import os
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


def csrc_files():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(CSRC + "*.hip") + glob.glob(CSRC + "*.hpp") + glob.glob(CSRC + "*.cpp"))}


def tiling(name):
    """The entries of the list <name>, from its definition: there is one in bath_amd/csrc, in bath_tilings.hpp."""
    defs = [f for f, text in csrc_files().items() for _ in re.finditer(r"#\s*define\s+%s\b" % name, text)]
    assert defs == ["bath_tilings.hpp"], (name, defs)
    m = re.search(r"#define %s\(X, \.\.\.\)((?:[^\n]*\\\n)*[^\n]*)\n" % name, src("bath_tilings.hpp"))
    assert m, name
    out = [int(x) for x in re.findall(r"X\((\d+), __VA_ARGS__\)", m.group(1))]
    assert out and out == sorted(set(out)) and len(out) == m.group(1).count("X("), name      # ascending: the pick takes the first that fits
    return out


def const_nodes(name, lst):
    """The limit <name> of bath_common.hpp: 64 nodes per lane times the last entry of <lst>, computed from the list."""
    assert "constexpr int %s = 64 * BATH_TILING_MAX(%s);" % (name, lst) in src("bath_common.hpp"), name
    return 64 * tiling(lst)[-1]


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
    """BATH_FS_COLUMNS, and that every frameshift launcher picks from it and dispatches over it."""
    fs = tiling("BATH_FS_COLUMNS")
    files = csrc_files()
    assert [f for f, text in files.items() if "#define BATH_FS_SWITCH" in text] == ["bath_fs_device.hpp"]
    assert "BATH_TILING_SWITCH(BATH_FS_COLUMNS, Cv," in body(files["bath_fs_device.hpp"], "#define BATH_FS_SWITCH")
    assert "#define BATH_TILING_CASE(N, ...) case N: { constexpr int CC = N; __VA_ARGS__ } break;" in files["bath_tilings.hpp"]
    for f in ("bath_frameshift.hip", "bath_fs_envelopes.hip", "bath_fs_chain.hip", "bath_fs_odds.hip", "bath_fs5_odds.hip"):
        assert "BATH_FS_SWITCH(" in files[f], f
    for f in ("bath_frameshift.hip", "bath_fs_odds.hip"):
        assert "BATH_TILING_PICK(BATH_FS_COLUMNS, " in files[f], f
    return fs


def sequence(entries):
    return r"(?<![\w.])" + r"\D{1,24}".join(str(x) for x in entries) + r"(?!\d)"


def test_every_tiling_list_is_stated_once():
    """What held the hand-written copies equal before: there are none.  Outside bath_tilings.hpp no source has a literal option loop,
    a case ladder on CC or the leading entries of a list in sequence; inside it each list stands once."""
    lists = {n: tiling(n) for n in ("BATH_FS_COLUMNS", "BATH_WAVE_COLUMNS", "BATH_SSVB_COLUMNS", "BATH_VIT_LANE_NR", "BATH_MSV_LANE_NR")}
    files = csrc_files()
    til = files.pop("bath_tilings.hpp")
    for f, text in files.items():
        assert "for (int opt : {" not in text, f
        assert not re.search(r"case \d+:\s*\{\s*constexpr int CC", text), f
        for n, l in lists.items():
            assert not re.search(sequence(l[:6]), text), "%s: a copy of %s" % (f, n)
    assert "for (int opt : {" not in til
    for n, l in lists.items():
        assert len(re.findall(sequence(l[:6]), til)) == sum(o[:6] == l[:6] for o in lists.values()), n


def test_frameshift_tests_reach_every_tiling_at_both_ends():
    import test_fs_tiling_gpu as t
    fs = fs_options()
    assert t.FS_COLUMNS == fs
    assert const_nodes("kFsMaxNodes", "BATH_FS_COLUMNS") == t.FS_MAX_NODES == 64 * fs[-1]
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
    opts = tiling("BATH_WAVE_COLUMNS")
    filt = src("bath_filters.hip")
    assert "BATH_TILING_SWITCH(BATH_WAVE_COLUMNS, C," in body(filt, "#define BATH_C_SWITCH") and "BATH_TILING_PICK(BATH_WAVE_COLUMNS, om->M)" in filt
    assert const_nodes("kCascadeMaxNodes", "BATH_WAVE_COLUMNS") == 64 * opts[-1]
    ms = set()
    for name, idx in t.MODELS:
        ms.add(int(name.split(":")[1]) if name.startswith("synthetic:") else ba.HMM(ol.GOLDEN + "/" + name, idx).M)
    reached = {columns(m, opts) for m in ms}
    assert None not in reached, "a filter test model is longer than the wave kernels take"
    assert reached == set(opts), "wave-filter tilings without a test: %s" % sorted(set(opts) - reached)


def test_vit_lane_tests_reach_every_instantiation():
    """vit_lane_kernel<NR> (BATH_VIT_LANE_NR) and msv_lane_kernel<NR> (BATH_MSV_LANE_NR): every instantiation has a test model, the Viterbi
    ones at the smallest and the largest model that selects them, and the first model beyond the kernel's range is there too."""
    import test_filters_gpu as t
    vit = src("bath_viterbi.hip")
    nrs = tiling("BATH_VIT_LANE_NR")
    assert t.VIT_LANE_NR == nrs
    assert "BATH_VIT_LANE_NR(BATH_VITL_CASE)" in body(vit, "int launch_vit_lane(")
    assert "BATH_VIT_LANE_NR(BATH_VITL_NAME)" in body(vit, "const char *vit_lane_kernel_name(")       # the names the window sweep reads back
    # the rule that picks NR for a model (bath_profile.hip), restated by t.vit_lane_nr: tied to the source's text here, and on the GPU
    # by the window sweep, which holds the name of the kernel that ran against it
    prof = src("bath_profile.hip")
    assert "int NRv = ((M + 1) / 2 + 15) / 16 * 16;" in prof
    assert "if (NRv == 80) NRv = std::max(68, ((M + 1) / 2 + 3) / 4 * 4);" in prof
    assert "if (NRv <= BATH_TILING_MAX(BATH_VIT_LANE_NR)) {" in prof and max(nrs) == 112
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
    msv = tiling("BATH_MSV_LANE_NR")
    assert msv[-1] == 76
    assert "BATH_MSV_LANE_NR(BATH_MSV_CASE)" in body(src("bath_msv_lane.hip"), "int launch_msv_lane(")
    assert "BATH_MSV_LANE_NR(BATH_MSV_STAGE_CASE)" in src("bath_pipeline.hip")          # the cascade's msv_stage_kernel<NR>
    assert "int NR = ((M + G - 1) / G + 1) / 2;" in prof and "if (G == 1 && NR <= 112) NR = (NR + 3) / 4 * 4;" in prof and "NR = std::max(NR, 16);" in prof
    assert "om->G != 1 || om->NR > BATH_TILING_MAX(BATH_MSV_LANE_NR)" in src("bath_msv_lane.hip")
    ms = set(int(x) for x in re.search(r'parametrize\("M", \[([0-9, ]+)\]\)\ndef test_msv_lane_every_register_tiling', open(t.__file__).read()).group(1).split(","))
    ms |= {int(n.split(":")[1]) if n.startswith("synthetic:") else ba.HMM(ol.GOLDEN + "/" + n, i).M for n, i in t.MODELS}     # test_msv_bit_exact
    reached = {max(16, ((m + 1) // 2 + 3) // 4 * 4) for m in ms if m <= 152}
    assert reached == set(msv), "msv_lane_kernel instantiations without a test: %s" % sorted(set(msv) - reached)


def test_cascade_and_ssv_window_tests_reach_every_tiling():
    import test_filters_gpu as tf
    import test_pipeline_gpu as tp
    pipe = src("bath_pipeline.hip")
    ssvb = tiling("BATH_SSVB_COLUMNS")
    # one launcher, which picks from the list and dispatches over it, for the cascade and for bath_hip_ssvfilter_bath
    launch = body(pipe[pipe.rindex("static int launch_ssv_bath("):], "static int launch_ssv_bath(")
    assert "BATH_TILING_SWITCH(BATH_SSVB_COLUMNS, BATH_TILING_PICK(BATH_SSVB_COLUMNS, om->M)," in launch and "ssv_bath_kernel<CC>" in launch
    assert len(re.findall(r"ssv_bath_kernel<", pipe)) == 1 and len(re.findall(r"[ (]launch_ssv_bath\(ctx, ", pipe)) == 2
    assert tf.SSV_BATH_COLUMNS == ssvb
    reached = {columns(m, ssvb) for m in tf.SSV_BATH_M}
    assert reached == set(ssvb), "ssv_bath_kernel tilings without a test: %s" % sorted(set(ssvb) - reached)
    # the OProfile's own limit (bath_profile.hip: 416 nodes per lane, at most 8 lanes per target) is where the list ends
    assert re.search(r"model longer than (\d+) nodes", src("bath_profile.hip")).group(1) == str(64 * ssvb[-1]) == str(max(tf.SSV_BATH_M))
    # the cascade end to end: 6, 12 and every tiling beyond 16 nodes per lane here (the golden-model and 1024-node cascade tests
    # run the others), and the refusal just past its limit
    wave = tiling("BATH_WAVE_COLUMNS")
    assert tp.CASCADE_MAX_NODES == const_nodes("kCascadeMaxNodes", "BATH_WAVE_COLUMNS") == max(tp.CASCADE_M)
    assert {columns(m, wave) for m in tp.CASCADE_M} >= {c for c in wave if c > 16 or c in (6, 12)}


def test_std_envelope_tests_reach_every_instantiation():
    """std_envelope_fill_kernel<C> and std_envelope_fill_mw_kernel<C> (bath_std_domains.hip): the instantiations are those of the two
    ladders in std_launch_fill, which the domain stage and bath_hip_std_envelopes_fill both call; test_std_tiling_gpu holds the
    smallest and the largest model of each, and its pipeline test the first model past them and the cascade's last."""
    import test_std_tiling_gpu as t
    dom = src("bath_std_domains.hip")
    helper = body(dom, "static int std_launch_fill(")
    fill = [int(x) for x in re.findall(r"\{ BATH_FILL\((\d+)\); \}", helper)]
    mw = [int(x) for x in re.findall(r"\{ BATH_FILL_MW\((\d+)\); \}", helper)]
    assert fill == t.STD_FILL_COLUMNS and mw == t.STD_FILL_MW_COLUMNS
    # one ladder each, in the helper and nowhere else; every launch of a fill kernel is the helper's macro
    assert len(re.findall(r"BATH_FILL\(\d+\)", dom)) == len(fill) and len(re.findall(r"BATH_FILL_MW\(\d+\)", dom)) == len(mw)
    assert dom.count("#define BATH_FILL(CC)") == 1 and dom.count("#define BATH_FILL_MW(CC)") == 1 and dom.count("static int std_launch_fill(") == 1
    assert len(re.findall(r"std_envelope_fill_kernel<[^C]", dom)) == 0 and len(re.findall(r"std_envelope_fill_mw_kernel<[^C]", dom)) == 0
    assert dom.count("(std_envelope_fill_kernel<CC>,") == 1 and dom.count("(std_envelope_fill_mw_kernel<CC>,") == 1
    assert len(re.findall(r"[ (]std_launch_fill\(ctx, M, fill, ", dom)) == 2                   # std_domains and the stage-level entry
    for f, text in csrc_files().items():
        assert f == "bath_std_domains.hip" or ("BATH_FILL" not in text and "std_envelope_fill" not in text), f
    # the pick: ceil(M / 64) nodes per lane takes the first entry that fits; the block kernel ceil(M / 256); its last entry has no test
    assert "const int c = (M + 63) / 64;" in helper and "const int c4 = (M + 255) / 256;" in helper
    for c in fill[:-1]:
        assert "(c <= %d) { BATH_FILL(%d); }" % (c, c) in helper
    for c in mw[:-1]:
        assert "(c4 <= %d) { BATH_FILL_MW(%d); }" % (c, c) in helper
    assert "else { BATH_FILL(%d); }" % fill[-1] in helper and "else { BATH_FILL_MW(%d); }" % mw[-1] in helper
    assert "if (M > 1024 ||" in helper and 64 * fill[-1] == 256 * mw[-1] == 1024 == t.STD_FILL_MAX_NODES
    # std_domains' default: a fill kernel up to 1024 nodes, the block kernel from 4 nodes per lane on
    choice = body(dom, "static int std_fill_choice(")
    assert "!(M <= 1024)) return 0;" in choice and "const int c = (M + 63) / 64;" in choice and "c >= 4) ? 2 : 1;" in choice
    assert 'std::getenv("BATH_HIP_STD_SERIAL")' in choice and 'std::getenv("BATH_HIP_STD_FILL_MW")' in choice
    assert "const int fill = std_fill_choice(M);" in dom
    missing = [(c, m) for c, lo, hi in lengths_per_column(fill) for m in (lo, hi) if m not in t.STD_M]
    assert not missing, "std_envelope_fill_kernel instantiations without a test at this model length: %s" % missing
    prev = 0
    for c in mw:
        assert 256 * prev + 1 in t.STD_M and 256 * c in t.STD_M, "std_envelope_fill_mw_kernel<%d> without a test at both ends" % c
        prev = c
    assert all(columns(m, fill) is not None for m in t.STD_M) and max(t.STD_M) == 1024
    # the default takes the block kernel from 193 nodes on: both sides of that are there
    assert 192 in t.STD_M and 193 in t.STD_M
    assert 1025 in t.PIPELINE_M and const_nodes("kCascadeMaxNodes", "BATH_WAVE_COLUMNS") in t.PIPELINE_M
    assert all(m <= 1024 and v == ["0"] for m, v in t.PIPELINE_M.items() if v) and {columns(m, fill) for m, v in t.PIPELINE_M.items() if v} == {4, 12}


def ssv_shapes():
    """The (NR, G) entries of BATH_SSV_SHAPES, from its one definition: X(NR, G), a list of pairs with a parser of its own."""
    defs = [f for f, text in csrc_files().items() for _ in re.finditer(r"#\s*define\s+BATH_SSV_SHAPES\b", text)]
    assert defs == ["bath_tilings.hpp"], defs
    m = re.search(r"#define BATH_SSV_SHAPES\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", src("bath_tilings.hpp"))
    assert m
    out = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", m.group(1))]
    assert out and len(out) == len(set(out)) == m.group(1).count("X(")
    return out


def test_ssv_tests_reach_every_shape():
    """ssv_lane_kernel<NR, G> (bath_filters.hip) and ssv_orf_kernel<NR, G> (bath_pipeline.hip): both launchers expand BATH_SSV_SHAPES and
    nothing else instantiates the kernels; the rule of bath_profile.hip selects listed shapes
    only and every listed shape for some model; every shape's cost table fits a workgroup's LDS; test_ssv_shapes_gpu runs every
    shape at the smallest and the largest model that selects it.  The cascade stops at 2048 nodes, so (144, 8) and (160, 8), 2049 to
    2560 nodes, are reached by the standalone filters alone: test_ssv_standalone_every_shape runs them."""
    import test_ssv_shapes_gpu as t
    shapes = ssv_shapes()
    table_bytes = lambda nr, g: 30 * 16 * ((nr * g // 4 + 1) | 1)
    too_big = [s for s in shapes if table_bytes(*s) > 160 * 1024]
    assert not too_big, "SSV shapes whose cost table exceeds a workgroup's 160 KB of LDS (they can never launch): %s" % too_big
    assert t.SSV_SHAPES == shapes
    files = csrc_files()
    filt, pipe, prof = files["bath_filters.hip"], files["bath_pipeline.hip"], files["bath_profile.hip"]
    assert "BATH_SSV_SHAPES(BATH_SSV_CASE)" in body(filt, "int launch_ssv_lane(") and "BATH_SSV_SHAPES(BATH_ORF_CASE)" in pipe
    for f, text in files.items():
        assert len(re.findall(r"\bBATH_SSV_SHAPES\(", text)) == {"bath_tilings.hpp": 1, "bath_filters.hip": 1, "bath_pipeline.hip": 1}.get(f, 0), f
        for kernel, home in (("ssv_lane_kernel", "bath_filters.hip"), ("ssv_orf_kernel", "bath_pipeline.hip")):
            inst = re.findall(kernel + r"<([^>]*)>", text)
            assert inst == (["N, GG"] * 2 if f == home else []), (f, kernel, inst)
    # the rule, tied to the source's text
    for line in ("int G = (M > 152 && M <= 304) ? 2 : 1;",
                 "while (G < 8 && M > 416 * G) G *= 2;",
                 'if (M > 416 * G) { ctx->set_error("model longer than 3328 nodes"); delete om; return BATH_EINVAL; }',
                 "int NR = ((M + G - 1) / G + 1) / 2;",
                 "if (G == 1 && NR <= 112) NR = (NR + 3) / 4 * 4;",
                 "else if (G == 2 && NR <= 76) NR = NR <= 40 ? 40 : (NR <= 72 ? (NR + 7) / 8 * 8 : 76);",
                 "else NR = std::max((NR + 15) / 16 * 16, G > 1 ? 112 : 16);",
                 "NR = std::max(NR, 16);",
                 "om->ssv_row_bytes = 16 * ((NR * G / 4 + 1) | 1);"):
        assert line in prof, line
    assert t.OPROFILE_MAX_NODES == 3328 == 416 * 8
    # the table's limit, stated once and used by both entry points before they launch
    common_hpp = files["bath_common.hpp"]
    assert "constexpr int kSsvRows = 30;" in common_hpp and "constexpr size_t kSsvLdsMax = 160 * 1024;" in common_hpp
    assert "constexpr int kSsvMaxNodes = %d;" % t.SSV_MAX_NODES in common_hpp
    fits = body(filt, "int ssv_table_fits(")
    assert "if ((size_t)kSsvRows * om->ssv_row_bytes <= kSsvLdsMax) return BATH_OK;" in fits and '"%s' % t.LDS_MESSAGE in fits
    assert "ssv_table_fits(ctx, om)" in body(filt, "int launch_ssv_lane(").split("hipLaunchKernelGGL")[0]
    assert pipe.index("ssv_table_fits(ctx, om)") < pipe.index("BATH_SSV_SHAPES(BATH_ORF_CASE)") and sum(text.count(t.LDS_MESSAGE) for text in files.values()) == 1
    # what the rule selects
    by_shape = {}
    for m in range(1, t.OPROFILE_MAX_NODES + 1):
        s = t.ssv_shape(m)
        if table_bytes(*s) <= 160 * 1024:
            by_shape.setdefault(s, []).append(m)
        else:
            assert m > t.SSV_MAX_NODES and s not in shapes           # refused by ssv_table_fits; ssv_bath_kernel<52> alone takes them
    assert t.ssv_shape(t.SSV_MAX_NODES) in shapes and max(m for ms in by_shape.values() for m in ms) == t.SSV_MAX_NODES
    selected = set(by_shape)
    assert not selected - set(shapes), "the rule selects shapes that are not instantiated: %s" % sorted(selected - set(shapes))
    assert not set(shapes) - selected, "instantiated shapes that no model selects: %s" % sorted(set(shapes) - selected)
    for s in shapes:
        assert s in t.SSV_M, "SSV shape %s has no entry in test_ssv_shapes_gpu.SSV_M: no test runs it" % (s,)
        lo, hi = t.SSV_M[s]
        ms = by_shape[s]
        assert (lo, hi) == (ms[0], ms[-1]), "SSV shape %s: the tests' models %d, %d are not its smallest and largest, %d, %d" % (s, lo, hi, ms[0], ms[-1])
    assert set(t.SSV_M) == set(shapes) and len(shapes) == 44
    # every entry is a test case, and the cascade leg leaves out only what lies beyond its limit
    assert {(m, nr, g) for (nr, g), (lo, hi) in t.SSV_M.items() for m in (lo, hi)} == set(t.DEFAULT_CASES)
    assert {c[1:] for c in t.DEFAULT_CASES} - {c[1:] for c in t.CASCADE_CASES} == {(144, 8), (160, 8)} and t.CASCADE_MAX_NODES == const_nodes("kCascadeMaxNodes", "BATH_WAVE_COLUMNS")
    assert all(t.ssv_shape(m) == (nr, g) for m, nr, g in t.DEFAULT_CASES)
    # seams: node 1, node M, every multiple of NR below M, odd multiples between the halves, even ones between lanes
    assert t.ssv_seams(1024, 128, 4) == [(1, "first")] + [(128 * i, "half" if i % 2 else "lane") for i in range(1, 8)] + [(1024, "last")]
    assert t.ssv_seams(1, 16, 1) == [(1, "first")] and t.ssv_seams(16, 16, 1) == [(1, "first"), (16, "last")] and t.ssv_seams(17, 16, 1)[1] == (16, "half")
