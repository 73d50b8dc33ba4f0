"""bath_amd -- MI355X (gfx950) backend for BATH's bathsearch DP hot path.

Thin Python mirror of the C ABI in include/bath_hip.h (the product is libbathhip.so: hand-written HIP
kernels behind `extern "C"` entry points).  Names follow the reference's objects:

    HMM          P7_HMM            (p7_hmmfile.c:1342)
    Profile      P7_PROFILE        (modelconfig.c:48  p7_ProfileConfig)
    FSProfile    P7_FS_PROFILE     (modelconfig.c:220 p7_ProfileConfig_fs)
    OProfile     P7_OPROFILE       (impl_sse/p7_oprofile.c:1091 p7_oprofile_Convert), device resident
    FSOProfile   P7_FS_OPROFILE    (impl_sse/p7_fs_oprofile.c:221), device resident
    SeqBlock     ESL_SQ_BLOCK      digital sequences, device resident
    Pipeline     P7_PIPELINE       (p7_pipeline.c:94, :1584), the filter cascade

There is no CPU fallback: importing works anywhere (so the CPU test tier can check the library
loads and exports every symbol), but creating a Context without a usable GPU raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("BATH_HIP_LIBRARY") or os.path.join(_HERE, "libbathhip.so")   # the override is for A/B timing of two builds

OK, EINVAL, ERANGE, ENORESULT = 0, 11, 16, 19
KP, K, NEVPARAM = 29, 20, 8
LOGSUM_TABLE, LOGSUM_EXACT, LOGSUM_TABLE_SERIAL, LOGSUM_CONTEXT = 0, 1, 2, 3
LOGSUM_ODDS = 4                                     # 3-codon parsers in odds-ratio space (what the reference's --fs runs)
# Context.set_fs_ensemble / set_std_ensemble: how a branch samples a multi-domain region's 200 stochastic tracebacks
ENSEMBLE_SERIAL, ENSEMBLE_STREAMS_HOST, ENSEMBLE_STREAMS_DEVICE = 0, 1, 2
ENSEMBLE_MODES = {"serial": ENSEMBLE_SERIAL, "streams": ENSEMBLE_STREAMS_HOST, "device": ENSEMBLE_STREAMS_DEVICE}
ENS_SAMPLES = 200
ARITH_STRICT, ARITH_ODDS3, ARITH_ODDS = 0, 1, 2     # bath_hip_calibrate_fs_arith; bathsearch / bathconvert --arith
ARITH_MODES = {"strict": ARITH_STRICT, "odds3": ARITH_ODDS3, "odds": ARITH_ODDS}
ENS_OK, ENS_IMPOSSIBLE, ENS_STEP_CAP, ENS_SEG_OVERFLOW = 0, 1, 2, 3      # per-trace status of the stream modes
ENS_REGION_OK, ENS_REGION_NO_TRACES = 0, 1

DNA_SYMS = "ACGT-RYMKSWHBVDN*~"
AMINO_SYMS = "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~"


class BathError(RuntimeError):
    pass


def build(force=False):
    """Compile libbathhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcdir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(srcdir, f) for f in os.listdir(srcdir) if f.endswith((".hip", ".cpp", ".hpp"))]
    srcs.append(os.path.join(_ROOT, "include", "bath_hip.h"))
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", srcdir])
    return LIB_PATH


class _Hmm(C.Structure):
    _fields_ = [("M", C.c_int32), ("max_length", C.c_int32), ("ct", C.c_int32), ("fsprob", C.c_float),
                ("t", C.POINTER(C.c_float)), ("mat", C.POINTER(C.c_float)), ("ins", C.POINTER(C.c_float)),
                ("compo", C.c_float * K), ("evparam", C.c_float * NEVPARAM), ("name", C.c_char * 128),
                ("acc", C.c_char * 64), ("consensus", C.c_char_p), ("rf", C.c_char_p), ("cs", C.c_char_p)]


class _Profile(C.Structure):
    _fields_ = [("M", C.c_int32), ("L", C.c_int32), ("max_length", C.c_int32), ("nj", C.c_float),
                ("tsc", C.POINTER(C.c_float)), ("rsc", C.POINTER(C.c_float)), ("xsc", (C.c_float * 2) * 4),
                ("evparam", C.c_float * NEVPARAM), ("compo", C.c_float * K)]


class _FsProfile(C.Structure):
    _fields_ = [("M", C.c_int32), ("L", C.c_int32), ("max_length", C.c_int32), ("codon_lengths", C.c_int32),
                ("maxcodons", C.c_int32), ("nj", C.c_float), ("fsprob", C.c_float),
                ("tsc", C.POINTER(C.c_float)), ("rsc", C.POINTER(C.c_float)),
                ("codons", C.POINTER(C.c_uint8)), ("indel_pos", C.POINTER(C.c_uint8)),
                ("xsc", (C.c_float * 2) * 4), ("evparam", C.c_float * NEVPARAM), ("compo", C.c_float * K)]


class OProfileScalars(C.Structure):
    _fields_ = [("tbm_b", C.c_uint8), ("tec_b", C.c_uint8), ("tjb_b", C.c_uint8), ("base_b", C.c_uint8), ("bias_b", C.c_uint8),
                ("scale_b", C.c_float), ("xw", (C.c_int16 * 2) * 4), ("scale_w", C.c_float),
                ("base_w", C.c_int16), ("ddbound_w", C.c_int16), ("xf", (C.c_float * 2) * 4)]


class PipelineParams(C.Structure):
    _fields_ = [("F1", C.c_double), ("F2", C.c_double), ("F3", C.c_double), ("F4", C.c_double),
                ("do_biasfilter", C.c_int32), ("fs_pipe", C.c_int32), ("min_orf_len", C.c_int32), ("ncbi_table", C.c_int32),
                ("nres_before", C.c_int64),
                # option state (include/bath_hip.h): --nonull2, --fsonly, --strand, -m / -M, --incT, --seed, -T
                ("do_null2", C.c_int32), ("std_pipe", C.c_int32), ("strands", C.c_int32), ("initiator", C.c_int32),
                ("inc_by_E", C.c_int32), ("seed", C.c_int32), ("T", C.c_double)]


STRAND_BOTH, STRAND_TOPONLY, STRAND_BOTTOMONLY = 0, 1, 2
INIT_ANY, INIT_TABLE, INIT_AUG = 0, 1, 2


class OrfResult(C.Structure):
    _fields_ = [("window", C.c_int64), ("strand", C.c_int32), ("frame", C.c_int32), ("start", C.c_int32), ("end", C.c_int32),
                ("n", C.c_int32), ("stage", C.c_int32), ("msv_status", C.c_int32), ("vit_status", C.c_int32),
                ("usc", C.c_float), ("nullsc", C.c_float), ("filtersc", C.c_float), ("vfsc", C.c_float), ("fwdsc", C.c_float),
                ("P", C.c_double)]


ORF_RESULT_DTYPE = np.dtype([("window", "<i8"), ("strand", "<i4"), ("frame", "<i4"), ("start", "<i4"), ("end", "<i4"),
                             ("n", "<i4"), ("stage", "<i4"), ("msv_status", "<i4"), ("vit_status", "<i4"),
                             ("usc", "<f4"), ("nullsc", "<f4"), ("filtersc", "<f4"), ("vfsc", "<f4"), ("fwdsc", "<f4"),
                             ("P", "<f8")], align=True)


class PipelineStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("nres", "n_orfs", "n_past_msv", "n_past_bias", "n_past_vit", "n_past_fwd",
                                          "pos_past_msv", "pos_past_bias", "pos_past_vit", "pos_past_fwd",
                                          "cells_msv", "cells_vit", "cells_fwd")]


class Orf(C.Structure):
    """bath_orf (include/bath_hip.h): one ORF of the six-frame translation."""
    _fields_ = [("window", C.c_int64), ("strand", C.c_int32), ("frame", C.c_int32), ("start", C.c_int32), ("end", C.c_int32),
                ("n", C.c_int32), ("aa_off", C.c_int64)]


class FsWindow(C.Structure):
    """bath_fs_window (include/bath_hip.h): one DNA window of the frameshift stage."""
    _fields_ = [("window", C.c_int64), ("strand", C.c_int32), ("n", C.c_int32), ("length", C.c_int32),
                ("orf_cnt", C.c_int32), ("k_min", C.c_int32), ("k_max", C.c_int32),
                ("tot_orfsc", C.c_float), ("nullsc", C.c_float), ("filtersc", C.c_float), ("fwdsc", C.c_float),
                ("P_tot", C.c_double), ("P_min", C.c_double), ("P_fs", C.c_double), ("P_null", C.c_double),
                ("branch", C.c_int32)]


class FsDomain(C.Structure):
    """bath_fs_domain (include/bath_hip.h): a domain of the frameshift branch with the scores of its hit."""
    _fields_ = [("window", C.c_int64), ("strand", C.c_int32), ("fs_window", C.c_int32),
                ("ienv", C.c_int32), ("jenv", C.c_int32), ("iali", C.c_int32), ("jali", C.c_int32), ("ihmm", C.c_int32), ("jhmm", C.c_int32),
                ("envsc", C.c_float), ("oasc", C.c_float), ("domcorrection", C.c_float), ("dombias", C.c_float),
                ("bitscore", C.c_float), ("pre_score", C.c_float), ("lnP", C.c_double), ("reported", C.c_int32), ("n_shifted_codons", C.c_int32),
                ("n_stops", C.c_int32), ("pid", C.c_float), ("ali_columns", C.c_int32), ("cigar_off", C.c_int64)]
    cigar = ""       # filled by Pipeline.run_hits / run_frameshift_domains


_DTYPES = {}


class DomainTrace(C.Structure):
    """bath_domain_trace: where a domain's trace lies in the arrays of bath_hip_domain_traces."""
    _fields_ = [("off", C.c_int64), ("N", C.c_int32), ("win_start", C.c_int32), ("orf_start", C.c_int32), ("frameshift", C.c_int32)]


class AliDisplayOpts(C.Structure):
    _fields_ = [("hmm_name", C.c_char_p), ("seq_name", C.c_char_p), ("consensus", C.c_char_p), ("rf", C.c_char_p), ("cs", C.c_char_p),
                ("M", C.c_int32), ("sqfrom", C.c_int64), ("sqto", C.c_int64), ("textw", C.c_int32), ("show_frameline", C.c_int32),
                ("initiator", C.c_int32)]


class FsRow(C.Structure):
    """bath_fs_row: one row of --fstblout."""
    _fields_ = [("type", C.c_char), ("length", C.c_int32), ("ali_start", C.c_int32), ("seq_start", C.c_int64)]


class DistItem(C.Structure):
    """bath_dist_item: windows [lo, hi) of query <query>."""
    _fields_ = [("query", C.c_int32), ("lo", C.c_int64), ("hi", C.c_int64)]


T_M, T_D, T_I = 1, 2, 3


def _np_dtype(T):
    """numpy's record dtype of a ctypes structure, converted once (the conversion walks the fields: 70 us for FsDomain)."""
    d = _DTYPES.get(T)
    if d is None:
        d = _DTYPES[T] = np.dtype(T)
    return d


FS_DOMAIN_DTYPE = _np_dtype(FsDomain)      # bath_fs_domain as a numpy record dtype


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_float), ("launches", C.c_int64), ("cells", C.c_double), ("bytes", C.c_double)]


class HmmWindow(C.Structure):
    _fields_ = [("target", C.c_int64), ("n", C.c_int32), ("k", C.c_int32), ("length", C.c_int32), ("score", C.c_float)]


class StdResult(C.Structure):
    _fields_ = [("fwdsc", C.c_float), ("bcksc", C.c_float), ("oasc", C.c_float), ("fwd_status", C.c_int32), ("bck_status", C.c_int32),
                ("ok", C.c_int32), ("null2", C.c_float * KP)]


class Fs5Result(C.Structure):
    _fields_ = [("fwdsc", C.c_float), ("bcksc", C.c_float), ("oasc", C.c_float), ("null2", C.c_float * KP)]


_CALIB_SCORE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(C.c_float))   # bath_calib_score_fn

# name -> (restype, argtypes); every symbol include/bath_hip.h declares
_vp, _u8p, _f32p, _i32p, _i64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
ABI = {
    "bath_hmmfile_count": (C.c_int, [C.c_char_p]),
    "bath_hmmfile_read": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.POINTER(_Hmm))]),
    "bath_hmm_destroy": (None, [C.POINTER(_Hmm)]),
    "bath_gencode_basic": (C.c_int, [C.c_int, _u8p]),
    "bath_profile_config": (C.c_int, [C.POINTER(_Hmm), C.c_int, C.POINTER(C.POINTER(_Profile))]),
    "bath_profile_destroy": (None, [C.POINTER(_Profile)]),
    "bath_fs_profile_config": (C.c_int, [C.POINTER(_Hmm), _u8p, C.c_int, C.c_int, C.POINTER(C.POINTER(_FsProfile))]),
    "bath_fs_profile_destroy": (None, [C.POINTER(_FsProfile)]),
    "bath_hip_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "bath_hip_finalize": (None, [_vp]),
    "bath_hip_last_error": (C.c_char_p, [_vp]),
    "bath_hip_synchronize": (C.c_int, [_vp]),
    "bath_hip_stream": (_vp, [_vp]),
    "bath_hip_set_fs_strict": (C.c_int, [_vp, C.c_int]),
    "bath_hip_set_fwd_group": (C.c_int, [_vp, C.c_int]),
    "bath_hip_set_fs_serial": (C.c_int, [_vp, C.c_int]),
    "bath_hip_set_fs_odds": (C.c_int, [_vp, C.c_int]),
    "bath_hip_set_fs5_odds": (C.c_int, [_vp, C.c_int]),
    "bath_hip_set_fs_ensemble": (C.c_int, [_vp, C.c_int]),
    "bath_hip_fs_ensemble_counters": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "bath_hip_set_std_ensemble": (C.c_int, [_vp, C.c_int]),
    "bath_hip_std_ensemble_counters": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "bath_hip_std_region_ensembles": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_uint32, _i32p, _i32p, _i32p, C.c_int64, _i64p, _i32p, _f32p, C.c_int64, _i64p]),
    "bath_selftest_std_ensemble": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, C.c_float, C.c_float, C.c_float, _u8p, C.c_int, _f32p, _f32p, C.c_uint32, _i32p, _i32p,
                                             _i32p, C.c_int, _i32p, _f32p, _i32p, C.c_int, _i32p]),
    "bath_selftest_std_ens_walk": (C.c_int, [C.c_int, _f32p, C.c_float, C.c_float, C.c_float, C.c_int, _f32p, _f32p, C.c_uint32, _i32p, _i32p, C.c_int, _i32p]),
    "bath_hip_fs5_region_ensembles": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _i32p, _i32p, _i32p, C.c_int64, _i64p, _i32p, C.c_int64, _i64p]),
    "bath_selftest_fs_ensemble_seeded": (C.c_int, [C.c_int, _f32p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _f32p, _f32p, C.c_uint32, _i32p, C.c_int, _i32p]),
    "bath_selftest_fs_ensemble_streams": (C.c_int, [C.c_int, _f32p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _f32p, _f32p, C.c_uint32,
                                                    _i32p, _i32p, _i32p, C.c_int, _i32p, _i32p, C.c_int, _i32p]),
    "bath_selftest_rng_jump": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]),
    "bath_selftest_ens_explog": (C.c_int, [C.c_int, _f32p, _f32p, _f32p]),
    "bath_selftest_compute_units": (C.c_int, [_vp]),
    "bath_selftest_compo_terms": (C.c_int, [C.c_int, C.c_float, _f32p]),
    "bath_selftest_len_sort": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _i32p, _i32p]),
    "bath_selftest_fs_windows": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _i32p, _i64p, _i32p, _vp]),
    "bath_selftest_fs_decide": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p, _f32p, C.c_int, C.c_int, C.c_double, C.c_int]),
    "bath_hip_trim": (C.c_int, [_vp]),
    "bath_hip_kernel_times": (C.c_int, [_vp, C.c_int, C.POINTER(KernelTime)]),
    "bath_hip_oprofile_convert": (C.c_int, [_vp, C.POINTER(_Profile), C.POINTER(_vp)]),
    "bath_hip_oprofile_destroy": (None, [_vp]),
    "bath_hip_oprofile_M": (C.c_int, [_vp]),
    "bath_hip_oprofile_scalars": (C.c_int, [_vp, C.c_int, C.POINTER(OProfileScalars)]),
    "bath_hip_oprofile_get_ssv_scores": (C.c_int, [_vp, _u8p]),
    "bath_hip_oprofile_get_vit": (C.c_int, [_vp, C.POINTER(C.c_int16), C.POINTER(C.c_int16)]),
    "bath_hip_oprofile_get_fwd": (C.c_int, [_vp, _f32p, _f32p]),
    "bath_hip_seqs_create": (C.c_int, [_vp, _u8p, _i64p, C.c_int64, C.POINTER(_vp)]),
    "bath_hip_seqs_destroy": (None, [_vp]),
    "bath_hip_seqs_count": (C.c_int64, [_vp]),
    "bath_hip_seqs_read": (C.c_int64, [_vp, _u8p, C.c_int64, _i64p, _i32p, _i32p]),
    "bath_hip_seqs_set_context": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "bath_hip_host_alloc": (C.c_void_p, [C.c_size_t]),
    "bath_hip_host_free": (None, [C.c_void_p]),
    "bath_hip_seqs_create_packed": (C.c_int, [_vp, _i64p, C.c_int64, C.POINTER(_vp)]),
    "bath_hip_seqs_upload_packed": (C.c_int, [_vp, C.c_void_p, _i64p, _i32p, _u8p, C.c_int64]),
    "bath_hip_seqs_upload_wait": (C.c_int, [_vp]),
    "bath_hip_fasta_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "bath_hip_fasta_destroy": (None, [_vp]),
    "bath_hip_fasta_feed": (C.c_int, [_vp, C.c_void_p, C.c_int64]),
    "bath_hip_fasta_finish": (C.c_int, [_vp]),
    "bath_hip_fasta_count": (C.c_int64, [_vp]),
    "bath_hip_fasta_symbols": (C.c_int64, [_vp]),
    "bath_hip_fasta_records": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_void_p]),
    "bath_hip_fasta_error": (C.c_int, [_vp, _i64p, _i64p, _i64p, _i32p]),
    "bath_hip_fasta_windows": (C.c_int64, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "bath_hip_fasta_seqs": (C.c_int, [_vp, C.c_void_p, C.c_int64, C.POINTER(_vp)]),
    "bath_hip_fasta_seqs_for": (C.c_int, [_vp, _vp, C.c_void_p, C.c_int64, C.POINTER(_vp)]),
    "bath_hip_fasta_codes": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _u8p]),
    "bath_hip_fasta_release": (C.c_int, [_vp, C.c_int64]),
    "bath_hip_ssvfilter": (C.c_int, [_vp, _vp, _vp, _f32p, _i32p]),
    "bath_hip_msvfilter": (C.c_int, [_vp, _vp, _vp, _f32p, _i32p]),
    "bath_hip_vitfilter": (C.c_int, [_vp, _vp, _vp, _f32p, _i32p]),
    "bath_hip_forward_parser": (C.c_int, [_vp, _vp, _vp, _f32p, _i32p]),
    "bath_hip_fwdparser_group": (C.c_int, [_vp, _vp, _vp, _f32p, _i32p]),
    "bath_hip_bias_filter": (C.c_int, [_vp, _vp, _vp, _f32p, _f32p]),
    "bath_hip_fwdback_parser": (C.c_int, [_vp, _vp, _vp, _i64p, _f32p, _f32p, _i32p, _i32p, _f32p, _f32p]),
    "bath_hip_translate_orfs": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(C.POINTER(Orf)), _i64p, C.POINTER(_u8p)]),
    "bath_hip_translate_orfs_opts": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(Orf)), _i64p, C.POINTER(_u8p)]),
    "bath_hip_orf_worklist": (C.c_int, [_vp, C.c_void_p, _i64p]),
    "bath_gencode_initiators": (C.c_int, [C.c_int, C.c_int, _u8p]),
    "bath_tophits_set_score_thresholds": (None, [_vp, C.c_int, C.c_double, C.c_int, C.c_double]),
    "bath_search_space_residues": (C.c_int64, [C.c_int, C.c_double, C.c_int, C.c_int64]),
    "bath_pipeline_params_default": (None, [C.POINTER(PipelineParams), C.c_int]),
    "bath_hip_pipeline_filters": (C.c_int, [_vp, _vp, _vp, C.POINTER(PipelineParams), C.POINTER(PipelineStats),
                                            C.POINTER(C.POINTER(OrfResult)), _i64p]),
    "bath_hip_pipeline_frameshift": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(PipelineParams), C.POINTER(PipelineStats),
                                              C.POINTER(C.POINTER(OrfResult)), _i64p, C.POINTER(C.POINTER(FsWindow)), _i64p]),
    "bath_hip_oprofile_set_consensus": (C.c_int, [_vp, C.c_char_p]),
    "bath_hip_domain_cigars": (C.c_void_p, [_vp]),
    "bath_hip_domain_traces": (C.c_int, [_vp, C.POINTER(C.POINTER(DomainTrace)), _i64p, C.POINTER(C.POINTER(C.c_int8)), C.POINTER(_i32p),
                                         C.POINTER(_i32p), C.POINTER(C.POINTER(C.c_int8)), C.POINTER(_f32p)]),
    "bath_alidisplay_print": (C.c_int64, [C.POINTER(DomainTrace), C.POINTER(C.c_int8), _i32p, _i32p, C.POINTER(C.c_int8), _f32p,
                                          _u8p, C.c_int32, C.POINTER(_FsProfile), C.POINTER(_Profile), _u8p, C.POINTER(AliDisplayOpts),
                                          C.c_char_p, C.c_int64]),
    "bath_selftest_rng_stream": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_double)]),
    "bath_selftest_fchoose": (C.c_int, [C.c_uint32, _f32p, C.c_int, C.c_int, _i32p]),
    "bath_hits_serialize": (C.c_int64, [C.c_void_p, C.c_int64, C.c_char_p, C.POINTER(DomainTrace), C.POINTER(C.c_int8), _i32p, _i32p, C.POINTER(C.c_int8), _f32p,
                                        C.c_void_p, C.c_int64]),
    "bath_hits_deserialize": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(_vp)]),
    "bath_hits_stream_size": (C.c_int64, [C.c_void_p, C.c_int64]),
    "bath_hits_destroy": (None, [_vp]),
    "bath_hits_count": (C.c_int64, [_vp]),
    "bath_hits_domains": (C.POINTER(FsDomain), [_vp]),
    "bath_hits_cigars": (C.c_void_p, [_vp, _i64p]),
    "bath_hits_traces": (C.c_int, [_vp, C.POINTER(C.POINTER(DomainTrace)), C.POINTER(C.POINTER(C.c_int8)), C.POINTER(_i32p), C.POINTER(_i32p),
                                   C.POINTER(C.POINTER(C.c_int8)), C.POINTER(_f32p)]),
    "bath_tophits_add_serialized": (C.c_int, [_vp, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                              C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "bath_dist_shard_range": (None, [C.c_int64, C.c_int, C.c_int, _i64p, _i64p]),
    "bath_dist_items": (C.c_int64, [_i64p, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(DistItem), C.c_int64]),
    "bath_dist_deal": (C.c_int, [C.POINTER(C.c_double), C.c_int64, C.c_int, _i32p]),
    "bath_selftest_cluster_segments": (C.c_int, [C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int, C.c_int, _i32p, C.c_int, _i32p]),
    "bath_selftest_fs_ensemble": (C.c_int, [C.c_int, _f32p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _f32p, _f32p, _i32p, C.c_int, _i32p]),
    "bath_tophits_create": (_vp, []),
    "bath_tophits_destroy": (None, [_vp]),
    "bath_tophits_add": (C.c_int, [_vp, C.POINTER(FsDomain), C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                   C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "bath_tophits_finalize": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_double]),
    "bath_tophits_count": (C.c_int64, [_vp]),
    "bath_tophits_reported": (C.c_int64, [_vp]),
    "bath_tophits_get": (C.c_int, [_vp, C.c_int64, C.POINTER(FsDomain), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "bath_tophits_targets": (C.c_int64, [_vp, C.c_int, C.c_int, C.c_char_p, C.c_int64]),
    "bath_tophits_domain_annotation": (C.c_int64, [_vp, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_int64]),
    "bath_tophits_pipeline_statistics": (C.c_int64, [_vp, C.POINTER(PipelineStats), C.POINTER(PipelineParams), C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int64]),
    "bath_tophits_set_inclusion": (None, [_vp, C.c_double]),
    "bath_tophits_tabular_targets": (C.c_int64, [_vp, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int64]),
    "bath_trace_frameshift_rows": (C.c_int64, [C.POINTER(DomainTrace), C.POINTER(C.c_int8), _i32p, _i32p, C.POINTER(C.c_int8), _u8p, C.c_int32,
                                               C.POINTER(_FsProfile), C.c_int64, C.c_int64, C.POINTER(FsRow), C.c_int64]),
    "bath_tophits_tabular_frameshifts": (C.c_int64, [_vp, C.c_char_p, C.c_char_p, C.POINTER(FsRow), _i64p, C.c_int64, C.c_int, C.c_char_p, C.c_int64]),
    "bath_hip_pipeline_hits": (C.c_int, [_vp, _vp, _vp, C.POINTER(PipelineParams), C.c_double, C.POINTER(PipelineStats),
                                         C.POINTER(C.POINTER(FsDomain)), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bath_hip_pipeline_frameshift_domains": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(PipelineParams), C.c_double, C.POINTER(PipelineStats),
                                                      C.POINTER(C.POINTER(FsWindow)), _i64p, C.POINTER(C.POINTER(FsDomain)), _i64p, _i64p]),
    "bath_hip_pipeline_timings": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), _f32p, _i64p]),
    "bath_hip_fsprofile_convert": (C.c_int, [_vp, C.POINTER(_FsProfile), C.POINTER(_vp)]),
    "bath_hip_fsprofile_destroy": (None, [_vp]),
    "bath_hip_fs3_forward_parser": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p, _f32p, _i64p]),
    "bath_hip_fs3_backward_parser": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p, _f32p, _i64p]),
    "bath_hip_vitfilter_bath": (C.c_int, [_vp, _vp, _vp, _f32p, C.c_double, _f32p, _i32p, C.POINTER(C.POINTER(HmmWindow)), _i64p]),
    "bath_hip_ssvfilter_bath": (C.c_int, [_vp, _vp, _vp, C.c_double, C.POINTER(C.POINTER(HmmWindow)), _i64p]),
    "bath_hip_forward_full": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_int, _f32p, _i32p, _f32p, _f32p]),
    "bath_hip_std_envelopes": (C.c_int, [_vp, _vp, _vp, C.POINTER(StdResult), _f32p, _f32p, _f32p, _f32p]),
    "bath_hip_std_envelopes_fill": (C.c_int, [_vp, _vp, _vp, C.POINTER(StdResult), _f32p, _f32p, _f32p, _f32p, C.c_int]),
    "bath_hip_fs5_envelopes_x": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(Fs5Result), _f32p, _f32p, _f32p, _f32p]),
    "bath_hip_fs5_forward_full": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p, _f32p, _f32p]),
    "bath_hip_fs5_envelopes": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(Fs5Result), _f32p, _i64p, _f32p, _i64p]),
    "bath_hip_fs5_forward_parser": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p]),
    "bath_hip_fs5_forward_parser_odds": (C.c_int, [_vp, _vp, _vp, C.c_int, _f32p]),
    "bath_calib_fit_scores": (C.c_int, [C.POINTER(C.c_uint32), _f32p, C.c_int, C.c_int, C.c_int, _CALIB_SCORE_FN, C.c_void_p, C.c_float,
                                        C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "bath_hip_calibrate_fs_arith": (C.c_int, [_vp, C.POINTER(_Hmm), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_double,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.c_int, C.POINTER(C.c_int)]),
    "bath_calib_sample": (C.c_int, [C.POINTER(C.c_uint32), _f32p, C.c_int, C.c_int, C.c_int, _u8p]),
    "bath_gumbel_fit_complete": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bath_gumbel_invcdf": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "bath_calib_tau": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "bath_bg_fs_nullone": (C.c_float, [C.c_int]),
    "bath_hmm_max_length": (C.c_int, [C.POINTER(_Hmm), C.c_double]),
    "bath_hip_calibrate_fs": (C.c_int, [_vp, C.POINTER(_Hmm), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_double,
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bath_calib_sample_batch": (C.c_int, [C.POINTER(C.c_uint32), _f32p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, _u8p]),
    "bath_hip_calibrate_fs_batch": (C.c_int, [_vp, C.POINTER(C.POINTER(_Hmm)), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int,
                                              C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bath_calib_skip": (C.c_int, [C.POINTER(C.c_uint32), _f32p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bath_hip_calibrate_fs_batch_at": (C.c_int, [_vp, C.POINTER(C.POINTER(_Hmm)), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                 C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double)]),
    # single-sequence models and their calibration (bathbuild)
    "bath_scorematrix_builtin": (C.c_char_p, [C.c_char_p]),
    "bath_scoresystem_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.POINTER(_vp), C.c_char_p, C.c_int]),
    "bath_scoresystem_destroy": (None, [_vp]),
    "bath_scoresystem_lambda": (C.c_double, [_vp]),
    "bath_scoresystem_conditionals": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "bath_hmm_from_sequence": (C.c_int, [_vp, _u8p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.POINTER(_Hmm))]),
    "bath_hmm_mean_match_relent": (C.c_double, [C.POINTER(_Hmm)]),
    "bath_hmm_mean_position_relent": (C.c_double, [C.POINTER(_Hmm)]),
    "bath_hmm_lambda": (C.c_double, [C.POINTER(_Hmm)]),
    "bath_hmm_write_ascii": (C.c_int64, [C.POINTER(_Hmm), C.c_int, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64]),
    "bath_calib_sample_amino": (C.c_int, [C.POINTER(C.c_uint32), _f32p, C.c_int, C.c_int, _u8p]),
    "bath_gumbel_fit_complete_loc": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "bath_hip_calibrate_batch": (C.c_int, [_vp, C.POINTER(C.POINTER(_Hmm)), C.c_int, C.c_int, C.POINTER(C.c_uint32), _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "bath_hip_calib_samples_create": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "bath_hip_calib_samples_destroy": (None, [_vp]),
    "bath_hip_calibrate": (C.c_int, [_vp, C.POINTER(_Hmm), C.c_int, C.POINTER(C.c_uint32), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "bath_hip_calibrate_std": (C.c_int, [_vp, C.POINTER(_Hmm), C.POINTER(C.c_uint32), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_double, C.POINTER(C.c_double)]),
    "bath_hip_calibrate_std_batch": (C.c_int, [_vp, C.POINTER(C.POINTER(_Hmm)), C.c_int, C.POINTER(C.c_uint32), _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
}

_lib = None


def lib():
    """Load libbathhip.so (raises BathError with the build hint if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BathError("libbathhip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(or `make -C bath_amd/csrc`). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)          # AttributeError => the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _u8(a):
    return a.ctypes.data_as(_u8p)


def _f32(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def _i64(a):
    return None if a is None else a.ctypes.data_as(_i64p)


def digitize(seq, syms):
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(syms):
        lut[ord(ch)] = i
        lut[ord(ch.lower())] = i
    if syms is DNA_SYMS:
        lut[ord("U")] = lut[ord("u")] = 3
        lut[ord("X")] = lut[ord("x")] = 15
    codes = lut[np.frombuffer(seq.encode(), dtype=np.uint8)]
    if (codes == 255).any():
        raise BathError("symbol outside the alphabet")
    return codes


class HMM:
    """A profile HMM read from a BATH3/f file."""

    def __init__(self, path, index=0):
        p = C.POINTER(_Hmm)()
        st = lib().bath_hmmfile_read(os.fsencode(path), index, C.byref(p))
        if st != OK:
            raise BathError("cannot read model %d of %s (status %d)" % (index, path, st))
        self._adopt(p)

    @classmethod
    def _from_pointer(cls, p):
        """A model the library made in memory (seq_model); owned by the object like one read from a file."""
        self = cls.__new__(cls)
        self._adopt(p)
        return self

    def _adopt(self, p):
        self._p = p
        self.M = p.contents.M
        self.ct = p.contents.ct
        self.max_length = p.contents.max_length
        self.name = p.contents.name.decode()
        self.acc = p.contents.acc.decode()
        self.consensus = p.contents.consensus.decode() if p.contents.consensus else ""
        self.rf = p.contents.rf.decode() if p.contents.rf else None
        self.cs = p.contents.cs.decode() if p.contents.cs else None
        self.evparam = np.array(p.contents.evparam[:], dtype=np.float32)

    @staticmethod
    def count(path):
        return lib().bath_hmmfile_count(os.fsencode(path))

    def __del__(self):
        if getattr(self, "_p", None):
            lib().bath_hmm_destroy(self._p)
            self._p = None


def gencode_basic(ncbi_table):
    b = np.zeros(64, dtype=np.uint8)
    if lib().bath_gencode_basic(ncbi_table, _u8(b)) != OK:
        raise BathError("unknown NCBI translation table %d" % ncbi_table)
    return b


class Profile:
    """p7_ProfileConfig(hmm, bg, gm, L, p7_LOCAL)."""

    def __init__(self, hmm, L=100):
        p = C.POINTER(_Profile)()
        st = lib().bath_profile_config(hmm._p, L, C.byref(p))
        if st != OK:
            raise BathError("profile config failed (%d)" % st)
        self._p, self.M, self.hmm = p, hmm.M, hmm

    def arrays(self):
        g = self._p.contents
        tsc = np.ctypeslib.as_array(g.tsc, shape=(self.M, 8)).copy()
        rsc = np.ctypeslib.as_array(g.rsc, shape=(KP, self.M + 1, 2)).copy()
        xsc = np.array([[g.xsc[i][j] for j in range(2)] for i in range(4)], dtype=np.float32)
        return tsc, rsc, xsc

    def __del__(self):
        if getattr(self, "_p", None):
            lib().bath_profile_destroy(self._p)
            self._p = None


class FSProfile:
    """p7_ProfileConfig_fs(hmm, bg, gcode, gm_fs, L, p7_LOCAL) for 3 or 5 codon lengths."""

    def __init__(self, hmm, codon_lengths, L_amino=100, ncbi_table=None):
        self.basic = gencode_basic(hmm.ct if ncbi_table is None else ncbi_table)
        p = C.POINTER(_FsProfile)()
        st = lib().bath_fs_profile_config(hmm._p, _u8(self.basic), codon_lengths, L_amino, C.byref(p))
        if st != OK:
            raise BathError("fs profile config failed (%d)" % st)
        self._p, self.M, self.hmm, self.codon_lengths = p, hmm.M, hmm, codon_lengths
        self.maxcodons = p.contents.maxcodons

    def arrays(self):
        g = self._p.contents
        nrows = self.maxcodons + KP
        tsc = np.ctypeslib.as_array(g.tsc, shape=(self.M, 8)).copy()
        rsc = np.ctypeslib.as_array(g.rsc, shape=(nrows, self.M + 1)).copy()
        codons = np.ctypeslib.as_array(g.codons, shape=(self.M + 1, self.maxcodons)).copy()
        indel = np.ctypeslib.as_array(g.indel_pos, shape=(self.M + 1, self.maxcodons)).copy()
        return tsc, rsc, codons, indel

    def __del__(self):
        if getattr(self, "_p", None):
            lib().bath_fs_profile_destroy(self._p)
            self._p = None


class Context:
    """One GPU + one HIP stream (the reference's per-thread WORKER_INFO, bathsearch.c:34)."""

    def __init__(self, device=0):
        h = _vp()
        st = lib().bath_hip_init(device, C.byref(h))
        if st != OK:
            raise BathError("bath_hip_init(device=%d) failed with status %d: no usable gfx950 GPU; "
                            "this backend has no CPU fallback" % (device, st))
        self._h = h

    def _check(self, st, what):
        if st != OK:
            raise BathError("%s failed (%d): %s" % (what, st, lib().bath_hip_last_error(self._h).decode()))

    def synchronize(self):
        """Waits for the context's stream; also makes the context's device the calling host thread's current one (HIP keeps a
        current device per thread, 0 in a new thread): what a worker thread calls first."""
        self._check(lib().bath_hip_synchronize(self._h), "synchronize")

    def trim(self):
        """Release the lanes, side contexts and side streams of this context (re-created on demand): before it sits idle beside
        worker contexts.  Arrays returned by earlier calls on this context are invalid afterwards."""
        self._check(lib().bath_hip_trim(self._h), "trim")

    def set_fs_strict(self, on=True):
        """True (the library's default): frameshift log-sums along the model in the reference's serial order, bit-identical to the
        generic reference.  False: the fast mode (wavefront scans, scores within O(1e-3) nats)."""
        self._check(lib().bath_hip_set_fs_strict(self._h, 1 if on else 0), "set_fs_strict")

    def set_fwd_group(self, mode):
        """Which kernel scores the cascade's Forward stage.  0 (the default) and 1: the group kernel (four targets per wave) for models
        of up to 160 nodes whose Forward rows are not kept for the domain stage, blocks of every size; the wave-per-target kernel
        otherwise.  2: never.  The two agree within the Forward parser's tolerance, not bit for bit."""
        self._check(lib().bath_hip_set_fwd_group(self._h, int(mode)), "set_fwd_group")

    def set_fs_odds(self, on=True):
        """True: the pipeline's 3-codon Forward and Backward parsers run in odds-ratio space (LOGSUM_ODDS, what the reference's
        --fs runs), and LOGSUM_CONTEXT on FS3ForwardParser / FS3BackwardParser means LOGSUM_ODDS.  False (the default): no change.
        The other frameshift stages follow set_fs_strict either way."""
        self._check(lib().bath_hip_set_fs_odds(self._h, 1 if on else 0), "set_fs_odds")

    def set_fs5_odds(self, on=True):
        """True: the 5-codon Forward and Backward of the envelopes and the regions' multihit Forward run in odds-ratio space (what
        the reference's --fs runs there), ahead of set_fs_strict, and LOGSUM_CONTEXT on FS5Envelopes means those kernels (c5_compat
        must be 0).  Decoding and optimal accuracy read their matrices unchanged.  False (the default): no change.  With
        set_fs_odds(True) as well, a --fs pass runs the reference's arithmetic everywhere but decoding and optimal accuracy."""
        self._check(lib().bath_hip_set_fs5_odds(self._h, 1 if on else 0), "set_fs5_odds")

    def set_fs_ensemble(self, mode):
        """How the frameshift branch samples the trace ensemble of a multi-domain region: ENSEMBLE_SERIAL (the default: one
        random-number stream per region, host threads), ENSEMBLE_STREAMS_HOST (a stream per trace, host threads) or
        ENSEMBLE_STREAMS_DEVICE (the same walks as 200 lanes of fs_ensemble_kernel; the matrices stay on the device).  Also by name:
        "serial", "streams", "device".  The two stream modes give identical results; against the serial mode envelopes agree as
        two seeds of the serial mode do."""
        self._check(lib().bath_hip_set_fs_ensemble(self._h, ENSEMBLE_MODES.get(mode, mode)), "set_fs_ensemble")

    def fs_ensemble_counters(self):
        """Since the context was created: regions of the stream modes outside the stream rule (serial walk instead), regions with
        more segments in a trace than the kernel keeps (host walk instead), bytes of Forward matrices the device mode kept off the host."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().bath_hip_fs_ensemble_counters(self._h, C.byref(a), C.byref(b), C.byref(c)), "fs_ensemble_counters")
        return {"bound_fallbacks": a.value, "overflow_fallbacks": b.value, "matrix_bytes_kept": c.value}

    def set_std_ensemble(self, mode):
        """The same choice as set_fs_ensemble for the STANDARD branch's multi-domain regions (a plain search; the windows of an --fs
        search that take the standard branch): ENSEMBLE_SERIAL (the default), ENSEMBLE_STREAMS_HOST or ENSEMBLE_STREAMS_DEVICE (200
        lanes of std_ensemble_kernel per region; the matrices stay on the device), also by name.  The two stream modes give identical
        domains; against the serial mode envelopes agree as two seeds of the serial mode do."""
        self._check(lib().bath_hip_set_std_ensemble(self._h, ENSEMBLE_MODES.get(mode, mode)), "set_std_ensemble")

    def std_ensemble_counters(self):
        """Since the context was created: regions a stream mode of set_std_ensemble sent to the serial ensemble (outside the stream
        rule, or more than 64 segments in a trace), regions the kernel sent to the host twin (more than 8), regions the kernel walked."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().bath_hip_std_ensemble_counters(self._h, C.byref(a), C.byref(b), C.byref(c)), "std_ensemble_counters")
        return {"serial_fallbacks": a.value, "twin_fallbacks": b.value, "kernel_regions": c.value}

    def set_fs_serial(self, on):
        """Measurement aid: the envelopes' Backward wavefront after the Forward one instead of beside it (bath_hip_set_fs_serial)."""
        self._check(lib().bath_hip_set_fs_serial(self._h, -1 if on is None else (1 if on else 0)), "set_fs_serial")

    @property
    def stream(self):
        return lib().bath_hip_stream(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().bath_hip_finalize(self._h)
            self._h = None

    def __del__(self):
        self.close()


class OProfile:
    """p7_oprofile_Convert(gm, om): the device-resident limited-precision profile."""

    def __init__(self, ctx, gm):
        h = _vp()
        ctx._check(lib().bath_hip_oprofile_convert(ctx._h, gm._p, C.byref(h)), "oprofile_convert")
        self.ctx, self._h, self.M, self.gm = ctx, h, gm.M, gm
        hmm = getattr(gm, "hmm", None)
        if hmm is not None and hmm.consensus:                 # om->consensus, copied by p7_oprofile_Convert
            ctx._check(lib().bath_hip_oprofile_set_consensus(h, hmm.consensus.encode()), "oprofile_set_consensus")

    def scalars(self, L):
        s = OProfileScalars()
        self.ctx._check(lib().bath_hip_oprofile_scalars(self._h, L, C.byref(s)), "oprofile_scalars")
        return s

    def ssv_scores(self):
        a = np.zeros((self.M + 1, KP), dtype=np.uint8)
        lib().bath_hip_oprofile_get_ssv_scores(self._h, _u8(a))
        return a

    def vit_arrays(self):
        rw = np.zeros((KP, self.M + 1), dtype=np.int16)
        tw = np.zeros((self.M + 1, 8), dtype=np.int16)
        lib().bath_hip_oprofile_get_vit(self._h, rw.ctypes.data_as(C.POINTER(C.c_int16)), tw.ctypes.data_as(C.POINTER(C.c_int16)))
        return rw, tw

    def fwd_arrays(self):
        rf = np.zeros((KP, self.M + 1), dtype=np.float32)
        tf = np.zeros((self.M + 1, 8), dtype=np.float32)
        lib().bath_hip_oprofile_get_fwd(self._h, _f32(rf), _f32(tf))
        return rf, tf

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().bath_hip_oprofile_destroy(self._h)
        self._h = None


class FSOProfile:
    """p7_fs_oprofile_Convert(gm_fs, om_fs)."""

    def __init__(self, ctx, gm_fs):
        h = _vp()
        ctx._check(lib().bath_hip_fsprofile_convert(ctx._h, gm_fs._p, C.byref(h)), "fsprofile_convert")
        self.ctx, self._h, self.M, self.gm = ctx, h, gm_fs.M, gm_fs

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().bath_hip_fsprofile_destroy(self._h)
        self._h = None


class SeqBlock:
    """A block of digital sequences resident in HBM.  <seqs>: list of uint8 code arrays, or (flat, offsets)."""

    def __init__(self, ctx, seqs, offsets=None):
        if offsets is None:
            lens = np.array([len(s) for s in seqs], dtype=np.int64)
            offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
            np.cumsum(lens, out=offsets[1:])
            flat = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
        else:
            flat = np.ascontiguousarray(seqs, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if flat.size == 0:
            flat = np.zeros(1, np.uint8)
        self.n = len(offsets) - 1
        self.lengths = np.diff(offsets)
        h = _vp()
        ctx._check(lib().bath_hip_seqs_create(ctx._h, _u8(flat), _i64(offsets), self.n, C.byref(h)), "seqs_create")
        self.ctx, self._h = ctx, h

    def set_context(self, context):
        """ESL_SQ.C per window: leading nucleotides shared with the previous window of the same target (or None)."""
        if context is None:
            self.ctx._check(lib().bath_hip_seqs_set_context(self._h, None), "seqs_set_context")
            return
        c = np.ascontiguousarray(context, dtype=np.int32)
        assert c.shape == (self.n,)
        self.ctx._check(lib().bath_hip_seqs_set_context(self._h, c.ctypes.data_as(C.POINTER(C.c_int32))), "seqs_set_context")

    def read(self):
        """The block as it lies on the device: (data bytes with their padding, offsets, lengths, contexts) copied to the host."""
        L = lib()
        nbytes = L.bath_hip_seqs_read(self._h, None, 0, None, None, None)
        if nbytes < 0:
            self.ctx._check(-1, "seqs_read")
        data = np.zeros(nbytes, np.uint8)
        off, ln, cx = np.zeros(max(self.n, 1), np.int64), np.zeros(max(self.n, 1), np.int32), np.zeros(max(self.n, 1), np.int32)
        if L.bath_hip_seqs_read(self._h, _u8(data), nbytes, _i64(off), ln.ctypes.data_as(_i32p), cx.ctypes.data_as(_i32p)) != nbytes:
            self.ctx._check(-1, "seqs_read")
        return data, off[:self.n], ln[:self.n], cx[:self.n]

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().bath_hip_seqs_destroy(self._h)
        self._h = None


def pack2(flat, offsets):
    """Host side of a streamed block: (packed bytes, exception sequence indices, positions, codes) for 1-byte DNA codes."""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    n = len(lens)
    bad = np.flatnonzero(flat[offsets[0]:offsets[-1]] > 3) + offsets[0]
    seq = np.searchsorted(offsets, bad, side="right") - 1
    pos = (bad - offsets[seq]).astype(np.int32)
    codes = flat[bad].copy()
    if n and (lens == lens[0]).all() and lens[0] % 4 == 0:                     # equal windows, whole bytes: one reshape
        q = (flat[offsets[0]:offsets[-1]] & 3).reshape(-1, 4)
        packed = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)
    else:
        parts = []
        for i in range(n):
            s = flat[offsets[i]:offsets[i + 1]] & 3
            pad = (-len(s)) % 4
            q = np.concatenate([s, np.zeros(pad, np.uint8)]).reshape(-1, 4)
            parts.append((q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8))
        packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return packed, seq.astype(np.int64), pos, codes


class PinnedBuffer:
    """Page-locked host memory (bath_hip_host_alloc) viewed as a numpy uint8 array: uploads from it are asynchronous."""

    def __init__(self, nbytes):
        self.ptr = lib().bath_hip_host_alloc(max(int(nbytes), 1))
        if not self.ptr:
            raise BathError("cannot allocate %d bytes of page-locked memory" % nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(int(nbytes), 1)).from_address(self.ptr))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().bath_hip_host_free(self.ptr)
            self.ptr = None


class StreamedBlock(SeqBlock):
    """A block that is refilled from the host in 2-bit form (bath_hip_seqs_create_packed / _upload_packed / _upload_wait)."""

    def __init__(self, ctx, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.n = len(offsets) - 1
        self.lengths = np.diff(offsets)
        h = _vp()
        ctx._check(lib().bath_hip_seqs_create_packed(ctx._h, _i64(offsets), self.n, C.byref(h)), "seqs_create_packed")
        self.ctx, self._h = ctx, h

    def upload(self, packed, exc_seq=None, exc_pos=None, exc_code=None):
        """Queue the transfer on the copy stream (returns at once for a PinnedBuffer / page-locked array)."""
        arr = packed.array if isinstance(packed, PinnedBuffer) else np.ascontiguousarray(packed, dtype=np.uint8)
        n_exc = 0 if exc_seq is None else len(exc_seq)
        es = np.ascontiguousarray(exc_seq if n_exc else np.zeros(1), dtype=np.int64)
        ep = np.ascontiguousarray(exc_pos if n_exc else np.zeros(1), dtype=np.int32)
        ec = np.ascontiguousarray(exc_code if n_exc else np.zeros(1), dtype=np.uint8)
        self._keep = (arr, es, ep, ec)
        self.ctx._check(lib().bath_hip_seqs_upload_packed(self._h, arr.ctypes.data, _i64(es), ep.ctypes.data_as(_i32p), _u8(ec), n_exc), "seqs_upload_packed")

    def wait(self):
        """Order the cascade after the upload and expand the block on the device."""
        self.ctx._check(lib().bath_hip_seqs_upload_wait(self._h), "seqs_upload_wait")


FASTA_RECORD_DTYPE = np.dtype([("hdr_begin", "<i8"), ("hdr_end", "<i8"), ("sym_start", "<i8"), ("length", "<i8")])   # bath_fasta_record
FASTA_WINDOW_DTYPE = np.dtype([("target", "<i8"), ("start0", "<i8"), ("n", "<i4"), ("context", "<i4")])             # bath_fasta_window


class FastaFormatError(BathError):
    """A byte the FASTA rules do not allow: .offset (in the file), .line (1-based), .record (0-based; -1: before the first header)."""

    def __init__(self, msg, offset, line, record, byte):
        super().__init__(msg)
        self.offset, self.line, self.record, self.byte = offset, line, record, byte


class FastaTargets:
    """The targets of a FASTA file parsed and digitised on the device (bath_hip_fasta_*): feed() the file's bytes in chunks of any
    size (page-locked ones upload asynchronously), finish(), then records() / windows() / seqs() / codes().  The codes of every
    record stay in device memory until release()."""

    def __init__(self, ctx):
        h = _vp()
        ctx._check(lib().bath_hip_fasta_create(ctx._h, C.byref(h)), "fasta_create")
        self.ctx, self._h, self.nbytes = ctx, h, 0
        self._recs = None

    def feed(self, buf, n=None):
        """The next bytes of the file: a PinnedBuffer (its first <n> bytes), bytes or a uint8 array."""
        if isinstance(buf, PinnedBuffer):
            ptr, n = buf.ptr, int(buf.array.size if n is None else n)
        else:
            arr = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8)
            arr = arr[:n] if n is not None else arr
            ptr, n = arr.ctypes.data, int(arr.size)
        if n == 0:
            return
        st = lib().bath_hip_fasta_feed(self._h, ptr, n)
        self.nbytes += n
        self._recs = None
        if st != OK:
            self._raise(st, "fasta_feed")

    def _raise(self, st, what):
        off, line, rec, byte = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        if lib().bath_hip_fasta_error(self._h, C.byref(off), C.byref(line), C.byref(rec), C.byref(byte)) == OK:
            if rec.value < 0:
                msg = "FASTA format error, line %d: sequence data before the first header" % line.value
            else:
                msg = "FASTA format error, line %d: illegal character %r in record %d" % (line.value, chr(byte.value), rec.value + 1)
            raise FastaFormatError(msg, off.value, line.value, rec.value, byte.value)
        self.ctx._check(st, what)

    def finish(self):
        st = lib().bath_hip_fasta_finish(self._h)
        self._recs = None
        if st != OK:
            self._raise(st, "fasta_finish")

    def __len__(self):
        return int(lib().bath_hip_fasta_count(self._h))

    def records(self):
        """The record table (FASTA_RECORD_DTYPE): header byte range in the file, first symbol, length."""
        if self._recs is None:
            n = len(self)
            out = np.zeros(n, dtype=FASTA_RECORD_DTYPE)
            if n:
                self.ctx._check(lib().bath_hip_fasta_records(self._h, 0, n, out.ctypes.data), "fasta_records")
            self._recs = out
        return self._recs

    @property
    def lengths(self):
        return self.records()["length"].copy()

    def windows(self, max_length, block_length, lo=0, hi=None):
        """The windows of records [lo, hi) (FASTA_WINDOW_DTYPE), as dist.split_targets lists them."""
        hi = len(self) if hi is None else hi
        n = lib().bath_hip_fasta_windows(self._h, lo, hi, int(max_length), int(block_length), None, 0)
        if n < 0:
            raise BathError("fasta_windows failed: %s" % lib().bath_hip_last_error(self.ctx._h).decode())
        out = np.zeros(n, dtype=FASTA_WINDOW_DTYPE)
        if n:
            lib().bath_hip_fasta_windows(self._h, lo, hi, int(max_length), int(block_length), out.ctypes.data, n)
        return out

    def seqs(self, windows, ctx=None):
        """A SeqBlock of the given windows (laid out by the device, contexts set).  ctx: another Context of the same device that
        the block is gathered for and belongs to (bath_hip_fasta_seqs_for: several contexts, one host thread each, may do so at once
        once the targets are finished or between two feeds); None: this handle's own context."""
        w = np.ascontiguousarray(windows, dtype=FASTA_WINDOW_DTYPE)
        h = _vp()
        wp = w.ctypes.data if len(w) else None
        if ctx is None:
            ctx = self.ctx
            ctx._check(lib().bath_hip_fasta_seqs(self._h, wp, len(w), C.byref(h)), "fasta_seqs")
        else:
            ctx._check(lib().bath_hip_fasta_seqs_for(ctx._h, self._h, wp, len(w), C.byref(h)), "fasta_seqs_for")
        blk = SeqBlock.__new__(SeqBlock)
        blk.ctx, blk._h, blk.n = ctx, h, len(w)
        blk.lengths = w["n"].astype(np.int64)
        return blk

    def codes(self, target, start=0, n=None):
        """Codes [start, start + n) of a record, copied to the host."""
        if n is None:
            n = int(self.records()["length"][target]) - start
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self.ctx._check(lib().bath_hip_fasta_codes(self._h, int(target), int(start), int(n), _u8(out)), "fasta_codes")
        return out[:n]

    def release(self, lo):
        self.ctx._check(lib().bath_hip_fasta_release(self._h, int(lo)), "fasta_release")

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib().bath_hip_fasta_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


def fasta_headers(path, records):
    """(name, description) of every record, split from the header bytes of the file (host side: no sequence byte is read)."""
    out = []
    with open(path, "rb") as fh:
        for r in records:
            fh.seek(int(r["hdr_begin"]))
            h = fh.read(int(r["hdr_end"] - r["hdr_begin"])).decode("latin-1").strip()
            parts = h.split(None, 1)
            out.append((parts[0] if parts else "", parts[1].strip() if len(parts) > 1 else ""))
    return out


def translate_orfs(ctx, dna, ncbi_table=1, min_orf_len=20, strands=STRAND_BOTH, initiator=INIT_ANY):
    """Six-frame translation of a DNA SeqBlock (esl_gencode_Process*, bathsearch.c:384-392); strands / initiator: --strand, -m / -M.

    Returns a list of (window, strand, frame, start, end, residues[np.uint8]) sorted by window, strand, frame, start."""
    orfs = C.POINTER(Orf)()
    n = C.c_int64(0)
    aa = _u8p()
    ctx._check(lib().bath_hip_translate_orfs_opts(ctx._h, dna._h, ncbi_table, min_orf_len, strands, initiator, C.byref(orfs), C.byref(n), C.byref(aa)), "translate_orfs")
    out = []
    if n.value == 0:
        return out
    last = orfs[n.value - 1]
    pool = np.ctypeslib.as_array(aa, shape=(last.aa_off + last.n,))      # residues are stored in list order
    for i in range(n.value):
        o = orfs[i]
        out.append((o.window, o.strand, o.frame, o.start, o.end, pool[o.aa_off:o.aa_off + o.n].copy()))
    return out


ORF_WORK_DTYPE = np.dtype([("aa_off", np.int64), ("window", np.int32), ("len_sf", np.int32)])   # bath_orf_work


def orf_worklist(ctx):
    """The length-sorted ORF work list the last translate_orfs call built on the device, in list order (bath_orf_work records:
    aa_off into the device's amino-acid stream pool, window, len_sf = residues | (strand*3 + frame) << 28)."""
    p = C.c_void_p()
    n = C.c_int64(0)
    ctx._check(lib().bath_hip_orf_worklist(ctx._h, C.byref(p), C.byref(n)), "orf_worklist")
    if n.value == 0:
        return np.zeros(0, ORF_WORK_DTYPE)
    buf = (C.c_char * (n.value * ORF_WORK_DTYPE.itemsize)).from_address(p.value)
    return np.frombuffer(buf, ORF_WORK_DTYPE).copy()


def _score_call(fn, what, ctx, om, sq):
    sc = np.zeros(sq.n, dtype=np.float32)
    st = np.zeros(sq.n, dtype=np.int32)
    ctx._check(fn(ctx._h, om._h, sq._h, _f32(sc), st.ctypes.data_as(_i32p)), what)
    return sc, st


def SSVFilter(ctx, om, sq):
    """p7_SSVFilter over a block: (scores[n] nats, status[n])."""
    return _score_call(lib().bath_hip_ssvfilter, "ssvfilter", ctx, om, sq)


def MSVFilter(ctx, om, sq):
    """p7_MSVFilter over a block."""
    return _score_call(lib().bath_hip_msvfilter, "msvfilter", ctx, om, sq)


def ViterbiFilter(ctx, om, sq):
    """p7_ViterbiFilter over a block."""
    return _score_call(lib().bath_hip_vitfilter, "vitfilter", ctx, om, sq)


def ForwardParser(ctx, om, sq):
    """p7_ForwardParser over a block."""
    return _score_call(lib().bath_hip_forward_parser, "forward_parser", ctx, om, sq)


def ForwardParserGroup(ctx, om, sq):
    """p7_ForwardParser over a block by the cascade's group kernel (a quarter wave per target; models of up to 160 nodes, BathError
    beyond): scores within the parser's tolerance of ForwardParser's, not bit-identical."""
    return _score_call(lib().bath_hip_fwdparser_group, "fwdparser_group", ctx, om, sq)


def FwdBackParser(ctx, om, sq):
    """p7_ForwardParser + p7_BackwardParser over a block: (fwd_sc[n], bck_sc[n], fwd_status[n], bck_status[n],
    [fwd xmx (L+1,6)], [bck xmx (L+1,6)]) with xmx columns {E,N,J,B,C,SCALE}."""
    n = sq.n
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((sq.lengths + 1) * 6, out=offs[1:])
    fsc, bsc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    fst, bst = np.zeros(n, np.int32), np.zeros(n, np.int32)
    fx, bx = np.zeros(max(int(offs[-1]), 1), np.float32), np.zeros(max(int(offs[-1]), 1), np.float32)
    ctx._check(lib().bath_hip_fwdback_parser(ctx._h, om._h, sq._h, _i64(offs), _f32(fsc), _f32(bsc), fst.ctypes.data_as(_i32p),
                                             bst.ctypes.data_as(_i32p), _f32(fx), _f32(bx)), "fwdback_parser")
    cut = lambda a: [a[offs[i]:offs[i + 1]].reshape(-1, 6) for i in range(n)]
    return fsc, bsc, fst, bst, cut(fx), cut(bx)


def BiasFilter(ctx, om, sq):
    """(p7_bg_NullOne, p7_bg_FilterScore) over a block."""
    nullsc = np.zeros(sq.n, dtype=np.float32)
    filtersc = np.zeros(sq.n, dtype=np.float32)
    ctx._check(lib().bath_hip_bias_filter(ctx._h, om._h, sq._h, _f32(nullsc), _f32(filtersc)), "bias_filter")
    return nullsc, filtersc


class Pipeline:
    """The filter cascade of p7_Pipeline_BATH over blocks of DNA windows."""

    def __init__(self, ctx, om, fs_pipe=False, ncbi_table=1, **overrides):
        self.ctx, self.om = ctx, om
        self.params = PipelineParams()
        lib().bath_pipeline_params_default(C.byref(self.params), 1 if fs_pipe else 0)
        self.params.ncbi_table = ncbi_table
        for k, v in overrides.items():
            setattr(self.params, k, v)

    def run(self, dna, want_results=True, copy=True):
        """copy=False: the records are a view of the library's page-locked result array, valid until the next pipeline call."""
        stats = PipelineStats()
        res = C.POINTER(OrfResult)()
        n = C.c_int64(0)
        self.ctx._check(lib().bath_hip_pipeline_filters(self.ctx._h, self.om._h, dna._h, C.byref(self.params), C.byref(stats),
                                                        C.byref(res) if want_results else None, C.byref(n)), "pipeline_filters")
        out = None
        if want_results:
            if n.value:
                buf = (OrfResult * n.value).from_address(C.addressof(res.contents))
                out = np.frombuffer(buf, dtype=ORF_RESULT_DTYPE)
                if copy:
                    out = out.copy()
            else:
                out = np.zeros(0, dtype=ORF_RESULT_DTYPE)
        return stats, out

    def run_frameshift(self, om_fs3, dna):
        """bathsearch --fs up to the branch decision: (stats, ORF records, list of FsWindow copies)."""
        stats = PipelineStats()
        res = C.POINTER(OrfResult)()
        n = C.c_int64(0)
        fw = C.POINTER(FsWindow)()
        nfw = C.c_int64(0)
        self.ctx._check(lib().bath_hip_pipeline_frameshift(self.ctx._h, self.om._h, om_fs3._h, dna._h, C.byref(self.params), C.byref(stats),
                                                           C.byref(res), C.byref(n), C.byref(fw), C.byref(nfw)), "pipeline_frameshift")
        if n.value:
            buf = (OrfResult * n.value).from_address(C.addressof(res.contents))
            out = np.frombuffer(buf, dtype=ORF_RESULT_DTYPE).copy()
        else:
            out = np.zeros(0, dtype=ORF_RESULT_DTYPE)
        wins = []
        for i in range(nfw.value):
            w = FsWindow()
            C.memmove(C.byref(w), C.byref(fw[i]), C.sizeof(FsWindow))
            wins.append(w)
        return stats, out, wins

    def run_hits(self, dna, E_report=10.0, arrays=False, nres_before=0):
        """bathsearch (no --fs) through domain definition and hit scores: (stats, [FsDomain], multi-domain regions skipped).
        arrays=True: (stats, HitArray, regions) -- the records as ONE numpy record array and the CIGAR strings as one bytes pool,
        copied out of the library with two memcpys instead of a Python object per hit (what TopHits.add_arrays and
        dist.gather_query_hits take).  nres_before: the residues the search counted before this block's first window (both strands;
        pli->nres on entry) -- with it a search cut into blocks reports the hits of the same search run as one block."""
        stats = PipelineStats()
        self.params.nres_before = int(nres_before)
        dm = C.POINTER(FsDomain)(); ndm = C.c_int64(0)
        nskip = C.c_int64(0)
        self.ctx._check(lib().bath_hip_pipeline_hits(self.ctx._h, self.om._h, dna._h, C.byref(self.params), E_report, C.byref(stats),
                                                     C.byref(dm), C.byref(ndm), C.byref(nskip)), "pipeline_hits")
        if arrays:
            return stats, self._hit_array(dm, ndm.value), nskip.value
        return stats, self._domains(dm, ndm.value), nskip.value

    def _hit_array(self, dm, n):
        if n == 0:
            return HitArray(np.zeros(0, dtype=FS_DOMAIN_DTYPE), b"")
        rec = np.frombuffer((FsDomain * n).from_address(C.addressof(dm.contents)), dtype=FS_DOMAIN_DTYPE).copy()
        base = lib().bath_hip_domain_cigars(self.ctx._h)
        last = int(rec["cigar_off"].max())
        end = last + len(C.string_at(base + last)) + 1 if base else 0
        return HitArray(rec, C.string_at(base, end) if base else b"")

    def _domains(self, dm, n):
        """Copies of the ctx-owned domain records, each with its --cigar string attached."""
        base = lib().bath_hip_domain_cigars(self.ctx._h)
        out = []
        for i in range(n):
            x = FsDomain()
            C.memmove(C.byref(x), C.byref(dm[i]), C.sizeof(FsDomain))
            x.cigar = C.string_at(base + x.cigar_off).decode() if base else ""
            out.append(x)
        return out

    def run_frameshift_domains(self, om_fs3, om_fs5, dna, E_report=10.0, arrays=False, nres_before=0):
        """bathsearch --fs through domain definition: (stats, [FsWindow], [FsDomain], multi-domain regions skipped).
        arrays=True: the windows and domains as numpy record arrays viewing the library's own memory (valid until the next
        pipeline call), without the per-record Python objects and CIGAR strings.  nres_before: as in run_hits."""
        stats = PipelineStats()
        self.params.nres_before = int(nres_before)
        fw = C.POINTER(FsWindow)(); nfw = C.c_int64(0)
        dm = C.POINTER(FsDomain)(); ndm = C.c_int64(0)
        nskip = C.c_int64(0)
        self.ctx._check(lib().bath_hip_pipeline_frameshift_domains(self.ctx._h, self.om._h, om_fs3._h, om_fs5._h, dna._h, C.byref(self.params), E_report,
                                                                   C.byref(stats), C.byref(fw), C.byref(nfw), C.byref(dm), C.byref(ndm), C.byref(nskip)),
                        "pipeline_frameshift_domains")
        if arrays:
            def view(ptr, n, T):
                if n == 0:
                    return np.zeros(0, dtype=_np_dtype(T))
                return np.frombuffer((T * n).from_address(C.addressof(ptr.contents)), dtype=_np_dtype(T))
            return stats, view(fw, nfw.value, FsWindow), view(dm, ndm.value, FsDomain), nskip.value

        def copies(ptr, n, T):
            out = []
            for i in range(n):
                x = T()
                C.memmove(C.byref(x), C.byref(ptr[i]), C.sizeof(T))
                out.append(x)
            return out
        return stats, copies(fw, nfw.value, FsWindow), self._domains(dm, ndm.value), nskip.value

    def traces(self):
        """P7_DOMAIN.tr of every domain of the last run_hits / run_frameshift_domains call (bath_hip_domain_traces): a list of
        (DomainTrace copy, st, k, i, c, pp) with numpy copies of the five arrays, entry d for domain d of that call."""
        tr = C.POINTER(DomainTrace)(); n = C.c_int64(0)
        st = C.POINTER(C.c_int8)(); k = _i32p(); i = _i32p(); c = C.POINTER(C.c_int8)(); pp = _f32p()
        self.ctx._check(lib().bath_hip_domain_traces(self.ctx._h, C.byref(tr), C.byref(n), C.byref(st), C.byref(k), C.byref(i), C.byref(c), C.byref(pp)),
                        "domain_traces")
        out = []
        for d in range(n.value):
            t = DomainTrace()
            C.memmove(C.byref(t), C.byref(tr[d]), C.sizeof(DomainTrace))
            sl = slice(t.off, t.off + t.N)
            grab = lambda p, dt: np.ctypeslib.as_array(p, shape=(t.off + t.N,))[sl].astype(dt).copy() if t.N else np.zeros(0, dt)
            out.append((t, grab(st, np.int8), grab(k, np.int32), grab(i, np.int32), grab(c, np.int8), grab(pp, np.float32)))
        return out

    def kernel_times(self):
        """Per-kernel device times of the stages after the cascade in the last run_frameshift_domains call:
        {name: (ms, launches, cells, bytes)}."""
        arr = (KernelTime * 32)()
        n = lib().bath_hip_kernel_times(self.ctx._h, 32, arr)
        return {arr[i].name.decode(): (float(arr[i].ms), int(arr[i].launches), float(arr[i].cells), float(arr[i].bytes)) for i in range(n)}

    def timings(self):
        names = (C.c_char_p * 32)()
        ms = np.zeros(32, dtype=np.float32)
        launches = np.zeros(32, dtype=np.int64)
        k = lib().bath_hip_pipeline_timings(self.ctx._h, 32, names, _f32(ms), _i64(launches))
        return [(names[i].decode(), float(ms[i]), int(launches[i])) for i in range(k)]


def alidisplay_print(trace, window_codes, hmm, sqfrom, sqto, seq_name, gm_fs5=None, gm=None, ncbi_table=1, textw=150, frameline=False,
                     initiator=INIT_ANY):
    """The alignment block of one hit (bath_alidisplay_print: p7_alidisplay_*_Create + p7_alidisplay_Print_BATH).
    trace: one entry of Pipeline.traces() (or the same six things from another source); window_codes: the digital nucleotides of
    windowsq (the strand read, from trace[0].win_start on); gm_fs5 / gm: FSProfile (5 codon lengths) / Profile objects."""
    t, st, k, i, c, pp = trace
    st = np.ascontiguousarray(st, np.int8); k = np.ascontiguousarray(k, np.int32); i = np.ascontiguousarray(i, np.int32)
    c = np.ascontiguousarray(c, np.int8); pp = np.ascontiguousarray(pp, np.float32)
    win = np.ascontiguousarray(window_codes, np.uint8)
    tr = DomainTrace(0, int(t.N), int(t.win_start), int(t.orf_start), int(t.frameshift))
    o = AliDisplayOpts(hmm.name.encode(), seq_name.encode(), hmm.consensus.encode(), hmm.rf.encode() if hmm.rf else None,
                       hmm.cs.encode() if hmm.cs else None, hmm.M, int(sqfrom), int(sqto), textw, 1 if frameline else 0, initiator)
    basic = gencode_basic(ncbi_table)
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
    args = [C.byref(tr), p8(st), k.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p), p8(c), _f32(pp), _u8(win), len(win),
            gm_fs5._p if gm_fs5 is not None else None, gm._p if gm is not None else None, _u8(basic), C.byref(o)]
    n = lib().bath_alidisplay_print(*args, None, 0)
    if n < 0:
        raise BathError("alidisplay_print failed")
    buf = C.create_string_buffer(n + 1)
    lib().bath_alidisplay_print(*args, buf, n)
    return buf.raw[:n].decode()


def frameshift_rows(trace, window_codes, gm_fs5, iali, jali):
    """The --fstblout rows of one hit (bath_trace_frameshift_rows: the loop of p7_tophits_TabularFrameshifts over its trace):
    [(type, length, seq_start, ali_start)], type 'D' / 'I' for a quasi-codon that lacks / has extra nucleotides, 'S' for a stop
    codon in a match state.  trace, window_codes, gm_fs5 as alidisplay_print takes them; a standard-branch trace has no rows."""
    t, st, k, i, c = trace[:5]
    st = np.ascontiguousarray(st, np.int8); k = np.ascontiguousarray(k, np.int32); i = np.ascontiguousarray(i, np.int32)
    c = np.ascontiguousarray(c, np.int8)
    win = np.ascontiguousarray(window_codes, np.uint8)
    tr = DomainTrace(0, int(t.N), int(t.win_start), int(t.orf_start), int(t.frameshift))
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
    args = [C.byref(tr), p8(st), k.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p), p8(c), _u8(win), len(win),
            gm_fs5._p if gm_fs5 is not None else None, int(iali), int(jali)]
    n = lib().bath_trace_frameshift_rows(*args, None, 0)
    if n < 0:
        raise BathError("frameshift_rows failed")
    rows = (FsRow * max(n, 1))()
    lib().bath_trace_frameshift_rows(*args, rows, n)
    return [(rows[x].type.decode(), int(rows[x].length), int(rows[x].seq_start), int(rows[x].ali_start)) for x in range(n)]


class HitArray:
    """The hits of a pipeline call as one numpy record array (dtype of FsDomain) plus the pool their cigar_off fields point into."""

    def __init__(self, rec, pool):
        self.rec, self.pool = rec, pool

    def __len__(self):
        return len(self.rec)

    def to_bytes(self, traces=None):
        """The library's hit stream (bath_hits_serialize: self-delimiting records in network byte order, after p7_hit_Serialize):
        what dist.gather_query_hits ships and what a C host would ship.  traces: one entry of Pipeline.traces() per hit, carried
        in the stream (what the alignment blocks of the main output need; read back by HitArray.traces_from_bytes)."""
        rec = np.ascontiguousarray(self.rec)
        pool = self.pool if self.pool else None
        keep = ()
        if traces is not None and len(rec):
            if len(traces) != len(rec):
                raise BathError("hits_serialize: %d traces for %d hits" % (len(traces), len(rec)))
            tr = (DomainTrace * len(rec))()
            off = 0
            for h, (t, *_a) in enumerate(traces):
                tr[h] = DomainTrace(off, int(t.N), int(t.win_start), int(t.orf_start), int(t.frameshift))
                off += int(t.N)
            cat = [np.ascontiguousarray(np.concatenate([x[j] for x in traces]) if off else np.zeros(1, dt), dt)
                   for j, dt in ((1, np.int8), (2, np.int32), (3, np.int32), (4, np.int8), (5, np.float32))]
            p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
            keep = (tr, cat)
            args = (rec.ctypes.data, len(rec), pool, tr, p8(cat[0]), cat[1].ctypes.data_as(_i32p), cat[2].ctypes.data_as(_i32p), p8(cat[3]),
                    _f32(cat[4]))
        else:
            args = (rec.ctypes.data, len(rec), pool, None, None, None, None, None, None)
        n = lib().bath_hits_serialize(*args, None, 0)
        if n < 0:
            raise BathError("hits_serialize failed")
        buf = C.create_string_buffer(n)
        if lib().bath_hits_serialize(*args, C.addressof(buf), n) != n:
            raise BathError("hits_serialize failed")
        del keep
        return buf.raw

    @staticmethod
    def traces_from_bytes(buf):
        """[(FsDomain, trace)] of a stream written with traces (bath_hits_deserialize, bath_hits_traces): every hit with its
        trace in the form of Pipeline.traces(), as alidisplay_print takes it."""
        h = _vp()
        if lib().bath_hits_deserialize(bytes(buf), len(buf), C.byref(h)) != OK:
            raise BathError("hits_deserialize failed")
        try:
            n = lib().bath_hits_count(h)
            if n == 0:
                return []
            tr = C.POINTER(DomainTrace)(); st = C.POINTER(C.c_int8)(); k = _i32p(); i = _i32p(); c = C.POINTER(C.c_int8)(); pp = _f32p()
            if lib().bath_hits_traces(h, C.byref(tr), C.byref(st), C.byref(k), C.byref(i), C.byref(c), C.byref(pp)) != OK:
                raise BathError("the hit stream carries no traces")
            dom = lib().bath_hits_domains(h)
            out = []
            for d in range(n):
                x = FsDomain()
                C.memmove(C.byref(x), C.byref(dom[d]), C.sizeof(FsDomain))
                t = DomainTrace()
                C.memmove(C.byref(t), C.byref(tr[d]), C.sizeof(DomainTrace))
                sl = slice(t.off, t.off + t.N)
                grab = lambda p, dt: np.ctypeslib.as_array(p, shape=(t.off + t.N,))[sl].astype(dt).copy() if t.N else np.zeros(0, dt)
                out.append((x, (t, grab(st, np.int8), grab(k, np.int32), grab(i, np.int32), grab(c, np.int8), grab(pp, np.float32))))
            return out
        finally:
            lib().bath_hits_destroy(h)

    @staticmethod
    def from_bytes(buf, p=0):
        """(HitArray, position behind the stream) from the stream that starts at buf[p] (bath_hits_deserialize)."""
        view = bytes(buf[p:]) if p else bytes(buf)
        size = lib().bath_hits_stream_size(view, len(view))
        if size < 0:
            raise BathError("not a hit stream")
        h = _vp()
        if lib().bath_hits_deserialize(view, size, C.byref(h)) != OK:
            raise BathError("hits_deserialize failed")
        try:
            n = lib().bath_hits_count(h)
            rec = np.frombuffer((FsDomain * n).from_address(C.addressof(lib().bath_hits_domains(h).contents)), dtype=FS_DOMAIN_DTYPE).copy() if n else np.zeros(0, dtype=FS_DOMAIN_DTYPE)
            k = C.c_int64(0)
            base = lib().bath_hits_cigars(h, C.byref(k))
            pool = C.string_at(base, k.value) if base and k.value else b""
        finally:
            lib().bath_hits_destroy(h)
        return HitArray(rec, pool), p + size

    @staticmethod
    def from_domains(domains):
        """From FsDomain objects carrying .cigar (the object path of run_hits / run_frameshift_domains)."""
        rec = np.zeros(len(domains), dtype=FS_DOMAIN_DTYPE)
        pool = bytearray()
        for i, d in enumerate(domains):
            rec[i] = np.frombuffer(bytes(d), dtype=FS_DOMAIN_DTYPE)[0]
            rec[i]["cigar_off"] = len(pool)
            pool += d.cigar.encode() + b"\0"
        return HitArray(rec, bytes(pool))

    @staticmethod
    def concat(parts):
        """One array from several: every part's cigar offsets moved behind the pools before it."""
        if len(parts) == 1:
            return parts[0]
        recs, pools, shift = [], [], 0
        for h in parts:
            r = h.rec.copy()
            r["cigar_off"][r["cigar_off"] >= 0] += shift            # -1 = the hit came without a CIGAR: stays -1
            recs.append(r); pools.append(h.pool); shift += len(h.pool)
        return HitArray(np.concatenate(recs) if recs else np.zeros(0, dtype=FS_DOMAIN_DTYPE), b"".join(pools))


class TopHits:
    """P7_TOPHITS for this path: collect the hits of pipeline calls, finish the search (E-values, duplicates, sorting,
    thresholds; bathsearch.c:868-921) and print --tblout (p7_tophits_TabularTargets) and --fstblout (p7_tophits_TabularFrameshifts)."""

    def __init__(self):
        self._h = lib().bath_tophits_create()

    def add(self, domains, names, lengths, seqidx0=0, accs=None, descs=None):
        n = len(domains)
        arr = (FsDomain * max(n, 1))()
        pool = bytearray()
        for i, d in enumerate(domains):
            C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(FsDomain))
            arr[i].cigar_off = len(pool)
            pool += d.cigar.encode() + b"\0"
        cig = C.create_string_buffer(bytes(pool) + b"\0")

        def strs(v):
            if v is None:
                return None
            a = (C.c_char_p * len(v))()
            for i, x in enumerate(v):
                a[i] = x.encode() if x else None
            return a
        lens = (C.c_int64 * len(lengths))(*[int(x) for x in lengths])
        st = lib().bath_tophits_add(self._h, arr, n, C.cast(cig, C.c_void_p), seqidx0, strs(names), strs(accs), strs(descs), lens)
        if st != OK:
            raise BathError("tophits_add failed (%d)" % st)

    def add_arrays(self, hits, names, lengths, seqidx0=0):
        """add() for a HitArray: the record array and the CIGAR pool go to the library as they are."""
        n = len(hits)
        if n == 0:
            return
        rec = np.ascontiguousarray(hits.rec)
        a = (C.c_char_p * len(names))(*[x.encode() for x in names])
        lens = (C.c_int64 * len(lengths))(*[int(x) for x in lengths])
        pool = C.create_string_buffer(hits.pool + b"\0")
        st = lib().bath_tophits_add(self._h, rec.ctypes.data_as(C.POINTER(FsDomain)), n, C.cast(pool, C.c_void_p), seqidx0, a, None, None, lens)
        if st != OK:
            raise BathError("tophits_add failed (%d)" % st)

    def add_serialized(self, buf, names, lengths, descs=None, accs=None, window_shift=0, seqidx0=0):
        """add() for a hit stream from another process (bath_tophits_add_serialized): the stream's window fields, plus
        <window_shift>, index <names>; a hit outside them is refused (BathError) and nothing is added."""
        def strs(v):
            if v is None:
                return None
            a = (C.c_char_p * max(len(v), 1))()
            for i, x in enumerate(v):
                a[i] = x.encode() if x else None
            return a
        lens = (C.c_int64 * max(len(lengths), 1))(*[int(x) for x in lengths])
        raw = bytes(buf)
        st = lib().bath_tophits_add_serialized(self._h, raw, len(raw), int(window_shift), len(names), int(seqidx0), strs(names), strs(accs),
                                               strs(descs), lens)
        if st != OK:
            raise BathError("tophits_add_serialized failed (%d)" % st)

    def reported(self):
        return int(lib().bath_tophits_reported(self._h))

    def set_score_thresholds(self, by_E=True, T=0.0, inc_by_E=True, incT=0.0):
        """-T / --incT: report / include by bit score instead of E-value (p7_pli_TargetReportable / Includable)."""
        lib().bath_tophits_set_score_thresholds(self._h, 1 if by_E else 0, T, 1 if inc_by_E else 0, incT)

    def finalize(self, nres, max_length, E=10.0):
        if lib().bath_tophits_finalize(self._h, nres, max_length, E) != OK:
            raise BathError("tophits_finalize failed")

    def hits(self):
        out = []
        for r in range(lib().bath_tophits_count(self._h)):
            d, idx, fl = FsDomain(), C.c_int64(0), C.c_int32(0)
            lib().bath_tophits_get(self._h, r, C.byref(d), C.byref(idx), C.byref(fl))
            out.append((d, idx.value, fl.value))
        return out

    def tblout(self, qname, qacc, M, fs_pipe=False, show_cigar=False, show_header=True):
        args = (self._h, qname.encode(), (qacc or "").encode(), M, int(fs_pipe), int(show_cigar), int(show_header))
        n = lib().bath_tophits_tabular_targets(*args, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().bath_tophits_tabular_targets(*args, buf, n)
        return buf.raw[:n].decode()

    def fstblout(self, qname, qacc, rows_by_reported_hit, show_header=True):
        """--fstblout (p7_tophits_TabularFrameshifts): rows_by_reported_hit[r] is frameshift_rows() of the r-th reported hit in
        the list's current order -- of hits(), those with flag 1.  The header is written only when the list holds a hit."""
        nrep = len(rows_by_reported_hit)
        off = (C.c_int64 * (nrep + 1))()
        flat = [x for rows in rows_by_reported_hit for x in rows]
        arr = (FsRow * max(len(flat), 1))()
        for r, rows in enumerate(rows_by_reported_hit):
            off[r + 1] = off[r] + len(rows)
        for x, (typ, length, seq_start, ali_start) in enumerate(flat):
            arr[x] = FsRow(typ.encode(), int(length), int(ali_start), int(seq_start))
        args = (self._h, qname.encode(), (qacc or "").encode(), arr, off, nrep, int(show_header))
        n = lib().bath_tophits_tabular_frameshifts(*args, None, 0)
        if n < 0:
            raise BathError("tophits_tabular_frameshifts failed: %d row lists for %d reported hits" % (nrep, self.reported()))
        buf = C.create_string_buffer(n + 1)
        lib().bath_tophits_tabular_frameshifts(*args, buf, n)
        return buf.raw[:n].decode()

    def annotations(self, M, fs_pipe=False):
        """Per reported hit, in rank order: the head of its 'Annotation for each hit' entry (p7_tophits_Domains)."""
        out = []
        for r in range(lib().bath_tophits_count(self._h)):
            n = lib().bath_tophits_domain_annotation(self._h, r, M, int(fs_pipe), None, 0)
            if n > 0:
                buf = C.create_string_buffer(n + 1)
                lib().bath_tophits_domain_annotation(self._h, r, M, int(fs_pipe), buf, n)
                out.append(buf.raw[:n].decode())
        return out

    def statistics(self, stats, params, nmodels, nnodes, nseqs):
        """The 'Internal pipeline statistics summary' block of the main output, without its timing lines (p7_pli_Statistics)."""
        args = (self._h, C.byref(stats), C.byref(params), nmodels, nnodes, nseqs)
        n = lib().bath_tophits_pipeline_statistics(*args, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().bath_tophits_pipeline_statistics(*args, buf, n)
        return buf.raw[:n].decode()

    def targets(self, fs_pipe=False, textw=120):
        """The 'Scores for complete hits' block of bathsearch's main output (p7_tophits_Targets)."""
        n = lib().bath_tophits_targets(self._h, int(fs_pipe), textw, None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().bath_tophits_targets(self._h, int(fs_pipe), textw, buf, n)
        return buf.raw[:n].decode()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().bath_tophits_destroy(self._h)
            self._h = None


def FS3ForwardParser(ctx, om3, dna, logsum=LOGSUM_TABLE, want_xmx=False):
    """p7_ForwardParser_Frameshift_3Codons over a block of DNA windows."""
    return _fs3(lib().bath_hip_fs3_forward_parser, "fs3_forward_parser", ctx, om3, dna, logsum, want_xmx)


def FS3BackwardParser(ctx, om3, dna, logsum=LOGSUM_TABLE, want_xmx=False):
    """p7_BackwardParser_Frameshift_3Codons over a block of DNA windows."""
    return _fs3(lib().bath_hip_fs3_backward_parser, "fs3_backward_parser", ctx, om3, dna, logsum, want_xmx)


def _fs3(fn, what, ctx, om3, dna, logsum, want_xmx):
    sc = np.zeros(dna.n, dtype=np.float32)
    xmx, offs = None, None
    if want_xmx:
        offs = np.zeros(dna.n + 1, dtype=np.int64)
        np.cumsum((dna.lengths + 1) * 5, out=offs[1:])
        xmx = np.zeros(int(offs[-1]), dtype=np.float32)
    ctx._check(fn(ctx._h, om3._h, dna._h, logsum, _f32(sc), _f32(xmx), _i64(offs)), what)
    if want_xmx:
        return sc, [xmx[offs[i]:offs[i + 1]].reshape(-1, 5) for i in range(dna.n)]
    return sc


def FS5Envelopes(ctx, om5, dna, logsum=LOGSUM_TABLE, c5_compat=False, want_pp=False, want_oa=False):
    """Forward/Backward/Decoding/OptimalAccuracy/Null2 (frameshift, 5 codon lengths) per envelope."""
    M = om5.M
    res = (Fs5Result * max(dna.n, 1))()
    pp = ppo = oa = oao = None
    if want_pp:
        ppo = np.zeros(dna.n + 1, dtype=np.int64)
        np.cumsum((dna.lengths + 1) * (M + 1) * 8, out=ppo[1:])
        pp = np.zeros(int(ppo[-1]), dtype=np.float32)
    if want_oa:
        oao = np.zeros(dna.n + 1, dtype=np.int64)
        np.cumsum((dna.lengths + 1) * (M + 1) * 3, out=oao[1:])
        oa = np.zeros(int(oao[-1]), dtype=np.float32)
    ctx._check(lib().bath_hip_fs5_envelopes(ctx._h, om5._h, dna._h, logsum, 1 if c5_compat else 0, res,
                                            _f32(pp), _i64(ppo), _f32(oa), _i64(oao)), "fs5_envelopes")
    out = {"fwdsc": np.array([res[i].fwdsc for i in range(dna.n)], dtype=np.float32),
           "bcksc": np.array([res[i].bcksc for i in range(dna.n)], dtype=np.float32),
           "oasc": np.array([res[i].oasc for i in range(dna.n)], dtype=np.float32),
           "null2": np.array([list(res[i].null2) for i in range(dna.n)], dtype=np.float32).reshape(dna.n, KP)}
    if want_pp:
        out["pp"] = [pp[ppo[i]:ppo[i + 1]].reshape(-1, M + 1, 8) for i in range(dna.n)]
    if want_oa:
        out["oa"] = [oa[oao[i]:oao[i + 1]].reshape(-1, M + 1, 3) for i in range(dna.n)]
    return out


def FS5ForwardFull(ctx, om5, dna, cfg_len_amino=100):
    """p7_Forward_Frameshift in the multihit configuration (what the stochastic tracebacks walk): scores, and per sequence the
    matrix (L+1, M+1, 8) {D, I, M_C0, M_C1..M_C5} and the special-state rows (L+1, 5) {E, N, J, B, C}."""
    M = om5.M
    rows = dna.lengths + 1
    fo = np.zeros(dna.n + 1, dtype=np.int64); np.cumsum(rows * (M + 1) * 8, out=fo[1:])
    xo = np.zeros(dna.n + 1, dtype=np.int64); np.cumsum(rows * 5, out=xo[1:])
    sc = np.zeros(dna.n, dtype=np.float32)
    fwd = np.zeros(int(fo[-1]), dtype=np.float32)
    xmx = np.zeros(int(xo[-1]), dtype=np.float32)
    ctx._check(lib().bath_hip_fs5_forward_full(ctx._h, om5._h, dna._h, cfg_len_amino, _f32(sc), _f32(fwd), _f32(xmx)), "fs5_forward_full")
    return sc, [fwd[fo[i]:fo[i + 1]] for i in range(dna.n)], [xmx[xo[i]:xo[i + 1]] for i in range(dna.n)]


STD_FILL_SERIAL, STD_FILL_WAVE, STD_FILL_BLOCK = 0, 1, 2


def StdEnvelopes(ctx, om, seqs, fill=STD_FILL_SERIAL):
    """rescore_isolated_domain_bath's passes over a SeqBlock of amino-acid envelopes (unihit, L = each envelope's length) with the
    domain stage's kernels chosen by <fill>: STD_FILL_SERIAL a lane per envelope, STD_FILL_WAVE std_envelope_fill_kernel<C>,
    STD_FILL_BLOCK std_envelope_fill_mw_kernel<C> (the last two for models of up to 1024 nodes).  Returns the StdResult array and,
    per envelope, the posteriors and the optimal-accuracy matrix (L+1, M+1, 3) {M, D, I} and their special-state rows (L+1, 5)
    {E, N, J, B, C}: what the stage's traceback reads (row 0 of the posteriors is not part of that)."""
    M = om.M
    rows = seqs.lengths.astype(np.int64) + 1
    do = np.zeros(seqs.n + 1, dtype=np.int64); np.cumsum(rows * (M + 1) * 3, out=do[1:])
    xo = np.zeros(seqs.n + 1, dtype=np.int64); np.cumsum(rows * 5, out=xo[1:])
    res = (StdResult * max(seqs.n, 1))()
    pp, oa = np.zeros(int(do[-1]), np.float32), np.zeros(int(do[-1]), np.float32)
    ppx, oax = np.zeros(int(xo[-1]), np.float32), np.zeros(int(xo[-1]), np.float32)
    ctx._check(lib().bath_hip_std_envelopes_fill(ctx._h, om._h, seqs._h, res, _f32(pp), _f32(oa), _f32(ppx), _f32(oax), int(fill)), "std_envelopes_fill")
    mats = lambda a: [a[do[i]:do[i + 1]].reshape(int(rows[i]), M + 1, 3) for i in range(seqs.n)]
    xrows = lambda a: [a[xo[i]:xo[i + 1]].reshape(int(rows[i]), 5) for i in range(seqs.n)]
    return res, mats(pp), mats(oa), xrows(ppx), xrows(oax)


def fs_ensemble_loop_scores(L=100):
    """(xNL, xNM, xE): log loop / move of N, C, J and log 1/2 of the multihit length-L configuration the region stage runs in."""
    pm = np.float32(3.0) / np.float32(L + 3.0)
    return (float(np.float32(np.log(np.float64(np.float32(1.0) - pm)))), float(np.float32(np.log(np.float64(pm)))),
            float(np.float32(-0.69314718055994529)))


def _ens_unpack(n, rs, ts, seg, so, env, eo):
    return [{"status": int(rs[r]), "trace_status": ts[r].copy(), "segments": seg[so[r]:so[r + 1]].copy(),
             "envelopes": [tuple(int(v) for v in e) for e in env[eo[r]:eo[r + 1]]]} for r in range(n)]


def FS5RegionEnsembles(ctx, om5, regions, seed=42):
    """The multi-domain region stage on its own, in the context's set_fs_ensemble mode: per region a dict with status (ENS_REGION_*),
    trace_status [200], segments [(trace, i, j, k, m)] in region coordinates (stream modes only) and envelopes [(i, j)]."""
    n = regions.n
    rs = np.zeros(max(n, 1), np.int32); ts = np.zeros((max(n, 1), ENS_SAMPLES), np.int32)
    so = np.zeros(n + 1, np.int64); eo = np.zeros(n + 1, np.int64)
    max_seg, max_env = 64 * ENS_SAMPLES * max(n, 1), 256 * max(n, 1)
    while True:
        seg = np.zeros((max_seg, 5), np.int32); env = np.zeros((max_env, 2), np.int32)
        p = lambda a: a.ctypes.data_as(_i32p)
        st = lib().bath_hip_fs5_region_ensembles(ctx._h, om5._h, regions._h, seed, p(rs), p(ts), p(seg), max_seg, _i64(so), p(env), max_env, _i64(eo))
        if st != ERANGE:
            break
        max_seg, max_env = max(max_seg, int(so[-1])), max(max_env, int(eo[-1]))
    ctx._check(st, "fs5_region_ensembles")
    return _ens_unpack(n, rs, ts, seg, so, env, eo)


def StdRegionEnsembles(ctx, om, regions, cfg_len=None, seed=42):
    """The standard branch's multi-domain region stage on its own, in the context's set_std_ensemble mode.  regions: a SeqBlock of
    amino-acid sequences, each one region; cfg_len: the length the model is configured for per region (None: the region's own).  Per
    region a dict as FS5RegionEnsembles gives, plus n2corr: the null2 correction of every envelope."""
    n = regions.n
    rs = np.zeros(max(n, 1), np.int32); ts = np.zeros((max(n, 1), ENS_SAMPLES), np.int32)
    so = np.zeros(n + 1, np.int64); eo = np.zeros(n + 1, np.int64)
    cfg = None if cfg_len is None else np.ascontiguousarray(cfg_len, np.int32)
    assert cfg is None or cfg.shape == (n,)
    max_seg, max_env = 64 * ENS_SAMPLES * max(n, 1), 64 * max(n, 1)          # (the twin keeps 64 segments a trace: no second run, which would count fallbacks twice)
    p = lambda a: a.ctypes.data_as(_i32p)
    while True:
        seg = np.zeros((max_seg, 5), np.int32); env = np.zeros((max_env, 2), np.int32); corr = np.zeros(max_env, np.float32)
        st = lib().bath_hip_std_region_ensembles(ctx._h, om._h, regions._h, None if cfg is None else p(cfg), seed, p(rs), p(ts), p(seg), max_seg, _i64(so),
                                                 p(env), _f32(corr), max_env, _i64(eo))
        if st != ERANGE or (int(so[-1]) <= max_seg and int(eo[-1]) <= max_env):
            break
        max_seg, max_env = max(max_seg, int(so[-1])), max(max_env, int(eo[-1]))
    ctx._check(st, "std_region_ensembles")
    out = _ens_unpack(n, rs, ts, seg, so, env, eo)
    for r in range(n):
        out[r]["n2corr"] = corr[eo[r]:eo[r + 1]].copy()
    return out


def std_ensemble_host(mode, M, tf, rf, pmove, tEL, tEM, res, fwd, fx, seed=42):
    """The standard branch's ensemble of one region on caller-supplied tables and matrices (no GPU), mode ENSEMBLE_SERIAL or
    ENSEMBLE_STREAMS_HOST: the dict of StdRegionEnsembles for the region, with n2sc, the per-residue null2 log odds, instead of n2corr.
    Raises BathError where the stream mode does not take the region."""
    tf, rf, fwd, fx = (np.ascontiguousarray(a, np.float32) for a in (tf, rf, fwd, fx))
    res = np.ascontiguousarray(res, np.uint8)
    Lr = len(res)
    assert tf.size >= (M + 1) * 8 and rf.size >= 20 * (M + 1) and fwd.size >= (Lr + 1) * (M + 1) * 3 and fx.size >= (Lr + 1) * 6
    rs, nseg, nenv = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ts = np.zeros(ENS_SAMPLES, np.int32); seg = np.zeros((64 * ENS_SAMPLES, 5), np.int32); env = np.zeros((256, 2), np.int32)
    n2sc = np.zeros(Lr, np.float32)
    p = lambda a: a.ctypes.data_as(_i32p)
    st = lib().bath_selftest_std_ensemble(ENSEMBLE_MODES.get(mode, mode), M, _f32(tf), _f32(rf), pmove, tEL, tEM, _u8(res), Lr, _f32(fwd), _f32(fx), seed,
                                          C.byref(rs), p(ts), p(seg), len(seg), C.byref(nseg), _f32(n2sc), p(env), len(env), C.byref(nenv))
    if st != OK:
        raise BathError("std_ensemble_host failed (%d)" % st)
    return {"status": rs.value, "trace_status": ts, "segments": seg[:nseg.value].copy(), "envelopes": [tuple(int(v) for v in e) for e in env[:nenv.value]],
            "n2sc": n2sc}


def std_ens_walk(M, tf, pmove, tEL, tEM, Lr, fwd, fx, rng_state, max_seg=64):
    """One walk of the standard branch's stream modes from generator state <rng_state>: (status, [(i, j, k, m)] first domain first)."""
    tf, fwd, fx = (np.ascontiguousarray(a, np.float32) for a in (tf, fwd, fx))
    st_, n = C.c_int32(0), C.c_int32(0)
    seg = np.zeros((max_seg, 4), np.int32)
    st = lib().bath_selftest_std_ens_walk(M, _f32(tf), pmove, tEL, tEM, Lr, _f32(fwd), _f32(fx), rng_state, C.byref(st_), seg.ctypes.data_as(_i32p), max_seg, C.byref(n))
    if st != OK:
        raise BathError("std_ens_walk failed (%d)" % st)
    return st_.value, [tuple(int(v) for v in g) for g in seg[:n.value]]


def fs_ensemble_streams(M, tsc, xNL, xNM, xE, ireg, Lr, fwd, fx, seed=42):
    """The host twin of ENSEMBLE_STREAMS_DEVICE on caller-supplied matrices (no GPU): the dict of FS5RegionEnsembles for one region,
    envelopes in window coordinates (shifted by ireg - 1).  Raises BathError(ERANGE) outside the stream rule."""
    tsc, fwd, fx = (np.ascontiguousarray(a, np.float32) for a in (tsc, fwd, fx))
    assert tsc.size >= M * 8 and fwd.size >= (Lr + 1) * (M + 1) * 8 and fx.size >= (Lr + 1) * 5
    rs, nseg, nenv = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ts = np.zeros(ENS_SAMPLES, np.int32); seg = np.zeros((64 * ENS_SAMPLES, 5), np.int32); env = np.zeros((256, 2), np.int32)
    p = lambda a: a.ctypes.data_as(_i32p)
    st = lib().bath_selftest_fs_ensemble_streams(M, _f32(tsc), xNL, xNM, xE, ireg, Lr, _f32(fwd), _f32(fx), seed, C.byref(rs), p(ts), p(seg), len(seg), C.byref(nseg),
                                                 p(env), len(env), C.byref(nenv))
    if st != OK:
        raise BathError("fs_ensemble_streams failed (%d)" % st)
    return {"status": rs.value, "trace_status": ts, "segments": seg[:nseg.value].copy(), "envelopes": [tuple(int(v) for v in e) for e in env[:nenv.value]]}


def fs_ensemble_serial(M, tsc, xNL, xNM, xE, ireg, Lr, fwd, fx, seed=42):
    """The serial ensemble (ENSEMBLE_SERIAL) on caller-supplied matrices (no GPU): its envelopes, window coordinates."""
    tsc, fwd, fx = (np.ascontiguousarray(a, np.float32) for a in (tsc, fwd, fx))
    env = np.zeros((256, 2), np.int32); n = C.c_int32(0)
    st = lib().bath_selftest_fs_ensemble_seeded(M, _f32(tsc), xNL, xNM, xE, ireg, Lr, _f32(fwd), _f32(fx), seed, env.ctypes.data_as(_i32p), len(env), C.byref(n))
    if st != OK:
        raise BathError("fs_ensemble_serial failed (%d)" % st)
    return [tuple(int(v) for v in e) for e in env[:n.value]]


class FsLane(C.Structure):
    """bath_fs_lane: one cascade lane's survivor lists for fs_windows_selftest."""
    _fields_ = [("cands", C.c_void_p), ("wins", C.c_void_p), ("n_c", C.c_int32), ("n_w", C.c_int32), ("cand_base", C.c_int32),
                ("first_window", C.c_int64), ("dpool", C.c_int64)]


FS_CAND_DTYPE = np.dtype([("window", "<i8"), ("aa_off", "<i8"), ("P", "<f8"), ("cand", "<i4"), ("sf", "<i4"), ("startj", "<i4"), ("len", "<i4"),
                          ("fwdsc", "<f4"), ("nullsc", "<f4"), ("fxoff", "<i8")], align=True)                       # bath_fs_cand
FS_HITWIN_DTYPE = np.dtype([("cand", "<i4"), ("n", "<i4"), ("k", "<i4"), ("length", "<i4"), ("score", "<f4")], align=True)   # bath_fs_hitwin
FS_ORF_DTYPE = np.dtype([("w", "<i8"), ("aa_off", "<i8"), ("P", "<f8"), ("cand", "<i4"), ("strand", "<i4"), ("start", "<i4"), ("end", "<i4"), ("n", "<i4"),
                         ("fwd_null", "<f4"), ("wb", "<i4"), ("we", "<i4"), ("dw_n", "<i4"), ("dw_len", "<i4"), ("dw_k", "<i4"), ("kmin", "<i4"), ("kmax", "<i4"),
                         ("g0", "<i4"), ("g1", "<i4"), ("pad_", "<i4")], align=True)                                 # bath_fs_orf
FS_WINDESC_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("seq_n", "<i4"), ("start", "<i4"), ("len", "<i4"), ("strand", "<i4"),
                             ("kmin", "<i4"), ("kmax", "<i4")], align=True)                                          # bath_fs_windesc


def fs_windows_selftest(ctx, om, om_fs3, dna, lanes, nc_total, F3=1e-5, std_pipe=1, driver=0):
    """bath_selftest_fs_windows.  lanes: list of (cands FS_CAND_DTYPE[], wins FS_HITWIN_DTYPE[], cand_base, first_window, dpool).
    Returns (status, None) when the build hands the block back or fails, else (OK, dict): n_orfs, nw, maxlen, pool_bytes, total, orfs
    (FS_ORF_DTYPE), windows (bath_fs_window records), grp [nw][2], voff, vlen, desc (FS_WINDESC_DTYPE)."""
    keep, arr = [], (FsLane * max(len(lanes), 1))()
    n = 0
    for k, (cands, wins, cand_base, first_window, dpool) in enumerate(lanes):
        cands, wins = np.ascontiguousarray(cands, FS_CAND_DTYPE), np.ascontiguousarray(wins, FS_HITWIN_DTYPE)
        keep += [cands, wins]
        arr[k] = FsLane(cands.ctypes.data if len(cands) else None, wins.ctypes.data if len(wins) else None, len(cands), len(wins), cand_base, first_window, dpool)
        n += len(cands)
    m = max(n, 1)
    hdr = np.zeros(6, np.int64)                        # bath_fs_winbuild: 4 int32, 2 int64
    orfs, windows = np.zeros(m, FS_ORF_DTYPE), np.zeros(m, _np_dtype(FsWindow))
    grp, voff, vlen, desc = np.zeros((m, 2), np.int32), np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros(m, FS_WINDESC_DTYPE)
    st = lib().bath_selftest_fs_windows(ctx._h, om._h, om_fs3._h, dna._h, F3, std_pipe, driver, C.addressof(arr), len(lanes), nc_total, hdr.ctypes.data,
                                        orfs.ctypes.data, windows.ctypes.data, grp.ctypes.data_as(_i32p), _i64(voff), vlen.ctypes.data_as(_i32p), desc.ctypes.data)
    if st == ENORESULT:
        return st, None
    ctx._check(st, "selftest_fs_windows")
    h32 = hdr.view(np.int32)
    n_orfs, nw = int(h32[0]), int(h32[1])
    return st, {"n_orfs": n_orfs, "nw": nw, "maxlen": int(h32[2]), "pool_bytes": int(hdr[2]), "total": int(hdr[3]), "orfs": orfs[:n_orfs],
                "windows": windows[:nw], "grp": grp[:nw], "voff": voff[:nw], "vlen": vlen[:nw], "desc": desc[:nw]}


def fs_decide_selftest(ctx, om_fs3, records, bias, fsc, do_biasfilter=1, std_pipe=1, F3=1e-5, driver=0):
    """bath_selftest_fs_decide: a copy of records (bath_fs_window records as a build leaves them) completed by the branch decision."""
    rec = np.ascontiguousarray(records, _np_dtype(FsWindow)).copy()
    bias, fsc = np.ascontiguousarray(bias, np.float32), np.ascontiguousarray(fsc, np.float32)
    assert bias.shape == (len(rec), 2, 3) and fsc.shape == (len(rec),)
    ctx._check(lib().bath_selftest_fs_decide(ctx._h, om_fs3._h, rec.ctypes.data, len(rec), _f32(bias), _f32(fsc), do_biasfilter, std_pipe, F3, driver), "selftest_fs_decide")
    return rec


def rng_jump(seed, n):
    """State of the fast generator n steps after seeding, by jump-ahead."""
    x = C.c_uint32(0)
    if lib().bath_selftest_rng_jump(seed, n, C.byref(x)) != OK:
        raise BathError("rng_jump failed")
    return x.value


def FS5ForwardParser(ctx, om5, dna, cfg_len_amino=100):
    """The score of p7_Forward_Frameshift in the multihit configuration of <cfg_len_amino> per window, and nothing else: no matrix
    leaves the kernel (what calibration needs of p7_ForwardParser_Frameshift_5Codons).  Always strict log-sums."""
    sc = np.zeros(dna.n, dtype=np.float32)
    ctx._check(lib().bath_hip_fs5_forward_parser(ctx._h, om5._h, dna._h, cfg_len_amino, _f32(sc)), "fs5_forward_parser")
    return sc


def FS5ForwardParserOdds(ctx, om5, dna, cfg_len_amino=100):
    """FS5ForwardParser in the reference's arithmetic: the multihit score of the 5-codon odds-ratio Forward (FS5ForwardFull under
    set_fs5_odds, bit for bit) and nothing else.  -inf for a window shorter than 5 nt and for an overflow.  Always odds ratios,
    whatever the context's switches say; a 3-codon profile is refused."""
    sc = np.zeros(dna.n, dtype=np.float32)
    ctx._check(lib().bath_hip_fs5_forward_parser_odds(ctx._h, om5._h, dna._h, cfg_len_amino, _f32(sc)), "fs5_forward_parser_odds")
    return sc


CALIB_SEED, CALIB_L, CALIB_N, CALIB_TAILP = 42, 100, 200, 0.04       # bathconvert.c:128, :157-160
FS_UNSET = -99999.0                                                   # p7_EVPARAM_UNSET: a tau the model file does not carry


def rng_state(seed=CALIB_SEED):
    """The fast generator's state right after seeding: what calib_sample and calibrate_fs carry from model to model."""
    return rng_jump(seed, 0)


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def calib_sample(state, L=CALIB_L, N=CALIB_N, ncbi_table=1, f=None):
    """N background sequences of L amino acids, reverse-translated with a random synonymous codon each (the stream of
    p7_fs_Tau_3codons / _5codons): (codes [N, 3L], the generator's state afterwards).  f: 20 frequencies (None: the background)."""
    st = C.c_uint32(state)
    dna = np.zeros((N, 3 * L), dtype=np.uint8)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    assert fa is None or fa.shape == (20,)
    if lib().bath_calib_sample(C.byref(st), _f32(fa), ncbi_table, L, N, _u8(dna) if dna.size else None) != OK:
        raise BathError("calib_sample failed: unknown translation table %d, or a residue without a codon in it" % ncbi_table)
    return dna, st.value


def calib_skip(state, n_sets=2, L=CALIB_L, N=CALIB_N, ncbi_table=1, f=None):
    """The generator's state after n_sets successive calib_sample calls from <state>, nothing stored: what a model that is passed
    over costs a file's carried generator (its 3-codon and its 5-codon set)."""
    st = C.c_uint32(state)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    assert fa is None or fa.shape == (20,)
    if lib().bath_calib_skip(C.byref(st), _f32(fa), ncbi_table, L, N, n_sets) != OK:
        raise BathError("calib_skip failed: unknown translation table %d, or a residue without a codon in it" % ncbi_table)
    return st.value


def gumbel_fit_complete(x):
    """Maximum-likelihood Gumbel (mu, lambda) of complete data (esl_gumbel_FitComplete)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    mu, lam = C.c_double(0), C.c_double(0)
    st = lib().bath_gumbel_fit_complete(_f64p(x), len(x), C.byref(mu), C.byref(lam))
    if st != OK:
        raise BathError("gumbel_fit_complete failed (%d)" % st)
    return mu.value, lam.value


def gumbel_invcdf(p, mu, lam):
    return lib().bath_gumbel_invcdf(p, mu, lam)


def calib_tau(xv, lambda_model, tailp=CALIB_TAILP):
    """tau of an exponential tail of slope lambda_model from N bit scores (evalues.c:651-658)."""
    x = np.ascontiguousarray(xv, dtype=np.float64)
    tau = C.c_double(0)
    st = lib().bath_calib_tau(_f64p(x), len(x), lambda_model, tailp, C.byref(tau))
    if st != OK:
        raise BathError("calib_tau failed (%d)" % st)
    return tau.value


def bg_fs_nullone(L_amino):
    return lib().bath_bg_fs_nullone(L_amino)


def hmm_max_length(hmm, emit_thresh=1e-7):
    """p7_Builder_MaxLength: MAXL of a model file that has none."""
    return lib().bath_hmm_max_length(hmm._p, emit_thresh)


def kernel_times(ctx):
    """Per-kernel device times recorded on the context since its spans were last reset (calibrate_fs resets them on entry):
    {name: (ms, launches, cells, bytes)}."""
    arr = (KernelTime * 32)()
    n = lib().bath_hip_kernel_times(ctx._h, 32, arr)
    return {arr[i].name.decode(): (float(arr[i].ms), int(arr[i].launches), float(arr[i].cells), float(arr[i].bytes)) for i in range(n)}


def calib_fit_scores(state, score, nullsc, L=CALIB_L, N=CALIB_N, ncbi_table=1, f=None):
    """The reference's redraw loop (evalues.c:633-649) over a Python scorer: score(dna [n, 3L] uint8) -> n float scores, one call per
    batch of sequences still missing; a sequence whose score is not finite is discarded and the next one is drawn from where the
    generator stands after it.  Returns (xv [N] bit scores, the generator's state afterwards, sequences redrawn); BathError
    (.status = ERANGE) when more than N were discarded."""
    def cb(_user, dna, n, L3, sc):
        try:
            got = np.asarray(score(np.ctypeslib.as_array(dna, shape=(n, L3))), dtype=np.float32)
            assert got.shape == (n,)
            np.ctypeslib.as_array(sc, shape=(n,))[:] = got
            return OK
        except Exception as e:                             # (an exception must not cross the C frames)
            err.append(e)
            return EINVAL
    err = []
    st = C.c_uint32(state)
    xv = np.zeros(N, np.float64)
    nre = C.c_int(0)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    assert fa is None or fa.shape == (20,)
    rc = lib().bath_calib_fit_scores(C.byref(st), _f32(fa), ncbi_table, L, N, _CALIB_SCORE_FN(cb), None, nullsc, _f64p(xv), C.byref(nre))
    if err:
        raise err[0]
    if rc != OK:
        e = BathError("calib_fit_scores failed (%d)%s" % (rc, ": more than N sequences had no finite score" if rc == ERANGE else ""))
        e.status, e.redrawn = rc, nre.value
        raise e
    return xv, st.value, nre.value


def calibrate_fs(ctx, hmm, ncbi_table, state, L=CALIB_L, N=CALIB_N, tailp=CALIB_TAILP, want_xv=False, arith="strict"):
    """p7_fs_Tau_3codons then p7_fs_Tau_5codons of one model on the GPU: (tau3, tau5, the generator's state afterwards), with
    want_xv also the two arrays of N bit scores the taus were fitted to and, in the odds modes, [sequences redrawn in the 3-codon
    fit, in the 5-codon fit] (strict has no redraw and keeps its five values).  arith (ARITH_MODES): "strict", the log-space parsers (nothing is ever redrawn); "odds3", the 3-codon parser in fp32 odds
    ratios; "odds", both parsers -- the reference's arithmetic, with its redraw of a sequence whose parser overflows."""
    if arith not in ARITH_MODES:
        raise ValueError("arith: expected one of %s" % ", ".join(ARITH_MODES))
    st = C.c_uint32(state)
    t3, t5 = C.c_double(0), C.c_double(0)
    x3 = np.zeros(N, np.float64) if want_xv else None
    x5 = np.zeros(N, np.float64) if want_xv else None
    px3, px5 = None if x3 is None else _f64p(x3), None if x5 is None else _f64p(x5)
    re2 = (C.c_int * 2)(0, 0)
    if arith == "strict":
        ctx._check(lib().bath_hip_calibrate_fs(ctx._h, hmm._p, ncbi_table, C.byref(st), L, N, tailp, C.byref(t3), C.byref(t5), px3, px5), "calibrate_fs")
    else:
        ctx._check(lib().bath_hip_calibrate_fs_arith(ctx._h, hmm._p, ncbi_table, C.byref(st), L, N, tailp, C.byref(t3), C.byref(t5), px3, px5,
                                                     ARITH_MODES[arith], re2), "calibrate_fs")
    if want_xv and arith != "strict":
        return t3.value, t5.value, st.value, x3, x5, [re2[0], re2[1]]
    return (t3.value, t5.value, st.value, x3, x5) if want_xv else (t3.value, t5.value, st.value)


CALIB_BATCH_MAX = 64                                                  # BATH_CALIB_BATCH_MAX: models per calibrate_fs_batch call


def calib_sample_batch(state, ncbi_tables, L=CALIB_L, N=CALIB_N, f=None):
    """The stream that len(ncbi_tables) successive calibrate_fs calls draw, in their order: per model its 3-codon set, then its
    5-codon set, each model with its own table.  (codes [n, 2, N, 3L], the generator's state afterwards); on error the state the
    caller holds is what it was."""
    tabs = np.ascontiguousarray(ncbi_tables, dtype=np.int32).reshape(-1)
    st = C.c_uint32(state)
    dna = np.zeros((len(tabs), 2, N, 3 * L), dtype=np.uint8)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    assert fa is None or fa.shape == (20,)
    if lib().bath_calib_sample_batch(C.byref(st), _f32(fa), tabs.ctypes.data_as(C.POINTER(C.c_int)), len(tabs), L, N, _u8(dna) if dna.size else _u8(np.zeros(1, np.uint8))) != OK:
        raise BathError("calib_sample_batch failed: an unknown translation table among %s, or a residue without a codon in one" % (list(map(int, tabs)),))
    return dna, st.value


def calibrate_fs_batch(ctx, hmms, ncbi_tables, state, L=CALIB_L, N=CALIB_N, tailp=CALIB_TAILP, want_xv=False):
    """calibrate_fs of several models (at most CALIB_BATCH_MAX) with the windows of all of them in each parser launch: what
    len(hmms) successive calibrate_fs calls with the state carried return, bit for bit, strict arithmetic only.
    (tau3 [n], tau5 [n], the generator's state afterwards), with want_xv also the bit scores xv3 [n, N], xv5 [n, N].  All or
    nothing: a BathError names the position in the batch of the model it is about, and the caller's state is what it was."""
    hmms = list(hmms)
    n = len(hmms)
    tabs = np.ascontiguousarray(ncbi_tables, dtype=np.int32).reshape(-1)
    if len(tabs) != n:
        raise ValueError("calibrate_fs_batch: %d models, %d translation tables" % (n, len(tabs)))
    st = C.c_uint32(state)
    ptrs = (C.POINTER(_Hmm) * max(n, 1))(*[h._p for h in hmms])
    t3, t5 = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
    x3 = np.zeros((max(n, 1), N), np.float64) if want_xv else None
    x5 = np.zeros((max(n, 1), N), np.float64) if want_xv else None
    ctx._check(lib().bath_hip_calibrate_fs_batch(ctx._h, ptrs, tabs.ctypes.data_as(C.POINTER(C.c_int)), n, C.byref(st), L, N, tailp, _f64p(t3), _f64p(t5),
                                                 None if x3 is None else _f64p(x3), None if x5 is None else _f64p(x5)), "calibrate_fs_batch")
    return (t3[:n], t5[:n], st.value, x3[:n], x5[:n]) if want_xv else (t3[:n], t5[:n], st.value)


def calibrate_fs_batch_at(ctx, hmms, ncbi_tables, states, L=CALIB_L, N=CALIB_N, tailp=CALIB_TAILP, want_xv=False):
    """calibrate_fs of several models (at most CALIB_BATCH_MAX), each from a generator state of its own, with the windows of all of
    them in each parser launch: per model what calibrate_fs(ctx, hmms[k], ncbi_tables[k], states[k]) returns, bit for bit, strict
    arithmetic only.  Models with one (state, table) share one pair of sample sets on the device.  (tau3 [n], tau5 [n], the state
    behind each model's samples [n]), with want_xv also xv3 [n, N], xv5 [n, N].  All or nothing: a BathError names the position in
    the batch of the model it is about."""
    hmms = list(hmms)
    n = len(hmms)
    tabs = np.ascontiguousarray(ncbi_tables, dtype=np.int32).reshape(-1)
    s_in = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1)
    if len(tabs) != n or len(s_in) != n:
        raise ValueError("calibrate_fs_batch_at: %d models, %d translation tables, %d generator states" % (n, len(tabs), len(s_in)))
    tabs, s_in = np.append(tabs, np.int32(1)), np.append(s_in, np.uint32(0))                # (n = 0: the library refuses, not a null pointer)
    s_out = np.zeros(n + 1, np.uint32)
    ptrs = (C.POINTER(_Hmm) * max(n, 1))(*[h._p for h in hmms])
    t3, t5 = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
    x3 = np.zeros((max(n, 1), N), np.float64) if want_xv else None
    x5 = np.zeros((max(n, 1), N), np.float64) if want_xv else None
    u32p = C.POINTER(C.c_uint32)
    ctx._check(lib().bath_hip_calibrate_fs_batch_at(ctx._h, ptrs, tabs.ctypes.data_as(C.POINTER(C.c_int)), n, s_in.ctypes.data_as(u32p), s_out.ctypes.data_as(u32p),
                                                    L, N, tailp, _f64p(t3), _f64p(t5), None if x3 is None else _f64p(x3), None if x5 is None else _f64p(x5)),
               "calibrate_fs_batch_at")
    out = [int(s) for s in s_out[:n]]
    return (t3[:n], t5[:n], out, x3[:n], x5[:n]) if want_xv else (t3[:n], t5[:n], out)


# ---- single-sequence models and their calibration: what bath_amd.bathbuild calls
CALIB_DEFAULTS = {"EmL": 200, "EmN": 200, "EvL": 200, "EvN": 200, "EfL": 100, "EfN": 200, "Eft": 0.04}   # p7_builder.c:116-122
SEQ_COMLOG = "[HMM created from a query sequence]"                     # seqmodel.c:54
DEGENERATE_AMINO = "BJZOUX"


def scorematrix_builtin(name="BLOSUM62"):
    """The NCBI-format text of a built-in score matrix (BLOSUM62 is the only one); BathError for any other name."""
    t = lib().bath_scorematrix_builtin(name.encode())
    if t is None:
        raise BathError("no matrix named %s is available as a built-in" % name)
    return t.decode()


class ScoreSystem:
    """p7_builder_LoadScoreSystem / _SetScoreSystem: a substitution matrix (built-in name, or an NCBI-format file) as conditional
    probabilities against the background, with the gap-open and gap-extend probabilities.  BathError carries the reference's message."""

    def __init__(self, mx="BLOSUM62", mxfile=None, popen=0.02, pextend=0.4):
        h, err = C.c_void_p(), C.create_string_buffer(1024)
        st = lib().bath_scoresystem_create(None if mx is None else mx.encode(), None if mxfile is None else os.fsencode(mxfile),
                                           popen, pextend, C.byref(h), err, len(err))
        if st != OK:
            e = BathError(err.value.decode() or "cannot set the score system (status %d)" % st)
            e.status = st
            raise e
        self._h, self.popen, self.pextend = h, popen, pextend
        self.lambda_ = lib().bath_scoresystem_lambda(h)

    def conditionals(self):
        """P(b | a) [20, 20] float64: row a is the match emission vector of a query residue a before it is narrowed to float."""
        q = np.zeros((K, K), np.float64)
        lib().bath_scoresystem_conditionals(self._h, _f64p(q))
        return q

    def __del__(self):
        if getattr(self, "_h", None):
            lib().bath_scoresystem_destroy(self._h)
            self._h = None


def strip_query(seq):
    """p7_SingleBuilder:513-524: the residues of a query with every non-residue symbol (gap, *, ~) dropped, as codes 0..19.  A
    degenerate code (BJZOUX) is refused by name: the reference indexes outside its K x K matrix there.  A symbol outside the
    amino alphabet is refused too."""
    codes = digitize(seq, AMINO_SYMS)
    bad = sorted({AMINO_SYMS[c] for c in codes if 21 <= c <= 26})
    if bad:
        raise BathError("the query holds the degenerate residue code%s %s: a single-sequence model has no emission row for it" %
                        ("s" if len(bad) > 1 else "", ", ".join(bad)))
    return np.ascontiguousarray(codes[codes < K])


def seq_model(score, seq, name, ct=1):
    """p7_SingleBuilder up to calibration: the HMM of one protein sequence (a string, or residue codes 0..19) under a ScoreSystem --
    p7_Seqmodel, p7_hmm_SetComposition, p7_hmm_SetConsensus -- in memory, uncalibrated, MAXL unset."""
    codes = strip_query(seq) if isinstance(seq, str) else np.ascontiguousarray(seq, dtype=np.uint8)
    if len(codes) < 1:
        raise BathError("the query %s holds no residue" % name)
    p = C.POINTER(_Hmm)()
    st = lib().bath_hmm_from_sequence(score._h, _u8(codes), len(codes), name.encode(), ct, C.byref(p))
    if st == ERANGE:
        raise BathError("the query's name %s... is longer than the 127 bytes a model's NAME holds" % name[:24])
    if st != OK:
        raise BathError("cannot build a model from the query %s (status %d)" % (name, st))
    return HMM._from_pointer(p)


def hmm_relent(hmm):
    """p7_MeanMatchRelativeEntropy: bits per match state (the summary's re/pos)."""
    return lib().bath_hmm_mean_match_relent(hmm._p)


def hmm_position_relent(hmm):
    """p7_MeanPositionRelativeEntropy: bits per match position weighted by occupancy, entry transitions counted (bathstat's re/pos)."""
    return lib().bath_hmm_mean_position_relent(hmm._p)


def hmm_lambda(hmm):
    """p7_Lambda: ln 2 + 1.44 / (M * re/pos)."""
    return lib().bath_hmm_lambda(hmm._p)


def hmm_set_max_length(hmm, maxl):
    hmm._p.contents.max_length = hmm.max_length = int(maxl)


def hmm_set_evparam(hmm, evparam):
    """Stores eight E-value parameters (MSV mu, lambda, Viterbi mu, lambda, Forward tau, lambda, FS3 tau, FS5 tau) as floats."""
    ev = np.asarray(evparam, dtype=np.float32)
    assert ev.shape == (NEVPARAM,)
    for i in range(NEVPARAM):
        hmm._p.contents.evparam[i] = float(ev[i])
    hmm.evparam = ev.copy()


def hmm_text(hmm, nseq=1, eff_nseq=1.0, desc=None, date=None, comlog=SEQ_COMLOG):
    """p7_hmmfile_WriteASCII in the BATH3/f format: the whole model's text (bytes)."""
    enc = lambda v: None if v is None else v.encode("latin-1")
    args = (hmm._p, nseq, eff_nseq, enc(desc), enc(date), enc(comlog))
    n = lib().bath_hmm_write_ascii(*args, None, 0)
    if n < 0:
        raise BathError("the model cannot be written")
    buf = C.create_string_buffer(n)
    lib().bath_hmm_write_ascii(*args, buf, n)
    return buf.raw


def calib_sample_amino(state, L, N, f=None):
    """N background sequences of L residues (esl_rsq_xfIID, the stream of p7_MSVMu / p7_ViterbiMu / p7_Tau): (codes [N, L], the
    generator's state afterwards)."""
    st = C.c_uint32(state)
    aa = np.zeros((N, L), dtype=np.uint8)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    if lib().bath_calib_sample_amino(C.byref(st), _f32(fa), L, N, _u8(aa) if aa.size else None) != OK:
        raise BathError("calib_sample_amino failed")
    return aa, st.value


def gumbel_fit_complete_loc(x, lam):
    """esl_gumbel_FitCompleteLoc: the ML mu of a Gumbel of known lambda."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    mu = C.c_double(0)
    st = lib().bath_gumbel_fit_complete_loc(_f64p(x), len(x), lam, C.byref(mu))
    if st != OK:
        raise BathError("gumbel_fit_complete_loc failed (%d)" % st)
    return mu.value


class CalibSamples:
    """The three standard sample sets of a calibration, resident on the device: drawn once from <state> (.state_after: the generator
    behind them), handed to every calibrate() call of a run that reseeds its generator per model."""

    def __init__(self, ctx, state, EmL=200, EmN=200, EvL=200, EvN=200, EfL=100, EfN=200):
        st, h = C.c_uint32(state), C.c_void_p()
        ctx._check(lib().bath_hip_calib_samples_create(ctx._h, C.byref(st), EmL, EmN, EvL, EvN, EfL, EfN, C.byref(h)), "calib_samples_create")
        self._h, self._ctx, self.state_before, self.state_after = h, ctx, state, st.value

    def close(self):
        if getattr(self, "_h", None):
            lib().bath_hip_calib_samples_destroy(self._h)
            self._h = None

    __del__ = close


def calibrate(ctx, hmm, ncbi_table, state, samples=None, EmL=200, EmN=200, EvL=200, EvN=200, EfL=100, EfN=200, Eft=0.04, arith="strict",
              want_xv=False, fs=True):
    """p7_Calibrate of a model in memory, on the GPU: lambda, the MSV and Viterbi mus, the Forward tau and the two frameshift taus
    are stored in the model (hmm.evparam).  Returns the generator's state afterwards; with want_xv also the bit scores the five
    fits saw, {"msv", "vit", "fwd", "fs3", "fs5"}.  samples: a CalibSamples drawn from <state> with these lengths and counts, or
    None to draw the three standard sets for this call.
    fs=False: the standard fits alone (bath_hip_calibrate_std), what the reference's search-time builder runs without --fs and
    --hmmout: evparam[0:6] as with fs=True bit for bit, evparam[6:8] unset (FS_UNSET), no frameshift sample drawn and no frameshift
    parser launched; the state returned is the one behind the three standard sets, want_xv gives {"msv", "vit", "fwd"}, and
    ncbi_table and arith are not read."""
    if arith not in ARITH_MODES:
        raise ValueError("arith: expected one of %s" % ", ".join(ARITH_MODES))
    st = C.c_uint32(state)
    n = [EmN, EvN, EfN, EfN, EfN] if fs else [EmN, EvN, EfN]
    xv = np.zeros(sum(n), np.float64) if want_xv else None
    re2 = (C.c_int * 2)(0, 0)
    if fs:
        ctx._check(lib().bath_hip_calibrate(ctx._h, hmm._p, ncbi_table, C.byref(st), None if samples is None else samples._h,
                                            EmL, EmN, EvL, EvN, EfL, EfN, Eft, ARITH_MODES[arith], None if xv is None else _f64p(xv), re2), "calibrate")
    else:
        ctx._check(lib().bath_hip_calibrate_std(ctx._h, hmm._p, C.byref(st), None if samples is None else samples._h,
                                                EmL, EmN, EvL, EvN, EfL, EfN, Eft, None if xv is None else _f64p(xv)), "calibrate")
    hmm.evparam = np.array(hmm._p.contents.evparam[:], dtype=np.float32)
    if not want_xv:
        return st.value
    cut = np.cumsum([0] + n)
    return st.value, {k: xv[cut[i]:cut[i + 1]].copy() for i, k in enumerate(("msv", "vit", "fwd", "fs3", "fs5")[:len(n)])}


def calibrate_batch(ctx, hmms, ncbi_table, state, samples, EmL=200, EmN=200, EvL=200, EvN=200, EfL=100, EfN=200, Eft=0.04, want_xv=False,
                    fs=True):
    """calibrate of several models (at most CALIB_BATCH_MAX) per kernel launch, for a run that reseeds its generator per model: every
    model starts from <state> and reads the sets of <samples> (a CalibSamples drawn from <state>, required) and one pair of
    frameshift sets behind them.  What len(hmms) calibrate calls from <state> in strict arithmetic give, bit for bit: evparam is
    stored in every model.  Returns the generator's state afterwards (the state one calibrate call leaves); with want_xv also a list
    of the five-key dicts calibrate returns, one per model.  All or nothing: a BathError names the position in the batch of the
    model it is about, and no model is changed.
    fs=False: what len(hmms) calibrate(fs=False) calls give (bath_hip_calibrate_std_batch): the three standard launches per tiling
    and nothing else; models up to the filter cascade's 2048 nodes."""
    hmms = list(hmms)
    n = len(hmms)
    st = C.c_uint32(state)
    ptrs = (C.POINTER(_Hmm) * max(n, 1))(*[h._p for h in hmms])
    sizes = [EmN, EvN, EfN, EfN, EfN] if fs else [EmN, EvN, EfN]
    xv = np.zeros((max(n, 1), sum(sizes)), np.float64) if want_xv else None
    if fs:
        ctx._check(lib().bath_hip_calibrate_batch(ctx._h, ptrs, n, ncbi_table, C.byref(st), None if samples is None else samples._h,
                                                  EmL, EmN, EvL, EvN, EfL, EfN, Eft, None if xv is None else _f64p(xv)), "calibrate_batch")
    else:
        ctx._check(lib().bath_hip_calibrate_std_batch(ctx._h, ptrs, n, C.byref(st), None if samples is None else samples._h,
                                                      EmL, EmN, EvL, EvN, EfL, EfN, Eft, None if xv is None else _f64p(xv)), "calibrate_batch")
    for h in hmms:
        h.evparam = np.array(h._p.contents.evparam[:], dtype=np.float32)
    if not want_xv:
        return st.value
    cut = np.cumsum([0] + sizes)
    return st.value, [{k: xv[m, cut[i]:cut[i + 1]].copy() for i, k in enumerate(("msv", "vit", "fwd", "fs3", "fs5")[:len(sizes)])} for m in range(n)]
