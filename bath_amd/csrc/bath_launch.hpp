// bath_launch.hpp -- host-side launchers and stage entry points shared between the units (bath_filters.hip, bath_pipeline.hip,
// bath_fs_stage.hip and the stages behind them).
#pragma once
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "bath_common.hpp"

namespace bath {

struct Cand {
  int64_t *window;  int32_t *sf;      // strand*3+frame
  int32_t *startj;  int32_t *len;     // first codon index within the stream, length in aa
  int16_t *v;                         // raw SSV maximum
  int64_t *off;                       // offset of the amino-acid sequence in the pool
  int32_t *msv_status, *vit_status, *fwd_status, *stage, *flags;
  float *usc, *nullsc, *filtersc, *vfsc, *fwdsc;
  double *P;
  int32_t *kminmax;                   // [2*cap]
};

// ORF records of a cascade pass, built and ordered on the device (bath_records.hip): one bath_orf_result per candidate with
// stage >= 1, ordered by (window, strand, frame, start); *d_out stays valid until the next call on ctx
int build_orf_records(bath_hip_ctx *ctx, const Cand &cand, int nc, int64_t window_offset, bath_orf_result **d_out, int64_t *n_out);

struct VitWindowArgs {            // p7_ViterbiFilter_BATH's extra inputs/outputs (vitfilter.c:286)
  double invP_vit, invP_msv;
  const float *d_filtersc;        // [n] indexed by sequence id
  const uint8_t *d_ssv_scores;    // [(M+1)*Kp]
  void *d_wins;                   // WindowRec[win_cap]
  int *d_win_count;
  int win_cap;
  int32_t *d_kminmax;             // [2n] min start node / max end node over the target's windows
};

// BATH_OK, or BATH_EINVAL with the context's error set: the model's SSV cost table exceeds a workgroup's LDS (beyond kSsvMaxNodes nodes)
int ssv_table_fits(bath_hip_ctx *ctx, const bath_hip_oprofile *om);
int launch_ssv_lane(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_order, int16_t *d_v);
int launch_ssv_classify(bath_hip_ctx *ctx, const bath_hip_oprofile *om, int64_t n, const int32_t *d_len, const int16_t *d_v, float *d_sc, int32_t *d_status);
int launch_msv_wave(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, float *d_sc, int32_t *d_status, const int *ntodo_dev, bool lane_ok = true);
// the same with a lane per target (bath_msv_lane.hip): BATH_OK, an error, or BATH_ENORESULT when the model does not fit a lane's tile
int launch_msv_lane(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, float *d_sc, int32_t *d_status, const int *ntodo_dev);
bool msv_stage_supported(const bath_hip_oprofile *om);          // the model fits a lane's tile: launch_msv_lane and the cascade's msv_stage_kernel apply
int launch_vit_wave(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, float *d_sc, int32_t *d_status,
                    const VitWindowArgs *wa, const int *ntodo_dev);
int launch_fwd_wave(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, float *d_sc, int32_t *d_status, const int *ntodo_dev,
                    float *d_xmx = nullptr, const int64_t *d_xmx_off = nullptr, float *d_dp = nullptr, const int64_t *d_dp_off = nullptr, int unihit = 0,
                    const int32_t *d_cfg_len = nullptr);
// Forward with a quarter wave per target, four targets of a length-sorted list per wave (bath_fwd_group.hip): models of up to
// kFwdGroupMaxNodes nodes, scores only (no rows, no matrix).  <d_sorted>: the list, longest first (launch_len_sort); its length is
// *ntodo_dev, or <ntodo> where that is null; <ntodo> bounds it either way.  <d_next>: an int that is zero when the kernel starts (its
// waves count the jobs they take beyond their first in it).
constexpr int kFwdGroupMaxNodes = 160;
bool fwd_group_supported(const bath_hip_oprofile *om);
int launch_fwd_group(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_sorted, int64_t ntodo, const int *ntodo_dev, int *d_next, float *d_sc, int32_t *d_status);
int launch_bwd_wave(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, int64_t n, const float *d_fwd_xmx, const int64_t *d_xmx_off,
                    float *d_sc, int32_t *d_status, float *d_bck_xmx, float *d_dp = nullptr, const int64_t *d_dp_off = nullptr, int unihit = 0);
int launch_bias_lane(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const float *d_eo, int eo_stride, const int32_t *d_todo, int64_t ntodo,
                     float *d_nullsc, float *d_filtersc);

int vit_lane_supported(const bath_hip_oprofile *om);
int launch_len_sort(bath_hip_ctx *ctx, const int32_t *d_todo, const int *d_ntodo, const int32_t *d_len, int *d_bins, int32_t *d_sorted);
int launch_vit_lane(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, const int *ntodo_dev,
                    float *d_sc, int32_t *d_status, const VitWindowArgs *wa, const int *skip_dev = nullptr);
const int *len_sort_count_longer(const int *d_bins, int T);     // device pointer: after launch_len_sort, the number of targets longer than T
int64_t lane_min_nt();                                           // blocks of fewer nucleotides keep the wave-per-target kernels (BATH_HIP_LANE_MIN_NT)
const char *vit_lane_kernel_name(const bath_hip_oprofile *om);   // "vit_lane_kernel<NR>" with the NR launch_vit_lane dispatches to
// length sort, the long targets to launch_vit_wave on the side stream (then <beside>, if any, behind it), the rest to launch_vit_lane, join
int launch_vit_sorted(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t cap, const int *d_ntodo, const int32_t *d_len,
                      int *d_bins, int32_t *d_sorted, float *d_sc, int32_t *d_status, const VitWindowArgs *wa, const std::function<int(hipStream_t)> &beside);
struct MsvConsts;
MsvConsts msv_consts(const bath_hip_oprofile *om);
struct VitConsts;
VitConsts vit_consts(const bath_hip_oprofile *om);
constexpr size_t kWaveTableLdsMax = 150 * 1024;      // Forward / Backward tables above this stay in global memory (160 KB of LDS per CU)

// ---- one standard sample set against several models per launch (bath_calib_batch.hip: calibration of a batch, bath_calibrate.hip)
// One model of such a launch is a StdBatchModel: what msv_wave_kernel, vit_wave_kernel and fwd_wave_kernel take as arguments, read by
// a block from a device array at blockIdx.y.  std_batch_model_fill writes one (std_batch_model_bytes bytes) for the host to upload;
// d_sc / d_status: [0] MSV, [1] Viterbi, [2] Forward, a value per target of that filter's set.  The model's length tables are there.
size_t std_batch_model_bytes();
void std_batch_model_fill(void *dst, const bath_hip_oprofile *om, float *const d_sc[3], int32_t *const d_status[3]);
// launch_fwd_wave's choice for this model: its tables stay in global memory (fwd_wave_kernel<C, true>)
bool fwd_wave_global_tables(const bath_hip_oprofile *om);
// d_models[n_models], all of the wave tiling <Cv> (Forward: and all with the same fwd_wave_global_tables, <gt>) and none longer
// than <Mmax>; filter 0 MSV, 1 Viterbi, 2 Forward, over the set <v>: one launch, grid (blocks over v.n, n_models)
int launch_std_wave_batch(bath_hip_ctx *ctx, hipStream_t stream, int filter, const void *d_models, int n_models, int Mmax, int Cv, bool gt, SeqView v);

// ---- what the two branches' domain stages share (bath_domaindef.hip: the frameshift branch, bath_std_domains.hip: the standard one)
constexpr double kLn2 = 0.69314718055994529;
inline double exp_logsurv(double x, double mu, double lambda) { return x < mu ? 0.0 : -lambda * (x - mu); }
// The --cigar string of an alignment, from one code per column: state | codon length << 4 | indel label << 8 (bath_domaindef.hip)
std::string cigar_from_columns(const uint16_t *S, int n);

// pli->nres as the reference's serial loop has it when it searches strand s of window w: every earlier window's W on both strands, this
// window's W once (top strand) or twice (bathsearch.c:1071, :1084; windows under 15 nt are skipped before the count, :1066), on top
// of what the search counted before this block.  pli->Z = (float) nres / (float) max_length (p7_domaindef.c:1033, p7_pipeline.c:1246).
struct RunningZ {
  std::vector<int64_t> before;          // [nwin] residues counted before window w
  const bath_hip_seqs *dna;
  int strands;                          // pli->strands: a window's W is counted once per strand SEARCHED (bathsearch.c:1069-1071, :1082-1084)
  RunningZ(const bath_hip_seqs *d, int64_t nres_before, int strands_ = BATH_STRAND_BOTH) : before((size_t)d->n), dna(d), strands(strands_) {
    int64_t acc = nres_before;
    const int per_window = strands == BATH_STRAND_BOTH ? 2 : 1;
    for (int64_t w = 0; w < d->n; w++) { before[(size_t)w] = acc; acc += per_window * W(w); }
  }
  int64_t W(int64_t w) const {
    const int n = dna->h_len[(size_t)w];
    return n < 15 ? 0 : (int64_t)(n - (dna->h_context.empty() ? 0 : dna->h_context[(size_t)w]));
  }
  float Z(int64_t w, int strand, int max_length) const {
    return (float)(before[(size_t)w] + ((strand && strands == BATH_STRAND_BOTH) ? 2 : 1) * W(w)) / (float)max_length;
  }
};

// What the domain stage reads of the pipeline's option state (bath_pipeline_params + the -E argument)
struct DomOpts {
  int64_t nres_before; double E; int do_null2, inc_by_E, strands; uint32_t seed; double T;
  DomOpts(const bath_pipeline_params &p, double E_report)
      : nres_before(p.nres_before), E(E_report), do_null2(p.do_null2), inc_by_E(p.inc_by_E), strands(p.strands), seed((uint32_t)p.seed), T(p.T) {}
  // p7_pipeline.c:1080, :1247: the early reporting test goes by inc_by_E (sic), against E with the running Z or against T
  bool reportable(double lnP, float Zf, float score) const { return inc_by_E ? (std::exp(lnP) * (double)Zf <= E) : ((double)score >= T); }
};

// Domain definition and hit scores of the standard branch (bath_std_domains.hip) for ORFs that passed the Forward filter, their
// residues in <d_pool>; appends to ctx->fs_domains, ctx->cigars and the context's traces
int std_domains(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const std::vector<PipelineSurvivor> &surv,
                const uint8_t *d_pool, const DomOpts &opt, int64_t *n_clustered_regions);

// ---- DNA regions gathered into a pool for the frameshift kernels (bath_fs_stage.hip)
struct FsWinDev {                  // one DNA window / envelope, device view
  int64_t src_off;                 // offset of its sequence in the DNA block
  int64_t dst_off;                 // offset of the region's copy in the pool
  int32_t seq_n, start, len, strand, kmin, kmax;   // start: 1-based on the strand being read
};
int fs_gather_view(bath_hip_ctx *ctx, const bath_hip_seqs *dna, std::vector<FsWinDev> &regs, const uint8_t *d_comp, bath_hip_seqs *view, const FsWinDev **d_desc_out);

// ---- the DNA windows of the frameshift stage (bath_fs_windows.hip): built by kernels, or on the host for the blocks they do not take
struct WindowRec;                  // bath_kernels.hpp
struct FsCandRec { int64_t window, aa_off; double P; int32_t cand, sf, startj, len; float fwdsc, nullsc; int64_t fxoff; };   // an ORF that passed F4, as a cascade lane leaves it
struct FsLaneSurv {                // one cascade lane's F4 survivors and their hit windows, in the lane's device memory
  const FsCandRec *d_c; const WindowRec *d_w;
  int32_t n_c, n_w, cand_base;     // counts; what makes the lane's candidate ids the block's
  int64_t first_window, dpool;     // ... its sequence indices the block's, its pool offsets relative to the first lane's pool
};
struct FsOrfDev {                  // an ORF that passed F4, in the order esl_gencode emits them per (sequence, strand)
  int64_t w, aa_off; double P;
  int32_t cand, strand, start, end, n; float fwd_null;
  int32_t wb, we;                  // its hit windows, a range of the ordered hit-window list
  int32_t dw_n, dw_len, dw_k;      // the DNA window it asks for (start on the strand, length; node of its best hit window)
  int32_t kmin, kmax;              // first / last model node over its hit windows
  int32_t g0, g1;                  // its (sequence, strand) group, a range of the ordered ORF list
  int32_t pad_;
};
struct FsWinBuild {                // what either build leaves: host copies (page-locked, valid until the next build) and device arrays
  int32_t n_orfs = 0, nw = 0, maxlen = 0;
  int64_t pool_bytes = 0, total = 0;
  const int64_t *h_voff = nullptr; const int32_t *h_vlen = nullptr;   // [nw] the windows' pool offsets and lengths: valid when the build returns
  const FsOrfDev *h_orfs = nullptr;         // [n_orfs]  } the device build: in flight when it returns, valid after the next synchronize of
  const int32_t *h_grp = nullptr;           // [2 nw]    } the context's stream (fs_decide); a window's group = a range of h_orfs
  bool host_built = false;                  // the host build: the records wait on the host (h_out) for a decision taken there
  const bath_fs_window *h_out = nullptr;
  bath_fs_window *d_out = nullptr;          // the device build: the records on the device (fs_decide completes them)
  const FsWinDev *d_desc = nullptr;         // the gather kernel's descriptors
  const int64_t *d_voff = nullptr; const int32_t *d_vlen = nullptr;   // the view's off[] / len[]
};
bool fs_windows_on_device();       // false under BATH_HIP_FS_WINDOWS_HOST=1: every block takes the host build
// BATH_OK; BATH_ENORESULT: an input the kernels do not take (the caller runs the host build); an error
int fs_build_windows_device(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna,
                            const bath_pipeline_params *prm, const FsLaneSurv *lanes, int nlanes, int nc_total, FsWinBuild *out);
// the same from the survivor lists on the host: sel[n] by candidate id, wins[nhw] by (candidate id, start), ids the block's own
int fs_build_windows_host(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                          const FsCandRec *sel, int n, const WindowRec *wins, int nhw, FsWinBuild *out);
// the order fs_build_windows_host reads the lists in: one lane's lists as the select kernels appended them -> by candidate id, its hit
// windows by (candidate id, start, k); then the lanes' lists as one, ids, sequence indices and pool offsets made the block's own
void fs_order_survivors(std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins);
void fs_merge_survivors(const FsLaneSurv *lanes, int nlanes, const std::vector<std::vector<FsCandRec>> &lsel, const std::vector<std::vector<WindowRec>> &lwin,
                        std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins);
bool fs_orf_in_window(const FsOrfDev &o, const bath_fs_window &r, int n_seq);   // the ORF lies inside the window of its strand (p7_pipeline.c:1405)
// after the parsers: scores -> P-values -> branch, where the windows were built; the completed records into h_out[nw]
int fs_decide(bath_hip_ctx *ctx, const bath_hip_fsprofile *om_fs3, const bath_pipeline_params *prm, const FsWinBuild &B, const float *d_bias,
              const float *d_fsc, const float *h_fsc, bath_fs_window *h_out);
float flogsum_host(float a, float b);                          // p7_FLogsum with its table, on the host

// ---- frameshift helpers for the pipeline (bath_frameshift.hip; fs5_envelopes_ex: bath_fs_envelopes.hip)
int fs_fork(bath_hip_ctx *ctx);   // the context's side stream waits for what the main stream holds so far
int fs_join(bath_hip_ctx *ctx);   // ... and the main stream for the side stream
int fs3_forward_scores(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, float *sc);   // table log-sum, host array out
const float *fsprofile_evparam(const bath_hip_fsprofile *om);
int fs_max_regions();
int fs3_regions(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, float loop, int32_t *regions_out, float *fwd_sc_out = nullptr, const int32_t *kept = nullptr);   // parsers + domain decoding + region heuristics (+ the Forward scores)
int fsprofile_codon_lengths(const bath_hip_fsprofile *om);
int fs_model_ok(bath_hip_ctx *ctx, const bath_hip_fsprofile *om);   // BATH_EINVAL with the context's error set beyond kFsMaxNodes
struct FsHostTables { int M, max_length, maxcodons; const float *tsc; const uint8_t *codons; const float *evparam; };
const FsHostTables fsprofile_host(const bath_hip_fsprofile *om);
struct FsTraceOut {               // what the pipeline keeps of an envelope's OA trace
  int32_t ihmm, jhmm, iali, jali, nshift, ok; float domcorrection;
  int32_t ncol, exact, nstops;    // alignment display: columns (first to last match state), identities with the consensus, stop codons
  float aliscore;                 // p7_pli_computeAliScores_BATH: sum of the per-column scores; negative = the domain is dropped
  int32_t col_off;                // where this envelope's columns start in the batch's dense column arrays
};
// <cons>: device array [M+1] of consensus residue codes or nullptr; <steps>/<step_off>: per alignment column
// state | codon length << 4 | indel label << 8 (the columns of all envelopes lie densely; those of envelope e start at (*step_off)[e])
int fs5_envelopes_ex(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                     bath_fs5_result *res, float *pp, float *oa, float *ppx, float *oax, FsTraceOut *trace,
                     const uint8_t *cons = nullptr, std::vector<uint16_t> *steps = nullptr, std::vector<int64_t> *step_off = nullptr,
                     std::vector<float> *step_pp = nullptr /* tr->pp of every column, parallel to steps */);

// ---- multi-domain regions (bath_ensemble.hip, host): envelopes and per-residue null2 scores from 200 stochastic tracebacks
int region_trace_ensemble(const bath_hip_oprofile *om, int cfg_L, const uint8_t *res, int Lr, const float *fwd, const float *fx,
                          std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env, uint32_t seed = 42);
// ... on the model as plain arrays (what the ensembles read of it): rf [Kp][M+1], tf [M+1][8], pmove of the configured length, xf_E
struct StdEnsModel { int M; const float *tf, *rf; float pmove, tEL, tEM; };
StdEnsModel std_ens_model(const bath_hip_oprofile *om, int cfg_L);          // after om->ensure_len_tables(cfg_L)
int region_trace_ensemble(const StdEnsModel &om, const uint8_t *res, int Lr, const float *fwd, const float *fx,
                          std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env, uint32_t seed = 42);
// ---- its per-trace-stream modes (bath_hip_set_std_ensemble; bath_std_ens_walk.hpp is the walk, bath_std_ensemble.hip the kernel)
void std_ensemble_walk_host(const StdEnsModel &om, int Lr, const float *fwd, const float *fx, uint32_t seed, int max_seg,
                            int32_t *status, int32_t *nseg, int32_t *seg, uint32_t *path);
int std_ensemble_consume(const StdEnsModel &om, const uint8_t *res, int Lr, const int32_t *status, const int32_t *nseg, const int32_t *seg, int max_seg,
                         const uint32_t *path, std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env, std::vector<int32_t> *segs_out = nullptr);
int std_region_trace_ensemble_streams(const StdEnsModel &om, const uint8_t *res, int Lr, const float *fwd, const float *fx, std::vector<float> *n2sc,
                                      std::vector<std::pair<int, int>> *env, uint32_t seed = 42, int *region_status = nullptr,
                                      std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);
// BATH_ENSEMBLE_STREAMS_DEVICE: std_ensemble_kernel queued on ctx->stream behind the regions' Forward, and what it wrote on its way
// to page-locked memory in one copy.  Once the stream is synchronized: out = per region status[200], nseg[200],
// seg[200][kEnsMaxSeg][kStdSegInts]; path + poff[e] = region e's path codes, [200][std_ens_path_words].  The matrices stay in device
// memory (d_fwd, d_fx) for the regions that fall back to a host walk.
constexpr int kStdEnsOutInts = 200 * (2 + 8 * 5);
struct StdEnsRun { const int32_t *out = nullptr; const uint32_t *path = nullptr; std::vector<int64_t> poff; const float *d_fwd = nullptr, *d_fx = nullptr; };
int std_region_ensembles_device(bath_hip_ctx *ctx, const bath_hip_oprofile *om, int64_t n, const int32_t *h_len, const int32_t *d_len, const int32_t *d_cfg,
                                const float *d_fwd, const int64_t *d_foff, const float *d_fx, const int64_t *d_xoff, uint32_t seed, StdEnsRun *run);
int std_ensemble_region_from_device(bath_hip_ctx *ctx, const StdEnsRun &run, int64_t e, const StdEnsModel &om, const uint8_t *res, int Lr,
                                    int64_t foff, int64_t xoff, uint32_t seed, std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env,
                                    int *region_status = nullptr, std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);
int std_region_ensemble_host(bath_hip_ctx *counters, int mode, const StdEnsModel &om, const uint8_t *res, int Lr, const float *fwd, const float *fx,
                             std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env, uint32_t seed, int *region_status = nullptr,
                             std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);

int fs_region_trace_ensemble(int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr, const float *fwd, const float *fx,
                             std::vector<std::pair<int, int>> *env, uint32_t seed = 42);
// ---- the per-trace-stream ensemble modes (bath_hip_set_fs_ensemble; bath_fs_ens_walk.hpp is the walk, bath_fs_ensemble.hip the kernel)
uint32_t ens_rng_jump(uint32_t x, uint64_t n);                           // the fast generator's state n steps after x
void fs_ensemble_start_states(uint32_t seed, uint32_t *states /* [200] */);   // trace t starts t * 2^20 steps into the region's generator
void fs_ensemble_walk_host(int M, const float *tsc, float xNL, float xNM, float xE, int Lr, const float *fwd, const float *fx, uint32_t seed,
                           int32_t *status, int32_t *nseg, int32_t *seg);
int fs_ensemble_consume(const int32_t *status, const int32_t *nseg, const int32_t *seg, int max_seg, int ireg, std::vector<std::pair<int, int>> *env,
                        std::vector<int32_t> *segs_out = nullptr);
// BATH_ERANGE: outside the stream rule or more than kEnsHostMaxSeg segments in a trace (the caller runs the serial ensemble)
int fs_region_trace_ensemble_streams(int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr, const float *fwd, const float *fx,
                                     std::vector<std::pair<int, int>> *env, uint32_t seed = 42, int *region_status = nullptr,
                                     std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);
// where fs5_region_forward left the regions in DEVICE memory, and the job list of the kernel that reads them next (longest first)
struct FsRegionDev { const float *d_fwd, *d_fx; const int64_t *d_foff, *d_xoff; const float *d_sc; const int32_t *job_order; unsigned *job_counter; };
int fs5_region_forward(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int cfg_len_amino,
                       const float **fwd, std::vector<int64_t> *fwd_off, const float **xmx, std::vector<int64_t> *xmx_off, std::vector<float> *sc,
                       const int **done_flags, const float **sc_live, FsRegionDev *dev = nullptr);
// BATH_ENSEMBLE_STREAMS_DEVICE: the regions' multihit Forward into device memory and fs_ensemble_kernel behind it on ctx->stream;
// returns after queueing.  Once the stream is synchronized: out = per region status[200], nseg[200], seg[200][kEnsMaxSeg][4]
// (kFsEnsOutInts ints), sc = the regions' Forward scores, both page-locked.  The matrices stay where *dev says until the
// context's next region stage (fs_ensemble_fetch_region copies one region's to the host: the fallbacks).
constexpr int kFsEnsOutInts = 200 * (2 + 8 * 4);
struct FsEnsRun { const int32_t *out = nullptr; const float *sc = nullptr; FsRegionDev dev{}; std::vector<int64_t> foff, xoff; };
int fs5_region_ensembles_device(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int cfg_len_amino, uint32_t seed,
                                float xNL, float xNM, float xE, FsEnsRun *run);
int fs_region_ensemble_host(bath_hip_ctx *counters, int mode, int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr,
                            const float *fwd, const float *fx, std::vector<std::pair<int, int>> *env, uint32_t seed, int *region_status = nullptr,
                            std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);
int fs_ensemble_region_from_device(bath_hip_ctx *ctx, bath_hip_ctx *counters, const FsEnsRun &run, int64_t e, int M, const float *tsc, float xNL, float xNM, float xE,
                                   int ireg, int Lr, uint32_t seed, std::vector<std::pair<int, int>> *env, int *region_status = nullptr,
                                   std::vector<int32_t> *segs_out = nullptr, int32_t *trace_status = nullptr);
int fs_ensemble_fetch_region(bath_hip_ctx *ctx, const FsEnsRun &run, int64_t e, std::vector<float> *fwd, std::vector<float> *fx);

// ---- six-frame translation + ORF work list (bath_orfs.hip)
struct OrfRec {                   // one ORF of the length-sorted work list
  int64_t aa_off;                 // offset of its first residue in the amino-acid stream pool
  int32_t w;                      // window
  int32_t len_sf;                 // length | (strand*3+frame) << 28
};
__host__ __device__ inline int orf_stream_pitch(int n) { return (n / 3 + 16) & ~15; }   // bytes reserved per frame of an n-nt window
size_t orf_aa_bytes(const bath_hip_seqs *dna);
int orf_slot_cap(int minlen);                                   // ORF records reserved per tile (all six frames)
int orf_tiles_ensure(bath_hip_ctx *ctx, const bath_hip_seqs *dna);   // fills dna->ntiles, d_tile_desc, d_tile_first
struct OrfTablesDev { const uint8_t *full, *fwd, *rev, *comp, *is_init; bool using_initiators; };   // 18^3 general table, canonical 64-entry tables per strand, complement, initiation codons
int orf_tables_upload(bath_hip_ctx *ctx, int ncbi_table, OrfTablesDev *t, int initiator = 0);
struct OrfBuffers {               // device buffers of one translation pass
  uint8_t *aa;                    // orf_aa_bytes()
  void *slots;                    // ntiles*orf_slot_cap() records of 8 bytes
  void *cross;                    // ntiles*6 records of 8 bytes: ORFs crossing tile edges
  int32_t *cnt, *prefix, *suffix; // ntiles*6 each (cnt uses ntiles)
  int *hist, *cursor, *ntotal;    // kOrfBins, kOrfBins*kOrfCursorStride (bin b at b*kOrfCursorStride), 1
  OrfRec *sorted;                 // the work list, longest ORFs first; *ntotal entries
};
void orf_buffers_carve(OrfBuffers *ob, void *aa, void *slots, void *sorted, void *misc /* 5*nent + kOrfMiscInts ints */, size_t nent);
int launch_orf_scan(bath_hip_ctx *ctx, const bath_hip_seqs *dna, const OrfTablesDev &tt, int minlen, const OrfBuffers &b,
                    unsigned long long *d_n_orfs, unsigned long long *d_orf_res, int strands = 0);

// ---- the cascade, returning the ORFs that pass the Forward filter (bath_pipeline.hip); *d_pool stays valid until the next pipeline call on ctx
int pipeline_filters_survivors(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                               bath_pipeline_stats *stats, std::vector<PipelineSurvivor> *out, const uint8_t **d_pool);
// The ORFs that passed F4 and (frameshift pipeline) their hit windows, from every lane of the cascade: candidate ids are made
// unique over the lanes, windows are the block's, and aa_off addresses the residues relative to <pool> (the first lane's pool;
// another lane's pool is another allocation in the same flat address space, its ORFs carry the distance between the two).
struct SurvivorSet {
  std::vector<FsCandRec> sel;        // by candidate id
  std::vector<WindowRec> wins;       // by (candidate id, n)
  int nc_total = 0;
  const uint8_t *pool = nullptr;
  // the first lane's device tables, which any lane holds alike: the codon tables, the model's SSV scores, the background frequencies
  OrfTablesDev tt{};
  const uint8_t *d_ssvsc = nullptr;
  const float *d_bgf = nullptr;
  // device_only: the lists stayed in the lanes' device memory (counts known, nothing copied): what bath_fs_windows.hip reads;
  // survivors_to_host() completes sel / wins from them when the host path must run after all
  bool on_device = false;
  std::vector<FsLaneSurv> lanes;
  std::vector<bath_hip_ctx *> lane_ctx;
  int n_states = 0;
};
int filters_with_survivors(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                           bath_pipeline_stats *stats, const bath_orf_result **results, int64_t *n_results, bool want_wins, SurvivorSet *out,
                           bool device_only = false);
// the host path after a device-only cascade (an input bath_fs_windows.hip does not take): the lanes' lists come over after all
int survivors_to_host(SurvivorSet *sv);

}  // namespace bath
