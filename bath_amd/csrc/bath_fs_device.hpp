// bath_fs_device.hpp -- device helpers shared by the frameshift kernels (bath_frameshift.hip, bath_fs_envelopes.hip, bath_fs_wavefront.hip, the odds-ratio
// kernels): p7_FLogsum with its table in LDS (logsum.c:105), DPP lane moves and scans, the longest-first job queue, the device profile.
#pragma once
#include <algorithm>
#include <vector>
#include <cmath>
#include <mutex>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

struct bath_hip_fsprofile {
  bath_hip_ctx *ctx = nullptr;
  int M = 0, codon_lengths = 0, maxcodons = 0, max_length = 0;
  int pitch = 0;                 // floats per emission row (M+1 rounded up to 4)
  float fsprob = 0.f;
  float evparam[BATH_NEVPARAM];
  float *d_rsc = nullptr;        // [(maxcodons+Kp)][pitch]
  float *d_tf = nullptr;         // [(M+2)][8] forward-ordered transitions per node
  float *d_tb = nullptr;         // [(M+2)][8] backward-ordered transitions per node
  float *d_logsum = nullptr;     // [16000]
  std::vector<float> h_tsc;      // [M*8] generic log transitions (OA traceback deltas on the host)
  float *d_tsc = nullptr;        // ... and on the device (fs_ensemble_kernel's stochastic tracebacks)
  std::vector<uint8_t> h_codons; // [(M+1)*maxcodons] best amino acid per (node, quasi-codon) (null2 along a trace)
  uint8_t *d_codons = nullptr;   // the same on the device (5-codon profiles)
  uint8_t *d_indel = nullptr;    // [(M+1)*maxcodons] indel-type label of that choice (hmmer.h:259-276), for the alignment display
  // length model: xsc[N|C|J][LOOP|MOVE] for L_amino, multihit (nj=1) and unihit (nj=0); host libm log()
  // (the tables grow under <grow_mu>; the old ones are retired, not freed: the profile is shared by contexts running side by side --
  // the regions' Forward beside the envelopes, worker contexts -- and another stream's kernel may still be reading them)
  mutable int maxL = -1;
  mutable float *d_loop[2] = {nullptr, nullptr}, *d_move[2] = {nullptr, nullptr};
  mutable std::mutex grow_mu;
  mutable std::vector<void *> retired;
  int ensure_len(int maxL_amino) const;
  // odds-ratio tables (BATH_LOGSUM_ODDS, bath_fs_odds.hip; the 5-codon odds mode, bath_fs5_odds.hip): expf of d_rsc's codon rows,
  // d_tf and d_tb, padded to the nodes of every lane, built on the first odds-mode call
  mutable float *d_odds_rsc = nullptr, *d_odds_tf = nullptr, *d_odds_tb = nullptr;
  mutable int odds_pitch = 0;    // floats per odds emission row; node k sits at column k (3-codon) or k-1 (5-codon: 16-byte aligned lane blocks)
  mutable std::mutex odds_mu;
  int ensure_odds() const;
};

namespace bath {

constexpr int kLogsumTbl = 16000;
// threads per block of the DP kernels that hold p7_FLogsum's 64 KB table in LDS: 8 waves share one copy, so two blocks = 16 waves
// fit a CU (4 per SIMD); with 4 waves per block the table limited a CU to 8 waves, and these kernels live on latency hiding
#ifndef BATH_FS_BLOCK
#define BATH_FS_BLOCK 512
#endif
#ifndef BATH_FS_WAVES           /* waves per SIMD the compiler must leave room for when a lane holds <= 3 nodes (0: no constraint) */
#define BATH_FS_WAVES 4
#endif
constexpr int kFsBlock = BATH_FS_BLOCK;
// Two 512-thread blocks (one 64 KB table each) fit a CU's LDS: 4 waves per SIMD if a wave keeps to 128 VGPRs.  Left alone the
// compiler takes 134-161 for the straight-line rows (one block per CU, 2 waves per SIMD); told to stay within 128 it spills
// 7-39 registers.  Measured on the bench's --fs pass (tools/fs_variants.sh): the parsers and Backward gain from the
// cap (fs3_fwd 9.5 -> 7.6 ms, fs_bwd<3> 7.1 -> 5.4, fs_bwd<5> 6.0 -> 5.4), the 5-codon Forward loses (3.7 -> 5.4: 39 spills
// in its row chain) and is left uncapped.  Models with more than 3 nodes per lane need the registers.
constexpr int fs_min_waves(int C) { return (C <= 3 && BATH_FS_WAVES > 0) ? BATH_FS_WAVES : 1; }

struct FsDev {
  int M, pitch, maxcodons;
  const float *rsc, *tf, *tb, *logsum;
};

// p7_FLogsum (logsum.c:105-111): truncating table lookup, or the exact form (logsum.c:109)
// Straight-line code: the table is read unconditionally at a clamped index and the early-out cases are a select.  With the
// obvious `if (...) return mx;` every log-sum became its own exec-masked basic block (165 branches in the 3-codon Forward
// kernel) and the compiler could not overlap the independent log-sums of a lane's nodes; the values are identical.
// v_max_f32 as the instruction: fmaxf() first quiets each operand the compiler cannot prove canonical (a loaded value, a DPP
// move) with a v_max_f32 x, x of its own -- two of the ten instructions of a table log-sum, in kernels that are chains of them.
// The operands here are never NaN (scores are finite or -inf).
__device__ __forceinline__ float vmax_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <bool EXACT>
__device__ __forceinline__ float flogsum(float a, float b, const float *tbl) {
  if (EXACT) {
    const float mx = fmaxf(a, b), mn = fminf(a, b);
    if (mn == -INFINITY || (mx - mn) >= 15.7f) return mx;
    return mx + log1pf(expf(mn - mx));
  }
  // <tbl> is the kernels' LDS copy of the table, ZERO from entry 15700 on (fs_load_logsum_table): the reference's early outs
  // "mn == -inf or mx - mn >= 15.7 -> mx" are then the look-up itself (mx + 0), and a log-sum is max, |a - b|, min, mul, cvt,
  // shift, ds_read, add.  (int)(d * 1000.f) >= 15700 exactly when d >= 15.7f: 15.7f * 1000.f rounds to 15700.0f and the float
  // below 15.7f to 15699.999.  a = b = -inf: |NaN| -> v_min returns 15.999 -> -inf + 0.
  const float dc = fminf(fabsf(a - b), 15.999f);
  return vmax_raw(a, b) + tbl[(int)(dc * 1000.f)];
}

// the same on the unpadded table in global memory (kernels that take a few log-sums per target)
__device__ __forceinline__ float flogsum_g(float a, float b, const float *tbl) {
  const float mx = fmaxf(a, b), mn = fminf(a, b);
  const float d = mx - mn;                                    // +inf when mn = -inf, NaN when both are
  const float dc = fminf(d, 15.999f);                         // (v_min_f32 returns the number when one operand is NaN)
  const float t = tbl[(int)(dc * 1000.f)];
  return (mn == -INFINITY || d >= 15.7f) ? mx : mx + t;
}

// p7_FLogsum's table into LDS, its entries for differences >= 15.7 (which the reference never reads) zeroed
__device__ __forceinline__ void fs_load_logsum_table(float *s_tbl, const float *g_tbl) {
  for (int i = threadIdx.x; i < 16000; i += blockDim.x) s_tbl[i] = (i < 15700) ? g_tbl[i] : 0.f;
}

// Cross-lane moves by DPP instead of ds_bpermute (__shfl_*): these kernels are chains of dependent operations, and a shuffle through
// the LDS crossbar costs ~100+ cycles of that chain where a DPP operand costs a VALU instruction.  <old> is what a lane without a
// source keeps: the identity of the combining operation, so that such lanes need no select.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_f(float v, float old) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_shr1(float v, float fill) { return dpp_f<0x138>(v, fill); }          // lane l <- lane l-1, lane 0 <- fill
__device__ __forceinline__ float wave_bcast_last(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }

// log-sum of a value per lane, result in every lane: an inclusive scan in lane order (row_shr 1/2/4/8, row_bcast 15/31), lane 63
// broadcast.
template <bool EXACT>
__device__ __forceinline__ float wave_logsum(float v, const float *tbl) {
  v = flogsum<EXACT>(v, dpp_f<0x111>(v, -INFINITY), tbl);
  v = flogsum<EXACT>(v, dpp_f<0x112>(v, -INFINITY), tbl);
  v = flogsum<EXACT>(v, dpp_f<0x114>(v, -INFINITY), tbl);
  v = flogsum<EXACT>(v, dpp_f<0x118>(v, -INFINITY), tbl);
  v = flogsum<EXACT>(v, dpp_f<0x142, 0xa>(v, -INFINITY), tbl);
  v = flogsum<EXACT>(v, dpp_f<0x143, 0xc>(v, -INFINITY), tbl);
  return wave_bcast_last(v);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// ---- shared by the odds-ratio kernels (bath_fs_odds.hip, bath_fs5_odds.hip)
constexpr float kOddsRescale = 1.0e4f;   // fwdback_fs.c:472: every value a later row reads is rescaled when E(i) (Backward: B(i)) passes it
constexpr int kOddsBlock = 256;          // 4 waves, one window or envelope each; nothing is shared inside a block

// x -> m x + a composed over the lanes below (DPP row_shr 1/2/4/8, row_bcast 15/31: the scan of d_chain_fwd); returns the
// composition's offset EXCLUSIVE of this lane: the value entering the lane's first node when the chain starts at 0.
// Lanes without a source see the identity map (m = 1, a = 0).
__device__ __forceinline__ float affine_scan_excl(float m, float a) {
#define BATH_ODDS_STEP(CTRL, MASK) { const float mp = dpp_f<CTRL, MASK>(m, 1.f), ap = dpp_f<CTRL, MASK>(a, 0.f); a = a + m * ap; m = m * mp; }
  BATH_ODDS_STEP(0x111, 0xf) BATH_ODDS_STEP(0x112, 0xf) BATH_ODDS_STEP(0x114, 0xf) BATH_ODDS_STEP(0x118, 0xf)
  BATH_ODDS_STEP(0x142, 0xa) BATH_ODDS_STEP(0x143, 0xc)
#undef BATH_ODDS_STEP
  return wave_shr1(a, 0.f);
}

// sum of a value per lane, in every lane
__device__ __forceinline__ float wave_sum(float v) {
  v = v + dpp_f<0x111>(v, 0.f);
  v = v + dpp_f<0x112>(v, 0.f);
  v = v + dpp_f<0x114>(v, 0.f);
  v = v + dpp_f<0x118>(v, 0.f);
  v = v + dpp_f<0x142, 0xa>(v, 0.f);
  v = v + dpp_f<0x143, 0xc>(v, 0.f);
  return wave_bcast_last(v);
}

// the transition rows are read again every row, from L1: held in registers across the row loop (where the compiler hoists them
// to) they take 8 C VGPRs, which halves the waves per SIMD at C = 4 and spills from C = 16 on.  The empty asm makes the pointer
// opaque to that hoisting.
__device__ __forceinline__ const float *per_row(const float *p) {
  asm volatile("" : "+s"(p));
  return p;
}

// row i of the special-state matrix, log value + running scale (logf(0) = -inf)
__device__ __forceinline__ void put_row(float *xo, int i, float E, float N, float J, float B, float Cc, double ts) {
  const float s = (float)ts;
  xo[i * 5 + 0] = logf(E) + s; xo[i * 5 + 1] = logf(N) + s; xo[i * 5 + 2] = logf(J) + s; xo[i * 5 + 3] = logf(B) + s; xo[i * 5 + 4] = logf(Cc) + s;
}


// Work distribution of the wave-per-window kernels.  Their duration is the longest chain of rows any one wave walks, so the
// windows are handed out longest first from a shared counter (<order> lists them by decreasing length): a wave that drew a
// long window early draws fewer later, instead of every wave taking windows wid, wid + nwaves, ... whatever their lengths.
// Sequences 0..n-1 by decreasing length, equal lengths in index order (what std::stable_sort gives): a counting sort -- the launchers
// sort every batch of DNA windows or envelopes once or twice per stage while the GPU waits (7.6 k windows: 0.2-0.3 ms per std::sort,
// ~20 us this way).  <sorted_len>, if not null, receives the lengths in that order.
inline void fs_order_by_length_desc(const int32_t *len, int64_t n, std::vector<int32_t> *order, std::vector<int32_t> *sorted_len = nullptr) {
  int32_t mx = 0;
  for (int64_t i = 0; i < n; i++) mx = std::max(mx, len[i]);
  if (order) order->resize((size_t)n);
  if (sorted_len) sorted_len->resize((size_t)n);
  if (n == 0) return;
  if ((int64_t)mx > 8 * n + 4096) {                              // a few long sequences: the comparison sort is the cheaper one
    std::vector<int32_t> ord((size_t)n);
    for (int64_t i = 0; i < n; i++) ord[(size_t)i] = (int32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return len[a] > len[b]; });
    if (sorted_len) for (int64_t i = 0; i < n; i++) (*sorted_len)[(size_t)i] = len[ord[(size_t)i]];
    if (order) order->swap(ord);
    return;
  }
  std::vector<int32_t> start((size_t)mx + 2, 0);
  for (int64_t i = 0; i < n; i++) start[(size_t)(mx - std::max(len[i], 0)) + 1]++;       // bucket 0 = the longest
  for (int32_t b = 0; b <= mx; b++) start[(size_t)b + 1] += start[(size_t)b];
  for (int64_t i = 0; i < n; i++) {
    const int32_t at = start[(size_t)(mx - std::max(len[i], 0))]++;
    if (order) (*order)[(size_t)at] = (int32_t)i;
    if (sorted_len) (*sorted_len)[(size_t)at] = len[i];
  }
}

struct FsJobs { const int32_t *order; unsigned *counter; };

// One model of a launch that holds several (fs3_fwd_batch_kernel, fs5_fwd_parser_batch_kernel: calibration, bath_calibrate.hip): what
// the single-model kernels take as arguments, read by a block from a device array at blockIdx.y.  <jobs.counter> is the model's own.
struct FsBatchModel {
  SeqView dna;
  FsDev p;
  const float *loop_tab, *move_tab;
  float *sc;
  FsJobs jobs;
  int cfg_len;               // the 5-codon parser's configuration length in amino acids (the 3-codon parser takes a window's own)
};

// The odds-ratio tables (ensure_odds) cover every node a lane of the C-column kernel owns, 1 .. 64 C, with zeros beyond M: a lane's
// loads are one vector offset plus immediates, and nodes beyond M come out 0 without a branch or a clamp.  The 5-codon kernels read
// node k's emission at column k-1, so a lane's C values start at lane*C -- whole 16-byte loads when 4 divides C.
struct FsOddsDev {
  int M, pitch;
  const float *rsc;          // [338 or 1367][pitch = 64 C + 4] expf(rsc): every codon, quasi-codon and degenerate row the kernels index
  const float *tf, *tb;      // [64 C + 2][8] expf of the log-space kernels' tf / tb (node 0 and nodes beyond M: zeros)
};
inline FsOddsDev fs_odds_dev(const bath_hip_fsprofile *om) { return FsOddsDev{om->M, om->odds_pitch, om->d_odds_rsc, om->d_odds_tf, om->d_odds_tb}; }
inline int fs_odds_grid(const bath_hip_ctx *ctx, int64_t n) {    // blocks of kOddsBlock threads, a wave per job, at most 8 per CU
  const int wpb = kOddsBlock / 64;
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + wpb - 1) / wpb, (int64_t)ctx->prop.multiProcessorCount * 8));
}

// every frameshift launcher's dispatch: the body sees C as the constant CC (M beyond kFsMaxNodes: fs_model_ok refuses it earlier)
#define BATH_FS_SWITCH(Cv, ...) \
  BATH_TILING_SWITCH(BATH_FS_COLUMNS, Cv, { ctx->set_error("frameshift kernels support models up to 1280 nodes"); return BATH_EINVAL; }, __VA_ARGS__)
static_assert(kFsMaxNodes == 1280, "BATH_FS_SWITCH's refusal names the limit");
__device__ __forceinline__ int64_t fs_next_job(const FsJobs &q, int64_t n, int lane) {
  unsigned j = 0;
  if (lane == 0) j = atomicAdd(q.counter, 1u);
  j = (unsigned)__shfl((int)j, 0, 64);
  return (int64_t)j < n ? (int64_t)q.order[j] : (int64_t)-1;
}

// ---- what the launchers of bath_frameshift.hip and bath_fs_envelopes.hip share
// the windows of <dna> by decreasing length and <k> zeroed job counters (bath_frameshift.hip)
int fs_schedule(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int k, FsJobs *jobs);
template <class K>
int fs_set_shmem(bath_hip_ctx *ctx, K kernel, size_t shmem) {   // a kernel whose dynamic LDS goes past the 64 KB every kernel may have
  if (shmem > 64 * 1024) BATH_HIP_TRY(ctx, bath::allow_max_lds((const void *)kernel));
  return BATH_OK;
}
// where window i's rows start when a window of L nucleotides has L + 1 rows of <per_row> floats, packed back to back: n + 1 offsets
inline std::vector<int64_t> fs_row_offsets(const bath_hip_seqs *dna, int64_t per_row) {
  std::vector<int64_t> off((size_t)dna->n + 1, 0);
  for (int64_t i = 0; i < dna->n; i++) off[(size_t)i + 1] = off[(size_t)i] + ((int64_t)dna->h_len[(size_t)i] + 1) * per_row;
  return off;
}

// ---- row-per-lane wavefront kernels of the envelopes (bath_fs_wavefront.hip)
int launch_fs5_fwd_wf(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int exact, int c5_compat,
                      float *d_sc, float *d_fwd, const int64_t *d_foff, float *d_xmx, const int64_t *d_xoff, DevBuf &ring_scratch, FsJobs jobs);
int launch_fs5_bwd_wf(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int exact,
                      float *d_sc, float *d_bck, const int64_t *d_boff, float *d_xmx, const int64_t *d_xoff, DevBuf &ring_scratch, DevBuf &terms_scratch, DevBuf &toff_scratch,
                      FsJobs jobs_sweep, FsJobs jobs_x);

// ---- decoding + optimal-accuracy fill with several waves per envelope, long models (bath_fs_decode.hip)
int fs5_decode_oa_mw_shape(int M, int *nodes_per_lane);     // waves per envelope (0: the one-wave kernel of bath_fs_envelopes.hip)
int launch_fs5_decode_oa_mw(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, const float *d_bsc,
                            float *d_fwd, const int64_t *d_foff, float *d_fx, const int64_t *d_xoff, const float *d_bck, const int64_t *d_boff, const float *d_bx,
                            float *d_colsum, float *d_oa, float *d_osc, float *d_ox, FsJobs jobs, int store_pp = 1, float *d_rowden = nullptr);

// ---- multihit recursions in the reference's serial order, chains batched per block (bath_fs_chain.hip)
int launch_fs3_fwd_chain(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int Cv, float tEL, float tEM,
                         float *d_sc, float *d_xmx, const int64_t *d_xoff, FsJobs jobs, int cu_share = 1);
int launch_fs3_bwd_chain(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int Cv, float tEL, float tEM,
                         float *d_sc, float *d_xmx, const int64_t *d_xoff, FsJobs jobs, int cu_share = 1 /* 2: the Forward parser runs beside it */);
int launch_fs5_fwd_chain(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int Cv, float tEL, float tEM, int c5_compat,
                         float *d_sc, float *d_fwd, const int64_t *d_foff, float *d_xmx, const int64_t *d_xoff, int cfg_len, FsJobs jobs, int *d_done);
// the score of launch_fs5_fwd_chain alone: the same kernel instantiated without its stores (calibration, bath_calibrate.hip)
int launch_fs5_fwd_parser(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int Cv, float tEL, float tEM,
                          float *d_sc, int cfg_len, FsJobs jobs);
// the two strict score-only parsers over several models per launch: d_models[n_models], all of the tiling <Cv> and none longer than
// <Mmax>, each with <n> windows (calibration of a batch of models, bath_calibrate.hip)
int launch_fs3_fwd_batch(bath_hip_ctx *ctx, hipStream_t stream, const FsBatchModel *d_models, int n_models, int Mmax, int Cv, int64_t n, float tEL, float tEM);
int launch_fs5_fwd_parser_batch(bath_hip_ctx *ctx, hipStream_t stream, const FsBatchModel *d_models, int n_models, int Mmax, int Cv, int64_t n, float tEL, float tEM);
// ---- the 3-codon parsers in odds-ratio space (bath_fs_odds.hip)
int launch_fs3_odds(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, bool backward,
                    float *d_sc, float *d_xmx, const int64_t *d_xoff, FsJobs jobs);
// ---- the 5-codon Forward (envelopes: unihit; regions: multihit) and Backward (envelopes) in odds-ratio space (bath_fs5_odds.hip)
enum Fs5OddsKind { kFs5OddsEnvFwd = 0, kFs5OddsEnvBwd = 1, kFs5OddsRegionFwd = 2 };
int launch_fs5_odds(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, Fs5OddsKind kind,
                    float *d_sc, float *d_mx, const int64_t *d_moff, float *d_xmx, const int64_t *d_xoff, int cfg_len, FsJobs jobs, int *d_done);
// the multihit score of launch_fs5_odds(kFs5OddsRegionFwd) alone: the same kernel instantiated without its stores (calibration in odds arithmetic)
int launch_fs5_odds_parser(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, float *d_sc, int cfg_len, FsJobs jobs);

}  // namespace bath
