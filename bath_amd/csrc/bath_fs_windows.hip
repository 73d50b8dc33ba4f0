// bath_fs_windows.hip -- p7_pli_BuildDNAWindows, the per-window ORF summary of p7_pli_Frameshift and the branch decision that
// follows the 3-codon Forward parser (p7_pipeline.c:462-572, :1364-1415, :1425-1465): ONE set of rules, two drivers.
//
// The rules (the ORFs' order on a strand, ORF -> the DNA window it asks for, fusing overlapping windows, a window's span and the
// ORFs inside it, the window's summary with P_tot, the branch decision) are the __host__ __device__ functions at the top of this file.
//   fs_build_windows_device   the default: kernels on the context's stream, fed by what the cascade's lanes left in device memory
//     merge     the lanes' F4 survivors and hit windows, ids made the block's own, sort keys formed
//     rank      the ORFs ordered by counting (keys are unique: rank = number of smaller keys; a few thousand records, tiled through
//               LDS, the comparisons spread over the chip) by (sequence, strand, the order esl_gencode emits a strand's ORFs)
//     hits      per hit window: its ORF's best window (highest score, then longest, then first) and k_min / k_max by atomics on the
//               ORF's slot -- the hit windows need no order of their own
//     orf       per ORF: its best hit window -> the DNA window it asks for (:486-527)
//     group     per (sequence, strand): windows ordered by start (p7_hmmwindow_SortByStart) ...
//     fuse      ... and overlapping ones fused, serially within the group as the reference does (:541-566)
//     summary   per fused window: the ORFs inside it -- count, k_min / k_max, the table log-sum of their Forward scores in the
//               reference's order, P_min, P_tot (:1376-1415, :1457)
//     layout    the pool offsets of the windows' copies and the sequence-block view the parsers read
//   fs_build_windows_host     the fallback for inputs the kernels do not take (more than 32768 surviving ORFs or 65536 hit windows
//     in a block, more than 16 cascade lanes, more than 1024 surviving ORFs on one strand of one sequence, a hit window beyond what the
//     kernels' key holds: hit_key_fits; BATH_HIP_FS_WINDOWS_HOST=1
//     sends every block here): the same steps as loops over the same rules, from the survivor lists fetched to the host, the
//     (sequence, strand) groups spread over up to four threads
// Both leave the same product (FsWinBuild): the ordered ORFs, the windows' records, gather descriptors, pool offsets and lengths, on
// the host (page-locked) and in the same device buffers.  After the parsers fs_decide forms null / bias / Forward scores -> P-values ->
// the branch of each window (:1425-1465) by the same rule where the windows were built: fsw_decide_kernel, the host reading the
// completed records once, or a host loop with libm's exp / log for a block of the host build.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"
#include "bath_fs_device.hpp"

namespace bath {

namespace {

constexpr int kMaxOrfs = 32768, kMaxHitWins = 65536, kMaxGroup = 1024;
// BATH_HIP_FSW_MAX_GROUP=g (tests): groups of more than g ORFs send the block to the host path, so that the fallback runs on small inputs
static int max_group() { static const int g = [] { const char *e = std::getenv("BATH_HIP_FSW_MAX_GROUP"); return e ? std::max(1, std::min(std::atoi(e), kMaxGroup)) : kMaxGroup; }(); return g; }
struct Key { uint64_t hi, lo; };
__host__ __device__ __forceinline__ bool key_less(const Key &a, const Key &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

struct DnaWinDev { int32_t n, k, length; };
struct BuildParams {
  int M, max_length;
  const float *prefix, *suffix;       // [M+1] P7_SCOREDATA window padding fractions (device or host arrays, as the caller's side reads them)
  double F3, ftau, flambda;
  int std_pipe;
  const float *tbl;                   // p7_FLogsum's table on the device (the host has flogsum_host)
};

// ================================================================================================================================
// The rules of p7_pli_BuildDNAWindows and of p7_pli_Frameshift's window summary, each stated once for the kernels and the host path.
// ================================================================================================================================

// min / max of 64-bit integers (host code resolves the unqualified names to the 32-bit overloads)
__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return (a < b) ? a : b; }
__host__ __device__ inline int64_t max64(int64_t a, int64_t b) { return (a > b) ? a : b; }

// an F4 survivor as a cascade lane left it -> the ORF record, ids and offsets made the block's own; no hit window seen yet
__host__ __device__ inline FsOrfDev fsw_orf_init(const FsCandRec &q, int64_t first_window, int64_t dpool, int32_t cand_base) {
  FsOrfDev o;
  o.w = q.window + first_window; o.aa_off = q.aa_off + dpool; o.P = q.P; o.cand = q.cand + cand_base;
  o.strand = q.sf / 3; o.n = q.len; o.start = q.sf % 3 + 3 * q.startj + 1; o.end = o.start + 3 * o.n - 1;
  o.fwd_null = q.fwdsc - q.nullsc;                                   // pli_tmp->fwdsc (p7_pipeline.c:1782)
  o.wb = -1; o.we = 0; o.dw_n = 0; o.dw_len = 0; o.dw_k = 0; o.kmin = 0x7fffffff; o.kmax = 0; o.g0 = o.g1 = 0; o.pad_ = 0;
  return o;
}

// the key that orders the ORFs: (sequence, strand), then the order esl_gencode emits a strand's ORFs -- when their closing stop
// codon is read; ORFs still open at the end follow, frame by frame.  The candidate id makes the keys pairwise different.
__host__ __device__ inline Key fsw_orf_key(const FsOrfDev &o, int n_seq) {
  const uint64_t ea = (o.end + 3 > n_seq) ? 1 : 0;
  const uint64_t val = ea ? (uint64_t)((o.start - 1) % 3) : (uint64_t)o.end;
  return Key{((uint64_t)o.w << 1) | (uint64_t)o.strand, (ea << 62) | (val << 31) | (uint64_t)(uint32_t)o.cand};
}

// the ORF's best hit window (o.wb: its index in <wins>, -1: none) says which DNA window the ORF asks for (p7_pipeline.c:486-527)
__host__ __device__ inline void fsw_orf_window(FsOrfDev &o, const WindowRec *wins, int n_seq, const BuildParams &p) {
  const int best = o.wb;
  int32_t cn, ck, cl;
  if (best >= 0) { cn = wins[best].n; ck = wins[best].k; cl = wins[best].length; o.we = best + 1; }
  else if (o.n >= p.M) { cn = (o.n - p.M) / 2 + 1; ck = p.M; cl = p.M; }            // :500-510: no window, centre of the model
  else { cn = 1; ck = p.M - ((p.M - o.n) / 2); cl = o.n; }
  if (best < 0) { o.wb = 0; o.we = 0; o.kmin = p.M; o.kmax = 0; }
  int64_t ws = (int64_t)((double)(uint32_t)cn - ((double)p.max_length * (0.1 + (double)p.prefix[ck - cl + 1])) + 1);     // :513
  int64_t wend = (int64_t)((double)((uint32_t)cn + (uint32_t)cl) + ((double)p.max_length * (0.1 + (double)p.suffix[ck])) - 2);   // :514
  ws = min64(0, ws);                                            // :516-517 (sic)
  wend = max64(o.n, wend);
  ws = max64(1, (int64_t)o.start + ws * 3);                     // :520-527, o.start already on the strand being read
  wend = min64(n_seq, (int64_t)o.start + wend * 3);
  o.dw_n = (int32_t)ws; o.dw_k = ck; o.dw_len = (int32_t)(wend - ws + 1);
}

// a group's windows wl[g0, g1), ordered by start: overlapping ones fused, left to right (:541-566, pct_overlap = 0); returns the windows left
__host__ __device__ inline int fsw_fuse(DnaWinDev *wl, int g0, int g1, int max_length) {
  int keep = g0;
  for (int i = g0 + 1; i < g1; i++) {
    DnaWinDev prev = wl[keep];
    const DnaWinDev cur = wl[i];
    const int64_t pe = (int64_t)prev.n + prev.length - 1, ce = (int64_t)cur.n + cur.length - 1;
    const int32_t ov = (int32_t)(min64(pe, ce) - max64(prev.n, cur.n) + 1);
    const int64_t ms = min64(prev.n, cur.n), me = max64(pe, ce);
    const int32_t ml = (int32_t)(me - ms + 1);
    if (((float)ov / (float)min(prev.length, cur.length) > 0.f) && ml < (2 * (max_length * 3))) { prev.n = (int32_t)ms; prev.length = ml; wl[keep] = prev; }
    else wl[++keep] = cur;
  }
  return keep - g0 + 1;
}

// a window's span in the coordinates of its sequence (:1373-1374), and whether an ORF of that strand lies inside it (:1405)
struct WinSpan { int64_t dstart, wstart, wend; };
__host__ __device__ inline WinSpan fsw_span(int strand, int n_seq, int32_t dw_n, int32_t dw_len) {
  WinSpan sp;
  sp.dstart = strand ? n_seq : 1;                                      // dnasq->start of a whole sequence
  sp.wstart = strand ? sp.dstart - ((int64_t)dw_n + dw_len) : sp.dstart + dw_n - 1;
  sp.wend = strand ? sp.dstart - dw_n + 1 : sp.wstart + dw_len - 1;
  return sp;
}
__host__ __device__ inline bool fsw_orf_inside(const FsOrfDev &o, int strand, int n_seq, const WinSpan &sp) {
  int64_t os, oe;
  if (strand) { const int64_t rs = (int64_t)n_seq - o.start + 1, re = (int64_t)n_seq - o.end + 1; os = sp.dstart - (n_seq - re + 1) + 1; oe = sp.dstart - (n_seq - rs + 1) + 1; }
  else { os = sp.dstart + o.start - 1; oe = sp.dstart + o.end - 1; }
  return os >= sp.wstart && oe <= sp.wend;
}

// a fused window <dw> of the group orfs[g0, g1): the summary of the ORFs that lie inside it (p7_pipeline.c:1376-1415) -> the record
// and the gather descriptor.  <seq_off>: the sequences' offsets in the DNA block; <logsum>: p7_FLogsum as the caller's side has it.
template <class LogSum>
__host__ __device__ inline void fsw_summarize(const FsOrfDev *orfs, int g0, int g1, const DnaWinDev &dw, int n_seq, const int64_t *seq_off, const BuildParams &p,
                                              LogSum logsum, bath_fs_window *out, FsWinDev *desc) {
  const int64_t w = orfs[g0].w;
  const int strand = orfs[g0].strand;
  const WinSpan sp = fsw_span(strand, n_seq, dw.n, dw.length);
  int orf_cnt = 0, k_min = p.M, k_max = 0;
  float tot = -INFINITY;
  double P_min = INFINITY;
  for (int b = g0; b < g1; b++) {
    const FsOrfDev &o = orfs[b];
    if (!fsw_orf_inside(o, strand, n_seq, sp)) continue;
    P_min = fmin(P_min, o.P);
    tot = logsum(tot, o.fwd_null);
    orf_cnt++;
    if (o.we > o.wb) { k_min = min(k_min, o.kmin); k_max = max(k_max, o.kmax); }
  }
  bath_fs_window r;
  memset(&r, 0, sizeof r);
  r.window = w; r.strand = strand; r.n = dw.n; r.length = dw.length;
  r.orf_cnt = orf_cnt; r.k_min = k_min; r.k_max = k_max; r.tot_orfsc = tot; r.P_min = P_min;
  const double x = (double)tot / 0.69314718055994529;
  r.P_tot = p.std_pipe ? ((x < p.ftau) ? 1.0 : exp(-p.flambda * (x - p.ftau))) : 1.0;              // :1457; --fsonly: 1
  *out = r;
  FsWinDev d;
  d.src_off = seq_off[w]; d.dst_off = 0; d.seq_n = n_seq; d.start = dw.n; d.len = dw.length; d.strand = strand; d.kmin = k_min; d.kmax = k_max;
  *desc = d;
}

// p7_pipeline.c:1425-1465 for one window: null score (p7_bg_fs_NullOne), bias filter score (p7_bg_fs_FilterScore: the three frames'
// Forward scores of the 2-state filter HMM from fs_bias_kernel, <bias>[2][3], summed with the table, plus the length term), Forward
// score -> P-values -> branch.  <lt>: the two terms that depend on the window's length alone, from the host's libm on either path
// (fsw_len_terms; the kernel looks them up, as the cascade's kernels look up theirs: the device's logf is not libm's to the last bit, and
// L3 * logf(p1) carries that bit into the filter score and the P-value)
struct FswLen { float null_frame, filt; };
inline FswLen fsw_len_terms(int L3) {
  const float p1 = (float)L3 / (float)(L3 + 1);
  return FswLen{(float)((float)L3 * std::log((double)p1) + std::log(1. - p1)),                         // p7_bg_fs_NullOne, p7_bg.c:380
                (float)L3 * logf(p1) + logf((float)(1. - p1))};                                        // p7_bg.c:561
}
template <class LogSum>
__host__ __device__ inline void fsw_decide(bath_fs_window &r, const float *bias, float fwdsc, const FswLen lt, LogSum logsum, int do_biasfilter, int std_pipe, double F3, double tau3, double lambda) {
  const double kLn2 = 0.69314718055994529, kLn3 = 1.0986122886681098;
  r.nullsc = (float)(lt.null_frame + kLn3);
  if (do_biasfilter) {
    float f2[2];
    for (int pass = 0; pass < 2; pass++) {
      const float *b = &bias[pass * 3];
      float sum = -INFINITY;
      for (int f = 0; f < 3; f++) sum = logsum(sum, b[f]);
      f2[pass] = (float)((double)sum + ((double)lt.filt + kLn3));                                      // p7_bg.c:561
    }
    r.filtersc = f2[0];
    if (r.k_min <= r.k_max && f2[1] > r.filtersc) r.filtersc = f2[1];                                  // :1432-1440
  } else r.filtersc = r.nullsc;
  r.fwdsc = fwdsc;
  const float seqscore = (float)((r.fwdsc - r.filtersc) / kLn2);
  const double x1 = (double)seqscore, x2 = (r.fwdsc - r.nullsc) / kLn2;
  r.P_fs = (x1 < tau3) ? 1.0 : exp(-lambda * (x1 - tau3));
  r.P_null = (x2 < tau3) ? 1.0 : exp(-lambda * (x2 - tau3));
  if (r.P_fs <= F3 && (r.P_null < r.P_tot || (r.P_null == r.P_tot && r.orf_cnt > 1) || r.P_min > F3)) r.branch = 1;
  else r.branch = std_pipe ? 2 : 0;                                                                    // :1480: --fsonly has no standard branch
}

// a window's copy in the pool: padded to 16 bytes + 16
__host__ __device__ inline long long fsw_pool_pitch(int len) { return ((long long)len + 15) / 16 * 16 + 16; }

struct LaneArgs { FsLaneSurv l[16]; int n; int c_begin[17], w_begin[17]; };

// the lanes' survivors as one list with the block's own ids, and the key that orders the ORFs
__global__ void fsw_merge_kernel(LaneArgs L, const int32_t *__restrict__ seq_len, FsOrfDev *__restrict__ orfs, Key *__restrict__ okey,
                                 WindowRec *__restrict__ wins) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_c = L.c_begin[L.n], n_w = L.w_begin[L.n];
  if (t < n_c) {
    int k = 0;
    while (t >= L.c_begin[k + 1]) k++;
    const FsCandRec q = L.l[k].d_c[t - L.c_begin[k]];
    const FsOrfDev o = fsw_orf_init(q, L.l[k].first_window, L.l[k].dpool, L.l[k].cand_base);
    orfs[t] = o;
    okey[t] = fsw_orf_key(o, seq_len[o.w]);
  }
  if (t < n_w) {
    int k = 0;
    while (t >= L.w_begin[k + 1]) k++;
    WindowRec w = L.l[k].d_w[t - L.w_begin[k]];
    w.cand += L.l[k].cand_base;
    wins[t] = w;
  }
}

// rank[i] += number of keys of this block's column range that are smaller than key i (the keys are pairwise different; rank zeroed
// before): the list's order without a sort network.  grid (rows of 256 keys, column ranges): the n^2 comparisons fill the chip.
__global__ __launch_bounds__(256) void fsw_rank_kernel(const Key *__restrict__ key, int n, int32_t *__restrict__ rank) {
  __shared__ Key tile[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Key mine = i < n ? key[i] : Key{~0ull, ~0ull};
  const int ntiles = (n + 255) / 256;
  const int t0 = (int)((long long)ntiles * blockIdx.y / gridDim.y), t1 = (int)((long long)ntiles * (blockIdx.y + 1) / gridDim.y);
  int r = 0;
  for (int t = t0; t < t1; t++) {
    const int j0 = t * 256;
    __syncthreads();
    if (j0 + (int)threadIdx.x < n) tile[threadIdx.x] = key[j0 + threadIdx.x];
    __syncthreads();
    const int m = min(256, n - j0);
    for (int j = 0; j < m; j++) r += key_less(tile[j], mine) ? 1 : 0;
  }
  if (i < n && r) atomicAdd(&rank[i], r);
}

// after the ORFs are in order: slot_of[cand] = the ORF's place (slot_of is -1 elsewhere)
__global__ void fsw_slot_kernel(const FsOrfDev *__restrict__ orfs, int n, int32_t *__restrict__ slot_of) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) slot_of[orfs[s].cand] = s;
}

// a hit window's rank among its ORF's windows as one integer: highest score first, then the longest, then the leftmost (:486-495).
// The key holds 12 bits of length and 20 bits of start, and the second pass 15 bits of k: hit_key_fits says whether a window fits
// (a block with one that does not goes to the host path).
__host__ __device__ __forceinline__ bool hit_key_fits(const WindowRec &x) { return (uint32_t)x.length <= 0xfffu && (uint32_t)x.n <= 0xfffffu && (uint32_t)x.k <= 0x7fffu; }
__device__ __forceinline__ unsigned long long hit_key(const WindowRec &x) {
  uint32_t u = __float_as_uint(x.score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                     // floats in their order as unsigned integers
  return ((unsigned long long)u << 32) | ((unsigned long long)((uint32_t)x.length & 0xfffu) << 20) | (unsigned long long)(0xfffffu - ((uint32_t)x.n & 0xfffffu));
}
// per hit window, pass 1: the best key and k_min / k_max of its ORF; pass 2: among the windows that hold the best key (equal score,
// length and start) the one with the smallest k, whatever order the select kernels appended them in: orfs[s].wb = k << 16 | index
// (fsw_orf_kernel takes the index out; records equal in k as well are interchangeable)
__global__ void fsw_hits1_kernel(const WindowRec *__restrict__ wins, int nhw, const int32_t *__restrict__ slot_of, unsigned long long *__restrict__ best_key, FsOrfDev *__restrict__ orfs,
                                 int *__restrict__ flags) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nhw) return;
  const WindowRec x = wins[t];
  const int s = slot_of[x.cand];
  if (s < 0) return;
  if (!hit_key_fits(x)) { atomicOr(flags, 1); return; }                 // the host path takes such a block
  atomicMax(&best_key[s], hit_key(x));
  atomicMin(&orfs[s].kmin, x.k - x.length + 1);
  atomicMax(&orfs[s].kmax, x.k);
}
__global__ void fsw_hits2_kernel(const WindowRec *__restrict__ wins, int nhw, const int32_t *__restrict__ slot_of, const unsigned long long *__restrict__ best_key, FsOrfDev *__restrict__ orfs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nhw) return;
  const WindowRec x = wins[t];
  const int s = slot_of[x.cand];
  if (s < 0 || !hit_key_fits(x) || hit_key(x) != best_key[s]) return;
  atomicMin(reinterpret_cast<unsigned int *>(&orfs[s].wb), ((unsigned int)x.k << 16) | (unsigned int)t);   // wb starts at -1 = 0xffffffff: "no hit window"; t < kMaxHitWins = 2^16
}

template <class T>
__global__ void fsw_scatter_kernel(const T *__restrict__ in, const int32_t *__restrict__ rank, int n, T *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[rank[i]] = in[i];
}

// per ORF (in order): its best hit window says which DNA window the ORF asks for
__global__ void fsw_orf_kernel(FsOrfDev *__restrict__ orfs, int n, const WindowRec *__restrict__ wins, const int32_t *__restrict__ seq_len, BuildParams p) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  FsOrfDev o = orfs[s];
  o.wb = (o.wb >= 0) ? (o.wb & 0xffff) : -1;                           // fsw_hits2_kernel's k << 16 | index
  fsw_orf_window(o, wins, seq_len[o.w], p);
  orfs[s] = o;
}

// per ORF: the bounds of its (sequence, strand) group, and its window's place in the group's list ordered by start
// (p7_hmmwindow_SortByStart; equal starts keep the ORFs' order)
__global__ void fsw_group_kernel(FsOrfDev *__restrict__ orfs, int n, DnaWinDev *__restrict__ sorted, int *__restrict__ flags, int group_cap) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int64_t w = orfs[s].w;
  const int strand = orfs[s].strand;
  int g0 = s, g1 = s + 1;
  while (g0 > 0 && orfs[g0 - 1].w == w && orfs[g0 - 1].strand == strand && s - g0 <= kMaxGroup) g0--;
  while (g1 < n && orfs[g1].w == w && orfs[g1].strand == strand && g1 - s <= kMaxGroup) g1++;
  if (g1 - g0 > group_cap) { atomicOr(flags, 1); return; }             // the host path takes such a block
  const int32_t my_n = orfs[s].dw_n;
  int r = 0;
  for (int b = g0; b < g1; b++) { const int32_t bn = orfs[b].dw_n; r += (bn < my_n || (bn == my_n && b < s)) ? 1 : 0; }
  sorted[g0 + r] = DnaWinDev{my_n, orfs[s].dw_k, orfs[s].dw_len};
  orfs[s].g0 = g0; orfs[s].g1 = g1;
}

// per group (its first ORF's thread): overlapping windows fused; cnt[g0] = windows left
__global__ void fsw_fuse_kernel(const FsOrfDev *__restrict__ orfs, int n, DnaWinDev *__restrict__ wl, int32_t *__restrict__ cnt, int max_length) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int g0 = orfs[s].g0, g1 = orfs[s].g1;
  cnt[s] = (s != g0) ? 0 : fsw_fuse(wl, g0, g1, max_length);
}

// exclusive prefix sums of cnt[0..n) by one block; total -> hdr[0]
__global__ __launch_bounds__(1024) void fsw_scan_kernel(const int32_t *__restrict__ cnt, int n, int32_t *__restrict__ base, int32_t *__restrict__ hdr) {
  __shared__ int part[1024];
  const int per = (n + 1023) / 1024;
  const int b = threadIdx.x * per, e = min(n, b + per);
  int s = 0;
  for (int i = b; i < e; i++) s += cnt[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int i = b; i < e; i++) { base[i] = run; run += cnt[i]; }
  if (threadIdx.x == 1023) hdr[0] = part[1023];
}

// per fused window: its summary, the record and the gather descriptor
__global__ void fsw_summary_kernel(const FsOrfDev *__restrict__ orfs, int n, const DnaWinDev *__restrict__ wl, const int32_t *__restrict__ cnt,
                                   const int32_t *__restrict__ base, const int64_t *__restrict__ seq_off, const int32_t *__restrict__ seq_len, BuildParams p,
                                   bath_fs_window *__restrict__ out, FsWinDev *__restrict__ desc, int32_t *__restrict__ grp) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int g0 = orfs[s].g0, g1 = orfs[s].g1;
  if (s - g0 >= cnt[g0]) return;
  const int64_t w = orfs[g0].w;
  const int idx = base[g0] + (s - g0);
  fsw_summarize(orfs, g0, g1, wl[s], seq_len[w], seq_off, p, [tbl = p.tbl](float a, float b) { return flogsum_g(a, b, tbl); }, &out[idx], &desc[idx]);
  grp[2 * idx] = g0; grp[2 * idx + 1] = g1;
}

// the pool offsets of the windows' copies (each padded to 16 bytes + 16), the view's off[] / len[], and the header:
// hdr = {windows, flags, longest window, -, pool bytes (2 ints), total nucleotides (2 ints)}
__global__ __launch_bounds__(1024) void fsw_layout_kernel(FsWinDev *__restrict__ desc, int32_t *__restrict__ hdr, int64_t *__restrict__ voff, int32_t *__restrict__ vlen) {
  __shared__ long long part[1024];
  __shared__ int pmax[1024];
  const int nw = hdr[0];
  const int per = (nw + 1023) / 1024;
  const int b = threadIdx.x * per, e = min(nw, b + per);
  long long s = 0, tot = 0;
  int mx = 0;
  for (int i = b; i < e; i++) { const int len = desc[i].len; s += fsw_pool_pitch(len); tot += len; mx = max(mx, len); }
  part[threadIdx.x] = s; pmax[threadIdx.x] = mx;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const long long v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    const int m = threadIdx.x >= d ? pmax[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v; pmax[threadIdx.x] = max(pmax[threadIdx.x], m);
    __syncthreads();
  }
  long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int i = b; i < e; i++) {
    const int len = desc[i].len;
    desc[i].dst_off = run; voff[i] = run; vlen[i] = len;
    run += fsw_pool_pitch(len);
  }
  // total nucleotides: a second, tiny reduction through the same array
  __syncthreads();
  const long long pool = part[1023];
  const int longest = pmax[1023];
  __syncthreads();
  part[threadIdx.x] = tot;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) { if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d]; __syncthreads(); }
  if (threadIdx.x == 0) {
    hdr[2] = longest;
    memcpy(&hdr[4], &pool, 8);
    const long long total = part[0];
    memcpy(&hdr[6], &total, 8);
  }
}

// per window, after the parsers: the branch decision
__global__ void fsw_decide_kernel(bath_fs_window *__restrict__ out, int nw, const float *__restrict__ bias /* [nw][2][3] */, const float *__restrict__ fsc,
                                  const float *__restrict__ tbl, const FswLen *__restrict__ len_terms /* by L3 */, int do_biasfilter, int std_pipe, double F3, double tau3, double lambda) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nw) return;
  bath_fs_window r = out[i];
  fsw_decide(r, &bias[(size_t)i * 6], fsc[i], len_terms[r.length / 3], [tbl](float a, float b) { return flogsum_g(a, b, tbl); }, do_biasfilter, std_pipe, F3, tau3, lambda);
  out[i] = r;
}

}  // namespace

// What a build leaves in Scratch::kFsWindowResult and (regions A and B) in the page-locked Pinned::kFsWindowResult, records back to back.  Two regions for the
// device path's read-back: A = what the host needs BEFORE it can launch the parsers (header, the windows' pool offsets and lengths),
// B = what it reads after the branch decision (ordered ORFs, group bounds; the records travel then, completed).
struct ResLayout { size_t hdr, voff, vlen, a_bytes, orf, grp, b_end, out, desc, bytes; };
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static ResLayout res_layout(int n) {
  static_assert(kMaxHitWins <= 0x10000, "fsw_hits2_kernel keeps a hit window's index in 16 bits");
  static_assert(sizeof(FsOrfDev) % 8 == 0 && sizeof(bath_fs_window) % 8 == 0 && sizeof(FsWinDev) % 8 == 0, "records are laid out back to back");
  ResLayout r;
  r.hdr = 0; r.voff = 256; r.vlen = r.voff + al256((size_t)n * 8); r.a_bytes = r.vlen + al256((size_t)n * 4);
  r.orf = r.a_bytes; r.grp = r.orf + al256((size_t)n * sizeof(FsOrfDev)); r.b_end = r.grp + al256((size_t)n * 8);
  r.out = r.b_end; r.desc = r.out + al256((size_t)n * sizeof(bath_fs_window)); r.bytes = r.desc + al256((size_t)n * sizeof(FsWinDev));
  return r;
}
// the product's pointers into the two buffers
static void res_bind(const ResLayout &r, char *h, char *d, FsWinBuild *B) {
  B->h_orfs = reinterpret_cast<const FsOrfDev *>(h + r.orf); B->h_grp = reinterpret_cast<const int32_t *>(h + r.grp);
  B->h_voff = reinterpret_cast<const int64_t *>(h + r.voff); B->h_vlen = reinterpret_cast<const int32_t *>(h + r.vlen);
  B->h_out = reinterpret_cast<const bath_fs_window *>(h + r.out);
  B->d_out = reinterpret_cast<bath_fs_window *>(d + r.out); B->d_desc = reinterpret_cast<const FsWinDev *>(d + r.desc);
  B->d_voff = reinterpret_cast<const int64_t *>(d + r.voff); B->d_vlen = reinterpret_cast<const int32_t *>(d + r.vlen);
}

bool fs_windows_on_device() {
  static const bool host = [] { const char *e = std::getenv("BATH_HIP_FS_WINDOWS_HOST"); return e && e[0] == '1'; }();
  return !host;
}

int fs_build_windows_device(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna,
                            const bath_pipeline_params *prm, const FsLaneSurv *lanes, int nlanes, int nc_total, FsWinBuild *B) {
  *B = FsWinBuild{};
  if (nlanes > 16) return BATH_ENORESULT;
  LaneArgs L{};
  L.n = nlanes;
  for (int k = 0; k < nlanes; k++) { L.l[k] = lanes[k]; L.c_begin[k + 1] = L.c_begin[k] + lanes[k].n_c; L.w_begin[k + 1] = L.w_begin[k] + lanes[k].n_w; }
  const int n = L.c_begin[nlanes], nhw = L.w_begin[nlanes];
  if (n == 0) return BATH_OK;
  if (n > kMaxOrfs || nhw > kMaxHitWins) return BATH_ENORESULT;
  const int M = om->M;
  // the window padding fractions of P7_SCOREDATA, once per profile and context
  DevBuf &b_pad = ctx->scratch[Scratch::kFsWindowPadding];
  if (ctx->fsw_pad_uid != om->uid || !b_pad.p) {
    BATH_HIP_TRY(ctx, b_pad.reserve((size_t)(M + 1) * 2 * sizeof(float) + 64));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(b_pad.p, om->prefix_lengths.data(), (size_t)(M + 1) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(b_pad.as<float>() + (M + 1), om->suffix_lengths.data(), (size_t)(M + 1) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->fsw_pad_uid = om->uid;
  }
  // workspace: the unordered ORFs, their keys and ranks, the hit windows, candidate -> slot, best keys, the groups' window lists, counts
  auto al = al256;
  const size_t o_orf0 = 0, o_okey = o_orf0 + al((size_t)n * sizeof(FsOrfDev)), o_orank = o_okey + al((size_t)n * sizeof(Key)),
               o_win = o_orank + al((size_t)n * 4), o_slot = o_win + al((size_t)std::max(nhw, 1) * sizeof(WindowRec)), o_best = o_slot + al((size_t)std::max(nc_total, 1) * 4),
               o_wl = o_best + al((size_t)n * 8), o_cnt = o_wl + al((size_t)n * sizeof(DnaWinDev)), o_base = o_cnt + al((size_t)n * 4), ws_bytes = o_base + al((size_t)n * 4);
  const ResLayout R = res_layout(n);
  DevBuf &b_ws = ctx->scratch[Scratch::kFsWindowWork], &b_res = ctx->scratch[Scratch::kFsWindowResult];
  BATH_HIP_TRY(ctx, b_ws.reserve(ws_bytes + 256));
  BATH_HIP_TRY(ctx, b_res.reserve(R.bytes + 256));
  if (ctx->stage[Pinned::kFsWindowResult].reserve(R.b_end + 256) != hipSuccess) { ctx->set_error("cannot allocate page-locked staging memory"); return BATH_EFAIL; }
  char *ws = b_ws.as<char>(), *rs = b_res.as<char>();
  FsOrfDev *d_orf0 = reinterpret_cast<FsOrfDev *>(ws + o_orf0), *d_orf = reinterpret_cast<FsOrfDev *>(rs + R.orf);
  Key *d_okey = reinterpret_cast<Key *>(ws + o_okey);
  int32_t *d_orank = reinterpret_cast<int32_t *>(ws + o_orank), *d_slot = reinterpret_cast<int32_t *>(ws + o_slot);
  WindowRec *d_win = reinterpret_cast<WindowRec *>(ws + o_win);
  unsigned long long *d_best = reinterpret_cast<unsigned long long *>(ws + o_best);
  DnaWinDev *d_wl = reinterpret_cast<DnaWinDev *>(ws + o_wl);
  int32_t *d_cnt = reinterpret_cast<int32_t *>(ws + o_cnt), *d_base = reinterpret_cast<int32_t *>(ws + o_base);
  int32_t *d_hdr = reinterpret_cast<int32_t *>(rs + R.hdr), *d_grp = reinterpret_cast<int32_t *>(rs + R.grp);
  bath_fs_window *d_out = reinterpret_cast<bath_fs_window *>(rs + R.out);
  FsWinDev *d_desc = reinterpret_cast<FsWinDev *>(rs + R.desc);
  int64_t *d_voff = reinterpret_cast<int64_t *>(rs + R.voff);
  int32_t *d_vlen = reinterpret_cast<int32_t *>(rs + R.vlen);
  hipStream_t s = ctx->stream;
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, 256, s));
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_orank, 0, (size_t)n * 4, s));
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_slot, 0xff, (size_t)std::max(nc_total, 1) * 4, s));
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_best, 0, (size_t)n * 8, s));
  const BuildParams p{M, om->max_length, b_pad.as<float>(), b_pad.as<float>() + (M + 1), prm->F3, (double)om->evparam[BATH_FTAU], (double)om->evparam[BATH_FLAMBDA],
                      prm->std_pipe, om_fs3->d_logsum};
  const int T = 256, gn = (n + T - 1) / T, gm = (std::max(n, nhw) + T - 1) / T, gh = (nhw + T - 1) / T;
  const int cols = std::max(1, std::min(gn, (ctx->prop.multiProcessorCount * 4) / std::max(gn, 1)));      // column ranges: about four blocks per CU in all
  hipLaunchKernelGGL(fsw_merge_kernel, dim3(gm), dim3(T), 0, s, L, dna->d_len, d_orf0, d_okey, d_win);
  hipLaunchKernelGGL(fsw_rank_kernel, dim3(gn, cols), dim3(256), 0, s, d_okey, n, d_orank);
  hipLaunchKernelGGL(fsw_scatter_kernel<FsOrfDev>, dim3(gn), dim3(T), 0, s, d_orf0, d_orank, n, d_orf);
  if (nhw > 0) {
    hipLaunchKernelGGL(fsw_slot_kernel, dim3(gn), dim3(T), 0, s, d_orf, n, d_slot);
    hipLaunchKernelGGL(fsw_hits1_kernel, dim3(gh), dim3(T), 0, s, d_win, nhw, d_slot, d_best, d_orf, d_hdr + 1);
    hipLaunchKernelGGL(fsw_hits2_kernel, dim3(gh), dim3(T), 0, s, d_win, nhw, d_slot, d_best, d_orf);
  }
  hipLaunchKernelGGL(fsw_orf_kernel, dim3(gn), dim3(T), 0, s, d_orf, n, d_win, dna->d_len, p);
  hipLaunchKernelGGL(fsw_group_kernel, dim3(gn), dim3(T), 0, s, d_orf, n, d_wl, d_hdr + 1, max_group());
  hipLaunchKernelGGL(fsw_fuse_kernel, dim3(gn), dim3(T), 0, s, d_orf, n, d_wl, d_cnt, om->max_length);
  hipLaunchKernelGGL(fsw_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, n, d_base, d_hdr);
  hipLaunchKernelGGL(fsw_summary_kernel, dim3(gn), dim3(T), 0, s, d_orf, n, d_wl, d_cnt, d_base, dna->d_off, dna->d_len, p, d_out, d_desc, d_grp);
  hipLaunchKernelGGL(fsw_layout_kernel, dim3(1), dim3(1024), 0, s, d_desc, d_hdr, d_voff, d_vlen);
  BATH_HIP_TRY(ctx, hipGetLastError());
  // region A now (the one synchronize of this stage), region B behind it on the same stream: it is complete long before the
  // decision's synchronize, which is the next time the host looks
  char *h = static_cast<char *>(ctx->stage[Pinned::kFsWindowResult].p);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h, rs, R.a_bytes, hipMemcpyDeviceToHost, s));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(s));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h + R.a_bytes, rs + R.a_bytes, R.b_end - R.a_bytes, hipMemcpyDeviceToHost, s));
  const int32_t *hdr = reinterpret_cast<const int32_t *>(h + R.hdr);
  if (hdr[1] != 0) { BATH_HIP_TRY(ctx, hipStreamSynchronize(s)); return BATH_ENORESULT; }      // a group beyond kMaxGroup: the host path
  B->n_orfs = n; B->nw = hdr[0]; B->maxlen = hdr[2];
  std::memcpy(&B->pool_bytes, &hdr[4], 8); std::memcpy(&B->total, &hdr[6], 8);
  res_bind(R, h, rs, B);
  return BATH_OK;
}

// The same product from the survivor lists on the host: <sel> in ascending candidate id, <wins> by (candidate id, start, k), ids the block's own
// (fs_order_survivors, fs_merge_survivors).
int fs_build_windows_host(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                          const FsCandRec *sel, int n, const WindowRec *wins, int nhw, FsWinBuild *B) {
  *B = FsWinBuild{};
  if (n == 0) return BATH_OK;
  const ResLayout R = res_layout(n);
  DevBuf &b_res = ctx->scratch[Scratch::kFsWindowResult];
  BATH_HIP_TRY(ctx, b_res.reserve(R.bytes + 256));
  if (ctx->stage[Pinned::kFsWindowResult].reserve(R.bytes + 256) != hipSuccess) { ctx->set_error("cannot allocate page-locked staging memory"); return BATH_EFAIL; }
  char *h = static_cast<char *>(ctx->stage[Pinned::kFsWindowResult].p);
  FsOrfDev *orfs = reinterpret_cast<FsOrfDev *>(h + R.orf);
  int32_t *grp = reinterpret_cast<int32_t *>(h + R.grp), *vlen = reinterpret_cast<int32_t *>(h + R.vlen);
  int64_t *voff = reinterpret_cast<int64_t *>(h + R.voff);
  bath_fs_window *out = reinterpret_cast<bath_fs_window *>(h + R.out);
  FsWinDev *desc = reinterpret_cast<FsWinDev *>(h + R.desc);
  const BuildParams p{om->M, om->max_length, om->prefix_lengths.data(), om->suffix_lengths.data(), prm->F3, (double)om->evparam[BATH_FTAU], (double)om->evparam[BATH_FLAMBDA],
                      prm->std_pipe, nullptr};

  // ---- the ORFs with their best hit window (highest score, then longest, then first -- in <wins>' order, the leftmost and of those the one with the smallest k: :486-495) and k_min / k_max, then in the reference's order
  struct Keyed { Key key; FsOrfDev o; };
  std::vector<Keyed> keyed((size_t)n);
  for (int i = 0, wi = 0; i < n; i++) {
    FsOrfDev o = fsw_orf_init(sel[i], 0, 0, 0);
    while (wi < nhw && wins[wi].cand < o.cand) wi++;
    for (; wi < nhw && wins[wi].cand == o.cand; wi++) {
      const WindowRec &x = wins[wi];
      if (o.wb < 0 || x.score > wins[o.wb].score || (x.score == wins[o.wb].score && x.length > wins[o.wb].length)) o.wb = wi;
      o.kmin = std::min(o.kmin, x.k - x.length + 1); o.kmax = std::max(o.kmax, x.k);
    }
    keyed[(size_t)i] = Keyed{fsw_orf_key(o, dna->h_len[(size_t)o.w]), o};
  }
  std::sort(keyed.begin(), keyed.end(), [](const Keyed &a, const Keyed &b) { return key_less(a.key, b.key); });
  std::vector<int> gstart;                                                   // first ORF of every (sequence, strand) group, and the end
  for (int s = 0; s < n; s++) {
    orfs[s] = keyed[(size_t)s].o;
    if (s == 0 || orfs[s].w != orfs[s - 1].w || orfs[s].strand != orfs[s - 1].strand) gstart.push_back(s);
  }
  gstart.push_back(n);
  const size_t ngroups = gstart.size() - 1;

  // ---- per group: the ORFs' windows, ordered by start (p7_hmmwindow_SortByStart) and fused, and the summary of every window that is
  // left, at the slot of the group's ORF of the same rank.  The groups are independent: host threads take contiguous runs of them.
  std::vector<DnaWinDev> wl((size_t)n);
  std::vector<bath_fs_window> out_slot((size_t)n);
  std::vector<FsWinDev> desc_slot((size_t)n);
  std::vector<int> cnt(ngroups);
  const int nparts = (int)std::max<size_t>(1, std::min<size_t>(4, ngroups / 256));
  auto build = [&](int part) {
    const size_t gb = ngroups * (size_t)part / (size_t)nparts, ge = ngroups * (size_t)(part + 1) / (size_t)nparts;
    for (size_t gi = gb; gi < ge; gi++) {
      const int g0 = gstart[gi], g1 = gstart[gi + 1];
      const int64_t w = orfs[g0].w;
      const int n_seq = dna->h_len[(size_t)w];
      for (int s = g0; s < g1; s++) {
        FsOrfDev &o = orfs[s];
        fsw_orf_window(o, wins, n_seq, p);
        o.g0 = g0; o.g1 = g1;
        wl[(size_t)s] = DnaWinDev{o.dw_n, o.dw_k, o.dw_len};
      }
      std::stable_sort(wl.begin() + g0, wl.begin() + g1, [](const DnaWinDev &a, const DnaWinDev &b) { return a.n < b.n; });
      cnt[gi] = fsw_fuse(wl.data(), g0, g1, p.max_length);
      for (int s = g0; s < g0 + cnt[gi]; s++)
        fsw_summarize(orfs, g0, g1, wl[(size_t)s], n_seq, dna->h_off.data(), p, flogsum_host, &out_slot[(size_t)s], &desc_slot[(size_t)s]);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nparts; t++) th.emplace_back(build, t);
  build(0);
  for (std::thread &t : th) t.join();

  // ---- the windows in order, their pool offsets, the view's off[] / len[]
  int nw = 0;
  for (size_t gi = 0; gi < ngroups; gi++)
    for (int s = gstart[gi]; s < gstart[gi] + cnt[gi]; s++, nw++) {
      out[nw] = out_slot[(size_t)s]; desc[nw] = desc_slot[(size_t)s];
      grp[2 * nw] = gstart[gi]; grp[2 * nw + 1] = gstart[gi + 1];
      const int len = desc[nw].len;
      desc[nw].dst_off = B->pool_bytes; voff[nw] = B->pool_bytes; vlen[nw] = len;
      B->pool_bytes += fsw_pool_pitch(len); B->total += len; B->maxlen = std::max(B->maxlen, len);
    }
  B->n_orfs = n; B->nw = nw;
  char *rs = b_res.as<char>();
  for (const auto &[off, bytes] : {std::pair<size_t, size_t>{R.voff, (size_t)nw * 8}, {R.vlen, (size_t)nw * 4}, {R.desc, (size_t)nw * sizeof(FsWinDev)}})
    BATH_HIP_TRY(ctx, hipMemcpyAsync(rs + off, h + off, bytes, hipMemcpyHostToDevice, ctx->stream));
  res_bind(R, h, rs, B);
  B->host_built = true;
  return BATH_OK;
}

bool fs_orf_in_window(const FsOrfDev &o, const bath_fs_window &r, int n_seq) {
  return fsw_orf_inside(o, r.strand, n_seq, fsw_span(r.strand, n_seq, r.n, r.length));
}

int fs_decide(bath_hip_ctx *ctx, const bath_hip_fsprofile *om_fs3, const bath_pipeline_params *prm, const FsWinBuild &B, const float *d_bias,
              const float *d_fsc, const float *h_fsc, bath_fs_window *h_out) {
  if (B.nw == 0) return BATH_OK;
  const float *ev3 = om_fs3->evparam;
  const double tau3 = (double)ev3[BATH_FTAUFS3], lambda = (double)ev3[BATH_FLAMBDA];
  if (B.host_built) {
    // the host build decides on the host: libm's exp() and log(), whose last bit the kernel's need not share
    if (ctx->stage[Pinned::kFsDecideDown].reserve((size_t)B.nw * 6 * sizeof(float) + 64) != hipSuccess) { ctx->set_error("cannot allocate page-locked staging memory"); return BATH_EFAIL; }
    const float *h_bias = static_cast<const float *>(ctx->stage[Pinned::kFsDecideDown].p);
    BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsDecideDown].p, d_bias, (size_t)B.nw * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < B.nw; i++) {
      h_out[i] = B.h_out[i];
      fsw_decide(h_out[i], &h_bias[(size_t)i * 6], h_fsc[i], fsw_len_terms(h_out[i].length / 3), flogsum_host, prm->do_biasfilter, prm->std_pipe, prm->F3, tau3, lambda);
    }
    return BATH_OK;
  }
  // the length terms by L3, up to the longest window of the block: kept by the context, extended (and uploaded again) when a block needs more
  DevBuf &b_len = ctx->scratch[Scratch::kFsWindowLenTerms];
  const size_t need = (size_t)std::max(B.maxlen, 0) / 3 + 1;
  if (ctx->fsw_len_terms.size() < need * 2 || !b_len.p) {
    const size_t n = std::max(need, ctx->fsw_len_terms.size());       // (two floats per L3: grows to twice what is asked for)
    ctx->fsw_len_terms.resize(2 * n);
    for (size_t L3 = 0; L3 < n; L3++) { const FswLen t = fsw_len_terms((int)L3); ctx->fsw_len_terms[2 * L3] = t.null_frame; ctx->fsw_len_terms[2 * L3 + 1] = t.filt; }
    BATH_HIP_TRY(ctx, b_len.reserve(2 * n * sizeof(float)));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(b_len.p, ctx->fsw_len_terms.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  hipLaunchKernelGGL(fsw_decide_kernel, dim3((unsigned)((B.nw + 255) / 256)), dim3(256), 0, ctx->stream, B.d_out, B.nw, d_bias, d_fsc, om_fs3->d_logsum,
                     b_len.as<FswLen>(), prm->do_biasfilter, prm->std_pipe, prm->F3, tau3, lambda);
  BATH_HIP_TRY(ctx, hipGetLastError());
  if (ctx->stage[Pinned::kFsDecideDown].reserve((size_t)B.nw * sizeof(bath_fs_window) + 64) != hipSuccess) { ctx->set_error("cannot allocate page-locked staging memory"); return BATH_EFAIL; }
  BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsDecideDown].p, B.d_out, (size_t)B.nw * sizeof(bath_fs_window), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(h_out, ctx->stage[Pinned::kFsDecideDown].p, (size_t)B.nw * sizeof(bath_fs_window));
  return BATH_OK;
}

void fs_order_survivors(std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins) {
  std::sort(sel->begin(), sel->end(), [](const FsCandRec &a, const FsCandRec &b) { return a.cand < b.cand; });
  // an ORF's windows in the order the Viterbi filter emits them (by start); windows of one start, which it never emits, by k
  std::stable_sort(wins->begin(), wins->end(), [](const WindowRec &a, const WindowRec &b) { return a.cand != b.cand ? a.cand < b.cand : (a.n != b.n ? a.n < b.n : a.k < b.k); });
}

void fs_merge_survivors(const FsLaneSurv *lanes, int nlanes, const std::vector<std::vector<FsCandRec>> &lsel, const std::vector<std::vector<WindowRec>> &lwin,
                        std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins) {
  sel->clear(); wins->clear();
  for (size_t k = 0; k < (size_t)nlanes; k++) {
    const FsLaneSurv &ls = lanes[k];
    for (FsCandRec q : lsel[k]) { q.cand += ls.cand_base; q.window += ls.first_window; q.aa_off += ls.dpool; if (nlanes > 1) q.fxoff = -1; sel->push_back(q); }
    for (WindowRec w : lwin[k]) { w.cand += ls.cand_base; wins->push_back(w); }
  }
}

}  // namespace bath

// ---- self-test hooks (include/bath_hip.h): the builder and the decision on lists a test makes up
static_assert(sizeof(bath_fs_cand) == sizeof(bath::FsCandRec) && offsetof(bath_fs_cand, fxoff) == offsetof(bath::FsCandRec, fxoff) && offsetof(bath_fs_cand, cand) == offsetof(bath::FsCandRec, cand), "bath_fs_cand is FsCandRec");
static_assert(sizeof(bath_fs_hitwin) == sizeof(bath::WindowRec) && offsetof(bath_fs_hitwin, score) == offsetof(bath::WindowRec, score), "bath_fs_hitwin is WindowRec");
static_assert(sizeof(bath_fs_orf) == sizeof(bath::FsOrfDev) && offsetof(bath_fs_orf, g1) == offsetof(bath::FsOrfDev, g1) && offsetof(bath_fs_orf, dw_n) == offsetof(bath::FsOrfDev, dw_n), "bath_fs_orf is FsOrfDev");
static_assert(sizeof(bath_fs_windesc) == sizeof(bath::FsWinDev) && offsetof(bath_fs_windesc, kmax) == offsetof(bath::FsWinDev, kmax), "bath_fs_windesc is FsWinDev");

extern "C" int bath_selftest_fs_windows(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna, double F3, int std_pipe,
                                        int driver, const bath_fs_lane *lanes, int nlanes, int nc_total, bath_fs_winbuild *hdr, bath_fs_orf *orfs,
                                        bath_fs_window *windows, int32_t *grp, int64_t *voff, int32_t *vlen, bath_fs_windesc *desc) {
  using namespace bath;
  if (!ctx || !om || !om_fs3 || !dna || !hdr || nlanes < 0 || (nlanes > 0 && !lanes) || (driver != 0 && driver != 1)) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  *hdr = bath_fs_winbuild{};
  bath_pipeline_params prm;
  bath_pipeline_params_default(&prm, 1);
  prm.F3 = F3; prm.std_pipe = std_pipe;
  size_t n = 0;
  for (int k = 0; k < nlanes; k++) {
    if (lanes[k].n_c < 0 || lanes[k].n_w < 0 || (lanes[k].n_c > 0 && !lanes[k].cands) || (lanes[k].n_w > 0 && !lanes[k].wins)) return BATH_EINVAL;
    n += (size_t)lanes[k].n_c;
  }
  if (n > 0 && (!orfs || !windows || !grp || !voff || !vlen || !desc)) return BATH_EINVAL;
  FsWinBuild B;
  int st;
  char *d_lists = nullptr;
  if (driver == 0) {
    std::vector<FsLaneSurv> dl((size_t)nlanes);
    std::vector<size_t> o_c((size_t)nlanes), o_w((size_t)nlanes);
    size_t bytes = 256;
    for (int k = 0; k < nlanes; k++) {
      o_c[(size_t)k] = bytes; bytes += ((size_t)lanes[k].n_c * sizeof(FsCandRec) + 255) / 256 * 256;
      o_w[(size_t)k] = bytes; bytes += ((size_t)lanes[k].n_w * sizeof(WindowRec) + 255) / 256 * 256;
    }
    BATH_HIP_TRY(ctx, hipMalloc((void **)&d_lists, bytes));
    hipError_t e = hipSuccess;
    for (int k = 0; k < nlanes && e == hipSuccess; k++) {
      FsLaneSurv &ls = dl[(size_t)k];
      ls.d_c = reinterpret_cast<const FsCandRec *>(d_lists + o_c[(size_t)k]); ls.d_w = reinterpret_cast<const WindowRec *>(d_lists + o_w[(size_t)k]);
      ls.n_c = lanes[k].n_c; ls.n_w = lanes[k].n_w; ls.cand_base = lanes[k].cand_base; ls.first_window = lanes[k].first_window; ls.dpool = lanes[k].dpool;
      if (ls.n_c) e = hipMemcpy(d_lists + o_c[(size_t)k], lanes[k].cands, (size_t)ls.n_c * sizeof(FsCandRec), hipMemcpyHostToDevice);
      if (ls.n_w && e == hipSuccess) e = hipMemcpy(d_lists + o_w[(size_t)k], lanes[k].wins, (size_t)ls.n_w * sizeof(WindowRec), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { (void)hipFree(d_lists); ctx->set_error(std::string("bath_selftest_fs_windows: ") + hipGetErrorString(e)); return BATH_EFAIL; }
    st = fs_build_windows_device(ctx, om, om_fs3, dna, &prm, dl.data(), nlanes, nc_total, &B);
  } else {
    std::vector<FsLaneSurv> hl((size_t)nlanes);
    std::vector<std::vector<FsCandRec>> lsel((size_t)nlanes);
    std::vector<std::vector<WindowRec>> lwin((size_t)nlanes);
    for (int k = 0; k < nlanes; k++) {
      FsLaneSurv &ls = hl[(size_t)k];
      ls = FsLaneSurv{};
      ls.n_c = lanes[k].n_c; ls.n_w = lanes[k].n_w; ls.cand_base = lanes[k].cand_base; ls.first_window = lanes[k].first_window; ls.dpool = lanes[k].dpool;
      lsel[(size_t)k].resize((size_t)ls.n_c); lwin[(size_t)k].resize((size_t)ls.n_w);
      if (ls.n_c) std::memcpy(lsel[(size_t)k].data(), lanes[k].cands, (size_t)ls.n_c * sizeof(FsCandRec));
      if (ls.n_w) std::memcpy(lwin[(size_t)k].data(), lanes[k].wins, (size_t)ls.n_w * sizeof(WindowRec));
      fs_order_survivors(&lsel[(size_t)k], &lwin[(size_t)k]);
    }
    std::vector<FsCandRec> sel;
    std::vector<WindowRec> wins;
    fs_merge_survivors(hl.data(), nlanes, lsel, lwin, &sel, &wins);
    st = fs_build_windows_host(ctx, om, dna, &prm, sel.data(), (int)sel.size(), wins.data(), (int)wins.size(), &B);
  }
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (st == BATH_OK && e == hipSuccess && B.nw > 0) {
    hdr->n_orfs = B.n_orfs; hdr->nw = B.nw; hdr->maxlen = B.maxlen; hdr->pool_bytes = B.pool_bytes; hdr->total = B.total;
    std::memcpy(orfs, B.h_orfs, (size_t)B.n_orfs * sizeof(FsOrfDev));
    std::memcpy(grp, B.h_grp, (size_t)B.nw * 8);
    std::memcpy(voff, B.h_voff, (size_t)B.nw * 8);
    std::memcpy(vlen, B.h_vlen, (size_t)B.nw * 4);
    if (B.host_built) std::memcpy(windows, B.h_out, (size_t)B.nw * sizeof(bath_fs_window));
    else e = hipMemcpy(windows, B.d_out, (size_t)B.nw * sizeof(bath_fs_window), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(desc, B.d_desc, (size_t)B.nw * sizeof(FsWinDev), hipMemcpyDeviceToHost);
  }
  if (d_lists) (void)hipFree(d_lists);
  if ((st == BATH_OK || st == BATH_ENORESULT) && e != hipSuccess) { ctx->set_error(std::string("bath_selftest_fs_windows: ") + hipGetErrorString(e)); st = BATH_EFAIL; }
  return st;
}

extern "C" int bath_selftest_fs_decide(bath_hip_ctx *ctx, const bath_hip_fsprofile *om_fs3, bath_fs_window *records, int nw, const float *bias, const float *fsc,
                                       int do_biasfilter, int std_pipe, double F3, int driver) {
  using namespace bath;
  if (!ctx || !om_fs3 || nw < 0 || (nw > 0 && (!records || !bias || !fsc)) || (driver != 0 && driver != 1)) return BATH_EINVAL;
  if (nw == 0) return BATH_OK;
  int maxlen = 0;
  for (int i = 0; i < nw; i++) { if (records[i].length < 0) return BATH_EINVAL; maxlen = std::max(maxlen, records[i].length); }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  bath_pipeline_params prm;
  bath_pipeline_params_default(&prm, 1);
  prm.F3 = F3; prm.std_pipe = std_pipe; prm.do_biasfilter = do_biasfilter;
  const size_t o_rec = 0, o_bias = al256((size_t)nw * sizeof(bath_fs_window)), o_fsc = o_bias + al256((size_t)nw * 6 * sizeof(float)), bytes = o_fsc + al256((size_t)nw * sizeof(float));
  char *d = nullptr;
  BATH_HIP_TRY(ctx, hipMalloc((void **)&d, bytes));
  hipError_t e = hipMemcpy(d + o_rec, records, (size_t)nw * sizeof(bath_fs_window), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_bias, bias, (size_t)nw * 6 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_fsc, fsc, (size_t)nw * sizeof(float), hipMemcpyHostToDevice);
  int st = BATH_EFAIL;
  if (e == hipSuccess) {
    std::vector<bath_fs_window> in(records, records + nw), out((size_t)nw);
    FsWinBuild B;
    B.nw = nw; B.maxlen = maxlen; B.host_built = driver == 1; B.h_out = in.data(); B.d_out = reinterpret_cast<bath_fs_window *>(d + o_rec);
    st = fs_decide(ctx, om_fs3, &prm, B, reinterpret_cast<const float *>(d + o_bias), reinterpret_cast<const float *>(d + o_fsc), fsc, out.data());
    if (st == BATH_OK) std::memcpy(records, out.data(), (size_t)nw * sizeof(bath_fs_window));
    e = hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(d);
  if (e != hipSuccess) { ctx->set_error(std::string("bath_selftest_fs_decide: ") + hipGetErrorString(e)); return BATH_EFAIL; }
  return st;
}
