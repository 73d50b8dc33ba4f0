// bath_pipeline.hip -- the filter cascade of p7_Pipeline_BATH() as a batched GPU pipeline.
//
// Reference control flow (src/p7_pipeline.c:1632-1791), per ORF of a DNA window and strand:
//   MSV (F1) -> bias filter (F1) -> ViterbiFilter_BATH (F2) or SSVFilter_BATH windows
//   -> local-composition re-filter -> ForwardParser (F3, or F4 when fs_pipe)
// with the ORFs produced by easel's six-frame translation (src/bathsearch.c:384-392).
//
// GPU formulation:
//   1. bath_orfs.hip: six-frame translation, ORF finding and a length-sorted ORF work list (lane per stream).
//   2. ssv_orf_kernel: one LANE per ORF (G lanes for long models) runs the SSV recurrence with the whole DP row in
//      registers, two binary16 cells each; lanes of a wave hold ORFs of equal length.  The lane compares its maximum with a
//      per-length threshold table computed on the host with the reference's double-precision P-value maths (so the
//      F1 decision is bit-identical) and appends the ~2% survivors to a candidate list.
//   3. survivors flow through decision kernels (lane per candidate) and DP kernels (lane or wave per candidate)
//      with device-side work lists: no host round trip until the final copy-out.  Their residues are read in place
//      from the amino-acid streams written by step 1.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"
#include "host_model.hpp"

using namespace bath;

namespace bath {

static const double kLog2 = 0.69314718055994529;

// ---------------------------------------------------------------------------------------------
// candidate storage (structure of arrays, indexed by candidate id)
// ---------------------------------------------------------------------------------------------
enum { FLAG_VIT_RUN = 1, FLAG_HAS_WIN = 2 };

struct Counters {                     // device-side counters, one struct per pipeline call
  int cand_count, todo_msv, todo_vit, todo_ssvb, todo_vit2, todo_fwd, win_count, overflow;
  int todo_lb;                                              // candidates that need the local-composition bias filter
  int fwd_next;                                             // fwd_group_kernel: jobs handed out beyond every wave's first (zero when the kernel starts, as all of these)
  unsigned long long n_orfs, orf_res;                       // ORFs >= minlen, their total aa
  unsigned long long n_past_msv, n_past_bias, n_past_vit, n_past_fwd;
  unsigned long long pos_past_msv, pos_past_bias, pos_past_vit, pos_past_fwd;
  unsigned long long res_vit, res_fwd;                      // residues entering Viterbi / Forward
  unsigned long long res_seen;                              // residues of ORFs lying inside a window's context: scored by SSV but not the reference's (p7_pipeline.c:1635)
};

struct Params {
  double F1, F2, F3, F4;
  int do_bias, fs_pipe, minlen;
  float evparam[BATH_NEVPARAM];
};

// ---------------------------------------------------------------------------------------------
// 1. SSV over the length-sorted ORF list, lane per ORF (persistent waves striding over the list)
// ---------------------------------------------------------------------------------------------
// (tiles of at most 76 registers: four 256-thread blocks per CU, 128 VGPRs each; a group of G lanes with such tiles has rows of at
// most 4 * 76 * G bytes, so four copies of its cost table always fit a CU's LDS -- a 1024-thread variant existed and could never be chosen)
template <int NR, int G>
__global__ __launch_bounds__(256, NR <= 76 ? 4 : 1) void ssv_orf_kernel(const uint8_t *__restrict__ aa, const OrfRec *__restrict__ orfs, const int *__restrict__ n_orfs_dev,
                                                      SeqView dna, const int16_t *__restrict__ cost_tab, int row_bytes,
                                                      const int16_t *__restrict__ emit_thresh, int thresh_max,
                                                      Cand cand, int cand_cap, Counters *__restrict__ ctr) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  {
    const int n32 = kSsvRows * row_bytes / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(cost_tab);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    for (int i = threadIdx.x; i < n32; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  constexpr int TPW = 64 / G;                                   // ORFs per wave
  const int64_t n_orfs = *n_orfs_dev;
  const int lane = threadIdx.x & 63;
  const int grank = SsvGroups<G>::rank(lane);
  const char *tile = lds + grank * (4 * NR);
  const unsigned tile_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const char *)tile;   // LDS byte address
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const s16x2 fl = {0, 0};                                      // the begin score
  for (int64_t tb = wave0 * TPW; tb < n_orfs; tb += nwaves * TPW) {
    const int64_t t = tb + SsvGroups<G>::slot(lane);
    const bool live = t < n_orfs;
    OrfRec rec{0, 0, 0};
    if (live) rec = orfs[t];
    const int L = rec.len_sf & 0x0fffffff;
    const uint8_t *s = aa + rec.aa_off;
    const int Lw = wave_max_i32(L);
    s16x2 reg[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) reg[r] = fl;
    s16x2 xE = fl, xE2 = fl;
    // residues 8 at a time, the next 8 in flight: an ORF's 64-byte sectors are touched by half as many loads as with a dword
    // per 4 rows (HBM traffic of the launch -32%, kernel -4%; the loop also stops at the wave's longest ORF instead of the next
    // multiple of 4 rows).  Staging the residues through LDS instead (three global_load_lds_dwordx4 per wave and 32 rows, double
    // buffered) was measured at -2% time and -20% traffic and not kept: most of the excess traffic is 128-byte lines shared by
    // ORFs of different lengths, which no read pattern of this kernel can merge.
    uint64_t qnext = (0 < L) ? *reinterpret_cast<const uint64_t *>(s) : 0x1d1d1d1d1d1d1d1dull;
    for (int i0 = 0; i0 < Lw; i0 += 8) {
      const uint64_t q = qnext;
      qnext = (i0 + 8 < L) ? *reinterpret_cast<const uint64_t *>(s + i0 + 8) : 0x1d1d1d1d1d1d1d1dull;
      const int nrow = min(8, Lw - i0);                              // wave-uniform
      // the row's overhead is kept to full-rate 32-bit ops: a bit-field extract on the dword holding the residue (no 64-bit
      // shift), a 24-bit multiply for the row offset (v_mul_lo_u32 is quarter rate); bytes inside an ORF are residue codes < 29
      for (int h = 0; h < 2; h++) {
        const uint32_t qh = h ? (uint32_t)(q >> 32) : (uint32_t)q;
        const int nh = min(4, nrow - 4 * h);                         // wave-uniform
        for (int j = 0; j < nh; j++) {
          int x = (int)__builtin_amdgcn_ubfe(qh, 8 * j, 8);
          x = (i0 + 4 * h + j < L) ? x : kRowReset;
          const unsigned carry = ssv_carry<NR, G>(reg, grank);
          ssv_row_pipe<NR, 3>(reg, xE, xE2, tile_addr + __umul24((unsigned)x, (unsigned)row_bytes), carry);
        }
      }
    }
    xE = ssv_max3(xE, xE2, xE2);
    const int v = ssv_group_max<G>(xE);
    if (dna.context) {                  // windows with context only: ORFs the previous window already searched do not count as MSV work
      unsigned long long r = 0;
      if (live && grank == 0) {
        const int sf = (int)((unsigned)rec.len_sf >> 28);
        const int64_t w = rec.w;
        const int startj = (int32_t)(rec.aa_off - (2 * dna.off[w] + 96 * w + (int64_t)sf * orf_stream_pitch(dna.len[w])));
        const int C = dna.context[w], start_s = sf % 3 + 3 * startj + 1;
        if (sf < 3 ? (start_s + 3 * L - 1 < C) : (dna.len[w] - start_s + 1 < C)) r = (unsigned long long)L;
      }
      if (__ballot(r != 0)) { for (int d = 32; d >= 1; d >>= 1) r += __shfl_xor(r, d, 64); if (lane == 0) atomicAdd(&ctr->res_seen, r); }
    }
    if (live && grank == 0 && v >= (int)emit_thresh[min(L, thresh_max)]) {
      const int sf = (int)((unsigned)rec.len_sf >> 28);
      const int64_t w = rec.w;
      const int64_t stream = 2 * dna.off[w] + 96 * w + (int64_t)sf * orf_stream_pitch(dna.len[w]);
      const int startj = (int32_t)(rec.aa_off - stream);
      bool seen = false;                // an ORF that lies inside the previous window's share of this one (p7_pipeline.c:1635-1637)
      if (dna.context) {
        const int C = dna.context[w], start_s = sf % 3 + 3 * startj + 1;
        seen = sf < 3 ? (start_s + 3 * L - 1 < C) : (dna.len[w] - start_s + 1 < C);
      }
      const int slot = seen ? cand_cap + 1 : atomicAdd(&ctr->cand_count, 1);
      if (seen) {
      } else if (slot < cand_cap) {
        cand.window[slot] = w; cand.sf[slot] = sf; cand.startj[slot] = startj; cand.len[slot] = L;
        cand.v[slot] = (int16_t)min(v, 32767); cand.off[slot] = rec.aa_off;
      } else atomicOr(&ctr->overflow, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// decision kernels (lane per candidate)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double d_gumbel_surv(double x, double mu, double lambda) {
  const double ey = -exp(-lambda * (x - mu));
  if (fabs(ey) < 5e-9) return -ey;
  return 1.0 - exp(ey);
}
__device__ __forceinline__ double d_exp_surv(double x, double mu, double lambda) { return (x < mu) ? 1.0 : exp(-lambda * (x - mu)); }

// a candidate's first visit: the SSV maximum classified (ssvfilter.c:876-925), every later stage's field at its start value
__device__ __forceinline__ int cand_classify(const Cand &cand, int c, int tjb, const MsvConsts &mc) {
  float sc = 0.f;
  const int st = ssv_classify(cand.v[c], tjb, mc, &sc);
  cand.usc[c] = sc; cand.msv_status[c] = st; cand.stage[c] = 0; cand.flags[c] = 0;
  cand.vfsc[c] = -INFINITY; cand.fwdsc[c] = -INFINITY; cand.vit_status[c] = 0; cand.filtersc[c] = 0.f; cand.P[c] = 1.0;
  cand.kminmax[2 * c] = 1 << 30; cand.kminmax[2 * c + 1] = 0;
  return st;
}

// ---- block-level counting and appending
// The decision kernels add to members of the one Counters struct and append ids to work lists whose lengths live there too: a
// few hot addresses, where returning global atomics serialise (~3 ns each on MI355X; the compiler already issues one per wave,
// not per lane).  A block therefore tallies in LDS -- NS 64-bit sums, and NL lists whose ids wait in LDS at a rank taken from an
// LDS atomic -- and touches each global address once: one atomicAdd per non-zero sum, and per non-empty list one atomicAdd that
// reserves the block's range, into which the lanes then copy the waiting ids.  A kernel that strides over its candidates
// tallies over all of its iterations; the lists alone are written out early when the next iteration might not fit (CAP ids per
// list, CAP >= 2 * blockDim.x for such a kernel, >= blockDim.x for one without a loop).
// Every counter keeps its value.  The ORDER of the ids inside a list differs from the per-wave appends this replaces -- which
// was a race between waves already, and nothing reads a list for its order: the Viterbi stage's length sort scatters the ids
// again, hit windows are appended by atomics of their own, and the records are sorted by key.
// tally_reset, tally_lists_full, tally_write_lists and tally_finish hold barriers: every lane of the block calls them, together.
template <int NL, int NS, int CAP>
struct BlockTally {
  int n[NL > 0 ? NL : 1], base[NL > 0 ? NL : 1];
  unsigned long long sum[NS > 0 ? NS : 1];
  int32_t ids[NL > 0 ? NL : 1][NL > 0 ? CAP : 1];
};
template <int NL, int NS>
struct TallyOut {                      // where a block's tally goes: the lists with their lengths, the 64-bit counters
  int32_t *list[NL > 0 ? NL : 1]; int *count[NL > 0 ? NL : 1];
  unsigned long long *sum[NS > 0 ? NS : 1];
};
template <int NL, int NS, int CAP>
__device__ __forceinline__ void tally_reset(BlockTally<NL, NS, CAP> &t) {
  if ((int)threadIdx.x < NL) t.n[threadIdx.x] = 0;
  if ((int)threadIdx.x < NS) t.sum[threadIdx.x] = 0ull;
  __syncthreads();
}
template <int NL, int NS, int CAP>
__device__ __forceinline__ void tally_add(BlockTally<NL, NS, CAP> &t, int k, unsigned long long v) { atomicAdd(&t.sum[k], v); }
template <int NL, int NS, int CAP>
__device__ __forceinline__ void tally_push(BlockTally<NL, NS, CAP> &t, int l, int32_t id) { t.ids[l][atomicAdd(&t.n[l], 1)] = id; }
// can every lane still push one id to every list?  (the same answer in all lanes)
template <int NL, int NS, int CAP>
__device__ __forceinline__ bool tally_lists_full(BlockTally<NL, NS, CAP> &t) {
  bool full = false;
  __syncthreads();
#pragma unroll
  for (int l = 0; l < NL; l++) full |= t.n[l] > CAP - (int)blockDim.x;
  __syncthreads();
  return full;
}
template <int NL, int NS, int CAP>
__device__ __forceinline__ void tally_write_lists(BlockTally<NL, NS, CAP> &t, const TallyOut<NL, NS> &o) {
  if (NL == 0) return;
  __syncthreads();
#pragma unroll
  for (int l = 0; l < NL; l++) if ((int)threadIdx.x == l && t.n[l] > 0) t.base[l] = atomicAdd(o.count[l], t.n[l]);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const int n = t.n[l], b = t.base[l];
    for (int i = threadIdx.x; i < n; i += blockDim.x) o.list[l][b + i] = t.ids[l][i];
  }
  __syncthreads();
  if ((int)threadIdx.x < NL) t.n[threadIdx.x] = 0;
  __syncthreads();
}
template <int NL, int NS, int CAP>
__device__ __forceinline__ void tally_finish(BlockTally<NL, NS, CAP> &t, const TallyOut<NL, NS> &o) {
  tally_write_lists(t, o);             // (its first barrier also orders the lanes' tally_add before the reads below)
  if (NL == 0) __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; k++) if ((int)threadIdx.x == k && t.sum[k] != 0ull) atomicAdd(o.sum[k], t.sum[k]);
}

// classify the SSV maxima; undecided targets go to the full-MSV list
__global__ __launch_bounds__(256) void classify_kernel(Cand cand, int cand_cap, Counters *__restrict__ ctr, const uint8_t *__restrict__ tjb_tab, MsvConsts mc,
                                                       int32_t *__restrict__ todo_msv) {
  __shared__ BlockTally<1, 0, 512> tally;
  tally_reset(tally);
  const TallyOut<1, 0> out{{todo_msv}, {&ctr->todo_msv}, {nullptr}};
  const int ncand = min(ctr->cand_count, cand_cap);
  for (int c0 = blockIdx.x * blockDim.x; c0 < ncand; c0 += gridDim.x * blockDim.x) {
    if (tally_lists_full(tally)) tally_write_lists(tally, out);
    const int c = c0 + threadIdx.x;
    if (c < ncand && cand_classify(cand, c, tjb_tab[cand.len[c]], mc) == BATH_ENORESULT) tally_push(tally, 0, c);
  }
  tally_finish(tally, out);
}

// MSV P-value (F1), bias filter (F1), then route to Viterbi (P > F2) or SSV windows (P <= F2): p7_pipeline.c:1649-1677
struct F1Tables { const float *eo, *nullsc, *p1, *lt1, *lt2; };      // the bias filter's emission odds [Kp][2]; by target length: null score, p1, the length corrections
// what cand_f1_bias tallies per block: the lists todo_vit and todo_ssvb, five counters
enum { F1_TODO_VIT = 0, F1_TODO_SSVB = 1, F1_NL = 2 };
enum { F1_N_MSV = 0, F1_POS_MSV, F1_N_BIAS, F1_POS_BIAS, F1_RES_VIT, F1_NS };
__device__ __forceinline__ TallyOut<F1_NL, F1_NS> f1_tally_out(Counters *__restrict__ ctr, int32_t *__restrict__ todo_vit, int32_t *__restrict__ todo_ssvb) {
  return TallyOut<F1_NL, F1_NS>{{todo_vit, todo_ssvb}, {&ctr->todo_vit, &ctr->todo_ssvb},
                                {&ctr->n_past_msv, &ctr->pos_past_msv, &ctr->n_past_bias, &ctr->pos_past_bias, &ctr->res_vit}};
}
// (a lane may leave this function early: it holds no barrier, and its callers reach tally_finish with every lane of the block)
template <int CAP>
__device__ __forceinline__ void cand_f1_bias(const Cand &cand, int c, BlockTally<F1_NL, F1_NS, CAP> &tally, const Params &p, const uint8_t *__restrict__ pool, int M,
                                             const float *s_eo /* the emission odds in LDS */, const F1Tables &t) {
  const int L = cand.len[c];
  const float usc = cand.usc[c];
  const float nullsc = t.nullsc[L];
  cand.nullsc[c] = nullsc;
  float seqsc = (float)((double)(usc - nullsc) / kLog2);
  double P = d_gumbel_surv(seqsc, p.evparam[0], p.evparam[1]);
  cand.P[c] = P;
  if (P > p.F1) return;
  tally_add(tally, F1_N_MSV, 1ull); tally_add(tally, F1_POS_MSV, (unsigned long long)L * 3ull);
  cand.stage[c] = 1;
  float filtersc = nullsc;
  if (p.do_bias) {
    filtersc = bias_forward(pool + cand.off[c], L, M, s_eo, t.p1[L]);
    filtersc = (filtersc + t.lt1[L]) + t.lt2[L];
    seqsc = (float)((double)(usc - filtersc) / kLog2);
    P = d_gumbel_surv(seqsc, p.evparam[0], p.evparam[1]);
    cand.P[c] = P; cand.filtersc[c] = filtersc;
    if (P > p.F1) return;
  }
  cand.filtersc[c] = filtersc;
  tally_add(tally, F1_N_BIAS, 1ull); tally_add(tally, F1_POS_BIAS, (unsigned long long)L * 3ull);
  cand.stage[c] = 2;
  if (P > p.F2) { cand.flags[c] |= FLAG_VIT_RUN; tally_push(tally, F1_TODO_VIT, c); tally_add(tally, F1_RES_VIT, (unsigned long long)L); }
  else tally_push(tally, F1_TODO_SSVB, c);
}

__global__ __launch_bounds__(256) void f1_bias_kernel(Cand cand, int cand_cap, Counters *__restrict__ ctr, Params p, const uint8_t *__restrict__ pool, int M, F1Tables t,
                                                      int32_t *__restrict__ todo_vit, int32_t *__restrict__ todo_ssvb) {
  __shared__ float s_eo[kKp * 2];                          // the filter HMM's emission odds: read once per residue, from LDS
  __shared__ BlockTally<F1_NL, F1_NS, 512> tally;
  for (int i = threadIdx.x; i < kKp * 2; i += blockDim.x) s_eo[i] = t.eo[i];
  tally_reset(tally);
  const TallyOut<F1_NL, F1_NS> out = f1_tally_out(ctr, todo_vit, todo_ssvb);
  const int ncand = min(ctr->cand_count, cand_cap);
  for (int c0 = blockIdx.x * blockDim.x; c0 < ncand; c0 += gridDim.x * blockDim.x) {
    if (tally_lists_full(tally)) tally_write_lists(tally, out);
    const int c = c0 + threadIdx.x;
    if (c < ncand) cand_f1_bias(cand, c, tally, p, pool, M, s_eo, t);
  }
  tally_finish(tally, out);
}

// The MSV stage of a large block in one kernel, a lane per candidate: what classify_kernel, msv_lane_kernel and f1_bias_kernel do
// one after the other, in that order and with their arithmetic (cand_classify, msv_lane_rows, cand_f1_bias: the same functions).
// The candidates are taken in the order ssv_orf_kernel appended them.  That kernel strides a length-sorted ORF list, so the 64
// lanes of a wave here hold ORFs of nearly one length already: both the MSV rows, which run to the wave's longest ORF, and the
// bias filter's recurrence, a dependent chain of two divisions and an fp64 logarithm per residue, end together (a counting sort
// in front of the kernel was measured: it saves the kernel 0.01 ms and costs 0.04).  A candidate's residues are read
// for the rows and again, from cache, for the bias filter.
template <int NR>
__global__ __launch_bounds__(256, 4) void msv_stage_kernel(Cand cand, int cand_cap, Counters *__restrict__ ctr,
                                                           const int16_t *__restrict__ cost_tab /* the MSV increment table */, int row_bytes,
                                                           const uint8_t *__restrict__ tjb_tab, MsvConsts mc, Params p, const uint8_t *__restrict__ pool, int M,
                                                           F1Tables t, int32_t *__restrict__ todo_vit, int32_t *__restrict__ todo_ssvb) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ float s_eo[kKp * 2];
  __shared__ BlockTally<F1_NL, F1_NS, 256> tally;          // a lane has one candidate: at most 256 ids per list
  // Not persistent: the grid covers the candidate buffer, a wave takes the 64 candidates at its place in the list and a block beyond
  // the list leaves at once.  (With a loop over several waves of candidates per wave, the fp64 logarithm's constants and the other
  // invariants of the bias loop are hoisted above the row loop, where the tile leaves no register for them: scratch spills.)
  const int ncand = min(ctr->cand_count, cand_cap);
  if ((int64_t)blockIdx.x * blockDim.x >= ncand) return;
  {
    const int n32 = kSsvRows * row_bytes / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(cost_tab);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    for (int i = threadIdx.x; i < n32; i += blockDim.x) dst[i] = src[i];
    for (int i = threadIdx.x; i < kKp * 2; i += blockDim.x) s_eo[i] = t.eo[i];
  }
  tally_reset(tally);
  const int64_t job = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = job < ncand;
  const int c = live ? (int)job : 0;
  const int L = live ? cand.len[c] : 0;
  const int tjb = tjb_tab[L];
  const bool rescore = live && cand_classify(cand, c, tjb, mc) == BATH_ENORESULT;   // every candidate of the cascade, in practice (bath_msv_lane.hip)
  const int Lr = rescore ? L : 0;
  const uint8_t *s = pool + (rescore ? cand.off[c] : 0);
  bool overflow = false;
  const int xJ = msv_lane_rows<NR>(lds, row_bytes, s, Lr, wave_max_i32(Lr), (uint8_t)((int8_t)tjb + (int8_t)mc.tbm), mc, &overflow);
  if (rescore) {
    if (overflow) { cand.usc[c] = INFINITY; cand.msv_status[c] = BATH_ERANGE; }
    else { cand.usc[c] = msv_lane_score(xJ, tjb, mc); cand.msv_status[c] = BATH_OK; }
  }
  if (live) cand_f1_bias(cand, c, tally, p, pool, M, s_eo, t);
  tally_finish(tally, f1_tally_out(ctr, todo_vit, todo_ssvb));
}

// p7_SSVFilter_BATH (msvfilter.c:250-427): diagonal windows for strong MSV hits, wave per candidate.
// Lane l owns nodes l*C+1 .. l*C+C (byte arithmetic of the reference kept exactly).  When the row maximum
// reaches the threshold, the reference scans its striped vectors q=0..Q-1, lanes 0..15 and keeps the strictly
// greatest byte (msvfilter.c:358-366): i.e. the first maximal cell in that order, found here by a wave min
// over the striped rank.
template <int C>
__global__ __launch_bounds__(256) void ssv_bath_kernel(Cand cand, const Counters *__restrict__ ctr, const int32_t *__restrict__ todo,
                                                       const uint8_t *__restrict__ pool, int M, const uint8_t *__restrict__ rb, int rb_stride,
                                                       const uint8_t *__restrict__ ssv_scores, const uint8_t *__restrict__ tjb_tab,
                                                       const float *__restrict__ nullsc_tab, MsvConsts mc, double invP_f1,
                                                       WindowRec *__restrict__ wins, int win_cap, Counters *__restrict__ ctrw) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int ntodo = ctr->todo_ssvb;
  const int Q = max(2, ((M - 1) / 16) + 1);
  for (int64_t job = wid; job < ntodo; job += nw) {
    const int c = todo[job];
    const int L = cand.len[c];
    const uint8_t *s = pool + cand.off[c];
    const int tjb = tjb_tab[L];
    const float nullsc = nullsc_tab[L];
    const int sc_thresh = (uint8_t)(int)ceil((((double)nullsc + ((double)(float)invP_f1 * kLog2) + 3.0) * (double)mc.scale_b) + mc.base + mc.tec + tjb);
    const int tjbm = (uint8_t)((int8_t)tjb + (int8_t)mc.tbm);
    const int xB = satu8(mc.base - tjbm);
    int kmin = 1 << 30, kmax = 0;
    int dp[C];
#pragma unroll
    for (int k = 0; k < C; k++) dp[k] = 0;
    const int ph = threadIdx.x & 63;
    int rbuf = (ph < L) ? (int)s[ph] : 0, rnext = 0;          // residues 64 rows at a time, a lane each, the next 64 in flight (see fwd_wave_kernel)
    for (int i = 1; i <= L; i++) {
      const int j = (i - 1) & 63;
      if (j == 0) { const int q = i - 1 + 64 + ph; rnext = (q < L) ? (int)s[q] : 0; }
      const int x = min(__builtin_amdgcn_readlane(rbuf, j), kKp - 1);
      if (j == 63) rbuf = rnext;
      const uint8_t *row = rb + (size_t)x * rb_stride;
      int prev = wave_shr1_i32(dp[C - 1], 0);
      int xE = 0;
#pragma unroll
      for (int k = 0; k < C; k++) {
        const int node = lane * C + k + 1;
        const int cost = (node <= M) ? (int)row[node] : 255;
        int sv = max(prev, xB);
        sv = satu8(sv + mc.bias);
        sv = satu8(sv - cost);
        prev = dp[k];
        dp[k] = sv;
        xE = max(xE, sv);
      }
      xE = wave_max_i32(xE);
      if (xE >= sc_thresh) {
        int rank = 1 << 30;
#pragma unroll
        for (int k = 0; k < C; k++) {
          const int node = lane * C + k + 1;
          if (node <= M && dp[k] == xE) rank = min(rank, ((node - 1) % Q) * 16 + (node - 1) / Q);
        }
        rank = wave_min_i32(rank);
        int end = (rank / 16) + Q * (rank % 16) + 1;
        int rem_sc = xE;
#pragma unroll
        for (int k = 0; k < C; k++) dp[k] = 0;
        int start = end, target_end = i, target_start = i;
        int sc = rem_sc;
        while (rem_sc > mc.base - tjb - mc.tbm && start >= 1 && target_start >= 1) {
          rem_sc -= mc.bias - (int)ssv_scores[(size_t)start * kKp + min((int)s[target_start - 1], kKp - 1)];
          --start; --target_start;
        }
        start++; target_start++;
        int k = end + 1, n = target_end + 1, max_end = target_end, max_sc = sc, since = 0;
        while (k < M && n <= L) {
          sc += mc.bias - (int)ssv_scores[(size_t)k * kKp + min((int)s[n - 1], kKp - 1)];
          if (sc >= max_sc) { max_sc = sc; max_end = n; since = 0; }
          else { since++; if (since == 5) break; }
          k++; n++;
        }
        end += (max_end - target_end);
        target_end = max_end;
        float ret = ((float)(max_sc - tjb) - (float)mc.base);
        ret /= mc.scale_b;
        ret = (float)((double)ret - 3.0);
        if (lane == 0) {
          const int slot = atomicAdd(&ctrw->win_count, 1);
          if (slot < win_cap) wins[slot] = WindowRec{c, target_start, end, end - start + 1, ret};
        }
        kmin = min(kmin, start); kmax = max(kmax, end);
        i = target_end;
        { const int base = i & ~63; rbuf = (base + ph < L) ? (int)s[base + ph] : 0; rnext = (base + 64 + ph < L) ? (int)s[base + 64 + ph] : 0; }   // the row loop jumped: refill
      }
    }
    if (lane == 0) { cand.kminmax[2 * c] = kmin; cand.kminmax[2 * c + 1] = kmax; }
  }
}

// after Viterbi / SSV windows: F2 test, local-composition re-filter (p7_pipeline.c:1672-1718)
enum { PV_TODO_LB = 0, PV_TODO_FWD = 1, PV_NL = 2 };
enum { PV_N_VIT = 0, PV_POS_VIT, PV_RES_FWD, PV_NS };
__global__ __launch_bounds__(256) void post_vit_kernel(Cand cand, int cand_cap, Counters *__restrict__ ctr, Params p, int32_t *__restrict__ todo_lb, int32_t *__restrict__ todo_fwd) {
  __shared__ BlockTally<PV_NL, PV_NS, 512> tally;
  tally_reset(tally);
  const TallyOut<PV_NL, PV_NS> out{{todo_lb, todo_fwd}, {&ctr->todo_lb, &ctr->todo_fwd}, {&ctr->n_past_vit, &ctr->pos_past_vit, &ctr->res_fwd}};
  const int ncand = min(ctr->cand_count, cand_cap);
  for (int c0 = blockIdx.x * blockDim.x; c0 < ncand; c0 += gridDim.x * blockDim.x) {
    if (tally_lists_full(tally)) tally_write_lists(tally, out);
    const int c = c0 + threadIdx.x;
    bool past = c < ncand && cand.stage[c] == 2;           // decide, then fall through: every lane comes round to the barriers above and below
    if (past && (cand.flags[c] & FLAG_VIT_RUN)) {
      const float seqsc = (float)((double)(cand.vfsc[c] - cand.filtersc[c]) / kLog2);
      const double P = d_gumbel_surv(seqsc, p.evparam[2], p.evparam[3]);
      cand.P[c] = P;
      if (P > p.F2) { cand.kminmax[2 * c] = 1 << 30; cand.kminmax[2 * c + 1] = 0; past = false; }
    }
    if (!past) continue;
    const int L = cand.len[c];
    tally_add(tally, PV_N_VIT, 1ull); tally_add(tally, PV_POS_VIT, (unsigned long long)L * 3ull);
    if (p.do_bias && cand.kminmax[2 * c] <= cand.kminmax[2 * c + 1]) {
      // the local-composition bias filter (p7_pipeline.c:1688-1712) is ~10^3 times the work of everything else here and only the
      // few per cent of candidates that passed Viterbi with a hit window need it: they go to a list and a dense kernel
      // (post_vit_local_kernel); done in place, every wave of this kernel would walk the long path for one or two of its lanes
      cand.flags[c] |= FLAG_HAS_WIN;
      tally_push(tally, PV_TODO_LB, c);
      continue;
    }
    cand.stage[c] = 3;
    tally_push(tally, PV_TODO_FWD, c); tally_add(tally, PV_RES_FWD, (unsigned long long)L);
  }
  tally_finish(tally, out);
}

// The local-composition bias filter in three dense steps.  (1) compo_terms_kernel, once per profile (build_compo_terms, when the
// OProfile is made: its inputs are constants of the model): the 20 x 256 possible terms
// bg_f[x] * exp((base_b - s) / scale_b) of p7_pli_ComputeLocalCompo (s: a byte score).  (2) local_compo_kernel: three candidates per
// wave, lanes 20g..20g+19 each add the terms of one residue over the window's nodes (the 20 sums are independent; each still adds in
// ascending k).  (3) post_vit_local_kernel: a lane per candidate does the serial rest -- normalisation, the 2-state filter HMM
// over the ORF, the decisions -- with its emission odds in LDS.
__host__ __device__ __forceinline__ float compo_term(float bg, int base_b, int sc, float scale_b) {
  const float lo = ((float)base_b - (float)sc) / scale_b;
  return bg * expf(lo);
}
__global__ void compo_terms_kernel(const float *__restrict__ bgf, int base_b, float scale_b, float *__restrict__ terms /* [20][256] */) {
  const int x = blockIdx.x, sc = threadIdx.x;
  terms[x * 256 + sc] = compo_term(bgf[x], base_b, sc, scale_b);
}

__global__ __launch_bounds__(64) void local_compo_kernel(Cand cand, const Counters *__restrict__ ctr, int M, const uint8_t *__restrict__ ssv_scores,
                                                         const float *__restrict__ terms, const int32_t *__restrict__ todo_lb, float *__restrict__ compo_out /* [todo_lb][20] */) {
  const int lane = threadIdx.x, g = lane / 20, x = lane % 20;
  const int ntodo = ctr->todo_lb;
  for (int base = blockIdx.x * 3; base < ntodo; base += gridDim.x * 3) {
    const int job = base + g;
    if (g >= 3 || job >= ntodo) continue;
    const int c = todo_lb[job];
    int k_start = cand.kminmax[2 * c], k_end = cand.kminmax[2 * c + 1];
    const int k_len = k_end - k_start + 1;
    if (k_len < 20) { k_start -= (20 - k_len) / 2; k_end += (20 - k_len) / 2; }
    k_start = max(1, k_start); k_end = min(M, k_end);
    const float *tx = terms + x * 256;
    float acc = 0.0f;
    for (int k = k_start; k <= k_end; k++) acc += tx[ssv_scores[(size_t)k * kKp + x]];
    compo_out[(size_t)job * 20 + x] = acc;
  }
}

__global__ __launch_bounds__(64) void post_vit_local_kernel(Cand cand, Counters *__restrict__ ctr, Params p, const uint8_t *__restrict__ pool, int M,
                                                            const float *__restrict__ bgf, const float *__restrict__ compo_in,
                                                            const float *__restrict__ p1_tab, const float *__restrict__ lt1_tab, const float *__restrict__ lt2_tab,
                                                            const int32_t *__restrict__ todo_lb, int32_t *__restrict__ todo_vit2, int32_t *__restrict__ todo_fwd) {
  __shared__ float s_eo[64][kKp * 2 + 1];
  __shared__ BlockTally<2, 2, 128> tally;                  // lists: todo_vit2, todo_fwd; counters: res_vit, res_fwd
  tally_reset(tally);
  const TallyOut<2, 2> out{{todo_vit2, todo_fwd}, {&ctr->todo_vit2, &ctr->todo_fwd}, {&ctr->res_vit, &ctr->res_fwd}};
  const int ntodo = ctr->todo_lb;
  for (int job0 = blockIdx.x * blockDim.x; job0 < ntodo; job0 += gridDim.x * blockDim.x) {
    if (tally_lists_full(tally)) tally_write_lists(tally, out);
    const int job = job0 + threadIdx.x;
    if (job >= ntodo) continue;
    const int c = todo_lb[job];
    const int L = cand.len[c];
    const float usc = cand.usc[c];
    float filtersc = cand.filtersc[c];
    const float vfsc = (cand.flags[c] & FLAG_VIT_RUN) ? cand.vfsc[c] : -INFINITY;
    float compo[20];
    for (int y = 0; y < 20; y++) compo[y] = compo_in[(size_t)job * 20 + y];
    float *eo = s_eo[threadIdx.x];
    local_compo_finish(compo, bgf, eo);
    float lf = bias_forward(pool + cand.off[c], L, M, eo, p1_tab[L]);
    lf = (lf + lt1_tab[L]) + lt2_tab[L];
    bool to_fwd = true;
    if (lf > filtersc) {
      filtersc = lf;
      cand.filtersc[c] = filtersc;
      if (vfsc == -INFINITY) {
        const float seqsc = (float)((double)(usc - filtersc) / kLog2);
        const double P = d_gumbel_surv(seqsc, p.evparam[0], p.evparam[1]);
        cand.P[c] = P;
        if (P > p.F2) { cand.stage[c] = 5; tally_push(tally, 0, c); tally_add(tally, 0, (unsigned long long)L); to_fwd = false; }
      } else {
        const float seqsc = (float)((double)(vfsc - filtersc) / kLog2);
        const double P = d_gumbel_surv(seqsc, p.evparam[2], p.evparam[3]);
        cand.P[c] = P;
        if (P > p.F2) to_fwd = false;                      // rejected; stays at stage 2 (the reference has already counted it past Vit)
      }
    }
    if (to_fwd) { cand.stage[c] = 3; tally_push(tally, 1, c); tally_add(tally, 1, (unsigned long long)L); }
  }
  tally_finish(tally, out);
}

// plain p7_ViterbiFilter re-run for candidates whose local filter score demanded it (p7_pipeline.c:1703-1708)
__global__ __launch_bounds__(256) void post_vit2_kernel(Cand cand, Counters *__restrict__ ctr, Params p, const int32_t *__restrict__ todo_vit2, int32_t *__restrict__ todo_fwd) {
  __shared__ BlockTally<1, 1, 512> tally;                  // list: todo_fwd; counter: res_fwd
  tally_reset(tally);
  const TallyOut<1, 1> out{{todo_fwd}, {&ctr->todo_fwd}, {&ctr->res_fwd}};
  const int ntodo = ctr->todo_vit2;
  for (int job0 = blockIdx.x * blockDim.x; job0 < ntodo; job0 += gridDim.x * blockDim.x) {
    if (tally_lists_full(tally)) tally_write_lists(tally, out);
    const int job = job0 + threadIdx.x;
    if (job >= ntodo) continue;
    const int c = todo_vit2[job];
    const float seqsc = (float)((double)(cand.vfsc[c] - cand.filtersc[c]) / kLog2);
    const double P = d_gumbel_surv(seqsc, p.evparam[2], p.evparam[3]);
    cand.P[c] = P;
    if (P > p.F2) { cand.stage[c] = 2; continue; }
    cand.stage[c] = 3;
    tally_push(tally, 0, c); tally_add(tally, 0, (unsigned long long)cand.len[c]);
  }
  tally_finish(tally, out);
}

// Forward P-value: F3, or F4 in the frameshift pipeline (p7_pipeline.c:1735-1738, 1779-1785)
__global__ __launch_bounds__(256) void final_kernel(Cand cand, Counters *__restrict__ ctr, Params p, const int32_t *__restrict__ todo_fwd) {
  __shared__ BlockTally<0, 2, 1> tally;                    // counters: n_past_fwd, pos_past_fwd; no list, so no barrier inside the loop
  tally_reset(tally);
  const TallyOut<0, 2> out{{nullptr}, {nullptr}, {&ctr->n_past_fwd, &ctr->pos_past_fwd}};
  const int ntodo = ctr->todo_fwd;
  for (int job = blockIdx.x * blockDim.x + threadIdx.x; job < ntodo; job += gridDim.x * blockDim.x) {
    const int c = todo_fwd[job];
    const float seqsc = (float)((double)(cand.fwdsc[c] - cand.filtersc[c]) / kLog2);
    const double P = d_exp_surv(seqsc, p.evparam[4], p.evparam[5]);
    cand.P[c] = P;
    if (P > (p.fs_pipe ? p.F4 : p.F3)) continue;
    cand.stage[c] = 4;
    tally_add(tally, 0, 1ull);
    if (!p.fs_pipe) tally_add(tally, 1, (unsigned long long)cand.len[c] * 3ull);
  }
  tally_finish(tally, out);
}

}  // namespace bath


// =================================================================================================
// host orchestration
// =================================================================================================
namespace bath {

// host twin of ssv_classify (ssvfilter.c:876-925), used only to build the emission threshold table
static int ssv_classify_host(int v, int tjb, const MsvConsts &c, float *sc) {
  if (tjb + c.tbm + c.tec + c.bias >= 127) return BATH_ENORESULT;
  unsigned xE = (v >= -1 - c.bias) ? 255u : (unsigned)(v + 256);
  if ((int)xE >= 255 - c.bias) { *sc = INFINITY; return (c.base - tjb - c.tbm < 128) ? BATH_ENORESULT : BATH_ERANGE; }
  xE = (xE + (unsigned)(c.base - tjb - c.tbm) - 128u) & 0xffffu;
  if ((int)xE >= 255 - c.bias) { *sc = INFINITY; return BATH_ERANGE; }
  unsigned xJ = (xE - (unsigned)c.tec) & 0xffffu;
  if ((int)xJ > c.base) return BATH_ENORESULT;
  float r = ((float)((int)xJ - tjb) - (float)c.base);
  r /= c.scale_b;
  r = (float)((double)r - 3.0);
  *sc = r;
  return BATH_OK;
}

// E[len] = smallest raw SSV maximum for which an ORF of <len> residues must be kept: either p7_SSVFilter
// would not return eslOK (overflow / J state possible -> needs the full MSV) or its score passes F1
// (p7_pipeline.c:1650-1652, same float/double operation order).
static void build_emit_table(const bath_hip_oprofile *om, double F1, int maxlen, std::vector<int16_t> &tab) {
  const MsvConsts mc = msv_consts(om);
  tab.assign((size_t)maxlen + 1, (int16_t)32767);
  for (int len = 0; len <= maxlen; len++) {
    const int tjb = om->lt.h_tjb[len];
    const float nullsc = om->lt.h_nullsc[len];
    auto keep = [&](int v) {
      float usc = 0.f;
      if (ssv_classify_host(v, tjb, mc, &usc) != BATH_OK) return true;
      const float seqsc = (float)((double)(usc - nullsc) / kLog2);
      return !(gumbel_surv(seqsc, om->evparam[0], om->evparam[1]) > F1);
    };
    // keep(v) is monotone in v (the score grows with v, and beyond the representable range the filter reports
    // overflow / "J state possible", which is kept too): smallest v with keep(v) by bisection over -128..127
    if (!keep(127)) continue;
    int lo = -128, hi = 127;
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (keep(mid)) hi = mid; else lo = mid + 1; }
    tab[(size_t)len] = (int16_t)lo;
  }
}

// The table depends on the model, F1 and the longest ORF only: kept with the profile (host and device) between calls.
static int ensure_emit_table(bath_hip_ctx *ctx, const bath_hip_oprofile *om, double F1, int maxlen) {
  std::lock_guard<std::mutex> lock(om->grow_mu);
  if (om->emit_F1 == F1 && om->emit_maxlen >= maxlen && om->d_emit) return BATH_OK;
  std::vector<int16_t> tab;
  build_emit_table(om, F1, maxlen, tab);
  if (om->d_emit) om->retired.push_back(om->d_emit);            // freed with the profile (bath_hip_oprofile_destroy)
  om->d_emit = nullptr;
  BATH_HIP_TRY(ctx, hipMalloc((void **)&om->d_emit, tab.size() * sizeof(int16_t) + 64));
  BATH_HIP_TRY(ctx, hipMemcpy(om->d_emit, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice));
  om->emit_F1 = F1; om->emit_maxlen = maxlen;
  return BATH_OK;
}

// The local-composition filter's term table of a new profile (bath_profile.hip calls this once, before anything shares the
// profile): compo_terms_kernel fills it, so that its floats are the device's own expf, as when the kernel ran in every call.
int build_compo_terms(bath_hip_ctx *ctx, bath_hip_oprofile *om) {
  BATH_HIP_TRY(ctx, hipMalloc((void **)&om->d_compo_terms, (size_t)(20 * 256 + 20) * sizeof(float) + 64));
  float *d_bgf = om->d_compo_terms + 20 * 256;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_bgf, kAminoBg, 20 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(compo_terms_kernel, dim3(20), dim3(256), 0, ctx->stream, d_bgf, (int)om->base_b, om->scale_b, om->d_compo_terms);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

static int wave_grid_blocks(bath_hip_ctx *ctx) { return ctx->prop.multiProcessorCount * 8; }

struct PipelineWork {
  // the device allocation is Scratch::kCascadeWork; this struct only carves it up
  Cand cand;
  int cand_cap = 0;
  uint8_t *pool = nullptr;             // the amino-acid streams of bath_orfs.hip (Scratch::kOrfAminoPool)
  int32_t *todo_msv = nullptr, *todo_vit = nullptr, *todo_ssvb = nullptr, *todo_vit2 = nullptr, *todo_fwd = nullptr, *todo_sorted = nullptr;
  int *len_bins = nullptr;
  WindowRec *wins = nullptr;
  int win_cap = 0;
  Counters *ctr = nullptr;
};

template <class T>
static T *carve(char *&p, size_t n) {
  T *r = reinterpret_cast<T *>(p);
  p += (n * sizeof(T) + 255) / 256 * 256;
  return r;
}

static size_t layout(PipelineWork &w, char *base, int cap, int win_cap) {
  char *p = base;
  const size_t n = (size_t)cap;
  w.cand_cap = cap; w.win_cap = std::max(2 * cap, win_cap);
  if (win_cap == 0) {                                     // tests: start with a window buffer that is too small (BATH_HIP_TEST_WINCAP)
    static const int forced = [] { const char *e = std::getenv("BATH_HIP_TEST_WINCAP"); return e ? std::atoi(e) : 0; }();
    if (forced > 0) w.win_cap = forced;
  }
  w.ctr = carve<Counters>(p, 1);
  w.cand.window = carve<int64_t>(p, n); w.cand.off = carve<int64_t>(p, n); w.cand.P = carve<double>(p, n);
  w.cand.sf = carve<int32_t>(p, n); w.cand.startj = carve<int32_t>(p, n); w.cand.len = carve<int32_t>(p, n);
  w.cand.msv_status = carve<int32_t>(p, n); w.cand.vit_status = carve<int32_t>(p, n); w.cand.fwd_status = carve<int32_t>(p, n); w.cand.stage = carve<int32_t>(p, n);
  w.cand.flags = carve<int32_t>(p, n); w.cand.kminmax = carve<int32_t>(p, 2 * n);
  w.cand.usc = carve<float>(p, n); w.cand.nullsc = carve<float>(p, n); w.cand.filtersc = carve<float>(p, n);
  w.cand.vfsc = carve<float>(p, n); w.cand.fwdsc = carve<float>(p, n);
  w.cand.v = carve<int16_t>(p, n);
  w.todo_msv = carve<int32_t>(p, n); w.todo_vit = carve<int32_t>(p, n); w.todo_ssvb = carve<int32_t>(p, n);
  w.todo_vit2 = carve<int32_t>(p, n); w.todo_fwd = carve<int32_t>(p, n); w.todo_sorted = carve<int32_t>(p, n);
  w.len_bins = carve<int>(p, 2048);
  w.wins = carve<WindowRec>(p, (size_t)w.win_cap);
  return (size_t)(p - base);
}

}  // namespace bath

// Self-test hook (host only, no GPU): the 20 x 256 term table by the host build of compo_term, the function compo_terms_kernel compiles.
extern "C" int bath_selftest_compo_terms(int base_b, float scale_b, float *terms) {
  if (!terms || !(scale_b > 0.f)) return BATH_EINVAL;
  for (int x = 0; x < 20; x++)
    for (int sc = 0; sc < 256; sc++) terms[x * 256 + sc] = bath::compo_term(kAminoBg[x], base_b, sc, scale_b);
  return BATH_OK;
}

extern "C" void bath_pipeline_params_default(bath_pipeline_params *p, int fs_pipe) {   // p7_pipeline.c:219-222, bathsearch.c:104
  p->F1 = 0.02; p->F2 = 1e-3; p->F3 = 1e-5; p->F4 = 5e-4;
  p->do_biasfilter = 1; p->fs_pipe = fs_pipe; p->min_orf_len = 20; p->ncbi_table = 1;
  p->nres_before = 0;
  p->do_null2 = 1; p->std_pipe = 1; p->strands = BATH_STRAND_BOTH; p->initiator = BATH_INIT_ANY;   // p7_pipeline.c:107, :199; bathsearch.c:97, :718-719
  p->inc_by_E = 1; p->seed = 42; p->T = 0.0;                                                        // p7_pipeline.c:98, :148, :165
}

extern "C" int bath_hip_pipeline_timings(const bath_hip_ctx *ctx, int max, const char **names, float *ms, int64_t *launches) {
  int n = std::min<int>(max, (int)ctx->timings.size());
  for (int i = 0; i < n; i++) { names[i] = ctx->timings[i].name; ms[i] = ctx->timings[i].ms; launches[i] = ctx->timings[i].launches; }
  return n;
}

namespace bath {
struct FilterState {               // what select_survivors reads after a lane's cascade (device memory stays in ctx->scratch)
  Cand cand{};
  const WindowRec *wins = nullptr;
  int cand_count = 0, win_count = 0, win_cap = 0;   // zero when the block is empty and the cascade returns before running
  // ... and what filters_with_survivors hands on with the survivors: the lane's pool and its model-dependent tables
  const uint8_t *pool = nullptr, *d_ssvsc = nullptr;
  const float *d_bgf = nullptr;
  OrfTablesDev tt{};
};
}  // namespace bath

// Where the Forward parser of the cascade leaves the special-state rows of its candidates (ctx->keep_fwd_rows): offsets in work-list
// order, (len + 1) x 6 floats each, by one wave (a chunk of 64 candidates per step, prefix sums by shuffle); a candidate whose rows
// would not fit <cap> floats gets -1 and no rows.
__global__ __launch_bounds__(64) void fwd_keep_offsets_kernel(const int32_t *__restrict__ todo, const int *__restrict__ ntodo_dev, const int32_t *__restrict__ len,
                                                              int64_t *__restrict__ off, int64_t cap) {
  const int lane = threadIdx.x, n = *ntodo_dev;
  int64_t base = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const int sid = j < n ? todo[j] : -1;
    const int64_t v = sid >= 0 ? ((int64_t)len[sid] + 1) * 6 : 0;
    int64_t incl = v;
    for (int d = 1; d < 64; d <<= 1) { const int64_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
    if (sid >= 0) off[sid] = (base + incl <= cap) ? base + incl - v : (int64_t)-1;
    base += __shfl(incl, 63, 64);
  }
}

// The cascade's wave kernels (BATH_WAVE_COLUMNS) stop at kCascadeMaxNodes, below what an OProfile holds (the SSV tiles go to 3328
// nodes): a longer model is refused here, before any kernel of the call runs, and not by the Viterbi stage halfway through a block.
static int cascade_model_ok(bath_hip_ctx *ctx, const bath_hip_oprofile *om) {
  if (om->M <= kCascadeMaxNodes) return BATH_OK;
  ctx->set_error("the filter cascade supports models up to " + std::to_string(kCascadeMaxNodes) + " nodes (this one has " + std::to_string(om->M) + ")");
  return BATH_EINVAL;
}

// p7_SSVFilter_BATH's windows for the <todo> candidates (their number: ctr->todo_ssvb), a wave per candidate, on <stream>: for the
// cascade's Viterbi stage and for bath_hip_ssvfilter_bath
static int launch_ssv_bath(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_oprofile *om, const Cand &cand, Counters *ctr, const int32_t *todo, const uint8_t *pool,
                           const uint8_t *ssv_scores, const MsvConsts &mc, double invP, WindowRec *wins, int win_cap) {
  BATH_TILING_SWITCH(BATH_SSVB_COLUMNS, BATH_TILING_PICK(BATH_SSVB_COLUMNS, om->M), { ctx->set_error("model too long for the SSV window kernel"); return BATH_EINVAL; },
    hipLaunchKernelGGL(ssv_bath_kernel<CC>, dim3(wave_grid_blocks(ctx) / 4), dim3(256), 0, stream, cand, ctr, todo, pool, om->M, om->d_rb, om->rb_stride, ssv_scores,
                       om->lt.d_tjb, om->lt.d_nullsc, mc, invP, wins, win_cap, ctr);)
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// the model's SSV scores by node and residue, [(M + 1) * Kp], as the window kernels and the local composition read them
static std::vector<uint8_t> host_ssv_scores(const bath_hip_oprofile *om) {
  std::vector<uint8_t> tab((size_t)(om->M + 1) * kKp, 0);
  bath_hip_oprofile_get_ssv_scores(om, tab.data());
  return tab;
}

static void stats_from_counters(bath_pipeline_stats *s, const Counters &hc, int64_t nres, int M) {
  s->nres = nres; s->n_orfs = (int64_t)hc.n_orfs;
  s->n_past_msv = (int64_t)hc.n_past_msv; s->n_past_bias = (int64_t)hc.n_past_bias;
  s->n_past_vit = (int64_t)hc.n_past_vit; s->n_past_fwd = (int64_t)hc.n_past_fwd;
  s->pos_past_msv = (int64_t)hc.pos_past_msv; s->pos_past_bias = (int64_t)hc.pos_past_bias;
  s->pos_past_vit = (int64_t)hc.pos_past_vit; s->pos_past_fwd = (int64_t)hc.pos_past_fwd;
  s->cells_msv = (int64_t)(hc.orf_res - hc.res_seen) * M; s->cells_vit = (int64_t)hc.res_vit * M; s->cells_fwd = (int64_t)hc.res_fwd * M;
}
static void stats_add(bath_pipeline_stats *tot, const bath_pipeline_stats &a) {
  tot->nres += a.nres; tot->n_orfs += a.n_orfs; tot->n_past_msv += a.n_past_msv; tot->n_past_bias += a.n_past_bias; tot->n_past_vit += a.n_past_vit;
  tot->n_past_fwd += a.n_past_fwd; tot->pos_past_msv += a.pos_past_msv; tot->pos_past_bias += a.pos_past_bias; tot->pos_past_vit += a.pos_past_vit;
  tot->pos_past_fwd += a.pos_past_fwd; tot->cells_msv += a.cells_msv; tot->cells_vit += a.cells_vit; tot->cells_fwd += a.cells_fwd;
}

namespace bath {
// What the stages of one cascade call share: run_filters builds it once, the attempts only read it.
struct Cascade {
  bath_hip_ctx *ctx; const bath_hip_oprofile *om; const bath_hip_seqs *dna; const bath_pipeline_params *prm;   // the model and the block
  int max_orf;                                    // the longest ORF the block can hold, in residues
  int64_t nres, max_orfs;                         // the block's residues as the reference counts them; the most ORFs it can hold
  Params P; MsvConsts mc;
  double invP_f1, invP_vit, invP_msv;             // the score thresholds of the window filters, from F1 and F2
  OrfTablesDev tt; const int16_t *d_emit; const uint8_t *d_ssvsc; const float *d_bgf;   // device tables
  OrfBuffers ob; size_t ssv_shmem; int dec_blocks;
  bool few_cands, few_msv, msv_stage;             // the block's path through the MSV and Viterbi stages (cascade_constants)
};

// Device time per stage: an event of ctx->ev_pool on the context's stream at begin() and at every lap(), which names the stage that
// ends there and says how many kernels it launched; finish() makes ctx->timings of them, for the attempt that did not overflow.
struct StageLaps {
  bath_hip_ctx *ctx;
  std::vector<StageTiming> laps;
  int begin() { laps.clear(); return record(); }
  int lap(const char *name, int64_t launches) { laps.push_back(StageTiming{name, 0.f, launches}); return record(); }
  int finish() {
    for (size_t i = 0; i < laps.size(); i++) BATH_HIP_TRY(ctx, hipEventElapsedTime(&laps[i].ms, ctx->ev_pool[i], ctx->ev_pool[i + 1]));
    ctx->timings = laps;
    return BATH_OK;
  }
 private:
  int record() {                                  // the event after laps.size() laps
    std::vector<hipEvent_t> &ev = ctx->ev_pool;
    while (ev.size() <= laps.size()) { hipEvent_t e; BATH_HIP_TRY(ctx, hipEventCreate(&e)); ev.push_back(e); }
    BATH_HIP_TRY(ctx, hipEventRecord(ev[laps.size()], ctx->stream));
    return BATH_OK;
  }
};
}  // namespace bath

// Per-call tables: the genetic code's codon tables, the SSV emission thresholds by ORF length (kept with the profile), and the SSV
// score table with the background frequencies behind it
static int cascade_tables(Cascade &C) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const bath_pipeline_params *prm = C.prm;
  int st;
  if (prm->strands < 0 || prm->strands > 2 || prm->initiator < 0 || prm->initiator > 2) { ctx->set_error("bath_pipeline_params: strands / initiator out of range"); return BATH_EINVAL; }
  if ((st = orf_tables_upload(ctx, prm->ncbi_table, &C.tt, prm->initiator)) != BATH_OK) return st;
  if ((st = ensure_emit_table(ctx, om, prm->F1, C.max_orf)) != BATH_OK) return st;
  DevBuf &b_tabs = ctx->scratch[Scratch::kSsvScoreTable];
  const size_t ssv_bytes = (size_t)(om->M + 1) * kKp;
  const size_t tabs_bytes = 8192 + ssv_bytes + 256 + 20 * 4 + 256;
  if (tabs_bytes > b_tabs.cap) ctx->tabs_uid = 0;                 // the buffer is about to be replaced: whatever it held is gone
  BATH_HIP_TRY(ctx, b_tabs.reserve(tabs_bytes));
  char *tp = b_tabs.as<char>();
  uint8_t *d_ssvsc = reinterpret_cast<uint8_t *>(tp); tp += (ssv_bytes + 255) / 256 * 256;
  float *d_bgf = reinterpret_cast<float *>(tp);
  if (ctx->tabs_uid != om->uid || ctx->tabs_ptr != b_tabs.p) {   // once per (context, profile): a database pass of small queries repeats this call per query
    const std::vector<uint8_t> ssv_scores = host_ssv_scores(om);
    BATH_HIP_TRY(ctx, hipMemcpyAsync(d_ssvsc, ssv_scores.data(), ssv_scores.size(), hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(d_bgf, kAminoBg, 20 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the host vector goes out of scope here
    ctx->tabs_uid = om->uid; ctx->tabs_ptr = b_tabs.p;
  }
  C.d_emit = om->d_emit; C.d_ssvsc = d_ssvsc; C.d_bgf = d_bgf;
  return BATH_OK;
}

// The thresholds and constants the kernels take by value, and the block's path through the MSV and Viterbi stages
static void cascade_constants(Cascade &C) {
  const bath_hip_oprofile *om = C.om; const bath_pipeline_params *prm = C.prm;
  C.P = Params{};
  C.P.F1 = prm->F1; C.P.F2 = prm->F2; C.P.F3 = prm->F3; C.P.F4 = prm->F4;
  C.P.do_bias = prm->do_biasfilter; C.P.fs_pipe = prm->fs_pipe; C.P.minlen = prm->min_orf_len;
  std::memcpy(C.P.evparam, om->evparam, sizeof C.P.evparam);
  C.mc = msv_consts(om);
  C.invP_f1 = gumbel_invsurv(prm->F1, om->evparam[0], om->evparam[1]);                    // p7_SSVFilter_BATH's threshold, msvfilter.c:302
  C.invP_vit = (double)(float)gumbel_invsurv(prm->F2, om->evparam[2], om->evparam[3]);   // vitfilter.c:314 (float invP)
  C.invP_msv = (double)(float)gumbel_invsurv(prm->F2, om->evparam[0], om->evparam[1]);   // vitfilter.c:319
  // The lane-per-ORF kernels pay off when the candidates fill the chip's lanes (65 k of them): a block of 10^9 nt leaves 4 x 10^5
  // Viterbi candidates, a 25 Mb query of configs[3] 5 x 10^3 -- 80 waves that each last as long as their longest ORF (0.7 ms whatever
  // their number) where the wave-per-ORF kernel takes 0.2 ms.  The candidate counts live on the device; the block's size is the
  // host's proxy.  tools/lane_crossover.py, M = 145, windows of 1 kb: Viterbi 0.72 (lane) / 0.19 (wave) ms at 12.5 k windows,
  // 0.71 / 0.63 at 100 k, 0.75 / 1.11 at 200 k; MSV 0.19 / 0.08, 0.22 / 0.10, 0.23 / 0.13, and 1.08 / 1.41 at 400 k.
  C.few_cands = C.dna->total < lane_min_nt(); C.few_msv = C.dna->total < 2 * lane_min_nt();
  C.msv_stage = !C.few_msv && msv_stage_supported(om);
}

// Capacity guess: all ORFs that could exist, scaled by the expected MSV pass rate (+ slack); retried on overflow.  The sums over the
// block's windows behind it are kept with the block (dna->cache_*) and leave C.nres and C.max_orfs.
static int cascade_capacity(Cascade &C, int64_t *cap_out) {
  const bath_hip_seqs *dna = C.dna; const bath_pipeline_params *prm = C.prm;
  if (dna->cache_minlen != prm->min_orf_len) {
    int64_t nres_c = 0, max_orfs_c = 0;
    for (int64_t i = 0; i < dna->n; i++) {
      const int n = dna->h_len[i];
      if (n < 15) continue;
      nres_c += 2 * (int64_t)(n - (dna->h_context.empty() ? 0 : dna->h_context[(size_t)i]));    // dnaSeq->W per strand
      max_orfs_c += 6 * (int64_t)((n / 3 + 1) / (prm->min_orf_len + 1) + 1);
    }
    dna->cache_minlen = prm->min_orf_len; dna->cache_nres = nres_c; dna->cache_max_orfs = max_orfs_c;
  }
  C.nres = prm->strands == BATH_STRAND_BOTH ? dna->cache_nres : dna->cache_nres / 2;   // W once per strand searched (bathsearch.c:1071, :1084)
  C.max_orfs = dna->cache_max_orfs;
  if (C.max_orfs >= (int64_t)INT32_MAX) { C.ctx->set_error("DNA block too large for one pipeline call (ORF list indices are 32-bit): split it"); return BATH_EINVAL; }
  int64_t cap = std::max<int64_t>(4096, (int64_t)((double)C.max_orfs * std::min(1.0, prm->F1 * 4.0 + 0.01)));
  cap = std::min<int64_t>(cap, std::max<int64_t>(C.max_orfs, 4096));
  {                                                         // tests: start with a candidate list that is too small (BATH_HIP_TEST_CANDCAP)
    static const int forced = [] { const char *e = std::getenv("BATH_HIP_TEST_CANDCAP"); return e ? std::atoi(e) : 0; }();
    if (forced > 0) cap = forced;                           // the first attempt only: a pass that overflows doubles it
  }
  *cap_out = cap;
  return BATH_OK;
}

// Translation / ORF work-list buffers (bath_orfs.hip), carved into C.ob; the SSV cost table's share of a workgroup's LDS
static int cascade_orf_buffers(Cascade &C) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const bath_hip_seqs *dna = C.dna;
  int st;
  if ((st = orf_tiles_ensure(ctx, dna)) != BATH_OK) return st;
  const size_t nent = (size_t)dna->ntiles * 6;
  DevBuf &b_aa = ctx->scratch[Scratch::kOrfAminoPool], &b_slots = ctx->scratch[Scratch::kOrfSlots], &b_orfs = ctx->scratch[Scratch::kOrfRecords], &b_misc = ctx->scratch[Scratch::kOrfMisc];
  BATH_HIP_TRY(ctx, b_aa.reserve(orf_aa_bytes(dna)));
  BATH_HIP_TRY(ctx, b_slots.reserve(((size_t)dna->ntiles * (size_t)orf_slot_cap(C.prm->min_orf_len) + 64) * 8));
  BATH_HIP_TRY(ctx, b_orfs.reserve((size_t)(C.max_orfs + 64) * sizeof(OrfRec)));
  BATH_HIP_TRY(ctx, b_misc.reserve((5 * nent + kOrfMiscInts) * sizeof(int32_t)));
  C.ob = OrfBuffers{};
  orf_buffers_carve(&C.ob, b_aa.p, b_slots.p, b_orfs.p, b_misc.p, nent);
  C.ssv_shmem = (size_t)kSsvRows * om->ssv_row_bytes;
  if ((st = ssv_table_fits(ctx, om)) != BATH_OK) return st;
  C.dec_blocks = ctx->prop.multiProcessorCount * 4;
  return BATH_OK;
}

// ---- the six stages of one attempt.  Each enqueues on the context's stream and ends with its lap.
static SeqView cand_view(const PipelineWork &W) { return SeqView{W.pool, W.cand.off, W.cand.len, W.cand_cap}; }   // the candidates as a sequence block

// 1. six-frame translation, ORFs, length-sorted work list
static int stage_translate(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  const int st = launch_orf_scan(C.ctx, C.dna, C.tt, C.prm->min_orf_len, C.ob, &W.ctr->n_orfs, &W.ctr->orf_res, C.prm->strands);
  return st != BATH_OK ? st : laps.lap("translate_orfs", 4);
}

// 2. SSV + F1 threshold, lane per ORF
static int stage_ssv_f1(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const bath_hip_seqs *dna = C.dna; const OrfBuffers &ob = C.ob; const int16_t *d_emit = C.d_emit;   // (the names the dispatch macro uses)
  const int NRk = om->NR, max_orf = C.max_orf, blocks = ctx->prop.multiProcessorCount * 4, ssv_threads = 256;
  const size_t ssv_shmem = C.ssv_shmem;
  bool launched = false;
#define BATH_ORF_CASE(N, GG)                                                                                                     \
  if (!launched && NRk == N && om->G == GG) {                                                                                    \
    if (ssv_shmem > 64 * 1024) (void)bath::allow_max_lds((const void *)ssv_orf_kernel<N, GG>); \
    hipLaunchKernelGGL((ssv_orf_kernel<N, GG>), dim3(blocks), dim3(ssv_threads), ssv_shmem, ctx->stream, W.pool, ob.sorted, ob.ntotal,                  \
                       dna->view(), om->d_ssv, om->ssv_row_bytes, d_emit, max_orf, W.cand, W.cand_cap, W.ctr);                   \
    launched = true;                                                                                                             \
  }
  BATH_SSV_SHAPES(BATH_ORF_CASE)
#undef BATH_ORF_CASE
  if (!launched) { ctx->set_error("SSV kernel: no tile shape for this model length"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, hipGetLastError());
  return laps.lap("ssv_f1", 1);
}

// 3. SSV status, full MSV for the undecided, F1 on the MSV score and the bias filter: one kernel with a lane per candidate for a large
// block, three for a small one.  Both leave the laps "classify_msv" and "f1_bias", the second empty on the one-kernel path.
static int stage_msv(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const Params &P = C.P; const MsvConsts &mc = C.mc;
  const int M = om->M, NRk = om->NR;
  const size_t ssv_shmem = C.ssv_shmem;
  const F1Tables f1t{om->d_bias_eo, om->lt.d_nullsc, om->lt.d_p1, om->lt.d_lt1, om->lt.d_lt2};
  int st;
  if (C.msv_stage) {
    bool launched = false;
#define BATH_MSV_STAGE_CASE(N, ...)                                                                                                         \
  if (!launched && NRk == N) {                                                                                                              \
    hipLaunchKernelGGL((msv_stage_kernel<N>), dim3((unsigned)((W.cand_cap + 255) / 256)), dim3(256), ssv_shmem, ctx->stream, W.cand, W.cand_cap, W.ctr, om->d_msv, \
                       om->ssv_row_bytes, om->lt.d_tjb, mc, P, W.pool, M, f1t, W.todo_vit, W.todo_ssvb);                                      \
    launched = true;                                                                                                                        \
  }
    BATH_MSV_LANE_NR(BATH_MSV_STAGE_CASE)
#undef BATH_MSV_STAGE_CASE
    if (!launched) { ctx->set_error("MSV stage kernel: no tile shape for this model length"); return BATH_EINVAL; }
    BATH_HIP_TRY(ctx, hipGetLastError());
    if ((st = laps.lap("classify_msv", 1)) != BATH_OK) return st;
    return laps.lap("f1_bias", 0);                            // the stage keeps its entry in the timings
  }
  hipLaunchKernelGGL(classify_kernel, dim3(C.dec_blocks), dim3(256), 0, ctx->stream, W.cand, W.cand_cap, W.ctr, om->lt.d_tjb, mc, W.todo_msv);
  BATH_HIP_TRY(ctx, hipGetLastError());
  if ((st = launch_msv_wave(ctx, om, cand_view(W), W.todo_msv, W.cand_cap, W.cand.usc, W.cand.msv_status, &W.ctr->todo_msv, !C.few_msv)) != BATH_OK) return st;
  if ((st = laps.lap("classify_msv", 2)) != BATH_OK) return st;
  hipLaunchKernelGGL(f1_bias_kernel, dim3(C.dec_blocks), dim3(256), 0, ctx->stream, W.cand, W.cand_cap, W.ctr, P, W.pool, M, f1t, W.todo_vit, W.todo_ssvb);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return laps.lap("f1_bias", 1);
}

// 4. Viterbi filter with windows (P > F2) / SSV windows (P <= F2)
static int stage_viterbi(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const int64_t cap = W.cand_cap;
  VitWindowArgs wa{};
  wa.invP_vit = C.invP_vit; wa.invP_msv = C.invP_msv;
  wa.d_filtersc = W.cand.filtersc; wa.d_ssv_scores = C.d_ssvsc; wa.d_wins = W.wins; wa.d_win_count = &W.ctr->win_count; wa.win_cap = W.win_cap;
  wa.d_kminmax = W.cand.kminmax;
  // p7_SSVFilter_BATH's windows for the candidates with P <= F2: other candidates than the Viterbi kernels', so it runs beside them
  auto launch_ssvb = [&](hipStream_t stream) -> int {
    return launch_ssv_bath(ctx, stream, om, W.cand, W.ctr, W.todo_ssvb, W.pool, C.d_ssvsc, C.mc, C.invP_f1, W.wins, W.win_cap);
  };
  int st;
  bool ssvb_done = false;
  if (vit_lane_supported(om) && !C.few_cands) {       // lane per ORF, ORFs bucketed by length, the long ones to the wave kernel (bath_viterbi.hip)
    if ((st = launch_vit_sorted(ctx, om, cand_view(W), W.todo_vit, cap, &W.ctr->todo_vit, W.cand.len, W.len_bins, W.todo_sorted, W.cand.vfsc, W.cand.vit_status, &wa,
                                launch_ssvb)) != BATH_OK) return st;      // ... and the SSV windows, all under the lane kernel
    ssvb_done = true;
  } else if ((st = launch_vit_wave(ctx, om, cand_view(W), W.todo_vit, cap, W.cand.vfsc, W.cand.vit_status, &wa, &W.ctr->todo_vit)) != BATH_OK) return st;
  if ((st = laps.lap("viterbi_windows", 4)) != BATH_OK) return st;
  if (!ssvb_done && (st = launch_ssvb(ctx->stream)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipGetLastError());
  return laps.lap("ssv_windows", 1);
}

// 5. F2, local composition re-filter, optional plain Viterbi re-run
static int stage_post_vit(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const Params &P = C.P;
  int st;
  hipLaunchKernelGGL(post_vit_kernel, dim3(C.dec_blocks), dim3(256), 0, ctx->stream, W.cand, W.cand_cap, W.ctr, P, W.todo_msv /* free by now */, W.todo_fwd);
  if (P.do_bias) {
    DevBuf &b_compo = ctx->scratch[Scratch::kLocalCompoSums];                                       // 20 sums per candidate (the 20 x 256 terms are the profile's)
    BATH_HIP_TRY(ctx, b_compo.reserve((size_t)W.cand_cap * 20 * 4 + 256));
    float *d_compo = b_compo.as<float>();
    hipLaunchKernelGGL(local_compo_kernel, dim3(16384), dim3(64), 0, ctx->stream, W.cand, W.ctr, om->M, C.d_ssvsc, om->d_compo_terms, W.todo_msv, d_compo);
    hipLaunchKernelGGL(post_vit_local_kernel, dim3(std::max(1, C.dec_blocks)), dim3(64), 0, ctx->stream, W.cand, W.ctr, P, W.pool, om->M, C.d_bgf, d_compo,
                       om->lt.d_p1, om->lt.d_lt1, om->lt.d_lt2, W.todo_msv, W.todo_vit2, W.todo_fwd);
  }
  BATH_HIP_TRY(ctx, hipGetLastError());
  if ((st = launch_vit_wave(ctx, om, cand_view(W), W.todo_vit2, W.cand_cap, W.cand.vfsc, W.cand.vit_status, nullptr, &W.ctr->todo_vit2)) != BATH_OK) return st;
  hipLaunchKernelGGL(post_vit2_kernel, dim3(64), dim3(256), 0, ctx->stream, W.cand, W.ctr, P, W.todo_vit2, W.todo_fwd);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return laps.lap("post_vit", 3);
}

// 6. Forward parser, F3/F4 (for the domain stage of a one-lane block it also leaves its special-state rows: ctx->keep_fwd_rows)
static int stage_forward(const Cascade &C, const PipelineWork &W, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_oprofile *om = C.om;
  const int64_t cap = W.cand_cap;
  int st;
  ctx->fwd_rows_kept = nullptr; ctx->fwd_rows_off = nullptr;
  float *d_keep = nullptr; int64_t *d_keep_off = nullptr;
  if (ctx->keep_fwd_rows) {
    constexpr int64_t kKeepFloats = (int64_t)8 << 20;                        // 32 MB: ~1.4 M residue rows; what does not fit is computed again by the domain stage
    DevBuf &b_rows = ctx->scratch[Scratch::kCascadeFwdRows], &b_roff = ctx->scratch[Scratch::kCascadeFwdRowOffsets];
    BATH_HIP_TRY(ctx, b_rows.reserve((size_t)kKeepFloats * sizeof(float) + 64)); BATH_HIP_TRY(ctx, b_roff.reserve((size_t)cap * sizeof(int64_t) + 64));
    d_keep = b_rows.as<float>(); d_keep_off = b_roff.as<int64_t>();
    hipLaunchKernelGGL(fwd_keep_offsets_kernel, dim3(1), dim3(64), 0, ctx->stream, W.todo_fwd, &W.ctr->todo_fwd, W.cand.len, d_keep_off, kKeepFloats);
    BATH_HIP_TRY(ctx, hipGetLastError());
  }
  // The candidates of a model of up to 160 nodes: four per wave, a quarter wave each, the list sorted by length so that a wave's four
  // end together (bath_fwd_group.hip; todo_sorted and len_bins are free since the Viterbi stage joined its side stream).
  // final_kernel reads the scores by candidate, whatever the list's order.  Blocks of every size take it -- it pays on the tens of
  // thousands of candidates of a large block, and a small block's few are scored by the same arithmetic: the group kernel and
  // fwd_wave_kernel agree within the parser's tolerance and not by bits, and an ORF's record does not depend on its block's size.
  const bool fwd_group = !d_keep && fwd_group_supported(om) && ctx->fwd_group != 2;
  if (fwd_group) {
    if ((st = launch_len_sort(ctx, W.todo_fwd, &W.ctr->todo_fwd, W.cand.len, W.len_bins, W.todo_sorted)) != BATH_OK) return st;
    if ((st = launch_fwd_group(ctx, om, cand_view(W), W.todo_sorted, cap, &W.ctr->todo_fwd, &W.ctr->fwd_next, W.cand.fwdsc, W.cand.fwd_status)) != BATH_OK) return st;
  } else if ((st = launch_fwd_wave(ctx, om, cand_view(W), W.todo_fwd, cap, W.cand.fwdsc, W.cand.fwd_status, &W.ctr->todo_fwd, d_keep, d_keep_off)) != BATH_OK) return st;
  if (d_keep) { ctx->fwd_rows_kept = d_keep; ctx->fwd_rows_off = d_keep_off; }
  hipLaunchKernelGGL(final_kernel, dim3(C.dec_blocks), dim3(256), 0, ctx->stream, W.cand, W.ctr, C.P, W.todo_fwd);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return laps.lap("forward_final", (d_keep ? 1 : 0) + (fwd_group ? 4 : 1) + 1);   // [row offsets,] Forward (the group kernel behind the sort's three), final_kernel
}

// One pass over the block with room for <cap> candidates and <win_need> hit windows (0: the default, twice the candidates): W laid out
// afresh in Scratch::kCascadeWork, the counters zeroed, the six stages, the counters in *hc once the stream is idle
static int cascade_attempt(const Cascade &C, int64_t cap, int win_need, PipelineWork &W, Counters *hc, StageLaps &laps) {
  bath_hip_ctx *ctx = C.ctx;
  DevBuf &b_work = ctx->scratch[Scratch::kCascadeWork];
  const size_t need = layout(W, nullptr, (int)cap, win_need);
  BATH_HIP_TRY(ctx, b_work.reserve(need + 4096));
  layout(W, b_work.as<char>(), (int)cap, win_need);
  W.pool = C.ob.aa;
  BATH_HIP_TRY(ctx, hipMemsetAsync(W.ctr, 0, sizeof(Counters), ctx->stream));
  int st;
  if ((st = laps.begin()) != BATH_OK) return st;
  if ((st = stage_translate(C, W, laps)) != BATH_OK) return st;
  if ((st = stage_ssv_f1(C, W, laps)) != BATH_OK) return st;
  if ((st = stage_msv(C, W, laps)) != BATH_OK) return st;
  if ((st = stage_viterbi(C, W, laps)) != BATH_OK) return st;
  if ((st = stage_post_vit(C, W, laps)) != BATH_OK) return st;
  if ((st = stage_forward(C, W, laps)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(hc, W.ctr, sizeof(Counters), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

// One record per ORF past MSV, assembled and ordered on the device (bath_records.hip).  A part of a larger block leaves them
// there: bath_hip_pipeline_filters copies every part's records straight into their place in one page-locked array.
static int cascade_records(const Cascade &C, const Cand &cand, int cand_count, const bath_orf_result **results, int64_t *n_results) {
  bath_hip_ctx *ctx = C.ctx; const bath_hip_seqs *dna = C.dna;
  bath_orf_result *d_rec = nullptr;
  int64_t nrec = 0;
  int st;
  // the records' sort key holds the window in 32 bits and the ORF's first codon in 28 (bath_records.hip)
  if (dna->n > (int64_t)UINT32_MAX || dna->maxlen / 3 >= (1 << 28)) { ctx->set_error("block too large for the ORF records' sort key (2^32 windows, 805 Mnt per window)"); return BATH_ERANGE; }
  if ((st = build_orf_records(ctx, cand, cand_count, dna->is_part ? dna->first_window : 0, &d_rec, &nrec)) != BATH_OK) return st;
  ctx->d_records = d_rec; ctx->n_records = nrec;
  if (!dna->is_part) {
    BATH_HIP_TRY(ctx, ctx->results_pinned.reserve((size_t)std::max<int64_t>(nrec, 1) * sizeof(bath_orf_result)));
    if (nrec > 0) BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->results_pinned.p, d_rec, (size_t)nrec * sizeof(bath_orf_result), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *results = ctx->results_pinned.as<bath_orf_result>();
  } else *results = nullptr;
  if (n_results) *n_results = nrec;
  return BATH_OK;
}

static int run_filters(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna,
                       const bath_pipeline_params *prm, bath_pipeline_stats *stats,
                       const bath_orf_result **results, int64_t *n_results, FilterState *state) {
  if (!ctx || !om || !dna || !prm) return BATH_EINVAL;
  if (cascade_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n_results) *n_results = 0;
  if (results) *results = nullptr;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (dna->n == 0) return BATH_OK;
  Cascade C{};
  C.ctx = ctx; C.om = om; C.dna = dna; C.prm = prm;
  C.max_orf = dna->maxlen / 3 + 1;
  int st = om->ensure_len_tables(C.max_orf);
  if (st != BATH_OK) return st;
  if ((st = cascade_tables(C)) != BATH_OK) return st;
  cascade_constants(C);
  int64_t cap = 0;
  if ((st = cascade_capacity(C, &cap)) != BATH_OK) return st;
  if ((st = cascade_orf_buffers(C)) != BATH_OK) return st;

  PipelineWork W;
  Counters hc{};
  StageLaps laps{ctx, {}};
  int win_need = 0;                                         // hit windows seen by a pass that ran out of room for them
  for (int attempt = 0;; attempt++) {
    if ((st = cascade_attempt(C, cap, win_need, W, &hc, laps)) != BATH_OK) return st;
    // the reference's window list grows without limit (p7_hmmwindow.c:83); here the kernels count every window they find and
    // drop those beyond the buffer, so a pass that found more windows than fit is repeated with room for all of them
    if (!(hc.overflow || hc.cand_count > cap || hc.win_count > W.win_cap)) break;
    if (attempt >= 4) { ctx->set_error("candidate / window buffers overflowed repeatedly"); return BATH_EMEM; }
    if (hc.overflow || hc.cand_count > cap) cap = std::max<int64_t>(cap * 2, (int64_t)hc.cand_count + 1024);
    if (hc.win_count > W.win_cap) win_need = hc.win_count + hc.win_count / 4 + 1024;
  }
  if ((st = laps.finish()) != BATH_OK) return st;

  if (stats) stats_from_counters(stats, hc, C.nres, om->M);
  if (results) {
    if ((st = cascade_records(C, W.cand, hc.cand_count, results, n_results)) != BATH_OK) return st;
  } else if (n_results) *n_results = (int64_t)hc.n_past_msv;
  if (state) {
    state->cand = W.cand; state->wins = W.wins; state->cand_count = hc.cand_count; state->win_count = hc.win_count; state->win_cap = W.win_cap;
    state->pool = W.pool; state->d_ssvsc = C.d_ssvsc; state->d_bgf = C.d_bgf; state->tt = C.tt;
  }
  return BATH_OK;
}

// ---- concurrent lanes --------------------------------------------------------------------------------------------
// The cascade's tail (decision kernels, wave-per-candidate DP over a few 10^5 survivors) is latency bound and leaves
// most of the chip idle, while SSV saturates the VALUs.  A large block is therefore cut into K parts of consecutive
// windows that run the whole cascade concurrently, each on its own HIP stream with its own scratch memory (a "lane"
// context) driven by its own host thread: one part's tail overlaps another part's translation and SSV.
static int pipeline_lane_count(const bath_hip_seqs *dna) {
  const char *e = std::getenv("BATH_HIP_LANES");                  // override for tests and tuning
  const int forced = e ? std::atoi(e) : 0;
  if (forced > 0) return (int)std::min<int64_t>(forced, std::max<int64_t>(dna->n, 1));
  if (dna->is_part || dna->n < 8) return 1;
  // measured on MI355X, 10^6 x 1 kb: 1 lane 17.2 ms, 2 lanes 15.5 ms per pass; 3 lanes 15.4-19.3 ms depending on how the
  // persistent grids of the three parts happen to interleave, 4 lanes 19.7 ms: two lanes is the robust choice
  int K = (dna->total >= ((int64_t)1 << 28)) ? 2 : 1;           // blocks under 256 MB: one launch sequence is short enough
  // ... and as many parts as it takes to keep a part's ORF list within 32-bit indices (run_filters: ~1 ORF per 27 nt on both
  // strands of iid DNA; a part of 16 GB holds ~6e8): a larger block is cut into more parts instead of being refused
  const int64_t by_size = (dna->total + ((int64_t)1 << 34) - 1) >> 34;
  if (by_size > K) K = (int)std::min<int64_t>(by_size, std::max<int64_t>(dna->n, 1));
  return K;
}

static int ensure_parts(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int K) {
  if ((int)dna->parts.size() == K) return BATH_OK;
  for (bath_hip_seqs *p : dna->parts) bath_hip_seqs_destroy(p);
  dna->parts.clear();
  int64_t w0 = 0;
  for (int k = 0; k < K; k++) {
    // cut where the running residue count passes the part's share of the total: equal shares
    int64_t w1 = w0;
    if (k == K - 1) w1 = dna->n;
    else {
      const int64_t target = dna->total_aligned / K * (k + 1);
      w1 = std::lower_bound(dna->h_off.begin() + w0, dna->h_off.end(), target) - dna->h_off.begin();
      w1 = std::max(w1, std::min(w0 + 1, dna->n));
    }
    bath_hip_seqs *p = new bath_hip_seqs();
    p->ctx = ctx; p->is_part = true; p->first_window = w0; p->n = w1 - w0;
    const int64_t base = w0 < dna->n ? dna->h_off[(size_t)w0] : dna->total_aligned;
    p->h_off.resize((size_t)p->n); p->h_len.assign(dna->h_len.begin() + w0, dna->h_len.begin() + w1);
    for (int64_t i = 0; i < p->n; i++) {
      p->h_off[(size_t)i] = dna->h_off[(size_t)(w0 + i)] - base;
      p->maxlen = std::max(p->maxlen, p->h_len[(size_t)i]);
      p->total += p->h_len[(size_t)i];
    }
    p->total_aligned = (w1 < dna->n ? dna->h_off[(size_t)w1] : dna->total_aligned) - base;
    p->d_data = dna->d_data + base;
    p->d_len = dna->d_len + w0;
    if (dna->d_context) { p->d_context = dna->d_context + w0; p->h_context.assign(dna->h_context.begin() + w0, dna->h_context.begin() + w1); }
    dna->parts.push_back(p);
    if (hipMalloc((void **)&p->d_off, (size_t)std::max<int64_t>(p->n, 1) * sizeof(int64_t)) != hipSuccess) { ctx->set_error("hipMalloc (block parts)"); return BATH_EMEM; }
    if (p->n > 0 && hipMemcpy(p->d_off, p->h_off.data(), (size_t)p->n * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) { ctx->set_error("hipMemcpy (block parts)"); return BATH_EFAIL; }
    w0 = w1;
  }
  return BATH_OK;
}

// The cascade of a block, as K concurrent parts when the block is large.  <after>(k, lane, part, S) runs on the lane's own host
// thread right after that part's cascade, with the lane's device state still in place (S: its candidate arrays, windows, pool).
template <class After>
static int run_filters_lanes(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna,
                             const bath_pipeline_params *prm, bath_pipeline_stats *stats,
                             const bath_orf_result **results, int64_t *n_results, std::vector<FilterState> *states, After after) {
  if (!ctx || !om || !dna || !prm) return BATH_EINVAL;
  if (cascade_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  const int K = pipeline_lane_count(dna);
  if (K <= 1) {
    states->assign(1, FilterState{});
    int st = run_filters(ctx, om, dna, prm, stats, results, n_results, &(*states)[0]);
    if (st != BATH_OK) return st;
    return after(0, ctx, dna, (*states)[0]);
  }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = om->ensure_len_tables(dna->maxlen / 3 + 1);            // the mutable state of the profile: fill it before the threads start
  if (st != BATH_OK) return st;
  if ((st = ensure_emit_table(ctx, om, prm->F1, dna->maxlen / 3 + 1)) != BATH_OK) return st;
  while ((int)ctx->lanes.size() < K) {
    bath_hip_ctx *lane = nullptr;
    if ((st = bath_hip_init(ctx->device, &lane)) != BATH_OK) { ctx->set_error("cannot create a pipeline lane"); return st; }
    mark_internal(lane);
    // Descending stream priorities: when two parts have work ready, the earlier part's workgroups are dispatched first.  Left to
    // the hardware queues the interleaving of the parts is a race and about every third process lands on a schedule that is
    // 20% slower (13.4 vs 16 ms per step on the bench block); with priorities it is 13.2-13.9 ms every time (tools/ab_probe.py).
    // Where the device reports no priority range the lane keeps the stream it was created with.
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
      (void)hipStreamDestroy(lane->stream);
      // hi is numerically the smallest value = highest priority
      if (hipStreamCreateWithPriority(&lane->stream, hipStreamNonBlocking, ctx->lanes.empty() ? hi : lo) != hipSuccess) { ctx->set_error("hipStreamCreateWithPriority"); return BATH_EFAIL; }
    }
    ctx->lanes.push_back(lane);
  }
  for (bath_hip_ctx *lane : ctx->lanes) { lane->fs_strict = ctx->fs_strict; lane->fs_odds = ctx->fs_odds; lane->fs5_odds = ctx->fs5_odds; lane->fwd_group = ctx->fwd_group; }
  if ((st = ensure_parts(ctx, dna, K)) != BATH_OK) return st;
  std::vector<bath_pipeline_stats> pst((size_t)K);
  std::vector<int64_t> pn((size_t)K, 0);
  std::vector<int> rc((size_t)K, BATH_OK);
  states->assign((size_t)K, FilterState{});
  // The lanes' streams are non-blocking streams of their own: nothing orders them after the context's stream, which may still
  // hold the block's upload and expansion kernels (bath_hip_seqs_upload_packed / _upload_wait) or the part offsets copied above.
  if (!ctx->ev_lanes) BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_lanes, hipEventDisableTiming));
  BATH_HIP_TRY(ctx, hipEventRecord(ctx->ev_lanes, ctx->stream));
  for (int k = 0; k < K; k++) BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->lanes[(size_t)k]->stream, ctx->ev_lanes, 0));
  if (!ctx->lane_pool) ctx->lane_pool = new LanePool();            // the lanes' host threads live as long as the context
  ctx->lane_pool->run(K, [&](int k) {
    bath_hip_ctx *lane = ctx->lanes[(size_t)k];
    const bath_orf_result *left_on_device = nullptr;               // a part's records stay in lane->d_records
    rc[(size_t)k] = run_filters(lane, om, dna->parts[(size_t)k], prm, &pst[(size_t)k], results ? &left_on_device : nullptr, &pn[(size_t)k], &(*states)[(size_t)k]);
    if (rc[(size_t)k] == BATH_OK) rc[(size_t)k] = after(k, lane, dna->parts[(size_t)k], (*states)[(size_t)k]);
  });
  for (int k = 0; k < K; k++)
    if (rc[(size_t)k] != BATH_OK) { ctx->set_error(ctx->lanes[(size_t)k]->err); return rc[(size_t)k]; }

  bath_pipeline_stats tot{};
  int64_t ntot = 0;
  for (int k = 0; k < K; k++) {
    stats_add(&tot, pst[(size_t)k]);
    ntot += pn[(size_t)k];
  }
  if (stats) *stats = tot;
  if (results) {                                                   // parts are consecutive windows; each part's records are ordered, on its device
    BATH_HIP_TRY(ctx, ctx->results_pinned.reserve((size_t)std::max<int64_t>(ntot, 1) * sizeof(bath_orf_result)));
    bath_orf_result *dst = ctx->results_pinned.as<bath_orf_result>();
    int64_t at = 0;
    for (int k = 0; k < K; k++) {
      bath_hip_ctx *lane = ctx->lanes[(size_t)k];
      const int64_t nk = pn[(size_t)k];
      if (nk > 0) BATH_HIP_TRY(ctx, hipMemcpyAsync(dst + at, lane->d_records, (size_t)nk * sizeof(bath_orf_result), hipMemcpyDeviceToHost, lane->stream));
      at += nk;
    }
    for (int k = 0; k < K; k++) BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->lanes[(size_t)k]->stream));
    *results = dst;
  }
  if (n_results) *n_results = ntot;
  // stage timings: device time summed over the lanes (they overlap in wall-clock time)
  ctx->timings.clear();
  for (int k = 0; k < K; k++) {
    const std::vector<StageTiming> &t = ctx->lanes[(size_t)k]->timings;
    for (size_t i = 0; i < t.size(); i++) {
      if (k == 0) ctx->timings.push_back(t[i]);
      else if (i < ctx->timings.size()) { ctx->timings[i].ms += t[i].ms; ctx->timings[i].launches += t[i].launches; }
    }
  }
  return BATH_OK;
}

extern "C" int bath_hip_pipeline_filters(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna,
                                         const bath_pipeline_params *prm, bath_pipeline_stats *stats,
                                         const bath_orf_result **results, int64_t *n_results) {
  std::vector<FilterState> states;
  return run_filters_lanes(ctx, om, dna, prm, stats, results, n_results, &states,
                           [](int, bath_hip_ctx *, const bath_hip_seqs *, const FilterState &) { return (int)BATH_OK; });
}

// ---- the cascade's survivors, for the hits path (pipeline_filters_survivors) and the frameshift stage (bath_fs_stage.hip) -------
namespace bath {

// The frameshift stage needs only the ORFs that passed F4 (a few thousand of the block's 10^5-10^6 MSV survivors) and their
// hit windows: select them on the device, so that what crosses PCIe is a few hundred KB instead of every candidate array.
// (FsCandRec: bath_launch.hpp)
__global__ void fs_select_cands_kernel(Cand cand, int nc, FsCandRec *__restrict__ out, int *__restrict__ count, const int64_t *__restrict__ fxoff /* kept Forward rows by candidate, or null */) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    if (cand.stage[c] != 4) continue;
    const int slot = atomicAdd(count, 1);
    out[slot] = FsCandRec{cand.window[c], cand.off[c], cand.P[c], c, cand.sf[c], cand.startj[c], cand.len[c], cand.fwdsc[c], cand.nullsc[c], fxoff ? fxoff[c] : (int64_t)-1};
  }
}
__global__ void fs_select_wins_kernel(const WindowRec *__restrict__ wins, int nwins, const int32_t *__restrict__ stage, WindowRec *__restrict__ out, int *__restrict__ count) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nwins; i += gridDim.x * blockDim.x) {
    const WindowRec w = wins[i];
    if (stage[w.cand] != 4) continue;
    out[atomicAdd(count, 1)] = w;
  }
}

static int fetch_survivors(bath_hip_ctx *lane, const FsLaneSurv &ls, std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins) {
  sel->resize((size_t)ls.n_c); wins->resize((size_t)ls.n_w);
  if (ls.n_c) BATH_HIP_TRY(lane, hipMemcpyAsync(sel->data(), ls.d_c, sel->size() * sizeof(FsCandRec), hipMemcpyDeviceToHost, lane->stream));
  if (ls.n_w) BATH_HIP_TRY(lane, hipMemcpyAsync(wins->data(), ls.d_w, wins->size() * sizeof(WindowRec), hipMemcpyDeviceToHost, lane->stream));
  BATH_HIP_TRY(lane, hipStreamSynchronize(lane->stream));
  fs_order_survivors(sel, wins);           // the kernels append in completion order: candidate order makes what follows deterministic
  return BATH_OK;
}

static int select_survivors(bath_hip_ctx *lane, const FilterState &S, bool want_wins, std::vector<FsCandRec> *sel, std::vector<WindowRec> *wins,
                            FsLaneSurv *dev = nullptr /* non-null: leave the lists on the device, report where */) {
  sel->clear(); wins->clear();
  if (dev) *dev = FsLaneSurv{};
  const int nc = S.cand_count;
  if (nc <= 0) return BATH_OK;
  const int nwins = want_wins ? std::min(S.win_count, S.win_cap) : 0;
  DevBuf &b_sel = lane->scratch[Scratch::kSurvivorSelect];
  const size_t o_c = 256, o_w = o_c + ((size_t)nc * sizeof(FsCandRec) + 255) / 256 * 256;
  BATH_HIP_TRY(lane, b_sel.reserve(o_w + (size_t)std::max(nwins, 1) * sizeof(WindowRec) + 256));
  int *d_cnt = b_sel.as<int>();
  FsCandRec *d_c = reinterpret_cast<FsCandRec *>(b_sel.as<char>() + o_c);
  WindowRec *d_w = reinterpret_cast<WindowRec *>(b_sel.as<char>() + o_w);
  BATH_HIP_TRY(lane, hipMemsetAsync(d_cnt, 0, 256, lane->stream));
  const int blocks = lane->prop.multiProcessorCount * 4;
  hipLaunchKernelGGL(fs_select_cands_kernel, dim3(blocks), dim3(256), 0, lane->stream, S.cand, nc, d_c, d_cnt, lane->fwd_rows_kept ? lane->fwd_rows_off : nullptr);
  if (nwins > 0) hipLaunchKernelGGL(fs_select_wins_kernel, dim3(blocks), dim3(256), 0, lane->stream, S.wins, nwins, S.cand.stage, d_w, d_cnt + 1);
  BATH_HIP_TRY(lane, hipGetLastError());
  int h_cnt[2] = {0, 0};
  BATH_HIP_TRY(lane, hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, lane->stream));
  BATH_HIP_TRY(lane, hipStreamSynchronize(lane->stream));
  FsLaneSurv ls{};
  ls.d_c = d_c; ls.d_w = d_w; ls.n_c = h_cnt[0]; ls.n_w = h_cnt[1];
  if (dev) { *dev = ls; return BATH_OK; }
  return fetch_survivors(lane, ls, sel, wins);
}

static void merge_lane_lists(SurvivorSet *out, const std::vector<std::vector<FsCandRec>> &lsel, const std::vector<std::vector<WindowRec>> &lwin) {
  fs_merge_survivors(out->lanes.data(), out->n_states, lsel, lwin, &out->sel, &out->wins);
}

int survivors_to_host(SurvivorSet *sv) {
  if (!sv->on_device) return BATH_OK;
  std::vector<std::vector<FsCandRec>> lsel((size_t)sv->n_states);
  std::vector<std::vector<WindowRec>> lwin((size_t)sv->n_states);
  for (size_t k = 0; k < (size_t)sv->n_states; k++) {
    const int st = fetch_survivors(sv->lane_ctx[k], sv->lanes[k], &lsel[k], &lwin[k]);
    if (st != BATH_OK) return st;
  }
  merge_lane_lists(sv, lsel, lwin);
  sv->on_device = false;
  return BATH_OK;
}

int filters_with_survivors(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                           bath_pipeline_stats *stats, const bath_orf_result **results, int64_t *n_results, bool want_wins, SurvivorSet *out, bool device_only) {
  std::vector<FilterState> states;
  const size_t nl = (size_t)std::max(1, pipeline_lane_count(dna));
  std::vector<std::vector<FsCandRec>> lsel(nl);
  std::vector<std::vector<WindowRec>> lwin(nl);
  std::vector<int64_t> first(nl, 0);
  std::vector<FsLaneSurv> ldev(nl);
  std::vector<bath_hip_ctx *> lctx(nl, nullptr);
  int st = run_filters_lanes(ctx, om, dna, prm, stats, results, n_results, &states,
                             [&](int k, bath_hip_ctx *lane, const bath_hip_seqs *part, const FilterState &S) {
                               if ((size_t)k >= nl) { lane->set_error("more pipeline lanes than the survivor merge was sized for"); return (int)BATH_EFAIL; }
                               first[(size_t)k] = part->is_part ? part->first_window : 0;
                               lctx[(size_t)k] = lane;
                               return select_survivors(lane, S, want_wins, &lsel[(size_t)k], &lwin[(size_t)k], device_only ? &ldev[(size_t)k] : nullptr);
                             });
  if (st != BATH_OK) return st;
  out->sel.clear(); out->wins.clear(); out->nc_total = 0;
  const FilterState S0 = states.empty() ? FilterState{} : states[0];          // the first lane's tables: any lane holds them alike
  out->pool = S0.pool; out->tt = S0.tt; out->d_ssvsc = S0.d_ssvsc; out->d_bgf = S0.d_bgf;
  out->n_states = (int)states.size();
  out->lanes.assign(ldev.begin(), ldev.begin() + (ptrdiff_t)states.size());
  out->lane_ctx.assign(lctx.begin(), lctx.begin() + (ptrdiff_t)states.size());
  for (size_t k = 0; k < states.size(); k++) {
    FsLaneSurv &ls = out->lanes[k];
    ls.cand_base = out->nc_total;
    ls.first_window = first[k];
    ls.dpool = (int64_t)(reinterpret_cast<intptr_t>(states[k].pool) - reinterpret_cast<intptr_t>(out->pool));
    out->nc_total += std::max(states[k].cand_count, 0);
  }
  out->on_device = device_only;
  if (!device_only) merge_lane_lists(out, lsel, lwin);                     // (the lanes fetched and ordered their lists as they finished)
  return BATH_OK;
}

}  // namespace bath

int bath::pipeline_filters_survivors(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                                     bath_pipeline_stats *stats, std::vector<PipelineSurvivor> *out, const uint8_t **d_pool) {
  out->clear();
  SurvivorSet sv;
  int st = filters_with_survivors(ctx, om, dna, prm, stats, nullptr, nullptr, false, &sv);
  if (st != BATH_OK) return st;
  *d_pool = sv.pool;
  out->reserve(sv.sel.size());
  for (const FsCandRec &q : sv.sel) {
    PipelineSurvivor o;
    o.window = q.window; o.aa_off = q.aa_off; o.strand = q.sf / 3; o.start = q.sf % 3 + 3 * q.startj + 1; o.n = q.len;
    o.fx_off = ctx->fwd_rows_kept ? q.fxoff : (int64_t)-1;
    out->push_back(o);
  }
  std::sort(out->begin(), out->end(), [](const PipelineSurvivor &a, const PipelineSurvivor &b) {
    if (a.window != b.window) return a.window < b.window;
    if (a.strand != b.strand) return a.strand < b.strand;
    return a.start < b.start;
  });
  return BATH_OK;
}

// =================================================================================================
// p7_ViterbiFilter_BATH / p7_SSVFilter_BATH over a block of amino-acid targets, with their hit windows: the batched forms
// the single-target prototypes of impl_hip/ bind (the pipeline above runs the same kernels on its own candidate lists).
// =================================================================================================
namespace bath {
static int windows_out(bath_hip_ctx *ctx, const WindowRec *d_wins, const int *d_count, int cap, const bath_hmm_window **wins, int64_t *nwins) {
  int n = 0;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(&n, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n > cap) { ctx->set_error("hit-window buffer too small"); return BATH_EMEM; }
  std::vector<WindowRec> h((size_t)n);
  if (n) BATH_HIP_TRY(ctx, hipMemcpy(h.data(), d_wins, (size_t)n * sizeof(WindowRec), hipMemcpyDeviceToHost));
  // the kernels append in completion order: restore the reference's order (by target, then by position in the target)
  std::sort(h.begin(), h.end(), [](const WindowRec &a, const WindowRec &b) { return a.cand != b.cand ? a.cand < b.cand : a.n < b.n; });
  ctx->hmm_windows.resize((size_t)n);
  for (int i = 0; i < n; i++) ctx->hmm_windows[(size_t)i] = bath_hmm_window{h[(size_t)i].cand, h[(size_t)i].n, h[(size_t)i].k, h[(size_t)i].length, h[(size_t)i].score};
  *wins = ctx->hmm_windows.data(); *nwins = n;
  return BATH_OK;
}
}  // namespace bath

extern "C" int bath_hip_vitfilter_bath(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, const float *filtersc, double P,
                                       float *sc, int32_t *status, const bath_hmm_window **wins, int64_t *nwins) {
  if (!ctx || !om || !sq || !filtersc || !sc || !wins || !nwins) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  *wins = nullptr; *nwins = 0;
  const int64_t n = sq->n;
  if (n == 0) return BATH_OK;
  const int M = om->M;
  int st = om->ensure_len_tables(sq->maxlen + 1);
  if (st != BATH_OK) return st;
  const std::vector<uint8_t> ssv_scores = host_ssv_scores(om);
  const int cap = (int)std::min<int64_t>((int64_t)1 << 26, sq->total / 2 + 16 * n + 1024);      // a window ends at least one residue after the last
  DevBuf &b = ctx->scratch[Scratch::kFilterBathWork];
  // The cascade's switch (run_filters): a batch as large as the ORFs of a block of lane_min_nt() nucleotides takes the lane-per-target
  // kernel through launch_vit_sorted, on an identity work list whose count lives on the device like the cascade's; smaller ones the
  // wave-per-target kernel.  Which one ran is left as the call's one kernel span (bath_hip_kernel_times).
  const bool lane = vit_lane_supported(om) && 3 * sq->total >= lane_min_nt() && n < (int64_t)INT32_MAX;
  const size_t n_list = lane ? (size_t)n : 0;
  const size_t o_sc = 0, o_st = o_sc + (size_t)n * 4, o_f = o_st + (size_t)n * 4, o_km = o_f + (size_t)n * 4, o_todo = o_km + (size_t)n * 8, o_sorted = o_todo + n_list * 4,
               o_bins = o_sorted + n_list * 4, o_cnt = (o_bins + (lane ? 2048 * sizeof(int) : 0) + 255) / 256 * 256, o_ssv = o_cnt + 256,
               o_w = (o_ssv + ssv_scores.size() + 255) / 256 * 256, total = o_w + (size_t)cap * sizeof(WindowRec);
  BATH_HIP_TRY(ctx, b.reserve(total + 256));
  char *p = b.as<char>();
  BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_f, filtersc, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_ssv, ssv_scores.data(), ssv_scores.size(), hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemsetAsync(p + o_cnt, 0, 256, ctx->stream));
  VitWindowArgs wa{};
  wa.invP_vit = (double)(float)gumbel_invsurv(P, om->evparam[2], om->evparam[3]);          // vitfilter.c:314 (float invP)
  wa.invP_msv = (double)(float)gumbel_invsurv(P, om->evparam[0], om->evparam[1]);          // vitfilter.c:319
  wa.d_filtersc = reinterpret_cast<const float *>(p + o_f); wa.d_ssv_scores = reinterpret_cast<const uint8_t *>(p + o_ssv);
  wa.d_wins = p + o_w; wa.d_win_count = reinterpret_cast<int *>(p + o_cnt); wa.win_cap = cap; wa.d_kminmax = reinterpret_cast<int32_t *>(p + o_km);
  float *d_sc = reinterpret_cast<float *>(p + o_sc);
  int32_t *d_st = reinterpret_cast<int32_t *>(p + o_st);
  std::vector<int32_t> todo(n_list);                  // (alive until windows_out has synchronized the stream)
  const int n32 = (int)n;
  ctx->spans_reset();
  const int span = ctx->span_begin(lane ? vit_lane_kernel_name(om) : "vit_wave_kernel", ctx->stream, (double)sq->total * M, 0.0);
  if (lane) {
    for (int64_t i = 0; i < n; i++) todo[(size_t)i] = (int32_t)i;
    int *d_ntodo = reinterpret_cast<int *>(p + o_cnt) + 16;            // behind the window count, in the same zeroed 256 bytes
    BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_todo, todo.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(d_ntodo, &n32, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    st = launch_vit_sorted(ctx, om, sq->view(), reinterpret_cast<const int32_t *>(p + o_todo), n, d_ntodo, sq->d_len, reinterpret_cast<int *>(p + o_bins),
                           reinterpret_cast<int32_t *>(p + o_sorted), d_sc, d_st, &wa, nullptr);
  } else st = launch_vit_wave(ctx, om, sq->view(), nullptr, n, d_sc, d_st, &wa, nullptr);
  if (st != BATH_OK) return st;
  ctx->span_end(span, ctx->stream);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc, p + o_sc, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (status) BATH_HIP_TRY(ctx, hipMemcpyAsync(status, p + o_st, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  return windows_out(ctx, reinterpret_cast<const WindowRec *>(p + o_w), wa.d_win_count, cap, wins, nwins);
}

extern "C" int bath_hip_ssvfilter_bath(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, double P,
                                       const bath_hmm_window **wins, int64_t *nwins) {
  if (!ctx || !om || !sq || !wins || !nwins) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  *wins = nullptr; *nwins = 0;
  const int64_t n = sq->n;
  if (n == 0) return BATH_OK;
  if (n >= (int64_t)INT32_MAX) return BATH_EINVAL;
  int st = om->ensure_len_tables(sq->maxlen + 1);
  if (st != BATH_OK) return st;
  const std::vector<uint8_t> ssv_scores = host_ssv_scores(om);
  const int cap = (int)std::min<int64_t>((int64_t)1 << 26, sq->total / 2 + 16 * n + 1024);
  DevBuf &b = ctx->scratch[Scratch::kFilterBathWork];
  const size_t o_todo = 0, o_km = o_todo + (size_t)n * 4, o_ctr = (o_km + (size_t)n * 8 + 255) / 256 * 256, o_ssv = o_ctr + 256 + sizeof(Counters),
               o_w = (o_ssv + ssv_scores.size() + 255) / 256 * 256, total = o_w + (size_t)cap * sizeof(WindowRec);
  BATH_HIP_TRY(ctx, b.reserve(total + 256));
  char *p = b.as<char>();
  std::vector<int32_t> todo((size_t)n);
  for (int64_t i = 0; i < n; i++) todo[(size_t)i] = (int32_t)i;
  Counters hc{};
  hc.todo_ssvb = (int)n;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_todo, todo.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_ctr, &hc, sizeof hc, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(p + o_ssv, ssv_scores.data(), ssv_scores.size(), hipMemcpyHostToDevice, ctx->stream));
  Cand cand{};                                        // the kernel reads a target's offset and length and writes its model range
  cand.off = sq->d_off; cand.len = sq->d_len; cand.kminmax = reinterpret_cast<int32_t *>(p + o_km);
  Counters *d_ctr = reinterpret_cast<Counters *>(p + o_ctr);
  const MsvConsts mc = msv_consts(om);
  const double invP = gumbel_invsurv(P, om->evparam[0], om->evparam[1]);                   // msvfilter.c:302
  if ((st = launch_ssv_bath(ctx, ctx->stream, om, cand, d_ctr, reinterpret_cast<const int32_t *>(p + o_todo), sq->d_data, reinterpret_cast<const uint8_t *>(p + o_ssv), mc, invP,
                            reinterpret_cast<WindowRec *>(p + o_w), cap)) != BATH_OK) return st;
  return windows_out(ctx, reinterpret_cast<const WindowRec *>(p + o_w), &d_ctr->win_count, cap, wins, nwins);
}
