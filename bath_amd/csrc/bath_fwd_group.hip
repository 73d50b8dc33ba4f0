// bath_fwd_group.hip -- the Forward parser of the filter cascade with a quarter wave per target.
//
//   fwd_group_kernel    <- p7_ForwardParser / forward_engine      src/impl_sse/fwdback.c:256-463
//
// fwd_wave_kernel (bath_filters.hip) gives a target a whole wave.  At the cascade's model lengths most of what a row costs there
// does not depend on the number of nodes a lane owns: the six steps of the D scan, the sum over the wave with its broadcast, the
// special states, the residue, the rescaling test and the loop are paid per wave-row, for one target.  Here a target has the 16 lanes
// of one DPP row, C = 10 nodes a lane, and a wave advances four targets in lock step: the scan takes the four row_shr steps and
// stays inside the row, the sum is a butterfly inside the row, and everything that is paid per wave-row is paid once for four
// targets.  The cells' arithmetic is fwd_wave_kernel's, operation by operation (fwdback.c:418-434, no contraction); the D scan and
// the sum over the model associate differently, so scores agree with it within the parser's tolerance and not bit for bit.
//
// The four targets of a wave are consecutive entries of a list sorted by length, longest first, so they end within a row or two of
// each other.  The wave runs to its longest target; a group that is done computes on (on padding residues, into state nobody reads):
// its score was taken at its own last row.  Groups never exchange data, so a target's score does not depend on its neighbours.
#include <algorithm>
#include <cmath>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

namespace bath {

constexpr int kFwdGroupC = 10;          // nodes per lane: 16 lanes hold kFwdGroupMaxNodes
static_assert(16 * kFwdGroupC == kFwdGroupMaxNodes, "a group is one DPP row of 16 lanes");

template <int CTRL>
__device__ __forceinline__ float row_dpp_f32(float v, float fill) {                  // a lane without a source keeps <fill>
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// Sum over the 16 lanes of a DPP row, every lane of the row left with the total: a butterfly (quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror), one fixed association, and a + b == b + a makes the 16 results the same bits.
__device__ __forceinline__ float row_sum_f32(float v) {
  v = v + row_dpp_f32<0xb1>(v, 0.f);
  v = v + row_dpp_f32<0x4e>(v, 0.f);
  v = v + row_dpp_f32<0x141>(v, 0.f);
  v = v + row_dpp_f32<0x140>(v, 0.f);
  return v;
}

// Waves are persistent: a wave's first job is its own number, every further one the next that no wave has taken (one atomicAdd per
// wave and job on *next, which is zero when the kernel starts).  Job j is entries 4j .. 4j+3 of the sorted list, so the long targets
// start first and the short ones fill in behind them; no wave waits for, or reads anything written by, another.
template <int C>
__global__ __launch_bounds__(256) void fwd_group_kernel(SeqView sq, int M, const float *__restrict__ g_rf, const float *__restrict__ g_tf,
                                                        const float *__restrict__ pmove_tab, FwdConsts c,
                                                        const int32_t *__restrict__ sorted, int64_t ntodo, const int *__restrict__ ntodo_dev,
                                                        int *__restrict__ next, float *__restrict__ sc, int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const float *s_rf = reinterpret_cast<const float *>(lds);                      // [Kp][wave_em_stride(M)], entry node - 1; 64 C zeros behind
  const int S = wave_em_stride(M);
  if (ntodo_dev) ntodo = min(ntodo, (int64_t)*ntodo_dev);
  const int64_t njobs = (ntodo + 3) >> 2;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if (((int64_t)blockIdx.x * blockDim.x >> 6) >= njobs) return;                  // none of the block's waves has a job in any round
  wave_em_fill<C>(reinterpret_cast<float *>(lds), g_rf, M, M + 1);
  __syncthreads();
  const int lane = threadIdx.x & 63, gl = lane & 15, grp = lane >> 4;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  // the lane's transitions, once; a node beyond M has zeros, which make its cells zeros: M, I and the D it hands on
  float tMM[C], tIM[C], tDM[C], tBM[C], tMD[C], tDD[C], tMI[C], tII[C];
#pragma unroll
  for (int k = 0; k < C; k++) {
    const int node = gl * C + k + 1;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 ta = node <= M ? *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8) : z;          // MM IM DM BM
    const float4 tb = node <= M ? *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8 + 4) : z;      // MD DD MI II
    tMM[k] = ta.x; tIM[k] = ta.y; tDM[k] = ta.z; tBM[k] = ta.w; tMD[k] = tb.x; tDD[k] = tb.y; tMI[k] = tb.z; tII[k] = tb.w;
  }
  // The D chain's maps are D -> A + D * B with B a product of tDD's: B does not depend on the row, so the factor every step of the
  // scan multiplies by is computed here, once (a lane without a source sees the identity's B = 1)
  float Bs[4];
  {
    float B = 1.f;
#pragma unroll
    for (int k = 0; k < C; k++) B *= tDD[k];
    Bs[0] = B; B = B * row_dpp_f32<0x111>(B, 1.f);
    Bs[1] = B; B = B * row_dpp_f32<0x112>(B, 1.f);
    Bs[2] = B; B = B * row_dpp_f32<0x114>(B, 1.f);
    Bs[3] = B;
  }

  for (int64_t job = wid; job < njobs;) {
    const int64_t ent = 4 * job + grp;
    const bool have = ent < ntodo;
    const int64_t sid = have ? (int64_t)sorted[ent] : 0;
    const int L = have ? sq.len[sid] : 0;
    const uint8_t *s = sq.data + (have ? sq.off[sid] : 0);
    int Lmax = max(L, __builtin_amdgcn_readlane(L, 0));                          // the wave's longest: the list is sorted, but a bin holds
    Lmax = max(Lmax, __builtin_amdgcn_readlane(L, 16));                          // one length only up to the sort's last bin
    Lmax = max(Lmax, __builtin_amdgcn_readlane(L, 32));
    Lmax = __builtin_amdgcn_readfirstlane(max(Lmax, __builtin_amdgcn_readlane(L, 48)));
    const float pmove = pmove_tab[L], ploop = 1.0f - pmove;
    float Mp[C], Ip[C], Dp[C];
#pragma unroll
    for (int k = 0; k < C; k++) Mp[k] = Ip[k] = Dp[k] = 0.f;
    float xN = 1.f, xE = 0.f, xJ = 0.f, xC = 0.f, xB = pmove;
    float totscale = 0.f;
    float endC = xC, endscale = totscale;                                        // xC and totscale behind the target's last row

    // four residues a read, one address per group, the next read in flight (as vit_lane_kernel's); behind the target's end: padding
    uint32_t wnext = (0 < L) ? *reinterpret_cast<const uint32_t *>(s) : 0x1d1d1d1du;
    for (int i0 = 0; i0 < Lmax; i0 += 4) {
      uint32_t w = wnext;
      wnext = (i0 + 4 < L) ? *reinterpret_cast<const uint32_t *>(s + i0 + 4) : 0x1d1d1d1du;
#pragma unroll 1
      for (int i = i0 + 1; i <= min(i0 + 4, Lmax); i++) {
        const int x = min((int)(w & 0xffu), kKp - 1);
        w >>= 8;
        float em[C];
        wave_em_load<C>(s_rf + x * S, gl, em);
        const float mIn = row_dpp_f32<0x111>(Mp[C - 1], 0.f), iIn = row_dpp_f32<0x111>(Ip[C - 1], 0.f), dIn = row_dpp_f32<0x111>(Dp[C - 1], 0.f);
        float Mc[C], Ic[C], md[C];
        float sumE = 0.f;
#pragma unroll
        for (int k = 0; k < C; k++) {
          const float m1 = (k == 0) ? mIn : Mp[k - 1];
          const float i1 = (k == 0) ? iIn : Ip[k - 1];
          const float d1 = (k == 0) ? dIn : Dp[k - 1];
          float sv = xB * tBM[k];
          sv = sv + m1 * tMM[k];
          sv = sv + i1 * tIM[k];
          sv = sv + d1 * tDM[k];
          sv = sv * em[k];
          Mc[k] = sv;
          sumE += sv;
          md[k] = sv * tMD[k];
          Ic[k] = Mp[k] * tMI[k] + Ip[k] * tII[k];
        }
        // D(node+1) = md(node) + D(node)*tDD(node): the lane's affine map over its C nodes, then an inclusive scan over the group's 16 lanes
        float A = 0.f;
#pragma unroll
        for (int k = 0; k < C; k++) A = md[k] + A * tDD[k];
        // by DPP inside the row; a lane without a source sees the identity map's A = 0: A + 0 * B = A
        A = A + row_dpp_f32<0x111>(A, 0.f) * Bs[0];
        A = A + row_dpp_f32<0x112>(A, 0.f) * Bs[1];
        A = A + row_dpp_f32<0x114>(A, 0.f) * Bs[2];
        A = A + row_dpp_f32<0x118>(A, 0.f) * Bs[3];
        float Dc[C];
        Dc[0] = row_dpp_f32<0x111>(A, 0.f);
#pragma unroll
        for (int k = 1; k < C; k++) Dc[k] = md[k - 1] + Dc[k - 1] * tDD[k - 1];
#pragma unroll
        for (int k = 0; k < C; k++) sumE += Dc[k];
        xE = row_sum_f32(sumE);
        xN = xN * ploop;
        xC = (xC * ploop) + (xE * c.xfE_move);
        xJ = (xJ * ploop) + (xE * c.xfE_loop);
        xB = (xJ * pmove) + (xN * pmove);
        // Rescaling is a target's own: rare, so the wave takes the path only when a group that is still running needs it, and the
        // others divide by one (x / 1, x * 1 and t + 0 are exact)
        const bool rescale = i <= L && xE > 1.0e4f;
        if (__any(rescale)) {
          const float by = rescale ? xE : 1.0f;
          xN = xN / by; xC = xC / by; xJ = xJ / by; xB = xB / by;
          const float inv = (float)(1.0 / (double)by);
#pragma unroll
          for (int k = 0; k < C; k++) { Mc[k] *= inv; Dc[k] *= inv; Ic[k] *= inv; }
          totscale += (float)log((double)by);
          xE = rescale ? 1.0f : xE;
        }
        endC = (i == L) ? xC : endC;
        endscale = (i == L) ? totscale : endscale;
#pragma unroll
        for (int k = 0; k < C; k++) { Mp[k] = Mc[k]; Ip[k] = Ic[k]; Dp[k] = Dc[k]; }
      }
    }
    if (have && gl == 0) {
      if (isnan(endC) || (L > 0 && endC == 0.0f) || isinf(endC)) { sc[sid] = -INFINITY; status[sid] = BATH_ERANGE; }
      else { sc[sid] = (float)((double)endscale + log((double)(endC * pmove))); status[sid] = BATH_OK; }
    }
    int taken = 0;
    if (lane == 0) taken = atomicAdd(next, 1);
    job = nw + (int64_t)__builtin_amdgcn_readfirstlane(taken);
  }
}

bool fwd_group_supported(const bath_hip_oprofile *om) { return om->M >= 1 && om->M <= kFwdGroupMaxNodes; }

int launch_fwd_group(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_sorted, int64_t ntodo, const int *ntodo_dev, int *d_next, float *d_sc, int32_t *d_status) {
  if (ntodo == 0) return BATH_OK;
  if (!fwd_group_supported(om)) { ctx->set_error("Forward group kernel: model longer than 160 nodes"); return BATH_EINVAL; }
  constexpr int C = kFwdGroupC;
  const size_t shmem = ((size_t)kKp * wave_em_stride(om->M) + 64 * (size_t)C) * sizeof(float);
  // One block per CU, a wave per SIMD: a wave of 64 issues back to back on a SIMD's 16 lanes, so a second one (the registers allow
  // two) adds no throughput where the longest target's rows set the stage's length, and takes issue slots from the other part's SSV
  // grid beside it.  Measured on the bench block (profiles/fwd_group_ab.txt): two blocks per CU 0.19 ms as one part against 0.23,
  // the same 0.16 ms per part of a block in two parts, and the step 0.08 ms slower.
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->prop.multiProcessorCount, (ntodo + 15) / 16));
  FwdConsts c{om->xf_E[0], om->xf_E[1]};
  hipLaunchKernelGGL(fwd_group_kernel<C>, dim3(grid), dim3(256), shmem, ctx->stream, v, om->M, om->d_rf, om->d_tf, om->lt.d_pmove, c, d_sorted, ntodo, ntodo_dev,
                     d_next, d_sc, d_status);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath

// p7_ForwardParser over a block by the group kernel: every target on the list, the list sorted by length as the cascade sorts its own.
extern "C" int bath_hip_fwdparser_group(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status) {
  if (!ctx || !om || !sq || !sc) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!fwd_group_supported(om)) { ctx->set_error("bath_hip_fwdparser_group: the group kernel takes models of up to 160 nodes"); return BATH_EINVAL; }
  if (sq->n > (int64_t)INT32_MAX) { ctx->set_error("bath_hip_fwdparser_group: more than 2^31 - 1 targets"); return BATH_ERANGE; }
  int st = om->ensure_len_tables(sq->maxlen);
  if (st != BATH_OK) return st;
  const int64_t n = sq->n;
  if (n == 0) return BATH_OK;
  DevBuf &b_sc = ctx->scratch[Scratch::kStdScores], &b_st = ctx->scratch[Scratch::kStdStatus], &b_work = ctx->scratch[Scratch::kFwdGroupWork];
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * sizeof(float)));
  BATH_HIP_TRY(ctx, b_st.reserve((size_t)n * sizeof(int32_t)));
  BATH_HIP_TRY(ctx, b_work.reserve((2 * (size_t)n + 2048 + 2) * sizeof(int32_t)));       // todo[n] | sorted[n] | the sort's 2048 bins | n | the kernel's job counter
  int32_t *d_todo = b_work.as<int32_t>(), *d_sorted = d_todo + n, *d_bins = d_sorted + n, *d_n = d_bins + 2048;
  std::vector<int32_t> todo((size_t)n + 2);
  for (int64_t i = 0; i < n; i++) todo[(size_t)i] = (int32_t)i;
  todo[(size_t)n] = (int32_t)n; todo[(size_t)n + 1] = 0;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_todo, todo.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_n, &todo[(size_t)n], 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  if ((st = launch_len_sort(ctx, d_todo, d_n, sq->d_len, d_bins, d_sorted)) != BATH_OK) return st;
  if ((st = launch_fwd_group(ctx, om, sq->view(), d_sorted, n, d_n, d_n + 1, b_sc.as<float>(), b_st.as<int32_t>())) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc, b_sc.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (status) BATH_HIP_TRY(ctx, hipMemcpyAsync(status, b_st.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}
