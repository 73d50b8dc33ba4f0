// bath_msv_lane.hip -- p7_MSVFilter's full recurrence (J state) with ONE LANE per target.
//
//   msv_lane_kernel <- p7_MSVFilter, the path after SSV returns eslENORESULT   impl_sse/msvfilter.c:106-207
//
// Every ORF that passes the F1 threshold scores above the point where p7_SSVFilter can vouch for its answer (xJ > base,
// ssvfilter.c:916), so ALL of the cascade's MSV survivors -- 576 k ORFs per 10^6 windows on the bench block -- are re-scored with
// the J state.  Rounds 1-3 did that with a wave per target (msv_wave_kernel: lanes own nodes, the row maximum is a wave
// reduction, 41 rows x ~0.6 us per target): 1.5 ms of an 10.9 ms step for 2 % of the cascade's cells.  But the MSV row has no
// dependency along the model either -- cell k reads cell k-1 of the PREVIOUS row; xE, xJ, xB are per-row scalars of the target --
// so the SSV kernel's layout applies: a lane keeps the whole row in registers, two cells per register (register r: nodes r+1 and
// NR+r+1, the diagonal shift folded into the in-place descending update), costs from an LDS table by residue, no cross-lane
// traffic.  Same number system (bath_kernels.hpp): a byte b of the reference is the binary16 number b * 2^-11, exact, and
// v_pk_add_f16 ... clamp saturates below at 0 like subs_epu8.  Per register and row: v_pk_max_f16 (the cell to the left or B),
// v_pk_add_f16 clamp (+ bias - cost), half a v_pk_maximum3_f16 (the row maximum).
// The reference saturates twice per cell, adds_epu8(sv, bias) at 255 and subs_epu8(., rsc) at 0 (msvfilter.c:160-162).  The upper
// saturation cannot act before the row's overflow test fires: every cell and B of the previous row satisfy v + bias < 255
// (that test, :172; base + bias < 255 by construction of the byte scores), so max(prev, B) + bias < 255 and one add of
// (bias - cost) with the lower clamp is the reference's arithmetic; a target whose row maximum reaches 255 - bias reports
// eslERANGE (score +inf) whatever its cells hold afterwards.
#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

namespace bath {

template <int NR>
__global__ __launch_bounds__(256, NR <= 76 ? 4 : 1) void msv_lane_kernel(SeqView sq, const int16_t *__restrict__ cost_tab /* the MSV increment table */, int row_bytes,
                                                                        const uint8_t *__restrict__ tjb_tab, MsvConsts c,
                                                                        const int32_t *__restrict__ todo, int64_t ntodo, const int *__restrict__ ntodo_dev,
                                                                        float *__restrict__ sc, int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  {
    const int n32 = kSsvRows * row_bytes / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(cost_tab);
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    for (int i = threadIdx.x; i < n32; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  if (ntodo_dev) ntodo = *ntodo_dev;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w * 64 < ntodo; w += nwaves) {
    const int64_t job = w * 64 + lane;
    const bool live = job < ntodo;
    const int64_t sid = live ? (todo ? (int64_t)todo[job] : job) : 0;
    const int L = live ? sq.len[sid] : 0;
    const uint8_t *s = sq.data + sq.off[sid];
    const int Lw = wave_max_i32(L);
    const int tjb = tjb_tab[L];
    const int tjbm = (uint8_t)((int8_t)tjb + (int8_t)c.tbm);
    bool overflow = false;
    const int xJ = msv_lane_rows<NR>(lds, row_bytes, s, L, Lw, tjbm, c, &overflow);
    if (live) {
      if (overflow) { sc[sid] = INFINITY; status[sid] = BATH_ERANGE; }
      else { sc[sid] = msv_lane_score(xJ, tjb, c); status[sid] = BATH_OK; }
    }
  }
}

// The lane-per-target MSV for models that fit one lane's tile of at most 76 registers (152 nodes); longer models and
// BATH_HIP_MSV_WAVE=1 keep the wave-per-target kernel.  The same condition admits the cascade's fused MSV stage (msv_stage_kernel,
// bath_pipeline.hip), which runs this kernel's rows between the SSV classification and the F1 / bias decisions of a candidate.
// launch_msv_lane returns BATH_ENORESULT when the kernel does not apply.
bool msv_stage_supported(const bath_hip_oprofile *om) {
  static const bool off = [] { const char *e = std::getenv("BATH_HIP_MSV_WAVE"); return e && e[0] == '1'; }();
  if (off || om->G != 1 || om->NR > BATH_TILING_MAX(BATH_MSV_LANE_NR) || !om->d_msv) return false;
  return true;
}

int launch_msv_lane(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, const int32_t *d_todo, int64_t ntodo, float *d_sc, int32_t *d_status, const int *ntodo_dev) {
  if (!msv_stage_supported(om)) return BATH_ENORESULT;
  if (ntodo == 0) return BATH_OK;
  const size_t shmem = (size_t)kSsvRows * om->ssv_row_bytes;
  const int64_t waves = (ntodo + 63) / 64;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)ctx->prop.multiProcessorCount * 4));
  bool launched = false;
#define BATH_MSV_CASE(N, ...)                                                                                                          \
  if (!launched && om->NR == N) {                                                                                                      \
    hipLaunchKernelGGL((msv_lane_kernel<N>), dim3(grid), dim3(256), shmem, ctx->stream, v, om->d_msv, om->ssv_row_bytes, om->lt.d_tjb,   \
                       MsvConsts{om->tbm_b, om->tec_b, om->base_b, om->bias_b, om->scale_b}, d_todo, ntodo, ntodo_dev, d_sc, d_status); \
    launched = true;                                                                                                                   \
  }
  BATH_MSV_LANE_NR(BATH_MSV_CASE)
#undef BATH_MSV_CASE
  if (!launched) return BATH_ENORESULT;
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath
