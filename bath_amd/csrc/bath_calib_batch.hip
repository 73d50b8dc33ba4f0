// bath_calib_batch.hip -- one standard sample set against several models per launch: the three standard filters of a batch of
// models under calibration (bath_hip_calibrate_batch, bath_calibrate.hip).
//
//   msv_wave_batch_kernel <- msv_wave_kernel's text (bath_msv_wave_rows.hpp)
//   vit_wave_batch_kernel <- vit_wave_kernel's text (bath_vit_wave_rows.hpp), no window outputs
//   fwd_wave_batch_kernel <- fwd_wave_kernel's text (bath_fwd_wave_rows.hpp), score only
//
// A builder that reseeds its generator for every model scores the same N sampled sequences against every model.  One model's N
// targets are N waves, a fraction of the chip; a batch's models are independent.  So the grid is (blocks over the set's targets,
// models of this tiling): a block reads its model's StdBatchModel from a device array at blockIdx.y, stages that model's rows into
// LDS once, and its waves take targets of the shared set, as the frameshift batch kernels do (bath_fs_chain.hip).  No block waits
// for another and nothing passes between workgroups.  Every target's arithmetic is the single-model kernel's own source, included
// as text, so a score depends on nothing but its model and its target: the batch equals the serial calls bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

namespace bath {

// what the three single-model kernels take as arguments, per model
struct StdBatchModel {
  int M, rb_stride;
  const uint8_t *rb, *tjb_tab;                 // MSV: byte costs [Kp][rb_stride], tJB by length
  const int16_t *rw, *tw, *xwmove_tab;         // Viterbi: word emissions [Kp][M+1], transitions [M+1][8], N/J/C move by length
  const float *rf, *tf, *pmove_tab;            // Forward: odds emissions [Kp][M+1], transitions [M+1][8], pmove by length
  MsvConsts mc;
  VitConsts vc;
  FwdConsts fc;
  float *sc[3];                                // MSV, Viterbi, Forward: a score and a status per target of that filter's set
  int32_t *status[3];
};

template <int C>
__global__ __launch_bounds__(256) void msv_wave_batch_kernel(SeqView sq, const StdBatchModel *__restrict__ models) {
  const StdBatchModel &m = models[blockIdx.y];
  const int M = m.M, rb_stride = m.rb_stride;
  const uint8_t *__restrict__ rb = m.rb, *__restrict__ tjb_tab = m.tjb_tab;
  const MsvConsts c = m.mc;
  const int32_t *todo = nullptr;
  int64_t ntodo = sq.n;
  const int *ntodo_dev = nullptr;
  float *__restrict__ sc = m.sc[0];
  int32_t *__restrict__ status = m.status[0];
#include "bath_msv_wave_rows.hpp"
}

template <int C>
__global__ __launch_bounds__(256) void vit_wave_batch_kernel(SeqView sq, const StdBatchModel *__restrict__ models) {
  const StdBatchModel &m = models[blockIdx.y];
  const int M = m.M;
  const int16_t *__restrict__ g_rw = m.rw, *__restrict__ g_tw = m.tw, *__restrict__ xwmove_tab = m.xwmove_tab;
  const uint8_t *__restrict__ tjb_tab = m.tjb_tab;
  const VitConsts c = m.vc;
  const int32_t *todo = nullptr;
  int64_t ntodo = sq.n;
  const int *ntodo_dev = nullptr;
  float *__restrict__ sc = m.sc[1];
  int32_t *__restrict__ status = m.status[1];
  const float *filtersc = nullptr; const uint8_t *ssv_scores = nullptr;              // plain p7_ViterbiFilter: no windows
  WindowRec *wins = nullptr; int *win_count = nullptr; const int win_cap = 0; int32_t *kminmax = nullptr;
#include "bath_vit_wave_rows.hpp"
}

template <int C, bool GT>
__global__ __launch_bounds__(256) void fwd_wave_batch_kernel(SeqView sq, const StdBatchModel *__restrict__ models) {
  const StdBatchModel &m = models[blockIdx.y];
  const int M = m.M;
  const float *__restrict__ g_rf = m.rf, *__restrict__ g_tf = m.tf, *__restrict__ pmove_tab = m.pmove_tab;
  const FwdConsts c = m.fc;
  const int32_t *todo = nullptr;
  int64_t ntodo = sq.n;
  const int *ntodo_dev = nullptr;
  float *__restrict__ sc = m.sc[2];
  int32_t *__restrict__ status = m.status[2];
  float *xmx = nullptr; const int64_t *xmx_off = nullptr; float *dp = nullptr; const int64_t *dp_off = nullptr;   // the score alone
  const int unihit = 0; const int32_t *cfg_len = nullptr;
#include "bath_fwd_wave_rows.hpp"
}

size_t std_batch_model_bytes() { return sizeof(StdBatchModel); }

void std_batch_model_fill(void *dst, const bath_hip_oprofile *om, float *const d_sc[3], int32_t *const d_status[3]) {
  StdBatchModel m{};
  m.M = om->M; m.rb_stride = om->rb_stride;
  m.rb = om->d_rb; m.tjb_tab = om->lt.d_tjb;
  m.rw = om->d_rw; m.tw = om->d_tw; m.xwmove_tab = om->lt.d_xwmove;
  m.rf = om->d_rf; m.tf = om->d_tf; m.pmove_tab = om->lt.d_pmove;
  m.mc = msv_consts(om); m.vc = vit_consts(om); m.fc = FwdConsts{om->xf_E[0], om->xf_E[1]};
  for (int s = 0; s < 3; s++) { m.sc[s] = d_sc[s]; m.status[s] = d_status[s]; }
  std::memcpy(dst, &m, sizeof m);
}

int launch_std_wave_batch(bath_hip_ctx *ctx, hipStream_t stream, int filter, const void *d_models, int n_models, int Mmax, int Cv, bool gt, SeqView v) {
  if (n_models < 1 || v.n < 1) return BATH_OK;
  if (filter < 0 || filter > 2 || Cv != BATH_TILING_PICK(BATH_WAVE_COLUMNS, Mmax)) { ctx->set_error("calibrate_batch: a launch holds the models of one tiling"); return BATH_EINVAL; }
  const StdBatchModel *dm = static_cast<const StdBatchModel *>(d_models);
  // blocks of four waves over the set, as the single-model launchers (a set of a few hundred targets never reaches their cap);
  // the dynamic LDS is the longest model's: a shorter model's block lays out its own rows in less of it
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((v.n + 3) / 4, (int64_t)ctx->prop.multiProcessorCount * 8)), (unsigned)n_models);
#define BATH_CB_SWITCH(...) BATH_TILING_SWITCH(BATH_WAVE_COLUMNS, Cv, { ctx->set_error("calibrate_batch: model too long for the wave kernels"); return BATH_EINVAL; }, __VA_ARGS__)
  if (filter == 0) {
    BATH_CB_SWITCH(hipLaunchKernelGGL(msv_wave_batch_kernel<CC>, grid, dim3(256), 0, stream, v, dm);)
  } else if (filter == 1) {
    const size_t shmem = ((size_t)kKp * vit_em_stride(Mmax) + 64 * (size_t)Cv) * sizeof(int16_t);
    BATH_CB_SWITCH({
      if (shmem > 64 * 1024) BATH_HIP_TRY(ctx, bath::allow_max_lds((const void *)vit_wave_batch_kernel<CC>));
      hipLaunchKernelGGL(vit_wave_batch_kernel<CC>, grid, dim3(256), shmem, stream, v, dm);
    })
  } else if (gt) {
    BATH_CB_SWITCH(hipLaunchKernelGGL((fwd_wave_batch_kernel<CC, true>), grid, dim3(256), 0, stream, v, dm);)
  } else {
    const size_t shmem = ((size_t)kKp * wave_em_stride(Mmax) + 64 * (size_t)Cv) * sizeof(float);
    if (shmem > kWaveTableLdsMax) { ctx->set_error("calibrate_batch: a Forward launch holds models on one side of the global-table threshold"); return BATH_EINVAL; }
    BATH_CB_SWITCH({
      if (shmem > 64 * 1024) BATH_HIP_TRY(ctx, bath::allow_max_lds((const void *)(fwd_wave_batch_kernel<CC, false>)));
      hipLaunchKernelGGL((fwd_wave_batch_kernel<CC, false>), grid, dim3(256), shmem, stream, v, dm);
    })
  }
#undef BATH_CB_SWITCH
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath
