// bath_fs_ensemble.hip -- the frameshift branch's trace ensemble of multi-domain regions on the GPU (BATH_ENSEMBLE_STREAMS_DEVICE).
//
// Reference: region_trace_ensemble_frameshift (p7_domaindef.c:891-958) with p7_StochasticTrace_Frameshift
// (generic_stotrace_frameshift.c:40-215).  The serial ensemble (bath_ensemble.hip) cannot run in parallel exactly: trace t starts
// where trace t-1 stopped drawing.  In the stream modes every trace draws from a slice of its own of the region's generator
// (bath_fs_ens_walk.hpp), so the 200 walks of a region are 200 lanes of one block, reading the region's multihit Forward matrix
// where fs5_fwd_chain / fs5_fwd_kernel / fs5_fwd_odds_kernel<C, true> left it in device memory.  What comes back to the host is a
// status, a count and up to 8 segments per trace; clustering (cluster_segments, unchanged) stays on the host.
//
// Shape.  One 256-thread block per region from a longest-first job counter; lanes 0..199 walk, lanes 200..255 idle through the
// job loop's barriers.  The lanes of a wave are in different states most of the time: the walk is a chain of dependent loads with a
// few hundred flops between them, and a wave executes the union of its lanes' paths.  That is accepted -- the alternative is a
// host core per region.  The E state (a normalisation over 2M + 1 cells) is done by the lane itself, streaming the row once per sum
// in ascending index, so its floats are the serial order's; lanes of a wave that sit in E at the same time run it together.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bath_fs_device.hpp"
#include "bath_fs_ens_walk.hpp"

namespace bath {

static_assert(kFsEnsOutInts == kEnsSamples * (2 + kEnsMaxSeg * 4), "per-region output record of fs_ensemble_kernel");
constexpr int kEnsBlock = 256;

__global__ void __launch_bounds__(kEnsBlock)
fs_ensemble_kernel(int64_t n, const int32_t *__restrict__ len, int M, const float *__restrict__ tsc, float xNL, float xNM, float xE,
                   const float *__restrict__ fwd, const int64_t *__restrict__ foff, const float *__restrict__ fx, const int64_t *__restrict__ xoff,
                   const float *__restrict__ sc, const uint32_t *__restrict__ states, int32_t *__restrict__ out, FsJobs jobs) {
  __shared__ int64_t s_job;
  const int t = (int)threadIdx.x;
  for (;;) {
    if (t == 0) { const unsigned j = atomicAdd(jobs.counter, 1u); s_job = (int64_t)j < n ? (int64_t)jobs.order[j] : (int64_t)-1; }
    __syncthreads();
    const int64_t job = s_job;
    __syncthreads();
    if (job < 0) return;
    if (t < kEnsSamples) {                                  // (no `continue` for the other lanes: every wave meets the barriers as one)
      int32_t *o = out + (size_t)job * kFsEnsOutInts;
      int32_t ns = 0;
      int st = kEnsImpossible;                              // Forward underflow: no valid traces (p7_domaindef.c:413)
      const int Lr = len[job];
      if (sc[job] > -INFINITY && Lr >= 1 && ens_streams_fit(Lr, M))
        st = ens_walk(M, tsc, xNL, xNM, xE, Lr, fwd + foff[job], fx + xoff[job], states[(size_t)job * kEnsSamples + t],
                      o + 2 * kEnsSamples + (size_t)t * kEnsMaxSeg * 4, kEnsMaxSeg, &ns);
      o[t] = st; o[kEnsSamples + t] = ns;
    }
  }
}

int fs5_region_ensembles_device(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino, uint32_t seed,
                                float xNL, float xNM, float xE, FsEnsRun *run) {
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  if (!om->d_tsc) { ctx->set_error("5-codon profile without its device transitions"); return BATH_EINVAL; }
  const float *unused_f = nullptr, *unused_x = nullptr;
  std::vector<float> unused_sc;
  int st = fs5_region_forward(ctx, om, dna, cfg_len_amino, &unused_f, &run->foff, &unused_x, &run->xoff, &unused_sc, nullptr, nullptr, &run->dev);
  if (st != BATH_OK) return st;
  // start states: one jump-ahead per trace, on the host (200 x 32 multiplications per region)
  std::vector<uint32_t> states((size_t)n * kEnsSamples);
  for (int64_t e = 0; e < n; e++) fs_ensemble_start_states(seed, states.data() + (size_t)e * kEnsSamples);
  DevBuf &b_states = ctx->scratch[Scratch::kFsEnsembleStates], &b_out = ctx->scratch[Scratch::kFsEnsembleOut];
  BATH_HIP_TRY(ctx, b_states.reserve(states.size() * sizeof(uint32_t) + 64));
  BATH_HIP_TRY(ctx, b_out.reserve((size_t)n * kFsEnsOutInts * sizeof(int32_t) + 64));
  if ((st = ctx->stage_upload(Pinned::kFsEnsembleStates, b_states.p, states.data(), states.size(), ctx->stream)) != BATH_OK) return st;
  const size_t out_bytes = (size_t)n * kFsEnsOutInts * sizeof(int32_t);
  if (ctx->stage[Pinned::kFsEnsembleOut].reserve(out_bytes + (size_t)n * sizeof(float) + 64) != hipSuccess) { ctx->set_error("cannot allocate page-locked memory for the ensembles' segments"); return BATH_EFAIL; }
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)ctx->prop.multiProcessorCount * 4));
  const double cells = (double)(run->foff[(size_t)n] / 8);
  const int s1 = ctx->span_begin("fs_ensemble_kernel", ctx->stream, cells, 0.0);
  hipLaunchKernelGGL(fs_ensemble_kernel, dim3(grid), dim3(kEnsBlock), 0, ctx->stream, n, dna->d_len, om->M, om->d_tsc, xNL, xNM, xE, run->dev.d_fwd, run->dev.d_foff,
                     run->dev.d_fx, run->dev.d_xoff, run->dev.d_sc, b_states.as<uint32_t>(), b_out.as<int32_t>(), FsJobs{run->dev.job_order, run->dev.job_counter});
  ctx->span_end(s1, ctx->stream);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsEnsembleOut].p, b_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsEnsembleOut].as<char>() + out_bytes, run->dev.d_sc, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  run->out = ctx->stage[Pinned::kFsEnsembleOut].as<int32_t>();
  run->sc = reinterpret_cast<const float *>(ctx->stage[Pinned::kFsEnsembleOut].as<char>() + out_bytes);
  ctx->fs_ens_bytes_kept += (int64_t)(run->foff[(size_t)n] + run->xoff[(size_t)n]) * 4;
  return BATH_OK;
}

// one region's matrix and rows from device memory (the stream is synchronized first): the regions that fall back to a host walk
int fs_ensemble_fetch_region(bath_hip_ctx *ctx, const FsEnsRun &run, int64_t e, std::vector<float> *fwd, std::vector<float> *fx) {
  const size_t nf = (size_t)(run.foff[(size_t)e + 1] - run.foff[(size_t)e]), nx = (size_t)(run.xoff[(size_t)e + 1] - run.xoff[(size_t)e]);
  fwd->resize(nf); fx->resize(nx);
  if (hipSetDevice(ctx->device) != hipSuccess) return BATH_EFAIL;             // (called from the ensembles' worker threads)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return BATH_EFAIL;
  if (hipMemcpy(fwd->data(), run.dev.d_fwd + run.foff[(size_t)e], nf * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return BATH_EFAIL;
  if (hipMemcpy(fx->data(), run.dev.d_fx + run.xoff[(size_t)e], nx * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return BATH_EFAIL;
  return BATH_OK;
}

// A region of the device mode on the host side: its envelopes from what the kernel left, or by a host walk where the kernel could
// not serve it.  env in window coordinates (ireg); segs_out / trace_status as fs_region_ensemble_host's.
int fs_ensemble_region_from_device(bath_hip_ctx *ctx, bath_hip_ctx *counters, const FsEnsRun &run, int64_t e, int M, const float *tsc, float xNL, float xNM, float xE,
                                   int ireg, int Lr, uint32_t seed, std::vector<std::pair<int, int>> *env, int *region_status,
                                   std::vector<int32_t> *segs_out, int32_t *trace_status) {
  env->clear();
  if (segs_out) segs_out->clear();
  if (trace_status) std::fill(trace_status, trace_status + kEnsSamples, 0);
  if (region_status) *region_status = kEnsRegionNoTraces;
  if (!(run.sc[e] > -INFINITY)) { if (trace_status) std::fill(trace_status, trace_status + kEnsSamples, (int32_t)kEnsImpossible); return BATH_OK; }
  const int32_t *o = run.out + (size_t)e * kFsEnsOutInts;
  bool overflow = false;
  for (int t = 0; t < kEnsSamples; t++) overflow = overflow || o[t] == kEnsSegOverflow;
  if (!ens_streams_fit(Lr, M) || overflow) {
    std::vector<float> f, x;
    if (fs_ensemble_fetch_region(ctx, run, e, &f, &x) != BATH_OK) return BATH_EFAIL;
    const bool fits = ens_streams_fit(Lr, M);                // a region is counted once: here as overflow, or by the host walk as outside the rule
    if (fits) counters->fs_ens_overflow_fallbacks++;
    return fs_region_ensemble_host(fits ? nullptr : counters, BATH_ENSEMBLE_STREAMS_HOST, M, tsc, xNL, xNM, xE, ireg, Lr, f.data(), x.data(), env, seed, region_status, segs_out, trace_status);
  }
  if (trace_status) std::copy(o, o + kEnsSamples, trace_status);
  const int rs = fs_ensemble_consume(o, o + kEnsSamples, o + 2 * kEnsSamples, kEnsMaxSeg, ireg, env, segs_out);
  if (region_status) *region_status = rs;
  return BATH_OK;
}

}  // namespace bath

extern "C" int bath_hip_fs5_region_ensembles(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, uint32_t seed,
                                             int32_t *region_status, int32_t *trace_status, int32_t *seg, int64_t max_seg, int64_t *seg_off,
                                             int32_t *env, int64_t max_env, int64_t *env_off) {
  using namespace bath;
  if (!ctx || !om || !dna || !region_status || !seg_off || !env_off || max_seg < 0 || max_env < 0 || (max_seg > 0 && !seg) || (max_env > 0 && !env) || om->codon_lengths != 5) {
    if (ctx) ctx->set_error("bath_hip_fs5_region_ensembles: needs a 5-codon profile and its output arrays");
    return BATH_EINVAL;
  }
  if (fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n = dna->n;
  seg_off[0] = 0; env_off[0] = 0;
  if (n == 0) return BATH_OK;
  const int M = om->M, mode = ctx->fs_ensemble;
  const FsHostTables h5 = fsprofile_host(om);
  const float pm = (2.0f + 1.0f) / (100.0f + 2.0f + 1.0f);                    // p7_fs_ReconfigLength(L = 100), multihit: as the domain stage
  const float xNL = (float)std::log((double)(1.0f - pm)), xNM = (float)std::log((double)pm), xE = (float)-0.69314718055994529;
  const float *h_f = nullptr, *h_x = nullptr;
  std::vector<int64_t> foff, xoff;
  std::vector<float> h_sc;
  FsEnsRun run;
  int st;
  if (mode == BATH_ENSEMBLE_STREAMS_DEVICE) {
    if ((st = fs5_region_ensembles_device(ctx, om, dna, 100, seed, xNL, xNM, xE, &run)) != BATH_OK) return st;
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else if ((st = fs5_region_forward(ctx, om, dna, 100, &h_f, &foff, &h_x, &xoff, &h_sc, nullptr, nullptr)) != BATH_OK) return st;
  std::vector<std::pair<int, int>> cl;
  std::vector<int32_t> segs;
  int64_t nseg = 0, nenv = 0;
  for (int64_t e = 0; e < n; e++) {
    const int Lr = dna->h_len[(size_t)e];
    int rs = kEnsRegionNoTraces;
    int32_t *ts = trace_status ? trace_status + (size_t)e * kEnsSamples : nullptr;
    cl.clear(); segs.clear();
    if (mode == BATH_ENSEMBLE_STREAMS_DEVICE) {
      if ((st = fs_ensemble_region_from_device(ctx, ctx, run, e, M, h5.tsc, xNL, xNM, xE, 1, Lr, seed, &cl, &rs, &segs, ts)) != BATH_OK) { ctx->set_error("region ensemble failed"); return st; }
    } else if (h_sc[(size_t)e] > -INFINITY && Lr >= 1) {
      if ((st = fs_region_ensemble_host(ctx, mode, M, h5.tsc, xNL, xNM, xE, 1, Lr, h_f + foff[(size_t)e], h_x + xoff[(size_t)e], &cl, seed, &rs, &segs, ts)) != BATH_OK) { ctx->set_error("region ensemble failed"); return st; }
    } else if (ts) std::fill(ts, ts + kEnsSamples, mode == BATH_ENSEMBLE_SERIAL ? 0 : (int32_t)kEnsImpossible);
    region_status[e] = rs;
    for (size_t q = 0; q + 5 <= segs.size(); q += 5, nseg++) if (nseg < max_seg) std::memcpy(seg + nseg * 5, segs.data() + q, 5 * sizeof(int32_t));
    for (const auto &c : cl) { if (nenv < max_env) { env[nenv * 2] = c.first; env[nenv * 2 + 1] = c.second; } nenv++; }
    seg_off[e + 1] = nseg; env_off[e + 1] = nenv;
  }
  if (nseg > max_seg || nenv > max_env) { ctx->set_error("bath_hip_fs5_region_ensembles: output arrays too small"); return BATH_ERANGE; }
  return BATH_OK;
}
