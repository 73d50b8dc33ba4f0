// bath_std_ensemble.hip -- the standard branch's trace ensemble of multi-domain regions on the GPU (bath_hip_set_std_ensemble:
// BATH_ENSEMBLE_STREAMS_DEVICE).
//
// Reference: region_trace_ensemble (p7_domaindef.c:766-850) with p7_StochasticTrace (impl_sse/stotrace.c:71-300).  As in the
// frameshift branch (bath_fs_ensemble.hip) the serial ensemble cannot run in parallel exactly, so in the stream modes every trace
// draws from a slice of its own of the region's generator and the 200 walks of a region (bath_std_ens_walk.hpp) are 200 lanes of one
// block, reading the region's multihit Forward matrix where fwd_wave_kernel left it in device memory.  What comes back to the host,
// in one copy for all regions: per trace a status, a count, up to 8 segments and the 2-bit M / I / D codes of the steps inside
// them.  The null2 contributions (p7_Null2_ByTrace), the clustering and the significance rules stay on the host
// (bath_ensemble.hip: std_ensemble_consume), the same code for the host twin and for this kernel.
//
// Shape.  One 256-thread block per region from a longest-first job counter; lanes 0..199 walk, lanes 200..255 idle through the job
// loop's barriers.  The lanes of a wave are in different states most of the time; every state's 2- or 4-entry choice goes through one
// normalise-and-roll path (std_ens_choose), so divergent lanes share that part, and the E state (a running sum over 2M cells of
// the row) is walked by the lane itself in ascending node order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bath_fs_device.hpp"
#include "bath_std_ens_walk.hpp"

namespace bath {

static_assert(kStdEnsOutInts == kEnsSamples * (2 + kEnsMaxSeg * kStdSegInts), "per-region output record of std_ensemble_kernel");
constexpr int kStdEnsBlock = 256;

__global__ void __launch_bounds__(kStdEnsBlock)
std_ensemble_kernel(int64_t n, const int32_t *__restrict__ len, const int32_t *__restrict__ cfg_len, int M, const float *__restrict__ tf,
                    const float *__restrict__ pmove_tab, float tEL, float tEM, const float *__restrict__ fwd, const int64_t *__restrict__ foff,
                    const float *__restrict__ fx, const int64_t *__restrict__ xoff, const uint32_t *__restrict__ states, int32_t *__restrict__ out,
                    uint32_t *__restrict__ path, const int64_t *__restrict__ poff, FsJobs jobs) {
  __shared__ int64_t s_job;
  const int t = (int)threadIdx.x;
  for (;;) {
    if (t == 0) { const unsigned j = atomicAdd(jobs.counter, 1u); s_job = (int64_t)j < n ? (int64_t)jobs.order[j] : (int64_t)-1; }
    __syncthreads();
    const int64_t job = s_job;
    __syncthreads();
    if (job < 0) return;
    if (t < kEnsSamples) {                                  // (no `continue` for the other lanes: every wave meets the barriers as one)
      int32_t *o = out + (size_t)job * kStdEnsOutInts;
      int32_t ns = 0;
      int st = kEnsImpossible;                              // an empty region: no valid traces
      const int Lr = len[job];
      if (Lr >= 1 && ens_streams_fit(Lr, M))                // (outside the rule the region has no path area: the host walks it)
        st = std_ens_walk(M, tf, pmove_tab[cfg_len[job]], tEL, tEM, Lr, fwd + foff[job], fx + xoff[job], states[(size_t)job * kEnsSamples + t],
                          o + 2 * kEnsSamples + (size_t)t * kEnsMaxSeg * kStdSegInts, kEnsMaxSeg, &ns,
                          path + poff[job] + (size_t)t * std_ens_path_words(Lr, M, kEnsMaxSeg));
      o[t] = st; o[kEnsSamples + t] = ns;
    }
  }
}

// Queues, behind the regions' Forward on ctx->stream: the start states and the job list up, the kernel, everything it wrote down in
// one copy.  Once the stream is synchronized run->out / run->path are valid (page-locked).
int std_region_ensembles_device(bath_hip_ctx *ctx, const bath_hip_oprofile *om, int64_t n, const int32_t *h_len, const int32_t *d_len, const int32_t *d_cfg,
                                const float *d_fwd, const int64_t *d_foff, const float *d_fx, const int64_t *d_xoff, uint32_t seed, StdEnsRun *run) {
  if (n == 0) return BATH_OK;
  const int M = om->M;
  run->d_fwd = d_fwd; run->d_fx = d_fx;
  run->poff.assign((size_t)n + 1, 0);
  for (int64_t e = 0; e < n; e++) {
    const int Lr = h_len[e];
    const bool walked = Lr >= 1 && ens_streams_fit(Lr, M);
    if (walked) ctx->std_ens_kernel_regions++;
    const int64_t words = walked ? (int64_t)kEnsSamples * std_ens_path_words(Lr, M, kEnsMaxSeg) : 0;
    run->poff[(size_t)e + 1] = run->poff[(size_t)e] + words;
  }
  // one upload: [job counter = 0, padded to 16 words][job order, longest first: n][path offsets: 2 words each, n + 1][start states: 200 n]
  std::vector<int32_t> order;
  fs_order_by_length_desc(h_len, n, &order);
  const size_t o_order = 16, o_poff = (o_order + (size_t)n + 1) & ~(size_t)1, o_states = o_poff + 2 * ((size_t)n + 1), up_words = o_states + (size_t)n * kEnsSamples;
  std::vector<uint32_t> up(up_words, 0u);
  std::memcpy(up.data() + o_order, order.data(), (size_t)n * 4);
  std::memcpy(up.data() + o_poff, run->poff.data(), ((size_t)n + 1) * 8);
  for (int64_t e = 0; e < n; e++) fs_ensemble_start_states(seed, up.data() + o_states + (size_t)e * kEnsSamples);   // one jump-ahead per trace
  DevBuf &b_up = ctx->scratch[Scratch::kStdEnsembleUpload], &b_out = ctx->scratch[Scratch::kStdEnsembleOut];
  const size_t out_words = (size_t)n * kStdEnsOutInts + (size_t)run->poff[(size_t)n];
  BATH_HIP_TRY(ctx, b_up.reserve(up_words * 4 + 64));
  BATH_HIP_TRY(ctx, b_out.reserve(out_words * 4 + 64));
  int st;
  if ((st = ctx->stage_upload(Pinned::kStdEnsembleUpload, b_up.p, up.data(), up_words, ctx->stream)) != BATH_OK) return st;
  if (ctx->stage[Pinned::kStdEnsembleOut].reserve(out_words * 4 + 64) != hipSuccess) { ctx->set_error("cannot allocate page-locked memory for the ensembles' segments"); return BATH_EFAIL; }
  uint32_t *d_up = b_up.as<uint32_t>();
  int32_t *d_out = b_out.as<int32_t>();
  uint32_t *d_path = reinterpret_cast<uint32_t *>(d_out + (size_t)n * kStdEnsOutInts);
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)ctx->prop.multiProcessorCount * 4));
  const int s1 = ctx->span_begin("std_ensemble_kernel", ctx->stream, 0.0, 0.0);
  hipLaunchKernelGGL(std_ensemble_kernel, dim3(grid), dim3(kStdEnsBlock), 0, ctx->stream, n, d_len, d_cfg, M, om->d_tf, om->lt.d_pmove, om->xf_E[0], om->xf_E[1],
                     d_fwd, d_foff, d_fx, d_xoff, d_up + o_states, d_out, d_path, reinterpret_cast<const int64_t *>(d_up + o_poff),
                     FsJobs{reinterpret_cast<const int32_t *>(d_up + o_order), d_up});
  ctx->span_end(s1, ctx->stream);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kStdEnsembleOut].p, b_out.p, out_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  run->out = ctx->stage[Pinned::kStdEnsembleOut].as<int32_t>();
  run->path = reinterpret_cast<const uint32_t *>(run->out + (size_t)n * kStdEnsOutInts);
  return BATH_OK;
}

// A region of the device mode on the host side: its null2 scores and envelopes from what the kernel left, or by a host walk on a copy
// of its matrix where the kernel could not serve it (called from the ensembles' worker threads, after the stream's synchronize).
int std_ensemble_region_from_device(bath_hip_ctx *ctx, const StdEnsRun &run, int64_t e, const StdEnsModel &om, const uint8_t *res, int Lr,
                                    int64_t foff, int64_t xoff, uint32_t seed, std::vector<float> *n2sc, std::vector<std::pair<int, int>> *env,
                                    int *region_status, std::vector<int32_t> *segs_out, int32_t *trace_status) {
  if (Lr < 1) return std_region_ensemble_host(nullptr, BATH_ENSEMBLE_STREAMS_HOST, om, res, Lr, nullptr, nullptr, n2sc, env, seed, region_status, segs_out, trace_status);
  const int32_t *o = run.out + (size_t)e * kStdEnsOutInts;
  const bool fits = ens_streams_fit(Lr, om.M);
  bool overflow = false;
  for (int t = 0; t < kEnsSamples && fits; t++) overflow = overflow || o[t] == kEnsSegOverflow;
  if (!fits || overflow) {
    std::vector<float> f((size_t)(Lr + 1) * (size_t)(om.M + 1) * 3), x((size_t)(Lr + 1) * 6);
    if (hipSetDevice(ctx->device) != hipSuccess) return BATH_EFAIL;
    if (hipMemcpy(f.data(), run.d_fwd + foff, f.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return BATH_EFAIL;
    if (hipMemcpy(x.data(), run.d_fx + xoff, x.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return BATH_EFAIL;
    if (fits) ctx->std_ens_twin_fallbacks++;                 // a region is counted once: here, or by the host walk as one for the serial ensemble
    return std_region_ensemble_host(fits ? nullptr : ctx, BATH_ENSEMBLE_STREAMS_HOST, om, res, Lr, f.data(), x.data(), n2sc, env, seed, region_status, segs_out, trace_status);
  }
  if (trace_status) std::copy(o, o + kEnsSamples, trace_status);
  const int rs = std_ensemble_consume(om, res, Lr, o, o + kEnsSamples, o + 2 * kEnsSamples, kEnsMaxSeg, run.path + run.poff[(size_t)e], n2sc, env, segs_out);
  if (rs < 0) return rs;
  if (region_status) *region_status = rs;
  return BATH_OK;
}

}  // namespace bath
