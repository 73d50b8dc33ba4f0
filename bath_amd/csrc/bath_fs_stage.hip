// bath_fs_stage.hip -- the frameshift stage between the filter cascade and the domain stage, up to the branch decision.
//
// It takes the cascade's F4 survivors and their hit windows (filters_with_survivors, bath_pipeline.hip), has the DNA windows built
// (bath_fs_windows.hip), copies them into a pool, runs their bias filter beside the 3-codon frameshift Forward or the region stage
// (bath_frameshift.hip) and leaves the branch decision to fs_decide (bath_fs_windows.hip).  fs_gather_view is also the domain
// stage's way of gathering envelopes (bath_domaindef.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

// =================================================================================================
// Frameshift stage: p7_pli_BuildDNAWindows + p7_pli_Frameshift up to the branch decision
// (p7_pipeline.c:462-572, 1339-1470).  The ORFs that passed F4 are few (10^-4 of all ORFs): window building is
// the reference's own serial logic on the host; the DNA windows' bias filter and 3-codon frameshift Forward run
// on the GPU, batched over all windows of the block.
// =================================================================================================
namespace bath {


// copy each window out of its sequence, reverse-complemented for the bottom strand
__global__ void fs_window_gather_kernel(const uint8_t *__restrict__ dna, const FsWinDev *__restrict__ wins, int nw, const uint8_t *__restrict__ comp,
                                        uint8_t *__restrict__ pool) {
  for (int w = blockIdx.x; w < nw; w += gridDim.x) {
    const FsWinDev d = wins[w];
    const uint8_t *src = dna + d.src_off;
    uint8_t *dst = pool + d.dst_off;
    for (int i = threadIdx.x; i < d.len; i += blockDim.x) {
      const int r = d.start - 1 + i;                     // 0-based position on the strand being read
      dst[i] = d.strand ? comp[min((int)src[d.seq_n - 1 - r], 17)] : src[r];
    }
  }
}

// p7_bg_fs_FilterScore (p7_bg.c:522-561) without its length term: esl_hmm_Forward of the 2-state filter HMM over the
// canonical residues of each of the three frames.  Lane per (window, pass): pass 0 uses the model's composition,
// pass 1 the local composition of nodes kmin..kmax (p7_pli_ComputeLocalCompo).  out[(w*2+pass)*3 + frame].
__global__ void fs_bias_kernel(const uint8_t *__restrict__ pool, const FsWinDev *__restrict__ wins, int nw, const uint8_t *__restrict__ aa_full, int M,
                               const float *__restrict__ eo_global, const uint8_t *__restrict__ ssv_scores, int base_b, float scale_b,
                               const float *__restrict__ bgf, float *__restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * nw) return;
  const int w = t >> 1, pass = t & 1;
  const FsWinDev d = wins[w];
  float eo_local[2 * kKp];
  const float *e = eo_global;
  if (pass == 1) {
    if (d.kmin > d.kmax) { out[t * 3] = out[t * 3 + 1] = out[t * 3 + 2] = -INFINITY; return; }
    local_compo_eo(ssv_scores, M, base_b, scale_b, bgf, d.kmin, d.kmax, eo_local);
    e = eo_local;
  }
  const uint8_t *s = pool + d.dst_off;
  const int L = d.len, L3 = L / 3;
  const float p1 = (float)L3 / (float)(L3 + 1);                             // p7_bg_SetLength(bg, length/3), p7_bg.c:193
  const float L1 = (float)M / 8.0f;
  const float t00 = p1, t01 = 1.0f - p1, t10 = 1.0f / (L1 + 1.0f), t11 = L1 / (L1 + 1.0f);
  for (int f = 0; f < 3; f++) {
    float logsc = 0.0f, d0 = 0.f, d1 = 0.f;
    int cnt = 0;
    for (int i = f; i + 2 < L; i += 3) {
      const int a = min((int)s[i], 17), b = min((int)s[i + 1], 17), c = min((int)s[i + 2], 17);
      const int x = aa_full[(a * 18 + b) * 18 + c];
      if (x >= 20) continue;                                                // esl_abc_XIsCanonical
      float n0, n1;
      if (cnt == 0) { n0 = e[2 * x] * 0.999f; n1 = e[2 * x + 1] * 0.001f; }
      else {
        n0 = 0.0f + d0 * t00; n0 = n0 + d1 * t10; n0 *= e[2 * x];
        n1 = 0.0f + d0 * t01; n1 = n1 + d1 * t11; n1 *= e[2 * x + 1];
      }
      const float mx = fmaxf(fmaxf(n0, 0.0f), n1);
      d0 = n0 / mx; d1 = n1 / mx;
      logsc += (float)log((double)mx);
      cnt++;
    }
    if (cnt == 0) logsc = -INFINITY;                                         // esl_hmm_Forward, L = 0: log(pi[M]) = log 0
    else { float end = 0.0f + d0 * 1.0f; end = end + d1 * 1.0f; logsc += (float)log((double)end); }
    out[t * 3 + f] = logsc;
  }
}

// Copies the regions described by <regs> (dst_off is filled in here) into one pool on the device, reverse-complemented
// for the bottom strand, and returns a sequence-block view of the pool (borrowed pointers: clear them before <view> dies).
int fs_gather_view(bath_hip_ctx *ctx, const bath_hip_seqs *dna, std::vector<FsWinDev> &regs, const uint8_t *d_comp, bath_hip_seqs *view, const FsWinDev **d_desc_out) {
  const int nw = (int)regs.size();
  int64_t pool_bytes = 0;
  for (FsWinDev &d : regs) { d.dst_off = pool_bytes; pool_bytes += ((int64_t)d.len + 15) / 16 * 16 + 16; }
  DevBuf &b_pool = ctx->scratch[Scratch::kFsGatherPool], &b_desc = ctx->scratch[Scratch::kFsGatherDesc];
  BATH_HIP_TRY(ctx, b_pool.reserve((size_t)pool_bytes + 256));
  const size_t desc_bytes = ((size_t)nw * sizeof(FsWinDev) + 255) / 256 * 256;
  BATH_HIP_TRY(ctx, b_desc.reserve(desc_bytes + (size_t)nw * 12 + 64));          // descriptors, then the view's off[] and len[]
  BATH_HIP_TRY(ctx, hipMemsetAsync(b_pool.p, 0x1d, (size_t)pool_bytes + 256, ctx->stream));
  FsWinDev *d_desc = b_desc.as<FsWinDev>();
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_desc, regs.data(), (size_t)nw * sizeof(FsWinDev), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(fs_window_gather_kernel, dim3((unsigned)std::max(1, std::min(nw, 65535))), dim3(256), 0, ctx->stream, dna->d_data, d_desc, nw, d_comp, b_pool.as<uint8_t>());
  BATH_HIP_TRY(ctx, hipGetLastError());
  view->ctx = ctx; view->n = nw; view->d_data = b_pool.as<uint8_t>(); view->is_part = true;
  view->h_off.resize((size_t)nw); view->h_len.resize((size_t)nw);
  view->maxlen = 0; view->total = 0;
  for (int i = 0; i < nw; i++) {
    view->h_off[(size_t)i] = regs[(size_t)i].dst_off; view->h_len[(size_t)i] = regs[(size_t)i].len;
    view->maxlen = std::max(view->maxlen, regs[(size_t)i].len); view->total += regs[(size_t)i].len;
  }
  view->total_aligned = pool_bytes;
  int64_t *d_voff = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(d_desc) + desc_bytes);
  int32_t *d_vlen = reinterpret_cast<int32_t *>(d_voff + nw);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_voff, view->h_off.data(), (size_t)nw * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_vlen, view->h_len.data(), (size_t)nw * 4, hipMemcpyHostToDevice, ctx->stream));
  view->d_off = d_voff; view->d_len = d_vlen;
  if (d_desc_out) *d_desc_out = d_desc;
  return BATH_OK;
}

// the same for windows built on the device (bath_fs_windows.hip): descriptors with their pool offsets, the view's off[] and
// len[] are already there; only the pool is reserved and the copy kernel launched
int fs_gather_view_built(bath_hip_ctx *ctx, const bath_hip_seqs *dna, const FsWinBuild &B, const uint8_t *d_comp, bath_hip_seqs *view, const FsWinDev **d_desc_out) {
  const int nw = B.nw;
  DevBuf &b_pool = ctx->scratch[Scratch::kFsWindowPool];             // its own pool, apart from the one the domain stage gathers into (kFsGatherPool)
  BATH_HIP_TRY(ctx, b_pool.reserve((size_t)B.pool_bytes + 256));
  BATH_HIP_TRY(ctx, hipMemsetAsync(b_pool.p, 0x1d, (size_t)B.pool_bytes + 256, ctx->stream));
  hipLaunchKernelGGL(fs_window_gather_kernel, dim3((unsigned)std::max(1, std::min(nw, 65535))), dim3(256), 0, ctx->stream, dna->d_data, B.d_desc, nw, d_comp, b_pool.as<uint8_t>());
  BATH_HIP_TRY(ctx, hipGetLastError());
  view->ctx = ctx; view->n = nw; view->d_data = b_pool.as<uint8_t>(); view->is_part = true;
  view->h_off.resize((size_t)nw); view->h_len.resize((size_t)nw);
  for (int i = 0; i < nw; i++) { view->h_off[(size_t)i] = B.h_voff[i]; view->h_len[(size_t)i] = B.h_vlen[i]; }
  view->maxlen = B.maxlen; view->total = B.total; view->total_aligned = B.pool_bytes;
  view->d_off = const_cast<int64_t *>(B.d_voff); view->d_len = const_cast<int32_t *>(B.d_vlen);
  if (d_desc_out) *d_desc_out = B.d_desc;
  return BATH_OK;
}

float flogsum_host(float a, float b) {               // p7_FLogsum, logsum.c:105-111 (table of logsum.c:89)
  // (a function-local static with an initialiser: built once, thread-safe -- worker contexts and the window threads call this concurrently)
  static const std::vector<float> tbl = [] { std::vector<float> t(16000); for (int i = 0; i < 16000; i++) t[i] = (float)std::log(1. + std::exp((double)-i / 1000.f)); return t; }();
  const float mx = std::max(a, b), mn = std::min(a, b);
  return (mn == -INFINITY || (mx - mn) >= 15.7f) ? mx : mx + tbl[(int)((mx - mn) * 1000.f)];
}

// ---- the stages of bath_hip_pipeline_frameshift, in the order it calls them (the cascade with its survivors: filters_with_survivors)

// p7_pli_BuildDNAWindows + the per-window ORF summary of p7_pli_Frameshift (bath_fs_windows.hip): by kernels, from the lists the
// cascade's lanes left on the device; on the host (B->host_built), from the lists fetched after all, for the blocks the kernels hand back
static int fs_stage_windows(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna,
                            const bath_pipeline_params &prm, bool try_device, SurvivorSet *sv, FsWinBuild *B) {
  int st = try_device ? fs_build_windows_device(ctx, om, om_fs3, dna, &prm, sv->lanes.data(), sv->n_states, sv->nc_total, B) : (int)BATH_ENORESULT;
  if (st != BATH_ENORESULT) return st;
  if ((st = survivors_to_host(sv)) != BATH_OK) return st;
  return fs_build_windows_host(ctx, om, dna, &prm, sv->sel.data(), (int)sv->sel.size(), sv->wins.data(), (int)sv->wins.size(), B);
}

// The windows' copies, their bias filter (into Scratch::kFsWindowBias) and the 3-codon frameshift Forward for all of them (scores
// into h_fsc[nw] and Scratch::kFs3FwdScores), the regions beside it where the domain stage will want them; both streams joined
static int fs_stage_scores(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna, const SurvivorSet &sv,
                           const FsWinBuild &B, float *h_fsc) {
  const int nw = B.nw;
  int st;
  DevBuf &b_out = ctx->scratch[Scratch::kFsWindowBias];
  bath_hip_seqs view;
  const FsWinDev *d_desc = nullptr;
  if ((st = fs_gather_view_built(ctx, dna, B, sv.tt.comp, &view, &d_desc)) != BATH_OK) return st;   // descriptors, offsets and lengths are on the device
  BATH_HIP_TRY(ctx, b_out.reserve((size_t)nw * 6 * sizeof(float) + 64));
  // the bias filter (a lane per window and pass, serial over the window) and the Forward parser are independent: the bias
  // kernel goes to the side stream, behind the gather
  if ((st = fs_fork(ctx)) != BATH_OK) return st;
  hipLaunchKernelGGL(fs_bias_kernel, dim3((unsigned)((2 * nw + 63) / 64)), dim3(64), 0, ctx->side_stream, view.d_data, d_desc, nw, sv.tt.full, om->M, om->d_bias_eo,
                     sv.d_ssvsc, (int)om->base_b, om->scale_b, sv.d_bgf, b_out.as<float>());
  BATH_HIP_TRY(ctx, hipGetLastError());
  ctx->fs_regions_all.clear();
  ctx->fs_keep_xoff.clear();
  if (ctx->fs_want_regions && nw <= (int64_t)ctx->prop.multiProcessorCount * 16) {
    // The domain stage follows: its Backward parser, domain decoding and region heuristics run here, for every window,
    // next to the Forward parser whose score decides the branch.  These kernels are bound by the row chain of the longest
    // window as long as every window has a wave of its own (16 waves per CU), so up to that many windows the ones that will
    // take the standard branch cost nothing extra and the frameshift-branch windows have their regions before the decision
    // is made.  Beyond it the kernels take a second round of windows and the Backward parser of the windows that turn out
    // not to need it costs more than it saves (bench block, 7.6 k windows: 49.6 ms instead of 35 + 11.6 ms).
    ctx->fs_regions_all.assign((size_t)nw * (size_t)(1 + 3 * fs_max_regions()), 0);
    const float pmove = (2.0f + 1.0f) / (100.0f + 2.0f + 1.0f);              // p7_fs_ReconfigLength(L = 100, nj = 1): the saved length (p7_domaindef.c:318)
    st = fs3_regions(ctx, om_fs3, &view, (float)std::log((double)(1.0f - pmove)), ctx->fs_regions_all.data(), h_fsc);
  } else {
    // more windows than both parsers can run side by side for: Forward for all of them, the domain stage runs the Backward parser
    // for the frameshift-branch windows only (a speculative Backward of the longest windows beside Forward did not pay: DESIGN.md 7)
    st = fs3_forward_scores(ctx, om_fs3, &view, h_fsc);
  }
  if (st != BATH_OK) return st;
  return fs_join(ctx);                                                      // the bias kernel's side stream
}

// The host's bookkeeping over the completed records: pos_past_fwd (returned), and the ORFs of the windows that take the standard
// branch (:1479-1487), from the ordered ORF list, into ctx->fs_std_orfs
static int64_t fs_std_branch_orfs(bath_hip_ctx *ctx, const bath_hip_seqs *dna, const bath_pipeline_params &prm, const FsWinBuild &B, const std::vector<bath_fs_window> &out, int nc) {
  int64_t pos_fwd = 0;
  std::vector<char> aligned((size_t)std::max(nc, 1), 0);                   // oxf_holder[i] == NULL: an overlapping window already took the ORF (:1485)
  for (int i = 0; i < B.nw; i++) {
    const bath_fs_window &r = out[(size_t)i];
    if (r.branch == 1) { pos_fwd += r.length; continue; }
    if (r.branch != 2) continue;
    const int n_seq = dna->h_len[(size_t)r.window];
    for (int32_t z = B.h_grp[2 * i]; z < B.h_grp[2 * i + 1]; z++) {
      const FsOrfDev &o = B.h_orfs[z];
      if (!fs_orf_in_window(o, r, n_seq) || o.P > prm.F3) continue;         // :1405, :1483
      if (aligned[(size_t)o.cand]) continue;
      aligned[(size_t)o.cand] = 1;
      pos_fwd += (int64_t)o.n * 3;
      PipelineSurvivor ps;
      ps.window = r.window; ps.aa_off = o.aa_off; ps.strand = r.strand; ps.start = o.start; ps.n = o.n; ps.win_start = r.n; ps.fs_window = i;
      ctx->fs_std_orfs.push_back(ps);
    }
  }
  return pos_fwd;
}

}  // namespace bath

extern "C" int bath_hip_pipeline_frameshift(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna,
                                            const bath_pipeline_params *prm_in, bath_pipeline_stats *stats,
                                            const bath_orf_result **results, int64_t *n_results,
                                            const bath_fs_window **fs_windows, int64_t *n_fs_windows) {
  if (!ctx || !om || !om_fs3 || !dna || !prm_in || !fs_windows || !n_fs_windows) return BATH_EINVAL;
  if (fsprofile_codon_lengths(om_fs3) != 3) { ctx->set_error("the frameshift stage needs the 3-codon frameshift profile"); return BATH_EINVAL; }
  if (fs_model_ok(ctx, om_fs3) != BATH_OK) return BATH_EINVAL;
  *fs_windows = nullptr; *n_fs_windows = 0;
  ctx->fs_windows.clear();
  bath_pipeline_params prm = *prm_in;
  prm.fs_pipe = 1;
  bath_pipeline_stats st_local{};
  StageClock clk;
  SurvivorSet sv;
  const bool try_device = fs_windows_on_device();
  int st = filters_with_survivors(ctx, om, dna, &prm, &st_local, results, n_results, true, &sv, try_device);
  if (st != BATH_OK) return st;
  clk.lap("fs:   cascade + F4 survivors selected");
  FsWinBuild B;
  if ((st = fs_stage_windows(ctx, om, om_fs3, dna, prm, try_device, &sv, &B)) != BATH_OK) return st;
  clk.lap(B.host_built ? "fs:   DNA windows (host)" : "fs:   DNA windows (device)");
  const int nw = B.nw;
  std::vector<bath_fs_window> out((size_t)nw);                              // (the records arrive completed, after the branch decision)
  int64_t pos_fwd = 0;
  ctx->fs_std_orfs.clear();
  ctx->fs_std_pool = sv.pool;
  if (nw > 0) {
    std::vector<float> h_fsc((size_t)nw);
    if ((st = fs_stage_scores(ctx, om, om_fs3, dna, sv, B, h_fsc.data())) != BATH_OK) return st;
    // scores -> P-values -> branch (fsw_decide_kernel); the host reads the completed records once
    if ((st = fs_decide(ctx, om_fs3, &prm, B, ctx->scratch[Scratch::kFsWindowBias].as<float>(), ctx->scratch[Scratch::kFs3FwdScores].as<float>(), h_fsc.data(), out.data())) != BATH_OK) return st;
    clk.lap("fs:   gather + bias + 3-codon Forward + branch decision (device)");
    pos_fwd = fs_std_branch_orfs(ctx, dna, prm, B, out, sv.nc_total);
  }
  clk.lap("fs:   branch decision");
  st_local.pos_past_fwd = pos_fwd;                                         // in the fs pipeline only this stage counts it (:1468, :1490)
  if (stats) *stats = st_local;
  ctx->fs_windows = out;
  *fs_windows = ctx->fs_windows.data(); *n_fs_windows = nw;
  return BATH_OK;
}
