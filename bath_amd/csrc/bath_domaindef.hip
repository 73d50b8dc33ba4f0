// bath_domaindef.hip -- the frameshift branch after the decision of p7_pli_Frameshift: domain definition on the DNA
// windows that take the branch, and the scores of the resulting hits.
//
// Reference (src/p7_pipeline.c:1464-1476): p7_BackwardParser_Frameshift_3Codons, then
//   p7_domaindef_ByPosteriorHeuristics_Frameshift_BATH  (src/p7_domaindef.c:301-473)
//     p7_DomainDecoding_Frameshift                      (generic form: src/generic_decoding_frameshift.c:204-290)
//     is_multidomain_region_frameshift                  (:684-714)
//     rescore_isolated_domain_frameshift                (:993-1175): Forward/Backward/decoding/OA/null2 of the envelope,
//       p7_OATrace_Frameshift (generic form: src/generic_optacc_frameshift.c:373-588), null2 along the trace
//   p7_pli_postDomainDef_Frameshift_BATH                (src/p7_pipeline.c:1005-1144): the hit's bit score, bias, P-value
//
// Division of labour.  Everything that touches a DP matrix runs on the GPU, batched over all windows / envelopes of the
// block: the 3-codon parsers (fs3_fwd_kernel, fs_bwd_kernel<.,3,.>), the five envelope kernels of bath_fs_envelopes.hip and
// the optimal-accuracy traceback with the null2 score of the aligned residues (fs5_trace_kernel, a lane per envelope), so
// the posterior and OA matrices (>1 MB per envelope) never leave the device; the posterior sums over the parsers'
// special-state rows and the region heuristics run there too (fs_regions_kernel, a lane per window).  What remains for
// the host is bookkeeping and the score arithmetic of the hit.
// Multi-domain regions (:396-455) are resolved by stochastic-trace clustering (bath_ensemble.hip); *n_clustered_regions counts them.
// Not built: the printed alignment blocks.
// The reference carries om_fs5's length configuration from one window to the next; here the domain decoding always uses
// the configuration bathsearch starts with (L = 100 residues, multihit; bathsearch.c:797).
//
// This unit is host code only: fs_branch_domains orchestrates the stages above beside the standard branch of the other windows
// (bath::std_domains, bath_std_domains.hip, on a host thread and a context of its own), and bath_hip_pipeline_frameshift_domains
// is its C entry point.  The two accessors that serve the hits of both branches are here as well: bath_hip_domain_cigars (with
// cigar_from_columns, which both branches call) and bath_hip_domain_traces.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bath_common.hpp"
#include "bath_host_threads.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

// The --cigar string of an alignment (p7_alidisplay_fs_Create, p7_alidisplay.c:777-815, 841-869; the non-frameshift display
// :1140-1200 is the special case "every codon has 3 nucleotides").  One code per alignment column:
// state (3 = M, 4 = D, 5 = I) | codon length << 4 | indel label << 8 (hmmer.h:259-276).
std::string bath::cigar_from_columns(const uint16_t *S, int n) {
  enum { sM = 3, sD = 4, sI = 5 };
  enum { L___X = 0, L_X__, L_XX_, L_X_X, L__XX, L_XXX, L_XXx, L_XxX, L_xXX, L_xxx, L_XXxX, L_XxXX, L_xXXX, L_XXxxX, L_XxxXX, L_xxXXX };
  std::string out;
  int cnt = 0;
  auto emit = [&](int v, char ch) { out += std::to_string(v); out += ch; };
  for (int z = 0; z < n; z++) {
    const int s = S[z] & 0xf, c = (S[z] >> 4) & 0xf, indel = S[z] >> 8;
    const int next = (z + 1 < n) ? (S[z + 1] & 0xf) : -1;
    if (s == sM) {
      if (next != sM || c != 3) {
        if (c == 3) cnt += 3;
        else if (indel == L_XX_ || indel == L_XXxX || indel == L_XXxxX) cnt += 2;
        else if (indel == L_X_X || indel == L_X__ || indel == L_XxXX || indel == L_XxxXX) cnt += 1;
        emit(cnt, 'M');
        cnt = 0;
        if (c == 1) emit(2, 'B'); else if (c == 2) emit(1, 'B'); else if (c == 4) emit(1, 'F'); else if (c == 5) emit(2, 'F');
        if (indel == L___X || indel == L_X_X || indel == L_XXxX || indel == L_XXxxX) cnt = 1;
        if (indel == L__XX || indel == L_XxXX || indel == L_XxxXX) cnt = 2;
        if (indel == L_xXXX || indel == L_xxXXX) cnt = 3;
        if (next != sM && cnt > 0) { emit(cnt, 'M'); cnt = 0; }
      } else cnt += 3;
    } else if (s == sI || s == sD) {
      cnt += 3;
      if (next != s) { emit(cnt, s == sI ? 'I' : 'D'); cnt = 0; }
    }
  }
  return out;
}

namespace {

// Wait for a flag another agent (a kernel writing to page-locked memory) will set: a few yields for the flag that is about to come,
// then sleeps -- a thread that polls through sched_yield for the 5-15 ms a region's matrix takes burns a core of the CPU quota
// (bath_host_threads.hpp).
inline void wait_for_flag(const int *flag) {
  for (int spins = 0; !__atomic_load_n(flag, __ATOMIC_ACQUIRE); spins++) {
    if (spins < 32) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(spins < 256 ? 20 : 100));
  }
}

struct Env { int sel, i, j; };        // nucleotides i..j of the window regs[sel]: an envelope, or a multi-domain region

// What every batch of envelopes reads beside its list of envelopes
struct EnvSource {
  const bath_hip_seqs *dna;
  const std::vector<FsWinDev> &regs;  // the windows that took the branch
  const bath_hip_fsprofile *om_fs5;
  int M;
  const uint8_t *d_comp, *d_cons;     // the complement table, the model's consensus residues
  size_t budget;                      // bytes of matrices per launch
};

// Envelopes through the envelope kernels, and what the hit stage reads of them (indexed from 0 within the batch)
struct EnvBatch {
  std::vector<FsWinDev> eregs;
  std::vector<bath_fs5_result> res;
  std::vector<FsTraceOut> traces;
  std::vector<uint16_t> steps;
  std::vector<float> pps;                                                    // tr->pp per column, parallel to steps
  std::vector<int64_t> step_off;
  int run(bath_hip_ctx *c, const EnvSource &s, const Env *list, int n);      // the batch <list> on context <c>, results into this (replacing what it held)
  void append(const EnvBatch &b);                                            // a finished batch joins this one, behind what it holds
};

int EnvBatch::run(bath_hip_ctx *c, const EnvSource &s, const Env *list, int n) {
  eregs.resize((size_t)n); res.resize((size_t)n); traces.resize((size_t)n); step_off.assign((size_t)n + 1, 0);
  steps.clear(); pps.clear();
  for (int e = 0; e < n; e++) {
    const FsWinDev &wr = s.regs[(size_t)list[e].sel];
    FsWinDev d = wr;
    d.start = wr.start + list[e].i - 1; d.len = list[e].j - list[e].i + 1;
    eregs[(size_t)e] = d;
  }
  for (int e0 = 0; e0 < n;) {
    int e1 = e0;
    size_t bytes = 0;
    while (e1 < n) {
      const size_t b = ((size_t)eregs[(size_t)e1].len + 1) * (size_t)(s.M + 1) * 56;
      if (e1 > e0 && bytes + b > s.budget) break;
      bytes += b; e1++;
    }
    std::vector<FsWinDev> chunk(eregs.begin() + e0, eregs.begin() + e1);
    std::vector<uint16_t> csteps;
    std::vector<float> cpps;
    std::vector<int64_t> coff;
    bath_hip_seqs view;
    // (a batch on another context runs on another host thread: its error text stays in that context until the caller has joined)
    int st2 = fs_gather_view(c, s.dna, chunk, s.d_comp, &view, nullptr);
    if (st2 != BATH_OK) return st2;
    st2 = fs5_envelopes_ex(c, s.om_fs5, &view, BATH_LOGSUM_CONTEXT, 0, res.data() + e0, nullptr, nullptr, nullptr, nullptr, traces.data() + e0, s.d_cons, &csteps, &coff, &cpps);
    if (st2 != BATH_OK) return st2;
    const int64_t base = (int64_t)steps.size();
    for (int k = 0; k < e1 - e0; k++) step_off[(size_t)(e0 + k)] = base + coff[(size_t)k];
    steps.insert(steps.end(), csteps.begin(), csteps.end());
    pps.insert(pps.end(), cpps.begin(), cpps.end());
    e0 = e1;
  }
  step_off[(size_t)n] = (int64_t)steps.size();
  return BATH_OK;
}

void EnvBatch::append(const EnvBatch &b) {
  const int64_t base = (int64_t)steps.size();
  if (step_off.empty()) step_off.push_back(0);
  step_off.pop_back();
  eregs.insert(eregs.end(), b.eregs.begin(), b.eregs.end());
  res.insert(res.end(), b.res.begin(), b.res.end());
  traces.insert(traces.end(), b.traces.begin(), b.traces.end());
  for (size_t k = 0; k + 1 < b.step_off.size(); k++) step_off.push_back(base + b.step_off[k]);
  steps.insert(steps.end(), b.steps.begin(), b.steps.end());
  pps.insert(pps.end(), b.pps.begin(), b.pps.end());
  step_off.push_back((int64_t)steps.size());
}

// p7_pli_postDomainDef_Frameshift_BATH over the envelopes <envs> and what the kernels left of them in <b> (same order): the hit's
// scores and coordinates; the hits, their --cigar strings and their traces are appended to the context's.  <fw>[sel[q]]: the
// DNA window of regs[q].
void fs_score_hits(bath_hip_ctx *ctx, const bath_hip_seqs *dna, const bath_fs_window *fw, const std::vector<int> &sel, const std::vector<Env> &envs,
                   const EnvBatch &b, const FsHostTables &h5, const DomOpts &opt) {
  const int ml = h5.max_length;
  const RunningZ runZ(dna, opt.nres_before, opt.strands);                     // pli->Z, p7_domaindef.c:1033: the count at the hit's window and strand
  for (size_t e = 0; e < envs.size(); e++) {
    const Env &en = envs[e];
    const bath_fs_window &win = fw[sel[(size_t)en.sel]];
    const int Ld = b.eregs[e].len;
    const float envsc = b.res[e].fwdsc;
    if (!(envsc > -INFINITY) || !(b.res[e].bcksc > -INFINITY)) continue;
    const float Zf = runZ.Z(win.window, win.strand, ml);
    {
      const float p1 = (float)(Ld / 3) / (float)(Ld / 3 + 1);
      const float per_frame = (float)((float)(Ld / 3) * std::log((double)p1) + std::log(1. - p1));
      const float nullsc = (float)(per_frame + std::log(3.0));
      const float seqscore = (float)((envsc - nullsc) / kLn2);
      if (opt.inc_by_E && exp_surv(seqscore, h5.evparam[7], h5.evparam[BATH_FLAMBDA]) * (double)Zf > opt.E) continue;    // :1034 (FTAUFS5)
    }
    const FsTraceOut &tq = b.traces[e];
    if (!tq.ok) continue;
    if (tq.aliscore < 0.0f) continue;                                          // p7_domaindef.c:1072: "repetitive garbage", no domain
    bath_fs_domain dm{};
    dm.window = win.window; dm.strand = win.strand; dm.fs_window = sel[(size_t)en.sel];
    // window coordinates first (:1148-1163), then the sequence's (p7_pipeline.c:1035-1049); envelope i..j in the window
    const int wi = en.i, wj = en.j;
    int iali = wi - 1 + tq.iali, jali = wi - 1 + tq.jali, ienv = wi, jenv = wj;
    const int ali_len = jali - iali + 1, env_len = jenv - ienv + 1;
    dm.ihmm = tq.ihmm; dm.jhmm = tq.jhmm;
    dm.envsc = envsc; dm.oasc = b.res[e].oasc; dm.domcorrection = std::max(0.f, tq.domcorrection);
    dm.n_shifted_codons = tq.nshift;
    if (ali_len >= 12) {
      const int64_t dstart = win.strand ? dna->h_len[(size_t)win.window] : 1;
      auto map = [&](int p) { return (int32_t)(win.strand ? dstart - (win.n + p) + 2 : dstart + win.n + p - 2); };
      dm.ienv = map(ienv); dm.jenv = map(jenv); dm.iali = map(iali); dm.jali = map(jali);
      float bitscore = envsc;                                                  // :1055-1059
      bitscore -= 2 * std::log(2. / ((env_len / 3.) + 2));
      bitscore += 2 * std::log(2. / (ml + 2));
      bitscore -= ((env_len - ali_len) / 3.) * std::log((double)((float)(env_len / 3.) / (float)((env_len / 3.) + 2)));
      bitscore += ((std::max(env_len, ml * 3) - ali_len) / 3.) * std::log((double)((float)ml / (float)(ml + 2)));
      const float dom_bias = opt.do_null2 ? flogsum_host(0.0f, (float)(std::log(1. / 256.) + dm.domcorrection)) : 0.0f;     // :1063-1066; bg->omega = 1/256, p7_bg.c:74
      const int nl = std::max(env_len / 3, ml);
      const float p1 = (float)nl / (float)(nl + 1);
      const float per_frame = (float)((float)nl * std::log((double)p1) + std::log(1. - p1));
      const float nullsc = (float)(per_frame + std::log(3.0));
      dm.dombias = dom_bias;
      dm.bitscore = (float)((bitscore - (nullsc + dom_bias)) / kLn2);
      dm.pre_score = (float)(bitscore / kLn2);
      dm.lnP = exp_logsurv(dm.bitscore, h5.evparam[7], h5.evparam[BATH_FLAMBDA]);
      dm.reported = opt.reportable(dm.lnP, Zf, dm.bitscore) ? 1 : 0;           // :1080
    } else { dm.ienv = ienv; dm.jenv = jenv; dm.iali = iali; dm.jali = jali; dm.reported = 0; }
    dm.n_stops = tq.nstops; dm.ali_columns = tq.ncol;
    dm.pid = tq.ncol > 0 ? ((float)tq.exact / tq.ncol) * 100 : 0.f;
    dm.cigar_off = (int64_t)ctx->cigars.size();
    ctx->cigars += cigar_from_columns(b.steps.data() + b.step_off[e], tq.ncol);
    ctx->cigars.push_back('\0');
    ctx->fs_domains.push_back(dm);
    // dom->tr: states z1..z2 in window coordinates (the i - 1 shift of p7_domaindef.c:1053-1054 applied to every i >= 0: a D state's 0 becomes wi - 1)
    ctx->trace_push(b.steps.data() + b.step_off[e], b.pps.size() == b.steps.size() ? b.pps.data() + b.step_off[e] : nullptr, tq.ncol, tq.ihmm,
                    wi - 1 + tq.iali, win.n, 0, 1, wi - 1);
  }
}

}  // namespace

static int fs_branch_domains(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3,
                             const bath_hip_fsprofile *om_fs5, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                             double E_report, bath_pipeline_stats *stats,
                             const bath_fs_window **fs_windows, int64_t *n_fs_windows,
                             const bath_fs_domain **domains, int64_t *n_domains, int64_t *n_clustered_regions, int64_t *std_clustered) {
  if (!ctx || !om || !om_fs3 || !om_fs5 || !dna || !prm || !domains || !n_domains) return BATH_EINVAL;
  if (fsprofile_codon_lengths(om_fs5) != 5) { ctx->set_error("domain definition needs the 5-codon frameshift profile"); return BATH_EINVAL; }
  if (fs_model_ok(ctx, om_fs3) != BATH_OK || fs_model_ok(ctx, om_fs5) != BATH_OK) return BATH_EINVAL;
  *domains = nullptr; *n_domains = 0;
  if (n_clustered_regions) *n_clustered_regions = 0;
  ctx->fs_domains.clear();
  ctx->cigars.clear();
  ctx->traces_clear();
  ctx->spans_reset();
  bath_pipeline_stats st_local{};
  const bath_fs_window *fw = nullptr;
  int64_t nfw = 0;
  StageClock clk;
  ctx->fs_want_regions = true;
  int st = bath_hip_pipeline_frameshift(ctx, om, om_fs3, dna, prm, &st_local, nullptr, nullptr, &fw, &nfw);
  ctx->fs_want_regions = false;
  if (st != BATH_OK) return st;
  clk.lap("fs: cascade + windows + decision");
  if (stats) *stats = st_local;
  if (fs_windows) *fs_windows = fw;
  if (n_fs_windows) *n_fs_windows = nfw;
  const FsHostTables h5 = fsprofile_host(om_fs5);
  if (!h5.codons) { ctx->set_error("5-codon profile without its codon table"); return BATH_EINVAL; }

  // ---- the windows that took the frameshift branch: both 3-codon parsers with their special-state rows
  std::vector<int> sel;
  std::vector<FsWinDev> regs;
  for (int64_t i = 0; i < nfw; i++) {
    if (fw[i].branch != 1) continue;
    FsWinDev d{};
    d.src_off = dna->h_off[(size_t)fw[i].window]; d.seq_n = dna->h_len[(size_t)fw[i].window]; d.start = fw[i].n; d.len = fw[i].length; d.strand = fw[i].strand;
    sel.push_back((int)i); regs.push_back(d);
  }
  if (sel.empty()) return BATH_OK;
  // ---- the standard branch of the other windows (p7_pipeline.c:1479-1510) needs nothing from the frameshift branch.  The
  // stages below are chains of latency-bound kernels, a PCIe-bound one and host work that leave most of the GPU idle, so the
  // standard-branch domains run beside them: own host thread, own context (stream, scratch, page-locked buffers), reading the
  // cascade's residue pool.  Their domains are put in front of the frameshift branch's, as when they ran first.
  std::thread std_thread;
  int std_rc = BATH_OK;
  int64_t std_nclust = 0;
  const char *ser = std::getenv("BATH_HIP_FS_STD_SERIAL");
  if (std_clustered && !ctx->fs_std_orfs.empty() && !(ser && ser[0] == '1')) {
    if (!ctx->aux && (st = bath_hip_init(ctx->device, &ctx->aux)) != BATH_OK) { ctx->set_error("cannot create the context of the standard branch"); return st; }
    mark_internal(ctx->aux);
    if ((st = om->ensure_len_tables(dna->maxlen / 3 + 1)) != BATH_OK) return st;      // the profile's mutable state: fill it before the thread starts
    bath_hip_ctx *aux = ctx->aux;
    aux->fs_domains.clear(); aux->cigars.clear(); aux->traces_clear();
    aux->std_ensemble = ctx->std_ensemble; aux->spans_reset();
    const DomOpts std_opt(*prm, E_report);
    std_thread = std::thread([&, aux, std_opt] {
      if (hipSetDevice(ctx->device) != hipSuccess) { std_rc = BATH_EFAIL; return; }
      std_rc = std_domains(aux, om, dna, ctx->fs_std_orfs, ctx->fs_std_pool, std_opt, &std_nclust);
    });
  }
  struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } };
  Joiner std_joiner{std_thread};                                              // also on error returns
  auto finish_std = [&]() -> int {
    if (!std_thread.joinable()) return BATH_OK;
    std_thread.join();
    if (std_rc != BATH_OK) { ctx->set_error(ctx->aux->err); return std_rc; }
    const int64_t shift = (int64_t)ctx->cigars.size();
    for (bath_fs_domain dm : ctx->aux->fs_domains) { dm.cigar_off += shift; ctx->fs_domains.push_back(dm); }
    ctx->cigars += ctx->aux->cigars;
    for (const bath_hip_ctx::TraceRec &t : ctx->aux->tr_recs)
      ctx->trace_push(ctx->aux->tr_codes.data() + t.col_off, ctx->aux->tr_pp.data() + t.col_off, t.ncol, t.k1, t.i_first, t.win_start, t.orf_start, t.frameshift, t.d_i);
    *std_clustered = std_nclust;
    return BATH_OK;
  };
  OrfTablesDev tt{};
  if ((st = orf_tables_upload(ctx, prm->ncbi_table, &tt, prm->initiator)) != BATH_OK) return st;
  const int nsel = (int)sel.size();
  const int RS = 1 + 3 * fs_max_regions();
  std::vector<int32_t> regions((size_t)nsel * RS, 0);
  const float pmove = (2.0f + 1.0f) / (100.0f + 2.0f + 1.0f);                 // p7_fs_ReconfigLength(L = 100, nj = 1), modelconfig.c:767-770
  const float loop = (float)std::log((double)(1.0f - pmove));
  if (ctx->fs_regions_all.size() == (size_t)nfw * (size_t)RS) {                // the decision stage already ran them for every window
    for (int q = 0; q < nsel; q++) std::memcpy(&regions[(size_t)q * RS], &ctx->fs_regions_all[(size_t)sel[(size_t)q] * RS], sizeof(int32_t) * (size_t)RS);
  } else {
    bath_hip_seqs view;
    if ((st = fs_gather_view(ctx, dna, regs, tt.comp, &view, nullptr)) != BATH_OK) return st;
    st = fs3_regions(ctx, om_fs3, &view, loop, regions.data(), nullptr, sel.data());   // Backward parser (Forward's rows are the decision stage's), domain decoding, region heuristics: all on the device
    if (st != BATH_OK) return st;
    clk.lap("fs: parsers + regions");
  }
  std::vector<Env> envs, mregs;
  for (int q = 0; q < nsel; q++) {
    const int32_t *r = &regions[(size_t)q * RS];
    if (r[0] > fs_max_regions()) { ctx->set_error("a DNA window has more regions than the region buffer holds"); return BATH_ERANGE; }
    for (int k = 0; k < r[0]; k++) {                                          // r[0] == -1: Backward underflow, the reference skips the window (:1471)
      const int i = r[1 + 3 * k], j = r[2 + 3 * k];
      if (r[3 + 3 * k]) mregs.push_back(Env{q, i, j});
      else if (j - i + 1 >= 15) envs.push_back(Env{q, i, j});                 // rescore_isolated_domain: Ld < 15 -> nothing
    }
  }
  if (n_clustered_regions) *n_clustered_regions = (int64_t)mregs.size();          // regions resolved by clustering (ddef->nclustered)

  // ---- envelopes: Forward, Backward, decoding, optimal accuracy, null2 on the GPU (unihit, length Ld/3)
  EnvBatch all;                                                              // every envelope the hit stage reads, in envs order
  // The envelope kernels keep three matrices per envelope in HBM (Forward 32 B, Backward 12 B, optimal accuracy 12 B per
  // cell): the envelopes go through in batches of at most 24 GB of matrices (BATH_HIP_ENV_MB overrides, for tests), so a block
  // of any size fits next to the DNA and the amino-acid streams.
  size_t budget = (size_t)24 << 30;
  {                                                                          // ... and at most half of what is free right now
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 2 < budget) budget = std::max<size_t>(free_b / 2, (size_t)64 << 20);
  }
  if (const char *e = std::getenv("BATH_HIP_ENV_MB")) budget = (size_t)std::max(1, std::atoi(e)) << 20;
  const EnvSource src{dna, regs, om_fs5, h5.M, tt.comp, om->d_cons, budget};    // (read by the ensembles' thread too: declared before its joiner)
  auto run_envelopes = [&](int e_begin, int e_end) -> int {                    // envs[e_begin, e_end) on this context, results appended (e_begin = what is done so far)
    EnvBatch b;
    const int st2 = b.run(ctx, src, envs.data() + e_begin, e_end - e_begin);
    if (st2 != BATH_OK) return st2;
    all.append(b);
    return BATH_OK;
  };
  const int n_single = (int)envs.size();
  const int n_single_early = n_single;
  int done = 0;

  // ---- multi-domain regions (p7_domaindef.c:396-455): Forward of the region in the multihit configuration (GPU), ensemble of
  // stochastic tracebacks and clustering (host, bath_ensemble.hip); every cluster is an envelope
  std::vector<std::vector<Env>> found;                                       // written by the ensemble threads: declared BEFORE the joiner, so it outlives the join on every return
  // bath_hip_set_fs_ensemble.  BATH_ENSEMBLE_STREAMS_DEVICE: the regions' matrices stay in device memory, fs_ensemble_kernel walks the
  // traces behind the Forward kernel on the same stream, and the ensembles' thread gets statuses and segments in one small copy
  // (ens_run, read by that thread: declared before the joiner as well); the other modes walk on host threads as before.
  const int ens_mode = ctx->fs_ensemble;
  const bool ens_dev = ens_mode == BATH_ENSEMBLE_STREAMS_DEVICE;
  FsEnsRun ens_run;
  std::atomic<int> ens_rc{BATH_OK};                                          // a failed copy or synchronize on the ensembles' threads: reported after the join
  // Strict mode, when this is the only context the host holds (host_contexts() == 1; BATH_HIP_FS_CLUSTERS_BESIDE=1|0 forces): the
  // clusters' envelopes go through the kernels on a context of their own as soon as the last ensemble is done, from the ensembles'
  // own thread -- beside the tail of the single-domain batch (its decoding and tracebacks) instead of after it: 62.2-62.5 ms per
  // pass against 64.3-65.0.  With other contexts at work the extra context's streams cost more than that (two workers 52-59 ms per
  // block against 48.5), and an idle one costs the fast mode 15 ms per pass (bath_hip_trim releases it; bath_hip_set_fs_strict(ctx, 0)
  // does so itself).  Written by that thread, read after the join.
  EnvBatch cl_batch;
  std::vector<Env> cl_envs;
  int cl_rc = BATH_OK;
  std::string cl_err;                                                        // that thread's error text: copied into ctx->err after the join (ctx->err is the caller thread's)
  bool cl_ran = false;
  bath_hip_ctx *rctx = ctx;                                                  // where the regions' Forward runs
  std::thread ensembles;
  Joiner joiner{ensembles};                                                  // also on error returns
  if (!mregs.empty()) {
    std::vector<FsWinDev> rregs(mregs.size());
    for (size_t e = 0; e < mregs.size(); e++) {
      FsWinDev d = regs[(size_t)mregs[e].sel];
      d.start = regs[(size_t)mregs[e].sel].start + mregs[e].i - 1; d.len = mregs[e].j - mregs[e].i + 1;
      rregs[e] = d;
    }
    const float *h_f = nullptr, *h_x = nullptr;                              // pinned buffers of the context
    const int *h_done = nullptr;
    const float *h_sc_live = nullptr;
    std::vector<float> h_sc;
    std::vector<int64_t> foff, xoff;
    const float pm = (2.0f + 1.0f) / (100.0f + 2.0f + 1.0f);                 // p7_fs_ReconfigLength(L = 100), multihit (nj = 1)
    const float xNL = (float)std::log((double)(1.0f - pm)), xNM = (float)std::log((double)pm), xE = (float)-kLn2;
    {
      // Strict mode: the regions' Forward is a chain of L x 2M dependent log-sums per region on a few CUs (bath_fs_chain.hip) and
      // the envelope kernels are bound by throughput (bath_fs_wavefront.hip), so the envelopes of the single-domain regions go
      // through the chip WHILE the regions' Forward runs: it gets a context of its own (stream, gather pool, offsets, job list).
      if (ctx->fs_strict && !ctx->aux2) {
        if ((st = bath_hip_init(ctx->device, &ctx->aux2)) != BATH_OK) { ctx->set_error("cannot create the context of the regions' Forward"); return st; }
        mark_internal(ctx->aux2);
        // HIP multiplexes its streams onto a few hardware queues (4 by default; the environment's GPU_MAX_HW_QUEUES) and two streams
        // that land on one queue run their kernels one after the other: with a dozen streams alive (lanes, side, copy, the standard branch) the
        // regions' Forward ended up behind the envelope kernels it is meant to run beside (+13 ms per pass in bench.py's process).
        // Streams of another priority get queues of their own; the regions' Forward is the critical path of this stage anyway.
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
          hipStream_t ps = nullptr;
          if (hipStreamCreateWithPriority(&ps, hipStreamNonBlocking, hi) == hipSuccess) { (void)hipStreamDestroy(ctx->aux2->stream); ctx->aux2->stream = ps; }
          else (void)hipGetLastError();
        }
      }
      rctx = ctx->fs_strict ? ctx->aux2 : ctx;
      if (rctx != ctx) { rctx->fs_strict = ctx->fs_strict; rctx->fs_odds = ctx->fs_odds; rctx->fs5_odds = ctx->fs5_odds; rctx->fs_ensemble = ctx->fs_ensemble; rctx->spans_reset(); }
      bath_hip_seqs view;
      if ((st = fs_gather_view(rctx, dna, rregs, tt.comp, &view, nullptr)) != BATH_OK) { if (rctx != ctx) ctx->set_error(rctx->err); return st; }
      // returns after the launch: a region's ensemble starts as soon as ITS matrix has landed in host memory (h_done[e]), so the
      // tracebacks run while the kernel is still streaming the other regions over PCIe (longest regions first, on both sides)
      if (ens_dev) st = fs5_region_ensembles_device(rctx, om_fs5, &view, 100, (uint32_t)prm->seed, xNL, xNM, xE, &ens_run);
      else
      st = fs5_region_forward(rctx, om_fs5, &view, 100, &h_f, &foff, &h_x, &xoff, &h_sc, &h_done, &h_sc_live);      // saveL: the configuration bathsearch starts with
      if (st != BATH_OK) { if (rctx != ctx) ctx->set_error(rctx->err); return st; }
    }
    found.assign(mregs.size(), {});
    // The ensembles are host work (200 dependent tracebacks per region from one random-number stream); the envelopes of the
    // single-domain regions do not depend on them, so their kernels run on the GPU meanwhile.
    { const char *lv = std::getenv("BATH_HIP_FS_LIVE"); if (lv && lv[0] == '0') (void)hipStreamSynchronize(rctx->stream); }
    ensembles = std::thread([&, h_f, h_x, xNL, xNM, xE, foff, xoff, h_done, h_sc_live, rregs] {
      bool dev_ok = true;                                                      // device mode: the kernel's small copy has landed
      if (ens_dev) dev_ok = hipSetDevice(ctx->device) == hipSuccess && hipStreamSynchronize(rctx->stream) == hipSuccess;
      if (!dev_ok) ens_rc = BATH_EFAIL;
      auto work = [&](int64_t first, int64_t step) {
        std::vector<std::pair<int, int>> cl;
        for (size_t e = (size_t)first; e < mregs.size(); e += (size_t)step) {
          const int Lr = rregs[e].len;
          if (ens_dev) {                                                       // shift, cluster; a host walk only for a region the kernel could not serve
            if (!dev_ok) continue;
            if (fs_ensemble_region_from_device(rctx, ctx, ens_run, (int64_t)e, h5.M, h5.tsc, xNL, xNM, xE, mregs[e].i, Lr, (uint32_t)prm->seed, &cl) != BATH_OK) { ens_rc = BATH_EFAIL; continue; }
          } else {
          wait_for_flag(h_done + e);                                           // this region's matrix is still on its way
          if (!(h_sc_live[e] > -INFINITY)) continue;                          // Forward underflow: no valid traces for this region (:413)
          if (ens_mode == BATH_ENSEMBLE_SERIAL) {
          if (fs_region_trace_ensemble(h5.M, h5.tsc, xNL, xNM, xE, mregs[e].i, Lr, h_f + foff[e], h_x + xoff[e], &cl, (uint32_t)prm->seed) != BATH_OK) continue;
          } else if (fs_region_ensemble_host(ctx, ens_mode, h5.M, h5.tsc, xNL, xNM, xE, mregs[e].i, Lr, h_f + foff[e], h_x + xoff[e], &cl, (uint32_t)prm->seed) != BATH_OK) continue;
          }
          for (const auto &c : cl) {
            const int i2 = std::max(1, c.first), j2 = c.second;               // :449
            if (j2 - i2 + 1 >= 15) found[e].push_back(Env{mregs[e].sel, i2, j2});
          }
        }
      };
      StageClock eclk;
      // shortest region first: that is the order in which their matrices finish arriving (all regions advance together, a wave
      // each, sharing the PCIe link), so a thread rarely waits for the region it drew
      run_striped((int64_t)mregs.size(), work, [&](int64_t e) { return -rregs[(size_t)e].len; });
      eclk.lap("fs:   (ensemble threads, start to end)");
      static const int beside_env = [] { const char *e = std::getenv("BATH_HIP_FS_CLUSTERS_BESIDE"); return e ? (e[0] == '1' ? 1 : 0) : -1; }();
      const bool clusters_beside = beside_env >= 0 ? beside_env == 1 : host_contexts() == 1;      // default: when this is the host's only context
      if (rctx != ctx && clusters_beside) {
        cl_ran = true;
        if (hipSetDevice(ctx->device) != hipSuccess) { cl_rc = BATH_EFAIL; cl_err = "hipSetDevice failed on the clusters' thread"; return; }
        if (!ctx->aux3 && bath_hip_init(ctx->device, &ctx->aux3) != BATH_OK) { cl_rc = BATH_EFAIL; cl_err = "cannot create the context of the clusters' envelopes"; return; }
        mark_internal(ctx->aux3);
        bath_hip_ctx *cctx = ctx->aux3;                                         // the clusters' envelopes on a context of their own
        cctx->fs_strict = ctx->fs_strict; cctx->fs_odds = ctx->fs_odds; cctx->fs5_odds = ctx->fs5_odds; cctx->fs_ensemble = ctx->fs_ensemble; cctx->spans_reset();
        for (size_t e = 0; e < mregs.size(); e++) cl_envs.insert(cl_envs.end(), found[e].begin(), found[e].end());
        if (!cl_envs.empty() && (cl_rc = cl_batch.run(cctx, src, cl_envs.data(), (int)cl_envs.size())) != BATH_OK) cl_err = cctx->err;
        eclk.lap("fs:   (clusters' envelope kernels + traces, same thread)");
      }
    });
    // strict mode: the first batch of envelopes goes through now, beside the regions' Forward (which runs on its own context)
    if (rctx != ctx && n_single_early > 0) {
      if ((st = run_envelopes(0, n_single_early)) != BATH_OK) {
        (void)hipStreamSynchronize(rctx->stream);
        if (h_done) for (size_t e = 0; e < mregs.size(); e++) { const_cast<float *>(h_sc_live)[e] = -INFINITY; __atomic_store_n(const_cast<int *>(h_done) + e, 1, __ATOMIC_RELEASE); }
        return st;
      }
      done = n_single_early;
      clk.lap("fs: envelope kernels + traces (single-domain regions, beside the regions' Forward)");
    }
    if (hipStreamSynchronize(rctx->stream) != hipSuccess) {                   // the region Forward itself (the ensembles are already at work)
      for (size_t e = 0; h_done && e < mregs.size(); e++) {                   // release the threads waiting for matrices that will not come
        const_cast<float *>(h_sc_live)[e] = -INFINITY;
        __atomic_store_n(const_cast<int *>(h_done) + e, 1, __ATOMIC_RELEASE);
      }
      ctx->set_error("region Forward failed"); return BATH_EFAIL;
    }
    clk.lap("fs: region Forward -> host memory");
  }

  // Order of the work.  The ensembles are host threads; the standard branch of the other windows (p7_pipeline.c:1479-1510)
  // needs nothing from them, so its kernels and host work run meanwhile.  Then ALL envelopes -- of the single-domain regions
  // and of the clusters -- go through the envelope kernels as one batch: those kernels last as long as their longest
  // envelope whatever the number of envelopes (one wave each), so two batches cost two such chains (14.3 + 9.4 ms on the
  // bench block) and one batch costs one.  BATH_HIP_FS_TWO_BATCHES=1: the single-domain regions first, during the ensembles.
  const char *tb = std::getenv("BATH_HIP_FS_TWO_BATCHES");
  const bool two_batches = tb && tb[0] == '1';
  if (ensembles.joinable() && two_batches && n_single > 0 && done == 0) {
    if ((st = run_envelopes(0, n_single)) != BATH_OK) return st;
    done = n_single;
    clk.lap("fs: envelope kernels + traces (single-domain regions)");
  }
  if (ensembles.joinable()) {
    ensembles.join();
    if (ens_rc.load() != BATH_OK) { ctx->set_error("the device ensemble of the multi-domain regions failed (stream synchronize or a region's copy to the host)"); return ens_rc.load(); }
    for (size_t e = 0; e < mregs.size(); e++) envs.insert(envs.end(), found[e].begin(), found[e].end());
    clk.lap("fs: ensembles (host threads)");
  }
  if ((st = finish_std()) != BATH_OK) return st;
  clk.lap("fs: standard-branch domains (own thread and stream), remainder");
  const int nenv = (int)envs.size();
  if (nenv == 0) return BATH_OK;
  if (cl_ran && done == n_single) {                                          // the clusters' batch ran beside the first one (same order as envs)
    if (cl_rc != BATH_OK) { ctx->set_error(cl_err.empty() ? "the clusters' envelope batch failed" : cl_err.c_str()); return cl_rc; }
    if (!cl_envs.empty()) all.append(cl_batch);
    done = nenv;
  }
  if (nenv > done && (st = run_envelopes(done, nenv)) != BATH_OK) return st;
  clk.lap("fs: envelope kernels + traces");

  // ---- traceback, null2 along the trace, the hit's scores
  fs_score_hits(ctx, dna, fw, sel, envs, all, h5, DomOpts(*prm, E_report));
  *domains = ctx->fs_domains.data(); *n_domains = (int64_t)ctx->fs_domains.size();
  return BATH_OK;
}

// p7_pli_Frameshift's two branches (p7_pipeline.c:1464-1510): windows that take the frameshift branch get the codon-model
// domain definition above; in the others every ORF with P <= F3 goes through the standard domain definition (bath_std_domains.hip), its
// alignment placed on the DNA window's coordinates.
extern "C" int bath_hip_pipeline_frameshift_domains(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3,
                                                    const bath_hip_fsprofile *om_fs5, const bath_hip_seqs *dna, const bath_pipeline_params *prm,
                                                    double E_report, bath_pipeline_stats *stats,
                                                    const bath_fs_window **fs_windows, int64_t *n_fs_windows,
                                                    const bath_fs_domain **domains, int64_t *n_domains, int64_t *n_clustered_regions) {
  bath_pipeline_stats st_local{};
  int64_t std_clustered = -1;                                                   // >= 0: the standard branch already ran, overlapped with the ensembles
  int64_t fs_clustered = 0;
  int st = fs_branch_domains(ctx, om, om_fs3, om_fs5, dna, prm, E_report, &st_local, fs_windows, n_fs_windows, domains, n_domains, &fs_clustered, &std_clustered);
  if (st != BATH_OK) return st;
  if (stats) *stats = st_local;
  int64_t nclust = fs_clustered;
  StageClock clk;
  if (std_clustered >= 0) nclust += std_clustered;
  else {
    if ((st = std_domains(ctx, om, dna, ctx->fs_std_orfs, ctx->fs_std_pool, DomOpts(*prm, E_report), &nclust)) != BATH_OK) return st;
    clk.lap("fs: standard-branch domains");
  }
  if (n_clustered_regions) *n_clustered_regions = nclust;
  *domains = ctx->fs_domains.data(); *n_domains = (int64_t)ctx->fs_domains.size();
  return BATH_OK;
}

extern "C" const char *bath_hip_domain_cigars(const bath_hip_ctx *ctx) { return ctx ? ctx->cigars.c_str() : nullptr; }

// P7_DOMAIN.tr of every domain of the last pipeline call: the trace kernels' columns expanded into the reference's arrays
extern "C" int bath_hip_domain_traces(bath_hip_ctx *ctx, const bath_domain_trace **tr, int64_t *n_traces,
                                      const int8_t **st, const int32_t **k, const int32_t **i, const int8_t **c, const float **pp) {
  if (!ctx || !tr || !n_traces) return BATH_EINVAL;
  if (ctx->tr_recs.size() != ctx->fs_domains.size()) { ctx->set_error("no traces for the domains of the last call"); return BATH_EINVAL; }
  if (!ctx->tr_valid) {
    const size_t ncols = ctx->tr_codes.size();
    ctx->tr_out.resize(ctx->tr_recs.size());
    ctx->tr_st.resize(ncols); ctx->tr_c.resize(ncols); ctx->tr_k.resize(ncols); ctx->tr_i.resize(ncols);
    for (size_t d = 0; d < ctx->tr_recs.size(); d++) {
      const bath_hip_ctx::TraceRec &t = ctx->tr_recs[d];
      ctx->tr_out[d] = bath_domain_trace{t.col_off, t.ncol, t.win_start, t.orf_start, t.frameshift};
      int kk = t.k1 - 1, ii = t.i_first - 1;
      for (int z = 0; z < t.ncol; z++) {
        const size_t q = (size_t)t.col_off + (size_t)z;
        const int s = ctx->tr_codes[q] & 0xf, cl = (ctx->tr_codes[q] >> 4) & 0xf;
        if (s == 3)      { kk++; ii += cl; ctx->tr_st[q] = BATH_T_M; ctx->tr_k[q] = kk; ctx->tr_i[q] = ii; ctx->tr_c[q] = (int8_t)cl; }
        else if (s == 5) { ii += 3;        ctx->tr_st[q] = BATH_T_I; ctx->tr_k[q] = kk; ctx->tr_i[q] = ii; ctx->tr_c[q] = 0; }
        else             { kk++;           ctx->tr_st[q] = BATH_T_D; ctx->tr_k[q] = kk; ctx->tr_i[q] = t.d_i; ctx->tr_c[q] = 0; }
      }
    }
    ctx->tr_valid = true;
  }
  *tr = ctx->tr_out.data(); *n_traces = (int64_t)ctx->tr_out.size();
  if (st) *st = ctx->tr_st.data();
  if (k) *k = ctx->tr_k.data();
  if (i) *i = ctx->tr_i.data();
  if (c) *c = ctx->tr_c.data();
  if (pp) *pp = ctx->tr_pp.data();
  return BATH_OK;
}
