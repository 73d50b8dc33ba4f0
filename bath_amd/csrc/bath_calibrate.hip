// bath_calibrate.hip -- the frameshift Forward taus of a model, by simulation: what bathconvert adds to a HMMER3 file.
//
// Reference: p7_fs_Tau_3codons / p7_fs_Tau_5codons (src/evalues.c:608-770) as bathconvert calls them (src/bathconvert.c:128-162):
// N = 200 sequences of L = 100 amino acids drawn from the background, reverse-translated with a random synonymous codon each
// (p7_codontable_Create / _GetCodon, src/hmmer.c:197-273), scored by the 3-codon and the 5-codon Forward parsers in the multihit
// configuration of length L; a Gumbel fitted to the N bit scores; tau where the Gumbel's tail of mass <tailp> starts, moved back to
// the origin of the exponential tail.  Also p7_Builder_MaxLength (src/p7_builder.c:678), which bathconvert runs for a file without MAXL.
//
// And p7_Calibrate (src/evalues.c:64-199) for a model built in memory (bathbuild on a protein sequence): the MSV and Viterbi mus and the
// Forward tau from three sets of background sequences through the filter kernels, then the two taus above (bath_hip_calibrate, at
// the end of this file).
//
// Where it runs.  The two parsers are the device's work (bath_hip_fs3_forward_parser; bath_hip_fs5_forward_parser, the score-only
// instantiation of the regions' chain kernel).  The sampler is a strictly serial consumer of one random-number stream carried from
// model to model (2 x 200 x 200 steps per model) and its output is 60 KB per parser: host code.  So are the fit (200 numbers) and MAXL.
// bath_hip_calibrate_fs_batch fits several models with the windows of all of them in each parser launch (the batch kernels of
// bath_fs_chain.hip); it is told where it stands, behind the single-model calls.  bath_hip_calibrate_batch, at the very end, is
// bath_hip_calibrate for several models that start from one generator state: every sample set scored against all of them per launch.
//
// easel is not part of the reference tree, so esl_rsq_xfIID, esl_rnd_FChoose, esl_rnd_Roll, esl_stats_DMean, esl_gumbel_FitComplete
// and esl_gumbel_invcdf are restated from their published behaviour, as bath_ensemble.hip restates the generator.  The reference
// redraws a sequence whose odds-ratio parser overflows (eslERANGE, evalues.c:645, :740); the strict log-space kernels cannot
// overflow, so bath_hip_calibrate_fs redraws nothing.  bath_hip_calibrate_fs_arith runs the parsers in the reference's odds-ratio
// arithmetic (bath_hip_fs3_forward_parser in BATH_LOGSUM_ODDS, bath_hip_fs5_forward_parser_odds) and there the redraw applies:
// bath_calib_fit_scores is that loop, host code around a batch scoring callback.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "bath_common.hpp"
#include "bath_fs_device.hpp"
#include "bath_host_threads.hpp"
#include "bath_launch.hpp"
#include "host_model.hpp"

using namespace bath;

static constexpr float kEvparamUnset = -99999.0f;           // p7_EVPARAM_UNSET

// p7_codontable_Create: for each amino acid its codons in x, y, z order over ACGT; num[a] of them (at most 6)
static void codon_table(const uint8_t basic[64], uint8_t table[20][6], int num[20]) {
  for (int a = 0; a < 20; a++) num[a] = 0;
  for (int c = 0; c < 64; c++) {
    const int a = basic[c];
    if (a < 20 && num[a] < 6) table[a][num[a]++] = (uint8_t)c;
  }
}

// esl_rsq_xfIID: L draws of esl_rnd_FChoose (f is used as it stands: no esl_vec_FNorm; a roll beyond its sum is drawn again)
static void draw_amino(FastRng &rng, const float *f, int L, uint8_t *aa) {
  for (int i = 0; i < L; i++) {
    int a = -1;
    while (a < 0) {
      const float roll = (float)rng.next();
      float acc = 0.f;
      for (int q = 0; q < 20; q++) { acc += f[q]; if (roll < acc) { a = q; break; } }
    }
    aa[(size_t)i] = (uint8_t)a;
  }
}

extern "C" int bath_calib_sample_amino(uint32_t *rng_state, const float *f, int L, int N, uint8_t *aa) {
  if (!rng_state || (!aa && (int64_t)L * N > 0) || L < 0 || N < 0) return BATH_EINVAL;
  if (!f) f = kAminoBg;
  FastRng rng = FastRng::from_state(*rng_state);
  for (int s = 0; s < N; s++) draw_amino(rng, f, L, aa + (size_t)s * L);
  *rng_state = rng.x;
  return BATH_OK;
}

// N sequences of the stream from <rng>; dna NULL: the draws alone (the generator moves as if they had been stored)
static int sample_sets(FastRng &rng, const float *f, const uint8_t table[20][6], const int num[20], int L, int N, uint8_t *dna) {
  std::vector<uint8_t> aa((size_t)L);
  for (int s = 0; s < N; s++) {
    draw_amino(rng, f, L, aa.data());
    uint8_t *d = dna ? dna + (size_t)s * 3 * L : nullptr;
    for (int i = 0; i < L; i++) {                          // p7_codontable_GetCodon: esl_rnd_Roll(r, num_codons[a])
      const int a = aa[(size_t)i];
      if (num[a] == 0) return BATH_EINVAL;                 // (eslEINVAL: the table has no codon for a residue the background emits)
      const int x = (int)(rng.next() * num[a]);
      if (!d) continue;
      const int c = table[a][x];
      d[3 * i] = (uint8_t)(c >> 4); d[3 * i + 1] = (uint8_t)((c >> 2) & 3); d[3 * i + 2] = (uint8_t)(c & 3);
    }
  }
  return BATH_OK;
}

extern "C" int bath_calib_sample(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, uint8_t *dna) {
  if (!rng_state || !dna || L < 0 || N < 0) return BATH_EINVAL;
  if (!f) f = kAminoBg;
  uint8_t basic[64], table[20][6];
  int num[20];
  if (bath_gencode_basic(ncbi_table, basic) != BATH_OK) return BATH_EINVAL;
  codon_table(basic, table, num);
  FastRng rng = FastRng::from_state(*rng_state);
  const int st = sample_sets(rng, f, table, num, L, N, dna);
  if (st != BATH_OK) return st;
  *rng_state = rng.x;
  return BATH_OK;
}

// What a model that is passed over costs a file's carried generator (bathfetch without an index): the draws of <n_sets> sample
// sets, nothing stored.  The draw count of a sequence is not fixed (a roll beyond the frequencies' sum is drawn again), so the
// generator is stepped, not jumped.
extern "C" int bath_calib_skip(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, int n_sets) {
  if (!rng_state || L < 0 || N < 0 || n_sets < 0) return BATH_EINVAL;
  if (!f) f = kAminoBg;
  uint8_t basic[64], table[20][6];
  int num[20];
  if (bath_gencode_basic(ncbi_table, basic) != BATH_OK) return BATH_EINVAL;
  codon_table(basic, table, num);
  FastRng rng = FastRng::from_state(*rng_state);
  for (int s = 0; s < n_sets; s++) {
    const int st = sample_sets(rng, f, table, num, L, N, nullptr);
    if (st != BATH_OK) return st;
  }
  *rng_state = rng.x;
  return BATH_OK;
}

// evalues.c:633-649 (and :728-744): for (i = 0; i < N; i++) { sample; score; if (eslERANGE) { i--; continue; } xv[i] = ... }.  The
// sequence after a discarded one is drawn from where the generator stands after the discarded one, so the sequences the serial
// loop sees are ONE stream of draws, whatever their scores: the batch form draws what is still missing from that stream, scores
// it in one call, keeps the finite scores in order and counts the others; the next batch continues the stream.  It ends when N
// are kept, which is where the serial loop's generator ends (the last sequence drawn is a kept one in both).
extern "C" int bath_calib_fit_scores(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, bath_calib_score_fn score, void *user,
                                     float nullsc, double *xv, int *n_redrawn) {
  if (!rng_state || !score || !xv || L < 1 || N < 1) return BATH_EINVAL;
  std::vector<uint8_t> dna((size_t)N * 3 * L);
  std::vector<float> sc((size_t)N);
  uint32_t state = *rng_state;
  int kept = 0, redrawn = 0;
  if (n_redrawn) *n_redrawn = 0;
  while (kept < N) {
    const int need = N - kept;
    int st = bath_calib_sample(&state, f, ncbi_table, L, need, dna.data());
    if (st != BATH_OK) return st;
    if ((st = score(user, dna.data(), need, 3 * L, sc.data())) != BATH_OK) return st;
    for (int j = 0; j < need; j++) {
      if (!std::isfinite(sc[(size_t)j])) {
        if (n_redrawn) *n_redrawn = redrawn + 1;
        if (++redrawn > N) return BATH_ERANGE;             // (the reference would loop on)
        continue;
      }
      xv[kept++] = (sc[(size_t)j] - nullsc) / 0.69314718055994529;           // evalues.c:649: float difference, double quotient
    }
  }
  *rng_state = state;
  return BATH_OK;
}

// Lawless's equation 4.1.6 for the ML lambda of a Gumbel on complete data, and its derivative (esl_gumbel.c: lawless416)
static void lawless416(const double *x, int n, double lambda, double *ret_f, double *ret_df) {
  double esum = 0., xesum = 0., xxesum = 0., xsum = 0.;
  for (int i = 0; i < n; i++) {
    const double e = std::exp(-1. * lambda * x[i]);
    xsum += x[i]; xesum += x[i] * e; xxesum += x[i] * x[i] * e; esum += e;
  }
  *ret_f = (1. / lambda) - (xsum / n) + (xesum / esum);
  *ret_df = ((xesum / esum) * (xesum / esum)) - (xxesum / esum) - (1. / (lambda * lambda));
}

// esl_gumbel_FitComplete: method-of-moments start, Newton-Raphson on lawless416 until |f| < 1e-5 (a bisection if a hundred steps
// do not get there), mu from Lawless 4.1.5.  One Newton step is taken past the stopping rule: the step that meets it has usually
// landed at 1e-10 already, and when it has only just met it (|f| ~ 1e-5 leaves lambda 2e-6 off) the extra step does -- the value
// then is the root to double precision either way, where easel's may be 2e-6 off it (1e-5 in tau, a tenth of its last printed digit).
extern "C" int bath_gumbel_fit_complete(const double *x, int n, double *ret_mu, double *ret_lambda) {
  if (!x || n < 2 || !ret_mu || !ret_lambda) return BATH_EINVAL;
  double sum = 0., sqsum = 0.;
  for (int i = 0; i < n; i++) { sum += x[i]; sqsum += x[i] * x[i]; }
  const double variance = (sqsum - sum * sum / (double)n) / ((double)n - 1.);     // esl_stats_DMean
  if (!(variance > 0.)) return BATH_EINVAL;
  double lambda = 3.14159265358979323846264338328 / std::sqrt(6. * variance);
  double fx = 0., dfx = 0.;
  const double tol = 1e-5;
  int i;
  for (i = 0; i < 100; i++) {
    lawless416(x, n, lambda, &fx, &dfx);
    const bool met = std::fabs(fx) < tol;
    if (met && dfx == 0.) break;
    lambda = lambda - fx / dfx;
    if (lambda <= 0.) lambda = 0.001;
    if (met) break;
  }
  if (i == 100) {                                          // Newton-Raphson failed: bracket the root, then bisect
    double left = 0., right = 3.14159265358979323846264338328 / std::sqrt(6. * variance);
    lawless416(x, n, right, &fx, &dfx);
    while (fx > 0.) { right *= 2.; if (right > 100.) return BATH_ENORESULT; lawless416(x, n, right, &fx, &dfx); }
    for (i = 0; i < 100; i++) {
      const double mid = (left + right) / 2.;
      lawless416(x, n, mid, &fx, &dfx);
      if (std::fabs(fx) < tol) { left = right = mid; break; }
      if (fx > 0.) left = mid; else right = mid;
    }
    if (i == 100) return BATH_ENORESULT;
    lambda = (left + right) / 2.;
  }
  double esum = 0.;
  for (i = 0; i < n; i++) esum += std::exp(-lambda * x[i]);
  *ret_mu = -std::log(esum / n) / lambda;
  *ret_lambda = lambda;
  return BATH_OK;
}

// esl_gumbel_FitCompleteLoc: the ML location of a Gumbel of known lambda on complete data
extern "C" int bath_gumbel_fit_complete_loc(const double *x, int n, double lambda, double *ret_mu) {
  if (!x || n < 2 || !ret_mu || !(lambda > 0.)) return BATH_EINVAL;
  double esum = 0.;
  for (int i = 0; i < n; i++) esum += std::exp(-lambda * x[i]);
  *ret_mu = -1. * std::log(esum / n) / lambda;
  return BATH_OK;
}

extern "C" double bath_gumbel_invcdf(double p, double mu, double lambda) { return mu - (std::log(-1. * std::log(p)) / lambda); }

// evalues.c:658, :753
extern "C" int bath_calib_tau(const double *xv, int n, double lambda_model, double tailp, double *ret_tau) {
  double gmu = 0., glam = 0.;
  const int st = bath_gumbel_fit_complete(xv, n, &gmu, &glam);
  if (st != BATH_OK) return st;
  *ret_tau = bath_gumbel_invcdf(1.0 - tailp, gmu, glam) + (std::log(tailp) / lambda_model);
  return BATH_OK;
}

// p7_bg_SetLength(bg, L) then p7_bg_fs_NullOne (p7_bg.c:189, :377): the null score of L amino acids in any of three frames
extern "C" float bath_bg_fs_nullone(int L_amino) {
  const float p1 = (float)L_amino / (float)(L_amino + 1);
  const float per_frame = (float)((float)L_amino * std::log((double)p1) + std::log(1. - p1));
  return (float)(per_frame + std::log(3.0));
}

// p7_Builder_MaxLength (p7_builder.c:678): the length beyond which a sequence emitted by the core model has probability < emit_thresh
extern "C" int bath_hmm_max_length(const bath_hmm *hmm, double emit_thresh) {
  if (!hmm || hmm->M < 1) return -1;
  const int m = hmm->M;
  if (m == 1) return 1;
  enum { MM = 0, MI, MD, IM, II, DM, DD };
  auto t = [&](int k, int s) -> double { return (double)hmm->t[(size_t)k * 7 + s]; };
  const int length_bound = std::max(m, std::min(20 * m, 100000));
  std::vector<double> I((size_t)(m + 1) * 2, 0.), Mx((size_t)(m + 1) * 2, 0.), D((size_t)(m + 1) * 2, 0.);
  auto at = [](std::vector<double> &v, int k, int c) -> double & { return v[(size_t)k * 2 + c]; };
  at(Mx, 1, 0) = 1.0;
  at(D, 2, 0) = t(1, MD);
  for (int k = 3; k <= m; k++) at(D, k, 0) = t(k - 1, DD) * at(D, k - 1, 0);
  at(I, 1, 1) = t(1, MI) * at(Mx, 1, 0);
  at(Mx, 2, 1) = t(1, MM) * at(Mx, 1, 0);
  for (int k = 3; k <= m; k++) {
    at(Mx, k, 1) = t(k - 1, DM) * at(D, k - 1, 0);
    at(D, k, 1) = t(k - 1, MD) * at(Mx, k - 1, 1) + t(k - 1, DD) * at(D, k - 1, 1);
  }
  double p_sum = at(Mx, m, 0) + at(Mx, m, 1) + at(D, m, 0) + at(D, m, 1);
  int cp = 0;
  for (int col = 3; col <= length_bound; col++) {
    const int pp = 1 - cp;
    double surv = 0.0;
    at(Mx, 1, cp) = at(D, 1, cp) = 0;
    at(I, 1, cp) = t(1, II) * at(I, 1, pp);
    surv += at(I, 1, cp);
    for (int k = 2; k <= m; k++) {
      at(Mx, k, cp) = t(k - 1, MM) * at(Mx, k - 1, pp) + t(k - 1, DM) * at(D, k - 1, pp) + t(k - 1, IM) * at(I, k - 1, pp);
      at(I, k, cp) = t(k, MI) * at(Mx, k, pp) + t(k, II) * at(I, k, pp);
      at(D, k, cp) = t(k - 1, MD) * at(Mx, k - 1, cp) + t(k - 1, DD) * at(D, k - 1, cp);
      surv += at(I, k, cp) + at(Mx, k, cp) * (1 - t(k, MD)) + at(D, k, cp) * (1 - t(k, DD));
    }
    surv += at(Mx, m, cp) * t(m, MD) + at(D, m, cp) * t(m, DD) - at(I, m, cp);
    p_sum += at(Mx, m, cp) + at(D, m, cp);
    surv /= surv + p_sum;
    if (surv < emit_thresh) return col;
    cp = 1 - cp;
  }
  return length_bound;
}

namespace {
// what bath_calib_fit_scores calls back: one batch of sampled sequences through one parser of the odds-ratio calibration
struct CalibScore {
  bath_hip_ctx *ctx;
  const bath_hip_fsprofile *om;
  int cfg_len, kind;                                        // kind 0: fs3 odds, 1: fs5 strict, 2: fs5 odds
  std::vector<int64_t> off;
  bool failed;                                              // the parser refused (its message stands)
};
int calib_score(void *user, const uint8_t *dna, int n, int L3, float *sc) {
  CalibScore *c = static_cast<CalibScore *>(user);
  c->off.resize((size_t)n + 1);
  for (int i = 0; i <= n; i++) c->off[(size_t)i] = (int64_t)i * L3;
  bath_hip_seqs *sq = nullptr;
  int st = bath_hip_seqs_create(c->ctx, dna, c->off.data(), n, &sq);
  if (st == BATH_OK) st = c->kind == 0 ? bath_hip_fs3_forward_parser(c->ctx, c->om, sq, BATH_LOGSUM_ODDS, sc, nullptr, nullptr)
                        : c->kind == 1 ? bath_hip_fs5_forward_parser(c->ctx, c->om, sq, c->cfg_len, sc)
                                       : bath_hip_fs5_forward_parser_odds(c->ctx, c->om, sq, c->cfg_len, sc);
  if (sq) bath_hip_seqs_destroy(sq);
  if (st != BATH_OK) c->failed = true;
  return st;
}
}  // namespace

// keep_spans: the caller (bath_hip_calibrate) has recorded this model's standard filters on the context and wants them kept
// lambda_known: the slope the taus are anchored with; <= 0: the model's own float (bathconvert reads it from the file, bathconvert.c:128-162;
// p7_Calibrate hands its double on, evalues.c:142-143)
static int calibrate_fs_strict(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                               double *tau3, double *tau5, double *xv3, double *xv5, bool keep_spans = false, double lambda_known = 0.);
static int calibrate_fs_any(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                            double *tau3, double *tau5, double *xv3, double *xv5, int arith, int *redrawn, bool keep_spans, double lambda_known = 0.);

extern "C" int bath_hip_calibrate_fs(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                                     double *tau3, double *tau5, double *xv3, double *xv5) {
  return calibrate_fs_strict(ctx, hmm, ncbi_table, rng_state, L, N, tailp, tau3, tau5, xv3, xv5);
}

extern "C" int bath_hip_calibrate_fs_arith(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                                           double *tau3, double *tau5, double *xv3, double *xv5, int arith, int *redrawn) {
  return calibrate_fs_any(ctx, hmm, ncbi_table, rng_state, L, N, tailp, tau3, tau5, xv3, xv5, arith, redrawn, false);
}

static int calibrate_fs_any(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                            double *tau3, double *tau5, double *xv3, double *xv5, int arith, int *redrawn, bool keep_spans, double lambda_known) {
  if (!ctx) return BATH_EINVAL;
  if (arith < BATH_ARITH_STRICT || arith > BATH_ARITH_ODDS) { ctx->set_error("calibrate_fs: arith is 0 (strict), 1 (3-codon parser in odds ratios) or 2 (both parsers)"); return BATH_EINVAL; }
  if (redrawn) redrawn[0] = redrawn[1] = 0;
  if (arith == BATH_ARITH_STRICT) return calibrate_fs_strict(ctx, hmm, ncbi_table, rng_state, L, N, tailp, tau3, tau5, xv3, xv5, keep_spans, lambda_known);
  if (!hmm || !rng_state || !tau3 || !tau5 || L < 2 || N < 2 || !(tailp > 0. && tailp < 1.)) { ctx->set_error("calibrate_fs: needs a model, a generator state, L >= 2, N >= 2 and 0 < tailp < 1"); return BATH_EINVAL; }
  uint8_t basic[64];
  if (bath_gencode_basic(ncbi_table, basic) != BATH_OK) { ctx->set_error("calibrate_fs: unknown NCBI translation table " + std::to_string(ncbi_table)); return BATH_EINVAL; }
  if (!keep_spans) ctx->spans_reset();
  const float nullsc = bath_bg_fs_nullone(L);
  const double lambda = lambda_known > 0. ? lambda_known : (double)hmm->evparam[5];   // p7_FLAMBDA
  std::vector<double> own((size_t)N);
  uint32_t state = *rng_state;
  for (int pass = 0; pass < 2; pass++) {
    const int cl = pass == 0 ? 3 : 5;
    bath_fs_profile *gm = nullptr;
    bath_hip_fsprofile *om = nullptr;
    int st = bath_fs_profile_config(hmm, basic, cl, L, &gm);
    if (st == BATH_OK) st = bath_hip_fsprofile_convert(ctx, gm, &om);
    double *xv = pass == 0 ? (xv3 ? xv3 : own.data()) : (xv5 ? xv5 : own.data());
    int nre = 0;
    if (st == BATH_OK) {
      CalibScore cs{ctx, om, L, pass == 0 ? 0 : (arith == BATH_ARITH_ODDS ? 2 : 1), {}, false};
      st = bath_calib_fit_scores(&state, kAminoBg, ncbi_table, L, N, calib_score, &cs, nullsc, xv, &nre);
      if (st == BATH_ERANGE) ctx->set_error("calibrate_fs: more than N sampled sequences had no finite score in the " + std::to_string(cl) + "-codon model");
      else if (st == BATH_EINVAL && !cs.failed) ctx->set_error("calibrate_fs: translation table " + std::to_string(ncbi_table) + " has no codon for a background residue");
    }
    if (redrawn) redrawn[pass] = nre;
    if (om) bath_hip_fsprofile_destroy(om);
    if (gm) bath_fs_profile_destroy(gm);
    if (st != BATH_OK) return st;
    if ((st = bath_calib_tau(xv, N, lambda, tailp, pass == 0 ? tau3 : tau5)) != BATH_OK) { ctx->set_error("calibrate_fs: the Gumbel fit did not converge"); return st; }
  }
  *rng_state = state;
  return BATH_OK;
}

static int calibrate_fs_strict(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                               double *tau3, double *tau5, double *xv3, double *xv5, bool keep_spans, double lambda_known) {
  if (!ctx) return BATH_EINVAL;
  if (!hmm || !rng_state || !tau3 || !tau5 || L < 2 || N < 2 || !(tailp > 0. && tailp < 1.)) { ctx->set_error("calibrate_fs: needs a model, a generator state, L >= 2, N >= 2 and 0 < tailp < 1"); return BATH_EINVAL; }
  uint8_t basic[64];
  if (bath_gencode_basic(ncbi_table, basic) != BATH_OK) { ctx->set_error("calibrate_fs: unknown NCBI translation table " + std::to_string(ncbi_table)); return BATH_EINVAL; }
  if (!keep_spans) ctx->spans_reset();                     // bath_hip_kernel_times afterwards: this model's two parser launches
  const float nullsc = bath_bg_fs_nullone(L);
  const double lambda = lambda_known > 0. ? lambda_known : (double)hmm->evparam[5];   // p7_FLAMBDA
  std::vector<uint8_t> dna((size_t)N * 3 * L);
  std::vector<int64_t> off((size_t)N + 1);
  for (int i = 0; i <= N; i++) off[(size_t)i] = (int64_t)i * 3 * L;
  std::vector<float> sc((size_t)N);
  std::vector<double> own((size_t)N);
  uint32_t state = *rng_state;
  for (int pass = 0; pass < 2; pass++) {                   // bathconvert.c:157-161: the 3-codon fit, then the 5-codon fit, one generator
    const int cl = pass == 0 ? 3 : 5;
    bath_fs_profile *gm = nullptr;
    bath_hip_fsprofile *om = nullptr;
    bath_hip_seqs *sq = nullptr;
    int st = bath_fs_profile_config(hmm, basic, cl, L, &gm);
    if (st == BATH_OK) st = bath_hip_fsprofile_convert(ctx, gm, &om);
    if (st == BATH_OK && (st = bath_calib_sample(&state, kAminoBg, ncbi_table, L, N, dna.data())) != BATH_OK) ctx->set_error("calibrate_fs: translation table " + std::to_string(ncbi_table) + " has no codon for a background residue");
    if (st == BATH_OK) st = bath_hip_seqs_create(ctx, dna.data(), off.data(), N, &sq);
    if (st == BATH_OK) st = pass == 0 ? bath_hip_fs3_forward_parser(ctx, om, sq, BATH_LOGSUM_TABLE_SERIAL, sc.data(), nullptr, nullptr)
                                      : bath_hip_fs5_forward_parser(ctx, om, sq, L, sc.data());
    if (sq) bath_hip_seqs_destroy(sq);
    if (om) bath_hip_fsprofile_destroy(om);
    if (gm) bath_fs_profile_destroy(gm);
    if (st != BATH_OK) return st;
    double *xv = pass == 0 ? (xv3 ? xv3 : own.data()) : (xv5 ? xv5 : own.data());
    for (int i = 0; i < N; i++) {
      if (!std::isfinite(sc[(size_t)i])) { ctx->set_error("calibrate_fs: a sampled sequence has no path through the " + std::to_string(cl) + "-codon model (L too short)"); return BATH_ERANGE; }
      xv[i] = (sc[(size_t)i] - nullsc) / 0.69314718055994529;    // evalues.c:649: float difference, double quotient
    }
    if ((st = bath_calib_tau(xv, N, lambda, tailp, pass == 0 ? tau3 : tau5)) != BATH_OK) { ctx->set_error("calibrate_fs: the Gumbel fit did not converge"); return st; }
  }
  *rng_state = state;
  return BATH_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Several models per launch.  One model's 2 x N windows give each of its two parser launches N blocks of one working wave on as many
// CUs, and a launch lasts L x t_row whatever the other CUs could do meanwhile.  In strict arithmetic nothing a kernel
// computes feeds the generator, so the samples of a whole batch can be drawn before the first launch (bath_calib_sample_batch: the
// stream that successive bath_hip_calibrate_fs calls would draw, in their order), every profile built and uploaded, and the windows of
// all models scored by one launch per parser and per tiling present (fs3_fwd_batch_kernel, fs5_fwd_parser_batch_kernel: a block reads
// its model's FsBatchModel at blockIdx.y): the 3-codon launches on the context's stream, the 5-codon ones beside them on its side
// stream, one synchronize, then the fits.  The result is defined by what it equals -- the serial calls, bit for bit -- because every
// window's arithmetic is the single-model kernel's own source and a window's score depends on nothing but its model and itself.
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int bath_calib_sample_batch(uint32_t *rng_state, const float *f, const int *ncbi_tables, int n_models, int L, int N, uint8_t *dna) {
  if (!rng_state || !ncbi_tables || !dna || n_models < 0 || L < 0 || N < 0) return BATH_EINVAL;
  uint32_t state = *rng_state;
  const size_t set = (size_t)N * 3 * L;
  for (int k = 0; k < n_models; k++)
    for (int pass = 0; pass < 2; pass++) {                   // bathconvert.c:157-161: a model's 3-codon set, then its 5-codon set
      const int st = bath_calib_sample(&state, f, ncbi_tables[k], L, N, dna + ((size_t)k * 2 + pass) * set);
      if (st != BATH_OK) return st;
    }
  *rng_state = state;
  return BATH_OK;
}

namespace {
// the profiles and the windows of a batch, freed however the call ends
struct CalibBatch {
  std::vector<bath_fs_profile *> gm;
  std::vector<bath_hip_fsprofile *> om;
  bath_hip_seqs *sq = nullptr;
  ~CalibBatch() {
    if (sq) bath_hip_seqs_destroy(sq);
    for (bath_hip_fsprofile *o : om) if (o) bath_hip_fsprofile_destroy(o);
    for (bath_fs_profile *g : gm) if (g) bath_fs_profile_destroy(g);
  }
};
}  // namespace

// Stages 3 to 5 of a batch, for its two callers: the profiles, the uploads, the grouped launches, the copy and the fits.  <dna> holds
// <n_pairs> pairs of sample sets, [pair][3-codon set, 5-codon set][N][3L]; model k reads pair pair_of[k] and its fits are anchored
// with lambda[k].  bath_hip_calibrate_fs_batch: a pair per model (the generator is carried) and the model's float lambda;
// bath_hip_calibrate_batch: every model on the one pair (the generator is reseeded per model) and p7_Lambda's double.  <who> opens
// the messages; <basic>: 64 codes per model.  Every model has a job counter of its own, whoever shares its windows.  <queue_more>,
// if any, is called once the launches are queued and joined, before the one synchronize (the caller's own copies).  Writes its
// results only when every fit has succeeded.
static int calibrate_fs_sets(bath_hip_ctx *ctx, const char *who_call, const bath_hmm *const *hmms, const uint8_t *basic, int n_models,
                             const uint8_t *dna, int n_pairs, const int *pair_of, const double *lambda, int L, int N, double tailp,
                             double *tau3, double *tau5, double *xv3, double *xv5, const std::function<int()> *queue_more) {
  const std::string call = who_call;
  const int sets = 2 * n_models;                           // (model, parser): a profile, a job counter, N scores
  const int64_t nwin = (int64_t)2 * n_pairs * N, nsc = (int64_t)sets * N, L3 = 3 * (int64_t)L;
  // ---- 3. the 2 x n_models profiles: built on host threads (independent of each other, host code), uploaded by this one
  CalibBatch B;
  B.gm.assign((size_t)sets, nullptr); B.om.assign((size_t)sets, nullptr);
  {
    std::vector<int> status((size_t)sets, BATH_OK);
    std::atomic<int> next{0};
    auto build = [&] {
      for (int s = next.fetch_add(1); s < sets; s = next.fetch_add(1))
        status[(size_t)s] = bath_fs_profile_config(hmms[s / 2], &basic[(size_t)(s / 2) * 64], s % 2 == 0 ? 3 : 5, L, &B.gm[(size_t)s]);
    };
    const int T = std::min(sets, host_thread_count());
    if (T <= 1) build();
    else {
      std::vector<std::thread> th;
      for (int t = 0; t < T; t++) th.emplace_back(build);
      for (std::thread &t : th) t.join();
    }
    for (int s = 0; s < sets; s++)
      if (status[(size_t)s] != BATH_OK) { ctx->set_error(call + ": model at position " + std::to_string(s / 2) + " of the batch: the profile cannot be configured"); return status[(size_t)s]; }
  }
  for (int s = 0; s < sets; s++) {
    int st = bath_hip_fsprofile_convert(ctx, B.gm[(size_t)s], &B.om[(size_t)s]);
    if (st == BATH_OK) st = B.om[(size_t)s]->ensure_len(L + 1);
    if (st != BATH_OK) return st;
    bath_fs_profile_destroy(B.gm[(size_t)s]); B.gm[(size_t)s] = nullptr;      // (a 5-codon profile of 1280 nodes is 7 MB on the host)
  }
  {
    std::vector<int64_t> off((size_t)nwin + 1);
    for (int64_t i = 0; i <= nwin; i++) off[(size_t)i] = i * L3;
    const int st = bath_hip_seqs_create(ctx, dna, off.data(), nwin, &B.sq);
    if (st != BATH_OK) return st;
  }
  // ---- 4. the grouped launches.  One buffer: a job counter per (model, parser), the job order (every window of a set has the set's
  // length: the identity), the descriptors -- the 3-codon parser's by tiling, then the 5-codon parser's by tiling -- and behind them the scores
  std::vector<int> by_tiling((size_t)n_models);
  for (int k = 0; k < n_models; k++) by_tiling[(size_t)k] = k;
  auto tiling = [&](int k) { return BATH_TILING_PICK(BATH_FS_COLUMNS, hmms[k]->M); };
  std::stable_sort(by_tiling.begin(), by_tiling.end(), [&](int a, int b) { return tiling(a) < tiling(b); });
  const size_t o_order = (size_t)sets * sizeof(unsigned), o_desc = (o_order + (size_t)N * sizeof(int32_t) + 15) / 16 * 16;
  const size_t o_sc = o_desc + (size_t)sets * sizeof(FsBatchModel), total = o_sc + (size_t)nsc * sizeof(float);
  DevBuf &b_work = ctx->scratch[Scratch::kCalibBatchWork];
  BATH_HIP_TRY(ctx, b_work.reserve(total));
  char *d_base = b_work.as<char>();
  float *d_sc = reinterpret_cast<float *>(d_base + o_sc);
  std::vector<char> up(o_sc, 0);
  for (int i = 0; i < N; i++) reinterpret_cast<int32_t *>(up.data() + o_order)[i] = i;
  const SeqView all = B.sq->view();
  for (int pass = 0; pass < 2; pass++)
    for (int j = 0; j < n_models; j++) {
      const int k = by_tiling[(size_t)j], s = 2 * k + pass;
      const int64_t w0 = ((int64_t)2 * pair_of[k] + pass) * N;               // the first window of the set this parser reads
      const bath_hip_fsprofile *om = B.om[(size_t)s];
      FsBatchModel m{};
      m.dna = SeqView{all.data, all.off + w0, all.len + w0, N, nullptr};
      m.p = FsDev{om->M, om->pitch, om->maxcodons, om->d_rsc, om->d_tf, om->d_tb, om->d_logsum};
      m.loop_tab = om->d_loop[0]; m.move_tab = om->d_move[0];
      m.sc = d_sc + (int64_t)s * N;
      m.jobs = FsJobs{reinterpret_cast<const int32_t *>(d_base + o_order), reinterpret_cast<unsigned *>(d_base) + s};
      m.cfg_len = L;
      std::memcpy(up.data() + o_desc + ((size_t)pass * n_models + j) * sizeof(FsBatchModel), &m, sizeof m);
    }
  int st = ctx->stage_upload(Pinned::kCalibBatchUpload, d_base, up.data(), up.size(), ctx->stream);
  if (st != BATH_OK) return st;
  if ((st = fs_fork(ctx)) != BATH_OK) return st;            // the 5-codon launches on the side stream, beside the 3-codon ones
  const float tE = (float)-0.69314718055994529;             // multihit (modelconfig.c:825-831)
  const FsBatchModel *d_desc = reinterpret_cast<const FsBatchModel *>(d_base + o_desc);
  for (int pass = 0; pass < 2; pass++) {
    hipStream_t stream = pass == 0 ? ctx->stream : ctx->side_stream;
    for (int j0 = 0; j0 < n_models;) {
      const int Cv = tiling(by_tiling[(size_t)j0]);
      int j1 = j0, Mmax = 0;
      double nodes = 0.;
      for (; j1 < n_models && tiling(by_tiling[(size_t)j1]) == Cv; j1++) { const int M = hmms[by_tiling[(size_t)j1]]->M; Mmax = std::max(Mmax, M); nodes += M; }
      const int sp = ctx->span_begin(pass == 0 ? "fs3_fwd_batch_kernel" : "fs5_fwd_parser_batch_kernel", stream, nodes * N * (double)L3, (double)(j1 - j0) * N * (double)L3);
      st = pass == 0 ? launch_fs3_fwd_batch(ctx, stream, d_desc + j0, j1 - j0, Mmax, Cv, N, tE, tE)
                     : launch_fs5_fwd_parser_batch(ctx, stream, d_desc + n_models + j0, j1 - j0, Mmax, Cv, N, tE, tE);
      ctx->span_end(sp, stream);
      if (st != BATH_OK) break;
      j0 = j1;
    }
    if (st != BATH_OK) break;
  }
  const int stj = fs_join(ctx);                            // (also after a refused launch: the context's streams stay in step)
  // ---- 5. one synchronize, then the fits
  std::vector<float> sc((size_t)nsc);
  if (st == BATH_OK && stj == BATH_OK && hipMemcpyAsync(sc.data(), d_sc, (size_t)nsc * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { ctx->set_error(call + ": cannot copy the scores"); st = BATH_EFAIL; }
  if (st == BATH_OK && stj == BATH_OK && queue_more) st = (*queue_more)();
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (st != BATH_OK) return st;
  if (stj != BATH_OK) return stj;
  const float nullsc = bath_bg_fs_nullone(L);
  std::vector<double> xv((size_t)nsc), taus((size_t)sets);
  for (int s = 0; s < sets; s++) {
    const int cl = s % 2 == 0 ? 3 : 5;
    double *x = &xv[(size_t)s * N];
    for (int i = 0; i < N; i++) {
      const float v = sc[(size_t)s * N + i];
      if (!std::isfinite(v)) { ctx->set_error(call + ": model at position " + std::to_string(s / 2) + " of the batch: a sampled sequence has no path through the " + std::to_string(cl) + "-codon model (L too short)"); return BATH_ERANGE; }
      x[i] = (v - nullsc) / 0.69314718055994529;             // evalues.c:649: float difference, double quotient
    }
    if ((st = bath_calib_tau(x, N, lambda[s / 2], tailp, &taus[(size_t)s])) != BATH_OK) {
      ctx->set_error(call + ": model at position " + std::to_string(s / 2) + " of the batch: the Gumbel fit did not converge");
      return st;
    }
  }
  for (int k = 0; k < n_models; k++) {
    tau3[k] = taus[(size_t)2 * k]; tau5[k] = taus[(size_t)2 * k + 1];
    if (xv3) std::copy(&xv[(size_t)2 * k * N], &xv[(size_t)(2 * k + 1) * N], xv3 + (size_t)k * N);
    if (xv5) std::copy(&xv[(size_t)(2 * k + 1) * N], &xv[(size_t)(2 * k + 2) * N], xv5 + (size_t)k * N);
  }
  return BATH_OK;
}

extern "C" int bath_hip_calibrate_fs_batch(bath_hip_ctx *ctx, const bath_hmm *const *hmms, const int *ncbi_tables, int n_models,
                                           uint32_t *rng_state, int L, int N, double tailp,
                                           double *tau3, double *tau5, double *xv3, double *xv5) {
  if (!ctx) return BATH_EINVAL;
  // ---- 1. everything that can be refused, before anything is drawn or written
  if (n_models < 1 || n_models > BATH_CALIB_BATCH_MAX) { ctx->set_error("calibrate_fs_batch: a batch holds 1 to " + std::to_string(BATH_CALIB_BATCH_MAX) + " models (this one " + std::to_string(n_models) + ")"); return BATH_EINVAL; }
  if (!hmms || !ncbi_tables || !rng_state || !tau3 || !tau5 || L < 2 || N < 2 || !(tailp > 0. && tailp < 1.)) { ctx->set_error("calibrate_fs_batch: needs models, their tables, a generator state, L >= 2, N >= 2 and 0 < tailp < 1"); return BATH_EINVAL; }
  std::vector<uint8_t> basic((size_t)n_models * 64);
  for (int k = 0; k < n_models; k++) {
    const std::string who = "calibrate_fs_batch: model at position " + std::to_string(k) + " of the batch: ";
    if (!hmms[k] || hmms[k]->M < 1) { ctx->set_error(who + "no model"); return BATH_EINVAL; }
    if (hmms[k]->M > kFsMaxNodes) { ctx->set_error(who + "frameshift kernels support models up to " + std::to_string(kFsMaxNodes) + " nodes (this one has " + std::to_string(hmms[k]->M) + ")"); return BATH_EINVAL; }
    if (bath_gencode_basic(ncbi_tables[k], &basic[(size_t)k * 64]) != BATH_OK) { ctx->set_error(who + "unknown NCBI translation table " + std::to_string(ncbi_tables[k])); return BATH_EINVAL; }
  }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->spans_reset();                                      // bath_hip_kernel_times afterwards: the batch's launches
  // ---- 2. the samples: [model][3-codon set, 5-codon set][N][3L]
  const int sets = 2 * n_models;
  const int64_t nwin = (int64_t)sets * N, L3 = 3 * (int64_t)L;
  std::vector<uint8_t> dna((size_t)nwin * L3);
  uint32_t state = *rng_state;
  for (int k = 0; k < n_models; k++) {                     // (model by model only to name the one whose table fails)
    if (bath_calib_sample_batch(&state, kAminoBg, ncbi_tables + k, 1, L, N, dna.data() + (size_t)k * 2 * N * L3) != BATH_OK) {
      ctx->set_error("calibrate_fs_batch: model at position " + std::to_string(k) + " of the batch: translation table " + std::to_string(ncbi_tables[k]) + " has no codon for a background residue");
      return BATH_EINVAL;
    }
  }
  // ---- 3. to 5.: a pair of sets per model, the slope the model's file gives (bathconvert.c:128-162)
  std::vector<int> pair_of((size_t)n_models);
  std::vector<double> lambda((size_t)n_models);
  for (int k = 0; k < n_models; k++) { pair_of[(size_t)k] = k; lambda[(size_t)k] = (double)hmms[k]->evparam[5]; }   // p7_FLAMBDA
  const int st = calibrate_fs_sets(ctx, "calibrate_fs_batch", hmms, basic.data(), n_models, dna.data(), n_models, pair_of.data(), lambda.data(), L, N, tailp,
                                   tau3, tau5, xv3, xv5, nullptr);
  if (st != BATH_OK) return st;
  *rng_state = state;
  return BATH_OK;
}

// Several models, each from a generator state of its own (bathfetch: with an index every key starts from a fresh generator; without
// one the caller has walked the file's generator to each selected model with bath_calib_skip).  Models with one (state, table) read
// one pair of sets: the sets are drawn once per distinct pair, in the order of first appearance.
extern "C" int bath_hip_calibrate_fs_batch_at(bath_hip_ctx *ctx, const bath_hmm *const *hmms, const int *ncbi_tables, int n_models,
                                              const uint32_t *states_in, uint32_t *states_out, int L, int N, double tailp,
                                              double *tau3, double *tau5, double *xv3, double *xv5) {
  if (!ctx) return BATH_EINVAL;
  // ---- 1. everything that can be refused, before anything is drawn or written
  if (n_models < 1 || n_models > BATH_CALIB_BATCH_MAX) { ctx->set_error("calibrate_fs_batch_at: a batch holds 1 to " + std::to_string(BATH_CALIB_BATCH_MAX) + " models (this one " + std::to_string(n_models) + ")"); return BATH_EINVAL; }
  if (!hmms || !ncbi_tables || !states_in || !states_out || !tau3 || !tau5 || L < 2 || N < 2 || !(tailp > 0. && tailp < 1.)) { ctx->set_error("calibrate_fs_batch_at: needs models, their tables, a generator state per model in and out, L >= 2, N >= 2 and 0 < tailp < 1"); return BATH_EINVAL; }
  std::vector<uint8_t> basic((size_t)n_models * 64);
  for (int k = 0; k < n_models; k++) {
    const std::string who = "calibrate_fs_batch_at: model at position " + std::to_string(k) + " of the batch: ";
    if (!hmms[k] || hmms[k]->M < 1) { ctx->set_error(who + "no model"); return BATH_EINVAL; }
    if (hmms[k]->M > kFsMaxNodes) { ctx->set_error(who + "frameshift kernels support models up to " + std::to_string(kFsMaxNodes) + " nodes (this one has " + std::to_string(hmms[k]->M) + ")"); return BATH_EINVAL; }
    if (bath_gencode_basic(ncbi_tables[k], &basic[(size_t)k * 64]) != BATH_OK) { ctx->set_error(who + "unknown NCBI translation table " + std::to_string(ncbi_tables[k])); return BATH_EINVAL; }
  }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->spans_reset();                                      // bath_hip_kernel_times afterwards: the batch's launches
  // ---- 2. the samples: [pair][3-codon set, 5-codon set][N][3L], a pair per distinct (state, table)
  const int64_t L3 = 3 * (int64_t)L;
  const size_t pair_bytes = (size_t)2 * N * L3;
  std::vector<int> pair_of((size_t)n_models), first_of;    // first_of[p]: the first model that reads pair p
  std::vector<uint32_t> after;                             // after[p]: the generator behind pair p
  std::vector<uint8_t> dna;
  for (int k = 0; k < n_models; k++) {
    int p = 0;
    for (; p < (int)first_of.size(); p++)
      if (states_in[first_of[(size_t)p]] == states_in[k] && ncbi_tables[first_of[(size_t)p]] == ncbi_tables[k]) break;
    if (p == (int)first_of.size()) {
      first_of.push_back(k);
      dna.resize((size_t)(p + 1) * pair_bytes);
      uint32_t state = states_in[k];
      if (bath_calib_sample_batch(&state, kAminoBg, ncbi_tables + k, 1, L, N, dna.data() + (size_t)p * pair_bytes) != BATH_OK) {
        ctx->set_error("calibrate_fs_batch_at: model at position " + std::to_string(k) + " of the batch: translation table " + std::to_string(ncbi_tables[k]) + " has no codon for a background residue");
        return BATH_EINVAL;
      }
      after.push_back(state);
    }
    pair_of[(size_t)k] = p;
  }
  // ---- 3. to 5.: the slope the model's file gives (bathfetch.c:321-325)
  std::vector<double> lambda((size_t)n_models);
  for (int k = 0; k < n_models; k++) lambda[(size_t)k] = (double)hmms[k]->evparam[5];   // p7_FLAMBDA
  const int st = calibrate_fs_sets(ctx, "calibrate_fs_batch_at", hmms, basic.data(), n_models, dna.data(), (int)first_of.size(), pair_of.data(), lambda.data(), L, N, tailp,
                                   tau3, tau5, xv3, xv5, nullptr);
  if (st != BATH_OK) return st;
  for (int k = 0; k < n_models; k++) states_out[k] = after[(size_t)pair_of[(size_t)k]];
  return BATH_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// p7_Calibrate (evalues.c:64-199) for a model built in memory: lambda, the MSV and Viterbi mus, the Forward tau, then the two
// frameshift taus from the same generator.
//
// The three standard sample sets (EmN x EmL, EvN x EvL, EfN x EfL residues, drawn in that order: evalues.c:119-121) depend on
// nothing a kernel computes, and a builder that reseeds its generator for every model (p7_builder.c:130-131, evalues.c:94-95)
// draws the same three for every model: bath_hip_calib_samples holds them on the device with the buffers the fits need, made
// once per run.  A model's three filters are queued on the context's stream one after another and their scores and statuses
// come back in one batch of copies behind them: one synchronize per model.  p7_MSVFilter is the SSV filter first and the full MSV
// filter for the sequences SSV cannot decide (eslENORESULT, msvfilter.c:90): those few, if any, take a second launch.
// ---------------------------------------------------------------------------------------------------------------------------
struct bath_hip_calib_samples {
  bath_hip_ctx *ctx = nullptr;
  int L[3] = {0, 0, 0}, N[3] = {0, 0, 0};                  // MSV, Viterbi, Forward
  uint32_t state_before = 0, state_after = 0;              // the generator before the first draw and after the last
  bath_hip_seqs *sq[3] = {nullptr, nullptr, nullptr};
  DevBuf order[2], v, sc[3], st[3], todo;                  // identity orders (every sequence of a set has the set's length), SSV maxima, results
};

extern "C" void bath_hip_calib_samples_destroy(bath_hip_calib_samples *S) {
  if (!S) return;
  if (S->ctx) (void)hipSetDevice(S->ctx->device);
  for (bath_hip_seqs *q : S->sq) if (q) bath_hip_seqs_destroy(q);
  for (DevBuf &b : S->order) b.release();
  for (DevBuf &b : S->sc) b.release();
  for (DevBuf &b : S->st) b.release();
  S->v.release(); S->todo.release();
  delete S;
}

static int calib_samples_create(bath_hip_ctx *ctx, uint32_t *rng_state, const int L[3], const int N[3], bath_hip_calib_samples **ret) {
  *ret = nullptr;
  for (int s = 0; s < 3; s++)
    if (L[s] < 1 || N[s] < 2 || (int64_t)L[s] * N[s] > (int64_t)1 << 28) { ctx->set_error("calibrate: every sample set needs a length >= 1 and at least 2 sequences (and at most 2^28 residues)"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  bath_hip_calib_samples *S = new bath_hip_calib_samples();
  S->ctx = ctx;
  S->state_before = *rng_state;
  uint32_t state = *rng_state;
  int st = BATH_OK;
  for (int s = 0; s < 3 && st == BATH_OK; s++) {
    S->L[s] = L[s]; S->N[s] = N[s];
    std::vector<uint8_t> aa((size_t)L[s] * N[s]);
    std::vector<int64_t> off((size_t)N[s] + 1);
    for (int i = 0; i <= N[s]; i++) off[(size_t)i] = (int64_t)i * L[s];
    st = bath_calib_sample_amino(&state, kAminoBg, L[s], N[s], aa.data());
    if (st == BATH_OK) st = bath_hip_seqs_create(ctx, aa.data(), off.data(), N[s], &S->sq[s]);
    if (st == BATH_OK && (S->sc[s].reserve((size_t)N[s] * sizeof(float)) != hipSuccess || S->st[s].reserve((size_t)N[s] * sizeof(int32_t)) != hipSuccess)) st = BATH_EMEM;
  }
  for (int s = 0; s < 2 && st == BATH_OK; s++) {
    std::vector<int32_t> order((size_t)N[s]);
    for (int i = 0; i < N[s]; i++) order[(size_t)i] = i;
    if (S->order[s].reserve(order.size() * sizeof(int32_t) + 16) != hipSuccess) { st = BATH_EMEM; break; }
    if (hipMemcpy(S->order[s].p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) st = BATH_EFAIL;
  }
  if (st == BATH_OK && (S->v.reserve((size_t)N[0] * sizeof(int16_t)) != hipSuccess || S->todo.reserve((size_t)N[0] * sizeof(int32_t)) != hipSuccess)) st = BATH_EMEM;
  if (st != BATH_OK) {
    if (st == BATH_EMEM || st == BATH_EFAIL) ctx->set_error("calibrate: cannot place the sample sets on the device");
    bath_hip_calib_samples_destroy(S);
    return st;
  }
  S->state_after = state;
  *rng_state = state;
  *ret = S;
  return BATH_OK;
}

extern "C" int bath_hip_calib_samples_create(bath_hip_ctx *ctx, uint32_t *rng_state, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN,
                                             bath_hip_calib_samples **ret) {
  if (!ctx) return BATH_EINVAL;
  if (!rng_state || !ret) { ctx->set_error("calib_samples_create: needs a generator state and a place for the handle"); return BATH_EINVAL; }
  const int L[3] = {EmL, EvL, EfL}, N[3] = {EmN, EvN, EfN};
  return calib_samples_create(ctx, rng_state, L, N, ret);
}

// the three standard fits of one model on the resident sets: mu[0] MSV, mu[1] Viterbi, mu[2] the Forward tau; xv: NULL or
// N[0] + N[1] + N[2] bit scores, set after set
static int calibrate_std(bath_hip_ctx *ctx, const bath_hip_oprofile *om, bath_hip_calib_samples *S, double lambda, double tailp, double mu[3], double *xv) {
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = om->ensure_len_tables(std::max(S->L[0], std::max(S->L[1], S->L[2])));
  if (st != BATH_OK) return st;
  const double M = (double)om->M;
  const bath_hip_seqs *qm = S->sq[0], *qv = S->sq[1], *qf = S->sq[2];
  int sp = ctx->span_begin("calib_msv", ctx->stream, M * S->L[0] * S->N[0], 0.);
  if ((st = launch_ssv_lane(ctx, om, qm->view(), S->order[0].as<int32_t>(), S->v.as<int16_t>())) != BATH_OK) return st;
  if ((st = launch_ssv_classify(ctx, om, qm->n, qm->d_len, S->v.as<int16_t>(), S->sc[0].as<float>(), S->st[0].as<int32_t>())) != BATH_OK) return st;
  ctx->span_end(sp, ctx->stream);
  sp = ctx->span_begin("calib_vit", ctx->stream, M * S->L[1] * S->N[1], 0.);
  st = vit_lane_supported(om) ? launch_vit_lane(ctx, om, qv->view(), S->order[1].as<int32_t>(), qv->n, nullptr, S->sc[1].as<float>(), S->st[1].as<int32_t>(), nullptr)
                              : launch_vit_wave(ctx, om, qv->view(), nullptr, qv->n, S->sc[1].as<float>(), S->st[1].as<int32_t>(), nullptr, nullptr);
  if (st != BATH_OK) return st;
  ctx->span_end(sp, ctx->stream);
  sp = ctx->span_begin("calib_fwd", ctx->stream, M * S->L[2] * S->N[2], 0.);
  if ((st = launch_fwd_wave(ctx, om, qf->view(), nullptr, qf->n, S->sc[2].as<float>(), S->st[2].as<int32_t>(), nullptr)) != BATH_OK) return st;
  ctx->span_end(sp, ctx->stream);

  std::vector<float> sc[3];
  std::vector<int32_t> status[3];
  for (int s = 0; s < 3; s++) {
    sc[s].resize((size_t)S->N[s]); status[s].resize((size_t)S->N[s]);
    BATH_HIP_TRY(ctx, hipMemcpyAsync(sc[s].data(), S->sc[s].p, (size_t)S->N[s] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(status[s].data(), S->st[s].p, (size_t)S->N[s] * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> todo;
  for (int i = 0; i < S->N[0]; i++) if (status[0][(size_t)i] == BATH_ENORESULT) todo.push_back(i);
  if (!todo.empty()) {                                     // msvfilter.c:90: SSV could not decide, the full MSV filter does
    BATH_HIP_TRY(ctx, hipMemcpyAsync(S->todo.p, todo.data(), todo.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    sp = ctx->span_begin("calib_msv", ctx->stream, 0., 0.);
    if ((st = launch_msv_wave(ctx, om, qm->view(), S->todo.as<int32_t>(), (int64_t)todo.size(), S->sc[0].as<float>(), S->st[0].as<int32_t>(), nullptr)) != BATH_OK) return st;
    ctx->span_end(sp, ctx->stream);
    BATH_HIP_TRY(ctx, hipMemcpyAsync(sc[0].data(), S->sc[0].p, (size_t)S->N[0] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(status[0].data(), S->st[0].p, (size_t)S->N[0] * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }

  const float maxsc[2] = {(float)((255 - om->base_b) / om->scale_b),            // evalues.c:305
                          (float)((32767.0 - om->base_w) / om->scale_w)};        // evalues.c:374
  static const char *const kWhat[3] = {"msv mu", "vit mu", "fwd tau"};
  std::vector<double> x;
  for (int s = 0; s < 3; s++) {
    const float nullsc = om->lt.h_nullsc[(size_t)S->L[s]];                       // p7_bg_SetLength(bg, L) + p7_bg_NullOne
    x.assign((size_t)S->N[s], 0.);
    for (int i = 0; i < S->N[s]; i++) {
      float v = sc[s][(size_t)i];
      const int32_t code = status[s][(size_t)i];
      if (code == BATH_ERANGE && s < 2) v = maxsc[s];
      else if (code != BATH_OK) { ctx->set_error(std::string("failed to determine ") + kWhat[s] + ": a sampled sequence's filter returned status " + std::to_string(code)); return code == BATH_ERANGE ? BATH_ERANGE : BATH_EFAIL; }
      x[(size_t)i] = (v - nullsc) / 0.69314718055994529;                          // float difference, double quotient
    }
    st = s < 2 ? bath_gumbel_fit_complete_loc(x.data(), S->N[s], lambda, &mu[s]) : bath_calib_tau(x.data(), S->N[s], lambda, tailp, &mu[s]);
    if (st != BATH_OK) { ctx->set_error(std::string("failed to determine ") + kWhat[s] + ": the fit did not converge"); return st; }
    if (xv) { std::copy(x.begin(), x.end(), xv); xv += S->N[s]; }
  }
  return BATH_OK;
}

// fs: the two frameshift taus behind the three standard fits (bath_hip_calibrate); without them (bath_hip_calibrate_std) no
// frameshift sample is drawn, no parser launched, and the two taus are left unset
static int calibrate_model(bath_hip_ctx *ctx, bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, bath_hip_calib_samples *samples,
                           int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, int arith, double *xv, int *redrawn, bool fs) {
  if (!ctx) return BATH_EINVAL;
  if (!hmm || hmm->M < 1 || !rng_state || !(Eft > 0. && Eft < 1.)) { ctx->set_error("calibrate: needs a model, a generator state and 0 < Eft < 1"); return BATH_EINVAL; }
  if (arith < BATH_ARITH_STRICT || arith > BATH_ARITH_ODDS) { ctx->set_error("calibrate: arith is 0 (strict), 1 (3-codon parser in odds ratios) or 2 (both parsers)"); return BATH_EINVAL; }
  if (!fs && hmm->M > kCascadeMaxNodes) {                  // before anything is drawn or launched (with fs the parsers' own limit is lower)
    ctx->set_error("calibrate: the filter cascade supports models up to " + std::to_string(kCascadeMaxNodes) + " nodes (this one has " + std::to_string(hmm->M) + ")");
    return BATH_EINVAL;
  }
  const int L[3] = {EmL, EvL, EfL}, N[3] = {EmN, EvN, EfN};
  uint32_t state = *rng_state;
  bath_hip_calib_samples *S = samples, *own = nullptr;
  if (S) {
    if (S->ctx != ctx || std::memcmp(S->L, L, sizeof L) || std::memcmp(S->N, N, sizeof N) || S->state_before != state) {
      ctx->set_error("calibrate: the resident sample sets were drawn for another context, other lengths or counts, or from another generator state");
      return BATH_EINVAL;
    }
    state = S->state_after;
  } else {
    const int st = calib_samples_create(ctx, &state, L, N, &own);
    if (st != BATH_OK) return st;
    S = own;
  }
  ctx->spans_reset();                                      // bath_hip_kernel_times afterwards: this model's filters and parsers
  bath_profile *gm = nullptr;
  bath_hip_oprofile *om = nullptr;
  int st = bath_profile_config(hmm, EvL, &gm);             // evalues.c:109 (the length does not matter: every fit sets its own)
  if (st == BATH_OK) st = bath_hip_oprofile_convert(ctx, gm, &om);
  const double lambda = bath_hmm_lambda(hmm);              // p7_Lambda
  double mu[3] = {0., 0., 0.};
  if (st == BATH_OK) st = calibrate_std(ctx, om, S, lambda, Eft, mu, xv);
  if (om) bath_hip_oprofile_destroy(om);
  if (gm) bath_profile_destroy(gm);
  if (own) bath_hip_calib_samples_destroy(own);
  if (st != BATH_OK) return st;
  float ev[BATH_NEVPARAM];
  std::memcpy(ev, hmm->evparam, sizeof ev);
  hmm->evparam[1] = hmm->evparam[3] = hmm->evparam[5] = (float)lambda;           // evalues.c:148-153
  hmm->evparam[0] = (float)mu[0]; hmm->evparam[2] = (float)mu[1]; hmm->evparam[4] = (float)mu[2];
  if (!fs) {                                               // evalues.c:124-155 without hmm->fs: the standard fits are the whole call
    hmm->evparam[6] = hmm->evparam[7] = kEvparamUnset;
    *rng_state = state;
    return BATH_OK;
  }
  double tau3 = 0., tau5 = 0.;
  double *xv3 = xv ? xv + EmN + EvN + EfN : nullptr, *xv5 = xv3 ? xv3 + EfN : nullptr;
  st = calibrate_fs_any(ctx, hmm, ncbi_table, &state, EfL, EfN, Eft, &tau3, &tau5, xv3, xv5, arith, redrawn, true, lambda);
  if (st != BATH_OK) { std::memcpy(hmm->evparam, ev, sizeof ev); return st; }
  hmm->evparam[6] = (float)tau3; hmm->evparam[7] = (float)tau5;
  *rng_state = state;
  return BATH_OK;
}

extern "C" int bath_hip_calibrate(bath_hip_ctx *ctx, bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, bath_hip_calib_samples *samples,
                                  int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, int arith, double *xv, int *redrawn) {
  return calibrate_model(ctx, hmm, ncbi_table, rng_state, samples, EmL, EmN, EvL, EvN, EfL, EfN, Eft, arith, xv, redrawn, true);
}

extern "C" int bath_hip_calibrate_std(bath_hip_ctx *ctx, bath_hmm *hmm, uint32_t *rng_state, bath_hip_calib_samples *samples,
                                      int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv) {
  return calibrate_model(ctx, hmm, 0, rng_state, samples, EmL, EmN, EvL, EvN, EfL, EfN, Eft, BATH_ARITH_STRICT, xv, nullptr, false);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Several models per call, for a builder that reseeds its generator for every model (p7_builder.c:130-131, evalues.c:94-95): every
// model starts from the same state, so all of them read the three resident standard sets and, with one translation table for the
// run, the same two frameshift sets behind them -- five shared sample sets against n_models models.  (bath_hip_calibrate_fs_batch
// is the other rule: the generator carried from model to model, a pair of frameshift sets each.)  Per standard filter and per tiling
// present one launch scores the set against the models of that tiling (bath_calib_batch.hip: the wave kernels' own text, a block's
// model at blockIdx.y; the full MSV kernel for every target, which scores what SSV and its classification decide alone, and the
// wave kernel's Viterbi, which is the lane kernel's int16 recurrence); the two frameshift parsers follow as calibrate_fs_sets
// queues them, the standard scores come back behind them, one synchronize, then the fits.  Defined by what it equals: n_models
// calls of bath_hip_calibrate in strict arithmetic, each from the same state, bit for bit.  All or nothing.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
struct StdBatch {
  std::vector<bath_hip_oprofile *> om;
  ~StdBatch() { for (bath_hip_oprofile *o : om) if (o) bath_hip_oprofile_destroy(o); }
};
}  // namespace

// fs: as calibrate_model's.  Without it (bath_hip_calibrate_std_batch) the batch is the three standard launches per tiling, the
// copies behind them and one synchronize; the limit is the wave kernels' own, not the frameshift kernels'.
static int calibrate_models(bath_hip_ctx *ctx, bath_hmm *const *hmms, int n_models, int ncbi_table, uint32_t *rng_state,
                            bath_hip_calib_samples *samples, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv, bool fs) {
  if (!ctx) return BATH_EINVAL;
  // ---- 1. everything that can be refused, before anything is drawn, launched or written
  if (n_models < 1 || n_models > BATH_CALIB_BATCH_MAX) { ctx->set_error("calibrate_batch: a batch holds 1 to " + std::to_string(BATH_CALIB_BATCH_MAX) + " models (this one " + std::to_string(n_models) + ")"); return BATH_EINVAL; }
  if (!hmms || !rng_state || !(Eft > 0. && Eft < 1.)) { ctx->set_error("calibrate_batch: needs models, a generator state and 0 < Eft < 1"); return BATH_EINVAL; }
  for (int k = 0; k < n_models; k++) {
    const std::string who = "calibrate_batch: model at position " + std::to_string(k) + " of the batch: ";
    if (!hmms[k] || hmms[k]->M < 1) { ctx->set_error(who + "no model"); return BATH_EINVAL; }
    if (fs && hmms[k]->M > kFsMaxNodes) { ctx->set_error(who + "frameshift kernels support models up to " + std::to_string(kFsMaxNodes) + " nodes (this one has " + std::to_string(hmms[k]->M) + ")"); return BATH_EINVAL; }
    if (hmms[k]->M > kCascadeMaxNodes) { ctx->set_error(who + "the filter cascade supports models up to " + std::to_string(kCascadeMaxNodes) + " nodes (this one has " + std::to_string(hmms[k]->M) + ")"); return BATH_EINVAL; }
  }
  std::vector<uint8_t> basic((size_t)n_models * 64);
  if (fs && bath_gencode_basic(ncbi_table, basic.data()) != BATH_OK) { ctx->set_error("calibrate_batch: unknown NCBI translation table " + std::to_string(ncbi_table)); return BATH_EINVAL; }
  for (int k = 1; k < n_models; k++) std::memcpy(&basic[(size_t)k * 64], basic.data(), 64);
  const int L[3] = {EmL, EvL, EfL}, N[3] = {EmN, EvN, EfN};
  bath_hip_calib_samples *S = samples;
  if (!S) { ctx->set_error("calibrate_batch: needs the resident sample sets (bath_hip_calib_samples_create)"); return BATH_EINVAL; }
  if (S->ctx != ctx || std::memcmp(S->L, L, sizeof L) || std::memcmp(S->N, N, sizeof N) || S->state_before != *rng_state) {
    ctx->set_error("calibrate: the resident sample sets were drawn for another context, other lengths or counts, or from another generator state");
    return BATH_EINVAL;
  }
  if (fs && EfL < 2) { ctx->set_error("calibrate_batch: the frameshift fits need EfL >= 2"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->spans_reset();                                      // bath_hip_kernel_times afterwards: this batch's launches
  // ---- 2. the two frameshift sets every model reads: drawn once, behind the standard sets
  uint32_t state = S->state_after;
  const size_t fs_set = fs ? (size_t)EfN * 3 * EfL : 0;
  std::vector<uint8_t> dna(2 * fs_set);
  for (int pass = 0; fs && pass < 2; pass++)
    if (bath_calib_sample(&state, kAminoBg, ncbi_table, EfL, EfN, dna.data() + (size_t)pass * fs_set) != BATH_OK) {
      ctx->set_error("calibrate_batch: translation table " + std::to_string(ncbi_table) + " has no codon for a background residue");
      return BATH_EINVAL;
    }
  // ---- 3. the standard profiles, their length tables, the models by tiling (Forward: and by where its tables lie)
  StdBatch B;
  B.om.assign((size_t)n_models, nullptr);
  const int maxL = std::max(L[0], std::max(L[1], L[2]));
  for (int k = 0; k < n_models; k++) {
    bath_profile *gm = nullptr;
    int st = bath_profile_config(hmms[k], EvL, &gm);       // evalues.c:109 (the length does not matter: every fit sets its own)
    if (st == BATH_OK) st = bath_hip_oprofile_convert(ctx, gm, &B.om[(size_t)k]);
    if (gm) bath_profile_destroy(gm);
    if (st == BATH_OK) st = B.om[(size_t)k]->ensure_len_tables(maxL);
    if (st != BATH_OK) return st;
  }
  auto tiling = [&](int k) { return BATH_TILING_PICK(BATH_WAVE_COLUMNS, hmms[k]->M); };
  auto key = [&](int k) { return 2 * tiling(k) + (fwd_wave_global_tables(B.om[(size_t)k]) ? 1 : 0); };
  std::vector<int> by_tiling((size_t)n_models);
  for (int k = 0; k < n_models; k++) by_tiling[(size_t)k] = k;
  std::stable_sort(by_tiling.begin(), by_tiling.end(), [&](int a, int b) { return key(a) < key(b); });
  // ---- 4. one buffer: the descriptors in launch order, behind them every model's scores and statuses, set after set
  const int64_t per_model = (int64_t)N[0] + N[1] + N[2], nres = per_model * n_models;
  const size_t desc = std_batch_model_bytes(), o_sc = ((size_t)n_models * desc + 15) / 16 * 16, o_st = o_sc + (size_t)nres * sizeof(float);
  DevBuf &b_work = ctx->scratch[Scratch::kCalibStdBatchWork];
  BATH_HIP_TRY(ctx, b_work.reserve(o_st + (size_t)nres * sizeof(int32_t)));
  char *d_base = b_work.as<char>();
  float *d_sc = reinterpret_cast<float *>(d_base + o_sc);
  int32_t *d_st = reinterpret_cast<int32_t *>(d_base + o_st);
  std::vector<char> up((size_t)n_models * desc, 0);
  for (int j = 0; j < n_models; j++) {
    const int k = by_tiling[(size_t)j];
    float *sc3[3]; int32_t *st3[3];
    int64_t at = (int64_t)k * per_model;
    for (int s = 0; s < 3; s++) { sc3[s] = d_sc + at; st3[s] = d_st + at; at += N[s]; }
    std_batch_model_fill(up.data() + (size_t)j * desc, B.om[(size_t)k], sc3, st3);
  }
  int st = ctx->stage_upload(Pinned::kCalibStdBatchUpload, d_base, up.data(), up.size(), ctx->stream);
  static const char *const kKernel[3] = {"msv_wave_batch_kernel", "vit_wave_batch_kernel", "fwd_wave_batch_kernel"};
  for (int s = 0; s < 3 && st == BATH_OK; s++)
    for (int j0 = 0; j0 < n_models && st == BATH_OK;) {
      const int k0 = by_tiling[(size_t)j0], Cv = tiling(k0);
      const bool gt = fwd_wave_global_tables(B.om[(size_t)k0]);
      int j1 = j0, Mmax = 0;
      double nodes = 0.;
      for (; j1 < n_models && tiling(by_tiling[(size_t)j1]) == Cv && (s < 2 || fwd_wave_global_tables(B.om[(size_t)by_tiling[(size_t)j1]]) == gt); j1++) {
        const int M = hmms[by_tiling[(size_t)j1]]->M; Mmax = std::max(Mmax, M); nodes += M;
      }
      const int sp = ctx->span_begin(kKernel[s], ctx->stream, nodes * L[s] * N[s], 0.);
      st = launch_std_wave_batch(ctx, ctx->stream, s, d_base + (size_t)j0 * desc, j1 - j0, Mmax, Cv, gt, S->sq[s]->view());
      ctx->span_end(sp, ctx->stream);
      j0 = j1;
    }
  if (st != BATH_OK) { (void)hipStreamSynchronize(ctx->stream); return st; }
  // ---- 5. the frameshift taus of the batch: every model on the one pair of sets, anchored with p7_Lambda's double as
  // bath_hip_calibrate hands it on (evalues.c:142-143); the standard results come back behind its launches, one synchronize
  std::vector<float> sc((size_t)nres);
  std::vector<int32_t> status((size_t)nres);
  const std::function<int()> queue_std = [&]() -> int {
    BATH_HIP_TRY(ctx, hipMemcpyAsync(sc.data(), d_sc, (size_t)nres * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(status.data(), d_st, (size_t)nres * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return BATH_OK;
  };
  std::vector<int> pair_of((size_t)n_models, 0);
  std::vector<double> lambda((size_t)n_models), tau3((size_t)n_models), tau5((size_t)n_models), x3, x5;
  for (int k = 0; k < n_models; k++) lambda[(size_t)k] = bath_hmm_lambda(hmms[k]);        // p7_Lambda
  if (fs) {
    if (xv) { x3.resize((size_t)n_models * EfN); x5.resize((size_t)n_models * EfN); }
    st = calibrate_fs_sets(ctx, "calibrate_batch", hmms, basic.data(), n_models, dna.data(), 1, pair_of.data(), lambda.data(), EfL, EfN, Eft,
                           tau3.data(), tau5.data(), xv ? x3.data() : nullptr, xv ? x5.data() : nullptr, &queue_std);
  } else {                                                 // the standard results alone: the copies, the one synchronize
    st = queue_std();
    const hipError_t sync = hipStreamSynchronize(ctx->stream);
    if (st == BATH_OK) BATH_HIP_TRY(ctx, sync);
  }
  if (st != BATH_OK) return st;
  // ---- 6. the standard fits (calibrate_std's, per model), into locals: nothing is written before the last has succeeded
  static const char *const kWhat[3] = {"msv mu", "vit mu", "fwd tau"};
  std::vector<double> mu((size_t)n_models * 3), x((size_t)nres);
  for (int k = 0; k < n_models; k++) {
    const bath_hip_oprofile *om = B.om[(size_t)k];
    const std::string who = "calibrate_batch: model at position " + std::to_string(k) + " of the batch: ";
    const float maxsc[2] = {(float)((255 - om->base_b) / om->scale_b),            // evalues.c:305
                            (float)((32767.0 - om->base_w) / om->scale_w)};        // evalues.c:374
    int64_t at = (int64_t)k * per_model;
    for (int s = 0; s < 3; at += N[s], s++) {
      const float nullsc = om->lt.h_nullsc[(size_t)L[s]];                          // p7_bg_SetLength(bg, L) + p7_bg_NullOne
      double *xs = &x[(size_t)at];
      for (int i = 0; i < N[s]; i++) {
        float v = sc[(size_t)(at + i)];
        const int32_t code = status[(size_t)(at + i)];
        if (code == BATH_ERANGE && s < 2) v = maxsc[s];
        else if (code != BATH_OK) { ctx->set_error(who + "failed to determine " + kWhat[s] + ": a sampled sequence's filter returned status " + std::to_string(code)); return code == BATH_ERANGE ? BATH_ERANGE : BATH_EFAIL; }
        xs[i] = (v - nullsc) / 0.69314718055994529;                                 // float difference, double quotient
      }
      st = s < 2 ? bath_gumbel_fit_complete_loc(xs, N[s], lambda[(size_t)k], &mu[(size_t)k * 3 + s]) : bath_calib_tau(xs, N[s], lambda[(size_t)k], Eft, &mu[(size_t)k * 3 + s]);
      if (st != BATH_OK) { ctx->set_error(who + "failed to determine " + kWhat[s] + ": the fit did not converge"); return st; }
    }
  }
  // ---- 7. every fit of every model is there: the parameters, the bit scores, the state one bath_hip_calibrate call leaves
  for (int k = 0; k < n_models; k++) {
    float *ev = hmms[k]->evparam;
    ev[1] = ev[3] = ev[5] = (float)lambda[(size_t)k];                               // evalues.c:148-153
    ev[0] = (float)mu[(size_t)k * 3]; ev[2] = (float)mu[(size_t)k * 3 + 1]; ev[4] = (float)mu[(size_t)k * 3 + 2];
    ev[6] = fs ? (float)tau3[(size_t)k] : kEvparamUnset; ev[7] = fs ? (float)tau5[(size_t)k] : kEvparamUnset;
    if (xv) {
      double *out = xv + (size_t)k * (size_t)(per_model + (fs ? 2 * (int64_t)EfN : 0));
      std::copy(&x[(size_t)k * per_model], &x[(size_t)(k + 1) * per_model], out);
      if (!fs) continue;
      std::copy(&x3[(size_t)k * EfN], &x3[(size_t)(k + 1) * EfN], out + per_model);
      std::copy(&x5[(size_t)k * EfN], &x5[(size_t)(k + 1) * EfN], out + per_model + EfN);
    }
  }
  *rng_state = state;
  return BATH_OK;
}

extern "C" int bath_hip_calibrate_batch(bath_hip_ctx *ctx, bath_hmm *const *hmms, int n_models, int ncbi_table, uint32_t *rng_state,
                                        bath_hip_calib_samples *samples, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv) {
  return calibrate_models(ctx, hmms, n_models, ncbi_table, rng_state, samples, EmL, EmN, EvL, EvN, EfL, EfN, Eft, xv, true);
}

extern "C" int bath_hip_calibrate_std_batch(bath_hip_ctx *ctx, bath_hmm *const *hmms, int n_models, uint32_t *rng_state,
                                            bath_hip_calib_samples *samples, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv) {
  return calibrate_models(ctx, hmms, n_models, 0, rng_state, samples, EmL, EmN, EvL, EvN, EfL, EfN, Eft, xv, false);
}
