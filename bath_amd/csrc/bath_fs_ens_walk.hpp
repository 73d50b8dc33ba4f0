// bath_fs_ens_walk.hpp -- one stochastic traceback of the frameshift ensemble, compiled for the host and for the device from this
// one source (the per-trace-stream modes of bath_hip_set_fs_ensemble: the host twin in bath_ensemble.hip, fs_ensemble_kernel in
// bath_fs_ensemble.hip).  The walk is generic_stotrace_frameshift.c:40-215 as bath_ensemble.hip's serial fs_region_trace_ensemble
// restates it -- the state switch, esl_vec_FLogNorm + esl_vec_FNorm, esl_rnd_FChoose, the codon-length choice, the early exits on
// -inf cells -- with two differences that make a host run and a device run of one trace the same to the last bit:
//   * every trace draws from a slice of its own of the region's generator (trace t starts t * 2^20 steps in: ens_rng_jump);
//   * expf / logf are the ones below: plain IEEE double arithmetic with explicit fma, no library call, contraction off.  glibc's
//     and ocml's expf differ in the last bit now and then, and one flipped `roll < acc` changes a trace.
// A trace is not stored: walking backwards, E opens a segment, the first M after it fixes sqto / hmmto, every M moves sqfrom /
// hmmfrom, B closes it (p7_trace_fs_Index read right to left).  A trace's segments therefore come out last domain first.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BATH_HD __host__ __device__
#else
#define BATH_HD
#endif

namespace bath {

constexpr int kEnsSamples = 200;            // traces per region (p7_domaindef.c:97)
constexpr int kEnsMaxSeg = 8;               // segments (domains) the kernel keeps per trace; one more is "segment overflow": the region goes to the host twin
constexpr int kEnsHostMaxSeg = 64;          // ... which keeps this many (beyond: the serial ensemble)
constexpr int kEnsStreamLog2 = 20;          // trace t starts t << 20 steps into the region's generator
constexpr int kEnsRollTries = 16;           // esl_rnd_FChoose draws again when roll >= the vector's sum (1 - a few ulp): never twice in practice
enum EnsStatus { kEnsOk = 0, kEnsImpossible = 1, kEnsStepCap = 2, kEnsSegOverflow = 3 };
enum { kEnsRegionOk = 0, kEnsRegionNoTraces = 1 };

// x <- 69069 x + 1 (mod 2^32), esl_randomness_CreateFast's generator (bath_ensemble.hip: FastRng)
BATH_HD inline float ens_rng_next(uint32_t &x) { x = x * 69069u + 1u; return (float)((double)x / 4294967296.0); }
BATH_HD inline int ens_step_cap(int Lr, int M) { return 4 * (Lr + M) + 64; }
// The stream rule: a trace draws at most 4 step_cap numbers -- ens_walk counts its draws and ends the trace with "step cap" when the
// budget is spent (a step needs two, the state's choice and the codon's; a retry is a once-in-10^7 event) -- so the slices of two
// traces cannot overlap while 4 step_cap < 2^20
BATH_HD inline bool ens_streams_fit(int Lr, int M) { return 4ll * ens_step_cap(Lr, M) < (1ll << kEnsStreamLog2); }

// ---- expf and logf of the stream modes.  Double arithmetic throughout (+, *, /, fma: each correctly rounded on both sides), one
// rounding to float at the end: within 0.5 ulp + 2^-30 of the true value (DESIGN.md 4.6f gives the measured figure).
BATH_HD inline double ens_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
BATH_HD inline double ens_bits_to_double(uint64_t u) { union { uint64_t u; double d; } c; c.u = u; return c.d; }
BATH_HD inline uint64_t ens_double_to_bits(double d) { union { uint64_t u; double d; } c; c.d = d; return c.u; }

BATH_HD inline float ens_expf(float xf) {
  if (!(xf == xf)) return xf;                               // NaN
  if (xf > 88.8f) return INFINITY;
  if (xf < -104.0f) return 0.0f;                            // below half the smallest fp32 subnormal (also -inf)
  const double x = (double)xf;
  const double shift = 6755399441055744.0;                  // 1.5 * 2^52: adding it rounds to the nearest integer
  const double n = (x * 1.4426950408889634 + shift) - shift;
  double r = ens_fma(-n, 0.6931471803691238, x);            // ln 2, high 32 bits: n * hi is exact
  r = ens_fma(-n, 1.9082149292705877e-10, r);               // |r| <= 0.3466
  double p = 1.0 / 39916800.0;                              // Taylor to r^11 / 11!: truncation below 2e-15
  p = ens_fma(p, r, 1.0 / 3628800.0);
  p = ens_fma(p, r, 1.0 / 362880.0);
  p = ens_fma(p, r, 1.0 / 40320.0);
  p = ens_fma(p, r, 1.0 / 5040.0);
  p = ens_fma(p, r, 1.0 / 720.0);
  p = ens_fma(p, r, 1.0 / 120.0);
  p = ens_fma(p, r, 1.0 / 24.0);
  p = ens_fma(p, r, 1.0 / 6.0);
  p = ens_fma(p, r, 0.5);
  p = ens_fma(p, r, 1.0);
  p = ens_fma(p, r, 1.0);
  const int64_t e = (int64_t)n + 1023;                      // -151 .. 129 + 1023: a normal double
  const double y = p * ens_bits_to_double((uint64_t)e << 52);
  return y > 3.4028234663852886e38 ? INFINITY : (float)y;
}

BATH_HD inline float ens_logf(float xf) {
  if (!(xf == xf) || xf < 0.0f) return NAN;
  if (xf == 0.0f) return -INFINITY;
  if (xf == INFINITY) return INFINITY;
  const uint64_t u = ens_double_to_bits((double)xf);        // every fp32, subnormals included, is a normal double
  int e = (int)(u >> 52) - 1023;
  double m = ens_bits_to_double((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);   // [1, 2)
  if (m > 1.4142135623730951) { m *= 0.5; e++; }            // [0.7071, 1.4142]
  const double f = m - 1.0, s = f / (2.0 + f), z = s * s;   // log m = 2 atanh(s), |s| <= 0.1716
  double p = 1.0 / 19.0;                                    // series to s^18 / 19: truncation below 1e-17
  p = ens_fma(p, z, 1.0 / 17.0);
  p = ens_fma(p, z, 1.0 / 15.0);
  p = ens_fma(p, z, 1.0 / 13.0);
  p = ens_fma(p, z, 1.0 / 11.0);
  p = ens_fma(p, z, 1.0 / 9.0);
  p = ens_fma(p, z, 1.0 / 7.0);
  p = ens_fma(p, z, 1.0 / 5.0);
  p = ens_fma(p, z, 1.0 / 3.0);
  p = ens_fma(p, z, 1.0);
  const double lm = 2.0 * s * p;
  const double de = (double)e;
  return (float)ens_fma(de, 0.6931471803691238, ens_fma(de, 1.9082149292705877e-10, lm));
}

// esl_vec_FLogNorm, then esl_vec_FNorm as esl_rnd_FChoose's callers do: max, cut-off sum, log, exp, Kahan sum, division
template <int N>
BATH_HD inline void ens_lognorm(float (&v)[N]) {
  float mx = v[0];
  for (int q = 1; q < N; q++) mx = v[q] > mx ? v[q] : mx;
  float denom;
  if (mx == INFINITY) denom = INFINITY;
  else if (mx == -INFINITY) denom = -INFINITY;
  else { float sum = 0.f; for (int q = 0; q < N; q++) if (v[q] > mx - 50.f) sum += ens_expf(v[q] - mx); denom = ens_logf(sum) + mx; }
  for (int q = 0; q < N; q++) v[q] = ens_expf(v[q] - denom);
  float sum = 0.f, comp = 0.f;
  for (int q = 0; q < N; q++) { const float y = v[q] - comp, t = sum + y; comp = (t - sum) - y; sum = t; }
  for (int q = 0; q < N; q++) v[q] = (sum != 0.0f) ? v[q] / sum : 1.0f / (float)N;
}

// esl_rnd_FChoose; -1 after kEnsRollTries rolls beyond the vector's sum (a vector of NaN: the serial code would draw for ever),
// -2 when the trace's draw budget is spent
template <int N>
BATH_HD inline int ens_roll(uint32_t &rng, int &budget, const float (&v)[N]) {
  for (int tries = 0; tries < kEnsRollTries; tries++) {
    if (budget-- <= 0) return -2;
    const float r = ens_rng_next(rng);
    float acc = 0.f;
    for (int q = 0; q < N; q++) { acc += v[q]; if (r < acc) return q; }
  }
  return -1;
}

// The E state: esl_vec_FLogNorm + esl_vec_FNorm + esl_rnd_FChoose over {-inf, M(i,1..M), -inf, D(i,2..M)} (2M + 1 entries), by one
// walker, nothing stored: the row is read once per sum, and every sum runs over the entries in ascending index with the floats of
// ens_lognorm / ens_roll.  Returns the entry chosen, -1 or -2 as ens_roll does.
BATH_HD inline int ens_choose_e(uint32_t &rng, int &budget, const float *row /* cells (i, 0..M), 8 floats each */, int M) {
  const int n = 2 * M + 1;
  auto at = [&](int q) -> float { return (q == 0 || q == M + 1) ? -INFINITY : (q <= M ? row[(size_t)q * 8 + 2] : row[(size_t)(q - M) * 8 + 0]); };
  float mx = at(0);
  for (int q = 1; q < n; q++) { const float x = at(q); mx = x > mx ? x : mx; }
  float denom;
  if (mx == INFINITY) denom = INFINITY;
  else if (mx == -INFINITY) denom = -INFINITY;
  else { float sum = 0.f; for (int q = 0; q < n; q++) { const float x = at(q); if (x > mx - 50.f) sum += ens_expf(x - mx); } denom = ens_logf(sum) + mx; }
  float sum = 0.f, comp = 0.f;
  for (int q = 0; q < n; q++) { const float y = ens_expf(at(q) - denom) - comp, t = sum + y; comp = (t - sum) - y; sum = t; }
  for (int tries = 0; tries < kEnsRollTries; tries++) {
    if (budget-- <= 0) return -2;
    const float r = ens_rng_next(rng);
    float acc = 0.f;
    for (int q = 0; q < n; q++) {
      const float p = ens_expf(at(q) - denom);
      acc += (sum != 0.0f) ? p / sum : 1.0f / (float)n;
      if (r < acc) return q;
    }
  }
  return -1;
}

// One trace.  fwd: (Lr+1) x (M+1) x {D, I, M_C0, M_C1..M_C5}; fx: (Lr+1) x {E,N,J,B,C}; tsc: generic [M][8] (log space).
// seg: up to max_seg x {sqfrom, sqto, hmmfrom, hmmto} in region coordinates, LAST domain first; *nseg: how many.
BATH_HD inline int ens_walk(int M, const float *tsc, float xNL, float xNM, float xE, int Lr, const float *fwd, const float *fx, uint32_t rng,
                            int32_t *seg, int max_seg, int32_t *nseg) {
  enum { gD = 0, gI = 1, gM = 2 };
  enum { gE = 0, gN, gJ, gB, gC };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC, sT };
  const size_t W = (size_t)(M + 1) * 8;
  auto DP = [&](int i, int k, int s) -> float { return fwd[(size_t)i * W + (size_t)k * 8 + s]; };
  auto X = [&](int i, int s) -> float { return fx[(size_t)i * 5 + s]; };
  auto TS = [&](int s, int k) -> float { return tsc[(size_t)k * 8 + s]; };
  const int step_cap = ens_step_cap(Lr, M);
  int budget = 4 * step_cap;                                // draws this trace may make (ens_streams_fit)
  int i = Lr, k = 0, c = 0, sprv = sC, nsteps = 2, ns = 0;
  int sqfrom = 0, sqto = 0, hmmfrom = 0, hmmto = 0;
  *nseg = 0;
  while (sprv != sS) {
    int scur = -1;
    switch (sprv) {
    case sC:
    case sJ: {
      const int g = sprv == sC ? gC : gJ;
      if (X(i, g) == -INFINITY) return kEnsImpossible;
      if (i < 4) { scur = sE; break; }
      float v[4] = {X(i - 3, g) + xNL, X(i - 2, g) + xNL, X(i - 1, g) + xNL, X(i, gE) + xE};
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      scur = q < 3 ? sprv : sE;
      break; }
    case sE: {
      if (X(i, gE) == -INFINITY) return kEnsImpossible;
      k = ens_choose_e(rng, budget, fwd + (size_t)i * W, M);
      if (k < 0) return k == -2 ? kEnsStepCap : kEnsImpossible;
      if (k <= M) scur = sM; else { k -= M; scur = sD; }
      break; }
    case sM: {
      float v[4] = {X(i, gB) + TS(BM, k - 1), DP(i, k - 1, gM) + TS(MM, k - 1), DP(i, k - 1, gI) + TS(IM, k - 1), DP(i, k - 1, gD) + TS(DM, k - 1)};
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      scur = q == 0 ? sB : (q == 1 ? sM : (q == 2 ? sI : sD));
      k--; break; }
    case sD: {
      if (k < 1 || DP(i, k, gD) == -INFINITY) return kEnsImpossible;        // (k < 1: nothing to read at node -1)
      float v[2] = {DP(i, k - 1, gM) + TS(MD, k - 1), DP(i, k - 1, gD) + TS(DD, k - 1)};
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      scur = q == 0 ? sM : sD;
      k--; break; }
    case sI: {
      if (k >= M || DP(i, k, gI) == -INFINITY || i < 3) return kEnsImpossible;   // (node M has no insert state: tsc ends at M - 1)
      float v[2] = {DP(i - 3, k, gM) + TS(MI, k), DP(i - 3, k, gI) + TS(II, k)};
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      scur = q == 0 ? sM : sI;
      i -= 3; break; }
    case sN:
      if (X(i, gN) == -INFINITY) return kEnsImpossible;
      scur = (i == 0) ? sS : sN; break;
    case sB: {
      if (X(i, gB) == -INFINITY) return kEnsImpossible;
      float v[2] = {X(i, gN) + xNM, X(i, gJ) + xNM};
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      scur = q == 0 ? sN : sJ;
      break; }
    default: return kEnsImpossible;
    }
    if (scur == sM) {                                       // codon length from the C1..C5 cells
      if (k < 1) return kEnsImpossible;                     // (the serial code reads node 0's cells here and then fails on its next step)
      float v[5];
      for (int q = 0; q < 5; q++) v[q] = DP(i, k, gM + 1 + q);
      ens_lognorm(v);
      const int q = ens_roll(rng, budget, v);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      c = q + 1;
      if (i - c < 0) scur = sB;
    } else c = 0;
    if (scur < 0 || k < 0 || i < 0) return kEnsImpossible;
    if (nsteps > step_cap) return kEnsStepCap;
    nsteps++;
    if (scur == sE) { sqfrom = sqto = hmmfrom = hmmto = 0; }
    else if (scur == sM) { if (!sqto) { sqto = i; hmmto = k; } sqfrom = i - c + 1; hmmfrom = k; }
    else if (scur == sB) {
      if (ns == max_seg) return kEnsSegOverflow;
      seg[ns * 4 + 0] = sqfrom; seg[ns * 4 + 1] = sqto; seg[ns * 4 + 2] = hmmfrom; seg[ns * 4 + 3] = hmmto;
      ns++;
    }
    if ((scur == sN || scur == sC || scur == sJ) && scur == sprv) i--;
    sprv = scur;
    i -= c;
    if (i < 0) return kEnsImpossible;
  }
  *nseg = ns;
  return kEnsOk;
}

}  // namespace bath
