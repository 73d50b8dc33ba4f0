// bath_std_ens_walk.hpp -- one stochastic traceback of the standard branch's ensemble, compiled for the host and for the device from
// this one source (the per-trace-stream modes of bath_hip_set_std_ensemble: the host twin in bath_ensemble.hip, std_ensemble_kernel in
// bath_std_ensemble.hip).  The walk is p7_StochasticTrace (impl_sse/stotrace.c:71-300) as bath_ensemble.hip's serial
// region_trace_ensemble restates it, on the region's multihit Forward matrix in scaled odds-ratio space, with these differences:
//   * every trace draws from a slice of its own of the region's generator (trace t starts t * 2^20 steps in: ens_rng_jump);
//   * the E state's running sum goes over M(i,1), D(i,1), M(i,2), D(i,2), ... in ascending node order (the serial code sums in
//     the striped order of the SSE matrix): a lane streams the row once, nothing is stored;
//   * a trace is not stored: E opens a segment, the first M after it fixes sqto / hmmto, every M moves sqfrom / hmmfrom, B closes it
//     (p7_trace_Index read right to left), so a trace's segments come out last domain first.  What p7_Null2_ByTrace needs of the path
//     -- which of M, I, D every step between a domain's last and first match state was -- is kept as one 2-bit code per step.
// The matrix holds probabilities, not logs: the walk has no transcendental at all.  Its float arithmetic is *, +, -, / and
// compares, each correctly rounded on both sides (the library is built with contraction off), and the E state's sum is IEEE double:
// a host run and a device run of one trace are the same to the last bit.
#pragma once
#include "bath_fs_ens_walk.hpp"

namespace bath {

constexpr int kStdSegInts = 5;              // a segment record: sqfrom, sqto, hmmfrom, hmmto, number of path codes
enum { kStdCodeM = 0, kStdCodeI = 1, kStdCodeD = 2 };

// Path codes a trace of at most max_seg segments can leave: a match or insert step consumes a residue (Lr in all), a domain has
// fewer than M delete steps.  Never more than the step cap.
BATH_HD inline int std_ens_code_cap(int Lr, int M, int max_seg) {
  const long long a = (long long)Lr + (long long)max_seg * M, b = ens_step_cap(Lr, M);
  return (int)(a < b ? a : b);
}
BATH_HD inline int std_ens_path_words(int Lr, int M, int max_seg) { return (std_ens_code_cap(Lr, M, max_seg) + 15) / 16; }

// esl_vec_FNorm (Kahan sum, division) and esl_rnd_FChoose on the first n (2..4) entries of p: one code path for every state's
// choice, so that lanes of a wave in different states normalise and roll together.  Returns the entry, -1 after kEnsRollTries
// rolls beyond the vector's sum (a vector with a NaN: the serial code would draw for ever), -2 when the draw budget is spent.
BATH_HD inline int std_ens_choose(uint32_t &rng, int &budget, float (&p)[4], int n) {
  float sum = 0.f, comp = 0.f;
  for (int q = 0; q < 4; q++) if (q < n) { const float y = p[q] - comp, t = sum + y; comp = (t - sum) - y; sum = t; }
  const float uniform = 1.0f / (float)n;
  for (int q = 0; q < 4; q++) p[q] = (q < n) ? ((sum != 0.0f) ? p[q] / sum : uniform) : 0.f;
  for (int tries = 0; tries < kEnsRollTries; tries++) {
    if (budget-- <= 0) return -2;
    const float r = ens_rng_next(rng);
    float acc = 0.f;
    for (int q = 0; q < 4; q++) if (q < n) { acc += p[q]; if (r < acc) return q; }
  }
  return -1;
}

// One trace.  fwd: (Lr+1) x (M+1) x {M, D, I}; fx: (Lr+1) x {E, N, J, B, C, SCALE}; tf: [M+1][8] {MM IM DM BM MD DD MI II}.
// seg: up to max_seg records of kStdSegInts ints in region coordinates, LAST domain first; *nseg: how many.  path: the 2-bit codes
// of all segments in walk order, 16 to a word, std_ens_path_words(Lr, M, max_seg) words.
BATH_HD inline int std_ens_walk(int M, const float *tf, float pmove, float tEL, float tEM, int Lr, const float *fwd, const float *fx, uint32_t rng,
                                int32_t *seg, int max_seg, int32_t *nseg, uint32_t *path) {
  enum { XE = 0, XN, XJ, XB, XC, XS };
  enum { cM = 0, cD = 1, cI = 2 };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC, sT };
  const size_t W = (size_t)(M + 1) * 3;
  const float ploop = 1.0f - pmove;
  const int step_cap = ens_step_cap(Lr, M), code_cap = std_ens_code_cap(Lr, M, max_seg);
  int budget = 4 * step_cap;                                // draws this trace may make (ens_streams_fit)
  int i = Lr, k = 0, s0 = sC, nsteps = 2, ns = 0, ncode = 0, seg_code0 = 0;
  int sqfrom = 0, sqto = 0, hmmfrom = 0, hmmto = 0;
  uint32_t word = 0;
  *nseg = 0;
  while (s0 != sS) {
    int s1 = -1, n = 0;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    switch (s0) {
    case sM: {
      if (k < 1 || i < 1) return kEnsImpossible;
      const float *tk = tf + (size_t)k * 8, *pr = fwd + (size_t)(i - 1) * W + (size_t)(k - 1) * 3;
      p[0] = fx[(size_t)(i - 1) * 6 + XB] * tk[BM]; p[1] = pr[cM] * tk[MM]; p[2] = pr[cI] * tk[IM]; p[3] = pr[cD] * tk[DM];
      n = 4; break; }
    case sD: {
      if (k < 1) return kEnsImpossible;
      if (k - 1 >= 1) {
        const float *c = fwd + (size_t)i * W + (size_t)(k - 1) * 3, *tk = tf + (size_t)(k - 1) * 8;
        p[0] = c[cM] * tk[MD]; p[1] = c[cD] * tk[DD];
      }
      n = 2; break; }
    case sI: {
      if (k < 1 || i < 1) return kEnsImpossible;
      const float *pr = fwd + (size_t)(i - 1) * W + (size_t)k * 3, *tk = tf + (size_t)k * 8;
      p[0] = pr[cM] * tk[MI]; p[1] = pr[cI] * tk[II];
      n = 2; break; }
    case sC:
    case sJ: {
      const int g = s0 == sC ? XC : XJ;
      p[0] = (i >= 1 ? fx[(size_t)(i - 1) * 6 + g] : 0.f) * ploop;            // (the serial code reads row -1 at i = 0, where C and J are 0)
      p[1] = fx[(size_t)i * 6 + XE] * (s0 == sC ? tEM : tEL) * fx[(size_t)i * 6 + XS];
      n = 2; break; }
    case sB:
      p[0] = fx[(size_t)i * 6 + XN] * pmove; p[1] = fx[(size_t)i * 6 + XJ] * pmove;
      n = 2; break;
    case sN: s1 = (i == 0) ? sS : sN; break;
    case sE: {                                              // select_e: the roll against a running sum in double
      if (budget-- <= 0) return kEnsStepCap;
      rng = rng * 69069u + 1u;
      const double roll = (double)rng / 4294967296.0;
      const float *c = fwd + (size_t)i * W;
      const float norm = (float)(1.0 / fx[(size_t)i * 6 + XE]);
      double sum = 0.0;
      for (int pass = 0; pass < 4 && s1 < 0; pass++)
        for (int kk = 1; kk <= M; kk++) {
          sum += c[(size_t)kk * 3 + cM] * norm; if (roll < sum) { k = kk; s1 = sM; break; }
          sum += c[(size_t)kk * 3 + cD] * norm; if (roll < sum) { k = kk; s1 = sD; break; }
        }
      if (s1 < 0) return kEnsImpossible;
      break; }
    default: return kEnsImpossible;
    }
    if (n) {
      const int q = std_ens_choose(rng, budget, p, n);
      if (q < 0) return q == -2 ? kEnsStepCap : kEnsImpossible;
      switch (s0) {
      case sM: s1 = q == 0 ? sB : (q == 1 ? sM : (q == 2 ? sI : sD)); k--; i--; break;
      case sD: s1 = q == 0 ? sM : sD; k--; break;
      case sI: s1 = q == 0 ? sM : sI; i--; break;
      case sB: s1 = q == 0 ? sN : sJ; break;
      default: s1 = q == 0 ? s0 : sE; break;                // C, J
      }
    }
    if (s1 < 0 || i < 0 || k < 0) return kEnsImpossible;
    if (nsteps > step_cap) return kEnsStepCap;
    nsteps++;
    if (s1 == sE) { sqfrom = sqto = hmmfrom = hmmto = 0; seg_code0 = ncode; }
    else if (s1 == sM || ((s1 == sI || s1 == sD) && sqto)) {
      if (s1 == sM) { if (!sqto) { sqto = i; hmmto = k; } sqfrom = i; hmmfrom = k; }
      if (ncode == code_cap) return kEnsStepCap;
      word |= (uint32_t)(s1 == sM ? kStdCodeM : (s1 == sI ? kStdCodeI : kStdCodeD)) << (2 * (ncode & 15));
      if ((++ncode & 15) == 0) { path[(ncode >> 4) - 1] = word; word = 0; }
    } else if (s1 == sB) {
      if (ns == max_seg) return kEnsSegOverflow;
      int32_t *g = seg + ns * kStdSegInts;
      g[0] = sqfrom; g[1] = sqto; g[2] = hmmfrom; g[3] = hmmto; g[4] = ncode - seg_code0;
      ns++;
    }
    if ((s1 == sN || s1 == sJ || s1 == sC) && s1 == s0) i--;
    if (i < 0) return kEnsImpossible;                       // (the serial code finds this a step later, after reading row -1)
    s0 = s1;
  }
  if (ncode & 15) path[ncode >> 4] = word;
  *nseg = ns;
  return kEnsOk;
}

}  // namespace bath
