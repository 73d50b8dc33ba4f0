// bath_fs5_odds.hip -- the 5-codon frameshift Forward and Backward in odds-ratio (probability) space: what the reference's
// bathsearch --fs runs for envelopes and multi-domain regions (p7_Forward_Frameshift impl_sse/fwdback_fs.c:2054-2610,
// p7_Backward_Frameshift :2634-2970; the stochastic-traceback Forward of p7_domaindef.c:411-414), not the log-space generic
// recursion (generic_fwdback_frameshift.c:64, :1035) the other modes restate.  Switched on by bath_hip_set_fs5_odds.
//
//   fs5_fwd_odds_kernel<C, MULTIHIT, STORE>
//       IVX(i,k)  = B(i-1) tBM(k-1) + M(i-1,k-1) tMM(k-1) + I(i-1,k-1) tIM(k-1) + D(i-1,k-1) tDM(k-1)   (rows 1, 2: B only)
//       M_c(i,k)  = IVX(i-c+1,k) e_c(k), c = 1..5 (c5_compat = 0, fwdback_fs.c:1464);  M(i,k) = sum_c M_c(i,k)
//       I(i,k)    = M(i-3,k) tMI(k) + I(i-3,k) tII(k);  D(i,k) = M(i,k-1) tMD(k-1) + D(i,k-1) tDD(k-1)
//       E(i)      = sum_k M(i,k) + D(i,k);  N, J, C from row i-3, B(i) = N(i) tNM + J(i) tJM; rows 1, 2: N = 1, B = tNM
//       MULTIHIT = false: the envelopes' unihit configuration (p7_fs_ReconfigUnihit: E->J impossible, E->C = 1);
//       MULTIHIT = true:  the regions' configuration of a fixed amino length (E->C = E->J = 1/2)
//       STORE = false:    the score alone (calibration's parser, bath_hip_fs5_forward_parser_odds): every store of a cell, of a
//                         special-state row and of <done> is compiled out with the logarithms that only fed them; the matrix and
//                         offset pointers are never read; the recurrence, the rescale and sc[job] are the same source
//   fs5_bwd_odds_kernel<C>  unihit, the mirror image, rows L down to 0: with the rows beyond L held at zero one formula covers
//       every row case of the generic code (:1054-1392; row L, the tail rows L-1 / L-2, the main recursion)
//
// Shape as bath_fs_odds.hip's: one wave per envelope or region (the longest-first job list), lane l owns the C consecutive nodes
// l*C+1 .. l*C+C; the D row is an affine recurrence (a per-lane composition and a 6-step DPP scan), E(i) and B(i) are DPP sums, no
// log-sum table and no LDS.  The state is the rings of M, I (3 rows), D (1) and IVX (4) in registers -- about 11 C floats -- plus
// the five emission rows.
//
// Rescaling as the reference's (fwdback_fs.c:2220, 2366, 2548): when E(i) (Backward: B(i), as fs3_bwd_odds_kernel) passes 1e4,
// every value a later row reads is multiplied by 1/E(i) and log E(i) joins the running scale.  Backward keeps scales of its own, so
// the envelope stage's Forward and Backward still run side by side.  Every matrix leaves the kernel in LOG space, log(value) + the
// running scale, in the layouts of the other modes -- Forward (L+1) x (M+1) x {D, I, M_C0, M_C1..M_C5}, Backward (L+1) x (M+1) x
// {D, I, M}, special states (L+1) x {E,N,J,B,C} -- so decoding, optimal accuracy, null2, the traces and the host ensembles read them
// unchanged.  A row's cells are stored as log(value before the row's rescale) + the scale before it: the same number as
// log(value after) + the scale after.  A lane's C nodes are contiguous (Forward: 8 C floats, two 16-byte stores per node), so a
// wave's stores are whole lines.
#include <cmath>
#include <cstring>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

#include "bath_fs_device.hpp"

namespace bath {

constexpr int kDegen5 = 1367;            // p7P_MAXCODONS5: marks a degenerate nucleotide (rows 1364..1366 are the degenerate codons)

// (wave-uniform: the emission rows' addresses stay in scalar registers)
__device__ __forceinline__ int nuc5(uint8_t c) { return __builtin_amdgcn_readfirstlane(c < 4 ? (int)c : kDegen5); }

// natural log of an odds ratio plus the scale, for the matrices (8 C values per lane and row): v_log_f32 (log2) times ln 2;
// 0 -> -inf.  Within ~1e-7 relative of logf, far inside the mode's bars.
__device__ __forceinline__ float ln_odds(float v, float s) { return __builtin_amdgcn_logf(v) * 0.6931471805599453f + s; }

// emissions fetched one row ahead, off the row's dependency chain, while the registers allow it
template <int C> constexpr bool odds5_ahead() { return C <= 6; }

template <int C>
__device__ __forceinline__ void load_row(float (&e)[C], const float *q) {
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      const float4 v = *reinterpret_cast<const float4 *>(q + c);
      e[c] = v.x; e[c + 1] = v.y; e[c + 2] = v.z; e[c + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; c++) e[c] = q[c];
  }
}

__device__ __forceinline__ void mark_done(int *done, int64_t job, int lane) {
  if (!done) return;
  __threadfence_system();                                    // every lane's stores first (system scope), then the flag
  if (lane == 0) __hip_atomic_store(done + job, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------
// Forward.  fwd[(i*(M+1)+k)*8 + {D,I,C0..C5}], xmx[i*5 + {E,N,J,B,C}].  Index 0 of a ring = the most recent row.
// tf[node] = {tMM(k-1), tIM(k-1), tDM(k-1), tBM(k-1), tMD(k), tDD(k), tMI(k), tII(k)}
// ---------------------------------------------------------------------------------------------
template <int C, bool MULTIHIT, bool STORE = true>
__global__ __launch_bounds__(kOddsBlock) void fs5_fwd_odds_kernel(SeqView dna, FsOddsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                                    float *__restrict__ sc, float *__restrict__ fwd, const int64_t *__restrict__ fwd_off,
                                                                    float *__restrict__ xmx, const int64_t *__restrict__ xmx_off,
                                                                    int cfg_len /* >= 0: the amino length the model is configured for, instead of L/3 */, FsJobs jobs,
                                                                    int *__restrict__ done /* host-visible: done[job] = 1 once the job's matrix and score have landed */) {
  const int lane = threadIdx.x & 63;
  const int M = p.M;
  const float tEL = MULTIHIT ? 0.5f : 0.f, tEM = MULTIHIT ? 0.5f : 1.f;
  // C = 20: the IVX ring in LDS (4 rows x 20 floats per thread, 80 KB per block, each thread its own column, no barrier) -- in
  // registers it is the 80 values that pushed the kernel past 512 registers into scratch
  constexpr bool IVL = C >= 20;
  __shared__ float s_iv[IVL ? 4 * C * kOddsBlock : 1];
  auto ivs = [&](int row, int c) -> float & { return s_iv[(((row & 3) * C) + c) * kOddsBlock + threadIdx.x]; };
  for (int64_t job = fs_next_job(jobs, dna.n, lane); job >= 0; job = fs_next_job(jobs, dna.n, lane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *fo = nullptr, *xo = nullptr;
    if constexpr (STORE) {
      fo = static_cast<float *>(__builtin_assume_aligned(fwd + fwd_off[job], 32));            // rows of (M+1) x 8 floats: every cell is 32-byte aligned
      xo = xmx + xmx_off[job];
    }
    if (L < 5) { if (lane == 0) sc[job] = -INFINITY; if constexpr (STORE) mark_done(done, job, lane); continue; }
    const int Lc = cfg_len >= 0 ? cfg_len : L / 3;
    const float tNL = expf(loop_tab[Lc]), tNM = expf(move_tab[Lc]), tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    // row 0, and node 0 of every row
    if constexpr (STORE) {
      const float4 ninf4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      for (int k = lane; k <= M; k += 64) { float4 *c4 = reinterpret_cast<float4 *>(fo + (size_t)k * 8); c4[0] = ninf4; c4[1] = ninf4; }
      for (int i = 1 + lane; i <= L; i += 64) { float4 *c4 = reinterpret_cast<float4 *>(fo + (size_t)i * (M + 1) * 8); c4[0] = ninf4; c4[1] = ninf4; }
      if (lane == 0) put_row(xo, 0, 0.f, 1.f, 0.f, tNM, 0.f, 0.0);
    }
    float Mr[3][C], Ir[3][C], Dr[C], iv[IVL ? 1 : 4][C];     // M, I of rows i-1..i-3; D of row i-1; IVX(i-1..i-4)
#pragma unroll
    for (int c = 0; c < C; c++) {
      Mr[0][c] = Mr[1][c] = Mr[2][c] = Ir[0][c] = Ir[1][c] = Ir[2][c] = Dr[c] = 0.f;
      if constexpr (IVL) { for (int r = 0; r < 4; r++) ivs(r, c) = 0.f; }
      else { iv[0][c] = iv[1][c] = iv[2][c] = iv[3][c] = 0.f; }
    }
    auto ivr = [&](int r, int c, int i) -> float { if constexpr (IVL) return ivs(i - 1 - r, c); else return iv[r][c]; };   // IVX(i-1-r)
    // specials of rows i-1, i-2, i-3 (row 0: N = 1, B = tNM); <unit> is 1 in the running scale, for the constants of rows 1, 2
    float xN[3] = {1.f, 1.f, 1.f}, xJ[3] = {0.f, 0.f, 0.f}, xC[3] = {0.f, 0.f, 0.f}, xB = tNM, unit = 1.f;
    double totscale = 0.0;
    // emissions of row i: codons ending at x_i (x, w, v, u, t = x_i .. x_{i-4}; before the start: the degenerate code)
    float e1n[C], e2n[C], e3n[C], e4n[C], e5n[C];
    auto fetch = [&](int xx, int ww, int vv, int uu, int tt) {
      const float *q = p.rsc + lane * C;
      load_row<C>(e1n, q + imin(xx * 341, 1366) * p.pitch);
      load_row<C>(e2n, q + imin(xx * 341 + ww * 85 + 1, 1365) * p.pitch);
      load_row<C>(e3n, q + imin(xx * 341 + ww * 85 + vv * 21 + 2, 1364) * p.pitch);
      load_row<C>(e4n, q + imin(xx * 341 + ww * 85 + vv * 21 + uu * 5 + 3, 1365) * p.pitch);
      load_row<C>(e5n, q + imin(xx * 341 + ww * 85 + vv * 21 + uu * 5 + tt + 4, 1366) * p.pitch);
    };
    int t = kDegen5, u = kDegen5, v = kDegen5, w = kDegen5, x = nuc5(d[0]);
    if (odds5_ahead<C>()) fetch(x, w, v, u, t);
    for (int i = 1; i <= L; i++) {
      if (!odds5_ahead<C>()) fetch(x, w, v, u, t);
      float e1[C], e2[C], e3[C], e4[C], e5[C];
#pragma unroll
      for (int c = 0; c < C; c++) { e1[c] = e1n[c]; e2[c] = e2n[c]; e3[c] = e3n[c]; e4[c] = e4n[c]; e5[c] = e5n[c]; }
      if (i < L) { t = u; u = v; v = w; w = x; x = nuc5(d[i]); if (odds5_ahead<C>()) fetch(x, w, v, u, t); }
      [[maybe_unused]] const float s = (float)totscale;
      [[maybe_unused]] float *row = STORE ? fo + (size_t)i * (M + 1) * 8 : nullptr;
      // row i-1 at node k-1 for the lane's first node; rows 1, 2 take B(i-1) only (generic :109, :150)
      const float g = (i <= 2) ? 0.f : 1.f;
      const float mIn = wave_shr1(Mr[0][C - 1], 0.f), iIn = wave_shr1(Ir[0][C - 1], 0.f), dIn = wave_shr1(Dr[C - 1], 0.f);
      const float *tf = per_row(p.tf);
      float Mc[C], Ic[C], ivc[C];
      [[maybe_unused]] float c1[STORE ? C : 1];
      float mloc = 1.f, aloc = 0.f;                          // the lane's D map: D(first node of the next lane) = mloc D(first node) + aloc
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int nd = lane * C + c + 1;                     // nodes beyond M: zero transitions and emissions, so everything comes out 0
        const float4 ta = *reinterpret_cast<const float4 *>(tf + nd * 8);
        const float4 tb = *reinterpret_cast<const float4 *>(tf + nd * 8 + 4);
        const float m1 = (c == 0) ? mIn : Mr[0][c - 1], i1 = (c == 0) ? iIn : Ir[0][c - 1], d1 = (c == 0) ? dIn : Dr[c - 1];
        const float ivn = xB * ta.w + g * (m1 * ta.x + i1 * ta.y + d1 * ta.z);
        ivc[c] = ivn;
        const float k1 = ivn * e1[c], k2 = ivr(0, c, i) * e2[c], k3 = ivr(1, c, i) * e3[c], k4 = ivr(2, c, i) * e4[c], k5 = ivr(3, c, i) * e5[c];
        const float mv = (k1 + (k2 + k3)) + (k4 + k5);
        Mc[c] = mv;
        if constexpr (STORE) c1[c] = k1;
        Ic[c] = Mr[2][c] * tb.z + Ir[2][c] * tb.w;           // node M: tMI(M) = tII(M) = 0
        aloc = aloc * tb.y + mv * tb.x;
        mloc = mloc * tb.y;
        if constexpr (STORE) if (nd <= M) reinterpret_cast<float4 *>(row + (size_t)nd * 8)[1] = make_float4(ln_odds(k2, s), ln_odds(k3, s), ln_odds(k4, s), ln_odds(k5, s));
      }
      float dcur = affine_scan_excl(mloc, aloc);
      float esum = 0.f, Dc[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int nd = lane * C + c + 1;
        const float2 tb = *reinterpret_cast<const float2 *>(tf + nd * 8 + 4);      // tMD(k), tDD(k)
        Dc[c] = dcur;
        esum += Mc[c] + dcur;
        if constexpr (STORE) if (nd <= M) reinterpret_cast<float4 *>(row + (size_t)nd * 8)[0] = make_float4(ln_odds(dcur, s), ln_odds(Ic[c], s), ln_odds(Mc[c], s), ln_odds(c1[c], s));
        dcur = dcur * tb.y + Mc[c] * tb.x;
      }
      float xE = wave_sum(esum);
      float nN, nJ, nC, nB;
      if (i <= 2) { nN = unit; nB = tNM * unit; }            // rows 1, 2 (:126-132, :166-167)
      else nN = xN[2] * tNL;
      nJ = MULTIHIT ? xJ[2] * tJL + xE * tEL : 0.f;          // unihit: J unreachable
      nC = xC[2] * tCL + xE * tEM;
      if (i > 2) nB = nN * tNM + nJ * tJM;
      if (xE > kOddsRescale) {                               // wave-uniform
        const float f = 1.0f / xE;
#pragma unroll
        for (int c = 0; c < C; c++) {
          Mc[c] *= f; Ic[c] *= f; Dc[c] *= f; ivc[c] *= f;
          Mr[0][c] *= f; Mr[1][c] *= f; Ir[0][c] *= f; Ir[1][c] *= f;
          if constexpr (IVL) { ivs(i - 1, c) *= f; ivs(i - 2, c) *= f; ivs(i - 3, c) *= f; }
          else { iv[0][c] *= f; iv[1][c] *= f; iv[2][c] *= f; }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) { xN[r] *= f; xJ[r] *= f; xC[r] *= f; }
        nN *= f; nJ *= f; nC *= f; nB *= f; unit *= f;
        totscale += (double)logf(xE);
        xE = 1.0f;
      }
      if constexpr (STORE) if (lane == 0) put_row(xo, i, xE, nN, nJ, nB, nC, totscale);
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
      xB = nB;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
        Dr[c] = Dc[c];
        if constexpr (IVL) ivs(i, c) = ivc[c];               // (over IVX(i-4), read above)
        else { iv[3][c] = iv[2][c]; iv[2][c] = iv[1][c]; iv[1][c] = iv[0][c]; iv[0][c] = ivc[c]; }
      }
    }
    if (lane == 0) {
      const float tot = xC[0] + xC[1] * tCL + xC[2] * tCL;    // C(L) + C(L-1) tCL + C(L-2) tCL
      sc[job] = (tot > 0.f && tot < INFINITY) ? (float)(totscale + (double)(logf(tot) + logf(tCM))) : -INFINITY;   // eslERANGE -> -inf, never NaN
    }
    if constexpr (STORE) mark_done(done, job, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// Backward (unihit: E(i) = C(i)).  bck[(i*(M+1)+k)*3 + {D,I,M}], xmx[i*5 + {E,N,J,B,C}].  Lanes own their nodes in DESCENDING order
// (logical lane = 63 - physical lane), as fs3_bwd_odds_kernel's: the descending D chain is then the same upward scan as Forward's.
// Rows of M (i+1 .. i+5) and I (i+1 .. i+3) in registers, index 0 = row i+1; rows beyond L are zero.
// tb[node] = {tMD(k), tMI(k), tMM(k), tDD(k), tDM(k), tII(k), tIM(k), tBM(k-1)}
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kOddsBlock) void fs5_bwd_odds_kernel(SeqView dna, FsOddsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                                    float *__restrict__ sc, float *__restrict__ bck, const int64_t *__restrict__ bck_off,
                                                                    float *__restrict__ xmx, const int64_t *__restrict__ xmx_off, FsJobs jobs) {
  const int M = p.M;
  const int plane = threadIdx.x & 63;
  const int lane = 63 - plane;
  for (int64_t job = fs_next_job(jobs, dna.n, plane); job >= 0; job = fs_next_job(jobs, dna.n, plane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *bo = bck + bck_off[job];
    float *xo = xmx + xmx_off[job];
    if (L < 5) { if (plane == 0) sc[job] = -INFINITY; continue; }
    const float tNL = expf(loop_tab[L / 3]), tNM = expf(move_tab[L / 3]), tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    // row 0 holds no cells (:1376-1380), and node 0 of every row
    for (int k = plane; k <= M; k += 64) { bo[(size_t)k * 3] = -INFINITY; bo[(size_t)k * 3 + 1] = -INFINITY; bo[(size_t)k * 3 + 2] = -INFINITY; }
    for (int i = 1 + plane; i <= L; i += 64) { float *c0 = bo + (size_t)i * (M + 1) * 3; c0[0] = -INFINITY; c0[1] = -INFINITY; c0[2] = -INFINITY; }
    float Mr[5][C], Ir[3][C];
#pragma unroll
    for (int c = 0; c < C; c++) {
      Mr[0][c] = Mr[1][c] = Mr[2][c] = Mr[3][c] = Mr[4][c] = Ir[0][c] = Ir[1][c] = Ir[2][c] = 0.f;
    }
    float xN[3] = {0.f, 0.f, 0.f}, xJ[3] = {0.f, 0.f, 0.f}, xC[3] = {0.f, 0.f, 0.f};     // rows i+1, i+2, i+3
    float n1 = 0.f, n2 = 0.f, unit = 1.f;
    double totscale = 0.0;
    // x, w, v, u, t = x_{i+1} .. x_{i+5}: the codons that START at nucleotide i+1, the codon's last base the most significant digit
    // (:1260-1270).  Beyond L: the degenerate code, whose (finite) scores multiply the zero rows beyond L.
    float e1n[C], e2n[C], e3n[C], e4n[C], e5n[C];
    auto fetch = [&](int xx, int ww, int vv, int uu, int tt) {
      const float *q = p.rsc + lane * C;
      load_row<C>(e1n, q + imin(xx * 341, 1366) * p.pitch);
      load_row<C>(e2n, q + imin(ww * 341 + xx * 85 + 1, 1365) * p.pitch);
      load_row<C>(e3n, q + imin(vv * 341 + ww * 85 + xx * 21 + 2, 1364) * p.pitch);
      load_row<C>(e4n, q + imin(uu * 341 + vv * 85 + ww * 21 + xx * 5 + 3, 1365) * p.pitch);
      load_row<C>(e5n, q + imin(tt * 341 + uu * 85 + vv * 21 + ww * 5 + xx + 4, 1366) * p.pitch);
    };
    int t = kDegen5, u = kDegen5, v = kDegen5, w = kDegen5, x = kDegen5;
    if (odds5_ahead<C>()) fetch(x, w, v, u, t);                // row L: no nucleotide after it
    for (int i = L; i >= 0; i--) {
      if (!odds5_ahead<C>()) fetch(x, w, v, u, t);
      float e1[C], e2[C], e3[C], e4[C], e5[C];
#pragma unroll
      for (int c = 0; c < C; c++) { e1[c] = e1n[c]; e2[c] = e2n[c]; e3[c] = e3n[c]; e4[c] = e4n[c]; e5[c] = e5n[c]; }
      if (i > 0) { t = u; u = v; v = w; w = x; x = nuc5(d[i - 1]); if (odds5_ahead<C>()) fetch(x, w, v, u, t); }    // x_i: the first nucleotide after row i-1
      const float s = (float)totscale;
      const float *tb = per_row(p.tb);
      float ivx[C];
      float bloc = 0.f;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int nd = lane * C + c + 1;
        ivx[c] = (Mr[0][c] * e1[c] + (Mr[1][c] * e2[c] + Mr[2][c] * e3[c])) + (Mr[3][c] * e4[c] + Mr[4][c] * e5[c]);
        bloc += ivx[c] * tb[nd * 8 + 7];
      }
      float xB = wave_sum(bloc);
      float nN = xN[2] * tNL + xB * tNM;
      if (i == 0) {
        if (plane == 0) {
          put_row(xo, 0, 0.f, nN, 0.f, xB, 0.f, totscale);
          const float tot = nN + n1 + n2;                      // N(0) + N(1) + N(2)
          sc[job] = (tot > 0.f && tot < INFINITY) ? (float)(totscale + (double)logf(tot)) : -INFINITY;
        }
        break;
      }
      float nJ = xJ[2] * tJL + xB * tJM;
      float nC = (i == L) ? tCM * unit : (i >= L - 2 ? tCL * tCM * unit : xC[2] * tCL);
      float xE = nC;                                         // E(i) = J(i) tEL + C(i) tEM with tEL = 0, tEM = 1
      const float ivNext = wave_shr1(ivx[0], 0.f);            // ivx at the node after the lane's last one
      float Mc[C], Ic[C], Dc[C], bd[C];
      float mloc = 1.f, aloc = 0.f;                          // D(lane's first node) = mloc D(first node of the next lane) + aloc
#pragma unroll
      for (int c = C - 1; c >= 0; c--) {
        const int nd = lane * C + c + 1;
        const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
        const float tdd = tb[nd * 8 + 3];
        bd[c] = (nd <= M ? xE : 0.f) + ivn * tb[nd * 8 + 4];
        aloc = aloc * tdd + bd[c];
        mloc = mloc * tdd;
      }
      float dn = affine_scan_excl(mloc, aloc);               // D(i, node after the lane's last one)
#pragma unroll
      for (int c = C - 1; c >= 0; c--) {
        const int nd = lane * C + c + 1;
        const float4 t0 = *reinterpret_cast<const float4 *>(tb + nd * 8);             // tMD tMI tMM tDD
        const float4 t1 = *reinterpret_cast<const float4 *>(tb + nd * 8 + 4);         // tDM tII tIM tBM
        const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
        Mc[c] = (nd <= M ? xE : 0.f) + dn * t0.x + Ir[2][c] * t0.y + ivn * t0.z;
        Ic[c] = Ir[2][c] * t1.y + ivn * t1.z;
        dn = dn * t0.w + bd[c];
        Dc[c] = dn;
      }
      {
        float *cell = bo + ((size_t)i * (M + 1) + lane * C + 1) * 3;
#pragma unroll
        for (int c = 0; c < C; c++)
          if (lane * C + c + 1 <= M) { cell[c * 3] = ln_odds(Dc[c], s); cell[c * 3 + 1] = ln_odds(Ic[c], s); cell[c * 3 + 2] = ln_odds(Mc[c], s); }
      }
      if (xB > kOddsRescale) {                               // wave-uniform
        const float f = 1.0f / xB;
#pragma unroll
        for (int c = 0; c < C; c++) {
          Mc[c] *= f; Ic[c] *= f;
          Mr[0][c] *= f; Mr[1][c] *= f; Mr[2][c] *= f; Mr[3][c] *= f; Ir[0][c] *= f; Ir[1][c] *= f;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) { xN[r] *= f; xJ[r] *= f; xC[r] *= f; }
        n1 *= f; n2 *= f; unit *= f;
        nN *= f; nJ *= f; nC *= f; xE *= f;
        totscale += (double)logf(xB);
        xB = 1.0f;
      }
      if (plane == 0) put_row(xo, i, xE, nN, nJ, xB, nC, totscale);
      if (i == 2) n2 = nN;
      if (i == 1) n1 = nN;
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[4][c] = Mr[3][c]; Mr[3][c] = Mr[2][c]; Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
      }
    }
  }
}

int launch_fs5_odds(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, Fs5OddsKind kind,
                    float *d_sc, float *d_mx, const int64_t *d_moff, float *d_xmx, const int64_t *d_xoff, int cfg_len, FsJobs jobs, int *d_done) {
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  if (om->codon_lengths != 5) { ctx->set_error("the 5-codon odds-ratio kernels need a 5-codon profile"); return BATH_EINVAL; }
  int st = om->ensure_odds();
  if (st != BATH_OK) return st;
  const int Cv = (om->odds_pitch - 4) / 64;                  // the tiling ensure_odds padded the tables for
  const FsOddsDev p = fs_odds_dev(om);
  const int grid = fs_odds_grid(ctx, n);
  // envelopes: the unihit length model of L/3 (d_loop[1]); regions: the multihit one of <cfg_len> (d_loop[0])
  BATH_FS_SWITCH(Cv, {
    if (kind == kFs5OddsEnvFwd)
      hipLaunchKernelGGL((fs5_fwd_odds_kernel<CC, false>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[1], om->d_move[1], d_sc, d_mx, d_moff,
                         d_xmx, d_xoff, -1, jobs, (int *)nullptr);
    else if (kind == kFs5OddsRegionFwd)
      hipLaunchKernelGGL((fs5_fwd_odds_kernel<CC, true>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[0], om->d_move[0], d_sc, d_mx, d_moff,
                         d_xmx, d_xoff, cfg_len, jobs, d_done);
    else
      hipLaunchKernelGGL((fs5_bwd_odds_kernel<CC>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[1], om->d_move[1], d_sc, d_mx, d_moff,
                         d_xmx, d_xoff, jobs);
  })
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// the multihit score of launch_fs5_odds(kFs5OddsRegionFwd) alone: the same kernel instantiated without its stores
int launch_fs5_odds_parser(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, float *d_sc, int cfg_len, FsJobs jobs) {
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  if (om->codon_lengths != 5) { ctx->set_error("the 5-codon odds-ratio kernels need a 5-codon profile"); return BATH_EINVAL; }
  int st = om->ensure_odds();
  if (st != BATH_OK) return st;
  const int Cv = (om->odds_pitch - 4) / 64;                  // the tiling ensure_odds padded the tables for
  const FsOddsDev p = fs_odds_dev(om);
  const int grid = fs_odds_grid(ctx, n);
  BATH_FS_SWITCH(Cv, {
    hipLaunchKernelGGL((fs5_fwd_odds_kernel<CC, true, false>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[0], om->d_move[0], d_sc,
                       (float *)nullptr, (const int64_t *)nullptr, (float *)nullptr, (const int64_t *)nullptr, cfg_len, jobs, (int *)nullptr);
  })
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath
