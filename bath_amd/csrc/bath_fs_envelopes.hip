// bath_fs_envelopes.hip -- the frameshift branch's envelope stage for gfx950: posterior decoding, optimal accuracy, null2 and the
// optimal-accuracy trace of a batch of envelopes, and fs5_envelopes_ex, the one function that launches them.
//
//   fs5_decode_oa_kernel  <- p7_Decoding_Frameshift + p7_OptimalAccuracy_Frameshift (fill)
//                            generic_decoding_frameshift.c:36, generic_optacc_frameshift.c:53
//   fs5_trace_kernel      <- p7_OATrace_Frameshift generic_optacc_frameshift.c:373, and the null2 score of the aligned residues,
//                            rescore_isolated_domain_frameshift p7_domaindef.c:1086; a lane per envelope (BATH_HIP_FS_TRACE_LANE=1)
//   fs5_trace_wave_kernel <- the same trace, correction and columns with a wave per envelope walking
//   fs5_null2_kernel      <- p7_Null2_fs_ByExpectation generic_null2_frameshift.c:46
//
// Forward and Backward of the envelopes are the row-per-lane wavefronts of bath_fs_wavefront.hip (the odds-ratio kernels of
// bath_fs5_odds.hip under bath_hip_set_fs5_odds), and long models decode with several waves per envelope (bath_fs_decode.hip).  The
// parsers, the regions and the regions' Forward are bath_frameshift.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

#include "bath_fs_device.hpp"

namespace bath {

// ---------------------------------------------------------------------------------------------
// Posterior decoding (generic_decoding_frameshift.c:36-156, with the column sums null2 needs, generic_null2_frameshift.c:62-68)
// AND the optimal-accuracy fill (generic_optacc_frameshift.c:53-324; TSCDELTA is 1 for a possible transition, FLT_MIN for an
// impossible one) in one walk over the rows.  Both go through the rows in ascending order and the OA row needs exactly the
// posteriors decoding has just produced, so the
// posteriors are taken from registers instead of being written (32 B/cell) and read back (32 B/cell) by a second kernel: the
// pass reads Forward (32 B) and Backward (12 B) and writes the posteriors (32 B, for the traceback) and the OA cells (12 B),
// 88 B/cell instead of 120, and -- what matters more for these latency-bound kernels -- one chain of dependent rows instead of
// two.  Lanes own C contiguous nodes (the OA recursion's layout); the row's normalising sum is a wave reduction; null2's
// column sums stay in registers (C <= 4) and are written once per envelope.
// ---------------------------------------------------------------------------------------------
#ifndef BATH_FS_OA_WAVES
#define BATH_FS_OA_WAVES 2
#endif
template <int C>
__global__ __launch_bounds__(256, (C <= 3 ? BATH_FS_OA_WAVES : 1)) void fs5_decode_oa_kernel(SeqView dna, int M, const float *__restrict__ tf, const float *__restrict__ loop_tab, const float *__restrict__ bcksc,
                                                            float *__restrict__ fwd, const int64_t *__restrict__ fwd_off, float *__restrict__ fx, const int64_t *__restrict__ x_off,
                                                            const float *__restrict__ bck, const int64_t *__restrict__ bck_off, const float *__restrict__ bx,
                                                            float *__restrict__ colsum /* [n][(M+1)*8 + 8], zeroed */, float *__restrict__ oa, float *__restrict__ oasc,
                                                            float ej, float ec, float *__restrict__ ox, FsJobs jobs,
                                                            int store_pp /* 0: the posterior matrix is NOT written (the pipeline reads it along the trace only: fs5_trace_kernel
                                                                            recomputes those cells from Forward, Backward and rowden) */,
                                                            float *__restrict__ rowden /* [rows]: 1 / (row sum) of every row, at x_off / 5; or null */) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_dl = reinterpret_cast<float *>(lds);                 // [(M+2)][8] TSCDELTA, same order as tf
  for (int i = threadIdx.x; i < (M + 2) * 8; i += blockDim.x) s_dl[i] = (tf[i] == -INFINITY) ? 1.17549435e-38f : 1.0f;
  __syncthreads();
  constexpr bool REGSUM = (C <= 4);
  const int lane = threadIdx.x & 63;
  for (int64_t job = fs_next_job(jobs, dna.n, lane); job >= 0; job = fs_next_job(jobs, dna.n, lane)) {
    const int L = dna.len[job];
    if (L < 5) { if (lane == 0) oasc[job] = -INFINITY; continue; }
    float *F = fwd + fwd_off[job];
    float *X = fx + x_off[job];
    const float *Bk = bck + bck_off[job];
    const float *Y = bx + x_off[job];
    float *O = oa + bck_off[job];
    float *OX = ox ? ox + x_off[job] : nullptr;
    float *cs = colsum + (size_t)job * ((size_t)(M + 1) * 8 + 8);
    const float overall = bcksc[job];
    const float tL = loop_tab[L / 3];
    // Forward special states of rows i, i-1, i-2, i-3 (read before their rows are overwritten with posteriors)
    float N0 = X[1], J0 = X[2], C0 = X[4], N1 = 0, N2 = 0, N3 = 0, J1 = 0, J2 = 0, J3 = 0, C1 = 0, C2 = 0, C3 = 0;
    // row 0: posteriors 0, OA cells -inf
    float *RD = rowden ? rowden + x_off[job] / 5 : nullptr;
    if (store_pp) for (int k = lane; k < (M + 1) * 8; k += 64) F[k] = 0.f;
    for (int k = lane; k <= M; k += 64) { O[(size_t)k * 3] = O[(size_t)k * 3 + 1] = O[(size_t)k * 3 + 2] = -INFINITY; }
    if (lane < 5) X[lane] = 0.f;
    if (OX && lane == 0) { OX[0] = -INFINITY; OX[1] = 0.f; OX[2] = -INFINITY; OX[3] = 0.f; OX[4] = -INFINITY; }
    float Mr[5][C], Ir[5][C], Dr[5][C];
#pragma unroll
    for (int r = 0; r < 5; r++)
#pragma unroll
      for (int c = 0; c < C; c++) Mr[r][c] = Ir[r][c] = Dr[r][c] = -INFINITY;
    float Bh[5] = {0.f, -INFINITY, -INFINITY, -INFINITY, -INFINITY};
    float Nh[3] = {0.f, 0.f, 0.f}, Jh[3] = {-INFINITY, -INFINITY, -INFINITY}, Ch[3] = {-INFINITY, -INFINITY, -INFINITY};
    float cL = -INFINITY, cL1 = -INFINITY, cL2 = -INFINITY;
    float csum[REGSUM ? C : 1][7];
    float sN = 0.f, sJ = 0.f, sC = 0.f;
    if (REGSUM) {
#pragma unroll
      for (int c = 0; c < C; c++)
#pragma unroll
        for (int q = 0; q < 7; q++) csum[c][q] = 0.f;
    }
    // Row i+1's Forward and Backward cells and special states are fetched while row i is worked on: a row's trip to HBM then
    // overlaps the previous row's chain (exp, the row sum, the optimal-accuracy scan) instead of heading this one's
    float4 fa_n[C], fb_n[C]; float bm_n[C], bi_n[C];
    float xn1 = 0.f, xn2 = 0.f, xn4 = 0.f, yn1 = 0.f, yn2 = 0.f, yn4 = 0.f;
    auto fetch_row = [&](int r) {
      const float *fq = F + (size_t)r * (M + 1) * 8;
      const float *bq = Bk + (size_t)r * (M + 1) * 3;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = imin(lane * C + c + 1, M);
        fa_n[c] = *reinterpret_cast<const float4 *>(fq + (size_t)node * 8);
        fb_n[c] = *reinterpret_cast<const float4 *>(fq + (size_t)node * 8 + 4);
        bm_n[c] = bq[(size_t)node * 3 + 2]; bi_n[c] = bq[(size_t)node * 3 + 1];
      }
      xn1 = X[r * 5 + 1]; xn2 = X[r * 5 + 2]; xn4 = X[r * 5 + 4]; yn1 = Y[r * 5 + 1]; yn2 = Y[r * 5 + 2]; yn4 = Y[r * 5 + 4];
    };
    fetch_row(1);
    for (int i = 1; i <= L; i++) {
      N3 = N2; N2 = N1; N1 = N0; J3 = J2; J2 = J1; J1 = J0; C3 = C2; C2 = C1; C1 = C0;
      float *fr = F + (size_t)i * (M + 1) * 8;
      float *orow = O + (size_t)i * (M + 1) * 3;
      float4 fa[C], fb[C]; float bmv[C], biv[C];
#pragma unroll
      for (int c = 0; c < C; c++) { fa[c] = fa_n[c]; fb[c] = fb_n[c]; bmv[c] = bm_n[c]; biv[c] = bi_n[c]; }
      const float x1 = xn1, x2 = xn2, x4 = xn4, y1 = yn1, y2 = yn2, y4 = yn4;
      if (i < L) fetch_row(i + 1);
      // ---- decoding of row i (generic_decoding_frameshift.c:62-150): exp(F + B - overall), then the row normalised to sum 1
      float pI[C], pC[C][6];
      float dloc = 0.f;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node <= M) {
          const float4 a = fa[c];
          const float4 b = fb[c];
          const float bm = bmv[c], bi = biv[c];
          pC[c][0] = expf(a.z + bm - overall); pC[c][1] = expf(a.w + bm - overall);
          pC[c][2] = expf(b.x + bm - overall); pC[c][3] = expf(b.y + bm - overall); pC[c][4] = expf(b.z + bm - overall); pC[c][5] = expf(b.w + bm - overall);
          dloc += pC[c][0];
          if (node < M) { pI[c] = expf(a.y + bi - overall); dloc += pI[c]; } else pI[c] = 0.f;
        } else {
          pI[c] = 0.f;
#pragma unroll
          for (int q = 0; q < 6; q++) pC[c][q] = 0.f;
        }
      }
      N0 = x1; J0 = x2; C0 = x4;
      float pn, pc, pj;
      if (i > 2) {
        pn = expf(N3 + y1 + tL - overall);
        pc = expf(C3 + y4 + tL - overall);
        pj = expf(J3 + y2 + tL - overall);
      } else { pn = expf(y1 - overall); pc = 0.f; pj = 0.f; }
      float denom = wave_sum_f32(dloc) + ((i > 2) ? (pn + pj + pc) : pn);
      denom = (float)(1.0 / (double)denom);
      pn *= denom; pc *= denom; pj *= denom;
      if (lane == 0) {
        if (store_pp) {
#pragma unroll
          for (int q = 0; q < 8; q++) fr[q] = 0.f;
        }
        if (RD) RD[i] = denom;
        X[i * 5 + 0] = 0.f; X[i * 5 + 3] = 0.f; X[i * 5 + 1] = pn; X[i * 5 + 4] = pc; X[i * 5 + 2] = pj;
        orow[0] = orow[1] = orow[2] = -INFINITY;
      }
      sN += pn; sJ += pj; sC += pc;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node > M) continue;
        pI[c] *= denom;
#pragma unroll
        for (int q = 0; q < 6; q++) pC[c][q] *= denom;
        if (store_pp) {
          *reinterpret_cast<float4 *>(fr + (size_t)node * 8) = make_float4(0.f, pI[c], pC[c][0], pC[c][1]);
          *reinterpret_cast<float4 *>(fr + (size_t)node * 8 + 4) = make_float4(pC[c][2], pC[c][3], pC[c][4], pC[c][5]);
        }
        if (REGSUM) {
          csum[c][0] += pI[c];
#pragma unroll
          for (int q = 0; q < 6; q++) csum[c][1 + q] += pC[c][q];
        } else {
          if (node < M) cs[(size_t)node * 8 + 1] += pI[c];
#pragma unroll
          for (int q = 0; q < 6; q++) cs[(size_t)node * 8 + 2 + q] += pC[c][q];
        }
      }
      // ---- optimal-accuracy row i (generic_optacc_frameshift.c:53-324) on the posteriors in registers
      float mIn[5], iIn[5], dIn[5];
#pragma unroll
      for (int r = 0; r < 5; r++) {
        mIn[r] = wave_shr1(Mr[r][C - 1], -INFINITY); iIn[r] = wave_shr1(Ir[r][C - 1], -INFINITY); dIn[r] = wave_shr1(Dr[r][C - 1], -INFINITY);
      }
      float Mc[C], Ic[C], am[C], bmul[C];
      float eloc = -INFINITY;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node > M) { Mc[c] = Ic[c] = -INFINITY; am[c] = -INFINITY; bmul[c] = 1.0f; continue; }
        const float dMM = s_dl[node * 8 + 0], dIM = s_dl[node * 8 + 1], dDM = s_dl[node * 8 + 2], dBM = s_dl[node * 8 + 3];
        const float dMD = s_dl[node * 8 + 4], dDD = s_dl[node * 8 + 5], dMI = s_dl[node * 8 + 6], dII = s_dl[node * 8 + 7];
        float best;
        if (i == 1) best = dBM * pC[c][1];
        else {
          float mx[6];
          const int cmax = (i >= 5) ? 5 : (i == 2 ? 2 : (i == 4 ? 4 : 3));
#pragma unroll
          for (int cl = 1; cl <= 5; cl++) {
            if (cl > cmax) { mx[cl] = -INFINITY; continue; }
            const float pv = pC[c][cl];
            if ((i == 2 && cl == 2) || (i == 4 && cl == 4)) mx[cl] = dBM * (0.0f + pv);
            else {
              const int r = cl - 1;
              const float m1 = (c == 0) ? mIn[r] : Mr[r][c - 1], i1 = (c == 0) ? iIn[r] : Ir[r][c - 1], d1 = (c == 0) ? dIn[r] : Dr[r][c - 1];
              mx[cl] = fmaxf(dMM * (m1 + pv), fmaxf(dIM * (i1 + pv), fmaxf(dDM * (d1 + pv), dBM * (Bh[r] + pv))));
            }
          }
          if (i == 2) best = fmaxf(mx[1], mx[2]);
          else if (i < 5) best = fmaxf(fmaxf(mx[1], mx[2]), fmaxf(mx[3], mx[4]));
          else best = fmaxf(fmaxf(mx[1], mx[2]), fmaxf(fmaxf(mx[3], mx[4]), mx[5]));
        }
        Mc[c] = best;
        Ic[c] = (i >= 3 && node < M) ? fmaxf(dMI * (Mr[2][c] + pI[c]), dII * (Ir[2][c] + pI[c])) : -INFINITY;
        am[c] = dMD * best;
        bmul[c] = dDD;
      }
      float A = -INFINITY, Bm = 1.0f;
#pragma unroll
      for (int c = 0; c < C; c++) { A = fmaxf(am[c], bmul[c] * A); Bm *= bmul[c]; }
      // lanes without a source see the identity map (A = -inf, B = 1); fmaxf ignores the NaN of 0 * -inf when B has underflowed
#define BATH_OA_STEP(CTRL, MASK) { const float Ap = dpp_f<CTRL, MASK>(A, -INFINITY), Bp = dpp_f<CTRL, MASK>(Bm, 1.0f); A = fmaxf(A, Bm * Ap); Bm *= Bp; }
      BATH_OA_STEP(0x111, 0xf) BATH_OA_STEP(0x112, 0xf) BATH_OA_STEP(0x114, 0xf) BATH_OA_STEP(0x118, 0xf) BATH_OA_STEP(0x142, 0xa) BATH_OA_STEP(0x143, 0xc)
#undef BATH_OA_STEP
      const float din = wave_shr1(A, -INFINITY);
      float Dc[C];
      Dc[0] = din;
#pragma unroll
      for (int c = 1; c < C; c++) Dc[c] = fmaxf(am[c - 1], bmul[c - 1] * Dc[c - 1]);
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node > M) { Dc[c] = -INFINITY; continue; }
        orow[(size_t)node * 3 + 0] = Dc[c]; orow[(size_t)node * 3 + 1] = Ic[c]; orow[(size_t)node * 3 + 2] = Mc[c];
        eloc = fmaxf(eloc, (node < M) ? Mc[c] : fmaxf(Mc[c], Dc[c]));
      }
      float xE = eloc;                                      // wave maximum: running maximum by DPP, last lane broadcast (max is exact in any order)
      xE = fmaxf(xE, dpp_f<0x111>(xE, -INFINITY)); xE = fmaxf(xE, dpp_f<0x112>(xE, -INFINITY)); xE = fmaxf(xE, dpp_f<0x114>(xE, -INFINITY));
      xE = fmaxf(xE, dpp_f<0x118>(xE, -INFINITY)); xE = fmaxf(xE, dpp_f<0x142, 0xa>(xE, -INFINITY)); xE = fmaxf(xE, dpp_f<0x143, 0xc>(xE, -INFINITY));
      xE = wave_bcast_last(xE);
      float nN, nJ, nC;
      if (i <= 2) { nJ = ej * xE; nC = ec * xE; nN = pn; }
      else { nJ = fmaxf(Jh[2] + pj, ej * xE); nC = fmaxf(Ch[2] + pc, ec * xE); nN = Nh[2] + pn; }
      const float nB = fmaxf(nN, nJ);
      if (OX && lane == 0) { float *r = OX + (size_t)i * 5; r[0] = xE; r[1] = nN; r[2] = nJ; r[3] = nB; r[4] = nC; }
      Nh[2] = Nh[1]; Nh[1] = Nh[0]; Nh[0] = nN;
      Jh[2] = Jh[1]; Jh[1] = Jh[0]; Jh[0] = nJ;
      Ch[2] = Ch[1]; Ch[1] = Ch[0]; Ch[0] = nC;
      Bh[4] = Bh[3]; Bh[3] = Bh[2]; Bh[2] = Bh[1]; Bh[1] = Bh[0]; Bh[0] = nB;
      cL2 = cL1; cL1 = cL; cL = nC;
#pragma unroll
      for (int c = 0; c < C; c++) {
#pragma unroll
        for (int r = 4; r > 0; r--) { Mr[r][c] = Mr[r - 1][c]; Ir[r][c] = Ir[r - 1][c]; Dr[r][c] = Dr[r - 1][c]; }
        Mr[0][c] = Mc[c]; Ir[0][c] = Ic[c]; Dr[0][c] = Dc[c];
      }
    }
    if (REGSUM) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node > M) continue;
        if (node < M) cs[(size_t)node * 8 + 1] = csum[c][0];
#pragma unroll
        for (int q = 0; q < 6; q++) cs[(size_t)node * 8 + 2 + q] = csum[c][1 + q];
      }
    }
    if (lane == 0) {
      float *xs = cs + (size_t)(M + 1) * 8;
      xs[1] = sN; xs[2] = sJ; xs[4] = sC;
      oasc[job] = cL + cL1 + cL2;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// null2 (generic_null2_frameshift.c:70-125) from the column sums: 20 lanes, each runs the reference's serial
// log-sum over the model for one residue, so the association is the reference's.
// ---------------------------------------------------------------------------------------------
// p7_OATrace_Frameshift (generic form: generic_optacc_frameshift.c:373-588) and the null2 score of the aligned residues
// (rescore_isolated_domain_frameshift, p7_domaindef.c:1086-1147), one LANE per envelope: the walk is serial (at most L+M
// steps of a few dependent loads), envelopes are independent, and doing it here means the posterior and OA matrices
// (>1 MB per envelope) never leave the device.  The trace is written backwards into <tbuf> and read forwards again.
#ifndef BATH_TRACE_SPREAD
#define BATH_TRACE_SPREAD 64
#endif
constexpr int kTraceSpread = BATH_TRACE_SPREAD;
__global__ void fs5_trace_kernel(SeqView dna, int M, int maxcodons, const float *__restrict__ tf, const uint8_t *__restrict__ codons,
                                 const float *__restrict__ pp, const int64_t *__restrict__ pp_off, const float *__restrict__ px, const int64_t *__restrict__ x_off,
                                 const float *__restrict__ oa, const int64_t *__restrict__ oa_off, const float *__restrict__ ox,
                                 const float *__restrict__ null2 /* [n][Kp] */, uint2 *__restrict__ tbuf, const int64_t *__restrict__ t_off, FsTraceOut *__restrict__ out,
                                 const uint8_t *__restrict__ indel_tab, const uint8_t *__restrict__ cons, uint16_t *__restrict__ steps,
                                 const float *__restrict__ amino /* rsc + maxcodons*pitch: the amino rows */, int pitch,
                                 float *__restrict__ step_pp /* posterior of every column's state (tr->pp), parallel to steps */, int *__restrict__ col_cursor,
                                 const float *__restrict__ bck /* null: <pp> holds the posterior matrix.  Else <pp> is the FORWARD matrix, untouched, and the
                                                                    posteriors the walk reads -- a match cell's five codon lengths, a column's state -- are formed here
                                                                    exactly as the decoding kernels form them: expf(F + B - overall) * rowden(i) */,
                                 const int64_t *__restrict__ bck_off, const float *__restrict__ bcksc, const float *__restrict__ rowden) {
  // One envelope per WAVE (kTraceSpread = 64 lanes apart): the walk is a state machine whose lanes diverge at every step (each
  // state's loads and compares run under their own exec mask, one after the other), so a wave holding 64 envelopes pays for
  // every state present among them at every step.  The chip has room for a wave per envelope: 2.77 -> 1.15 ms on the bench's
  // 4.8 k envelopes (8 per wave: 1.53, 4 per wave: 1.36).
  if (threadIdx.x % kTraceSpread) return;
  const int64_t job = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kTraceSpread;
  if (job >= dna.n) return;
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC, sT };
  enum { XE = 0, XN, XJ, XB, XC };
  const float kTiny = 1.17549435e-38f;                          // FLT_MIN: TSCDELTA of an impossible transition
  const int L = dna.len[job];
  const uint8_t *dsq = dna.data + dna.off[job] - 1;             // dsq[1..L]
  const float *P = pp + pp_off[job], *PX = px + x_off[job], *O = oa + oa_off[job], *OX = ox + x_off[job];
  const float *BK = bck ? bck + bck_off[job] : nullptr, *RD = bck ? rowden + x_off[job] / 5 : nullptr;
  const float overall = bck ? bcksc[job] : 0.f;
  // posterior of cell (i, k): q = 1: the insert state, q = 2: the match state (all codon lengths), q = 3..7: codon lengths 1..5
  auto post = [&](int i, int k, int q) -> float {
    const float f = P[((size_t)i * (M + 1) + k) * 8 + q];
    if (!BK) return f;
    if (q == 1 && k >= M) return 0.f;
    const float b = BK[((size_t)i * (M + 1) + k) * 3 + (q == 1 ? 1 : 2)];
    return expf(f + b - overall) * RD[i];
  };
  uint2 *T = tbuf + t_off[job];
  const int cap = (int)(t_off[job + 1] - t_off[job]);
  FsTraceOut r{0, 0, 0, 0, 0, 0, 0.f, 0, 0, 0, 0.f, 0};
  auto dl = [&](int node, int s) { return (node >= 1 && node <= M && tf[(size_t)node * 8 + s] != -INFINITY) ? 1.0f : kTiny; };
  auto OM = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 2]; };
  auto OI = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 1]; };
  auto OD = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 0]; };
  int n = 0;
  auto push = [&](int st, int k, int i, int c) { if (n < cap) T[n] = make_uint2((unsigned)st | ((unsigned)c << 8) | ((unsigned)k << 16), (unsigned)i); n++; };
  int i = L, k = 0, c = 0, prev = sC;
  bool bad = (L < 5);
  push(sT, k, i, c); push(sC, k, i, c);
  while (!bad && prev != sS) {
    int cur = -1;
    switch (prev) {
    case sM: {          // transitions into node k: MM, IM, DM, BM are tf[k][0..3]
      const float p0 = dl(k, 0) * OM(i, k - 1), p1 = dl(k, 1) * OI(i, k - 1), p2 = dl(k, 2) * OD(i, k - 1), p3 = dl(k, 3) * OX[(size_t)i * 5 + XB];
      cur = sM; float b = p0;
      if (p1 > b) { b = p1; cur = sI; }
      if (p2 > b) { b = p2; cur = sD; }
      if (p3 > b) { b = p3; cur = sB; }
      k--; break; }
    case sD: {          // transitions leaving node k-1: MD, DD are tf[k-1][4..5]
      const float p0 = dl(k - 1, 4) * OM(i, k - 1), p1 = dl(k - 1, 5) * OD(i, k - 1);
      cur = p0 >= p1 ? sM : sD; k--; break; }
    case sI: {          // MI, II of node k: tf[k][6..7]
      const float p0 = dl(k, 6) * OM(i - 3, k), p1 = dl(k, 7) * OI(i - 3, k);
      cur = p0 >= p1 ? sM : sI; i -= 3; break; }
    case sN: cur = (i == 0) ? sS : sN; break;
    case sC: {
      if (i < 4) { cur = sE; break; }
      const float p0 = OX[(size_t)(i - 3) * 5 + XC] + PX[(size_t)i * 5 + XC];
      const float p1 = (i < L) ? OX[(size_t)(i - 2) * 5 + XC] + PX[(size_t)(i + 1) * 5 + XC] : kTiny;
      const float p2 = (i < L - 1) ? OX[(size_t)(i - 1) * 5 + XC] + PX[(size_t)(i + 2) * 5 + XC] : kTiny;
      const float p3 = OX[(size_t)i * 5 + XE];
      cur = sC; float b = p0;
      if (p1 > b) b = p1;
      if (p2 > b) b = p2;
      if (p3 > b) { b = p3; cur = sE; }
      break; }
    case sJ: {
      if (i <= 5) { cur = sE; break; }
      const float p0 = OX[(size_t)i * 5 + XJ] + PX[(size_t)i * 5 + XJ], p1 = kTiny * OX[(size_t)i * 5 + XE];      // unihit: E->J impossible
      cur = (p1 > p0) ? sE : sJ; break; }
    case sE: {
      float mx = -INFINITY; int smax = -1, kmax = -1;
      for (int q = 1; q <= M; q++) {
        const float m = OM(i, q), d = OD(i, q);
        if (m > mx) { mx = m; smax = sM; kmax = q; }
        if (d > mx) { mx = d; smax = sD; kmax = q; }
      }
      k = kmax; cur = smax; break; }
    case sB: cur = (OX[(size_t)i * 5 + XN] > OX[(size_t)i * 5 + XJ]) ? sN : sJ; break;
    default: bad = true; break;
    }
    if (bad || cur < 0 || k < 0 || i < 0) { bad = true; break; }
    if (cur == sM) {
      c = 1; float b = post(i, k, 3);
#pragma unroll
      for (int q = 1; q < 5; q++) { const float v = post(i, k, 3 + q); if (v > b) { b = v; c = q + 1; } }
    } else c = 0;
    push(cur, k, i, c);
    if ((cur == sN || cur == sC || cur == sJ) && cur == prev) i--;
    prev = cur;
    i -= c;
    if (n > cap) bad = true;
  }
  if (!bad) {
    // forward order = T[n-1] .. T[0]
    const float *n2 = null2 + (size_t)job * kKp;
    auto st_of = [&](int z) { return (int)(T[n - 1 - z].x & 0xffu); };
    auto c_of = [&](int z) { return (int)((T[n - 1 - z].x >> 8) & 0xffu); };
    auto k_of = [&](int z) { return (int)(T[n - 1 - z].x >> 16); };
    auto i_of = [&](int z) { return (int)T[n - 1 - z].y; };
    int z1 = 0, z2 = n - 1;
    while (z1 < n && st_of(z1) != sM) z1++;
    while (z2 >= 0 && st_of(z2) != sM) z2--;
    if (z1 < n && z2 >= 0) {
      r.ok = 1;
      r.ihmm = k_of(z1); r.jhmm = k_of(z2);
      r.iali = i_of(z1) - (c_of(z1) - 1); r.jali = i_of(z2);
      float corr = 0.f;
      int t = -1, u = -1, v = -1, w = -1, x = -1, pos = 1, z = 0;
      while (pos <= L && z < n) {
        x = dsq[pos] < 4 ? (int)dsq[pos] : 1367;
        const int s = st_of(z);
        if (s == sN || s == sC || s == sJ) { if (i_of(z) == pos && pos > 2) pos++; z++; }
        else if (s == sM) {
          if (i_of(z) == pos) {
            int ci, capi;
            switch (c_of(z)) {
            case 1: ci = x * 341; capi = 1366; break;
            case 2: ci = x * 341 + w * 85 + 1; capi = 1365; break;
            case 3: ci = x * 341 + w * 85 + v * 21 + 2; capi = 1364; break;
            case 4: ci = x * 341 + w * 85 + v * 21 + u * 5 + 3; capi = 1365; break;
            default: ci = x * 341 + w * 85 + v * 21 + u * 5 + t + 4; capi = 1366; break;
            }
            if (c_of(z) != 3) r.nshift++;
            const float sc = logf(n2[codons[(size_t)k_of(z) * maxcodons + min(ci, capi)]]);
            if (sc != -INFINITY) corr += sc;
            z++;
          }
          pos++;
        } else if (s == sI) {
          if (i_of(z) == pos) {
            const float sc = logf(n2[codons[(size_t)k_of(z) * maxcodons + min(x * 341 + w * 85 + v * 21 + 2, 1364)]]);
            if (sc != -INFINITY) corr += sc;
            z++;
          }
          pos++;
        } else z++;
        t = u; u = v; v = w; w = x;
      }
      r.domcorrection = corr;
      // what the alignment display keeps of the trace (p7_alidisplay_fs_Create, p7_alidisplay.c:700-925): per column the
      // state, codon length and indel type (for --cigar), identities with the consensus, stop codons
      r.ncol = z2 - z1 + 1;
      // the columns of all envelopes lie DENSELY in <steps> / <step_pp>, each envelope's range reserved here (the host copies the
      // columns that exist -- a third of a nucleotide per column -- instead of every envelope's worst case of L + M + 16)
      r.col_off = steps ? atomicAdd(col_cursor, r.ncol) : 0;
      uint16_t *S = steps ? steps + r.col_off : nullptr;
      float *SP = (steps && step_pp) ? step_pp + r.col_off : nullptr;
      // ... and p7_pli_computeAliScores_BATH (p7_pipeline.c:781-979): per column the amino row score of the quasi-codon's best
      // amino acid plus the transition that entered the state (the last match state gets no MM: inner loops stop at z1 < z2)
      float ali = 0.f;
      int prevs = sB;
      for (int zz = z1; zz <= z2; zz++) {
        const int s = st_of(zz), cc = (s == sM) ? c_of(zz) : (s == sI ? 3 : 0), kk = k_of(zz), ii = i_of(zz);
        unsigned code = (unsigned)s;
        float colsc = 0.f;
        if (s == sI) colsc = tf[(size_t)kk * 8 + (prevs == sI ? 7 : 6)];
        else if (s == sD) colsc = tf[(size_t)(kk - 1) * 8 + (prevs == sD ? 5 : 4)];
        if (cc > 0 && ii - cc + 1 >= 1 && ii <= L) {
          int nn[5] = {0, 0, 0, 0, 0};
          bool degen = false;
          for (int q = 0; q < cc; q++) { nn[q] = dsq[ii - cc + 1 + q]; degen |= nn[q] >= 4; }
          int ci;
          switch (cc) {                                       // p7P_CODON{1..5}_FS5, hmmer.h:292-316; the last nucleotide is the most significant
          case 1: ci = degen ? 1366 : nn[0] * 341; break;
          case 2: ci = degen ? 1365 : nn[1] * 341 + nn[0] * 85 + 1; break;
          case 3: ci = degen ? 1364 : nn[2] * 341 + nn[1] * 85 + nn[0] * 21 + 2; break;
          case 4: ci = degen ? 1365 : nn[3] * 341 + nn[2] * 85 + nn[1] * 21 + nn[0] * 5 + 3; break;
          default: ci = degen ? 1366 : nn[4] * 341 + nn[3] * 85 + nn[2] * 21 + nn[1] * 5 + nn[0] + 4; break;
          }
          const int indel = indel_tab ? indel_tab[(size_t)kk * maxcodons + ci] : 5;
          const bool stop = (cc == 3) && (indel == 6 || indel == 7 || indel == 8);      // p7P_XXx, p7P_XxX, p7P_xXX
          if (stop) r.nstops++;
          if (s == sM && cons && codons[(size_t)kk * maxcodons + ci] == cons[kk]) r.exact++;
          code |= (unsigned)cc << 4 | (unsigned)indel << 8;
          if (s == sM && amino) {
            colsc = amino[(size_t)codons[(size_t)kk * maxcodons + ci] * pitch + kk];
            if (prevs == sI) colsc += tf[(size_t)kk * 8 + 1];
            else if (prevs == sD) colsc += tf[(size_t)kk * 8 + 2];
            else if (prevs == sM && zz < z2) colsc += tf[(size_t)kk * 8 + 0];
          }
        }
        ali += colsc;
        prevs = s;
        if (S) S[zz - z1] = (uint16_t)code;
        // get_postprob (generic_optacc_frameshift.c:425-440): a match state's total posterior (all codon lengths), an insert state's; 0 for D
        if (SP) SP[zz - z1] = (s == sM) ? post(ii, kk, 2) : (s == sI ? post(ii, kk, 1) : 0.0f);
      }
      r.aliscore = ali;
    }
  }
  out[job] = r;
}

// The same trace, correction and columns with the WAVE walking (round 5; fs5_trace_kernel above stays as the one-lane restatement the
// tests compare with, BATH_HIP_FS_TRACE_LANE=1).  A lane on its own pays a trip to memory for every decision -- two per match step
// (the optimal-accuracy cells, then the five codon-length posteriors of the cell it chose), one per residue of the correction loop,
// several per column: ~2 ms for the longest envelope of a pass, at the tail of the pass.  Here all 64 lanes follow the same state
// machine on uniform state and fill look-ahead buffers together:
//   * a match run of whole codons walks the slope-3 diagonal: on entering cell (i, k) lane d fetches cell (i - 3d, k - d) -- its
//     optimal-accuracy cells, B of its row, which transitions into node k - d + 1 exist, and its five codon-length posteriors
//     (formed like the decoding kernels form them when the matrix was not stored) -- and the steps take them by v_readlane until
//     a quasi-codon, an insert or a delete leaves the diagonal;
//   * the C and N flanks are decided / written 64 rows at a time; the E state's first maximum is a lane-parallel scan + a wave
//     reduction over (value, scan position);
//   * the correction loop (rescore_isolated_domain_frameshift's walk over the residues, whose nucleotide window also shifts on
//     iterations that do not advance -- kept as it is) runs serially on chunks of the trace and of the residues held a lane each,
//     its table look-ups deferred to 64 at a time, its sum in the reference's order;
//   * the columns are a lane each.
__global__ __launch_bounds__(64) void fs5_trace_wave_kernel(SeqView dna, int M, int maxcodons, const float *__restrict__ tf, const uint8_t *__restrict__ codons,
                                 const float *__restrict__ pp, const int64_t *__restrict__ pp_off, const float *__restrict__ px, const int64_t *__restrict__ x_off,
                                 const float *__restrict__ oa, const int64_t *__restrict__ oa_off, const float *__restrict__ ox,
                                 const float *__restrict__ null2 /* [n][Kp] */, uint2 *__restrict__ tbuf, const int64_t *__restrict__ t_off, FsTraceOut *__restrict__ out,
                                 const uint8_t *__restrict__ indel_tab, const uint8_t *__restrict__ cons, uint16_t *__restrict__ steps,
                                 const float *__restrict__ amino, int pitch, float *__restrict__ step_pp, int *__restrict__ col_cursor,
                                 const float *__restrict__ bck, const int64_t *__restrict__ bck_off, const float *__restrict__ bcksc, const float *__restrict__ rowden) {
  const int lane = threadIdx.x;
  const int64_t job = blockIdx.x;
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC, sT };
  enum { XE = 0, XN, XJ, XB, XC };
  const float kTiny = 1.17549435e-38f;
  const int L = dna.len[job];
  const uint8_t *dsq = dna.data + dna.off[job] - 1;             // dsq[1..L]
  const float *P = pp + pp_off[job], *PX = px + x_off[job], *O = oa + oa_off[job], *OX = ox + x_off[job];
  const float *BK = bck ? bck + bck_off[job] : nullptr, *RD = bck ? rowden + x_off[job] / 5 : nullptr;
  const float overall = bck ? bcksc[job] : 0.f;
  auto post = [&](int i, int k, int q) -> float {
    const float f = P[((size_t)i * (M + 1) + k) * 8 + q];
    if (!BK) return f;
    if (q == 1 && k >= M) return 0.f;
    const float b = BK[((size_t)i * (M + 1) + k) * 3 + (q == 1 ? 1 : 2)];
    return expf(f + b - overall) * RD[i];
  };
  auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
  auto rlf = [](float v, int d) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), d)); };
  uint2 *T = tbuf + t_off[job];
  const int cap = (int)(t_off[job + 1] - t_off[job]);
  FsTraceOut r{0, 0, 0, 0, 0, 0, 0.f, 0, 0, 0, 0.f, 0};
  auto dl = [&](int node, int s) { return (node >= 1 && node <= M && tf[(size_t)node * 8 + s] != -INFINITY) ? 1.0f : kTiny; };
  auto OM = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 2]; };
  auto OI = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 1]; };
  auto OD = [&](int i, int k) { return O[((size_t)i * (M + 1) + k) * 3 + 0]; };
  auto entry = [](int st, int k, int i, int c) { return make_uint2((unsigned)st | ((unsigned)c << 8) | ((unsigned)k << 16), (unsigned)i); };
  int n = 0;
  auto push = [&](int st, int k, int i, int c) { if (n < cap && lane == 0) T[n] = entry(st, k, i, c); n++; };
  int i = L, k = 0, c = 0, prev = sC;
  bool bad = (L < 5);
  push(sT, k, i, c); push(sC, k, i, c);
  // the diagonal look-ahead: lane d holds cell (bi0 - 3 d, bk0 - d)
  float bM = 0.f, bI = 0.f, bD = 0.f, bXB = 0.f, bd0 = 0.f, bd1 = 0.f, bd2 = 0.f, bd3 = 0.f, bp[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int bi0 = -(1 << 28), bk0 = -(1 << 28);
  while (!bad && prev != sS) {
    i = uni(i); k = uni(k); prev = uni(prev); n = uni(n);
    int cur = -1, dd = -1;
    if (prev == sC) {
      // rows i, i-1, ...: lane d decides row i - d; the rows that stay in C are written and skipped together
      const int rr = i - lane;
      bool stay = false;
      if (rr >= 4) {
        const float p0 = OX[(size_t)(rr - 3) * 5 + XC] + PX[(size_t)rr * 5 + XC];
        const float p1 = (rr < L) ? OX[(size_t)(rr - 2) * 5 + XC] + PX[(size_t)(rr + 1) * 5 + XC] : kTiny;
        const float p2 = (rr < L - 1) ? OX[(size_t)(rr - 1) * 5 + XC] + PX[(size_t)(rr + 2) * 5 + XC] : kTiny;
        const float p3 = OX[(size_t)rr * 5 + XE];
        float b = p0;
        if (p1 > b) b = p1;
        if (p2 > b) b = p2;
        stay = !(p3 > b);
      }
      const unsigned long long m = __ballot(stay);
      const int ns = (~m == 0ull) ? 64 : (__ffsll((long long)~m) - 1);
      if (ns > 0) {
        if (lane < ns && n + lane < cap) T[n + lane] = entry(sC, k, i - lane, 0);
        n += ns; i -= ns;
        if (n > cap) bad = true;
        continue;
      }
      cur = sE;
    } else if (prev == sN) {
      // N(i) <- N(i-1) ... <- N(1), then S at row 0: one entry per row, nothing to read
      for (int b0 = 0; b0 < i; b0 += 64) { const int rr = i - b0 - lane; if (rr >= 1 && n + b0 + lane < cap) T[n + b0 + lane] = entry(sN, k, rr, 0); }
      n += i; i = 0;
      push(sS, k, 0, 0);
      if (n > cap) bad = true;
      prev = sS;
      continue;
    } else if (prev == sM) {
      dd = bk0 - (k - 1);
      if (dd < 0 || dd >= 64 || bi0 - 3 * dd != i) {
        bi0 = i; bk0 = k - 1; dd = 0;
        const int ri = max(i - 3 * lane, 0), rk = max(k - 1 - lane, 0);
        bM = OM(ri, rk); bI = OI(ri, rk); bD = OD(ri, rk); bXB = OX[(size_t)ri * 5 + XB];
        bd0 = dl(rk + 1, 0); bd1 = dl(rk + 1, 1); bd2 = dl(rk + 1, 2); bd3 = dl(rk + 1, 3);
#pragma unroll
        for (int q = 0; q < 5; q++) bp[q] = post(ri, rk, 3 + q);
      }
      dd = uni(dd);
      const float p0 = rlf(bd0, dd) * rlf(bM, dd), p1 = rlf(bd1, dd) * rlf(bI, dd), p2 = rlf(bd2, dd) * rlf(bD, dd), p3 = rlf(bd3, dd) * rlf(bXB, dd);
      cur = sM; float b = p0;
      if (p1 > b) { b = p1; cur = sI; }
      if (p2 > b) { b = p2; cur = sD; }
      if (p3 > b) { b = p3; cur = sB; }
      k--;
    } else if (prev == sD) {
      const float p0 = dl(k - 1, 4) * OM(i, max(k - 1, 0)), p1 = dl(k - 1, 5) * OD(i, max(k - 1, 0));
      cur = p0 >= p1 ? sM : sD; k--;
    } else if (prev == sI) {
      const float p0 = dl(k, 6) * OM(max(i - 3, 0), k), p1 = dl(k, 7) * OI(max(i - 3, 0), k);
      cur = p0 >= p1 ? sM : sI; i -= 3;
    } else if (prev == sJ) {
      if (i <= 5) cur = sE;
      else { const float p0 = OX[(size_t)i * 5 + XJ] + PX[(size_t)i * 5 + XJ], p1 = kTiny * OX[(size_t)i * 5 + XE]; cur = (p1 > p0) ? sE : sJ; }
    } else if (prev == sE) {
      // the first maximum of M(i,1), D(i,1), M(i,2), D(i,2), ... (a later cell must be strictly larger)
      float mx = -INFINITY; int pos = 1 << 30;
      for (int q = 1 + lane; q <= M; q += 64) {
        const float m = OM(i, q), d = OD(i, q);
        if (m > mx) { mx = m; pos = 2 * q; }
        if (d > mx) { mx = d; pos = 2 * q + 1; }
      }
      const float best = wave_max_f32(mx);
      const int bpos = wave_min_i32((mx == best && best > -INFINITY) ? pos : (1 << 30));
      if (bpos >= (1 << 30)) bad = true;
      else { k = bpos >> 1; cur = (bpos & 1) ? sD : sM; }
    } else if (prev == sB) {
      cur = (OX[(size_t)i * 5 + XN] > OX[(size_t)i * 5 + XJ]) ? sN : sJ;
    } else bad = true;
    if (bad || cur < 0 || k < 0 || i < 0) { bad = true; break; }
    if (cur == sM) {
      float v0, v1, v2, v3, v4;
      if (prev == sM) { v0 = rlf(bp[0], dd); v1 = rlf(bp[1], dd); v2 = rlf(bp[2], dd); v3 = rlf(bp[3], dd); v4 = rlf(bp[4], dd); }
      else { v0 = post(i, k, 3); v1 = post(i, k, 4); v2 = post(i, k, 5); v3 = post(i, k, 6); v4 = post(i, k, 7); }
      c = 1; float b = v0;
      if (v1 > b) { b = v1; c = 2; }
      if (v2 > b) { b = v2; c = 3; }
      if (v3 > b) { b = v3; c = 4; }
      if (v4 > b) { b = v4; c = 5; }
    } else c = 0;
    push(cur, k, i, c);
    if ((cur == sN || cur == sC || cur == sJ) && cur == prev) i--;
    prev = cur;
    i -= c;
    if (n > cap) bad = true;
  }
  if (bad) { if (lane == 0) out[job] = r; return; }
  __threadfence();                                                            // the trace entries, written by lane 0 or a lane each, read below by every lane
  {
    // forward order = T[n-1] .. T[0]
    const float *n2 = null2 + (size_t)job * kKp;
    // the first and the last match state
    int z1 = n, z2 = -1;
    for (int zb = 0; zb < n; zb += 64) {
      const int z = zb + lane;
      const bool isM = z < n && (int)(T[n - 1 - z].x & 0xffu) == sM;
      const unsigned long long m = __ballot(isM);
      if (m) { if (z1 == n) z1 = zb + __ffsll((long long)m) - 1; z2 = zb + 63 - __clzll((long long)m); }
    }
    if (z1 < n && z2 >= 0) {
      r.ok = 1;
      const uint2 e1 = T[n - 1 - z1], e2 = T[n - 1 - z2];
      r.ihmm = (int)(e1.x >> 16); r.jhmm = (int)(e2.x >> 16);
      r.iali = (int)e1.y - ((int)((e1.x >> 8) & 0xffu) - 1); r.jali = (int)e2.y;
      // ---- the correction: the reference's loop over the residues, on chunks of the trace and of the residues held a lane each
      float corr = 0.f;
      int nshift = 0;
      {
        int t = -1, u = -1, v = -1, w = -1, x = -1, pos = 1, z = 0;
        int zb = 0, pb = 1;                                                   // the chunks: lane l holds entry zb + l, residue pb + l
        uint2 te = (zb + lane < n) ? T[n - 1 - (zb + lane)] : make_uint2(0u, 0u);
        int re = (pb + lane <= L) ? (int)dsq[pb + lane] : 0;
        int pk = 0, pc = 0, npend = 0;                                        // pending look-ups: lane e holds (node, codon index) of the e-th
        auto flush = [&]() {
          float sc = 0.f;
          if (lane < npend) sc = logf(n2[codons[(size_t)pk * maxcodons + pc]]);
          for (int l = 0; l < npend; l++) { const float q = rlf(sc, l); if (q != -INFINITY) corr += q; }
          npend = 0;
        };
        while (pos <= L && z < n) {
          pos = uni(pos); z = uni(z);
          if (z - zb >= 64) { zb = z; te = (zb + lane < n) ? T[n - 1 - (zb + lane)] : make_uint2(0u, 0u); }
          if (pos - pb >= 64) { pb = pos; re = (pb + lane <= L) ? (int)dsq[pb + lane] : 0; }
          const int rv = __builtin_amdgcn_readlane(re, pos - pb);
          x = rv < 4 ? rv : 1367;
          const unsigned ex = (unsigned)__builtin_amdgcn_readlane((int)te.x, z - zb);
          const int ei = __builtin_amdgcn_readlane((int)te.y, z - zb);
          const int s = (int)(ex & 0xffu), cz = (int)((ex >> 8) & 0xffu), kz = (int)(ex >> 16);
          if (s == sN || s == sC || s == sJ) { if (ei == pos && pos > 2) pos++; z++; }
          else if (s == sM || s == sI) {
            if (ei == pos) {
              int ci, capi;
              if (s == sI) { ci = x * 341 + w * 85 + v * 21 + 2; capi = 1364; }
              else {
                switch (cz) {
                case 1: ci = x * 341; capi = 1366; break;
                case 2: ci = x * 341 + w * 85 + 1; capi = 1365; break;
                case 3: ci = x * 341 + w * 85 + v * 21 + 2; capi = 1364; break;
                case 4: ci = x * 341 + w * 85 + v * 21 + u * 5 + 3; capi = 1365; break;
                default: ci = x * 341 + w * 85 + v * 21 + u * 5 + t + 4; capi = 1366; break;
                }
                if (cz != 3) nshift++;
              }
              if (lane == npend) { pk = kz; pc = min(ci, capi); }
              if (++npend == 64) flush();
              z++;
            }
            pos++;
          } else z++;
          t = u; u = v; v = w; w = x;
        }
        flush();
      }
      r.nshift = nshift;
      r.domcorrection = corr;
      // ---- the columns (p7_alidisplay_fs_Create, p7_pli_computeAliScores_BATH), a lane each; the score summed in column order
      r.ncol = z2 - z1 + 1;
      int col_off = 0;
      if (steps) { if (lane == 0) col_off = atomicAdd(col_cursor, r.ncol); col_off = uni(col_off); }
      r.col_off = col_off;
      uint16_t *S = steps ? steps + col_off : nullptr;
      float *SP = (steps && step_pp) ? step_pp + col_off : nullptr;
      float ali = 0.f;
      int nstops = 0, exact = 0;
      for (int zb = z1; zb <= z2; zb += 64) {
        const int zz = zb + lane;
        const bool in = zz <= z2;
        float colsc = 0.f;
        bool stop = false, same = false;
        if (in) {
          const uint2 e = T[n - 1 - zz];
          const int s = (int)(e.x & 0xffu), cc0 = (int)((e.x >> 8) & 0xffu), kk = (int)(e.x >> 16), ii = (int)e.y;
          const int prevs = (zz == z1) ? (int)sB : (int)(T[n - zz].x & 0xffu);
          const int cc = (s == sM) ? cc0 : (s == sI ? 3 : 0);
          unsigned code = (unsigned)s;
          if (s == sI) colsc = tf[(size_t)kk * 8 + (prevs == sI ? 7 : 6)];
          else if (s == sD) colsc = tf[(size_t)(kk - 1) * 8 + (prevs == sD ? 5 : 4)];
          if (cc > 0 && ii - cc + 1 >= 1 && ii <= L) {
            int nn[5] = {0, 0, 0, 0, 0};
            bool degen = false;
            for (int q = 0; q < cc; q++) { nn[q] = dsq[ii - cc + 1 + q]; degen |= nn[q] >= 4; }
            int ci;
            switch (cc) {
            case 1: ci = degen ? 1366 : nn[0] * 341; break;
            case 2: ci = degen ? 1365 : nn[1] * 341 + nn[0] * 85 + 1; break;
            case 3: ci = degen ? 1364 : nn[2] * 341 + nn[1] * 85 + nn[0] * 21 + 2; break;
            case 4: ci = degen ? 1365 : nn[3] * 341 + nn[2] * 85 + nn[1] * 21 + nn[0] * 5 + 3; break;
            default: ci = degen ? 1366 : nn[4] * 341 + nn[3] * 85 + nn[2] * 21 + nn[1] * 5 + nn[0] + 4; break;
            }
            const int indel = indel_tab ? indel_tab[(size_t)kk * maxcodons + ci] : 5;
            stop = (cc == 3) && (indel == 6 || indel == 7 || indel == 8);
            same = s == sM && cons && codons[(size_t)kk * maxcodons + ci] == cons[kk];
            code |= (unsigned)cc << 4 | (unsigned)indel << 8;
            if (s == sM && amino) {
              colsc = amino[(size_t)codons[(size_t)kk * maxcodons + ci] * pitch + kk];
              if (prevs == sI) colsc += tf[(size_t)kk * 8 + 1];
              else if (prevs == sD) colsc += tf[(size_t)kk * 8 + 2];
              else if (prevs == sM && zz < z2) colsc += tf[(size_t)kk * 8 + 0];
            }
          }
          if (S) S[zz - z1] = (uint16_t)code;
          if (SP) SP[zz - z1] = (s == sM) ? post(ii, kk, 2) : (s == sI ? post(ii, kk, 1) : 0.0f);
        }
        nstops += __popcll(__ballot(stop)); exact += __popcll(__ballot(same));
        const int nin = min(64, z2 - zb + 1);
        for (int l = 0; l < nin; l++) ali += rlf(colsc, l);
      }
      r.nstops = nstops; r.exact = exact;
      r.aliscore = ali;
    }
  }
  if (lane == 0) out[job] = r;
}

__global__ void fs5_null2_kernel(int64_t n, const int32_t *__restrict__ len, int M, int pitch, const float *__restrict__ amino /* rsc + maxcodons*pitch */,
                                 const float *__restrict__ logsum, const float *__restrict__ colsum, float *__restrict__ null2 /* [n][Kp] */) {
  const int64_t job = blockIdx.x;
  const int x = threadIdx.x;
  if (job >= n) return;
  const int Ld = len[job];
  float *out = null2 + (size_t)job * kKp;
  if (Ld < 5) { if (x < kKp) out[x] = 1.0f; return; }
  const float *cs = colsum + (size_t)job * ((size_t)(M + 1) * 8 + 8);
  const float *xs = cs + (size_t)(M + 1) * 8;
  const float lld = (float)-log((double)(float)Ld);
  __shared__ float res[20];
  if (x < 20) {
    float xf = (float)log((double)xs[1]) + lld;
    xf = flogsum_g(xf, (float)log((double)xs[4]) + lld, logsum);
    xf = flogsum_g(xf, (float)log((double)xs[2]) + lld, logsum);
    float v = -INFINITY;
    for (int k = 1; k < M; k++) {
      v = flogsum_g(v, ((float)log((double)cs[(size_t)k * 8 + 2]) + lld) + amino[(size_t)x * pitch + k], logsum);
      v = flogsum_g(v, (float)log((double)cs[(size_t)k * 8 + 1]) + lld, logsum);
    }
    v = flogsum_g(v, ((float)log((double)cs[(size_t)M * 8 + 2]) + lld) + amino[(size_t)x * pitch + M], logsum);
    v = flogsum_g(v, xf, logsum);
    res[x] = expf(v);
    out[x] = res[x];
  }
  __syncthreads();
  if (x == 0) {
    // esl_abc_FAvgScVec: degenerate residues = plain mean over members; gap, '*', '~' = 1
    const int mem[5][2] = {{2, 11}, {7, 9}, {3, 13}, {8, 8}, {1, 1}};
    for (int dx = 0; dx < 5; dx++) {
      const int a = mem[dx][0], b = mem[dx][1];
      out[21 + dx] = (a == b) ? res[a] / 1.0f : ((a < b ? res[a] + res[b] : res[b] + res[a]) / 2.0f);
    }
    float s = 0.f;
    for (int y = 0; y < 20; y++) s += res[y];
    out[26] = s / 20.0f;
    out[20] = 1.0f; out[27] = 1.0f; out[28] = 1.0f;
  }
}

}  // namespace bath

// A batch of envelopes between the stages of fs5_envelopes_ex; per envelope, rows = L+1: fwd rows*(M+1)*8, bck / oa rows*(M+1)*3, xmx rows*5
struct Fs5EnvBatch {
  std::vector<int64_t> foff, boff, xoff;   // where envelope i's Forward matrix, Backward / OA matrix and special-state rows start, in floats
  int64_t *d_foff, *d_boff, *d_xoff;       // ... on the device, back to back in Scratch::kEnvOffsets
  float *d_fsc, *d_bsc, *d_osc;            // Forward, Backward and OA scores, back to back in Scratch::kEnvScores
  float *d_ox;                             // Scratch::kFs5OaRows, or null: the caller wants neither <oax> nor a trace
  double cells5;                           // (L+1) x (M+1) cells of all envelopes
  size_t cs_stride;                        // floats per envelope in Scratch::kEnvNull2Work: null2's column sums
  // The posterior matrix (32 B per cell) is written only when the caller wants it back (<pp>): the pipeline reads posteriors along the
  // optimal-accuracy trace only (O(L + M) cells of (L+1)(M+1)), and fs5_trace_kernel forms those from the Forward and Backward matrices --
  // which then stay as they are -- and the rows' normalising factors (4 B per ROW) with the decoding kernels' own arithmetic, value for value
  bool store_pp;
  float *d_rowden;                         // Scratch::kFs5RowDenominators, or null: the posterior matrix is stored
  FsJobs jq[4];                            // Forward, Backward's sweep, decoding, Backward's special-state rows
};

// The batch's buffers, and its offsets on their way to the device
static int fs5_env_upload(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, bool want_ox, Fs5EnvBatch &b) {
  const int64_t n = dna->n; const int M = om->M;
  b.cs_stride = (size_t)(M + 1) * 8 + 8;
  b.foff = fs_row_offsets(dna, (int64_t)(M + 1) * 8); b.boff = fs_row_offsets(dna, (int64_t)(M + 1) * 3); b.xoff = fs_row_offsets(dna, 5);
  const std::vector<int64_t> &foff = b.foff, &boff = b.boff, &xoff = b.xoff;
  DevBuf &b_f = ctx->scratch[Scratch::kEnvFwdMatrix], &b_b = ctx->scratch[Scratch::kEnvBwdMatrix], &b_o = ctx->scratch[Scratch::kFs5OaMatrix], &b_fx = ctx->scratch[Scratch::kEnvFwdRows], &b_bx = ctx->scratch[Scratch::kEnvBwdRows];
  DevBuf &b_off = ctx->scratch[Scratch::kEnvOffsets], &b_sc = ctx->scratch[Scratch::kEnvScores], &b_cs = ctx->scratch[Scratch::kEnvNull2Work], &b_n2 = ctx->scratch[Scratch::kEnvNull2], &b_ox = ctx->scratch[Scratch::kFs5OaRows];
  DevBuf &b_rowden = ctx->scratch[Scratch::kFs5RowDenominators];
  if (want_ox) BATH_HIP_TRY(ctx, b_ox.reserve((size_t)xoff[n] * 4 + 64));
  BATH_HIP_TRY(ctx, b_f.reserve((size_t)foff[n] * 4 + 64)); BATH_HIP_TRY(ctx, b_b.reserve((size_t)boff[n] * 4 + 64)); BATH_HIP_TRY(ctx, b_o.reserve((size_t)boff[n] * 4 + 64));
  BATH_HIP_TRY(ctx, b_fx.reserve((size_t)xoff[n] * 4 + 64)); BATH_HIP_TRY(ctx, b_bx.reserve((size_t)xoff[n] * 4 + 64));
  BATH_HIP_TRY(ctx, b_off.reserve((size_t)(n + 1) * 3 * sizeof(int64_t)));
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 3 * sizeof(float)));
  BATH_HIP_TRY(ctx, b_cs.reserve((size_t)n * b.cs_stride * sizeof(float)));
  BATH_HIP_TRY(ctx, b_n2.reserve((size_t)n * kKp * sizeof(float)));
  BATH_HIP_TRY(ctx, b_rowden.reserve((size_t)(xoff[(size_t)n] / 5 + 8) * sizeof(float)));
  b.d_foff = b_off.as<int64_t>(); b.d_boff = b.d_foff + (n + 1); b.d_xoff = b.d_boff + (n + 1);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(b.d_foff, foff.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(b.d_boff, boff.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(b.d_xoff, xoff.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  b.d_fsc = b_sc.as<float>(); b.d_bsc = b.d_fsc + n; b.d_osc = b.d_bsc + n;
  b.d_ox = want_ox ? b_ox.as<float>() : nullptr;
  b.d_rowden = b.store_pp ? nullptr : b_rowden.as<float>();
  b.cells5 = (double)(foff[(size_t)n] / 8);
  return BATH_OK;
}

// Forward and Backward: the row-per-lane wavefronts (bath_fs_wavefront.hip), the reference's order of every sum, in EVERY mode --
// the unihit recursion has no sum that a scan could shorten, so the fast mode's envelopes are the strict ones (the node-per-lane
// scan kernels this replaced in fast mode were 13 times slower at 1024 nodes and are gone)
// (odds5: the odds-ratio kernels of bath_fs5_odds.hip, node per lane; Backward with scales of its own, so still beside Forward)
static int fs5_env_forward_backward(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, bool odds5, bool exact, int c5_compat, Fs5EnvBatch &b) {
  int st;
  auto &s = ctx->scratch;
  float *f = s[Scratch::kEnvFwdMatrix].as<float>(), *fx = s[Scratch::kEnvFwdRows].as<float>(), *bk = s[Scratch::kEnvBwdMatrix].as<float>(), *bx = s[Scratch::kEnvBwdRows].as<float>();
  if ((st = fs_schedule(ctx, dna, 4, b.jq)) != BATH_OK) return st;
  if ((st = fs_fork(ctx)) != BATH_OK) return st;                                // Backward on the side stream, concurrently with Forward
  const int s1 = ctx->span_begin(odds5 ? "fs5_fwd_odds_kernel" : "fs5_fwd_kernel", ctx->stream, b.cells5, b.cells5 * 32.0);
  if (odds5) st = launch_fs5_odds(ctx, ctx->stream, om, dna, kFs5OddsEnvFwd, b.d_fsc, f, b.d_foff, fx, b.d_xoff, -1, b.jq[0], nullptr);
  else st = launch_fs5_fwd_wf(ctx, ctx->stream, om, dna, exact, c5_compat, b.d_fsc, f, b.d_foff, fx, b.d_xoff, s[Scratch::kFs5FwdRing], b.jq[0]);
  if (st != BATH_OK) return st;
  ctx->span_end(s1, ctx->stream);
  static const bool serial_env = [] { const char *e = std::getenv("BATH_HIP_FS_SERIAL"); return e && e[0] == '1'; }();   // timing probes: Backward after Forward
  const bool serial = ctx->fs_serial >= 0 ? ctx->fs_serial != 0 : serial_env;                                           // (bath_hip_set_fs_serial)
  hipStream_t bs = serial ? ctx->stream : ctx->side_stream;
  const int s2 = ctx->span_begin(odds5 ? "fs5_bwd_odds_kernel" : "fs_bwd_kernel<5>", bs, b.cells5, b.cells5 * 12.0);
  if (odds5) st = launch_fs5_odds(ctx, bs, om, dna, kFs5OddsEnvBwd, b.d_bsc, bk, b.d_boff, bx, b.d_xoff, -1, b.jq[1], nullptr);
  else st = launch_fs5_bwd_wf(ctx, bs, om, dna, exact, b.d_bsc, bk, b.d_boff, bx, b.d_xoff, s[Scratch::kFs5BwdRing], s[Scratch::kFs5BwdTerms], s[Scratch::kFs5BwdTermOffsets], b.jq[1], b.jq[3]);
  if (st != BATH_OK) return st;
  ctx->span_end(s2, bs);
  return fs_join(ctx);
}

// decoding + optimal-accuracy fill, one walk over the rows
static int fs5_env_decode_oa(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, const Fs5EnvBatch &b) {
  int st;
  const int64_t n = dna->n; const int M = om->M;
  auto &s = ctx->scratch;
  float *f = s[Scratch::kEnvFwdMatrix].as<float>(), *fx = s[Scratch::kEnvFwdRows].as<float>(), *bk = s[Scratch::kEnvBwdMatrix].as<float>(), *bx = s[Scratch::kEnvBwdRows].as<float>();
  float *cs = s[Scratch::kEnvNull2Work].as<float>(), *o = s[Scratch::kFs5OaMatrix].as<float>();
  BATH_HIP_TRY(ctx, hipMemsetAsync(cs, 0, (size_t)n * b.cs_stride * sizeof(float), ctx->stream));
  const int Cv = BATH_TILING_PICK(BATH_FS_COLUMNS, M);
  const size_t oa_shmem = (size_t)(M + 2) * 8 * sizeof(float);
  BATH_FS_SWITCH(Cv, {
    int mw_nodes = 0;
    // reads Forward 32 + Backward 12, writes OA 12 B/cell -- and the posteriors, 32 more, only when the caller asked for the matrix
    const double oa_bytes = b.cells5 * (b.store_pp ? 88.0 : 56.0);
    if (fs5_decode_oa_mw_shape(M, &mw_nodes) > 0) {        // long models: a block of waves per envelope (bath_fs_decode.hip)
      const int s3 = ctx->span_begin("fs5_decode_oa_kernel", ctx->stream, b.cells5, oa_bytes);
      if ((st = launch_fs5_decode_oa_mw(ctx, ctx->stream, om, dna, b.d_bsc, f, b.d_foff, fx, b.d_xoff, bk, b.d_boff, bx,
                                        cs, o, b.d_osc, b.d_ox, b.jq[2], b.store_pp ? 1 : 0, b.d_rowden)) != BATH_OK) return st;
      ctx->span_end(s3, ctx->stream);
    } else {
      if ((st = fs_set_shmem(ctx, fs5_decode_oa_kernel<CC>, oa_shmem)) != BATH_OK) return st;
      const int s3 = ctx->span_begin("fs5_decode_oa_kernel", ctx->stream, b.cells5, oa_bytes);
      const int oa_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)ctx->prop.multiProcessorCount * (CC <= 3 ? BATH_FS_OA_WAVES : 1)));
      hipLaunchKernelGGL((fs5_decode_oa_kernel<CC>), dim3(oa_grid), dim3(256), oa_shmem, ctx->stream, dna->view(), M, om->d_tf, om->d_loop[1], b.d_bsc, f, b.d_foff,
                         fx, b.d_xoff, bk, b.d_boff, bx, cs, o, b.d_osc,
                         1.17549435e-38f /* E->J impossible in unihit mode: TSCDELTA = FLT_MIN */, 1.0f, b.d_ox, b.jq[2],
                         b.store_pp ? 1 : 0, b.d_rowden);
      ctx->span_end(s3, ctx->stream);
    }
  })
  return BATH_OK;
}

static int fs5_env_null2(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna) {
  const int64_t n = dna->n; const int M = om->M;
  const int s5 = ctx->span_begin("fs5_null2_kernel", ctx->stream, (double)n * M, (double)n * M * 32.0);
  hipLaunchKernelGGL(fs5_null2_kernel, dim3((unsigned)n), dim3(32), 0, ctx->stream, n, dna->d_len, M, om->pitch, om->d_rsc + (size_t)om->maxcodons * om->pitch, om->d_logsum,
                     ctx->scratch[Scratch::kEnvNull2Work].as<float>(), ctx->scratch[Scratch::kEnvNull2].as<float>());
  ctx->span_end(s5, ctx->stream);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// optimal-accuracy traceback + null2 along the trace, on the device; the trace records and the columns to the host
static int fs5_env_trace(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, const Fs5EnvBatch &b, FsTraceOut *trace,
                         const uint8_t *cons, std::vector<uint16_t> *steps, std::vector<int64_t> *step_off, std::vector<float> *step_pp) {
  const int64_t n = dna->n; const int M = om->M;
  if (!om->d_codons) { ctx->set_error("traceback needs the profile's codon table"); return BATH_EINVAL; }
  std::vector<int64_t> toff((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; i++) toff[(size_t)i + 1] = toff[(size_t)i] + dna->h_len[(size_t)i] + M + 16;
  DevBuf &b_tb = ctx->scratch[Scratch::kEnvTraceColumns], &b_to = ctx->scratch[Scratch::kFs5TraceOut], &b_steps = ctx->scratch[Scratch::kFs5TraceSteps];
  BATH_HIP_TRY(ctx, b_tb.reserve((size_t)toff[(size_t)n] * sizeof(uint2) + (size_t)(n + 1) * sizeof(int64_t) + 256));
  // dense columns: [cursor (256 B)] [pp: 4 B per column] [codes: 2 B per column], at most toff[n] columns
  const size_t col_cap = (size_t)toff[(size_t)n];
  if (col_cap >= (size_t)INT32_MAX) { ctx->set_error("envelope batch too large for the trace columns' 32-bit offsets: lower BATH_HIP_ENV_MB"); return BATH_ERANGE; }
  if (steps) BATH_HIP_TRY(ctx, b_steps.reserve(256 + col_cap * (sizeof(float) + sizeof(uint16_t)) + 64));
  int *d_cursor = steps ? b_steps.as<int>() : nullptr;
  float *d_step_pp = steps ? reinterpret_cast<float *>(b_steps.as<char>() + 256) : nullptr;
  uint16_t *d_steps = steps ? reinterpret_cast<uint16_t *>(d_step_pp + col_cap) : nullptr;
  if (steps) BATH_HIP_TRY(ctx, hipMemsetAsync(d_cursor, 0, sizeof(int), ctx->stream));
  BATH_HIP_TRY(ctx, b_to.reserve((size_t)n * sizeof(FsTraceOut) + 64));
  int64_t *d_toff = reinterpret_cast<int64_t *>(b_tb.as<char>() + ((size_t)toff[(size_t)n] * sizeof(uint2) + 255) / 256 * 256);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_toff, toff.data(), (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  const int s6 = ctx->span_begin("fs5_trace_kernel", ctx->stream, (double)toff[(size_t)n], 0.0);
  const bool lane_trace = [] { const char *e = std::getenv("BATH_HIP_FS_TRACE_LANE"); return e && e[0] == '1'; }();      // A/B and tests: the walk by one lane
  const auto kernel = lane_trace ? fs5_trace_kernel : fs5_trace_wave_kernel;
  const unsigned grid = lane_trace ? (unsigned)((n * kTraceSpread + 63) / 64) : (unsigned)n;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, ctx->stream, dna->view(), M, om->maxcodons, om->d_tf, om->d_codons,
                     ctx->scratch[Scratch::kEnvFwdMatrix].as<float>(), b.d_foff, ctx->scratch[Scratch::kEnvFwdRows].as<float>(), b.d_xoff, ctx->scratch[Scratch::kFs5OaMatrix].as<float>(), b.d_boff,
                     b.d_ox, ctx->scratch[Scratch::kEnvNull2].as<float>(), b_tb.as<uint2>(), d_toff,
                     b_to.as<FsTraceOut>(), om->d_indel, cons, d_steps,
                     om->d_rsc + (size_t)om->maxcodons * om->pitch, om->pitch, step_pp ? d_step_pp : nullptr, d_cursor,
                     b.store_pp ? nullptr : ctx->scratch[Scratch::kEnvBwdMatrix].as<float>(), b.d_boff, b.d_bsc, b.d_rowden);
  ctx->span_end(s6, ctx->stream);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipMemcpyAsync(trace, b_to.p, (size_t)n * sizeof(FsTraceOut), hipMemcpyDeviceToHost, ctx->stream));
  if (steps) {                                                // columns z1..z2 of envelope e: (*steps)[step_off[e] .. +trace[e].ncol)
    int total = 0;
    BATH_HIP_TRY(ctx, hipMemcpyAsync(&total, d_cursor, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (also: toff is a local)
    steps->resize((size_t)total);
    if (total > 0) BATH_HIP_TRY(ctx, hipMemcpyAsync(steps->data(), d_steps, (size_t)total * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    if (step_pp) {
      step_pp->resize((size_t)total);
      if (total > 0) BATH_HIP_TRY(ctx, hipMemcpyAsync(step_pp->data(), d_step_pp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    step_off->assign((size_t)n + 1, (int64_t)total);
    for (int64_t e = 0; e < n; e++) (*step_off)[(size_t)e] = trace[e].ok ? (int64_t)trace[e].col_off : (int64_t)total;
  }
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));       // toff is a local
  return BATH_OK;
}

// scores and null2 into <res>; the matrices and rows the caller asked for
static int fs5_env_download(bath_hip_ctx *ctx, int64_t n, const Fs5EnvBatch &b, bath_fs5_result *res, float *pp, float *oa, float *ppx, float *oax) {
  std::vector<float> h_sc((size_t)n * 3), h_n2((size_t)n * kKp);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h_sc.data(), b.d_fsc, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h_n2.data(), ctx->scratch[Scratch::kEnvNull2].p, (size_t)n * kKp * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (pp) BATH_HIP_TRY(ctx, hipMemcpyAsync(pp, ctx->scratch[Scratch::kEnvFwdMatrix].p, (size_t)b.foff[n] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (oa) BATH_HIP_TRY(ctx, hipMemcpyAsync(oa, ctx->scratch[Scratch::kFs5OaMatrix].p, (size_t)b.boff[n] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (ppx) BATH_HIP_TRY(ctx, hipMemcpyAsync(ppx, ctx->scratch[Scratch::kEnvFwdRows].p, (size_t)b.xoff[n] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (oax) BATH_HIP_TRY(ctx, hipMemcpyAsync(oax, b.d_ox, (size_t)b.xoff[n] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < n; i++) {
    res[i].fwdsc = h_sc[i]; res[i].bcksc = h_sc[n + i]; res[i].oasc = h_sc[2 * n + i];
    std::memcpy(res[i].null2, &h_n2[(size_t)i * kKp], sizeof(float) * kKp);
  }
  return BATH_OK;
}

// Envelope rescoring; layouts per envelope i, rows = L_i+1: pp rows*(M+1)*8, oa rows*(M+1)*3, ppx / oax rows*5
// {E,N,J,B,C} (posterior and OA special-state rows), each packed back to back in envelope order.
int bath::fs5_envelopes_ex(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                           bath_fs5_result *res, float *pp, float *oa, float *ppx, float *oax, FsTraceOut *trace,
                           const uint8_t *cons, std::vector<uint16_t> *steps, std::vector<int64_t> *step_off, std::vector<float> *step_pp) {
  if (!ctx || !om || !dna || om->codon_lengths != 5) { if (ctx) ctx->set_error("fs5 envelopes need a 5-codon profile"); return BATH_EINVAL; }
  if (logsum_mode == BATH_LOGSUM_ODDS) { ctx->set_error("the 5-codon kernels have no odds-ratio mode"); return BATH_EINVAL; }
  if (fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (dna->n == 0) return BATH_OK;
  int st = om->ensure_len(dna->maxlen / 3 + 1);
  if (st != BATH_OK) return st;
  Fs5EnvBatch b;
  b.store_pp = pp != nullptr;
  if ((st = fs5_env_upload(ctx, om, dna, oax || trace, b)) != BATH_OK) return st;
  // BATH_LOGSUM_CONTEXT: the odds-ratio kernels while bath_hip_set_fs5_odds is on (before fs_strict), else strict / fast
  const bool odds5 = logsum_mode == BATH_LOGSUM_CONTEXT && ctx->fs5_odds;
  if (odds5 && c5_compat) { ctx->set_error("the 5-codon odds-ratio mode implements c5_compat = 0 only (fwdback_fs.c:1464)"); return BATH_EINVAL; }
  if (odds5 && (st = om->ensure_odds()) != BATH_OK) return st;                  // (the first call builds the tables: before the streams fork)
  if (logsum_mode == BATH_LOGSUM_CONTEXT) logsum_mode = ctx->fs_strict ? BATH_LOGSUM_TABLE_SERIAL : BATH_LOGSUM_TABLE;
  if ((st = fs5_env_forward_backward(ctx, om, dna, odds5, logsum_mode == BATH_LOGSUM_EXACT, c5_compat, b)) != BATH_OK) return st;
  if ((st = fs5_env_decode_oa(ctx, om, dna, b)) != BATH_OK) return st;
  if ((st = fs5_env_null2(ctx, om, dna)) != BATH_OK) return st;
  if (trace && (st = fs5_env_trace(ctx, om, dna, b, trace, cons, steps, step_off, step_pp)) != BATH_OK) return st;
  return fs5_env_download(ctx, dna->n, b, res, pp, oa, ppx, oax);
}

extern "C" int bath_hip_fs5_envelopes(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                                      bath_fs5_result *res, float *pp, const int64_t *pp_off_h, float *oa, const int64_t *oa_off_h) {
  (void)pp_off_h; (void)oa_off_h;
  return bath::fs5_envelopes_ex(ctx, om, dna, logsum_mode, c5_compat, res, pp, oa, nullptr, nullptr, nullptr);
}

extern "C" int bath_hip_fs5_envelopes_x(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                                        bath_fs5_result *res, float *pp, float *oa, float *ppx, float *oax) {
  return bath::fs5_envelopes_ex(ctx, om, dna, logsum_mode, c5_compat, res, pp, oa, ppx, oax, nullptr);
}
