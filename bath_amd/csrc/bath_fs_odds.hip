// bath_fs_odds.hip -- the 3-codon frameshift Forward and Backward parsers in odds-ratio (probability) space, BATH_LOGSUM_ODDS:
// what the reference's bathsearch --fs runs (p7_ForwardParser_Frameshift_3Codons impl_sse/fwdback_fs.c:97-533,
// p7_BackwardParser_Frameshift_3Codons :565-1050), not the log-space generic recursion the other modes restate.
//
//   fs3_fwd_odds_kernel<C>  IVX(i,k) = B(i-2) tBM(k-1) + M(i-2,k-1) tMM(k-1) + I(i-2,k-1) tIM(k-1) + D(i-2,k-1) tDM(k-1)
//                           M(i,k)   = IVX(i,k) e2(k) + IVX(i-1,k) e3(k) + IVX(i-2,k) e4(k)
//                           I(i,k)   = M(i-3,k) tMI(k) + I(i-3,k) tII(k)
//                           D(i,k)   = M(i,k-1) tMD(k-1) + D(i,k-1) tDD(k-1)
//                           E(i)     = sum_k M(i,k) + D(i,k);  N, J, B, C from row i-3 (fwdback_fs.c:462-465)
//   fs3_bwd_odds_kernel<C>  the mirror image, rows L down to 0; with rows beyond L held at zero one formula covers every row
//                           case of the generic code (oracle/sse/sse_fs.c documents the derivation)
//
// One wave per DNA window (the longest-first job list), lane l owns the C consecutive nodes l*C+1 .. l*C+C.  Without log-sums the
// D row is an affine recurrence D(k+1) = tDD(k) D(k) + M(k) tMD(k): each lane composes its C steps into one map x -> m x + a, a
// 6-step DPP scan composes the maps across the wave, and D at a lane's first node is the exclusive prefix.  E(i) and B(i) are
// DPP sums.  There is no log-sum table and no LDS: a row is about 12 C multiply-adds and two 6-step scans per lane, so a wave
// costs a few hundred cycles per row where the log-space chains cost a dependent table look-up per node.
//
// Rescaling as the reference's (fwdback_fs.c:467-495): when E(i) (Backward: B(i)) passes 1e4, every value a later row reads --
// the register rows of M, D, I and IVX and the special-state rings -- is multiplied by 1/E(i) together, and log E(i) joins the
// running scale.  The special-state rows leave the kernel in LOG space, log(value) + the running scale, in the (L+1) x
// {E,N,J,B,C} layout of the other modes, so the region heuristics and domain decoding read them unchanged.
#include <cmath>
#include <cstring>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

#include "bath_fs_device.hpp"

namespace bath {

constexpr int kDegen3 = 338;             // p7P_MAXCODONS3: marks a degenerate nucleotide (rows 336 / 337 are the degenerate codons)

// (wave-uniform: the emission rows' addresses stay in scalar registers)
__device__ __forceinline__ int nuc3(uint8_t c) { return __builtin_amdgcn_readfirstlane(c < 4 ? (int)c : kDegen3); }

// emissions fetched one row ahead, off the row's dependency chain, while the registers allow it
template <int C> constexpr bool odds_ahead() { return C <= 8; }

// ---------------------------------------------------------------------------------------------
// Forward.  Rows of M, I (i-1, i-2, i-3), D and IVX (i-1, i-2) live in registers; index 0 = the most recent row.
// tf[node] = {tMM(k-1), tIM(k-1), tDM(k-1), tBM(k-1), tMD(k), tDD(k), tMI(k), tII(k)}
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kOddsBlock) void fs3_fwd_odds_kernel(SeqView dna, FsOddsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                                   float tE, float *__restrict__ sc, float *__restrict__ xmx, const int64_t *__restrict__ xmx_off, FsJobs jobs) {
  const int lane = threadIdx.x & 63;
  const float tEL = expf(tE), tEM = tEL;
  for (int64_t job = fs_next_job(jobs, dna.n, lane); job >= 0; job = fs_next_job(jobs, dna.n, lane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *xo = xmx ? xmx + xmx_off[job] : nullptr;
    if (L < 3) { if (lane == 0) sc[job] = -INFINITY; continue; }
    const float tNL = expf(loop_tab[L / 3]), tNM = expf(move_tab[L / 3]), tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    float Mr[3][C], Ir[3][C], Dr[2][C], iv1[C], iv2[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
      Mr[0][c] = Mr[1][c] = Mr[2][c] = Ir[0][c] = Ir[1][c] = Ir[2][c] = 0.f;
      Dr[0][c] = Dr[1][c] = iv1[c] = iv2[c] = 0.f;
    }
    // specials of rows i-1, i-2, i-3: rows 0 and 1 hold N = 1, B = tNM (:448-452)
    float xN[3] = {1.f, 1.f, 1.f}, xJ[3] = {0.f, 0.f, 0.f}, xC[3] = {0.f, 0.f, 0.f}, xB[3] = {tNM, tNM, tNM};
    double totscale = 0.0;
    if (xo && lane == 0) for (int i = 0; i < 2; i++) put_row(xo, i, 0.f, 1.f, 0.f, tNM, 0.f, 0.0);
    // emissions of row i: codons ending at x_i (x, w, v, u = x_i, x_{i-1}, x_{i-2}, x_{i-3})
    float e2n[C], e3n[C], e4n[C];
    auto fetch = [&](int xx, int ww, int vv, int uu) {
      const float *q2 = p.rsc + imin(xx * 84 + ww * 21, 337) * p.pitch + lane * C + 1;
      const float *q3 = p.rsc + imin(xx * 84 + ww * 21 + vv * 5 + 1, 336) * p.pitch + lane * C + 1;
      const float *q4 = p.rsc + imin(xx * 84 + ww * 21 + vv * 5 + uu + 2, 337) * p.pitch + lane * C + 1;
#pragma unroll
      for (int c = 0; c < C; c++) { e2n[c] = q2[c]; e3n[c] = q3[c]; e4n[c] = q4[c]; }
    };
    int u = kDegen3, v = kDegen3, w = kDegen3, x = nuc3(d[0]);
    int xn = nuc3(d[1]);
    if (odds_ahead<C>()) fetch(xn, x, w, v);
    for (int i = 2; i <= L; i++) {
      u = v; v = w; w = x; x = xn;
      if (!odds_ahead<C>()) fetch(x, w, v, u);
      float e2[C], e3[C], e4[C];
#pragma unroll
      for (int c = 0; c < C; c++) { e2[c] = e2n[c]; e3[c] = e3n[c]; e4[c] = e4n[c]; }
      if (i < L) { xn = nuc3(d[i]); if (odds_ahead<C>()) fetch(xn, x, w, v); }
      // row i-2 at node k-1 for the lane's first node
      const float mIn = wave_shr1(Mr[1][C - 1], 0.f), iIn = wave_shr1(Ir[1][C - 1], 0.f), dIn = wave_shr1(Dr[1][C - 1], 0.f);
      const float b2 = xB[1];
      const float *tf = per_row(p.tf);
      float Mc[C], Ic[C], Dc[C], ivc[C], dd[C];
      float mloc = 1.f, aloc = 0.f;                          // the lane's D map: D(first node of the next lane) = mloc D(first node) + aloc
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int nd = lane * C + c + 1;                     // nodes beyond M: zero transitions, so IVX, M, I and D come out 0
        const float4 ta = *reinterpret_cast<const float4 *>(tf + nd * 8);
        const float4 tb = *reinterpret_cast<const float4 *>(tf + nd * 8 + 4);
        const float m1 = (c == 0) ? mIn : Mr[1][c - 1], i1 = (c == 0) ? iIn : Ir[1][c - 1], d1 = (c == 0) ? dIn : Dr[1][c - 1];
        const float iv = b2 * ta.w + m1 * ta.x + i1 * ta.y + d1 * ta.z;
        ivc[c] = iv;
        const float mv = iv * e2[c] + iv1[c] * e3[c] + iv2[c] * e4[c];
        Mc[c] = mv;
        Ic[c] = Mr[2][c] * tb.z + Ir[2][c] * tb.w;
        dd[c] = mv * tb.x;                                   // what node k hands to D(k+1) besides D(k) tDD(k)
        aloc = aloc * tb.y + dd[c];
        mloc = mloc * tb.y;
        Dc[c] = tb.y;                                        // (tDD(k) until the chain below overwrites it)
      }
      float dcur = affine_scan_excl(mloc, aloc);
      float esum = 0.f;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const float tdd = Dc[c];
        Dc[c] = dcur;
        esum += Mc[c] + dcur;
        dcur = dcur * tdd + dd[c];
      }
      float xE = wave_sum(esum);
      float nN, nJ, nC;
      if (i == 2) { nN = 1.f; nJ = xE * tEL; nC = xE * tEM; }
      else { nN = xN[2] * tNL; nJ = xJ[2] * tJL + xE * tEL; nC = xC[2] * tCL + xE * tEM; }
      float nB = nN * tNM + nJ * tJM;
      if (xE > kOddsRescale) {                                   // wave-uniform
        const float f = 1.0f / xE;
#pragma unroll
        for (int c = 0; c < C; c++) {
          Mc[c] *= f; Ic[c] *= f; Dc[c] *= f; ivc[c] *= f;
          Mr[0][c] *= f; Mr[1][c] *= f; Ir[0][c] *= f; Ir[1][c] *= f; Dr[0][c] *= f; iv1[c] *= f;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) { xN[r] *= f; xJ[r] *= f; xC[r] *= f; xB[r] *= f; }
        nN *= f; nJ *= f; nC *= f; nB *= f;
        totscale += (double)logf(xE);                        // (a libm double log here takes 40 VGPRs of its own)
        xE = 1.0f;
      }
      if (xo && lane == 0) put_row(xo, i, xE, nN, nJ, nB, nC, totscale);
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
      xB[2] = xB[1]; xB[1] = xB[0]; xB[0] = nB;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
        Dr[1][c] = Dr[0][c]; Dr[0][c] = Dc[c];
        iv2[c] = iv1[c]; iv1[c] = ivc[c];
      }
    }
    if (lane == 0) {
      const float tot = xC[0] + xC[1] * tCL + xC[2] * tCL;    // C(L) + C(L-1) tCL + C(L-2) tCL (:513-529)
      sc[job] = (tot > 0.f && tot < INFINITY) ? (float)(totscale + (double)(logf(tot) + logf(tCM))) : -INFINITY;   // eslERANGE -> -inf, never NaN
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward.  Lanes own their nodes in DESCENDING order (logical lane = 63 - physical lane), as fs_bwd_kernel's: "the lane holding
// the next nodes" is the physical lane below, so the descending D chain is the same upward scan as Forward's.
// Rows of M (i+1 .. i+4) and I (i+1 .. i+3) in registers, index 0 = row i+1; rows beyond L are zero.
// tb[node] = {tMD(k), tMI(k), tMM(k), tDD(k), tDM(k), tII(k), tIM(k), tBM(k-1)}
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kOddsBlock) void fs3_bwd_odds_kernel(SeqView dna, FsOddsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                                   float tE, float *__restrict__ sc, float *__restrict__ xmx, const int64_t *__restrict__ xmx_off, FsJobs jobs) {
  const int M = p.M;
  const int plane = threadIdx.x & 63;
  const int lane = 63 - plane;
  const float tEL = expf(tE), tEM = tEL;
  for (int64_t job = fs_next_job(jobs, dna.n, plane); job >= 0; job = fs_next_job(jobs, dna.n, plane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *xo = xmx ? xmx + xmx_off[job] : nullptr;
    if (L < 3) { if (plane == 0) sc[job] = -INFINITY; continue; }
    const float tNL = expf(loop_tab[L / 3]), tNM = expf(move_tab[L / 3]), tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    float Mr[4][C], Ir[3][C], msk[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
      Mr[0][c] = Mr[1][c] = Mr[2][c] = Mr[3][c] = Ir[0][c] = Ir[1][c] = Ir[2][c] = 0.f;
      msk[c] = (lane * C + c + 1 <= M) ? 1.f : 0.f;
    }
    float xN[3] = {0.f, 0.f, 0.f}, xJ[3] = {0.f, 0.f, 0.f}, xC[3] = {0.f, 0.f, 0.f};     // rows i+1, i+2, i+3
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    double totscale = 0.0;
    // x_{i+1} .. x_{i+4} as x, w, v, u.  Rows with fewer than c nucleotides after them read a clamped degenerate row: the M rows
    // they multiply (beyond L) are zero.
    float e2n[C], e3n[C], e4n[C];
    auto fetch = [&](int xx, int ww, int vv, int uu) {        // the codon's LAST nucleotide is the macro's last argument
      const float *q2 = p.rsc + imin(ww * 84 + xx * 21, 337) * p.pitch + lane * C + 1;
      const float *q3 = p.rsc + imin(vv * 84 + ww * 21 + xx * 5 + 1, 336) * p.pitch + lane * C + 1;
      const float *q4 = p.rsc + imin(uu * 84 + vv * 21 + ww * 5 + xx + 2, 337) * p.pitch + lane * C + 1;
#pragma unroll
      for (int c = 0; c < C; c++) { e2n[c] = q2[c]; e3n[c] = q3[c]; e4n[c] = q4[c]; }
    };
    int u = kDegen3, v = kDegen3, w = kDegen3, x = kDegen3;
    if (odds_ahead<C>()) fetch(x, w, v, u);                  // row L: no nucleotide after it
    for (int i = L; i >= 0; i--) {
      if (!odds_ahead<C>()) fetch(x, w, v, u);
      float e2[C], e3[C], e4[C];
#pragma unroll
      for (int c = 0; c < C; c++) { e2[c] = e2n[c]; e3[c] = e3n[c]; e4[c] = e4n[c]; }
      if (i > 0) { u = v; v = w; w = x; x = nuc3(d[i - 1]); if (odds_ahead<C>()) fetch(x, w, v, u); }    // x_i: the first nucleotide after row i-1
      const float *tb = per_row(p.tb);
      float ivx[C];
      float bloc = 0.f;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int nd = lane * C + c + 1;
        ivx[c] = Mr[1][c] * e2[c] + Mr[2][c] * e3[c] + Mr[3][c] * e4[c];
        bloc += ivx[c] * tb[nd * 8 + 7];
      }
      float xB = wave_sum(bloc);
      float nN = xN[2] * tNL + xB * tNM;
      if (i == 0) {
        n0 = nN;
        if (xo && plane == 0) put_row(xo, 0, 0.f, nN, 0.f, xB, 0.f, totscale);
        break;
      }
      float nJ = xJ[2] * tJL + xB * tJM;
      float nC = (i == L) ? tCM : (i >= L - 2 ? tCL * tCM : xC[2] * tCL);
      float xE = nJ * tEL + nC * tEM;
      const float ivNext = wave_shr1(ivx[0], 0.f);            // ivx at the node after the lane's last one
      float Mc[C], Ic[C], Dc[C], bd[C], tdd[C];
      float mloc = 1.f, aloc = 0.f;                          // D(lane's first node) = mloc D(first node of the next lane) + aloc
#pragma unroll
      for (int c = C - 1; c >= 0; c--) {
        const int nd = lane * C + c + 1;
        const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
        tdd[c] = tb[nd * 8 + 3];
        bd[c] = xE * msk[c] + ivn * tb[nd * 8 + 4];
        aloc = aloc * tdd[c] + bd[c];
        mloc = mloc * tdd[c];
      }
      float dn = affine_scan_excl(mloc, aloc);               // D(i, node after the lane's last one)
#pragma unroll
      for (int c = C - 1; c >= 0; c--) {
        const int nd = lane * C + c + 1;
        const float4 t0 = *reinterpret_cast<const float4 *>(tb + nd * 8);             // tMD tMI tMM tDD
        const float4 t1 = *reinterpret_cast<const float4 *>(tb + nd * 8 + 4);         // tDM tII tIM tBM
        const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
        Mc[c] = xE * msk[c] + dn * t0.x + Ir[2][c] * t0.y + ivn * t0.z;
        Ic[c] = Ir[2][c] * t1.y + ivn * t1.z;
        dn = dn * tdd[c] + bd[c];
        Dc[c] = dn;
      }
      if (xB > kOddsRescale) {                                   // wave-uniform
        const float f = 1.0f / xB;
#pragma unroll
        for (int c = 0; c < C; c++) {
          Mc[c] *= f; Ic[c] *= f; Dc[c] *= f;
          Mr[0][c] *= f; Mr[1][c] *= f; Mr[2][c] *= f; Ir[0][c] *= f; Ir[1][c] *= f;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) { xN[r] *= f; xJ[r] *= f; xC[r] *= f; }
        n1 *= f; n2 *= f;
        nN *= f; nJ *= f; nC *= f; xE *= f;
        totscale += (double)logf(xB);
        xB = 1.0f;
      }
      (void)Dc;                                              // (a row's D is read by nothing after it: M and D of row i only need D(i, k+1))
      if (xo && plane == 0) put_row(xo, i, xE, nN, nJ, xB, nC, totscale);
      if (i == 2) n2 = nN;
      if (i == 1) n1 = nN;
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[3][c] = Mr[2][c]; Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
      }
    }
    if (plane == 0) {
      const float tot = n0 + n1 + n2;
      sc[job] = (tot > 0.f && tot < INFINITY) ? (float)(totscale + (double)logf(tot)) : -INFINITY;
    }
  }
}

}  // namespace bath

// odds-ratio tables, built on the first odds-mode call for the profile (a strict-only user pays nothing): expf of the log-space
// tables the other kernels read (-inf -> 0), padded with zeros to the 64 C nodes the kernel's lanes own
int bath_hip_fsprofile::ensure_odds() const {
  std::lock_guard<std::mutex> lock(odds_mu);
  if (d_odds_rsc) return BATH_OK;
  const int Cv = BATH_TILING_PICK(BATH_FS_COLUMNS, M);
  if (codon_lengths != 3 && codon_lengths != 5) { ctx->set_error("odds-ratio mode needs a 3- or 5-codon profile"); return BATH_EINVAL; }
  if (Cv < 0) return bath::fs_model_ok(ctx, this);
  const int nodes = 64 * Cv + 2, opitch = 64 * Cv + 4;
  // every codon, quasi-codon and degenerate row the kernels index (p7P_MAXCODONS3 / p7P_MAXCODONS5); the 5-codon kernels read node k
  // at column k-1, so that a lane's C nodes start on a 16-byte boundary when 4 divides C
  const int nrows = codon_lengths == 5 ? 1367 : bath::kDegen3, col0 = codon_lengths == 5 ? 1 : 0;
  const size_t nt = (size_t)(M + 2) * 8;
  std::vector<float> r((size_t)nrows * pitch), tf(nt), tb(nt);
  BATH_HIP_TRY(ctx, hipMemcpy(r.data(), d_rsc, r.size() * sizeof(float), hipMemcpyDeviceToHost));
  BATH_HIP_TRY(ctx, hipMemcpy(tf.data(), d_tf, nt * sizeof(float), hipMemcpyDeviceToHost));
  BATH_HIP_TRY(ctx, hipMemcpy(tb.data(), d_tb, nt * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> ro((size_t)nrows * opitch, 0.f), tfo((size_t)nodes * 8, 0.f), tbo((size_t)nodes * 8, 0.f);
  for (int row = 0; row < nrows; row++)
    for (int k = 1; k <= M; k++) ro[(size_t)row * opitch + k - col0] = std::exp(r[(size_t)row * pitch + k]);      // exp(-inf) = 0
  for (size_t a = 8; a < (size_t)(M + 1) * 8; a++) { tfo[a] = std::exp(tf[a]); tbo[a] = std::exp(tb[a]); }
  float *dr = nullptr, *dtf = nullptr, *dtb = nullptr;
  BATH_HIP_TRY(ctx, hipMalloc((void **)&dr, ro.size() * sizeof(float) + 64));
  BATH_HIP_TRY(ctx, hipMalloc((void **)&dtf, tfo.size() * sizeof(float) + 64));
  BATH_HIP_TRY(ctx, hipMalloc((void **)&dtb, tbo.size() * sizeof(float) + 64));
  BATH_HIP_TRY(ctx, hipMemcpy(dr, ro.data(), ro.size() * sizeof(float), hipMemcpyHostToDevice));
  BATH_HIP_TRY(ctx, hipMemcpy(dtf, tfo.data(), tfo.size() * sizeof(float), hipMemcpyHostToDevice));
  BATH_HIP_TRY(ctx, hipMemcpy(dtb, tbo.data(), tbo.size() * sizeof(float), hipMemcpyHostToDevice));
  odds_pitch = opitch;
  d_odds_tf = dtf; d_odds_tb = dtb;
  d_odds_rsc = dr;                                            // published last: its presence means the tables are complete
  return BATH_OK;
}

namespace bath {

int launch_fs3_odds(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, bool backward,
                    float *d_sc, float *d_xmx, const int64_t *d_xoff, FsJobs jobs) {
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  int st = om->ensure_odds();
  if (st != BATH_OK) return st;
  const FsOddsDev p = fs_odds_dev(om);
  const int grid = fs_odds_grid(ctx, n);
  const float tE = (float)-0.69314718055994529;
  BATH_FS_SWITCH(BATH_TILING_PICK(BATH_FS_COLUMNS, om->M), {
    if (backward) hipLaunchKernelGGL((fs3_bwd_odds_kernel<CC>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[0], om->d_move[0], tE, d_sc, d_xmx, d_xoff, jobs);
    else hipLaunchKernelGGL((fs3_fwd_odds_kernel<CC>), dim3(grid), dim3(kOddsBlock), 0, stream, dna->view(), p, om->d_loop[0], om->d_move[0], tE, d_sc, d_xmx, d_xoff, jobs);
  })
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath
