// bath_frameshift.hip -- the frameshift-aware parsers and the regions' Forward for gfx950, batched over DNA windows / regions, the
// frameshift profile on the device, and the region heuristics (fs_regions_kernel).  The envelopes are bath_fs_envelopes.hip.
//
//   fs3_fwd_kernel   <- p7_ForwardParser_Frameshift_3Codons  impl_sse/fwdback_fs.c:97
//                       (scalar twin p7_GForwardParser_Frameshift_3Codons generic_fwdback_frameshift.c:451)
//   fs_bwd_kernel<3> <- p7_BackwardParser_Frameshift_3Codons impl_sse/fwdback_fs.c:565  / generic :1422
//   fs5_fwd_kernel   <- p7_Forward_Frameshift                impl_sse/fwdback_fs.c:2054 / generic :64
//   fs_bwd_kernel<5> <- p7_Backward_Frameshift               impl_sse/fwdback_fs.c:2634 / generic :1035
//
// One wavefront owns one DNA window; lanes own contiguous blocks of model nodes; the nucleotide
// recurrence (rows i-1..i-5) lives in registers as ring buffers; the D->D chain along the model and
// the E-state sum are wavefront scans/reductions.  Arithmetic is the log-space arithmetic of the
// generic reference with p7_FLogsum's 16000-entry table (logsum.c:105) held in LDS, so every
// individual log-sum is bit-identical to the reference's; only the ASSOCIATION of the sums along the
// model differs (scan instead of a serial loop), which with a 0.001-nat table moves scores by
// O(1e-3) nats (the reference's own SIMD-vs-generic tolerance is 1.0 nat, fwdback_fs.c:3189).
#include <cmath>
#include <cstring>
#include <vector>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

using namespace bath;

#include "bath_fs_device.hpp"

namespace bath {

// D(i,k) = LS(M(i,k-1)+tMD(k-1), D(i,k-1)+tDD(k-1)) for this lane's nodes, chained across lanes.
// md[c] = M(i,node_c)+tMD(node_c) and dd[c] = tDD(node_c) describe the step OUT of node c.
// Returns D at the lane's nodes in Dout[]; the step into the lane's first node comes from the previous lane.
template <int C, bool EXACT>
__device__ __forceinline__ void d_chain_fwd(const float (&md)[C], const float (&dd)[C], float (&Dout)[C], const float *tbl) {
  // lane function f(x) = LS(A, x + B): value handed to the next lane's first node
  float A = -INFINITY, B = 0.f;
#pragma unroll
  for (int c = 0; c < C; c++) { A = flogsum<EXACT>(md[c], A + dd[c], tbl); B += dd[c]; }
  // lanes without a source see the identity map (A = -inf, B = 0): LS(A, -inf + B) = A, B + 0 = B
#define BATH_DCHAIN_STEP(CTRL, MASK) { const float Ap = dpp_f<CTRL, MASK>(A, -INFINITY), Bp = dpp_f<CTRL, MASK>(B, 0.f); A = flogsum<EXACT>(A, Ap + B, tbl); B = B + Bp; }
  BATH_DCHAIN_STEP(0x111, 0xf) BATH_DCHAIN_STEP(0x112, 0xf) BATH_DCHAIN_STEP(0x114, 0xf) BATH_DCHAIN_STEP(0x118, 0xf)
  BATH_DCHAIN_STEP(0x142, 0xa) BATH_DCHAIN_STEP(0x143, 0xc)
#undef BATH_DCHAIN_STEP
  const float din = wave_shr1(A, -INFINITY);
  Dout[0] = din;
#pragma unroll
  for (int c = 1; c < C; c++) Dout[c] = flogsum<EXACT>(md[c - 1], Dout[c - 1] + dd[c - 1], tbl);
}

// ---------------------------------------------------------------------------------------------
// 3-codon Forward parser.  Row convention of the reference's parser: IVX(i,k) collects the paths
// leaving row i-2 (generic_fwdback_frameshift.c:562-569), so codon lengths 2,3,4 read IVX(i), IVX(i-1), IVX(i-2).
// tf[node] = {tMM(k-1), tIM(k-1), tDM(k-1), tBM(k-1), tMD(k), tDD(k), tMI(k), tII(k)}
// ---------------------------------------------------------------------------------------------
template <int C, int MODE>
__global__ __launch_bounds__(kFsBlock, fs_min_waves(C)) void fs3_fwd_kernel(SeqView dna, FsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                      float tEL, float tEM, float *__restrict__ sc, float *__restrict__ xmx, const int64_t *__restrict__ xmx_off, FsJobs jobs) {
  constexpr bool EXACT = (MODE == 1);   // 0: table + scans, 1: exact log-sums (strict mode runs the chain kernels, bath_fs_chain.hip)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_tbl = reinterpret_cast<float *>(lds);
  float *s_tf = s_tbl + kLogsumTbl;
  fs_load_logsum_table(s_tbl, p.logsum);
  for (int i = threadIdx.x; i < (p.M + 2) * 8; i += blockDim.x) s_tf[i] = p.tf[i];
  __syncthreads();
  const int M = p.M;
  const int lane = threadIdx.x & 63;
#define LS(a, b) flogsum<EXACT>((a), (b), s_tbl)
  for (int64_t job = fs_next_job(jobs, dna.n, lane); job >= 0; job = fs_next_job(jobs, dna.n, lane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *xo = xmx ? xmx + xmx_off[job] : nullptr;
    if (L < 3) { if (lane == 0) sc[job] = -INFINITY; continue; }
    const float tNL = loop_tab[L / 3], tNM = move_tab[L / 3], tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    // rows i-1, i-2, i-3 of M/I/D (index 0 = most recent) and IVX(i-1), IVX(i-2)
    float Mr[3][C], Ir[3][C], Dr[3][C], iv1[C], iv2[C];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < C; c++) Mr[r][c] = Ir[r][c] = Dr[r][c] = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; c++) iv1[c] = iv2[c] = -INFINITY;
    // specials of rows i-1, i-2, i-3
    float xN[3] = {0.f, 0.f, 0.f}, xJ[3] = {-INFINITY, -INFINITY, -INFINITY}, xC[3] = {-INFINITY, -INFINITY, -INFINITY}, xB[3] = {tNM, tNM, tNM};
    if (xo && lane == 0) for (int i = 0; i < 2; i++) { xo[i * 5 + 0] = -INFINITY; xo[i * 5 + 1] = 0.f; xo[i * 5 + 2] = -INFINITY; xo[i * 5 + 3] = tNM; xo[i * 5 + 4] = -INFINITY; }
    int v = 338, w = 338, x = (d[0] < 4) ? d[0] : 338;                // p7P_MAXCODONS3 marks a degenerate nucleotide
    float cL = -INFINITY, cL1 = -INFINITY, cL2 = -INFINITY;           // C(L), C(L-1), C(L-2) for the final score

    // The emission scores of a row depend on the nucleotides only, not on the DP state: they are fetched one row ahead, so
    // that their trip to L2 (the table has 0.2-1.5 MB) overlaps the previous row's log-sum chains instead of heading the
    // row's dependency chain.
    float e2n[C], e3n[C], e4n[C];
    auto fetch = [&](int xx, int ww, int vv, int uu) {
      const float *q2 = p.rsc + (size_t)imin(xx * 84 + ww * 21, 337) * p.pitch;
      const float *q3 = p.rsc + (size_t)imin(xx * 84 + ww * 21 + vv * 5 + 1, 336) * p.pitch;
      const float *q4 = p.rsc + (size_t)imin(xx * 84 + ww * 21 + vv * 5 + uu + 2, 337) * p.pitch;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node <= M) { e2n[c] = q2[node]; e3n[c] = q3[node]; e4n[c] = q4[node]; } else { e2n[c] = e3n[c] = e4n[c] = -INFINITY; }
      }
    };
    int xn = (d[1] < 4) ? d[1] : 338;                                  // nucleotide of row 2
    fetch(xn, x, w, v);
    for (int i = 2; i <= L; i++) {
      v = w; w = x; x = xn;
      float e2[C], e3[C], e4[C];
#pragma unroll
      for (int c = 0; c < C; c++) { e2[c] = e2n[c]; e3[c] = e3n[c]; e4[c] = e4n[c]; }
      if (i < L) { xn = (d[i] < 4) ? d[i] : 338; fetch(xn, x, w, v); }
      // values of row i-2 at node-1 for the lane's first node
      const float mIn = wave_shr1(Mr[1][C - 1], -INFINITY), iIn = wave_shr1(Ir[1][C - 1], -INFINITY), dIn = wave_shr1(Dr[1][C - 1], -INFINITY);
      float Mc[C], Ic[C], ivc[C], md[C], dd[C];
      float eloc = -INFINITY;
      // nodes beyond M read the all -inf transition row M+1 and -inf emissions: every value below comes out -inf without a
      // branch (a per-node `if (node <= M)` splits the row into exec-masked blocks and serialises the lane's log-sums)
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1, nd = imin(node, M + 1);
        const float4 ta = *reinterpret_cast<const float4 *>(s_tf + nd * 8);
        const float4 tb = *reinterpret_cast<const float4 *>(s_tf + nd * 8 + 4);
        const float m1 = (c == 0) ? mIn : Mr[1][c - 1], i1 = (c == 0) ? iIn : Ir[1][c - 1], d1 = (c == 0) ? dIn : Dr[1][c - 1];
        float iv;
        if (i == 2) iv = xB[1] + ta.w;                                           // row 2: IVX3(2,k) = B(0) + tBM (:503)
        else iv = LS(m1 + ta.x, LS(i1 + ta.y, LS(d1 + ta.z, xB[1] + ta.w)));     // from row i-2, B(i-2)
        ivc[c] = iv;
        float mv = iv + e2[c];
        if (i > 2) { mv = LS(mv, iv1[c] + e3[c]); mv = LS(mv, iv2[c] + e4[c]); }
        Mc[c] = mv;
        const float ins = LS(Mr[2][c] + tb.z, Ir[2][c] + tb.w);
        Ic[c] = (i > 2 && node < M) ? ins : -INFINITY;
        md[c] = mv + tb.x; dd[c] = tb.y;
      }
      float Dc[C];
      d_chain_fwd<C, EXACT>(md, dd, Dc, s_tbl);
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        Dc[c] = (node <= M) ? Dc[c] : -INFINITY;
        eloc = LS(Mc[c], LS(Dc[c], eloc));                          // nodes beyond M hold -inf: the sum is unchanged
      }
      const float xE = wave_logsum<EXACT>(eloc, s_tbl);
      float nN, nJ, nC, nB;
      if (i == 2) { nN = 0.f; nJ = xE + tEL; nC = xE + tEM; }
      else { nN = xN[2] + tNL; nJ = LS(xJ[2] + tJL, xE + tEL); nC = LS(xC[2] + tCL, xE + tEM); }
      nB = LS(nN + tNM, nJ + tJM);
      if (xo && lane == 0) { xo[i * 5 + 0] = xE; xo[i * 5 + 1] = nN; xo[i * 5 + 2] = nJ; xo[i * 5 + 3] = nB; xo[i * 5 + 4] = nC; }
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
      xB[2] = xB[1]; xB[1] = xB[0]; xB[0] = nB;
      cL2 = cL1; cL1 = cL; cL = nC;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
        Dr[2][c] = Dr[1][c]; Dr[1][c] = Dr[0][c]; Dr[0][c] = Dc[c];
        iv2[c] = iv1[c]; iv1[c] = ivc[c];
      }
    }
    if (lane == 0) sc[job] = LS(cL, LS(cL1 + tCL, cL2 + tCL)) + tCM;
  }
#undef LS
}

// ---------------------------------------------------------------------------------------------
// 5-codon Forward, full matrix: fwd[(i*(M+1)+k)*8 + {D,I,C0..C5}], xmx[i*5 + {E,N,J,B,C}].
// IVX(i,k) collects the paths leaving row i-1; codon length c reads IVX(i-c+1).
// c5_compat selects the ring slot the generic reference reads for 5-nt codons.
// ---------------------------------------------------------------------------------------------
template <int C, int MODE, bool UNIHIT = false>
__global__ __launch_bounds__(kFsBlock) void fs5_fwd_kernel(SeqView dna, FsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                      float tEL, float tEM, int c5_compat, float *__restrict__ sc,
                                                      float *__restrict__ fwd, const int64_t *__restrict__ fwd_off, float *__restrict__ xmx, const int64_t *__restrict__ xmx_off,
                                                      int cfg_len /* >= 0: the amino length the model is configured for, instead of L/3 */, FsJobs jobs,
                                                      int *__restrict__ done = nullptr /* host-visible: done[job] = 1 once the job's matrix and score have landed */) {
  constexpr bool EXACT = (MODE == 1);   // 0: table + scans, 1: exact log-sums (strict mode runs the chain kernels, bath_fs_chain.hip)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_tbl = reinterpret_cast<float *>(lds);
  float *s_tf = s_tbl + kLogsumTbl;
  fs_load_logsum_table(s_tbl, p.logsum);
  for (int i = threadIdx.x; i < (p.M + 2) * 8; i += blockDim.x) s_tf[i] = p.tf[i];
  __syncthreads();
  const int M = p.M;
  const int lane = threadIdx.x & 63;
#define LS(a, b) flogsum<EXACT>((a), (b), s_tbl)
  for (int64_t job = fs_next_job(jobs, dna.n, lane); job >= 0; job = fs_next_job(jobs, dna.n, lane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *fo = fwd + fwd_off[job];
    float *xo = xmx + xmx_off[job];
    if (L < 5) {
      if (lane == 0) sc[job] = -INFINITY;
      if (done) { __threadfence_system(); if (lane == 0) __hip_atomic_store(done + job, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
      continue;
    }
    const int Lc = cfg_len >= 0 ? cfg_len : L / 3;
    const float tNL = loop_tab[Lc], tNM = move_tab[Lc], tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    float Mr[3][C], Ir[3][C], Dr1[C], iv[4][C];       // M,I of rows i-1..i-3 (C0 totals); D of row i-1; IVX(i-1..i-4)
#pragma unroll
    for (int c = 0; c < C; c++) {
      Mr[0][c] = Mr[1][c] = Mr[2][c] = Ir[0][c] = Ir[1][c] = Ir[2][c] = Dr1[c] = -INFINITY;
      iv[0][c] = iv[1][c] = iv[2][c] = iv[3][c] = -INFINITY;
    }
    // row 0
    for (int k = lane; k <= M; k += 64)
#pragma unroll
      for (int s = 0; s < 8; s++) fo[(size_t)k * 8 + s] = -INFINITY;
    if (lane == 0) { xo[0] = -INFINITY; xo[1] = 0.f; xo[2] = -INFINITY; xo[3] = tNM; xo[4] = -INFINITY; }
    float xN[3] = {0.f, 0.f, 0.f}, xJ[3] = {-INFINITY, -INFINITY, -INFINITY}, xC[3] = {-INFINITY, -INFINITY, -INFINITY};
    float xBprev = tNM;
    int t = 1367, u = 1367, v = 1367, w = 1367, x = 1367;
    float cL = -INFINITY, cL1 = -INFINITY, cL2 = -INFINITY;

    for (int i = 1; i <= L; i++) {
      t = u; u = v; v = w; w = x; x = (d[i - 1] < 4) ? d[i - 1] : 1367;
      const float *r1 = p.rsc + (size_t)imin(x * 341, 1366) * p.pitch;
      const float *r2 = p.rsc + (size_t)imin(x * 341 + w * 85 + 1, 1365) * p.pitch;
      const float *r3 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + 2, 1364) * p.pitch;
      const float *r4 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + u * 5 + 3, 1365) * p.pitch;
      const float *r5 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + u * 5 + t + 4, 1366) * p.pitch;
      const float mIn = wave_shr1(Mr[0][C - 1], -INFINITY), iIn = wave_shr1(Ir[0][C - 1], -INFINITY), dIn = wave_shr1(Dr1[C - 1], -INFINITY);
      float Mc[C], Ic[C], ivc[C], md[C], dd[C];
      float *row = fo + (size_t)i * (M + 1) * 8;
      if (lane == 0) {
#pragma unroll
        for (int s = 0; s < 8; s++) row[s] = -INFINITY;
      }
      // straight-line per node (see fs3_fwd_kernel): nodes beyond M read transition row M+1 (-inf) and emission column M
      // (finite, but added to a -inf IVX), so their values come out -inf; only the stores are guarded
      float cc[C][5];
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1, nd = imin(node, M + 1), ne = imin(node, M);
        const float4 ta = *reinterpret_cast<const float4 *>(s_tf + nd * 8);
        const float4 tb = *reinterpret_cast<const float4 *>(s_tf + nd * 8 + 4);
        const float m1 = (c == 0) ? mIn : Mr[0][c - 1], i1 = (c == 0) ? iIn : Ir[0][c - 1], d1 = (c == 0) ? dIn : Dr1[c - 1];
        float ivn;
        if (i <= 2) ivn = xBprev + ta.w;                                          // rows 1,2: only B(i-1) enters (:109,:150)
        else ivn = LS(m1 + ta.x, LS(i1 + ta.y, LS(d1 + ta.z, xBprev + ta.w)));
        ivc[c] = ivn;
        const float c1 = ivn + r1[ne];
        const float c2 = (i >= 2) ? iv[0][c] + r2[ne] : -INFINITY;
        const float c3 = (i >= 3) ? iv[1][c] + r3[ne] : -INFINITY;
        const float c4 = (i >= 4) ? iv[2][c] + r4[ne] : -INFINITY;
        const float c5 = (i >= 5) ? (c5_compat ? ivn : iv[3][c]) + r5[ne] : -INFINITY;
        float c0;
        if (i == 1) c0 = c1;
        else if (i == 2) c0 = LS(c1, c2);
        else if (i < 5) c0 = LS(c1, LS(c2, LS(c3, c4)));
        else c0 = LS(LS(c1, LS(c2, c3)), LS(c4, c5));
        Mc[c] = c0;
        const float ins = LS(Mr[2][c] + tb.z, Ir[2][c] + tb.w);
        Ic[c] = (i >= 3 && node < M) ? ins : -INFINITY;
        md[c] = c0 + tb.x; dd[c] = tb.y;
        cc[c][0] = c1; cc[c][1] = c2; cc[c][2] = c3; cc[c][3] = c4; cc[c][4] = c5;
      }
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node <= M) {
          float *cell = row + (size_t)node * 8;
          cell[1] = Ic[c]; cell[2] = Mc[c]; cell[3] = cc[c][0]; cell[4] = cc[c][1]; cell[5] = cc[c][2]; cell[6] = cc[c][3]; cell[7] = cc[c][4];
        }
      }
      float Dc[C];
      d_chain_fwd<C, EXACT>(md, dd, Dc, s_tbl);
      float eloc = -INFINITY;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        Dc[c] = (node <= M) ? Dc[c] : -INFINITY;
        eloc = LS(Mc[c], LS(Dc[c], eloc));
      }
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1;
        if (node <= M) row[(size_t)node * 8] = Dc[c];
      }
      const float xE = wave_logsum<EXACT>(eloc, s_tbl);
      float nN, nJ, nC, nB;
      if (i <= 2) { nN = 0.f; nJ = xE + tEL; nC = xE + tEM; nB = tNM; }           // :126-132, :166-167
      else {
        nN = xN[2] + tNL; nJ = LS(xJ[2] + tJL, xE + tEL); nC = LS(xC[2] + tCL, xE + tEM);
        nB = LS(nN + tNM, nJ + tJM);
      }
      if constexpr (UNIHIT) {
        // unihit (tEL = -inf): J is unreachable, J(i) = -inf and B(i) = N(i) + tNM -- the values above, said without reading E(i).
        // The row's E reduction (C log-sums per lane + 6 across the wave) then feeds C(i) only and leaves the chain that the
        // next row waits for.
        nJ = -INFINITY; nB = nN + tNM;
      }
      if (lane == 0) { xo[i * 5 + 0] = xE; xo[i * 5 + 1] = nN; xo[i * 5 + 2] = nJ; xo[i * 5 + 3] = nB; xo[i * 5 + 4] = nC; }
      xN[2] = xN[1]; xN[1] = xN[0]; xN[0] = nN;
      xJ[2] = xJ[1]; xJ[1] = xJ[0]; xJ[0] = nJ;
      xC[2] = xC[1]; xC[1] = xC[0]; xC[0] = nC;
      xBprev = nB;
      cL2 = cL1; cL1 = cL; cL = nC;
#pragma unroll
      for (int c = 0; c < C; c++) {
        Mr[2][c] = Mr[1][c]; Mr[1][c] = Mr[0][c]; Mr[0][c] = Mc[c];
        Ir[2][c] = Ir[1][c]; Ir[1][c] = Ir[0][c]; Ir[0][c] = Ic[c];
        Dr1[c] = Dc[c];
        iv[3][c] = iv[2][c]; iv[2][c] = iv[1][c]; iv[1][c] = iv[0][c]; iv[0][c] = ivc[c];
      }
    }
    if (lane == 0) sc[job] = LS(cL, LS(cL1 + tCL, cL2 + tCL)) + tCM;
    if (done) {                                                  // every lane's stores first (system scope), then the flag
      __threadfence_system();
      if (lane == 0) __hip_atomic_store(done + job, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
#undef LS
}

// ---------------------------------------------------------------------------------------------
// 3-codon Backward parser (the envelopes' 5-codon Backward is fs5_bwd_wf_kernel, bath_fs_wavefront.hip).
// tb[node] = {tMD(k), tMI(k), tMM(k), tDD(k), tDM(k), tII(k), tIM(k), tBM(k-1)}
// Row types follow the reference: rows without an emitted codon, "tail" rows with no i+3 row,
// accumulate-left-to-right rows (L-3, L-4) and the main recursion (generic_fwdback_frameshift.c:1054-1323, 1442-1677).
// ---------------------------------------------------------------------------------------------
template <int C, int MODE>
__global__ __launch_bounds__(kFsBlock, fs_min_waves(C)) void fs_bwd_kernel(SeqView dna, FsDev p, const float *__restrict__ loop_tab, const float *__restrict__ move_tab,
                                                     float tEL, float tEM, float *__restrict__ sc,
                                                     float *__restrict__ bck, const int64_t *__restrict__ bck_off, float *__restrict__ xmx, const int64_t *__restrict__ xmx_off, FsJobs jobs) {
  constexpr bool EXACT = (MODE == 1);   // 0: table + scans, 1: exact log-sums (strict mode runs the chain kernels, bath_fs_chain.hip)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_tbl = reinterpret_cast<float *>(lds);
  float *s_tb = s_tbl + kLogsumTbl;
  fs_load_logsum_table(s_tbl, p.logsum);
  for (int i = threadIdx.x; i < (p.M + 2) * 8; i += blockDim.x) s_tb[i] = p.tb[i];
  __syncthreads();
  constexpr int DEG = 338;
  constexpr int NR = 5;                             // rows i+1..i+5 of M kept in registers
  const int M = p.M;
  // Lanes own their nodes in DESCENDING order (logical lane = 63 - physical lane): Backward's chains run from node M down, and with
  // this order "the lane holding the next nodes" is the physical lane below, so the chains are the same upward DPP scans as Forward's
  const int plane = threadIdx.x & 63;
  const int lane = 63 - plane;
#define LS(a, b) flogsum<EXACT>((a), (b), s_tbl)
  for (int64_t job = fs_next_job(jobs, dna.n, plane); job >= 0; job = fs_next_job(jobs, dna.n, plane)) {
    const int L = dna.len[job];
    const uint8_t *d = dna.data + dna.off[job];
    float *bo = bck ? bck + bck_off[job] : nullptr;
    float *xo = xmx ? xmx + xmx_off[job] : nullptr;
    if (L < 5) { if (lane == 0) sc[job] = -INFINITY; continue; }
    const float tNL = loop_tab[L / 3], tNM = move_tab[L / 3], tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    float Mr[NR][C], Ir3[3][C];                     // M(i+1..i+5); I(i+1..i+3)
#pragma unroll
    for (int r = 0; r < NR; r++)
#pragma unroll
      for (int c = 0; c < C; c++) Mr[r][c] = -INFINITY;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < C; c++) Ir3[r][c] = -INFINITY;
    float xN3[3] = {-INFINITY, -INFINITY, -INFINITY}, xJ3[3] = {-INFINITY, -INFINITY, -INFINITY}, xC3[3] = {-INFINITY, -INFINITY, -INFINITY};
    float n0 = -INFINITY, n1 = -INFINITY, n2 = -INFINITY;           // N(0), N(1), N(2)
    const int first_emit = L - 2;
    int u = DEG, v = DEG, w = (d[L - 1] < 4) ? d[L - 1] : DEG, x = DEG;

    for (int i = L; i >= 0; i--) {
      float Mc[C], Ic[C], Dc[C];
      float xE, xNn, xJn, xCn, xBn = -INFINITY;
      if (i > first_emit) {
        // rows before any codon can be emitted (:1054-1073, :1442-1465)
        xCn = (i == L) ? tCM : tCL + tCM;
        xJn = xNn = -INFINITY;
        xE = xCn + tEM;
        // D(i,k) = LS(E, D(i,k+1)+tDD(k)), M(i,k) = LS(E, D(i,k+1)+tMD(k)): reverse chain
        float A = -INFINITY, B = 0.f;                // lane function applied to D(i, last node of lane + 1)
        // node M's and node M+1's transition rows are -inf: node M falls out of the general formula (LS(E, -inf) = E) and
        // nodes beyond M are deselected, without a branch per node
#pragma unroll
        for (int c = C - 1; c >= 0; c--) {
          const int node = lane * C + c + 1;
          const float tdd = s_tb[imin(node, M + 1) * 8 + 3];
          const float An = LS(xE, A + tdd);
          A = (node <= M) ? An : A; B = (node <= M) ? B + tdd : B;
        }
        // lanes without a source see the identity map (A = -inf, B = 0)
#define BATH_BCHAIN_STEP(CTRL, MASK) { const float An = dpp_f<CTRL, MASK>(A, -INFINITY), Bn = dpp_f<CTRL, MASK>(B, 0.f); A = LS(A, An + B); B = B + Bn; }
        BATH_BCHAIN_STEP(0x111, 0xf) BATH_BCHAIN_STEP(0x112, 0xf) BATH_BCHAIN_STEP(0x114, 0xf) BATH_BCHAIN_STEP(0x118, 0xf)
        BATH_BCHAIN_STEP(0x142, 0xa) BATH_BCHAIN_STEP(0x143, 0xc)
#undef BATH_BCHAIN_STEP
        const float dnext = wave_shr1(A, -INFINITY);
#pragma unroll
        for (int c = C - 1; c >= 0; c--) {
          const int node = lane * C + c + 1, nd = imin(node, M + 1);
          const float dn = (c == C - 1) ? dnext : Dc[c + 1];
          const float mv = LS(xE, dn + s_tb[nd * 8 + 0]), dv = LS(xE, dn + s_tb[nd * 8 + 3]);
          Mc[c] = (node <= M) ? mv : -INFINITY; Dc[c] = (node <= M) ? dv : -INFINITY;
          Ic[c] = -INFINITY;
        }
      } else {
        if (i < first_emit) { u = v; v = w; w = x; }
        x = (d[i] < 4) ? d[i] : DEG;                // x_{i+1}
        const int avail = L - i;
        const bool mainrow = (i <= L - 5);
        const bool tail = (avail < 3);
        const float *r2 = nullptr, *r3 = nullptr, *r4 = nullptr;
        if (avail >= 2) r2 = p.rsc + (size_t)imin(w * 84 + x * 21, 337) * p.pitch;
        if (avail >= 3) r3 = p.rsc + (size_t)imin(v * 84 + w * 21 + x * 5 + 1, 336) * p.pitch;
        if (avail >= 4) r4 = p.rsc + (size_t)imin(u * 84 + v * 21 + w * 5 + x + 2, 337) * p.pitch;
        // ivx[k] = logsum_c M(i+c,k)+e_c(k);  B(i) = logsum_k ivx[k]+tBM(k-1)
        float ivx[C];
        float bloc = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; c++) {
          // nodes beyond M: their M rows are -inf, so ivx comes out -inf and the B term (transition row M+1 = -inf) drops out
          const int node = lane * C + c + 1, ne = imin(node, M), nd = imin(node, M + 1);
          float a;
          if (mainrow) a = LS(Mr[1][c] + r2[ne], LS(Mr[2][c] + r3[ne], Mr[3][c] + r4[ne]));
          else {
            a = Mr[1][c] + r2[ne];
            if (avail >= 3) a = LS(a, Mr[2][c] + r3[ne]);
            if (avail >= 4) a = LS(a, Mr[3][c] + r4[ne]);
          }
          ivx[c] = a;
          bloc = LS(bloc, a + s_tb[nd * 8 + 7]);
        }
        xBn = wave_logsum<EXACT>(bloc, s_tbl);
        if (i == 0) {
          n0 = LS(xN3[2] + tNL, xBn + tNM);
          if (xo && lane == 0) { xo[0] = -INFINITY; xo[1] = n0; xo[2] = -INFINITY; xo[3] = xBn; xo[4] = -INFINITY; }
          if (bo) for (int k = lane; k <= M; k += 64) { bo[(size_t)k * 3] = bo[(size_t)k * 3 + 1] = bo[(size_t)k * 3 + 2] = -INFINITY; }
          break;
        }
        if (tail) { xJn = xBn + tJM; xNn = xBn + tNM; xCn = tCL + tCM; }
        else { xJn = LS(xJ3[2] + tJL, xBn + tJM); xCn = xC3[2] + tCL; xNn = LS(xN3[2] + tNL, xBn + tNM); }
        xE = LS(xJn + tEL, xCn + tEM);
        // ivx at node+1 for every node of the lane
        const float ivNext = wave_shr1(ivx[0], -INFINITY);
        // D chain (descending): D(k) = LS(LS(E, D(k+1)+tDD(k)), ivx(k+1)+tDM(k)); a(k) := LS(E, ivx(k+1)+tDM(k)) up to association
        float A = -INFINITY, B = 0.f;
        float base[C];
        // node M needs no special case: its transitions out are -inf, so base = -inf and D(M) = M(M) = E fall out of the general
        // formulas (LS(x, -inf) = x); nodes beyond M are deselected
#pragma unroll
        for (int c = C - 1; c >= 0; c--) {
          const int node = lane * C + c + 1, nd = imin(node, M + 1);
          const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
          const float tdd = s_tb[nd * 8 + 3], tdm = s_tb[nd * 8 + 4];
          base[c] = ivn + tdm;
          const float An = (!mainrow && !tail) ? LS(A + tdd, LS(xE, base[c])) : LS(LS(xE, A + tdd), base[c]);
          A = (node <= M) ? An : A; B = (node <= M) ? B + tdd : B;
        }
        // lanes without a source see the identity map (A = -inf, B = 0)
#define BATH_BCHAIN_STEP(CTRL, MASK) { const float An = dpp_f<CTRL, MASK>(A, -INFINITY), Bn = dpp_f<CTRL, MASK>(B, 0.f); A = LS(A, An + B); B = B + Bn; }
        BATH_BCHAIN_STEP(0x111, 0xf) BATH_BCHAIN_STEP(0x112, 0xf) BATH_BCHAIN_STEP(0x114, 0xf) BATH_BCHAIN_STEP(0x118, 0xf)
        BATH_BCHAIN_STEP(0x142, 0xa) BATH_BCHAIN_STEP(0x143, 0xc)
#undef BATH_BCHAIN_STEP
        const float dnext = wave_shr1(A, -INFINITY);
#pragma unroll
        for (int c = C - 1; c >= 0; c--) {
          const int node = lane * C + c + 1, nd = imin(node, M + 1);
          const float dn = (c == C - 1) ? dnext : Dc[c + 1];
          const float ivn = (c == C - 1) ? ivNext : ivx[c + 1];
          const float4 t0 = *reinterpret_cast<const float4 *>(s_tb + nd * 8);          // tMD tMI tMM tDD
          const float tii = s_tb[nd * 8 + 5], tim = s_tb[nd * 8 + 6];
          const float tmd = t0.x, tmi = t0.y, tmm = t0.z, tdd = t0.w;
          float mv, dv, iv_;
          if (tail) {
            mv = LS(dn + tmd, LS(ivn + tmm, xE));
            dv = LS(LS(xE, dn + tdd), base[c]);
            iv_ = ivn + tim;
          } else if (!mainrow) {
            mv = LS(dn + tmd, LS(Ir3[2][c] + tmi, LS(ivn + tmm, xE)));
            dv = LS(dn + tdd, LS(xE, base[c]));
            iv_ = LS(Ir3[2][c] + tii, ivn + tim);
          } else {
            mv = LS(LS(dn + tmd, LS(Ir3[2][c] + tmi, ivn + tmm)), xE);
            dv = LS(LS(xE, dn + tdd), base[c]);
            iv_ = LS(Ir3[2][c] + tii, ivn + tim);
          }
          // node M: -inf transitions make mv = dv = E and iv_ = -inf by themselves; nodes beyond M hold -inf
          Mc[c] = (node <= M) ? mv : -INFINITY; Dc[c] = (node <= M) ? dv : -INFINITY; Ic[c] = (node <= M) ? iv_ : -INFINITY;
        }
      }
      // store row i
      if (bo) {
        float *row = bo + (size_t)i * (M + 1) * 3;
        if (lane == 0) row[0] = row[1] = row[2] = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int node = lane * C + c + 1;
          if (node <= M) { row[(size_t)node * 3 + 0] = Dc[c]; row[(size_t)node * 3 + 1] = Ic[c]; row[(size_t)node * 3 + 2] = Mc[c]; }
        }
      }
      if (xo && lane == 0) { xo[i * 5 + 0] = xE; xo[i * 5 + 1] = xNn; xo[i * 5 + 2] = xJn; xo[i * 5 + 3] = xBn; xo[i * 5 + 4] = xCn; }
      if (i == 2) n2 = xNn;
      if (i == 1) n1 = xNn;
      xN3[2] = xN3[1]; xN3[1] = xN3[0]; xN3[0] = xNn;
      xJ3[2] = xJ3[1]; xJ3[1] = xJ3[0]; xJ3[0] = xJn;
      xC3[2] = xC3[1]; xC3[1] = xC3[0]; xC3[0] = xCn;
#pragma unroll
      for (int c = 0; c < C; c++) {
#pragma unroll
        for (int r = NR - 1; r > 0; r--) Mr[r][c] = Mr[r - 1][c];
        Mr[0][c] = Mc[c];
        Ir3[2][c] = Ir3[1][c]; Ir3[1][c] = Ir3[0][c]; Ir3[0][c] = Ic[c];
      }
    }
    if (lane == 0) sc[job] = LS(n0, LS(n1, n2));
  }
#undef LS
}

}  // namespace bath

// =================================================================================================
// host side
// =================================================================================================

int bath_hip_fsprofile::ensure_len(int maxL_amino) const {
  std::lock_guard<std::mutex> lock(grow_mu);
  if (maxL_amino <= maxL) return BATH_OK;
  const int n = std::max(maxL_amino, 4096) + 1;
  for (int h = 0; h < 2; h++) {
    const float nj = (h == 0) ? 1.0f : 0.0f;                       // 0: multihit (parsers), 1: unihit (envelopes)
    std::vector<float> lo(n), mv(n);
    for (int L = 0; L < n; L++) {
      const float pmove = (2.0f + nj) / ((float)L + 2.0f + nj);    // p7_fs_ReconfigLength, modelconfig.c:767-770
      const float ploop = 1.0f - pmove;
      lo[L] = (float)std::log((double)ploop); mv[L] = (float)std::log((double)pmove);
    }
    float *nl = nullptr, *nm = nullptr;                            // complete before they are published; the old tables are freed with the profile
    BATH_HIP_TRY(ctx, hipMalloc((void **)&nl, n * sizeof(float)));
    BATH_HIP_TRY(ctx, hipMalloc((void **)&nm, n * sizeof(float)));
    BATH_HIP_TRY(ctx, hipMemcpy(nl, lo.data(), n * sizeof(float), hipMemcpyHostToDevice));
    BATH_HIP_TRY(ctx, hipMemcpy(nm, mv.data(), n * sizeof(float), hipMemcpyHostToDevice));
    if (d_loop[h]) retired.push_back(d_loop[h]);
    if (d_move[h]) retired.push_back(d_move[h]);
    d_loop[h] = nl; d_move[h] = nm;
  }
  maxL = n - 1;
  return BATH_OK;
}

extern "C" void bath_hip_fsprofile_destroy(bath_hip_fsprofile *om) {
  if (!om) return;
  for (void *p : {(void *)om->d_codons, (void *)om->d_indel, (void *)om->d_rsc, (void *)om->d_tf, (void *)om->d_tb, (void *)om->d_logsum, (void *)om->d_tsc, (void *)om->d_loop[0], (void *)om->d_loop[1],
                  (void *)om->d_move[0], (void *)om->d_move[1], (void *)om->d_odds_rsc, (void *)om->d_odds_tf, (void *)om->d_odds_tb})
    if (p) (void)hipFree(p);
  for (void *p : om->retired) (void)hipFree(p);
  delete om;
}

extern "C" int bath_hip_fsprofile_convert(bath_hip_ctx *ctx, const bath_fs_profile *gm, bath_hip_fsprofile **ret) {
  *ret = nullptr;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int M = gm->M;
  bath_hip_fsprofile *om = new bath_hip_fsprofile();
  om->ctx = ctx; om->M = M; om->codon_lengths = gm->codon_lengths; om->maxcodons = gm->maxcodons; om->max_length = gm->max_length;
  om->fsprob = gm->fsprob;
  std::memcpy(om->evparam, gm->evparam, sizeof om->evparam);
  om->h_tsc.assign(gm->tsc, gm->tsc + (size_t)M * 8);
  if (gm->codons) {
    om->h_codons.assign(gm->codons, gm->codons + (size_t)(M + 1) * gm->maxcodons);
    BATH_HIP_TRY(ctx, hipMalloc((void **)&om->d_codons, om->h_codons.size() + 64));
    BATH_HIP_TRY(ctx, hipMemcpy(om->d_codons, om->h_codons.data(), om->h_codons.size(), hipMemcpyHostToDevice));
    if (gm->indel_pos) {
      BATH_HIP_TRY(ctx, hipMalloc((void **)&om->d_indel, om->h_codons.size() + 64));
      BATH_HIP_TRY(ctx, hipMemcpy(om->d_indel, gm->indel_pos, om->h_codons.size(), hipMemcpyHostToDevice));
    }
  }
  om->pitch = (M + 1 + 3) / 4 * 4;
  const int nrows = gm->maxcodons + kKp;
  std::vector<float> rsc((size_t)nrows * om->pitch, -INFINITY);
  for (int r = 0; r < nrows; r++) std::memcpy(&rsc[(size_t)r * om->pitch], gm->rsc + (size_t)r * (M + 1), sizeof(float) * (M + 1));
  enum { MM, IM, DM, BM, MD, DD, MI, II };
  auto tsc = [&](int k, int s) -> float { return (k >= 0 && k < M) ? gm->tsc[(size_t)k * 8 + s] : -INFINITY; };
  std::vector<float> tf((size_t)(M + 2) * 8, -INFINITY), tb((size_t)(M + 2) * 8, -INFINITY);
  for (int k = 1; k <= M; k++) {
    float *f = &tf[(size_t)k * 8];
    f[0] = tsc(k - 1, MM); f[1] = tsc(k - 1, IM); f[2] = tsc(k - 1, DM); f[3] = tsc(k - 1, BM);
    f[4] = tsc(k, MD); f[5] = tsc(k, DD); f[6] = tsc(k, MI); f[7] = tsc(k, II);
    float *b = &tb[(size_t)k * 8];
    b[0] = tsc(k, MD); b[1] = tsc(k, MI); b[2] = tsc(k, MM); b[3] = tsc(k, DD); b[4] = tsc(k, DM); b[5] = tsc(k, II); b[6] = tsc(k, IM);
    b[7] = tsc(k - 1, BM);
  }
  std::vector<float> tbl(kLogsumTbl);
  for (int i = 0; i < kLogsumTbl; i++) tbl[i] = (float)std::log(1. + std::exp((double)-i / 1000.f));     // p7_FLogsumInit, logsum.c:89
  auto up = [&](float **dst, const std::vector<float> &src) -> hipError_t {
    hipError_t e = hipMalloc((void **)dst, src.size() * sizeof(float) + 64);
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice);
  };
  BATH_HIP_TRY(ctx, up(&om->d_rsc, rsc));
  BATH_HIP_TRY(ctx, up(&om->d_tf, tf));
  BATH_HIP_TRY(ctx, up(&om->d_tb, tb));
  BATH_HIP_TRY(ctx, up(&om->d_logsum, tbl));
  BATH_HIP_TRY(ctx, up(&om->d_tsc, om->h_tsc));
  int st = om->ensure_len(4096);
  if (st != BATH_OK) { bath_hip_fsprofile_destroy(om); return st; }
  *ret = om;
  return BATH_OK;
}

namespace bath {

// logsum_mode -> kernel MODE: 0 table + wavefront scans, 1 exact log-sums (BATH_LOGSUM_TABLE_SERIAL, "strict", runs the chain
// kernels of bath_fs_chain.hip instead)
#define BATH_FS_MODE(modev, BODY)                         \
  switch (modev) {                                        \
    case 1: { constexpr int MD = 1; BODY } break;         \
    default: { constexpr int MD = 0; BODY } break;        \
  }

// what BATH_LOGSUM_CONTEXT means for the 3-codon parsers: odds ratios when bath_hip_set_fs_odds switched them on, else strict / fast
static int fs3_ctx_mode(const bath_hip_ctx *ctx) {
  return ctx->fs_odds ? BATH_LOGSUM_ODDS : (ctx->fs_strict ? BATH_LOGSUM_TABLE_SERIAL : BATH_LOGSUM_TABLE);
}

static FsDev fsdev(const bath_hip_fsprofile *om) { return FsDev{om->M, om->pitch, om->maxcodons, om->d_rsc, om->d_tf, om->d_tb, om->d_logsum}; }

static int fs_grid_dp(bath_hip_ctx *ctx, int64_t n) {           // blocks of kFsBlock threads, two per CU
  const int wpb = kFsBlock / 64;
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + wpb - 1) / wpb, (int64_t)ctx->prop.multiProcessorCount * 2));
}

// xmx rows live in a device buffer laid out like the host array the caller passes (offsets in floats)
static int upload_offsets(bath_hip_ctx *ctx, DevBuf &buf, const int64_t *off, int64_t n) {
  BATH_HIP_TRY(ctx, buf.reserve((size_t)(n + 1) * sizeof(int64_t)));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(buf.p, off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  return BATH_OK;
}

// the windows of <dna> by decreasing length and <k> zeroed job counters (one per kernel launch that will draw from the list),
// queued on ctx->stream; jobs[i] is what launch i passes to its kernel
int fs_schedule(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int k, FsJobs *jobs) {
  const int64_t n = dna->n;
  std::vector<int32_t> order;
  fs_order_by_length_desc(dna->h_len.data(), n, &order);
  if (k > 64) { ctx->set_error("fs_schedule: more than 64 job counters"); return BATH_EINVAL; }
  DevBuf &b = ctx->scratch[Scratch::kFsJobList];
  BATH_HIP_TRY(ctx, b.reserve(256 + (size_t)n * sizeof(int32_t) + 64));
  BATH_HIP_TRY(ctx, hipMemsetAsync(b.p, 0, 256, ctx->stream));
  if (ctx->stage_upload(Pinned::kFsJobOrder, b.as<char>() + 256, order.data(), (size_t)n, ctx->stream) != BATH_OK) return BATH_EFAIL;   // through page-locked staging: no synchronize
  for (int i = 0; i < k; i++) jobs[i] = FsJobs{reinterpret_cast<const int32_t *>(b.as<char>() + 256), b.as<unsigned>() + i};
  return BATH_OK;
}

// One 3-codon parser over the windows of <dna>, on <stream> and inside a span (<cells>, <bytes>) of its own: the odds-ratio, the strict
// chain or the table-scan kernel, by <mode>.  <cu_share>: the strict launch is sized for 1 / cu_share of the chip (the other parser's beside it)
static int fs3_launch_parser(bath_hip_ctx *ctx, hipStream_t stream, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int mode, bool backward,
                             float *d_sc, float *d_rows, const int64_t *d_off, FsJobs jobs, int cu_share, double cells, double bytes) {
  int st = BATH_OK;
  const int Cv = BATH_TILING_PICK(BATH_FS_COLUMNS, om->M);
  const float tE = (float)-0.69314718055994529;
  const bool odds = mode == BATH_LOGSUM_ODDS;
  const int sp = ctx->span_begin(odds ? (backward ? "fs3_bwd_odds_kernel" : "fs3_fwd_odds_kernel") : (backward ? "fs_bwd_kernel<3>" : "fs3_fwd_kernel"), stream, cells, bytes);
  if (odds) st = launch_fs3_odds(ctx, stream, om, dna, backward, d_sc, d_rows, d_off, jobs);
  else if (mode == BATH_LOGSUM_TABLE_SERIAL) st = (backward ? launch_fs3_bwd_chain : launch_fs3_fwd_chain)(ctx, stream, om, dna, Cv, tE, tE, d_sc, d_rows, d_off, jobs, cu_share);
  else {
    const size_t shmem = (size_t)(kLogsumTbl + (om->M + 2) * 8) * sizeof(float);
    const int grid_dp = fs_grid_dp(ctx, dna->n);
    BATH_FS_SWITCH(Cv, BATH_FS_MODE(mode, {
      if (!backward) {
        if ((st = fs_set_shmem(ctx, fs3_fwd_kernel<CC, MD>, shmem)) != BATH_OK) return st;
        hipLaunchKernelGGL((fs3_fwd_kernel<CC, MD>), dim3(grid_dp), dim3(kFsBlock), shmem, stream, dna->view(), fsdev(om), om->d_loop[0], om->d_move[0], tE, tE, d_sc, d_rows, d_off, jobs);
      } else {
        if ((st = fs_set_shmem(ctx, fs_bwd_kernel<CC, MD>, shmem)) != BATH_OK) return st;
        hipLaunchKernelGGL((fs_bwd_kernel<CC, MD>), dim3(grid_dp), dim3(kFsBlock), shmem, stream, dna->view(), fsdev(om), om->d_loop[0], om->d_move[0], tE, tE, d_sc, (float *)nullptr, (const int64_t *)nullptr, d_rows, d_off, jobs);
      }
    }))
  }
  if (st == BATH_OK) ctx->span_end(sp, stream);
  return st;
}

// The regions' multihit 5-codon Forward on ctx->stream, inside its span: the odds-ratio kernel while bath_hip_set_fs5_odds is on
// (before fs_strict), else the strict chain kernel or the table-scan kernel
static int fs5_launch_region_forward(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, float *d_sc, float *d_f, const int64_t *d_foff,
                                     float *d_fx, const int64_t *d_xoff, int cfg_len_amino, FsJobs jobs, int *d_done, double cells) {
  int st = BATH_OK;
  const int Cv = BATH_TILING_PICK(BATH_FS_COLUMNS, om->M);
  const float tE = (float)-0.69314718055994529;                               // multihit: E->C and E->J both log 1/2 (modelconfig.c:825-831)
  const int mode = ctx->fs_strict ? BATH_LOGSUM_TABLE_SERIAL : BATH_LOGSUM_TABLE;
  const int s1 = ctx->span_begin(ctx->fs5_odds ? "fs5_fwd_odds_kernel(regions)" : "fs5_fwd_kernel(regions)", ctx->stream, cells, cells * 32.0);
  if (ctx->fs5_odds) st = launch_fs5_odds(ctx, ctx->stream, om, dna, kFs5OddsRegionFwd, d_sc, d_f, d_foff, d_fx, d_xoff, cfg_len_amino, jobs, d_done);
  else if (mode == BATH_LOGSUM_TABLE_SERIAL) st = launch_fs5_fwd_chain(ctx, ctx->stream, om, dna, Cv, tE, tE, 0, d_sc, d_f, d_foff, d_fx, d_xoff, cfg_len_amino, jobs, d_done);
  else {
    const size_t shmem = (size_t)(kLogsumTbl + (om->M + 2) * 8) * sizeof(float);
    BATH_FS_SWITCH(Cv, BATH_FS_MODE(mode, {
      if ((st = fs_set_shmem(ctx, fs5_fwd_kernel<CC, MD>, shmem)) != BATH_OK) return st;
      hipLaunchKernelGGL((fs5_fwd_kernel<CC, MD>), dim3(fs_grid_dp(ctx, dna->n)), dim3(kFsBlock), shmem, ctx->stream, dna->view(), fsdev(om), om->d_loop[0], om->d_move[0], tE, tE, 0, d_sc,
                         d_f, d_foff, d_fx, d_xoff, cfg_len_amino, jobs, d_done);
    }))
  }
  if (st == BATH_OK) ctx->span_end(s1, ctx->stream);
  return st;
}

}  // namespace bath

static int fs3_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int logsum_mode, float *sc, float *xmx,
                      const int64_t *xmx_off, bool backward, DevBuf *keep = nullptr /* the rows stay in this device buffer instead of going to <xmx> */) {
  if (!ctx || !om || !dna || om->codon_lengths != 3) { if (ctx) ctx->set_error("fs3 parser needs a 3-codon profile"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  if (logsum_mode == BATH_LOGSUM_CONTEXT) logsum_mode = fs3_ctx_mode(ctx);
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  int st = om->ensure_len(dna->maxlen / 3 + 1);
  if (st != BATH_OK) return st;
  DevBuf &b_sc = ctx->scratch[Scratch::kFs3FwdScores], &b_x = ctx->scratch[Scratch::kFs3FwdRows], &b_off = ctx->scratch[Scratch::kFs3RowOffsets];
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * sizeof(float)));
  float *d_x = nullptr;
  if (xmx || keep) {
    DevBuf &bx = keep ? *keep : b_x;
    BATH_HIP_TRY(ctx, bx.reserve((size_t)xmx_off[n] * sizeof(float) + 64));
    if ((st = upload_offsets(ctx, b_off, xmx_off, n)) != BATH_OK) return st;
    d_x = bx.as<float>();
  }
  FsJobs jq[1];
  if ((st = fs_schedule(ctx, dna, 1, jq)) != BATH_OK) return st;
  if ((st = fs3_launch_parser(ctx, ctx->stream, om, dna, logsum_mode, backward, b_sc.as<float>(), d_x, b_off.as<int64_t>(), jq[0], 1,
                              (double)dna->total * om->M, (double)dna->total * ((xmx || keep) ? 21.0 : 1.0))) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc, b_sc.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (xmx) BATH_HIP_TRY(ctx, hipMemcpyAsync(xmx, d_x, (size_t)xmx_off[n] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

// p7_DomainDecoding_Frameshift (generic form, generic_decoding_frameshift.c:204-290) and the region heuristics of
// p7_domaindef_ByPosteriorHeuristics_Frameshift_BATH (p7_domaindef.c:328-392, is_multidomain_region_frameshift :684-714)
// on the parsers' special-state rows, one WAVE per window: the posterior terms (11 expf per position) are elementwise and
// computed by all 64 lanes; the two running sums and the scan for regions are serial and short, lane 0 does them with the
// reference's own order of additions.  Only the regions (a few integers per window) travel to the host.
constexpr int kMaxRegions = 64;       // regions kept per DNA window; a window with more reports the true count and the call fails loudly (the reference has no cap)
__global__ __launch_bounds__(64) void fs_regions_kernel(int64_t n, const int32_t *__restrict__ len, const float *__restrict__ fx, const float *__restrict__ bx,
                                  const int64_t *__restrict__ x_off, const int64_t *__restrict__ fx_off /* where the Forward rows start (they may live in another buffer) */,
                                  const float *__restrict__ tbl, float loop, float *__restrict__ work /* 3 floats per xmx row */,
                                  int32_t *__restrict__ regions /* [n][1 + 3*kMaxRegions]: count, then {i, j, multidomain} */) {
  const int64_t w = blockIdx.x;
  const int lane = threadIdx.x;
  if (w >= n) return;
  enum { XE = 0, XN, XJ, XB, XC };
  const int L = len[w];
  const float *F = fx + fx_off[w], *B = bx + x_off[w];
  float *btot = work + (x_off[w] / 5) * 3, *etot = btot + (L + 1), *mocc = etot + (L + 1);
  int32_t *out = regions + w * (1 + 3 * kMaxRegions);
  int nreg = 0;
  if (L < 6) { if (lane == 0) out[0] = 0; return; }
  const float Z = flogsum_g(B[0 * 5 + XN], flogsum_g(B[1 * 5 + XN], B[2 * 5 + XN], tbl), tbl);
  if (!(Z > -INFINITY)) { if (lane == 0) out[0] = -1; return; }               // Backward underflow: the window is skipped (p7_pipeline.c:1471)
  auto em = [&](int s, int a, int b) { return expf(F[(size_t)a * 5 + s] + B[(size_t)b * 5 + s] + loop - Z); };
  for (int i = lane; i <= L; i += 64) {
    if (i < 3) { btot[i] = etot[i] = mocc[i] = 0.f; continue; }
    btot[i] = expf(F[(size_t)(i - 3) * 5 + XB] + B[(size_t)(i - 3) * 5 + XB] - Z);      // the terms; summed below
    etot[i] = expf(F[(size_t)i * 5 + XE] + B[(size_t)i * 5 + XE] - Z);
    float p = 0.0f;
    if (i < L - 1) {
      p += em(XN, i - 3, i); p += em(XN, i - 2, i + 1); p += em(XN, i - 1, i + 2);
      p += em(XC, i - 3, i); p += em(XC, i - 2, i + 1); p += em(XC, i - 1, i + 2);
      p += em(XJ, i - 3, i); p += em(XJ, i - 2, i + 1); p += em(XJ, i - 1, i + 2);
    } else if (i == L - 1) {
      p += em(XN, L - 4, L - 1); p += em(XN, L - 3, L); p += em(XC, L - 4, L - 1); p += em(XC, L - 3, L); p += em(XJ, L - 4, L - 1); p += em(XJ, L - 3, L);
    } else {
      p += em(XN, L - 3, L); p += em(XC, L - 3, L); p += em(XJ, L - 3, L);
    }
    mocc[i] = (float)(1. - p);
  }
  __syncthreads();
  if (lane != 0) return;
  out[0] = 0;
  for (int i = 3; i <= L; i++) { btot[i] = btot[i - 3] + btot[i]; etot[i] = etot[i - 3] + etot[i]; }
  const float rt1 = 0.25f, rt2 = 0.10f, rt3 = 0.20f;                         // p7_domaindef.c:80-82
  bool triggered = false;
  int d = 0;
  for (int j = 1; j < L; j++) {
    if (!triggered) { if (mocc[j] >= rt1) triggered = true; d = j; continue; }
    bool found = false;
    while (d > 1 && !found) {                                                // the start must show in all three frames
      int run = 0;
      d--;
      while (run < 3 && d > 3 && mocc[d] - (btot[d] - btot[d - 3]) < rt2) { d--; run++; }
      if (run == 3) found = true;
    }
    const int i = max(1, d - 3);
    d = j + 1;
    found = false;
    while (d < L && !found) {
      int run = 0;
      d++;
      while (run < 3 && d < L && mocc[d] - (etot[d] - etot[d - 3]) < rt2) { d++; run++; }
      if (run == 3) found = true;
    }
    j = min(L, d + 3);
    if (j - i + 1 >= 12) {
      float best = -1.0f;                                                    // is_multidomain_region_frameshift
      for (int ph = 0; ph < 3; ph++) {
        const int f = (j - i + 1 - ph) % 3;
        for (int z = i + 2 + ph; z <= j - f; z += 3) best = fmaxf(best, fminf(etot[z] - etot[i - 1 + ph], btot[j - f] - btot[z - 3]));
      }
      if (nreg < kMaxRegions) { out[1 + 3 * nreg] = i; out[2 + 3 * nreg] = j; out[3 + 3 * nreg] = best >= rt3 ? 1 : 0; }
      nreg++;
    }
    triggered = false;
  }
  out[0] = nreg;                        // may exceed kMaxRegions: the host checks
}

namespace bath {
// Both 3-codon parsers and the regions of every window of <dna>; regions_out[i] = {count (or -1: Backward underflow),
// then count x {i, j, multidomain}}, 1 + 3*fs_max_regions() ints per window.
int fs_max_regions() { return kMaxRegions; }
// Forward and Backward of a batch are independent and, with few windows, each is bound by the latency of its longest window's
// row chain: run Backward on the context's side stream while Forward runs on the main one.
int fs_fork(bath_hip_ctx *ctx) {
  if (!ctx->side_stream) {
    BATH_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
    BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  BATH_HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
  return BATH_OK;
}
int fs_join(bath_hip_ctx *ctx) {
  BATH_HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->side_stream));
  BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  return BATH_OK;
}

int fs3_regions(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, float loop, int32_t *regions_out, float *fwd_sc_out, const int32_t *kept) {
  if (!ctx || !om || !dna || om->codon_lengths != 3) { if (ctx) ctx->set_error("fs3 parser needs a 3-codon profile"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  int st = om->ensure_len(dna->maxlen / 3 + 1);
  if (st != BATH_OK) return st;
  const std::vector<int64_t> xoff = fs_row_offsets(dna, 5);
  DevBuf &b_sc = ctx->scratch[Scratch::kFs3FwdScores], &b_fx = ctx->scratch[Scratch::kFs3FwdRows], &b_off = ctx->scratch[Scratch::kFs3RowOffsets], &b_bx = ctx->scratch[Scratch::kFs3BwdRows], &b_work = ctx->scratch[Scratch::kFs3RegionWork], &b_reg = ctx->scratch[Scratch::kFs3RegionList];
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * sizeof(float)));
  BATH_HIP_TRY(ctx, b_fx.reserve((size_t)xoff[(size_t)n] * sizeof(float) + 64));
  BATH_HIP_TRY(ctx, b_bx.reserve((size_t)xoff[(size_t)n] * sizeof(float) + 64));
  BATH_HIP_TRY(ctx, b_work.reserve((size_t)xoff[(size_t)n] / 5 * 3 * sizeof(float) + 64));
  const size_t reg_ints = (size_t)n * (1 + 3 * kMaxRegions);
  BATH_HIP_TRY(ctx, b_reg.reserve(reg_ints * sizeof(int32_t) + 64));
  if ((st = upload_offsets(ctx, b_off, xoff.data(), n)) != BATH_OK) return st;
  // <kept>: window q of <dna> is window kept[q] of the block whose Forward rows fs3_forward_scores left on the device -- the
  // reference runs the Forward parser once per window too (p7_pipeline.c:1450, rows kept in pli->oxf)
  const bool reuse = kept && !ctx->fs_keep_xoff.empty() && fwd_sc_out == nullptr;
  DevBuf &b_foff = ctx->scratch[Scratch::kFsKeptFwdRowOffsets];
  const float *d_fx = b_fx.as<float>();
  const int64_t *d_fxoff = b_off.as<int64_t>();
  std::vector<int64_t> fsel;
  if (reuse) {
    fsel.resize((size_t)n);
    for (int64_t q = 0; q < n; q++) fsel[(size_t)q] = ctx->fs_keep_xoff[(size_t)kept[q]];
    BATH_HIP_TRY(ctx, b_foff.reserve((size_t)n * sizeof(int64_t)));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(b_foff.p, fsel.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    d_fx = ctx->scratch[Scratch::kFsKeptFwdRows].as<float>(); d_fxoff = b_foff.as<int64_t>();
  }
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 2 * sizeof(float)));
  FsJobs jq[2];
  if ((st = fs_schedule(ctx, dna, 2, jq)) != BATH_OK) return st;
  const int mode = fs3_ctx_mode(ctx);
  // strict mode: CUs each parser's launch is sized for when both run side by side -- half the chip each; Backward alone when the
  // Forward rows are reused
  constexpr int kParserCuShare = 2;
  if ((st = fs_fork(ctx)) != BATH_OK) return st;
  const double cells3 = (double)(xoff[(size_t)n] / 5) * om->M;                // rows x nodes; algorithmic HBM bytes: 1 B/nt in + 20 B/row out
  const double bytes3 = (double)(xoff[(size_t)n] / 5) * 21.0;
  if (!reuse && (st = fs3_launch_parser(ctx, ctx->stream, om, dna, mode, false, b_sc.as<float>(), b_fx.as<float>(), b_off.as<int64_t>(), jq[0], kParserCuShare, cells3, bytes3)) != BATH_OK) return st;
  if ((st = fs3_launch_parser(ctx, ctx->side_stream, om, dna, mode, true, b_sc.as<float>() + n, b_bx.as<float>(), b_off.as<int64_t>(), jq[1], reuse ? 1 : kParserCuShare, cells3, bytes3)) != BATH_OK) return st;
  if ((st = fs_join(ctx)) != BATH_OK) return st;
  const int s3 = ctx->span_begin("fs_regions_kernel", ctx->stream, (double)(xoff[(size_t)n] / 5), (double)(xoff[(size_t)n] / 5) * 52.0);
  hipLaunchKernelGGL(fs_regions_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, dna->d_len, d_fx, b_bx.as<float>(), b_off.as<int64_t>(), d_fxoff, om->d_logsum, loop,
                     b_work.as<float>(), b_reg.as<int32_t>());
  ctx->span_end(s3, ctx->stream);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipMemcpyAsync(regions_out, b_reg.p, reg_ints * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (fwd_sc_out) BATH_HIP_TRY(ctx, hipMemcpyAsync(fwd_sc_out, b_sc.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

// used by the pipeline's frameshift stage (bath_fs_stage.hip)
int fs3_forward_scores(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, float *sc) {
  ctx->fs_keep_xoff.clear();
  const int mode = fs3_ctx_mode(ctx);
  if (!ctx->fs_want_regions) return fs3_parser(ctx, om3, dna, mode, sc, nullptr, nullptr, false);
  // the domain stage follows: the special-state rows of every window stay on the device (20 B per nucleotide), so that the
  // windows that take the frameshift branch need the Backward parser only
  std::vector<int64_t> xoff = fs_row_offsets(dna, 5);
  const int st = fs3_parser(ctx, om3, dna, mode, sc, nullptr, xoff.data(), false, &ctx->scratch[Scratch::kFsKeptFwdRows]);
  if (st == BATH_OK) ctx->fs_keep_xoff = std::move(xoff);
  return st;
}
const float *fsprofile_evparam(const bath_hip_fsprofile *om) { return om->evparam; }
int fsprofile_codon_lengths(const bath_hip_fsprofile *om) { return om->codon_lengths; }
int fs_model_ok(bath_hip_ctx *ctx, const bath_hip_fsprofile *om) {
  if (om->M <= kFsMaxNodes) return BATH_OK;
  ctx->set_error("frameshift kernels support models up to " + std::to_string(kFsMaxNodes) + " nodes (this one has " + std::to_string(om->M) + ")");
  return BATH_EINVAL;
}
}  // namespace bath

extern "C" int bath_hip_fs3_forward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, int logsum_mode,
                                           float *sc, float *xmx, const int64_t *xmx_offsets) {
  return fs3_parser(ctx, om3, dna, logsum_mode, sc, xmx, xmx_offsets, false);
}
extern "C" int bath_hip_fs3_backward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, int logsum_mode,
                                            float *sc, float *xmx, const int64_t *xmx_offsets) {
  return fs3_parser(ctx, om3, dna, logsum_mode, sc, xmx, xmx_offsets, true);
}

namespace bath {
const FsHostTables fsprofile_host(const bath_hip_fsprofile *om) {
  return FsHostTables{om->M, om->max_length, om->maxcodons, om->h_tsc.data(), om->h_codons.empty() ? nullptr : om->h_codons.data(), om->evparam};
}
}  // namespace bath

extern "C" int bath_hip_fs5_forward_full(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino,
                                         float *sc, float *fwd, float *xmx) {
  if (!ctx || !om || !dna || !sc || om->codon_lengths != 5) { if (ctx) ctx->set_error("needs a 5-codon profile"); return BATH_EINVAL; }
  if (bath::fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (dna->n == 0) return BATH_OK;
  const float *h_f = nullptr, *h_x = nullptr;
  std::vector<int64_t> foff, xoff;
  std::vector<float> h_sc;
  const int st = bath::fs5_region_forward(ctx, om, dna, cfg_len_amino, &h_f, &foff, &h_x, &xoff, &h_sc, nullptr, nullptr);
  if (st != BATH_OK) return st;
  std::memcpy(sc, h_sc.data(), (size_t)dna->n * sizeof(float));
  if (fwd) std::memcpy(fwd, h_f, (size_t)foff[(size_t)dna->n] * sizeof(float));
  if (xmx) std::memcpy(xmx, h_x, (size_t)xoff[(size_t)dna->n] * sizeof(float));
  return BATH_OK;
}

// The score of bath_hip_fs5_forward_full and nothing else, strict (<odds> false) or in the reference's arithmetic
static int fs5_forward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino, float *sc, bool odds) {
  if (!ctx || !om || !dna || !sc || om->codon_lengths != 5) { if (ctx) ctx->set_error("needs a 5-codon profile"); return BATH_EINVAL; }
  if (cfg_len_amino < 0) { ctx->set_error(std::string(odds ? "fs5_forward_parser_odds" : "fs5_forward_parser") + ": the configuration length is negative"); return BATH_EINVAL; }
  if (bath::fs_model_ok(ctx, om) != BATH_OK) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n = dna->n;
  if (n == 0) return BATH_OK;
  int st = om->ensure_len(std::max(dna->maxlen / 3 + 1, cfg_len_amino));
  if (st != BATH_OK) return st;
  DevBuf &b_sc = ctx->scratch[Scratch::kEnvScores];
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 3 * sizeof(float)));
  bath::FsJobs jq[1];
  if ((st = bath::fs_schedule(ctx, dna, 1, jq)) != BATH_OK) return st;
  const float tE = (float)-0.69314718055994529;                               // multihit (modelconfig.c:825-831)
  const int sp = ctx->span_begin(odds ? "fs5_fwd_odds_parser_kernel" : "fs5_fwd_parser_kernel", ctx->stream, (double)dna->total * om->M, (double)dna->total);
  if (odds) st = bath::launch_fs5_odds_parser(ctx, ctx->stream, om, dna, b_sc.as<float>(), cfg_len_amino, jq[0]);
  else st = bath::launch_fs5_fwd_parser(ctx, ctx->stream, om, dna, BATH_TILING_PICK(BATH_FS_COLUMNS, om->M), tE, tE, b_sc.as<float>(), cfg_len_amino, jq[0]);
  if (st != BATH_OK) return st;
  ctx->span_end(sp, ctx->stream);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc, b_sc.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

// No matrix, no special-state rows leave the kernel (fs5_fwd_chain_kernel<C, 256, false>).
// Strict log-sums whatever bath_hip_set_fs_strict / bath_hip_set_fs5_odds say: its caller is calibration, whose numbers go into a file.
extern "C" int bath_hip_fs5_forward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino, float *sc) {
  return fs5_forward_parser(ctx, om, dna, cfg_len_amino, sc, false);
}

// bath_hip_fs5_forward_parser in the reference's arithmetic: the multihit score of fs5_fwd_odds_kernel and nothing else
// (fs5_fwd_odds_kernel<C, true, false>).  Odds ratios whatever the context's switches say; -inf for a window shorter than 5 nt and
// for an overflow (the reference's eslERANGE, which its calibration answers with a redraw: bath_calib_fit_scores).
extern "C" int bath_hip_fs5_forward_parser_odds(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino, float *sc) {
  return fs5_forward_parser(ctx, om, dna, cfg_len_amino, sc, true);
}

// p7_Forward_Frameshift of regions in the MULTIHIT configuration of a fixed amino length (p7_domaindef.c:411-414: the model's
// saved length), matrices and special-state rows copied to the host for the stochastic-trace ensemble (bath_ensemble.hip).
// fwd: (L+1) x (M+1) x {D, I, M_C0, M_C1..M_C5}; xmx: (L+1) x {E,N,J,B,C}.  sc[e] = -inf: no path (the region is dropped).
int bath::fs5_region_forward(bath_hip_ctx *ctx, const bath_hip_fsprofile *om, const bath_hip_seqs *dna, int cfg_len_amino,
                             const float **fwd, std::vector<int64_t> *fwd_off, const float **xmx, std::vector<int64_t> *xmx_off, std::vector<float> *sc,
                             const int **done_flags, const float **sc_live, FsRegionDev *dev) {
  // dev != nullptr (BATH_ENSEMBLE_STREAMS_DEVICE): the matrices, rows and scores stay in device memory for fs_ensemble_kernel, which
  // follows on ctx->stream -- no page-locked destination, no flags; returns right after the launch with *dev filled in.
  // done_flags != nullptr: return right after the launch.  *done_flags (page-locked, one int per region) turns 1 when that region's
  // matrix, rows and score (*sc_live) have landed in host memory; the caller synchronises the stream before it reuses the buffers.
  const int64_t n = dna->n;
  const int M = om->M;
  int st = om->ensure_len(std::max(dna->maxlen / 3 + 1, cfg_len_amino));
  if (st != BATH_OK) return st;
  std::vector<int64_t> &foff = *fwd_off, &xoff = *xmx_off;
  foff = fs_row_offsets(dna, (int64_t)(M + 1) * 8); xoff = fs_row_offsets(dna, 5);
  DevBuf &b_f = ctx->scratch[Scratch::kEnvFwdMatrix], &b_fx = ctx->scratch[Scratch::kEnvFwdRows], &b_off = ctx->scratch[Scratch::kEnvOffsets], &b_sc = ctx->scratch[Scratch::kEnvScores];
  // The matrices are for the host (the ensembles' tracebacks).  The kernel is bound by its row chain, not by where its stores
  // go, so it writes them straight into page-locked host memory: the transfer rides along with the computation (32 B/cell,
  // ~27 GB/s on the bench block) instead of following it as a copy of its own.  BATH_HIP_FS_REGION_COPY=1: HBM first, then copy.
  const size_t x_bytes = ((size_t)xoff[(size_t)n] * 4 + 255) / 256 * 256;     // then: done flags [n], scores [n]
  if (!dev) { BATH_HIP_TRY(ctx, ctx->stage[Pinned::kFsRegionMatrices].reserve((size_t)foff[(size_t)n] * 4 + 64, true)); BATH_HIP_TRY(ctx, ctx->stage[Pinned::kFsRegionRows].reserve(x_bytes + (size_t)n * 8 + 64, true)); }
  float *d_f = nullptr, *d_fx = nullptr;
  if (!dev) {
    const char *e = std::getenv("BATH_HIP_FS_REGION_COPY");
    void *pf = nullptr, *px = nullptr;
    if (!(e && e[0] == '1') && hipHostGetDevicePointer(&pf, ctx->stage[Pinned::kFsRegionMatrices].p, 0) == hipSuccess && hipHostGetDevicePointer(&px, ctx->stage[Pinned::kFsRegionRows].p, 0) == hipSuccess) {
      d_f = static_cast<float *>(pf); d_fx = static_cast<float *>(px);
    } else (void)hipGetLastError();
  }
  const bool direct = d_f != nullptr;
  int *h_done = dev ? nullptr : reinterpret_cast<int *>(static_cast<char *>(ctx->stage[Pinned::kFsRegionRows].p) + x_bytes);
  float *h_sc = h_done ? reinterpret_cast<float *>(h_done + n) : nullptr;
  const bool live = direct && done_flags != nullptr;
  if (done_flags) { *done_flags = h_done; *sc_live = h_sc; }
  for (int64_t i = 0; h_done && i < n; i++) h_done[i] = 0;
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 3 * sizeof(float)));            // BEFORE its pointer is taken: on a fresh context it is null, and a growing buffer moves
  int *d_done = live ? reinterpret_cast<int *>(reinterpret_cast<char *>(d_fx) + x_bytes) : nullptr;
  float *d_sc_out = live ? reinterpret_cast<float *>(d_done + n) : b_sc.as<float>();
  if (!direct) {                             // (device destination: buffers of its own -- the envelope batches of the same context use kEnvFwdMatrix / kEnvFwdRows)
    DevBuf &bf = dev ? ctx->scratch[Scratch::kFsRegionFwdMatrix] : b_f, &bx = dev ? ctx->scratch[Scratch::kFsRegionFwdRows] : b_fx;
    BATH_HIP_TRY(ctx, bf.reserve((size_t)foff[(size_t)n] * 4 + 64)); BATH_HIP_TRY(ctx, bx.reserve((size_t)xoff[(size_t)n] * 4 + 64));
    d_f = bf.as<float>(); d_fx = bx.as<float>();
  }
  BATH_HIP_TRY(ctx, b_off.reserve((size_t)(n + 1) * 3 * sizeof(int64_t)));
  int64_t *d_foff = b_off.as<int64_t>(), *d_xoff = d_foff + (n + 1);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_foff, foff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_xoff, xoff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  FsJobs jq[2];                                                                // [1]: the ensemble kernel's (device destination)
  if ((st = fs_schedule(ctx, dna, dev ? 2 : 1, jq)) != BATH_OK) return st;
  if ((st = fs5_launch_region_forward(ctx, om, dna, d_sc_out, d_f, d_foff, d_fx, d_xoff, cfg_len_amino, jq[0], d_done, (double)(foff[(size_t)n] / 8))) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipGetLastError());
  if (dev) { *dev = FsRegionDev{d_f, d_fx, d_foff, d_xoff, d_sc_out, jq[1].order, jq[1].counter}; return BATH_OK; }
  sc->resize((size_t)n);
  *fwd = ctx->stage[Pinned::kFsRegionMatrices].as<float>(); *xmx = ctx->stage[Pinned::kFsRegionRows].as<float>();      // page-locked: the matrices are a few MB per region
  if (live) return BATH_OK;                                                  // the flags tell the rest
  if (!direct) {
    BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsRegionMatrices].p, b_f.p, (size_t)foff[(size_t)n] * 4, hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kFsRegionRows].p, b_fx.p, (size_t)xoff[(size_t)n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc->data(), b_sc.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (done_flags) for (int64_t i = 0; i < n; i++) { h_sc[i] = (*sc)[(size_t)i]; h_done[i] = 1; }
  return BATH_OK;
}
