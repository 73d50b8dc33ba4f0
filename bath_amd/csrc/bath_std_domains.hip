// bath_std_domains.hip -- the standard (non-frameshift) branch's domain definition: what p7_Pipeline_BATH does with an ORF that
// passed the Forward filter (src/p7_pipeline.c:1741-1771), and what p7_pli_Frameshift does with the ORFs of a window that does
// not take the frameshift branch (:1479-1510).
//
// Reference: p7_BackwardParser, p7_domaindef_ByPosteriorHeuristics_BATH (src/p7_domaindef.c:491-614) with
// rescore_isolated_domain_bath (:1194-1325), then p7_pli_postDomainDef_BATH (src/p7_pipeline.c:1172-1300).
//
// std_domains runs four stages over all survivors of a block:
//  (a) Both parsers with their special-state rows (the wave-per-target kernels of bath_filters.hip; Forward's rows are copied
//      where the cascade kept them), then domain decoding and the region heuristics: std_regions_wave_kernel, a wave per ORF
//      with its rows in LDS, by default; std_regions_kernel, a lane per ORF, under BATH_HIP_STD_SERIAL=1 or when the rows of the
//      longest ORF do not fit in LDS.
//  (b) The multi-domain regions (p7_domaindef.c:539-583): Forward of every region with its full matrix, then the
//      stochastic-trace ensemble in the context's mode (bath_hip_set_std_ensemble) and its clustering; every cluster is an envelope.
//  (c) The envelopes: full Forward / Backward (unihit, L = Ld), then a fill kernel picked by model length (std_fill_choice:
//      posterior decoding, the optimal-accuracy fill and null2 with a wave or a block of four waves per envelope) and the
//      traceback with a wave per envelope (std_trace_wave_kernel).  std_envelope_kernel, a lane per envelope working serially on
//      the matrices in HBM, does all of it for models past 1024 nodes and behind BATH_HIP_STD_SERIAL=1, and the traceback alone
//      behind BATH_HIP_STD_TRACE_LANE=1.  The matrices never leave the device.
//  (d) On the host: coordinates on the sequence, the score corrections, the P-value, the "aliscore < 0" rule (:1286), the
//      --cigar string and the trace of every hit.
// Behind them: bath_hip_pipeline_hits (cascade + std_domains) and the stage-level entry points that impl_hip/ and the kernel
// tests call (bath_hip_forward_full, bath_hip_std_envelopes[_fill], bath_hip_std_region_ensembles).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "bath_common.hpp"
#include "bath_host_threads.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"
#include "bath_std_ens_walk.hpp"

using namespace bath;

namespace {

constexpr int kStdMaxRegions = 48;       // regions kept per ORF; an ORF with more reports the true count and the call fails loudly (the reference has no cap)

// the residues of each target of a view, to out + xoff[t] / 6 (a block per target)
// rows of target q: (len[q] + 1) x 6 floats from src + src_off[q] to dst + dst_off[q]
__global__ void copy_rows_kernel(int64_t n, const int32_t *__restrict__ len, const float *__restrict__ src, const int64_t *__restrict__ src_off,
                                 float *__restrict__ dst, const int64_t *__restrict__ dst_off) {
  for (int64_t q = blockIdx.x; q < n; q += gridDim.x) {
    const float *a = src + src_off[q];
    float *b = dst + dst_off[q];
    const int m = (len[q] + 1) * 6;
    for (int i = threadIdx.x; i < m; i += blockDim.x) b[i] = a[i];
  }
}
__global__ void gather_residues_kernel(SeqView v, const int64_t *__restrict__ xoff, uint8_t *__restrict__ out) {
  for (int64_t t = blockIdx.x; t < v.n; t += gridDim.x) {
    const uint8_t *s = v.data + v.off[t];
    uint8_t *d = out + xoff[t] / 6;
    for (int i = threadIdx.x; i < v.len[t]; i += blockDim.x) d[i] = s[i];
  }
}

// p7_DomainDecoding (impl_sse/decoding.c:155-196) + region heuristics (p7_domaindef.c:520-533, 642-654), lane per ORF
__global__ void std_regions_kernel(int64_t n, const int32_t *__restrict__ len, const float *__restrict__ fx, const float *__restrict__ bx,
                                   const int64_t *__restrict__ x_off, const float *__restrict__ pmove_tab, float *__restrict__ work /* 3 floats per row */,
                                   int32_t *__restrict__ regions /* [n][1 + 3*kStdMaxRegions] */) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  enum { XE = 0, XN, XJ, XB, XC, XS };
  const int L = len[t];
  const float *F = fx + x_off[t], *B = bx + x_off[t];
  float *btot = work + (x_off[t] / 6) * 3, *etot = btot + (L + 1), *mocc = etot + (L + 1);
  int32_t *out = regions + t * (1 + 3 * kStdMaxRegions);
  out[0] = 0;
  const float ploop = 1.0f - pmove_tab[L];                                   // xf[N|J|C][LOOP] of the multihit model at this length
  float scaleproduct = (float)(1.0 / (double)B[XN]);
  btot[0] = etot[0] = mocc[0] = 0.f;
  for (int i = 1; i <= L; i++) {
    btot[i] = btot[i - 1] + (F[(size_t)(i - 1) * 6 + XB] * B[(size_t)(i - 1) * 6 + XB] * F[(size_t)(i - 1) * 6 + XS] * scaleproduct);
    scaleproduct *= F[(size_t)(i - 1) * 6 + XS] / B[(size_t)(i - 1) * 6 + XS];              // 1 unless Backward had to use its own scale factors
    etot[i] = etot[i - 1] + (F[(size_t)i * 6 + XE] * B[(size_t)i * 6 + XE] * F[(size_t)i * 6 + XS] * scaleproduct);
    float njcp = F[(size_t)(i - 1) * 6 + XN] * B[(size_t)i * 6 + XN] * ploop * scaleproduct;
    njcp += F[(size_t)(i - 1) * 6 + XJ] * B[(size_t)i * 6 + XJ] * ploop * scaleproduct;
    njcp += F[(size_t)(i - 1) * 6 + XC] * B[(size_t)i * 6 + XC] * ploop * scaleproduct;
    mocc[i] = (float)(1. - njcp);
  }
  const float rt1 = 0.25f, rt2 = 0.10f, rt3 = 0.20f;
  int i = -1, nreg = 0;
  bool triggered = false;
  for (int j = 1; j <= L; j++) {
    if (!triggered) {
      if (mocc[j] - (btot[j] - btot[j - 1]) < rt2) i = j;
      else if (i == -1) i = j;
      if (mocc[j] >= rt1) triggered = true;
    } else if (mocc[j] - (etot[j] - etot[j - 1]) < rt2) {
      float best = -1.0f;
      for (int z = i; z <= j; z++) best = fmaxf(best, fminf(etot[z] - etot[i - 1], btot[j] - btot[z - 1]));
      if (nreg < kStdMaxRegions) { out[1 + 3 * nreg] = i; out[2 + 3 * nreg] = j; out[3 + 3 * nreg] = best >= rt3 ? 1 : 0; }
      nreg++;
      i = -1; triggered = false;
    }
  }
  out[0] = nreg;                           // may exceed kStdMaxRegions: the host checks
}

// The same with a WAVE per ORF and the rows in LDS (ORFs up to Lcap residues; the lane kernel above takes longer ones).  The per-row
// terms are elementwise (64 lanes); what the reference accumulates in sequence -- the running scale product, btot, etot -- one lane
// accumulates in that order from LDS; the region scan runs uniformly on all lanes with the inner "best split" maximum spread over
// them (a maximum does not care about order).  Same operations in the same order as the lane kernel: identical regions.  The lane
// kernel walked its ORF alone, every row a trip to L2: 1.2 ms for the bench block's 7.6 k ORFs against ~0.1 ms.
__global__ __launch_bounds__(64) void std_regions_wave_kernel(int64_t n, const int32_t *__restrict__ len, const float *__restrict__ fx, const float *__restrict__ bx,
                                                              const int64_t *__restrict__ x_off, const float *__restrict__ pmove_tab, int Lcap,
                                                              int32_t *__restrict__ regions /* [n][1 + 3*kStdMaxRegions] */) {
  extern __shared__ float sm[];                                              // sp, btot, etot, mocc: (Lcap + 1) floats each
  enum { XE = 0, XN, XJ, XB, XC, XS };
  const int lane = threadIdx.x;
  float *ssp = sm, *sb = sm + (Lcap + 1), *se = sb + (Lcap + 1), *smo = se + (Lcap + 1);
  for (int64_t t = blockIdx.x; t < n; t += gridDim.x) {
    const int L = len[t];
    if (L > Lcap) continue;
    const float *F = fx + x_off[t], *B = bx + x_off[t];
    int32_t *out = regions + t * (1 + 3 * kStdMaxRegions);
    const float ploop = 1.0f - pmove_tab[L];
    __syncthreads();                                                         // the previous ORF's readers are done
    for (int i = 1 + lane; i <= L; i += 64) smo[i] = F[(size_t)(i - 1) * 6 + XS] / B[(size_t)(i - 1) * 6 + XS];
    __syncthreads();
    if (lane == 0) {                                                         // scaleproduct after row i (before row i+1)
      float sp = (float)(1.0 / (double)B[XN]);
      ssp[0] = sp;
      for (int i = 1; i <= L; i++) { sp *= smo[i]; ssp[i] = sp; }
    }
    __syncthreads();
    for (int i = 1 + lane; i <= L; i += 64) {
      const float spb = ssp[i - 1], spa = ssp[i];
      sb[i] = F[(size_t)(i - 1) * 6 + XB] * B[(size_t)(i - 1) * 6 + XB] * F[(size_t)(i - 1) * 6 + XS] * spb;
      se[i] = F[(size_t)i * 6 + XE] * B[(size_t)i * 6 + XE] * F[(size_t)i * 6 + XS] * spa;
      float njcp = F[(size_t)(i - 1) * 6 + XN] * B[(size_t)i * 6 + XN] * ploop * spa;
      njcp += F[(size_t)(i - 1) * 6 + XJ] * B[(size_t)i * 6 + XJ] * ploop * spa;
      njcp += F[(size_t)(i - 1) * 6 + XC] * B[(size_t)i * 6 + XC] * ploop * spa;
      smo[i] = (float)(1. - njcp);
    }
    __syncthreads();
    if (lane == 0) {                                                         // btot, etot: sums in the reference's order
      sb[0] = se[0] = smo[0] = 0.f;
      float b = 0.f, e = 0.f;
      for (int i = 1; i <= L; i++) { b = b + sb[i]; sb[i] = b; e = e + se[i]; se[i] = e; }
    }
    __syncthreads();
    const float rt1 = 0.25f, rt2 = 0.10f, rt3 = 0.20f;
    int i = -1, nreg = 0;
    bool triggered = false;
    for (int j = 1; j <= L; j++) {                                           // uniform over the wave: every lane reads the same LDS words
      if (!triggered) {
        if (smo[j] - (sb[j] - sb[j - 1]) < rt2) i = j;
        else if (i == -1) i = j;
        if (smo[j] >= rt1) triggered = true;
      } else if (smo[j] - (se[j] - se[j - 1]) < rt2) {
        float best = -1.0f;
        for (int z = i + lane; z <= j; z += 64) best = fmaxf(best, fminf(se[z] - se[i - 1], sb[j] - sb[z - 1]));
        best = wave_max_f32(best);
        if (lane == 0 && nreg < kStdMaxRegions) { out[1 + 3 * nreg] = i; out[2 + 3 * nreg] = j; out[3 + 3 * nreg] = best >= rt3 ? 1 : 0; }
        nreg++;
        i = -1; triggered = false;
      }
    }
    if (lane == 0) out[0] = nreg;                                            // may exceed kStdMaxRegions: the host checks
  }
}

struct StdEnvOut { int32_t i1, k1, i2, k2, ok; float oasc, domcorrection; int32_t ncol, exact; float aliscore; int32_t pp_off; };

// p7_Decoding + p7_OptimalAccuracy + p7_OATrace + p7_Null2_ByExpectation on one envelope per lane (unihit model).
// fwd / bck: (L+1) x (M+1) x {M, D, I}; on return bck holds the posteriors and fwd the OA matrix, as in the reference.
constexpr int kStdTraceSpread = 64;
constexpr size_t kStdFillSlack = 64 * 16 * 3 * sizeof(float);    // std_envelope_fill_kernel reads the cells of all 64 x C node slots of a row, also past node M
__global__ void std_envelope_kernel(SeqView sq, int M, const float *__restrict__ tf, const float *__restrict__ rf, float *__restrict__ fwd, float *__restrict__ bck,
                                    const int64_t *__restrict__ dp_off, const float *__restrict__ fx, const float *__restrict__ bx, const int64_t *__restrict__ x_off,
                                    float *__restrict__ ppx_all, float *__restrict__ oax_all, float *__restrict__ em_all /* [n][2*(M+1)] */, StdEnvOut *__restrict__ out,
                                    const uint8_t *__restrict__ cons /* [M+1] or null */, uint8_t *__restrict__ tbuf, const int64_t *__restrict__ t_off,
                                    int filled /* std_envelope_fill_kernel already did decoding, OA fill and null2: traceback only */,
                                    const float *__restrict__ msc /* [Kp][M+1] log-odds */, const float *__restrict__ tsc /* [M][8] log */,
                                    const uint8_t *__restrict__ nt /* the DNA block */, const int64_t *__restrict__ nt_base, const int64_t *__restrict__ nt_dir,
                                    float *__restrict__ null2_out = nullptr /* optional [n][Kp]: the null2 vector itself (filled == 0 only) */,
                                    float *__restrict__ col_pp = nullptr /* tr->pp of the alignment columns, first to last, all envelopes densely */,
                                    int *__restrict__ col_cursor = nullptr) {
  // one envelope per wave: the traceback is a state machine and lanes in different states run one after the other (see
  // fs5_trace_kernel); the chip has room for a wave per envelope
  if (threadIdx.x % kStdTraceSpread) return;
  const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kStdTraceSpread;
  if (t >= sq.n) return;
  enum { XE = 0, XN, XJ, XB, XC, XS };
  enum { cM = 0, cD = 1, cI = 2 };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC };
  const int L = sq.len[t];
  const uint8_t *dsq = sq.data + sq.off[t] - 1;                              // dsq[1..L]
  const size_t W = (size_t)(M + 1) * 3;
  float *F = fwd + dp_off[t], *Bk = bck + dp_off[t];
  const float *FX = fx + x_off[t], *BX = bx + x_off[t];
  float *PX = ppx_all + (x_off[t] / 6) * 5, *OX = oax_all + (x_off[t] / 6) * 5;
  StdEnvOut r{-1, -1, -1, -1, 0, 0.f, 0.f, 0, 0, 0.f, 0};
  const float ploop = 1.0f - 2.0f / ((float)L + 2.0f);                       // unihit: xf[N|J|C][LOOP]
  const float *P = Bk;
  float *O = F;
  if (filled) {
    const StdEnvOut pre = out[t];
    if (!pre.ok) { out[t] = r; return; }
    r.oasc = pre.oasc; r.domcorrection = pre.domcorrection;
  }
  if (!filled) {
  // ---- p7_Decoding (decoding.c:61-118): posteriors overwrite Backward
  float scaleproduct = (float)(1.0 / (double)BX[XN]);
  for (int k = 0; k <= M; k++) Bk[(size_t)k * 3] = Bk[(size_t)k * 3 + 1] = Bk[(size_t)k * 3 + 2] = 0.f;
  for (int s = 0; s < 5; s++) PX[s] = 0.f;
  for (int i = 1; i <= L; i++) {
    const float totr = scaleproduct * FX[(size_t)i * 6 + XS];
    const float *f = F + (size_t)i * W;
    float *b = Bk + (size_t)i * W;
    for (int k = 1; k <= M; k++) {
      b[(size_t)k * 3 + cM] = f[(size_t)k * 3 + cM] * (b[(size_t)k * 3 + cM] * totr);
      b[(size_t)k * 3 + cD] = 0.0f;
      b[(size_t)k * 3 + cI] = f[(size_t)k * 3 + cI] * (b[(size_t)k * 3 + cI] * totr);
    }
    float *px = PX + (size_t)i * 5;
    px[XE] = 0.f; px[XB] = 0.f;
    px[XN] = FX[(size_t)(i - 1) * 6 + XN] * BX[(size_t)i * 6 + XN] * ploop * scaleproduct;
    px[XJ] = FX[(size_t)(i - 1) * 6 + XJ] * BX[(size_t)i * 6 + XJ] * ploop * scaleproduct;
    px[XC] = FX[(size_t)(i - 1) * 6 + XC] * BX[(size_t)i * 6 + XC] * ploop * scaleproduct;
    scaleproduct *= FX[(size_t)i * 6 + XS] / BX[(size_t)i * 6 + XS];
  }
  if (isinf(scaleproduct)) { out[t] = r; return; }                           // eslERANGE: the domain is dropped (p7_domaindef.c:1214)
  // ---- p7_OptimalAccuracy (optacc.c:58-173): the OA matrix overwrites Forward
  auto allow = [](float tr, float v) { return tr > 0.0f ? v : 0.0f; };
  for (int k = 0; k <= M; k++) O[(size_t)k * 3] = O[(size_t)k * 3 + 1] = O[(size_t)k * 3 + 2] = -INFINITY;
  OX[XE] = -INFINITY; OX[XN] = 0.f; OX[XJ] = -INFINITY; OX[XB] = 0.f; OX[XC] = -INFINITY;
  for (int i = 1; i <= L; i++) {
    const float *p = P + (size_t)i * W, *pr = O + (size_t)(i - 1) * W;
    float *c = O + (size_t)i * W;
    const float xB = OX[(size_t)(i - 1) * 5 + XB];
    c[0] = c[1] = c[2] = -INFINITY;
    float xE = -INFINITY, dcv = -INFINITY;
    for (int k = 1; k <= M; k++) {
      const float *tr = tf + (size_t)k * 8;
      float sv = allow(tr[BM], xB);
      sv = fmaxf(sv, allow(tr[MM], pr[(size_t)(k - 1) * 3 + cM]));
      sv = fmaxf(sv, allow(tr[IM], pr[(size_t)(k - 1) * 3 + cI]));
      sv = fmaxf(sv, allow(tr[DM], pr[(size_t)(k - 1) * 3 + cD]));
      sv = sv + p[(size_t)k * 3 + cM];
      xE = fmaxf(xE, sv);
      c[(size_t)k * 3 + cM] = sv;
      c[(size_t)k * 3 + cD] = dcv;
      dcv = fmaxf(allow(tr[MD], sv), allow(tr[DD], dcv));
      c[(size_t)k * 3 + cI] = fmaxf(allow(tr[MI], pr[(size_t)k * 3 + cM]), allow(tr[II], pr[(size_t)k * 3 + cI])) + p[(size_t)k * 3 + cI];
    }
    for (int k = 1; k <= M; k++) xE = fmaxf(xE, c[(size_t)k * 3 + cD]);
    float *ox = OX + (size_t)i * 5;
    const float *opx = OX + (size_t)(i - 1) * 5, *px = PX + (size_t)i * 5;
    ox[XE] = xE;
    ox[XJ] = fmaxf(opx[XJ] + px[XJ], 0.0f);                                  // unihit: xf[E][LOOP] == 0 -> the E->J term is 0.0 (optacc.c:156)
    ox[XC] = fmaxf(opx[XC] + px[XC], xE);
    ox[XN] = opx[XN] + px[XN];
    ox[XB] = fmaxf(ox[XN], ox[XJ]);
  }
  r.oasc = OX[(size_t)L * 5 + XC];
  }
  // ---- p7_OATrace (optacc.c:225-430); select_e walks the cells in the reference's striped order
  {
    const int Q = max(2, (M - 1) / 4 + 1);
    auto path = [](float tr, float v) { return tr == 0.0f ? -INFINITY : v; };
    int i = L, k = 0, s0 = sC, steps = 0;
    bool bad = false;
    // the alignment columns from the last match state back to the first, for the display (p7_alidisplay_nonfs_Create)
    uint8_t *T = tbuf + t_off[t];
    const int cap = (int)(t_off[t + 1] - t_off[t]);
    int ncol = 0, exact = 0;
    while (s0 != sS && !bad) {
      int s1 = -1;
      switch (s0) {
      case sM: {
        const float *tr = tf + (size_t)k * 8, *pr = O + (size_t)(i - 1) * W;
        const float pm = path(tr[MM], pr[(size_t)(k - 1) * 3 + cM]), pi = path(tr[IM], pr[(size_t)(k - 1) * 3 + cI]);
        const float pd = path(tr[DM], pr[(size_t)(k - 1) * 3 + cD]), pb = path(tr[BM], OX[(size_t)(i - 1) * 5 + XB]);
        s1 = sM; float b = pm;
        if (pi > b) { b = pi; s1 = sI; }
        if (pd > b) { b = pd; s1 = sD; }
        if (pb > b) { b = pb; s1 = sB; }
        k--; i--; break; }
      case sD: {
        const float *tr = tf + (size_t)(k - 1) * 8, *c = O + (size_t)i * W;
        const float pm = (k - 1 >= 1) ? path(tr[MD], c[(size_t)(k - 1) * 3 + cM]) : -INFINITY;
        const float pd = (k - 1 >= 1) ? path(tr[DD], c[(size_t)(k - 1) * 3 + cD]) : -INFINITY;
        s1 = pm >= pd ? sM : sD; k--; break; }
      case sI: {
        const float *tr = tf + (size_t)k * 8, *pr = O + (size_t)(i - 1) * W;
        s1 = path(tr[MI], pr[(size_t)k * 3 + cM]) >= path(tr[II], pr[(size_t)k * 3 + cI]) ? sM : sI; i--; break; }
      case sN: s1 = (i == 0) ? sS : sN; break;
      case sC: s1 = (OX[(size_t)(i - 1) * 5 + XC] + PX[(size_t)i * 5 + XC] > OX[(size_t)i * 5 + XE]) ? sC : sE; break;
      case sJ: s1 = sJ; break;                                                // unihit: E->J impossible, path[1] = -inf (optacc.c:384)
      case sE: {
        const float *c = O + (size_t)i * W;
        float mx = -INFINITY; int smax = -1, kmax = -1;
        for (int q = 0; q < Q; q++) {
          for (int rr = 0; rr < 4; rr++) { const int kk = rr * Q + q + 1; if (kk <= M && c[(size_t)kk * 3 + cM] >= mx) { mx = c[(size_t)kk * 3 + cM]; smax = sM; kmax = kk; } }
          for (int rr = 0; rr < 4; rr++) { const int kk = rr * Q + q + 1; if (kk <= M && c[(size_t)kk * 3 + cD] > mx) { mx = c[(size_t)kk * 3 + cD]; smax = sD; kmax = kk; } }
        }
        k = kmax; s1 = smax; break; }
      case sB: s1 = (OX[(size_t)i * 5 + XN] > OX[(size_t)i * 5 + XJ]) ? sN : sJ; break;
      default: bad = true; break;
      }
      if (bad || s1 < 0 || i < 0 || k < 0) { bad = true; break; }
      if (s1 == sM) { if (r.i2 < 0) { r.i2 = i; r.k2 = k; } r.i1 = i; r.k1 = k; }
      if ((s1 == sM || s1 == sD || s1 == sI) && r.i2 >= 0) {
        if (ncol < cap) T[ncol] = (uint8_t)s1;
        ncol++;
        if (s1 == sM) { r.ncol = ncol; if (cons && min((int)dsq[i], kKp - 1) == cons[k]) exact++; r.exact = exact; }
      }
      if ((s1 == sN || s1 == sJ || s1 == sC) && s1 == s0) i--;
      s0 = s1;
      if (++steps > 4 * (L + M) + 64) bad = true;
    }
    if (bad || r.i1 <= 0) { out[t] = r; return; }
    // ---- p7_pli_computeAliScores_BATH (p7_pipeline.c:781-979) on the columns, first to last match state: the emission score of
    // each codon's amino acid (X for a codon with a degenerate nucleotide, p7P_DEGEN5_C) plus the transition that entered the
    // state; the last match state gets no MM transition (the reference's inner loops stop at z1 < z2).  Negative total: the
    // caller drops the domain (p7_domaindef.c:1286).
    if (msc && r.ncol <= cap) {
      const size_t W1 = (size_t)M + 1;
      const int64_t base = nt_base[t], dir = nt_dir[t];
      float total = 0.f;
      int prev = sB, kk = r.k1 - 1, ii = r.i1 - 1;
      for (int idx = r.ncol - 1; idx >= 0; idx--) {
        const int s = T[idx];
        float sc;
        if (s == sM) {
          kk++; ii++;
          int amino = min((int)dsq[ii], kKp - 1);
          const int64_t c0 = base + dir * (int64_t)(3 * (ii - 1));
          if (nt[c0] >= 4 || nt[c0 + dir] >= 4 || nt[c0 + 2 * dir] >= 4) amino = 26;
          sc = msc[(size_t)amino * W1 + kk];
          if (prev == sI) sc += tsc[(size_t)(kk - 1) * 8 + IM];
          else if (prev == sD) sc += tsc[(size_t)(kk - 1) * 8 + DM];
          else if (prev == sM && idx > 0) sc += tsc[(size_t)(kk - 1) * 8 + MM];
        } else if (s == sI) { ii++; sc = tsc[(size_t)kk * 8 + (prev == sI ? II : MI)]; }
        else { kk++; sc = tsc[(size_t)(kk - 1) * 8 + (prev == sD ? DD : MD)]; }
        total += sc;
        prev = s;
      }
      r.aliscore = total;
    }
    // ---- the posterior of every column's state, first to last (p7_OATrace's get_postprob, optacc.c: M and I cells of the
    // posterior matrix; a delete state has none), for bath_hip_domain_traces
    if (col_pp && r.ncol <= cap && r.ncol > 0) {
      r.pp_off = atomicAdd(col_cursor, r.ncol);
      float *out_pp = col_pp + r.pp_off;
      int kk = r.k1 - 1, ii = r.i1 - 1;
      for (int idx = r.ncol - 1; idx >= 0; idx--) {
        const int s = T[idx];
        float v = 0.0f;
        if (s == sM) { kk++; ii++; v = P[(size_t)ii * W + (size_t)kk * 3 + cM]; }
        else if (s == sI) { ii++; v = P[(size_t)ii * W + (size_t)kk * 3 + cI]; }
        else kk++;
        out_pp[r.ncol - 1 - idx] = v;
      }
    }
  }
  // ---- p7_Null2_ByExpectation (null2.c:50-124) and the correction over the envelope (p7_domaindef.c:1264-1272)
  if (!filled) {
    float *em = em_all + (size_t)t * 2 * (M + 1);
    float xN = PX[5 + XN], xC = PX[5 + XC], xJ = PX[5 + XJ];
    for (int k = 1; k <= M; k++) { em[2 * k] = P[W + (size_t)k * 3 + cM]; em[2 * k + 1] = P[W + (size_t)k * 3 + cI]; }
    for (int i = 2; i <= L; i++) {
      const float *p = P + (size_t)i * W;
      for (int k = 1; k <= M; k++) { em[2 * k] = p[(size_t)k * 3 + cM] + em[2 * k]; em[2 * k + 1] = p[(size_t)k * 3 + cI] + em[2 * k + 1]; }
      xN += PX[(size_t)i * 5 + XN]; xC += PX[(size_t)i * 5 + XC]; xJ += PX[(size_t)i * 5 + XJ];
    }
    const float norm = (float)(1.0 / (double)(float)L);
    for (int k = 1; k <= M; k++) { em[2 * k] *= norm; em[2 * k + 1] *= norm; }
    xN *= norm; xC *= norm; xJ *= norm;
    const float xfactor = xN + xC + xJ;
    float null2[kKp];
    for (int x = 0; x < 20; x++) {
      const float *e = rf + (size_t)x * (M + 1);
      float sv = 0.f;
      for (int k = 1; k <= M; k++) { sv += em[2 * k] * e[k]; sv += em[2 * k + 1]; }
      null2[x] = sv + xfactor;
    }
    const int mem[6][2] = {{2, 11}, {7, 9}, {3, 13}, {8, 8}, {1, 1}, {-1, -1}};      // B=DN J=IL Z=EQ O=K U=C X=any
    for (int dx = 0; dx < 6; dx++) {
      float sum = 0.f; int cnt = 0;
      if (dx == 5) { for (int y = 0; y < 20; y++) { sum += null2[y]; cnt++; } }
      else { const int a = min(mem[dx][0], mem[dx][1]), b = max(mem[dx][0], mem[dx][1]); sum += null2[a]; cnt++; if (b != a) { sum += null2[b]; cnt++; } }
      null2[21 + dx] = sum / (float)cnt;
    }
    null2[20] = 1.0f; null2[27] = 1.0f; null2[28] = 1.0f;
    if (null2_out) for (int x = 0; x < kKp; x++) null2_out[(size_t)t * kKp + x] = null2[x];
    float corr = 0.f;
    for (int pos = 1; pos <= L; pos++) corr += logf(null2[min((int)dsq[pos], kKp - 1)]);
    r.domcorrection = corr;
  }
  r.ok = 1;
  out[t] = r;
}

// p7_OATrace and what follows it in std_envelope_kernel (alignment score, the columns' posteriors) for an envelope whose matrices
// std_envelope_fill_kernel left behind, with the WAVE walking instead of one lane.  The walk is a chain of decisions, each on cells
// whose address the previous decision gives: a lane on its own pays a trip to memory per step (0.8 us; 900 steps for a 459-node
// model).  Here every lane follows the same state machine on the same (uniform) state and the cells come from look-ahead buffers
// filled by all 64 lanes at once:
//   * a match run walks a diagonal: on entering (i, k) lane d fetches what the step from (i - d, k - d) will need -- the three cells
//     of (i - 1 - d, k - 1 - d), B of that row, the four transitions into node k - d, the residue and the consensus residue of the
//     cell it leads to -- and the steps take them by v_readlane until the path leaves the diagonal or the 64 are used;
//   * the C flank is decided 64 rows at a time (a ballot of "stays in C"); the N flank needs no reads at all;
//   * the E state's choice among the 2 M cells of a row (the reference scans them in its striped order: ties go to the LAST match
//     cell of the scan, else to the FIRST delete cell) is a lane-parallel scan and two wave maxima over (value, rank);
//   * the columns' scores and posteriors are gathered a lane per column (prefix counts of the column kinds by ballot), and the
//     score is summed in the reference's order, first to last column.
// Same decisions on the same values: the trace is the serial kernel's, state for state (tests/test_hits_gpu.py runs both).
__global__ __launch_bounds__(64) void std_trace_wave_kernel(SeqView sq, int M, const float *__restrict__ tf, const float *__restrict__ fwd, const float *__restrict__ bck,
                                                            const int64_t *__restrict__ dp_off, const int64_t *__restrict__ x_off,
                                                            const float *__restrict__ ppx_all, const float *__restrict__ oax_all, StdEnvOut *__restrict__ out,
                                                            const uint8_t *__restrict__ cons /* [M+1] or null */, uint8_t *__restrict__ tbuf, const int64_t *__restrict__ t_off,
                                                            const float *__restrict__ msc /* [Kp][M+1] log-odds */, const float *__restrict__ tsc /* [M][8] log */,
                                                            const uint8_t *__restrict__ nt /* the DNA block */, const int64_t *__restrict__ nt_base, const int64_t *__restrict__ nt_dir,
                                                            float *__restrict__ col_pp, int *__restrict__ col_cursor) {
  enum { XE = 0, XN, XJ, XB, XC, XS };
  enum { cM = 0, cD = 1, cI = 2 };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  enum { sS = 0, sN, sB, sM, sD, sI, sE, sJ, sC };
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int L = sq.len[t];
  const uint8_t *dsq = sq.data + sq.off[t] - 1;                              // dsq[1..L]
  const size_t W = (size_t)(M + 1) * 3;
  const float *O = fwd + dp_off[t], *P = bck + dp_off[t];
  const float *PX = ppx_all + (x_off[t] / 6) * 5, *OX = oax_all + (x_off[t] / 6) * 5;
  StdEnvOut r{-1, -1, -1, -1, 0, 0.f, 0.f, 0, 0, 0.f, 0};
  {
    const StdEnvOut pre = out[t];
    if (!pre.ok) { if (lane == 0) out[t] = r; return; }
    r.oasc = pre.oasc; r.domcorrection = pre.domcorrection;
  }
  auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
  auto rlf = [](float v, int d) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), d)); };
  auto path = [](float tr, float v) { return tr == 0.0f ? -INFINITY : v; };
  const int Q = max(2, (M - 1) / 4 + 1);
  uint8_t *T = tbuf + t_off[t];
  const int cap = (int)(t_off[t + 1] - t_off[t]);
  int i = L, k = 0, s0 = sC, steps = 0, ncol = 0, exact = 0;
  bool bad = false;
  // the diagonal look-ahead: lane d holds what the match step from (di0 - d, dk0 - d) reads
  float dM = 0.f, dI = 0.f, dD = 0.f, dXB = 0.f;
  float4 dT = make_float4(0.f, 0.f, 0.f, 0.f);
  int dRes = 0, dCons = -1, di0 = -(1 << 20), dk0 = -(1 << 20);
  while (s0 != sS && !bad) {
    i = uni(i); k = uni(k); s0 = uni(s0);
    int s1 = -1;
    bool from_diag = false; int dd = 0;
    if (s0 == sC) {
      const int rr = i - lane;
      bool stay = false;
      if (rr >= 1) stay = OX[(size_t)(rr - 1) * 5 + XC] + PX[(size_t)rr * 5 + XC] > OX[(size_t)rr * 5 + XE];
      const unsigned long long m = __ballot(stay);
      const int n = (~m == 0ull) ? 64 : (__ffsll((long long)~m) - 1);         // rows i, i-1, ... that stay in C
      if (n > 0) { i -= n; steps += n; if (steps > 4 * (L + M) + 64) bad = true; continue; }
      s1 = sE;
    } else if (s0 == sN) {                                                    // N(i) <- N(i-1) ... <- N(0) <- S: nothing to read
      steps += i + 1; i = 0; s0 = sS; continue;
    } else if (s0 == sM) {
      dd = di0 - i;
      if (dd < 0 || dd >= 64 || dk0 - k != dd) {
        const int ii = max(i - 1 - lane, 0), kk = max(k - 1 - lane, 0);
        const float *pr = O + (size_t)ii * W + (size_t)kk * 3;
        dM = pr[cM]; dI = pr[cI]; dD = pr[cD]; dXB = OX[(size_t)ii * 5 + XB];
        dT = *reinterpret_cast<const float4 *>(tf + (size_t)max(k - lane, 0) * 8);
        dRes = min((int)dsq[max(ii, 1)], kKp - 1); dCons = cons ? (int)cons[kk] : -1;
        di0 = i; dk0 = k; dd = 0;
      }
      dd = uni(dd);
      const float pm = path(rlf(dT.x, dd), rlf(dM, dd)), pi = path(rlf(dT.y, dd), rlf(dI, dd));
      const float pd = path(rlf(dT.z, dd), rlf(dD, dd)), pb = path(rlf(dT.w, dd), rlf(dXB, dd));
      s1 = sM; float b = pm;
      if (pi > b) { b = pi; s1 = sI; }
      if (pd > b) { b = pd; s1 = sD; }
      if (pb > b) { b = pb; s1 = sB; }
      k--; i--; from_diag = true;
    } else if (s0 == sD) {
      const float *tr = tf + (size_t)max(k - 1, 0) * 8, *c = O + (size_t)i * W;
      const float pm = (k - 1 >= 1) ? path(tr[MD], c[(size_t)(k - 1) * 3 + cM]) : -INFINITY;
      const float pd = (k - 1 >= 1) ? path(tr[DD], c[(size_t)(k - 1) * 3 + cD]) : -INFINITY;
      s1 = pm >= pd ? sM : sD; k--;
    } else if (s0 == sI) {
      const float *tr = tf + (size_t)k * 8, *pr = O + (size_t)(i - 1) * W;
      s1 = path(tr[MI], pr[(size_t)k * 3 + cM]) >= path(tr[II], pr[(size_t)k * 3 + cI]) ? sM : sI; i--;
    } else if (s0 == sJ) {
      s1 = sJ;                                                                // unihit: E->J impossible, path[1] = -inf (optacc.c:384)
    } else if (s0 == sE) {
      // select_e over the reference's striped order q = 0..Q-1: the four match cells rr*Q + q + 1 (>=: a later one takes a tie),
      // then the four delete cells (>: an earlier one keeps it).  rank: scan position, match cells above all delete cells.
      const float *c = O + (size_t)i * W;
      float mx = -INFINITY; int rank = -1;
      for (int q = lane; q < Q; q += 64) {
        for (int rr = 0; rr < 4; rr++) { const int kk = rr * Q + q + 1; if (kk <= M) { const float v = c[(size_t)kk * 3 + cM]; const int rk = (1 << 24) + q * 8 + rr; if (v > mx || (v == mx && rk > rank)) { mx = v; rank = rk; } } }
        for (int rr = 0; rr < 4; rr++) { const int kk = rr * Q + q + 1; if (kk <= M) { const float v = c[(size_t)kk * 3 + cD]; const int rk = (1 << 23) - (q * 8 + 4 + rr); if (v > mx || (v == mx && rk > rank)) { mx = v; rank = rk; } } }
      }
      const float best = wave_max_f32(mx);
      const int brank = wave_max_i32((mx == best) ? rank : -1);
      if (brank < 0) bad = true;
      else if (brank >= (1 << 24)) { const int pq = brank - (1 << 24); k = (pq & 7) * Q + (pq >> 3) + 1; s1 = sM; }
      else { const int pq = (1 << 23) - brank; k = ((pq & 7) - 4) * Q + (pq >> 3) + 1; s1 = sD; }
    } else if (s0 == sB) {
      s1 = (OX[(size_t)i * 5 + XN] > OX[(size_t)i * 5 + XJ]) ? sN : sJ;
    } else bad = true;
    if (bad || s1 < 0 || i < 0 || k < 0) { bad = true; break; }
    if (s1 == sM) { if (r.i2 < 0) { r.i2 = i; r.k2 = k; } r.i1 = i; r.k1 = k; }
    if ((s1 == sM || s1 == sD || s1 == sI) && r.i2 >= 0) {
      if (ncol < cap && lane == 0) T[ncol] = (uint8_t)s1;
      ncol++;
      if (s1 == sM) {
        r.ncol = ncol;
        if (cons) {
          int res, cn;
          if (from_diag) { res = __builtin_amdgcn_readlane(dRes, dd); cn = __builtin_amdgcn_readlane(dCons, dd); }
          else { res = min((int)dsq[i], kKp - 1); cn = (int)cons[k]; }
          if (res == cn) exact++;
        }
        r.exact = exact;
      }
    }
    if ((s1 == sN || s1 == sJ || s1 == sC) && s1 == s0) i--;
    s0 = s1;
    if (++steps > 4 * (L + M) + 64) bad = true;
  }
  if (bad || r.i1 <= 0) { if (lane == 0) out[t] = r; return; }
  __threadfence();                                                            // lane 0's column bytes, read below by every lane
  // ---- the columns, first to last match state (column j of the alignment = T[ncol' - 1 - j], ncol' = r.ncol), a lane per
  // column: its node and residue from prefix counts of the column kinds; p7_pli_computeAliScores_BATH (p7_pipeline.c:781-979)
  // summed in the reference's order, and the posterior of every column's state (optacc.c, get_postprob)
  const int nc = r.ncol;
  if (nc <= cap && nc > 0) {
    const size_t W1 = (size_t)M + 1;
    const int64_t base = nt_base[t], dir = nt_dir[t];
    int pp_off = 0;
    if (col_pp) { if (lane == 0) pp_off = atomicAdd(col_cursor, nc); pp_off = uni(pp_off); r.pp_off = pp_off; }
    float total = 0.f;
    int kbase = r.k1 - 1, ibase = r.i1 - 1, prev_last = sB;
    for (int jb = 0; jb < nc; jb += 64) {
      const int j = jb + lane;
      const bool in = j < nc;
      const int s = in ? (int)T[nc - 1 - j] : -1;
      const unsigned long long bMm = __ballot(s == sM), bIm = __ballot(s == sI), bDm = __ballot(s == sD);
      const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
      const int kk = kbase + __popcll((bMm | bDm) & upto), ii = ibase + __popcll((bMm | bIm) & upto);
      int prev = __shfl_up(s, 1, 64);
      if (lane == 0) prev = prev_last;
      float sc = 0.f, ppv = 0.f;
      if (in) {
        if (s == sM) {
          int amino = min((int)dsq[ii], kKp - 1);
          const int64_t c0 = base + dir * (int64_t)(3 * (ii - 1));
          if (nt[c0] >= 4 || nt[c0 + dir] >= 4 || nt[c0 + 2 * dir] >= 4) amino = 26;
          sc = msc[(size_t)amino * W1 + kk];
          if (prev == sI) sc += tsc[(size_t)(kk - 1) * 8 + IM];
          else if (prev == sD) sc += tsc[(size_t)(kk - 1) * 8 + DM];
          else if (prev == sM && j < nc - 1) sc += tsc[(size_t)(kk - 1) * 8 + MM];
          ppv = P[(size_t)ii * W + (size_t)kk * 3 + cM];
        } else if (s == sI) { sc = tsc[(size_t)kk * 8 + (prev == sI ? II : MI)]; ppv = P[(size_t)ii * W + (size_t)kk * 3 + cI]; }
        else sc = tsc[(size_t)(kk - 1) * 8 + (prev == sD ? DD : MD)];
        if (col_pp) col_pp[pp_off + j] = ppv;
      }
      const int nin = min(64, nc - jb);
      if (msc) for (int l = 0; l < nin; l++) total += rlf(sc, l);
      kbase += __popcll(bMm | bDm); ibase += __popcll(bMm | bIm);
      prev_last = __builtin_amdgcn_readlane(s, 63);
    }
    if (msc) r.aliscore = total;
  }
  r.ok = 1;
  if (lane == 0) out[t] = r;
}

// The same decoding, optimal-accuracy fill and null2 with a WAVE per envelope: lanes own C consecutive nodes each, rows are
// walked in order with the previous row in registers (neighbours by shuffle), the row's D chain D(k+1) = max(MD_k ? M_k : 0,
// DD_k ? D_k : 0) is a wavefront scan over functions x -> pass ? max(c, x) : c (closed under composition), xE a wave max.
// max / select only, so the OA matrix is bit-identical to the serial fill and the traceback (std_envelope_kernel with
// filled = 1, a lane per envelope) takes the same path.  Posteriors live in registers only: their column sums for null2 are
// accumulated on the fly in the serial kernel's order; only null2's sum over the nodes is associated differently (wave sum).
// The lane-per-envelope fill took 35 ms for 1500 envelopes (every cell a dependent trip to HBM); this one is well under 1 ms.
template <int C>
__global__ __launch_bounds__(256) void std_envelope_fill_kernel(SeqView sq, int M, const float *__restrict__ tf, const float *__restrict__ rf, float *__restrict__ fwd,
                                                                float *__restrict__ bck, const int64_t *__restrict__ dp_off, const float *__restrict__ fx,
                                                                const float *__restrict__ bx, const int64_t *__restrict__ x_off, float *__restrict__ ppx_all,
                                                                float *__restrict__ oax_all, StdEnvOut *__restrict__ out,
                                                                float *__restrict__ null2_out /* optional [n][Kp]: the null2 vector itself */) {
  enum { XE = 0, XN, XJ, XB, XC, XS };
  enum { cM = 0, cD = 1, cI = 2 };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // What the row loop needs per node, in registers, so that it has no branch per node (a wave alone on its SIMD issues an
  // instruction every five cycles or so: with a branch, two compares and two selects per allow() the row of a 459-node model took
  // 1300 instructions, 3.6 us): the transitions as all-ones / zero masks (allow(tr, v) = v AND mask: exact, v or +0.0), and for
  // the nodes beyond M limits that turn what is computed for them into the values the guarded code left there (min(x, -inf)).
  auto band = [](float v, unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); };
  auto vmax = [](float x, float y) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };      // (no operand is ever NaN: see bath_fs_device.hpp)
  auto vmin = [](float x, float y) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
  unsigned kBM[C], kMM[C], kIM[C], kDM[C], kMD[C], kDD[C], kMI[C], kII[C], vm[C];
  float lim[C], npz[C], plim[C];
  const bool full = lane * C + C <= M, partial = !full && lane * C + 1 <= M;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const int node = lane * C + c + 1;
    const bool ok = node <= M;
    const float *tq = tf + (size_t)min(node, M) * 8;
    auto mk = [&](int q) { return (ok && tq[q] > 0.0f) ? 0xffffffffu : 0u; };
    kMM[c] = mk(MM); kIM[c] = mk(IM); kDM[c] = mk(DM); kBM[c] = mk(BM); kMD[c] = mk(MD); kDD[c] = mk(DD); kMI[c] = mk(MI); kII[c] = mk(II);
    vm[c] = ok ? 0xffffffffu : 0u;
    lim[c] = ok ? INFINITY : -INFINITY;
    const bool pass = !ok || tq[DD] > 0.0f;                                 // a node that is not there: the identity of the D chain
    npz[c] = pass ? -INFINITY : 0.0f;
    plim[c] = pass ? INFINITY : -INFINITY;
  }
  for (int64_t t0 = wid; t0 < sq.n; t0 += nw) {
    const int64_t t = __builtin_amdgcn_readfirstlane((int)t0);              // (the wave's envelope: uniform, so that its pointers are scalars)
    const int L = sq.len[t];
    const uint8_t *dsq = sq.data + sq.off[t] - 1;
    const size_t W = (size_t)(M + 1) * 3;
    float *F = fwd + dp_off[t];
    float *Bk = bck + dp_off[t];
    const float *FX = fx + x_off[t], *BX = bx + x_off[t];
    float *PX = ppx_all + (x_off[t] / 6) * 5, *OX = oax_all + (x_off[t] / 6) * 5;
    const float ploop = 1.0f - 2.0f / ((float)L + 2.0f);
    float pvM[C], pvI[C], pvD[C], emM[C], emI[C];
#pragma unroll
    for (int c = 0; c < C; c++) { pvM[c] = pvI[c] = pvD[c] = -INFINITY; emM[c] = emI[c] = 0.f; }
    float oxN = 0.f, oxJ = -INFINITY, oxC = -INFINITY, oxB = 0.f, sN = 0.f, sC = 0.f, sJ = 0.f;
    float scaleproduct = (float)(1.0 / (double)BX[XN]);
    for (int k = lane; k <= M; k += 64) F[(size_t)k * 3] = F[(size_t)k * 3 + 1] = F[(size_t)k * 3 + 2] = -INFINITY;      // OA row 0
    if (lane == 0) {
      for (int q = 0; q < 5; q++) PX[q] = 0.f;
      OX[XE] = -INFINITY; OX[XN] = 0.f; OX[XJ] = -INFINITY; OX[XB] = 0.f; OX[XC] = -INFINITY;
    }
    // Nothing in a row waits for memory: the Forward and Backward cells of row i + 1 are fetched while row i is worked on, and the
    // special states arrive 64 rows at a time, a lane each (lane l of a chunk: Forward's N, J, C of row r - 1 and its scale factor of
    // row r, Backward's N, J, C and scale factor of row r), the next 64 in flight.
    // (a lane reads its C nodes' cells whether they exist or not -- the buffers end in slack for that -- and masks what it read)
    float fM[C], fI[C], bM[C], bI[C];
    const size_t lane0 = (size_t)(lane * C + 1) * 3;
    auto fetch_row = [&](int r) {
      const float *fq = F + (size_t)r * W + lane0, *bq = Bk + (size_t)r * W + lane0;
#pragma unroll
      for (int c = 0; c < C; c++) { fM[c] = fq[3 * c + cM]; fI[c] = fq[3 * c + cI]; bM[c] = bq[3 * c + cM]; bI[c] = bq[3 * c + cI]; }
    };
    float xb[8], xn[8];
    auto fetch_x = [&](int r0, float (&v)[8]) {                             // rows r0 .. r0 + 63, a lane each
      const int r = min(r0 + lane, L);
      v[0] = FX[(size_t)(r - 1) * 6 + XN]; v[1] = FX[(size_t)(r - 1) * 6 + XJ]; v[2] = FX[(size_t)(r - 1) * 6 + XC]; v[3] = FX[(size_t)r * 6 + XS];
      v[4] = BX[(size_t)r * 6 + XN]; v[5] = BX[(size_t)r * 6 + XJ]; v[6] = BX[(size_t)r * 6 + XC]; v[7] = BX[(size_t)r * 6 + XS];
    };
    if (L >= 1) { fetch_row(1); fetch_x(1, xb); }
    for (int i = 1; i <= L; i++) {
      const int j = (i - 1) & 63;
      if (j == 0 && i + 64 <= L) fetch_x(i + 64, xn);
      float xv[8];
#pragma unroll
      for (int q = 0; q < 8; q++) xv[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xb[q]), j));
      if (j == 63) {
#pragma unroll
        for (int q = 0; q < 8; q++) xb[q] = xn[q];
      }
      const float totr = scaleproduct * xv[3];
      float *frow = F + (size_t)i * W;
      float *brow = Bk + (size_t)i * W;
      // posteriors of this row (p7_Decoding), special states included; they replace the Backward row as in the reference
      // (p7_Decoding(om, ox1, ox2, ox2), p7_domaindef.c:1249: the traceback kernel reads a column's posterior there)
      float pM[C], pI[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        pM[c] = band(fM[c] * (bM[c] * totr), vm[c]);
        pI[c] = band(fI[c] * (bI[c] * totr), vm[c]);
        if (i == 1) { emM[c] = pM[c]; emI[c] = pI[c]; } else { emM[c] = pM[c] + emM[c]; emI[c] = pI[c] + emI[c]; }
      }
      if (i < L) fetch_row(i + 1);                                          // in flight during the optimal-accuracy part of this row
      const float pxN = xv[0] * xv[4] * ploop * scaleproduct;
      const float pxJ = xv[1] * xv[5] * ploop * scaleproduct;
      const float pxC = xv[2] * xv[6] * ploop * scaleproduct;
      if (i == 1) { sN = pxN; sC = pxC; sJ = pxJ; } else { sN += pxN; sC += pxC; sJ += pxJ; }
      scaleproduct *= xv[3] / xv[7];
      // optimal-accuracy row (p7_OptimalAccuracy)
      const float mIn = wave_shr1_f32(pvM[C - 1], -INFINITY), iIn = wave_shr1_f32(pvI[C - 1], -INFINITY), dIn = wave_shr1_f32(pvD[C - 1], -INFINITY);
      float cuM[C], cuI[C], cuD[C];
      float fc = -INFINITY; unsigned fpass = 0xffffffffu;                   // the lane's composite D-chain function
      float xE = -INFINITY;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const float m1 = c == 0 ? mIn : pvM[c - 1], i1 = c == 0 ? iIn : pvI[c - 1], d1 = c == 0 ? dIn : pvD[c - 1];
        float sv = band(oxB, kBM[c]);
        sv = vmax(sv, band(m1, kMM[c]));
        sv = vmax(sv, band(i1, kIM[c]));
        sv = vmax(sv, band(d1, kDM[c]));
        sv = vmin(sv + pM[c], lim[c]);                                      // (a node beyond M: -inf)
        cuM[c] = sv;
        xE = vmax(xE, sv);
        cuI[c] = vmin(vmax(band(pvM[c], kMI[c]), band(pvI[c], kII[c])) + pI[c], lim[c]);
        const float cst = vmin(band(sv, kMD[c]), lim[c]);                   // f_node(x) = max(cst, DD ? x : 0); beyond M: the identity (cst = -inf, pass)
        const float g = vmax(cst, npz[c]);                                  // pass ? cst : max(cst, 0)
        fc = vmax(g, vmin(fc, plim[c]));                                    // pass ? max(g, fc) : g -- f_node o (what the lane has so far)
        fpass &= kDD[c] | ~vm[c];
      }
      // inclusive scan of the lanes' functions, then the value entering each lane: D(first node of the lane)
      // by DPP; lanes without a source see the identity function (c = -inf, pass): max and select only, any scan order gives the same
      float sc_c = fc; int sc_p = fpass ? 1 : 0;
#define BATH_OAS_STEP(CTRL, MASK) { const float oc = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000, __builtin_bit_cast(int, sc_c), CTRL, MASK, 0xf, false)); \
                                    const int op = __builtin_amdgcn_update_dpp(1, sc_p, CTRL, MASK, 0xf, false); \
                                    if (sc_p) { sc_c = fmaxf(sc_c, oc); sc_p = op; } }
      BATH_OAS_STEP(0x111, 0xf) BATH_OAS_STEP(0x112, 0xf) BATH_OAS_STEP(0x114, 0xf) BATH_OAS_STEP(0x118, 0xf) BATH_OAS_STEP(0x142, 0xa) BATH_OAS_STEP(0x143, 0xc)
#undef BATH_OAS_STEP
      float din = wave_shr1_f32(sc_c, -INFINITY);                           // prefix over lanes 0..lane-1 applied to D(1) = -inf
#pragma unroll
      for (int c = 0; c < C; c++) {
        cuD[c] = vmin(din, lim[c]);
        xE = vmax(xE, cuD[c]);
        din = vmax(band(cuM[c], kMD[c]), band(din, kDD[c]));
        pvM[c] = cuM[c]; pvI[c] = cuI[c]; pvD[c] = cuD[c];
      }
      // the row's posteriors over Backward's, its OA cells over Forward's: a lane whose C nodes all exist stores them without a test
      if (full) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          float *bq = brow + (size_t)(lane * C + 1) * 3 + 3 * c, *fq = frow + (size_t)(lane * C + 1) * 3 + 3 * c;
          bq[cM] = pM[c]; bq[cD] = 0.0f; bq[cI] = pI[c];
          fq[cM] = cuM[c]; fq[cD] = cuD[c]; fq[cI] = cuI[c];
        }
      } else if (partial) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int node = lane * C + c + 1;
          if (node <= M) {
            brow[(size_t)node * 3 + cM] = pM[c]; brow[(size_t)node * 3 + cI] = pI[c]; brow[(size_t)node * 3 + cD] = 0.0f;
            frow[(size_t)node * 3 + cM] = cuM[c]; frow[(size_t)node * 3 + cD] = cuD[c]; frow[(size_t)node * 3 + cI] = cuI[c];
          }
        }
      }
      xE = wave_max_f32(xE);
      oxJ = fmaxf(oxJ + pxJ, 0.0f);
      oxC = fmaxf(oxC + pxC, xE);
      oxN = oxN + pxN;
      oxB = fmaxf(oxN, oxJ);
      if (lane == 0) {
        frow[0] = frow[1] = frow[2] = -INFINITY;
        float *px = PX + (size_t)i * 5, *ox = OX + (size_t)i * 5;
        px[XE] = 0.f; px[XN] = pxN; px[XJ] = pxJ; px[XB] = 0.f; px[XC] = pxC;
        ox[XE] = xE; ox[XN] = oxN; ox[XJ] = oxJ; ox[XB] = oxB; ox[XC] = oxC;
      }
    }
    StdEnvOut r{-1, -1, -1, -1, 0, 0.f, 0.f, 0, 0};
    if (!isinf(scaleproduct)) {                                             // else eslERANGE: the domain is dropped
      // p7_Null2_ByExpectation and the correction over the envelope
      const float norm = (float)(1.0 / (double)(float)L);
#pragma unroll
      for (int c = 0; c < C; c++) { emM[c] *= norm; emI[c] *= norm; }
      const float xfactor = sN * norm + sC * norm + sJ * norm;
      float null2[kKp];
      for (int x = 0; x < 20; x++) {
        const float *e = rf + (size_t)x * (M + 1);
        float sv = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) { const int node = lane * C + c + 1; if (node <= M) { sv += emM[c] * e[node]; sv += emI[c]; } }
        null2[x] = wave_sum_f32(sv) + xfactor;
      }
      const int mem[6][2] = {{2, 11}, {7, 9}, {3, 13}, {8, 8}, {1, 1}, {-1, -1}};      // B=DN J=IL Z=EQ O=K U=C X=any
      for (int dx = 0; dx < 6; dx++) {
        float sum = 0.f; int cnt = 0;
        if (dx == 5) { for (int y = 0; y < 20; y++) { sum += null2[y]; cnt++; } }
        else { const int a = min(mem[dx][0], mem[dx][1]), b = max(mem[dx][0], mem[dx][1]); sum += null2[a]; cnt++; if (b != a) { sum += null2[b]; cnt++; } }
        null2[21 + dx] = sum / (float)cnt;
      }
      null2[20] = 1.0f; null2[27] = 1.0f; null2[28] = 1.0f;
      if (null2_out && lane == 0)
#pragma unroll
        for (int x = 0; x < kKp; x++) null2_out[(size_t)t * kKp + x] = null2[x];
      float corr = 0.f;
      for (int pos = 1 + lane; pos <= L; pos += 64) {
        const int x = min((int)dsq[pos], kKp - 1);
        float v = null2[0];
#pragma unroll
        for (int q = 1; q < kKp; q++) v = (x == q) ? null2[q] : v;          // registers cannot be indexed: select
        corr += logf(v);
      }
      r.domcorrection = wave_sum_f32(corr);
      r.oasc = oxC;
      r.ok = 1;
    }
    if (lane == 0) out[t] = r;
  }
}

// The same fill with a BLOCK of four waves per envelope (round 5): models beyond 192 nodes, where a single wave holds 4-16 nodes per
// lane and a row is hundreds of instructions that one wave issues one every ~5 cycles.  Wave w owns nodes 64 w C + 1 .. 64 (w+1) C
// (C = 1, 2, 4: up to 1024 nodes), a lane C consecutive nodes as before.  What crosses a wave boundary goes through LDS: the
// previous row's last cells of wave w - 1 (M, I, D of the node to the left), the waves' composite D-chain functions (wave w applies
// those of waves 0 .. w - 1 to D(1) = -inf before its own lanes' prefixes) and the waves' row maxima for xE -- which no cell of the
// next row reads (unihit: B comes from N and J, and J does not read E), so wave 0 folds them into C and the special-state rows one
// row late.  Two LDS-only barriers per row.  max / select / AND arithmetic as in the one-wave kernel: the same OA matrix,
// posteriors and special rows bit for bit; only null2's sums over the nodes and the residues associate by wave (as they already
// differ between the one-wave kernel and the serial one).
template <int C>
__global__ __launch_bounds__(256) void std_envelope_fill_mw_kernel(SeqView sq, int M, const float *__restrict__ tf, const float *__restrict__ rf, float *__restrict__ fwd,
                                                                   float *__restrict__ bck, const int64_t *__restrict__ dp_off, const float *__restrict__ fx,
                                                                   const float *__restrict__ bx, const int64_t *__restrict__ x_off, float *__restrict__ ppx_all,
                                                                   float *__restrict__ oax_all, StdEnvOut *__restrict__ out,
                                                                   float *__restrict__ null2_out /* optional [n][Kp]: the null2 vector itself */) {
  enum { XE = 0, XN, XJ, XB, XC, XS };
  enum { cM = 0, cD = 1, cI = 2 };
  enum { MM = 0, IM, DM, BM, MD, DD, MI, II };
  constexpr int NW = 4;
  __shared__ float s_nbr[2][NW][3];        // [row parity][wave]: M, I, D of the wave's last node
  __shared__ float s_fc[NW];
  __shared__ int s_fp[NW];
  __shared__ float s_xe[2][NW];            // [row parity][wave]: the wave's maximum over the row's M and D cells
  __shared__ float s_sum[NW][20];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = wv * 64 + lane;                                              // the lane's rank among the block's 256
  auto lds_barrier = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); };
  auto band = [](float v, unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); };
  auto vmax = [](float x, float y) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
  auto vmin = [](float x, float y) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
  unsigned kBM[C], kMM[C], kIM[C], kDM[C], kMD[C], kDD[C], kMI[C], kII[C], vm[C];
  float lim[C], npz[C], plim[C];
  const bool full = gl * C + C <= M, partial = !full && gl * C + 1 <= M;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const int node = gl * C + c + 1;
    const bool ok = node <= M;
    const float *tq = tf + (size_t)min(node, M) * 8;
    auto mk = [&](int q) { return (ok && tq[q] > 0.0f) ? 0xffffffffu : 0u; };
    kMM[c] = mk(MM); kIM[c] = mk(IM); kDM[c] = mk(DM); kBM[c] = mk(BM); kMD[c] = mk(MD); kDD[c] = mk(DD); kMI[c] = mk(MI); kII[c] = mk(II);
    vm[c] = ok ? 0xffffffffu : 0u;
    lim[c] = ok ? INFINITY : -INFINITY;
    const bool pass = !ok || tq[DD] > 0.0f;
    npz[c] = pass ? -INFINITY : 0.0f;
    plim[c] = pass ? INFINITY : -INFINITY;
  }
  for (int64_t t = blockIdx.x; t < sq.n; t += gridDim.x) {
    const int L = sq.len[t];
    const uint8_t *dsq = sq.data + sq.off[t] - 1;
    const size_t W = (size_t)(M + 1) * 3;
    float *F = fwd + dp_off[t];
    float *Bk = bck + dp_off[t];
    const float *FX = fx + x_off[t], *BX = bx + x_off[t];
    float *PX = ppx_all + (x_off[t] / 6) * 5, *OX = oax_all + (x_off[t] / 6) * 5;
    const float ploop = 1.0f - 2.0f / ((float)L + 2.0f);
    float pvM[C], pvI[C], pvD[C], emM[C], emI[C];
#pragma unroll
    for (int c = 0; c < C; c++) { pvM[c] = pvI[c] = pvD[c] = -INFINITY; emM[c] = emI[c] = 0.f; }
    float oxN = 0.f, oxJ = -INFINITY, oxC = -INFINITY, oxB = 0.f, sN = 0.f, sC = 0.f, sJ = 0.f;
    float scaleproduct = (float)(1.0 / (double)BX[XN]);
    for (int k = threadIdx.x; k <= M; k += blockDim.x) F[(size_t)k * 3] = F[(size_t)k * 3 + 1] = F[(size_t)k * 3 + 2] = -INFINITY;      // OA row 0
    if (threadIdx.x == 0) {
      for (int q = 0; q < 5; q++) PX[q] = 0.f;
      OX[XE] = -INFINITY; OX[XN] = 0.f; OX[XJ] = -INFINITY; OX[XB] = 0.f; OX[XC] = -INFINITY;
    }
    if (lane == 63) { s_nbr[0][wv][0] = s_nbr[0][wv][1] = s_nbr[0][wv][2] = -INFINITY; }          // "row 0" as row 1 reads it
    float fM[C], fI[C], bM[C], bI[C];
    const size_t lane0 = (size_t)(gl * C + 1) * 3;
    auto fetch_row = [&](int r) {
      const float *fq = F + (size_t)r * W + lane0, *bq = Bk + (size_t)r * W + lane0;
#pragma unroll
      for (int c = 0; c < C; c++) { fM[c] = fq[3 * c + cM]; fI[c] = fq[3 * c + cI]; bM[c] = bq[3 * c + cM]; bI[c] = bq[3 * c + cI]; }
    };
    float xb[8], xn[8];
    auto fetch_x = [&](int r0, float (&v)[8]) {                             // rows r0 .. r0 + 63, a lane each (every wave its own copy)
      const int r = min(r0 + lane, L);
      v[0] = FX[(size_t)(r - 1) * 6 + XN]; v[1] = FX[(size_t)(r - 1) * 6 + XJ]; v[2] = FX[(size_t)(r - 1) * 6 + XC]; v[3] = FX[(size_t)r * 6 + XS];
      v[4] = BX[(size_t)r * 6 + XN]; v[5] = BX[(size_t)r * 6 + XJ]; v[6] = BX[(size_t)r * 6 + XC]; v[7] = BX[(size_t)r * 6 + XS];
    };
    if (L >= 1) { fetch_row(1); fetch_x(1, xb); }
    float pxN_prev = 0.f, pxJ_prev = 0.f, pxC_prev = 0.f;
    // wave 0: C and the special-state rows of row r, once the waves' maxima of that row have crossed the barrier that ended it
    // (oxN, oxJ, oxB still hold row r's values then: they are advanced at the end of the next row)
    auto finish_row = [&](int r) {
      float xE = s_xe[r & 1][0];
#pragma unroll
      for (int w = 1; w < NW; w++) xE = vmax(xE, s_xe[r & 1][w]);
      oxC = fmaxf(oxC + pxC_prev, xE);
      if (lane == 0) {
        float *px = PX + (size_t)r * 5, *ox = OX + (size_t)r * 5;
        px[XE] = 0.f; px[XN] = pxN_prev; px[XJ] = pxJ_prev; px[XB] = 0.f; px[XC] = pxC_prev;
        ox[XE] = xE; ox[XN] = oxN; ox[XJ] = oxJ; ox[XB] = oxB; ox[XC] = oxC;
      }
    };
    lds_barrier();
    for (int i = 1; i <= L; i++) {
      const int par = i & 1;
      const int j = (i - 1) & 63;
      if (j == 0 && i + 64 <= L) fetch_x(i + 64, xn);
      float xv[8];
#pragma unroll
      for (int q = 0; q < 8; q++) xv[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xb[q]), j));
      if (j == 63) {
#pragma unroll
        for (int q = 0; q < 8; q++) xb[q] = xn[q];
      }
      const float totr = scaleproduct * xv[3];
      float *frow = F + (size_t)i * W;
      float *brow = Bk + (size_t)i * W;
      float pM[C], pI[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        pM[c] = band(fM[c] * (bM[c] * totr), vm[c]);
        pI[c] = band(fI[c] * (bI[c] * totr), vm[c]);
        if (i == 1) { emM[c] = pM[c]; emI[c] = pI[c]; } else { emM[c] = pM[c] + emM[c]; emI[c] = pI[c] + emI[c]; }
      }
      if (i < L) fetch_row(i + 1);
      const float pxN = xv[0] * xv[4] * ploop * scaleproduct;
      const float pxJ = xv[1] * xv[5] * ploop * scaleproduct;
      const float pxC = xv[2] * xv[6] * ploop * scaleproduct;
      if (i == 1) { sN = pxN; sC = pxC; sJ = pxJ; } else { sN += pxN; sC += pxC; sJ += pxJ; }
      scaleproduct *= xv[3] / xv[7];
      float mIn = wave_shr1_f32(pvM[C - 1], -INFINITY), iIn = wave_shr1_f32(pvI[C - 1], -INFINITY), dIn = wave_shr1_f32(pvD[C - 1], -INFINITY);
      if (lane == 0 && wv > 0) { mIn = s_nbr[par ^ 1][wv - 1][0]; iIn = s_nbr[par ^ 1][wv - 1][1]; dIn = s_nbr[par ^ 1][wv - 1][2]; }
      float cuM[C], cuI[C], cuD[C];
      float fc = -INFINITY; unsigned fpass = 0xffffffffu;
      float xE = -INFINITY;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const float m1 = c == 0 ? mIn : pvM[c - 1], i1 = c == 0 ? iIn : pvI[c - 1], d1 = c == 0 ? dIn : pvD[c - 1];
        float sv = band(oxB, kBM[c]);
        sv = vmax(sv, band(m1, kMM[c]));
        sv = vmax(sv, band(i1, kIM[c]));
        sv = vmax(sv, band(d1, kDM[c]));
        sv = vmin(sv + pM[c], lim[c]);
        cuM[c] = sv;
        xE = vmax(xE, sv);
        cuI[c] = vmin(vmax(band(pvM[c], kMI[c]), band(pvI[c], kII[c])) + pI[c], lim[c]);
        const float cst = vmin(band(sv, kMD[c]), lim[c]);
        const float g = vmax(cst, npz[c]);
        fc = vmax(g, vmin(fc, plim[c]));
        fpass &= kDD[c] | ~vm[c];
      }
      float sc_c = fc; int sc_p = fpass ? 1 : 0;
#define BATH_OAS_STEP(CTRL, MASK) { const float oc = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000, __builtin_bit_cast(int, sc_c), CTRL, MASK, 0xf, false)); \
                                    const int op = __builtin_amdgcn_update_dpp(1, sc_p, CTRL, MASK, 0xf, false); \
                                    if (sc_p) { sc_c = fmaxf(sc_c, oc); sc_p = op; } }
      BATH_OAS_STEP(0x111, 0xf) BATH_OAS_STEP(0x112, 0xf) BATH_OAS_STEP(0x114, 0xf) BATH_OAS_STEP(0x118, 0xf) BATH_OAS_STEP(0x142, 0xa) BATH_OAS_STEP(0x143, 0xc)
#undef BATH_OAS_STEP
      if (lane == 63) { s_fc[wv] = sc_c; s_fp[wv] = sc_p; }                   // the wave's composite function
      if (wv == 0 && i > 1) finish_row(i - 1);                                // (row i - 1's maxima are behind the barrier that ended it)
      lds_barrier();                                                           // ---- barrier 1: the waves' functions of this row
      float xin = -INFINITY;                                                   // D entering this wave: the waves before it applied to D(1) = -inf
      for (int w = 0; w < wv; w++) xin = s_fp[w] ? vmax(s_fc[w], xin) : s_fc[w];
      const float ec = wave_shr1_f32(sc_c, -INFINITY);                         // exclusive prefix of this wave's lanes (lane 0: the identity)
      int ep = __builtin_amdgcn_update_dpp(1, sc_p, 0x138, 0xf, 0xf, false);   // wave_shr:1
      if (lane == 0) ep = 1;
      float din = ep ? vmax(ec, xin) : ec;
#pragma unroll
      for (int c = 0; c < C; c++) {
        cuD[c] = vmin(din, lim[c]);
        xE = vmax(xE, cuD[c]);
        din = vmax(band(cuM[c], kMD[c]), band(din, kDD[c]));
        pvM[c] = cuM[c]; pvI[c] = cuI[c]; pvD[c] = cuD[c];
      }
      if (full) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          float *bq = brow + lane0 + 3 * c, *fq = frow + lane0 + 3 * c;
          bq[cM] = pM[c]; bq[cD] = 0.0f; bq[cI] = pI[c];
          fq[cM] = cuM[c]; fq[cD] = cuD[c]; fq[cI] = cuI[c];
        }
      } else if (partial) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int node = gl * C + c + 1;
          if (node <= M) {
            brow[(size_t)node * 3 + cM] = pM[c]; brow[(size_t)node * 3 + cI] = pI[c]; brow[(size_t)node * 3 + cD] = 0.0f;
            frow[(size_t)node * 3 + cM] = cuM[c]; frow[(size_t)node * 3 + cD] = cuD[c]; frow[(size_t)node * 3 + cI] = cuI[c];
          }
        }
      }
      if (threadIdx.x == 0) { frow[0] = frow[1] = frow[2] = -INFINITY; }
      xE = wave_max_f32(xE);
      if (lane == 63) { s_nbr[par][wv][0] = pvM[C - 1]; s_nbr[par][wv][1] = pvI[C - 1]; s_nbr[par][wv][2] = pvD[C - 1]; s_xe[par][wv] = xE; }
      // N, J and B of this row (every wave its own copy: none of them reads E); C waits for xE (finish_row, one row late)
      oxJ = fmaxf(oxJ + pxJ, 0.0f);
      oxN = oxN + pxN;
      oxB = fmaxf(oxN, oxJ);
      pxN_prev = pxN; pxJ_prev = pxJ; pxC_prev = pxC;
      lds_barrier();                                                           // ---- barrier 2: neighbours and maxima of row i
    }
    if (wv == 0 && L >= 1) finish_row(L);
    // oasc = C(L) lives in wave 0: hand it to everybody with the null2 sums below
    StdEnvOut r{-1, -1, -1, -1, 0, 0.f, 0.f, 0, 0};
    if (!isinf(scaleproduct)) {                                             // else eslERANGE: the domain is dropped
      const float norm = (float)(1.0 / (double)(float)L);
#pragma unroll
      for (int c = 0; c < C; c++) { emM[c] *= norm; emI[c] *= norm; }
      const float xfactor = sN * norm + sC * norm + sJ * norm;
      float null2[kKp];
      for (int x = 0; x < 20; x++) {
        const float *e = rf + (size_t)x * (M + 1);
        float sv = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) { const int node = gl * C + c + 1; if (node <= M) { sv += emM[c] * e[node]; sv += emI[c]; } }
        const float ws = wave_sum_f32(sv);
        if (lane == 0) s_sum[wv][x] = ws;
      }
      lds_barrier();
      for (int x = 0; x < 20; x++) null2[x] = (((s_sum[0][x] + s_sum[1][x]) + s_sum[2][x]) + s_sum[3][x]) + xfactor;
      lds_barrier();
      const int mem[6][2] = {{2, 11}, {7, 9}, {3, 13}, {8, 8}, {1, 1}, {-1, -1}};      // B=DN J=IL Z=EQ O=K U=C X=any
      for (int dx = 0; dx < 6; dx++) {
        float sum = 0.f; int cnt = 0;
        if (dx == 5) { for (int y = 0; y < 20; y++) { sum += null2[y]; cnt++; } }
        else { const int a = min(mem[dx][0], mem[dx][1]), b = max(mem[dx][0], mem[dx][1]); sum += null2[a]; cnt++; if (b != a) { sum += null2[b]; cnt++; } }
        null2[21 + dx] = sum / (float)cnt;
      }
      null2[20] = 1.0f; null2[27] = 1.0f; null2[28] = 1.0f;
      if (null2_out && threadIdx.x == 0)
#pragma unroll
        for (int x = 0; x < kKp; x++) null2_out[(size_t)t * kKp + x] = null2[x];
      float corr = 0.f;
      for (int pos = 1 + (int)threadIdx.x; pos <= L; pos += (int)blockDim.x) {
        const int x = min((int)dsq[pos], kKp - 1);
        float v = null2[0];
#pragma unroll
        for (int q = 1; q < kKp; q++) v = (x == q) ? null2[q] : v;
        corr += logf(v);
      }
      const float wc = wave_sum_f32(corr);
      if (lane == 0) s_sum[wv][0] = wc;
      lds_barrier();
      r.domcorrection = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0];
      r.oasc = oxC;                                                         // (wave 0's: the only reader is thread 0 below)
      r.ok = 1;
    }
    if (threadIdx.x == 0) out[t] = r;
    lds_barrier();                                                          // the LDS slots are the next envelope's
  }
}

}  // namespace

namespace {

// Where target i of a batch lies in the kernels' buffers: its special-state rows, (len + 1) x 6 floats from x[i], and its
// matrix, (len + 1) x (M + 1) x 3 floats from dp[i]; x[n] and dp[n] are the totals.
struct BlockOffsets { std::vector<int64_t> x, dp; };
BlockOffsets block_offsets(const bath_hip_seqs *sq, int M) {
  BlockOffsets o;
  o.x.assign((size_t)sq->n + 1, 0); o.dp.assign((size_t)sq->n + 1, 0);
  for (int64_t i = 0; i < sq->n; i++) {
    o.x[(size_t)i + 1] = o.x[(size_t)i] + ((int64_t)sq->h_len[(size_t)i] + 1) * 6;
    o.dp[(size_t)i + 1] = o.dp[(size_t)i] + ((int64_t)sq->h_len[(size_t)i] + 1) * (M + 1) * 3;
  }
  return o;
}

// Stretches of a residue pool as a sequence view: a borrowed one (is_part, bath_common.hpp) that lives on the stack; its device
// arrays come with StdStaging::upload_view.
bath_hip_seqs part_view(bath_hip_ctx *ctx, std::vector<int64_t> off, std::vector<int32_t> len) {
  bath_hip_seqs v;
  v.ctx = ctx; v.n = (int64_t)off.size(); v.is_part = true;
  v.h_off = std::move(off); v.h_len = std::move(len);
  for (int32_t l : v.h_len) v.maxlen = std::max(v.maxlen, l);
  return v;
}

// The buffers of the envelope kernels for the <n> envelopes that <o> places: both matrices (with the slack the fill kernels read
// past the last node), both parsers' rows, the posterior and optimal-accuracy rows, null2's work area and the kernels' records.
int std_reserve_envelope_buffers(bath_hip_ctx *ctx, const BlockOffsets &o, int64_t n, int M) {
  const size_t nx = (size_t)o.x[(size_t)n], ndp = (size_t)o.dp[(size_t)n];
  auto &s = ctx->scratch;
  BATH_HIP_TRY(ctx, s[Scratch::kEnvFwdMatrix].reserve(ndp * 4 + 64 + kStdFillSlack)); BATH_HIP_TRY(ctx, s[Scratch::kEnvBwdMatrix].reserve(ndp * 4 + 64 + kStdFillSlack));
  BATH_HIP_TRY(ctx, s[Scratch::kStdFwdRows].reserve(nx * 4 + 64)); BATH_HIP_TRY(ctx, s[Scratch::kStdBwdRows].reserve(nx * 4 + 64));
  BATH_HIP_TRY(ctx, s[Scratch::kStdPosteriorRows].reserve(nx / 6 * 5 * 4 + 64)); BATH_HIP_TRY(ctx, s[Scratch::kStdOaRows].reserve(nx / 6 * 5 * 4 + 64));
  BATH_HIP_TRY(ctx, s[Scratch::kEnvNull2Work].reserve((size_t)n * 2 * (M + 1) * 4 + 64)); BATH_HIP_TRY(ctx, s[Scratch::kStdEnvOut].reserve((size_t)n * sizeof(StdEnvOut) + 64));
  return BATH_OK;
}

}  // namespace

// The multi-domain regions of a batch: p7_Forward of every region in the multihit configuration of length cfg[e] (full matrix),
// then its stochastic-trace ensemble in the context's bath_hip_set_std_ensemble mode; per region the clusters' envelopes
// (region coordinates) with their null2 corrections (null2_is_done: p7_domaindef.c:1270-1272).  <v> and the d_ arrays are on the
// device already.  Modes 0 and 1: the kernel writes matrices, special-state rows and residues straight into page-locked host memory,
// the transfer rides along with the computation, and host threads walk.  Mode 2: the matrices and rows stay in device memory,
// std_ensemble_kernel walks behind the Forward kernel on the same stream, and the host gets statuses, segments and path codes.
struct StdRegionOut { int status = 0; std::vector<std::pair<int, int>> env; std::vector<float> corr; std::vector<int32_t> segs, trace_status; };
static int std_region_stage(bath_hip_ctx *ctx, const bath_hip_oprofile *om, SeqView v, int64_t nm, const int32_t *h_len, const std::vector<int32_t> &cfg,
                            const std::vector<int64_t> &mxoff, const std::vector<int64_t> &mdpoff, const int64_t *d_xoff, const int64_t *d_dpoff,
                            const int32_t *d_cfg, uint32_t seed, bool detail, std::vector<StdRegionOut> *out, StageClock &clk) {
  int st;
  const int mode = ctx->std_ensemble;
  const bool dev = mode == BATH_ENSEMBLE_STREAMS_DEVICE;
  out->assign((size_t)nm, StdRegionOut{});
  DevBuf &b_fx = ctx->scratch[Scratch::kStdFwdRows], &b_sc = ctx->scratch[Scratch::kStdScores], &b_st = ctx->scratch[Scratch::kStdStatus], &b_dp = ctx->scratch[Scratch::kStdRegionFwdMatrix];
  BATH_HIP_TRY(ctx, b_fx.reserve((size_t)mxoff[(size_t)nm] * 4 + 64)); BATH_HIP_TRY(ctx, b_sc.reserve((size_t)nm * 8)); BATH_HIP_TRY(ctx, b_st.reserve((size_t)nm * 8));
  // Residues of region e: h_res + roff[e], one row's worth of bytes per residue row (roff = the x-row offsets / 6).
  const size_t x_bytes = ((size_t)mxoff[(size_t)nm] * 4 + 255) / 256 * 256;
  if (dev) BATH_HIP_TRY(ctx, b_dp.reserve((size_t)mdpoff[(size_t)nm] * 4 + 64)); else BATH_HIP_TRY(ctx, ctx->stage[Pinned::kStdRegionMatrices].reserve((size_t)mdpoff[(size_t)nm] * 4 + 64));
  BATH_HIP_TRY(ctx, ctx->stage[Pinned::kStdRegionRows].reserve(x_bytes + (size_t)mxoff[(size_t)nm] / 6 + 64));
  float *h_dp = ctx->stage[Pinned::kStdRegionMatrices].as<float>(), *h_x = ctx->stage[Pinned::kStdRegionRows].as<float>();      // page-locked
  const uint8_t *h_res = reinterpret_cast<const uint8_t *>(ctx->stage[Pinned::kStdRegionRows].p) + x_bytes;
  std::vector<int64_t> roff((size_t)nm + 1, 0);
  for (int64_t e = 0; e <= nm; e++) roff[(size_t)e] = mxoff[(size_t)e] / 6;
  void *dv_dp = nullptr, *dv_x = nullptr;
  if ((!dev && hipHostGetDevicePointer(&dv_dp, ctx->stage[Pinned::kStdRegionMatrices].p, 0) != hipSuccess) || hipHostGetDevicePointer(&dv_x, ctx->stage[Pinned::kStdRegionRows].p, 0) != hipSuccess) {
    ctx->set_error("page-locked host memory is not mapped into the device's address space"); return BATH_EFAIL;
  }
  float *dst_x = dev ? b_fx.as<float>() : static_cast<float *>(dv_x), *dst_dp = dev ? b_dp.as<float>() : static_cast<float *>(dv_dp);
  if ((st = launch_fwd_wave(ctx, om, v, nullptr, nm, b_sc.as<float>(), b_st.as<int32_t>(), nullptr, dst_x, d_xoff, dst_dp, d_dpoff, 0, d_cfg)) != BATH_OK) return st;
  hipLaunchKernelGGL(gather_residues_kernel, dim3((unsigned)std::min<int64_t>(nm, 4096)), dim3(64), 0, ctx->stream, v, d_xoff, static_cast<uint8_t *>(dv_x) + x_bytes);
  BATH_HIP_TRY(ctx, hipGetLastError());
  StdEnsRun run;
  if (dev && (st = std_region_ensembles_device(ctx, om, nm, h_len, v.len, d_cfg, dst_dp, d_dpoff, dst_x, d_xoff, seed, &run)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  clk.lap(dev ? "std:   region Forward + ensemble kernel" : "std:   region Forward + copy to host");
  // the regions are independent (each ensemble starts from the seed): host threads take them round-robin, results are
  // kept in region order
  if (om->ensure_len_tables(*std::max_element(cfg.begin(), cfg.end())) != BATH_OK) return BATH_EFAIL;
  std::atomic<int> rc{BATH_OK};
  auto work = [&](int64_t first, int64_t step) {
    std::vector<float> n2sc;
    std::vector<std::pair<int, int>> cl;
    for (int64_t e = first; e < nm; e += step) {
      StdRegionOut &o = (*out)[(size_t)e];
      const int Lr = h_len[e];
      const StdEnsModel m = std_ens_model(om, cfg[(size_t)e]);
      if (detail) o.trace_status.assign(kEnsSamples, 0);
      int rs = 0, r;
      if (dev) r = std_ensemble_region_from_device(ctx, run, e, m, h_res + roff[(size_t)e], Lr, mdpoff[(size_t)e], mxoff[(size_t)e], seed, &n2sc, &cl, &rs,
                                                   detail ? &o.segs : nullptr, detail ? o.trace_status.data() : nullptr);
      else r = std_region_ensemble_host(ctx, mode, m, h_res + roff[(size_t)e], Lr, h_dp + mdpoff[(size_t)e], h_x + mxoff[(size_t)e], &n2sc, &cl, seed, &rs,
                                        detail ? &o.segs : nullptr, detail ? o.trace_status.data() : nullptr);
      if (r != BATH_OK) { rc = r; continue; }
      o.status = rs;
      if (rs != kEnsRegionOk) continue;                     // a failed ensemble: the region has no envelopes
      for (const auto &c : cl) {
        float corr = 0.f;
        for (int pos = c.first; pos <= c.second; pos++) corr += n2sc[(size_t)pos];     // null2_is_done: p7_domaindef.c:1270-1272
        o.env.push_back(c); o.corr.push_back(corr);
      }
    }
  };
  run_striped(nm, work, [&](int64_t e) { return h_len[e]; });
  if (rc.load() != BATH_OK) { ctx->set_error("a multi-domain region's ensemble failed (a copy from the device, or records that do not add up)"); return rc.load(); }
  clk.lap(dev ? "std:   ensembles (null2 + clustering, host threads)" : "std:   ensembles (host threads)");
  return BATH_OK;
}

// The fill kernel std_domains runs before the traceback: 0 none (std_envelope_kernel does everything, a lane per envelope:
// BATH_HIP_STD_SERIAL=1, or a model beyond the fill kernels' 1024 nodes), 1 a wave per envelope, 2 a block of four waves per
// envelope -- from 4 nodes per lane on (BATH_HIP_STD_FILL_MW=0: never, =1: for every model).
static int std_fill_choice(int M) {
  const char *e = std::getenv("BATH_HIP_STD_SERIAL");
  if ((e && e[0] == '1') || !(M <= 1024)) return 0;
  const int c = (M + 63) / 64;
  const char *mwe = std::getenv("BATH_HIP_STD_FILL_MW");
  return (mwe ? mwe[0] == '1' : c >= 4) ? 2 : 1;
}

// Launches std_envelope_fill_kernel<C> (fill == 1) or std_envelope_fill_mw_kernel<C> (fill == 2) for a model of M nodes over <ne>
// envelopes: the one place where a model length picks an instantiation of either (tests/test_tiling_coverage_cpu.py reads it).
static int std_launch_fill(bath_hip_ctx *ctx, int M, int fill, SeqView v, int64_t ne, const float *tf, const float *rf, float *f, float *b, const int64_t *dpo,
                           const float *fx, const float *bx, const int64_t *xoff, float *px, float *ox, StdEnvOut *out, float *null2_out) {
  if (M > 1024 || (fill != 1 && fill != 2)) { ctx->set_error("the standard branch's fill kernels take models of up to 1024 nodes"); return BATH_ERANGE; }
  if (fill == 2) {
    const unsigned mgrid = (unsigned)std::min<int64_t>(ne, (int64_t)ctx->prop.multiProcessorCount * 8);
#define BATH_FILL_MW(CC) hipLaunchKernelGGL(std_envelope_fill_mw_kernel<CC>, dim3(mgrid), dim3(256), 0, ctx->stream, v, M, tf, rf, f, b, dpo, fx, bx, xoff, px, ox, out, null2_out)
    const int c4 = (M + 255) / 256;
    if (c4 <= 1) { BATH_FILL_MW(1); } else if (c4 <= 2) { BATH_FILL_MW(2); } else { BATH_FILL_MW(4); }
#undef BATH_FILL_MW
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>((ne + 3) / 4, (int64_t)ctx->prop.multiProcessorCount * 8);
#define BATH_FILL(CC) hipLaunchKernelGGL(std_envelope_fill_kernel<CC>, dim3(grid), dim3(256), 0, ctx->stream, v, M, tf, rf, f, b, dpo, fx, bx, xoff, px, ox, out, null2_out)
    const int c = (M + 63) / 64;
    if (c <= 1) { BATH_FILL(1); } else if (c <= 2) { BATH_FILL(2); } else if (c <= 3) { BATH_FILL(3); } else if (c <= 4) { BATH_FILL(4); }
    else if (c <= 6) { BATH_FILL(6); } else if (c <= 8) { BATH_FILL(8); } else if (c <= 12) { BATH_FILL(12); } else { BATH_FILL(16); }
#undef BATH_FILL
  }
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// The small transfers of a stage go through page-locked memory (Pinned::kStdUploads, Pinned::kStdDownloads): a hipMemcpyAsync from or to
// pageable memory is staged by the runtime and holds the host ~20 us, and one query's domain stage had two dozen of them -- a
// fifth of its time on a 12.5 Mb block (configs[3]).  up_begin() sizes the staging area for ALL uploads of a stage (it may move
// while nothing is in flight: every stage ends with a synchronize); a sequence view's three arrays travel as ONE copy.
// Downloads: into page-locked memory, then (after the stage's synchronize) a host copy into the vector the code reads.
struct StdStaging {
  bath_hip_ctx *ctx;
  size_t up_used = 0;
  static size_t view_bytes(int64_t n) { return (size_t)n * 12 + (size_t)(n + 1) * 8 + 256; }
  int up_begin(size_t bytes) { up_used = 0; BATH_HIP_TRY(ctx, ctx->stage[Pinned::kStdUploads].reserve(bytes + 1024)); return BATH_OK; }
  int up(void *dst, std::initializer_list<std::pair<const void *, size_t>> parts) {
    size_t bytes = 0;
    for (const auto &q : parts) bytes += q.second;
    const size_t end = up_used + ((bytes + 63) & ~(size_t)63);
    if (end > ctx->stage[Pinned::kStdUploads].cap) { ctx->set_error("staging area of the domain stage too small"); return BATH_EFAIL; }      // before anything is written
    char *h = static_cast<char *>(ctx->stage[Pinned::kStdUploads].p) + up_used;
    bytes = 0;
    for (const auto &q : parts) { std::memcpy(h + bytes, q.first, q.second); bytes += q.second; }
    up_used = end;
    BATH_HIP_TRY(ctx, hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return BATH_OK;
  }
  // The device arrays of a view into <d_pool> (Scratch::kStdViewArrays): its offsets, its targets' row offsets <xo> (*d_xo: where
  // they lie on the device) and its lengths
  int upload_view(bath_hip_seqs &v, const std::vector<int64_t> &xo, const uint8_t *d_pool, const int64_t **d_xo) {
    const int64_t n = v.n;
    DevBuf &b_idx = ctx->scratch[Scratch::kStdViewArrays];
    BATH_HIP_TRY(ctx, b_idx.reserve(view_bytes(n)));
    int64_t *d_off = b_idx.as<int64_t>();
    *d_xo = d_off + n;
    int32_t *d_len = reinterpret_cast<int32_t *>(d_off + n + n + 1);
    const int rc = up(d_off, {{v.h_off.data(), (size_t)n * 8}, {xo.data(), (size_t)(n + 1) * 8}, {v.h_len.data(), (size_t)n * 4}});      // contiguous on the device too
    if (rc != BATH_OK) return rc;
    v.d_data = const_cast<uint8_t *>(d_pool); v.d_off = d_off; v.d_len = d_len;
    return BATH_OK;
  }
  int down_reserve(size_t bytes) { BATH_HIP_TRY(ctx, ctx->stage[Pinned::kStdDownloads].reserve(bytes + 1024)); return BATH_OK; }
};

struct StdEnv { int s, i, j; bool clustered; float n2corr; };      // residues i..j of survivor s; a cluster's envelope comes with its null2 correction
constexpr int kStdRegionStride = 1 + 3 * kStdMaxRegions;           // ints per ORF in the regions kernels' output

// Both parsers' special-state rows for the survivors.  Forward's: the reference has them from the filter (pli->oxf,
// p7_pipeline.c:1741-1771).  When the cascade of this call kept them (ctx->fwd_rows_kept: a one-lane block through
// bath_hip_pipeline_hits) the survivors' rows are copied into place; otherwise (the standard branch of the --fs pipeline, blocks
// cut into lanes, rows that did not fit) the parser runs again.
static int std_parsers(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const std::vector<PipelineSurvivor> &surv, const bath_hip_seqs &view, const BlockOffsets &o,
                       const int64_t *d_xoff, StdStaging &sg) {
  int st;
  const int64_t ns = view.n;
  DevBuf &b_fx = ctx->scratch[Scratch::kStdFwdRows], &b_bx = ctx->scratch[Scratch::kStdBwdRows], &b_sc = ctx->scratch[Scratch::kStdScores], &b_st = ctx->scratch[Scratch::kStdStatus];
  BATH_HIP_TRY(ctx, b_fx.reserve((size_t)o.x[(size_t)ns] * 4 + 64)); BATH_HIP_TRY(ctx, b_bx.reserve((size_t)o.x[(size_t)ns] * 4 + 64));
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)ns * 8)); BATH_HIP_TRY(ctx, b_st.reserve((size_t)ns * 8));
  bool kept = ctx->fwd_rows_kept != nullptr;
  for (int64_t i = 0; i < ns && kept; i++) kept = surv[(size_t)i].fx_off >= 0;
  if (kept) {
    std::vector<int64_t> src((size_t)ns);
    for (int64_t i = 0; i < ns; i++) src[(size_t)i] = surv[(size_t)i].fx_off;
    DevBuf &b_src = ctx->scratch[Scratch::kStdKeptRowSource];
    BATH_HIP_TRY(ctx, b_src.reserve((size_t)ns * 8 + 64));
    if ((st = sg.up(b_src.p, {{src.data(), (size_t)ns * 8}})) != BATH_OK) return st;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)std::min<int64_t>(ns, 65535)), dim3(256), 0, ctx->stream, ns, view.d_len, ctx->fwd_rows_kept, b_src.as<int64_t>(), b_fx.as<float>(), d_xoff);
    BATH_HIP_TRY(ctx, hipGetLastError());
  } else if ((st = launch_fwd_wave(ctx, om, view.view(), nullptr, ns, b_sc.as<float>(), b_st.as<int32_t>(), nullptr, b_fx.as<float>(), d_xoff)) != BATH_OK) return st;
  return launch_bwd_wave(ctx, om, view.view(), ns, b_fx.as<float>(), d_xoff, b_sc.as<float>() + ns, b_st.as<int32_t>() + ns, b_bx.as<float>());
}

// Domain decoding and the region heuristics over the parsers' rows, into Scratch::kStdRegionList ([ns][kStdRegionStride])
static int std_launch_regions(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs &view, const BlockOffsets &o, const int64_t *d_xoff) {
  const int64_t ns = view.n;
  DevBuf &b_fx = ctx->scratch[Scratch::kStdFwdRows], &b_bx = ctx->scratch[Scratch::kStdBwdRows], &b_work = ctx->scratch[Scratch::kStdRegionWork], &b_reg = ctx->scratch[Scratch::kStdRegionList];
  BATH_HIP_TRY(ctx, b_work.reserve((size_t)o.x[(size_t)ns] / 6 * 3 * 4 + 64));
  BATH_HIP_TRY(ctx, b_reg.reserve((size_t)ns * kStdRegionStride * 4 + 64));
  const char *e = std::getenv("BATH_HIP_STD_SERIAL");
  const size_t shm = (size_t)4 * ((size_t)view.maxlen + 1) * sizeof(float);
  if (shm <= (size_t)128 * 1024 && !(e && e[0] == '1')) {                     // a wave per ORF, rows in LDS
    if (shm > 64 * 1024) BATH_HIP_TRY(ctx, bath::allow_max_lds((const void *)std_regions_wave_kernel));
    hipLaunchKernelGGL(std_regions_wave_kernel, dim3((unsigned)std::min<int64_t>(ns, 65535)), dim3(64), shm, ctx->stream, ns, view.d_len, b_fx.as<float>(), b_bx.as<float>(),
                       d_xoff, om->lt.d_pmove, view.maxlen, b_reg.as<int32_t>());
  } else
    hipLaunchKernelGGL(std_regions_kernel, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, ctx->stream, ns, view.d_len, b_fx.as<float>(), b_bx.as<float>(), d_xoff, om->lt.d_pmove,
                       b_work.as<float>(), b_reg.as<int32_t>());
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// Stage (a): the survivors as a sequence view into the amino-acid streams, both parsers, the regions kernel; the regions come
// back as envelopes (single-domain regions) and multi-domain regions
static int std_stage_regions(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const std::vector<PipelineSurvivor> &surv, const uint8_t *d_pool, StdStaging &sg,
                             std::vector<StdEnv> *envs, std::vector<StdEnv> *mregs) {
  int st;
  const int64_t ns = (int64_t)surv.size();
  std::vector<int64_t> off((size_t)ns);
  std::vector<int32_t> len((size_t)ns);
  for (int64_t i = 0; i < ns; i++) { off[(size_t)i] = surv[(size_t)i].aa_off; len[(size_t)i] = surv[(size_t)i].n; }
  bath_hip_seqs view = part_view(ctx, std::move(off), std::move(len));
  const BlockOffsets o = block_offsets(&view, om->M);
  if ((st = om->ensure_len_tables(view.maxlen)) != BATH_OK) return st;
  if ((st = sg.up_begin(StdStaging::view_bytes(ns) + (size_t)ns * 8 + 256)) != BATH_OK) return st;                 // (+ the kept Forward rows' offsets, std_parsers)
  const int64_t *d_xoff = nullptr;
  if ((st = sg.upload_view(view, o.x, d_pool, &d_xoff)) != BATH_OK) return st;
  if ((st = std_parsers(ctx, om, surv, view, o, d_xoff, sg)) != BATH_OK) return st;
  if ((st = std_launch_regions(ctx, om, view, o, d_xoff)) != BATH_OK) return st;
  std::vector<int32_t> regions((size_t)ns * kStdRegionStride);
  if ((st = sg.down_reserve(regions.size() * 4)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kStdDownloads].p, ctx->scratch[Scratch::kStdRegionList].p, regions.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(regions.data(), ctx->stage[Pinned::kStdDownloads].p, regions.size() * 4);
  for (int64_t q = 0; q < ns; q++) {
    const int32_t *r = &regions[(size_t)q * kStdRegionStride];
    if (r[0] > kStdMaxRegions) { ctx->set_error("an ORF has more regions than the region buffer holds"); return BATH_ERANGE; }
    for (int k = 0; k < r[0]; k++) (r[3 + 3 * k] ? mregs : envs)->push_back(StdEnv{(int)q, r[1 + 3 * k], r[2 + 3 * k], false, 0.f});
  }
  return BATH_OK;
}

// Stage (b): the multi-domain regions (p7_domaindef.c:539-583): p7_Forward of the region with the ORF's multihit configuration on
// the GPU, then the stochastic-trace ensemble and its clustering (std_region_stage); every cluster is one more envelope
static int std_stage_multidomain(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const std::vector<PipelineSurvivor> &surv, const uint8_t *d_pool, StdStaging &sg,
                                 const std::vector<StdEnv> &mregs, uint32_t seed, std::vector<StdEnv> *envs, StageClock &clk) {
  int st;
  const int64_t nm = (int64_t)mregs.size();
  std::vector<int64_t> off((size_t)nm);
  std::vector<int32_t> len((size_t)nm), cfg((size_t)nm);
  for (int64_t e = 0; e < nm; e++) {
    const StdEnv &en = mregs[(size_t)e];
    off[(size_t)e] = surv[(size_t)en.s].aa_off + en.i - 1; len[(size_t)e] = en.j - en.i + 1;
    cfg[(size_t)e] = surv[(size_t)en.s].n;
  }
  bath_hip_seqs mv = part_view(ctx, std::move(off), std::move(len));
  const BlockOffsets o = block_offsets(&mv, om->M);
  if ((st = sg.up_begin(StdStaging::view_bytes(nm) + (size_t)(nm + 1) * 8 + (size_t)nm * 4 + 256)) != BATH_OK) return st;
  const int64_t *d_xoff = nullptr;
  if ((st = sg.upload_view(mv, o.x, d_pool, &d_xoff)) != BATH_OK) return st;
  DevBuf &b_mdpo = ctx->scratch[Scratch::kEnvOffsets], &b_cfg = ctx->scratch[Scratch::kStdRegionCfgLen];
  BATH_HIP_TRY(ctx, b_mdpo.reserve((size_t)(nm + 1) * 8)); BATH_HIP_TRY(ctx, b_cfg.reserve((size_t)nm * 4 + 64));
  if ((st = sg.up(b_mdpo.p, {{o.dp.data(), (size_t)(nm + 1) * 8}})) != BATH_OK) return st;
  if ((st = sg.up(b_cfg.p, {{cfg.data(), (size_t)nm * 4}})) != BATH_OK) return st;
  std::vector<StdRegionOut> ro;
  if ((st = std_region_stage(ctx, om, mv.view(), nm, mv.h_len.data(), cfg, o.x, o.dp, d_xoff, b_mdpo.as<int64_t>(), b_cfg.as<int32_t>(), seed, false, &ro, clk)) != BATH_OK) return st;
  for (int64_t e = 0; e < nm; e++) {                      // in region order
    const StdEnv &en = mregs[(size_t)e];
    for (size_t c = 0; c < ro[(size_t)e].env.size(); c++)
      envs->push_back(StdEnv{en.s, en.i + ro[(size_t)e].env[c].first - 1, en.i + ro[(size_t)e].env[c].second - 1, true, ro[(size_t)e].corr[c]});
  }
  return BATH_OK;
}

// What the envelope kernels leave on the host for the hits
struct StdEnvBatch {
  std::vector<int64_t> toff;          // std_trace_offsets
  std::vector<StdEnvOut> eo;          // [ne] the kernels' records
  std::vector<float> envsc;           // [ne] the envelopes' Forward scores
  std::vector<uint8_t> tcols;         // the traces' columns, envelope e's from toff[e], last column first
  std::vector<float> col_pp;          // the posteriors of the columns that exist, densely (StdEnvOut::pp_off)
};

// Three arrays of ne + 1, ne and ne entries, as the trace kernels read them: the envelopes' slices of the column buffer; then, per
// envelope, where the codon of its first residue starts in the DNA block and which way the strand runs (for the degenerate-codon
// test of the alignment score)
static std::vector<int64_t> std_trace_offsets(int M, const bath_hip_seqs *dna, const std::vector<PipelineSurvivor> &surv, const std::vector<StdEnv> &envs) {
  const size_t ne = envs.size();
  std::vector<int64_t> toff(ne + 1 + 2 * ne, 0);
  for (size_t e = 0; e < ne; e++) {
    const StdEnv &en = envs[e];
    toff[e + 1] = toff[e] + (en.j - en.i + 1) + M + 2;
    const PipelineSurvivor &o = surv[(size_t)en.s];
    const int64_t p = (int64_t)o.start + 3 * (int64_t)(en.i - 1);           // strand position (1-based) of that codon's first nucleotide
    const int64_t woff = dna->h_off[(size_t)o.window], wn = dna->h_len[(size_t)o.window];
    toff[ne + 1 + e] = o.strand ? woff + wn - p : woff + p - 1;
    toff[ne + 1 + ne + e] = o.strand ? -1 : 1;
  }
  return toff;
}

// The traceback over filled matrices with a wave per envelope; with a lane per envelope under BATH_HIP_STD_TRACE_LANE=1 (A/B and
// tests), and where no fill kernel ran (<filled> == 0) that kernel does the decoding, the OA fill and null2 as well.
static int std_launch_trace(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, SeqView v, int filled, const int64_t *d_exoff, float *d_col_pp, int *d_col_cursor) {
  const int64_t ne = v.n;
  const int M = om->M;
  auto &s = ctx->scratch;
  float *f = s[Scratch::kEnvFwdMatrix].as<float>(), *b = s[Scratch::kEnvBwdMatrix].as<float>(), *px = s[Scratch::kStdPosteriorRows].as<float>(), *ox = s[Scratch::kStdOaRows].as<float>();
  const int64_t *dpo = s[Scratch::kEnvOffsets].as<int64_t>(), *toff = s[Scratch::kStdTraceOffsets].as<int64_t>();
  StdEnvOut *out = s[Scratch::kStdEnvOut].as<StdEnvOut>();
  uint8_t *tb = s[Scratch::kEnvTraceColumns].as<uint8_t>();
  const bool lane_trace = [] { const char *e = std::getenv("BATH_HIP_STD_TRACE_LANE"); return e && e[0] == '1'; }();
  if (filled && !lane_trace)
    hipLaunchKernelGGL(std_trace_wave_kernel, dim3((unsigned)ne), dim3(64), 0, ctx->stream, v, M, om->d_tf, f, b, dpo, d_exoff, px, ox, out, om->d_cons, tb, toff,
                       om->d_msc, om->d_tsc, dna->d_data, toff + ne + 1, toff + 2 * ne + 1, d_col_pp, d_col_cursor);
  else
    hipLaunchKernelGGL(std_envelope_kernel, dim3((unsigned)((ne * kStdTraceSpread + 63) / 64)), dim3(64), 0, ctx->stream, v, M, om->d_tf, om->d_rf, f, b, dpo,
                       s[Scratch::kStdFwdRows].as<float>(), s[Scratch::kStdBwdRows].as<float>(), d_exoff, px, ox, s[Scratch::kEnvNull2Work].as<float>(), out,
                       om->d_cons, tb, toff, filled, om->d_msc, om->d_tsc, dna->d_data, toff + ne + 1, toff + 2 * ne + 1, nullptr, d_col_pp, d_col_cursor);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

// The batch's results to the host: what does not depend on the number of columns first (with the count), then the columns' posteriors
static int std_download_envelopes(bath_hip_ctx *ctx, StdStaging &sg, int64_t ne, const int *d_col_cursor, const float *d_col_pp, StdEnvBatch *out) {
  int st;
  out->eo.resize((size_t)ne); out->envsc.resize((size_t)ne); out->tcols.resize((size_t)out->toff[(size_t)ne]);
  const size_t ntc = out->tcols.size();
  const size_t o_tc = 64, o_eo = o_tc + ((ntc + 63) & ~(size_t)63), o_sc = o_eo + (((size_t)ne * sizeof(StdEnvOut) + 63) & ~(size_t)63), o_end = o_sc + (size_t)ne * 4;
  if ((st = sg.down_reserve(o_end)) != BATH_OK) return st;
  char *h = static_cast<char *>(ctx->stage[Pinned::kStdDownloads].p);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h, d_col_cursor, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h + o_tc, ctx->scratch[Scratch::kEnvTraceColumns].p, ntc, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h + o_eo, ctx->scratch[Scratch::kStdEnvOut].p, (size_t)ne * sizeof(StdEnvOut), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h + o_sc, ctx->scratch[Scratch::kStdScores].p, (size_t)ne * 4, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  int total = 0;
  std::memcpy(&total, h, sizeof(int));
  std::memcpy(out->tcols.data(), h + o_tc, ntc);
  std::memcpy(out->eo.data(), h + o_eo, (size_t)ne * sizeof(StdEnvOut));
  std::memcpy(out->envsc.data(), h + o_sc, (size_t)ne * 4);
  out->col_pp.resize((size_t)total);
  if (total > 0) {
    if ((st = sg.down_reserve((size_t)total * sizeof(float))) != BATH_OK) return st;
    BATH_HIP_TRY(ctx, hipMemcpyAsync(ctx->stage[Pinned::kStdDownloads].p, d_col_pp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out->col_pp.data(), ctx->stage[Pinned::kStdDownloads].p, (size_t)total * sizeof(float));
  }
  return BATH_OK;
}

// Stage (c): the envelopes' full Forward / Backward (unihit, L = Ld), then decoding, OA, null2 and the traceback, and what the
// hits need of it on the host
static int std_stage_envelopes(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const std::vector<PipelineSurvivor> &surv, const uint8_t *d_pool,
                               StdStaging &sg, const std::vector<StdEnv> &envs, StdEnvBatch *out) {
  int st;
  const int64_t ne = (int64_t)envs.size();
  const int M = om->M;
  std::vector<int64_t> off((size_t)ne);
  std::vector<int32_t> len((size_t)ne);
  for (int64_t e = 0; e < ne; e++) { off[(size_t)e] = surv[(size_t)envs[(size_t)e].s].aa_off + envs[(size_t)e].i - 1; len[(size_t)e] = envs[(size_t)e].j - envs[(size_t)e].i + 1; }
  bath_hip_seqs ev = part_view(ctx, std::move(off), std::move(len));
  const BlockOffsets o = block_offsets(&ev, M);
  if ((st = sg.up_begin(StdStaging::view_bytes(ne) + (size_t)(4 * ne + 2) * 8 + 512)) != BATH_OK) return st;      // the view, the columns' offsets (3 ne + 1), the matrices' (ne + 1)
  const int64_t *d_exoff = nullptr;
  if ((st = sg.upload_view(ev, o.x, d_pool, &d_exoff)) != BATH_OK) return st;
  if ((st = std_reserve_envelope_buffers(ctx, o, ne, M)) != BATH_OK) return st;
  DevBuf &b_f = ctx->scratch[Scratch::kEnvFwdMatrix], &b_b = ctx->scratch[Scratch::kEnvBwdMatrix], &b_dpo = ctx->scratch[Scratch::kEnvOffsets], &b_fx = ctx->scratch[Scratch::kStdFwdRows], &b_bx = ctx->scratch[Scratch::kStdBwdRows];
  DevBuf &b_sc = ctx->scratch[Scratch::kStdScores], &b_st = ctx->scratch[Scratch::kStdStatus], &b_tb = ctx->scratch[Scratch::kEnvTraceColumns], &b_toff = ctx->scratch[Scratch::kStdTraceOffsets];
  out->toff = std_trace_offsets(M, dna, surv, envs);
  const size_t ncols = (size_t)out->toff[(size_t)ne];
  if (ncols >= (size_t)INT32_MAX) { ctx->set_error("too many envelopes for the trace columns' 32-bit offsets"); return BATH_ERANGE; }
  // [columns: 1 B each, per envelope] [cursor] [the columns' posteriors, densely: 4 B per column that exists]
  const size_t tb_cols = (ncols + 255) / 256 * 256;
  BATH_HIP_TRY(ctx, b_tb.reserve(tb_cols + 256 + ncols * sizeof(float) + 64)); BATH_HIP_TRY(ctx, b_toff.reserve(out->toff.size() * 8));
  BATH_HIP_TRY(ctx, b_dpo.reserve((size_t)(ne + 1) * 8)); BATH_HIP_TRY(ctx, b_sc.reserve((size_t)ne * 8)); BATH_HIP_TRY(ctx, b_st.reserve((size_t)ne * 8));
  int *d_col_cursor = reinterpret_cast<int *>(b_tb.as<char>() + tb_cols);
  float *d_col_pp = reinterpret_cast<float *>(b_tb.as<char>() + tb_cols + 256);
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_col_cursor, 0, sizeof(int), ctx->stream));
  if ((st = sg.up(b_toff.p, {{out->toff.data(), out->toff.size() * 8}})) != BATH_OK) return st;
  if ((st = sg.up(b_dpo.p, {{o.dp.data(), (size_t)(ne + 1) * 8}})) != BATH_OK) return st;
  if ((st = launch_fwd_wave(ctx, om, ev.view(), nullptr, ne, b_sc.as<float>(), b_st.as<int32_t>(), nullptr, b_fx.as<float>(), d_exoff, b_f.as<float>(), b_dpo.as<int64_t>(), 1)) != BATH_OK) return st;
  if ((st = launch_bwd_wave(ctx, om, ev.view(), ne, b_fx.as<float>(), d_exoff, b_sc.as<float>() + ne, b_st.as<int32_t>() + ne, b_bx.as<float>(), b_b.as<float>(), b_dpo.as<int64_t>(), 1)) != BATH_OK) return st;
  // decoding + OA fill + null2: a wave or a block per envelope; then the traceback.  BATH_HIP_STD_SERIAL=1 (tests) or a model longer
  // than 1024 nodes: everything in the lane-per-envelope kernel.
  const int fill = std_fill_choice(M);
  if (fill && (st = std_launch_fill(ctx, M, fill, ev.view(), ne, om->d_tf, om->d_rf, b_f.as<float>(), b_b.as<float>(), b_dpo.as<int64_t>(), b_fx.as<float>(), b_bx.as<float>(), d_exoff,
                                    ctx->scratch[Scratch::kStdPosteriorRows].as<float>(), ctx->scratch[Scratch::kStdOaRows].as<float>(), ctx->scratch[Scratch::kStdEnvOut].as<StdEnvOut>(), nullptr)) != BATH_OK) return st;
  if ((st = std_launch_trace(ctx, om, dna, ev.view(), fill ? 1 : 0, d_exoff, d_col_pp, d_col_cursor)) != BATH_OK) return st;
  return std_download_envelopes(ctx, sg, ne, d_col_cursor, d_col_pp, out);
}

// Stage (d): p7_pli_postDomainDef_BATH: coordinates on the sequence, score corrections, P-value; the hits, their --cigar
// strings and their traces are appended to the context's
static void std_stage_hits(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const std::vector<PipelineSurvivor> &surv, const std::vector<StdEnv> &envs,
                           const StdEnvBatch &b, const DomOpts &opt) {
  const int ml = om->max_length;
  const RunningZ runZ(dna, opt.nres_before, opt.strands);                    // pli->Z, p7_pipeline.c:1246: the count at the hit's window and strand
  for (size_t e = 0; e < envs.size(); e++) {
    const StdEnvOut &t = b.eo[e];
    if (!t.ok) continue;
    if (t.aliscore < 0.0f) continue;                                         // p7_domaindef.c:1286: "repetitive garbage", no domain
    const StdEnv &en = envs[e];
    const PipelineSurvivor &o = surv[(size_t)en.s];
    const float Zf = runZ.Z(o.window, o.strand, ml);
    const int seq_n = dna->h_len[(size_t)o.window];
    bath_fs_domain dm{};
    dm.window = o.window; dm.strand = o.strand; dm.fs_window = o.fs_window;
    dm.ihmm = t.k1; dm.jhmm = t.k2; dm.envsc = b.envsc[e]; dm.oasc = t.oasc;
    dm.domcorrection = std::max(0.f, en.clustered ? en.n2corr : t.domcorrection);
    // alignment in nucleotides of the window (the ORF itself in the plain pipeline): p7_trace_fs_Convert puts a residue on its
    // codon's last nucleotide, offset by where the ORF starts in the window
    const int a1 = t.i1 + en.i - 1, a2 = t.i2 + en.i - 1, shift = o.start - o.win_start;
    int iali = shift + a1 * 3 - 2, jali = shift + a2 * 3, ienv = en.i, jenv = en.j;
    const int env_len = jenv - ienv + 1, ali_len = (jali - iali + 1) / 3;
    if (ali_len < 4) continue;                                               // p7_pipeline.c:1197
    if (!o.strand) {
      dm.ienv = 1 + o.start + ienv * 3 - 4; dm.jenv = 1 + o.start + jenv * 3 - 2;
      dm.iali = 1 + o.win_start + iali - 2; dm.jali = 1 + o.win_start + jali - 2;
    } else {                                                                 // the reference's orfsq->start is the top-strand coordinate
      const int ostart_ref = seq_n - o.start + 1;
      dm.ienv = 1 + ostart_ref - ienv * 3 + 2; dm.jenv = 1 + ostart_ref - jenv * 3;
      dm.jali = seq_n - (o.win_start + jali) + 2; dm.iali = seq_n - (o.win_start + iali) + 2;
    }
    float bitscore = dm.envsc;                                               // :1222-1226
    bitscore -= 2 * std::log(2. / (env_len + 2));
    bitscore += 2 * std::log(2. / (ml + 2));
    bitscore -= (env_len - ali_len) * std::log((double)((float)env_len / (float)(env_len + 2)));
    bitscore += (ml - ali_len) * std::log((double)((float)ml / (float)(ml + 2)));
    const float dom_bias = opt.do_null2 ? flogsum_host(0.0f, (float)(std::log(1. / 256.) + dm.domcorrection)) : 0.0f;   // :1230-1233
    const float p1 = (float)ml / (float)(ml + 1);
    const float nullsc = (float)((float)ml * std::log((double)p1) + std::log(1. - p1));      // p7_bg_NullOne at max_length
    dm.dombias = dom_bias;
    dm.bitscore = (float)((bitscore - (nullsc + dom_bias)) / kLn2);
    dm.pre_score = (float)(bitscore / kLn2);
    dm.lnP = (double)(float)exp_logsurv(dm.bitscore, om->evparam[BATH_FTAU], om->evparam[BATH_FLAMBDA]);
    dm.reported = opt.reportable(dm.lnP, Zf, dm.bitscore) ? 1 : 0;           // :1247-1248
    // columns were written last to first; every codon has 3 nucleotides
    const int nc = std::min<int>(t.ncol, (int)(b.toff[e + 1] - b.toff[e]));
    std::vector<uint16_t> cols((size_t)nc);
    for (int z = 0; z < nc; z++) cols[(size_t)z] = (uint16_t)(b.tcols[(size_t)b.toff[e] + (size_t)(nc - 1 - z)] | (3u << 4) | (5u << 8));
    dm.ali_columns = nc; dm.n_stops = 0;
    dm.pid = nc > 0 ? ((float)t.exact / nc) * 100 : 0.f;
    dm.cigar_off = (int64_t)ctx->cigars.size();
    ctx->cigars += cigar_from_columns(cols.data(), nc);
    ctx->cigars.push_back('\0');
    // dom->tr after p7_trace_fs_Convert (p7_trace.c:405): a residue sits on its codon's last nucleotide, start = orf_start - window_start
    const bool have_pp = (size_t)t.pp_off + (size_t)nc <= b.col_pp.size() && nc == t.ncol;
    ctx->trace_push(cols.data(), have_pp ? b.col_pp.data() + t.pp_off : nullptr, nc, t.k1, shift + a1 * 3 - 2, o.win_start, o.start, 0, 0);
    ctx->fs_domains.push_back(dm);
  }
}

// Domain definition and hit scores for ORFs that passed the Forward filter; appends to ctx->fs_domains.
int bath::std_domains(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const std::vector<PipelineSurvivor> &surv,
                      const uint8_t *d_pool, const DomOpts &opt, int64_t *n_clustered_regions) {
  int st;
  if (surv.empty()) return BATH_OK;
  StageClock clk;
  StdStaging sg{ctx};
  std::vector<StdEnv> envs, mregs;
  if ((st = std_stage_regions(ctx, om, surv, d_pool, sg, &envs, &mregs)) != BATH_OK) return st;
  clk.lap("std:   parsers + regions");
  if (n_clustered_regions) *n_clustered_regions += (int64_t)mregs.size();      // regions resolved by clustering (ddef->nclustered)
  if (!mregs.empty() && (st = std_stage_multidomain(ctx, om, surv, d_pool, sg, mregs, opt.seed, &envs, clk)) != BATH_OK) return st;
  if (envs.empty()) return BATH_OK;
  StdEnvBatch batch;
  if ((st = std_stage_envelopes(ctx, om, dna, surv, d_pool, sg, envs, &batch)) != BATH_OK) return st;
  clk.lap("std:   envelope kernels");
  std_stage_hits(ctx, om, dna, surv, envs, batch, opt);
  clk.lap("std:   post-processing (host)");
  return BATH_OK;
}

extern "C" int bath_hip_pipeline_hits(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna, const bath_pipeline_params *prm_in,
                                      double E_report, bath_pipeline_stats *stats, const bath_fs_domain **domains, int64_t *n_domains,
                                      int64_t *n_clustered_regions) {
  if (!ctx || !om || !dna || !prm_in || !domains || !n_domains) return BATH_EINVAL;
  *domains = nullptr; *n_domains = 0;
  int64_t nclust = 0;
  ctx->fs_domains.clear();
  ctx->cigars.clear();
  ctx->traces_clear();
  ctx->spans_reset();
  bath_pipeline_params prm = *prm_in;
  prm.fs_pipe = 0;
  bath_pipeline_stats st_local{};
  std::vector<PipelineSurvivor> surv;
  const uint8_t *d_pool = nullptr;
  StageClock clk;
  // the cascade's Forward parser leaves its special-state rows for the domain stage (BATH_HIP_KEEP_FWD=0: the domain stage runs the
  // parser again, as it did until round 5)
  const bool keep = [] { const char *e = std::getenv("BATH_HIP_KEEP_FWD"); return !(e && e[0] == '0'); }();
  ctx->keep_fwd_rows = keep;
  int st = pipeline_filters_survivors(ctx, om, dna, &prm, &st_local, &surv, &d_pool);
  ctx->keep_fwd_rows = false;
  if (st != BATH_OK) { ctx->fwd_rows_kept = nullptr; return st; }
  clk.lap("std: cascade + survivors to the host");
  if (stats) *stats = st_local;
  for (PipelineSurvivor &o : surv) o.win_start = o.start;                  // windowsq is the ORF's own stretch of DNA (p7_pipeline.c:1755)
  st = std_domains(ctx, om, dna, surv, d_pool, DomOpts(prm, E_report), &nclust);
  ctx->fwd_rows_kept = nullptr; ctx->fwd_rows_off = nullptr;
  if (st != BATH_OK) return st;
  if (n_clustered_regions) *n_clustered_regions = nclust;
  *domains = ctx->fs_domains.data(); *n_domains = (int64_t)ctx->fs_domains.size();
  return BATH_OK;
}

// =================================================================================================================
// Full-matrix entry points over a block of amino-acid targets: what the single-target prototypes p7_Forward / p7_Backward /
// p7_Decoding / p7_OptimalAccuracy / p7_Null2_ByExpectation of impl_hip/ bind (the domain stage above runs the same kernels).
// =================================================================================================================
extern "C" int bath_hip_forward_full(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, const int32_t *cfg_len, int unihit,
                                     float *sc, int32_t *status, float *dp, float *xmx) {
  if (!ctx || !om || !sq || !sc) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n = sq->n;
  if (n == 0) return BATH_OK;
  const int M = om->M;
  int maxcfg = sq->maxlen;
  if (cfg_len) for (int64_t i = 0; i < n; i++) maxcfg = std::max(maxcfg, (int)cfg_len[i]);
  int st = om->ensure_len_tables(maxcfg + 1);
  if (st != BATH_OK) return st;
  const BlockOffsets o = block_offsets(sq, M);
  DevBuf &b_f = ctx->scratch[Scratch::kEnvFwdMatrix], &b_off = ctx->scratch[Scratch::kEnvOffsets], &b_fx = ctx->scratch[Scratch::kEnvFwdRows], &b_sc = ctx->scratch[Scratch::kEnvScores], &b_cfg = ctx->scratch[Scratch::kStdRegionCfgLen];
  BATH_HIP_TRY(ctx, b_f.reserve((size_t)o.dp[(size_t)n] * 4 + 64)); BATH_HIP_TRY(ctx, b_fx.reserve((size_t)o.x[(size_t)n] * 4 + 64));
  BATH_HIP_TRY(ctx, b_off.reserve((size_t)(n + 1) * 16)); BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 8)); BATH_HIP_TRY(ctx, b_cfg.reserve((size_t)n * 4 + 64));
  int64_t *d_xo = b_off.as<int64_t>(), *d_dpo = d_xo + (n + 1);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_xo, o.x.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_dpo, o.dp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (cfg_len) BATH_HIP_TRY(ctx, hipMemcpyAsync(b_cfg.p, cfg_len, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  float *d_sc = b_sc.as<float>();
  int32_t *d_st = reinterpret_cast<int32_t *>(d_sc + n);
  if ((st = launch_fwd_wave(ctx, om, sq->view(), nullptr, n, d_sc, d_st, nullptr, b_fx.as<float>(), d_xo, b_f.as<float>(), d_dpo, unihit ? 1 : 0,
                            cfg_len ? b_cfg.as<int32_t>() : nullptr)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(sc, d_sc, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (status) BATH_HIP_TRY(ctx, hipMemcpyAsync(status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (dp) BATH_HIP_TRY(ctx, hipMemcpyAsync(dp, b_f.p, (size_t)o.dp[(size_t)n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (xmx) BATH_HIP_TRY(ctx, hipMemcpyAsync(xmx, b_fx.p, (size_t)o.x[(size_t)n] * 4, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return BATH_OK;
}

extern "C" int bath_hip_std_envelopes_fill(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, bath_std_result *res,
                                           float *pp, float *oa, float *ppx, float *oax, int fill) {
  if (!ctx || !om || !sq || !res || fill < 0 || fill > 2) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n = sq->n;
  if (n == 0) return BATH_OK;
  const int M = om->M;
  if (fill && M > 1024) { ctx->set_error("the standard branch's fill kernels take models of up to 1024 nodes"); return BATH_ERANGE; }
  int st = om->ensure_len_tables(sq->maxlen + 1);
  if (st != BATH_OK) return st;
  const BlockOffsets o = block_offsets(sq, M);
  std::vector<int64_t> toff((size_t)n + 1, 0);
  for (int64_t e = 0; e < n; e++) toff[(size_t)e + 1] = toff[(size_t)e] + sq->h_len[(size_t)e] + M + 2;
  DevBuf &b_f = ctx->scratch[Scratch::kEnvFwdMatrix], &b_b = ctx->scratch[Scratch::kEnvBwdMatrix], &b_off = ctx->scratch[Scratch::kEnvOffsets], &b_fx = ctx->scratch[Scratch::kStdFwdRows], &b_bx = ctx->scratch[Scratch::kStdBwdRows], &b_px = ctx->scratch[Scratch::kStdPosteriorRows],
         &b_ox = ctx->scratch[Scratch::kStdOaRows], &b_em = ctx->scratch[Scratch::kEnvNull2Work], &b_out = ctx->scratch[Scratch::kStdEnvOut], &b_tb = ctx->scratch[Scratch::kEnvTraceColumns], &b_sc = ctx->scratch[Scratch::kStdScores], &b_n2 = ctx->scratch[Scratch::kEnvNull2];
  const size_t nx = (size_t)o.x[(size_t)n], ndp = (size_t)o.dp[(size_t)n];
  if ((st = std_reserve_envelope_buffers(ctx, o, n, M)) != BATH_OK) return st;
  BATH_HIP_TRY(ctx, b_tb.reserve((size_t)toff[(size_t)n] + 64)); BATH_HIP_TRY(ctx, b_off.reserve((size_t)(n + 1) * 24));
  BATH_HIP_TRY(ctx, b_sc.reserve((size_t)n * 16)); BATH_HIP_TRY(ctx, b_n2.reserve((size_t)n * kKp * 4 + 64));
  int64_t *d_xo = b_off.as<int64_t>(), *d_dpo = d_xo + (n + 1), *d_to = d_dpo + (n + 1);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_xo, o.x.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_dpo, o.dp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_to, toff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  float *d_sc = b_sc.as<float>();
  int32_t *d_st = reinterpret_cast<int32_t *>(d_sc + 2 * n);
  if ((st = launch_fwd_wave(ctx, om, sq->view(), nullptr, n, d_sc, d_st, nullptr, b_fx.as<float>(), d_xo, b_f.as<float>(), d_dpo, 1)) != BATH_OK) return st;
  if ((st = launch_bwd_wave(ctx, om, sq->view(), n, b_fx.as<float>(), d_xo, d_sc + n, d_st + n, b_bx.as<float>(), b_b.as<float>(), d_dpo, 1)) != BATH_OK) return st;
  // p7_Decoding, p7_OptimalAccuracy, p7_Null2_ByExpectation (and the traceback, unused here), a lane per envelope: posteriors
  // overwrite Backward, the OA matrix overwrites Forward, as in the reference.  fill 1 / 2: the domain stage's fill kernel for this
  // model first, then the lane-per-envelope kernel for the traceback alone, as std_domains runs them: what comes back is what the
  // traceback read
  if (fill) {
    BATH_HIP_TRY(ctx, hipMemsetAsync(b_n2.p, 0, (size_t)n * kKp * 4, ctx->stream));       // (an envelope whose decoding overflows gets no null2)
    if ((st = std_launch_fill(ctx, M, fill, sq->view(), n, om->d_tf, om->d_rf, b_f.as<float>(), b_b.as<float>(), d_dpo, b_fx.as<float>(), b_bx.as<float>(), d_xo,
                              b_px.as<float>(), b_ox.as<float>(), b_out.as<StdEnvOut>(), b_n2.as<float>())) != BATH_OK) return st;
  }
  hipLaunchKernelGGL(std_envelope_kernel, dim3((unsigned)((n * kStdTraceSpread + 63) / 64)), dim3(64), 0, ctx->stream, sq->view(), M, om->d_tf, om->d_rf, b_f.as<float>(), b_b.as<float>(), d_dpo,
                     b_fx.as<float>(), b_bx.as<float>(), d_xo, b_px.as<float>(), b_ox.as<float>(), b_em.as<float>(), b_out.as<StdEnvOut>(),
                     (const uint8_t *)nullptr, b_tb.as<uint8_t>(), d_to, fill ? 1 : 0, (const float *)nullptr, (const float *)nullptr, (const uint8_t *)nullptr,
                     (const int64_t *)nullptr, (const int64_t *)nullptr, b_n2.as<float>());
  BATH_HIP_TRY(ctx, hipGetLastError());
  std::vector<StdEnvOut> eo((size_t)n);
  std::vector<float> h_sc((size_t)n * 2), h_n2((size_t)n * kKp);
  std::vector<int32_t> h_st((size_t)n * 2);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(eo.data(), b_out.p, (size_t)n * sizeof(StdEnvOut), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h_sc.data(), d_sc, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h_st.data(), d_st, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(h_n2.data(), b_n2.p, (size_t)n * kKp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (pp) BATH_HIP_TRY(ctx, hipMemcpyAsync(pp, b_b.p, ndp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (oa) BATH_HIP_TRY(ctx, hipMemcpyAsync(oa, b_f.p, ndp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (ppx) BATH_HIP_TRY(ctx, hipMemcpyAsync(ppx, b_px.p, nx / 6 * 5 * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (oax) BATH_HIP_TRY(ctx, hipMemcpyAsync(oax, b_ox.p, nx / 6 * 5 * 4, hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t e = 0; e < n; e++) {
    bath_std_result &r = res[(size_t)e];
    r.fwdsc = h_sc[(size_t)e]; r.bcksc = h_sc[(size_t)(n + e)]; r.fwd_status = h_st[(size_t)e]; r.bck_status = h_st[(size_t)(n + e)];
    r.ok = eo[(size_t)e].ok; r.oasc = eo[(size_t)e].oasc;
    std::memcpy(r.null2, &h_n2[(size_t)e * kKp], sizeof(float) * kKp);
  }
  return BATH_OK;
}

extern "C" int bath_hip_std_envelopes(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, bath_std_result *res,
                                      float *pp, float *oa, float *ppx, float *oax) {
  return bath_hip_std_envelopes_fill(ctx, om, sq, res, pp, oa, ppx, oax, 0);
}

// The multi-domain region stage of the standard branch on its own (include/bath_hip.h)
extern "C" int bath_hip_std_region_ensembles(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *regions, const int32_t *cfg_len, uint32_t seed,
                                             int32_t *region_status, int32_t *trace_status, int32_t *seg, int64_t max_seg, int64_t *seg_off,
                                             int32_t *env, float *env_n2corr, int64_t max_env, int64_t *env_off) {
  if (!ctx || !om || !regions || !region_status || !seg_off || !env_off || max_seg < 0 || max_env < 0 || (max_seg > 0 && !seg) || (max_env > 0 && (!env || !env_n2corr))) {
    if (ctx) ctx->set_error("bath_hip_std_region_ensembles: needs a profile, the regions and its output arrays");
    return BATH_EINVAL;
  }
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n = regions->n;
  seg_off[0] = 0; env_off[0] = 0;
  ctx->spans_reset();
  if (n == 0) return BATH_OK;
  std::vector<int32_t> cfg((size_t)n);
  for (int64_t e = 0; e < n; e++) {
    cfg[(size_t)e] = cfg_len ? cfg_len[e] : regions->h_len[(size_t)e];
    if (cfg[(size_t)e] < 0) { ctx->set_error("bath_hip_std_region_ensembles: negative configuration length"); return BATH_EINVAL; }
  }
  int st = om->ensure_len_tables(std::max(regions->maxlen, *std::max_element(cfg.begin(), cfg.end())) + 1);
  if (st != BATH_OK) return st;
  const BlockOffsets o = block_offsets(regions, om->M);
  DevBuf &b_off = ctx->scratch[Scratch::kEnvOffsets], &b_cfg = ctx->scratch[Scratch::kStdRegionCfgLen];
  BATH_HIP_TRY(ctx, b_off.reserve((size_t)(n + 1) * 16)); BATH_HIP_TRY(ctx, b_cfg.reserve((size_t)n * 4 + 64));
  int64_t *d_xo = b_off.as<int64_t>(), *d_dpo = d_xo + (n + 1);
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_xo, o.x.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(d_dpo, o.dp.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(b_cfg.p, cfg.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  std::vector<StdRegionOut> ro;
  StageClock clk;
  if ((st = std_region_stage(ctx, om, regions->view(), n, regions->h_len.data(), cfg, o.x, o.dp, d_xo, d_dpo, b_cfg.as<int32_t>(), seed, true, &ro, clk)) != BATH_OK) return st;
  int64_t nseg = 0, nenv = 0;
  for (int64_t e = 0; e < n; e++) {
    const StdRegionOut &r = ro[(size_t)e];
    region_status[e] = r.status;
    if (trace_status) std::copy(r.trace_status.begin(), r.trace_status.end(), trace_status + (size_t)e * kEnsSamples);
    for (size_t q = 0; q + 5 <= r.segs.size(); q += 5, nseg++) if (nseg < max_seg) std::memcpy(seg + nseg * 5, r.segs.data() + q, 5 * sizeof(int32_t));
    for (size_t c = 0; c < r.env.size(); c++, nenv++) if (nenv < max_env) { env[nenv * 2] = r.env[c].first; env[nenv * 2 + 1] = r.env[c].second; env_n2corr[nenv] = r.corr[c]; }
    seg_off[e + 1] = nseg; env_off[e + 1] = nenv;
  }
  if (nseg > max_seg || nenv > max_env) { ctx->set_error("bath_hip_std_region_ensembles: output arrays too small"); return BATH_ERANGE; }
  return BATH_OK;
}
