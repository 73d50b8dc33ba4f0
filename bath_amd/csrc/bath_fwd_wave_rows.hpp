// bath_fwd_wave_rows.hpp -- the body of the wave-per-target Forward parser kernel (p7_ForwardParser / forward_engine,
// fwdback.c:256-463; odds-ratio space, sparse rescaling as :418-434), as text: included by fwd_wave_kernel<C, GT> (bath_filters.hip)
// and by fwd_wave_batch_kernel<C, GT> (bath_calib_batch.hip: a block's model read from a descriptor at blockIdx.y, score only).
// Included, not called.  The includer provides, as parameters or locals: C; GT; SeqView sq; int M; const float *g_rf,
// *g_tf, *pmove_tab; FwdConsts c; const int32_t *todo; int64_t ntodo; const int *ntodo_dev; float *sc; int32_t *status; float *xmx;
// const int64_t *xmx_off; float *dp; const int64_t *dp_off; int unihit; const int32_t *cfg_len.
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const float *s_rf = reinterpret_cast<const float *>(lds);                      // !GT: [Kp][wave_em_stride(M)], entry node - 1
  const int S = wave_em_stride(M);
  if (ntodo_dev) ntodo = *ntodo_dev;
  if (!GT) {
    wave_em_fill<C>(reinterpret_cast<float *>(lds), g_rf, M, M + 1);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // the lane's transitions, once (!GT): MM IM DM BM / MD DD MI II of its C nodes
  float4 tra[GT ? 1 : C], trb[GT ? 1 : C];
  if constexpr (!GT) {
#pragma unroll
    for (int k = 0; k < C; k++) {
      const int node = min(lane * C + k + 1, M);
      tra[k] = *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8); trb[k] = *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8 + 4);
    }
  }

  for (int64_t job = wid; job < ntodo; job += nw) {
    const int64_t sid = todo ? (int64_t)todo[job] : job;
    const int L = sq.len[sid];
    const uint8_t *s = sq.data + sq.off[sid];
    // unihit (envelope rescoring, p7_oprofile_ReconfigUnihit): nj = 0, so pmove = 2/(L+2); a plain float division, as on the host
    // cfg_len: the length the model was configured for when that is not this target's (a region of an ORF, p7_domaindef.c:553)
    const float pmove = unihit ? (2.0f / ((float)L + 2.0f)) : pmove_tab[cfg_len ? cfg_len[sid] : L], ploop = 1.0f - pmove;
    float *dprow = dp ? dp + dp_off[sid] : nullptr;        // full matrix (p7_Forward): (L+1) x (M+1) x {M, D, I}
    if (dprow) for (int k = lane; k <= M; k += 64) { dprow[(size_t)k * 3] = dprow[(size_t)k * 3 + 1] = dprow[(size_t)k * 3 + 2] = 0.f; }
    float Mp[C], Ip[C], Dp[C];
#pragma unroll
    for (int k = 0; k < C; k++) Mp[k] = Ip[k] = Dp[k] = 0.f;
    float xN = 1.f, xE = 0.f, xJ = 0.f, xC = 0.f, xB = pmove;
    float totscale = 0.f;
    float *xrow = (xmx && xmx_off[sid] >= 0) ? xmx + xmx_off[sid] : nullptr;      // (L+1) x {E,N,J,B,C,SCALE}, P7_OMX xmx (impl_sse.h:253-262); a negative offset: not wanted for this target
    if (xrow && lane == 0) { xrow[0] = xE; xrow[1] = xN; xrow[2] = xJ; xrow[3] = xB; xrow[4] = xC; xrow[5] = 1.0f; }

    // The residues arrive 64 rows at a time, a lane each, the next 64 in flight: with a load per row every row of a launch of a
    // few dozen targets (one query's envelopes) waited for its own trip to memory
    int rbuf = (lane < L) ? (int)s[lane] : 0, rnext = 0;
    for (int i = 1; i <= L; i++) {
      const int j = (i - 1) & 63;
      if (j == 0) { const int q = i - 1 + 64 + lane; rnext = (q < L) ? (int)s[q] : 0; }
      const int x = min(__builtin_amdgcn_readlane(rbuf, j), kKp - 1);
      if (j == 63) rbuf = rnext;
      float em[C];
      if constexpr (!GT) wave_em_load<C>(s_rf + (size_t)x * S, lane, em);
      else {
#pragma unroll
        for (int k = 0; k < C; k++) em[k] = g_rf[(size_t)x * (M + 1) + min(lane * C + k + 1, M)];
      }
      const float mIn = wave_shr1_f32(Mp[C - 1], 0.f), iIn = wave_shr1_f32(Ip[C - 1], 0.f), dIn = wave_shr1_f32(Dp[C - 1], 0.f);
      float Mc[C], Ic[C], md[C], tdd[C];
      float sumE = 0.f;
#pragma unroll
      for (int k = 0; k < C; k++) {
        const int node = lane * C + k + 1;
        if (node <= M) {
          float4 ta, tb;                                                                      // MM IM DM BM / MD DD MI II
          if constexpr (GT) { ta = *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8); tb = *reinterpret_cast<const float4 *>(g_tf + (size_t)node * 8 + 4); }
          else { ta = tra[k]; tb = trb[k]; }
          const float m1 = (k == 0) ? mIn : Mp[k - 1];
          const float i1 = (k == 0) ? iIn : Ip[k - 1];
          const float d1 = (k == 0) ? dIn : Dp[k - 1];
          float sv = xB * ta.w;
          sv = sv + m1 * ta.x;
          sv = sv + i1 * ta.y;
          sv = sv + d1 * ta.z;
          sv = sv * em[k];
          Mc[k] = sv;
          sumE += sv;
          md[k] = sv * tb.x;
          tdd[k] = tb.y;
          Ic[k] = Mp[k] * tb.z + Ip[k] * tb.w;
        } else { Mc[k] = 0.f; Ic[k] = 0.f; md[k] = 0.f; tdd[k] = 0.f; }
      }
      // D(node+1) = md(node) + D(node)*tDD(node): affine maps composed by wavefront scan
      float A = 0.f, B = 1.f;
#pragma unroll
      for (int k = 0; k < C; k++) { A = md[k] + A * tdd[k]; B *= tdd[k]; }
      // by DPP; lanes without a source see the identity map (A = 0, B = 1): A + 0 * B = A, B * 1 = B
#define BATH_FWD_STEP(CTRL, MASK) { const float Ap = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, A), CTRL, MASK, 0xf, false)), \
                                                 Bp = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0x3f800000, __builtin_bit_cast(int, B), CTRL, MASK, 0xf, false)); \
                                    A = A + Ap * B; B = B * Bp; }
      BATH_FWD_STEP(0x111, 0xf) BATH_FWD_STEP(0x112, 0xf) BATH_FWD_STEP(0x114, 0xf) BATH_FWD_STEP(0x118, 0xf) BATH_FWD_STEP(0x142, 0xa) BATH_FWD_STEP(0x143, 0xc)
#undef BATH_FWD_STEP
      const float din = wave_shr1_f32(A, 0.f);
      float Dc[C];
      Dc[0] = din;
#pragma unroll
      for (int k = 1; k < C; k++) Dc[k] = md[k - 1] + Dc[k - 1] * tdd[k - 1];
#pragma unroll
      for (int k = 0; k < C; k++) sumE += Dc[k];
      xE = wave_sum_f32(sumE);
      xN = xN * ploop;
      xC = (xC * ploop) + (xE * c.xfE_move);
      xJ = (xJ * ploop) + (xE * c.xfE_loop);
      xB = (xJ * pmove) + (xN * pmove);
      float scale = 1.0f;
      if (xE > 1.0e4f) {
        xN = xN / xE; xC = xC / xE; xJ = xJ / xE; xB = xB / xE;
        const float inv = (float)(1.0 / (double)xE);
#pragma unroll
        for (int k = 0; k < C; k++) { Mc[k] *= inv; Dc[k] *= inv; Ic[k] *= inv; }
        totscale += (float)log((double)xE);
        scale = xE;
        xE = 1.0f;
      }
      if (xrow && lane == 0) { float *r = xrow + (size_t)i * 6; r[0] = xE; r[1] = xN; r[2] = xJ; r[3] = xB; r[4] = xC; r[5] = scale; }
      if (dprow) {
        float *r = dprow + (size_t)i * (M + 1) * 3;
        if (lane == 0) r[0] = r[1] = r[2] = 0.f;
#pragma unroll
        for (int k = 0; k < C; k++) { const int node = lane * C + k + 1; if (node <= M) { r[(size_t)node * 3] = Mc[k]; r[(size_t)node * 3 + 1] = Dc[k]; r[(size_t)node * 3 + 2] = Ic[k]; } }
      }
#pragma unroll
      for (int k = 0; k < C; k++) { Mp[k] = Mc[k]; Ip[k] = Ic[k]; Dp[k] = Dc[k]; }
    }
    if (lane == 0) {
      if (isnan(xC) || (L > 0 && xC == 0.0f) || isinf(xC)) { sc[sid] = -INFINITY; status[sid] = BATH_ERANGE; }
      else { sc[sid] = (float)((double)totscale + log((double)(xC * pmove))); status[sid] = BATH_OK; }
    }
  }
