// bath_vit_wave_rows.hpp -- the body of the wave-per-target Viterbi filter kernel (p7_ViterbiFilter[_BATH], vitfilter.c:83-465), as
// text: included by vit_wave_kernel<C> (bath_filters.hip) and by vit_wave_batch_kernel<C> (bath_calib_batch.hip: a block's model read
// from a descriptor at blockIdx.y, no window outputs).  Included, not called.  The includer provides, as parameters or
// locals: C; SeqView sq; int M; const int16_t *g_rw, *g_tw, *xwmove_tab; const uint8_t *tjb_tab; VitConsts c; const int32_t *todo;
// int64_t ntodo; const int *ntodo_dev; float *sc; int32_t *status; and the window outputs (null: plain p7_ViterbiFilter)
// const float *filtersc; const uint8_t *ssv_scores; WindowRec *wins; int *win_count; int win_cap; int32_t *kminmax.
  // Emission rows in LDS as [Kp][S] int16, entry node - 1, S a multiple of 8 (a lane's C nodes: aligned vector reads that follow the
  // previous lane's, no bank conflicts; 64 C entries of padding behind the last row); the lane's transitions in registers, read
  // once (as 16 bytes per node in LDS they were 16 C bytes apart from lane to lane: a 32-way conflict at C = 8).  See fwd_wave_kernel.
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int16_t *s_rw = reinterpret_cast<int16_t *>(lds);
  const int S = vit_em_stride(M);
  for (int i = threadIdx.x; i < kKp * S + 64 * C; i += blockDim.x) { const int x = i / S, k = i - x * S; s_rw[i] = (x < kKp && k < M) ? g_rw[(size_t)x * (M + 1) + k + 1] : (int16_t)-32768; }
  __syncthreads();
  enum { MM, IM, DM, BM, MD, DD, MI, II };
  const int lane = threadIdx.x & 63;
  int4 twq[C];
#pragma unroll
  for (int k = 0; k < C; k++) twq[k] = *reinterpret_cast<const int4 *>(g_tw + (size_t)min(lane * C + k + 1, M) * 8);
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const bool do_win = (wins != nullptr);
  if (ntodo_dev) ntodo = *ntodo_dev;

  for (int64_t job = wid; job < ntodo; job += nw) {
    const int64_t sid = todo ? (int64_t)todo[job] : job;
    const int L = sq.len[sid];
    const uint8_t *s = sq.data + sq.off[sid];
    const int xw_move = xwmove_tab[L];
    int sc_thresh = 0, sc_ext_thresh = 0, skip_until = 0, kmin = 1 << 30, kmax = 0;
    if (do_win) {
      const double fsc = (double)filtersc[sid];
      sc_thresh = (int)(int16_t)(int)ceil(((fsc + 0.69314718055994529 * c.invP_vit + 3.0) * (double)c.scale_w) -
                                          (double)(float)c.xwE_move - (double)(float)xw_move + (double)(float)c.base_w);
      sc_ext_thresh = (int)ceil(((fsc + 0.69314718055994529 * c.invP_msv + 3.0) * (double)c.scale_b) + c.base_b + c.tec_b + (int)tjb_tab[L]);
    }
    int Mp[C], Ip[C], Dp[C];
#pragma unroll
    for (int k = 0; k < C; k++) Mp[k] = Ip[k] = Dp[k] = -32768;
    int xN = c.base_w;
    int xB = (int16_t)(xN + xw_move);
    int xJ = -32768, xC = -32768, xE = -32768;
    bool overflow = false;

    const int ph = threadIdx.x & 63;
    int rbuf = (ph < L) ? (int)s[ph] : 0, rnext = 0;          // residues 64 rows at a time, a lane each, the next 64 in flight (see fwd_wave_kernel)
    for (int i = 1; i <= L; i++) {
      const int j = (i - 1) & 63;
      if (j == 0) { const int q = i - 1 + 64 + ph; rnext = (q < L) ? (int)s[q] : 0; }
      const int x = min(__builtin_amdgcn_readlane(rbuf, j), kKp - 1);
      if (j == 63) rbuf = rnext;
      int em[C];
      {
        const int16_t *rw = s_rw + (size_t)x * S + lane * C;
        if constexpr (C % 8 == 0) {
#pragma unroll
          for (int q = 0; q < C / 8; q++) {
            const int4 v = *reinterpret_cast<const int4 *>(rw + 8 * q);
            const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int h = 0; h < 4; h++) { em[8 * q + 2 * h] = (int16_t)(w[h] & 0xffff); em[8 * q + 2 * h + 1] = w[h] >> 16; }
          }
        } else if constexpr (C % 4 == 0) {
#pragma unroll
          for (int q = 0; q < C / 4; q++) {
            const int2 v = *reinterpret_cast<const int2 *>(rw + 4 * q);
            em[4 * q] = (int16_t)(v.x & 0xffff); em[4 * q + 1] = v.x >> 16; em[4 * q + 2] = (int16_t)(v.y & 0xffff); em[4 * q + 3] = v.y >> 16;
          }
        } else if constexpr (C % 2 == 0) {
#pragma unroll
          for (int q = 0; q < C / 2; q++) { const int v = *reinterpret_cast<const int *>(rw + 2 * q); em[2 * q] = (int16_t)(v & 0xffff); em[2 * q + 1] = v >> 16; }
        } else {
#pragma unroll
          for (int q = 0; q < C; q++) em[q] = (int)rw[q];
        }
      }
      const int mIn = wave_shr1_i32(Mp[C - 1], -32768), iIn = wave_shr1_i32(Ip[C - 1], -32768), dIn = wave_shr1_i32(Dp[C - 1], -32768);
      int Mc[C], Ic[C], dcv[C], tdd[C];
      int xEl = -32768;
#pragma unroll
      for (int k = 0; k < C; k++) {
        const int node = lane * C + k + 1;
        if (node <= M) {
          const int4 tq = twq[k];
          const int tMM = (int16_t)(tq.x & 0xffff), tIM = (int16_t)(tq.x >> 16);
          const int tDM = (int16_t)(tq.y & 0xffff), tBM = (int16_t)(tq.y >> 16);
          const int tMD = (int16_t)(tq.z & 0xffff), tDD = (int16_t)(tq.z >> 16);
          const int tMI = (int16_t)(tq.w & 0xffff), tII = (int16_t)(tq.w >> 16);
          const int m1 = (k == 0) ? mIn : Mp[k - 1];
          const int i1 = (k == 0) ? iIn : Ip[k - 1];
          const int d1 = (k == 0) ? dIn : Dp[k - 1];
          int sv = sat16(xB + tBM);
          sv = max(sv, sat16(m1 + tMM));
          sv = max(sv, sat16(i1 + tIM));
          sv = max(sv, sat16(d1 + tDM));
          sv = sat16(sv + em[k]);
          Mc[k] = sv;
          xEl = max(xEl, sv);
          dcv[k] = sat16(sv + tMD);
          tdd[k] = tDD;
          Ic[k] = max(sat16(Mp[k] + tMI), sat16(Ip[k] + tII));
        } else {
          Mc[k] = -32768; Ic[k] = -32768; dcv[k] = -32768; tdd[k] = -32768;
        }
      }
      xE = wave_max_i32(xEl);
      if (xE >= 32767) { overflow = true; break; }
      xN = (int16_t)(xN + 0);
      xC = (int16_t)max(xC + 0, xE + c.xwE_move);
      xJ = (int16_t)max(xJ + 0, xE + c.xwE_loop);
      xB = (int16_t)max(xJ + xw_move, xN + xw_move);

      if (do_win && i > skip_until && xE >= sc_thresh) {           // vitfilter.c:386-424
        int rank = 1 << 30;
#pragma unroll
        for (int k = 0; k < C; k++) {
          const int node = lane * C + k + 1;
          if (node <= M && Mc[k] == xE) rank = min(rank, ((node - 1) % c.Q8) * 8 + (node - 1) / c.Q8);
        }
        rank = wave_min_i32(rank);
        const int k_start = (rank / 8) + c.Q8 * (rank % 8) + 1;
        int max_k_end = k_start, max_i_end = i, sc_ext = sc_ext_thresh, max_sc_ext = sc_ext, since = 0;
        int kk = k_start + 1, nn = i + 1;
        while (kk <= M && nn <= L) {
          sc_ext += c.bias_b - (int)ssv_scores[(size_t)kk * kKp + min((int)s[nn - 1], kKp - 1)];
          if (sc_ext >= max_sc_ext) { max_sc_ext = sc_ext; max_k_end = kk; max_i_end = nn; since = 0; }
          else if (++since == 5) break;
          kk++; nn++;
        }
        if (lane == 0) {
          int slot = atomicAdd(win_count, 1);
          if (slot < win_cap) wins[slot] = WindowRec{(int32_t)sid, i, max_k_end, max_k_end - k_start + 1, 0.0f};
        }
        kmax = max(kmax, max_k_end);
        kmin = min(kmin, k_start);
        skip_until = max_i_end;
      }

      // exact D row: D(node+1) = max(dcv(node), D(node)+tDD(node)); chain across lanes by scan
      int A = -(1 << 28), B = 0;
#pragma unroll
      for (int k = 0; k < C; k++) { A = max(dcv[k], A + tdd[k]); B += tdd[k]; A = max(A, -(1 << 28)); }
      // inclusive scan of f_l(x) = max(A_l, x + B_l)
      // by DPP; lanes without a source see the identity map (A = -2^28, B = 0).  Integer (max,+): any scan order gives the same D row
#define BATH_VIT_STEP(CTRL, MASK) { const int Ap = dpp_i<CTRL, MASK>(A, -(1 << 28)), Bp = dpp_i<CTRL, MASK>(B, 0); A = max(A, max(Ap, -(1 << 28)) + B); B = max(B + Bp, -(1 << 28)); }
      BATH_VIT_STEP(0x111, 0xf) BATH_VIT_STEP(0x112, 0xf) BATH_VIT_STEP(0x114, 0xf) BATH_VIT_STEP(0x118, 0xf) BATH_VIT_STEP(0x142, 0xa) BATH_VIT_STEP(0x143, 0xc)
#undef BATH_VIT_STEP
      int din = wave_shr1_i32(A, -32768);
      din = max(din, -32768);
      int Dc[C];
      Dc[0] = din;
#pragma unroll
      for (int k = 1; k < C; k++) Dc[k] = max(dcv[k - 1], sat16(Dc[k - 1] + tdd[k - 1]));
#pragma unroll
      for (int k = 0; k < C; k++) { Mp[k] = Mc[k]; Ip[k] = Ic[k]; Dp[k] = Dc[k]; }
    }
    if (lane == 0) {
      if (overflow) { sc[sid] = INFINITY; status[sid] = BATH_ERANGE; }
      else if (xC > -32768) {
        float r = (float)xC + (float)xw_move - (float)c.base_w;
        r /= c.scale_w;
        r = (float)((double)r - 3.0);
        sc[sid] = r; status[sid] = BATH_OK;
      } else { sc[sid] = -INFINITY; status[sid] = BATH_OK; }
      if (do_win && kminmax) { kminmax[2 * sid] = kmin; kminmax[2 * sid + 1] = kmax; }
    }
  }
