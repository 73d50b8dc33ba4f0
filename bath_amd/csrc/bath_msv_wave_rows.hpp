// bath_msv_wave_rows.hpp -- the body of the wave-per-target MSV kernel (p7_MSVFilter with the J state, msvfilter.c:106-207), as text:
// included by msv_wave_kernel<C> (bath_filters.hip: one model, its tables as kernel arguments) and by msv_wave_batch_kernel<C>
// (bath_calib_batch.hip: a block's model read from a descriptor at blockIdx.y).  Included, not called, as bath_fs3_fwd_chain_rows.hpp
// is.  The includer provides, as parameters or locals: C; SeqView sq; int M; const uint8_t *rb; int rb_stride;
// const uint8_t *tjb_tab; MsvConsts c; const int32_t *todo; int64_t ntodo; const int *ntodo_dev; float *sc; int32_t *status.
// Lane l owns nodes l*C+1 .. l*C+C; the waves of the launch's x dimension share the ntodo jobs.
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if (ntodo_dev) ntodo = *ntodo_dev;
  for (int64_t job = wid; job < ntodo; job += nw) {
    const int64_t sid = todo ? (int64_t)todo[job] : job;
    const int L = sq.len[sid];
    const uint8_t *s = sq.data + sq.off[sid];
    const int tjb = tjb_tab[L];
    const int tjbm = (uint8_t)((int8_t)tjb + (int8_t)c.tbm);
    int dp[C];
#pragma unroll
    for (int k = 0; k < C; k++) dp[k] = 0;
    int xJ = 0;
    int xB = satu8(c.base - tjbm);
    bool overflow = false;
    const int ph = threadIdx.x & 63;
    int rbuf = (ph < L) ? (int)s[ph] : 0, rnext = 0;          // residues 64 rows at a time, a lane each, the next 64 in flight (see fwd_wave_kernel)
    for (int i = 0; i < L; i++) {
      const int j = i & 63;
      if (j == 0) { const int q = i + 64 + ph; rnext = (q < L) ? (int)s[q] : 0; }
      const int x = min(__builtin_amdgcn_readlane(rbuf, j), kKp - 1);
      if (j == 63) rbuf = rnext;
      const uint8_t *row = rb + (size_t)x * rb_stride;
      int prev = wave_shr1_i32(dp[C - 1], 0);
      int xE = 0;
#pragma unroll
      for (int k = 0; k < C; k++) {
        const int node = lane * C + k + 1;
        const int cost = (node <= M) ? (int)row[node] : 255;
        int sv = max(prev, xB);
        sv = satu8(sv + c.bias);
        sv = satu8(sv - cost);
        prev = dp[k];
        dp[k] = sv;
        xE = max(xE, sv);
      }
      xE = wave_max_i32(xE);
      if (satu8(xE + c.bias) == 255) { overflow = true; break; }
      xE = satu8(xE - c.tec);
      xJ = max(xJ, xE);
      xB = satu8(max(c.base, xJ) - tjbm);
    }
    if (lane == 0) {
      if (overflow) { sc[sid] = INFINITY; status[sid] = BATH_ERANGE; }
      else {
        float r = ((float)(xJ - tjb) - (float)c.base);
        r /= c.scale_b;
        r = (float)((double)r - 3.0);
        sc[sid] = r; status[sid] = BATH_OK;
      }
    }
  }
