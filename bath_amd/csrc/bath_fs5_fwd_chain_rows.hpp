// bath_fs5_fwd_chain_rows.hpp -- the body of the strict 5-codon Forward chain kernels: no header, a function body, included by
// bath_fs_chain.hip inside fs5_fwd_chain_kernel<C, THREADS, STORE> and fs5_fwd_parser_batch_kernel<C, THREADS> (the reason is told at
// fs3_fwd_chain_kernel).  It reads, as the including kernel names them: C, STORE; dna, p, loop_tab, move_tab, tEL, tEM, c5_compat, sc,
// fwd, fwd_off, xmx, xmx_off, done (STORE false: none of the five is read), cfg_len, jobs, W.
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_tbl = reinterpret_cast<float *>(lds);
  float *s_tf = s_tbl + kLogsumTbl;
  const int M = p.M;
  const int stride = fs_chain_stride(C);
  float *s_stage = s_tf + (M + 2) * 8;                          // [W][2][stride]; row 0 of each pair of slots is used
  float *s_e = s_stage + (size_t)W * 2 * stride;
  int *s_ctl = reinterpret_cast<int *>(s_e + 2 * kChainMaxWaves);   // [0]: first job of the block's batch; [4]: the row whose serial part is done
  if (threadIdx.x == 0) s_ctl[4] = 0;
  int pair = 0;
  fs_load_logsum_table(s_tbl, p.logsum);
  for (int i = threadIdx.x; i < (M + 2) * 8; i += blockDim.x) s_tf[i] = p.tf[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#define LS(a, b) flogsum<false>((a), (b), s_tbl)
  for (;;) {
    if (threadIdx.x == 0) s_ctl[0] = (int)atomicAdd(jobs.counter, (unsigned)W);
    __syncthreads();
    const int64_t base = s_ctl[0];
    if (base >= dna.n) break;
    const int64_t job = (wv < W && base + wv < dna.n) ? (int64_t)jobs.order[base + wv] : (int64_t)-1;
    const int Lmax = dna.len[jobs.order[base]];
    const int L = job >= 0 ? dna.len[job] : 0;
    const bool live = job >= 0 && L >= 5;
    const uint8_t *d = job >= 0 ? dna.data + dna.off[job] : dna.data;
    float *fo = (STORE && job >= 0) ? fwd + fwd_off[job] : fwd;
    float *xo = (STORE && job >= 0) ? xmx + xmx_off[job] : xmx;
    const int Lc = cfg_len >= 0 ? cfg_len : L / 3;
    const float tNL = loop_tab[Lc], tNM = move_tab[Lc], tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    float Mr0[C], Mr1[C], Mr2[C], Ir0[C], Ir1[C], Ir2[C], Dr1[C], iv0[C], iv1[C], iv2[C], iv3[C];   // M, I of rows i-1..i-3; D of row i-1; IVX(i-1..i-4)
#pragma unroll
    for (int c = 0; c < C; c++) Mr0[c] = Mr1[c] = Mr2[c] = Ir0[c] = Ir1[c] = Ir2[c] = Dr1[c] = iv0[c] = iv1[c] = iv2[c] = iv3[c] = -INFINITY;
    if (STORE && live) {
      for (int k = lane; k <= M; k += 64)
#pragma unroll
        for (int q = 0; q < 8; q++) fo[(size_t)k * 8 + q] = -INFINITY;
      if (lane == 0) { xo[0] = -INFINITY; xo[1] = 0.f; xo[2] = -INFINITY; xo[3] = tNM; xo[4] = -INFINITY; }
    }
    float xN0 = 0.f, xN1 = 0.f, xN2 = 0.f, xJ0 = -INFINITY, xJ1 = -INFINITY, xJ2 = -INFINITY, xC0 = -INFINITY, xC1 = -INFINITY, xC2 = -INFINITY;   // rows i-1, i-2, i-3
    float xBprev = tNM;
    auto nuc = [&](int i) -> int { return (i >= 1 && i <= L) ? ((d[i - 1] < 4) ? (int)d[i - 1] : 1367) : 1367; };
    // the emission scores of a row are loaded during the chain of the row before: nothing in a row waits for global memory
    float E1[C], E2[C], E3[C], E4[C], E5[C];
    auto load_emissions = [&](int i) {
      const int x = nuc(i), w = nuc(i - 1), v = nuc(i - 2), u = nuc(i - 3), t = nuc(i - 4);
      const float *r1 = p.rsc + (size_t)imin(x * 341, 1366) * p.pitch;
      const float *r2 = p.rsc + (size_t)imin(x * 341 + w * 85 + 1, 1365) * p.pitch;
      const float *r3 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + 2, 1364) * p.pitch;
      const float *r4 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + u * 5 + 3, 1365) * p.pitch;
      const float *r5 = p.rsc + (size_t)imin(x * 341 + w * 85 + v * 21 + u * 5 + t + 4, 1366) * p.pitch;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int ne = imin(lane * C + c + 1, M);
        E1[c] = r1[ne]; E2[c] = r2[ne]; E3[c] = r3[ne]; E4[c] = r4[ne]; E5[c] = r5[ne];
      }
    };
    load_emissions(1);
    for (int i = 1; i <= Lmax; i++) {
      ++pair;
      if (wv >= W) { lds_barrier(); chain_keepalive(s_ctl + 4, pair); lds_barrier(); continue; }   // a poller without a window
      const bool act = live && i <= L;
      const float mIn = wave_shr1(Mr0[C - 1], -INFINITY), iIn = wave_shr1(Ir0[C - 1], -INFINITY), dIn = wave_shr1(Dr1[C - 1], -INFINITY);
      float Mc[C], Ic[C], ivc[C];
      float *row = STORE ? fo + (size_t)(act ? i : 0) * (M + 1) * 8 : nullptr;
      if (STORE && act && lane == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) row[q] = -INFINITY;
      }
      // The cells of the row, then their stores.  Rows >= 5 (all but four of a window) go through a loop without branches, so that
      // the log-sums of a lane's C nodes -- independent of each other -- are interleaved; the first rows take the general form.
      float q1[C], q2[C], q3[C], q4[C], q5[C];
      auto cells = [&](auto early_tag) {
        constexpr bool EARLY = decltype(early_tag)::value;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int node = lane * C + c + 1, nd = imin(node, M + 1);
          const float4 ta = *reinterpret_cast<const float4 *>(s_tf + nd * 8);
          const float4 tb = *reinterpret_cast<const float4 *>(s_tf + nd * 8 + 4);
          const float m1 = (c == 0) ? mIn : Mr0[c - 1], i1 = (c == 0) ? iIn : Ir0[c - 1], d1 = (c == 0) ? dIn : Dr1[c - 1];
          const float e1 = E1[c], e2 = E2[c], e3 = E3[c], e4 = E4[c], e5 = E5[c];
          float ivn = LS(m1 + ta.x, LS(i1 + ta.y, LS(d1 + ta.z, xBprev + ta.w)));  // :332-335
          if (EARLY && i <= 2) ivn = xBprev + ta.w;                                  // rows 1, 2: only B(i-1) enters (:109, :150)
          ivc[c] = ivn;
          const float c1 = ivn + e1;
          const float c2 = (!EARLY || i >= 2) ? iv0[c] + e2 : -INFINITY;
          const float c3 = (!EARLY || i >= 3) ? iv1[c] + e3 : -INFINITY;
          const float c4 = (!EARLY || i >= 4) ? iv2[c] + e4 : -INFINITY;
          const float c5 = !EARLY ? (c5_compat ? ivn : iv3[c]) + e5 : -INFINITY;
          float c0;
          if (!EARLY) c0 = LS(LS(c1, LS(c2, c3)), LS(c4, c5));
          else if (i == 1) c0 = c1;
          else if (i == 2) c0 = LS(c1, c2);
          else c0 = LS(c1, LS(c2, LS(c3, c4)));
          Mc[c] = c0;
          const float ins = LS(Mr2[c] + tb.z, Ir2[c] + tb.w);
          Ic[c] = ((!EARLY || i >= 3) && node < M) ? ins : -INFINITY;
          q1[c] = c1; q2[c] = c2; q3[c] = c3; q4[c] = c4; q5[c] = c5;
          s_stage[((size_t)wv * 2) * stride + node] = c0;           // (the slots past node M exist)
        }
      };
      if (i >= 5) cells(std::false_type{}); else cells(std::true_type{});
      if (STORE && act) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int node = lane * C + c + 1;
          if (node <= M) {
            float *cell = row + (size_t)node * 8;
            cell[1] = Ic[c]; cell[2] = Mc[c]; cell[3] = q1[c]; cell[4] = q2[c]; cell[5] = q3[c]; cell[6] = q4[c]; cell[7] = q5[c];
          }
        }
      }
      load_emissions(i + 1);
      lds_barrier();
      // ---- the serial part, a lane per window: D(i,k), E(i) in the reference's order; rows >= 5 pair M(i,M) and D(i,M) first (:392-394)
      if (wv == 0 && lane < W) {
        float *st = s_stage + (size_t)lane * 2 * stride;
        float dch = -INFINITY, ech = -INFINITY;
        FwdChainRegs r{ech, dch, st[1], s_tf[1 * 8 + 4], s_tf[1 * 8 + 5], lds_addr(st + 1), lds_addr(s_tf + 2 * 8 + 4)};   // tMD(k), tDD(k)
        fwd_chain_nodes(r, M - 1, lds_addr(s_tbl), 15.999f);
        ech = r.e; dch = r.d;
        const float Mn = r.Mk;                                    // M(i,M)
        st[M] = dch;
        ech = (i >= 5) ? LS(LS(Mn, dch), ech) : LS(Mn, LS(dch, ech));
        s_e[lane] = ech;
      }
      if (wv == 0) chain_done(s_ctl + 4, pair); else if (chain_poller(wv)) chain_keepalive(s_ctl + 4, pair);
      lds_barrier();
      float Dc[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1, ne = imin(node, M);
        const float dv = s_stage[((size_t)wv * 2) * stride + ne];
        Dc[c] = (node <= M) ? dv : -INFINITY;
        if (STORE && act && node <= M) row[(size_t)node * 8] = Dc[c];
      }
      const float xE = s_e[wv];
      float nN, nJ, nC, nB;
      if (i <= 2) { nN = 0.f; nJ = xE + tEL; nC = xE + tEM; nB = tNM; }           // :126-132, :166-167
      else {
        nN = xN2 + tNL; nJ = LS(xJ2 + tJL, xE + tEL); nC = LS(xC2 + tCL, xE + tEM);
        nB = LS(nN + tNM, nJ + tJM);
      }
      if (act) {
        if (STORE && lane == 0) { xo[i * 5 + 0] = xE; xo[i * 5 + 1] = nN; xo[i * 5 + 2] = nJ; xo[i * 5 + 3] = nB; xo[i * 5 + 4] = nC; }
        xN2 = xN1; xN1 = xN0; xN0 = nN; xJ2 = xJ1; xJ1 = xJ0; xJ0 = nJ; xC2 = xC1; xC1 = xC0; xC0 = nC;
        xBprev = nB;
#pragma unroll
        for (int c = 0; c < C; c++) {
          Mr2[c] = Mr1[c]; Mr1[c] = Mr0[c]; Mr0[c] = Mc[c];
          Ir2[c] = Ir1[c]; Ir1[c] = Ir0[c]; Ir0[c] = Ic[c];
          Dr1[c] = Dc[c];
          iv3[c] = iv2[c]; iv2[c] = iv1[c]; iv1[c] = iv0[c]; iv0[c] = ivc[c];
        }
        if (i == L) {                                             // this window is complete: score, then the flag the host waits for
          if (lane == 0) sc[job] = LS(xC0, LS(xC1 + tCL, xC2 + tCL)) + tCM;
          if (STORE && done) { __threadfence_system(); if (lane == 0) __hip_atomic_store(done + job, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
        }
      }
    }
    if (job >= 0 && !live) {
      if (lane == 0) sc[job] = -INFINITY;
      if (STORE && done) { __threadfence_system(); if (lane == 0) __hip_atomic_store(done + job, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
    }
    __syncthreads();
  }
#undef LS
