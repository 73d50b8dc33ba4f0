// bath_fs3_fwd_chain_rows.hpp -- the body of the strict 3-codon Forward parser's chain kernels: no header, a function body, included
// by bath_fs_chain.hip inside fs3_fwd_chain_kernel<C> and fs3_fwd_batch_kernel<C> (the reason is told there).  It reads, as the
// including kernel names them: C; dna, p, loop_tab, move_tab, tEL, tEM, sc, xmx, xmx_off (xmx null: scores only), jobs, W.
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float *s_tbl = reinterpret_cast<float *>(lds);
  float *s_tf = s_tbl + kLogsumTbl;
  const int M = p.M;
  const int stride = fs_chain_stride(C);
  float *s_stage = s_tf + (M + 2) * 8;                          // [W][2][stride]
  float *s_e = s_stage + (size_t)W * 2 * stride;                // [W][2] E(i) of the pair's rows
  int *s_ctl = reinterpret_cast<int *>(s_e + 2 * kChainMaxWaves);   // [0]: first job of the block's batch; [4]: the row pair whose serial part is done
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
    const int Lmax = dna.len[jobs.order[base]];                 // the batch's longest window (the list is sorted by length)
    const int L = job >= 0 ? dna.len[job] : 0;
    const uint8_t *d = job >= 0 ? dna.data + dna.off[job] : dna.data;
    float *xo = (xmx && job >= 0) ? xmx + xmx_off[job] : nullptr;
    const int Lc = L / 3;
    const float tNL = loop_tab[Lc], tNM = move_tab[Lc], tJL = tNL, tJM = tNM, tCL = tNL, tCM = tNM;
    // rows i-1 ("1"), i-2 ("2"), i-3 ("3") of the pair (i, i+1)
    float M1[C], I1[C], D1[C], M2[C], I2[C], D2[C], M3[C], I3[C], iv_1[C], iv_2[C];
#pragma unroll
    for (int c = 0; c < C; c++) M1[c] = I1[c] = D1[c] = M2[c] = I2[c] = D2[c] = M3[c] = I3[c] = iv_1[c] = iv_2[c] = -INFINITY;
    float N1 = 0.f, N2 = 0.f, N3 = 0.f, J1 = -INFINITY, J2 = -INFINITY, J3 = -INFINITY, C1 = -INFINITY, C2 = -INFINITY, C3 = -INFINITY;
    float B1 = tNM, B2 = tNM;                                   // B(i-1), B(i-2)
    if (xo && lane == 0 && L >= 3)
      for (int i = 0; i < 2; i++) { xo[i * 5 + 0] = -INFINITY; xo[i * 5 + 1] = 0.f; xo[i * 5 + 2] = -INFINITY; xo[i * 5 + 3] = tNM; xo[i * 5 + 4] = -INFINITY; }
    auto nuc = [&](int i) -> int { return (i >= 1 && i <= L) ? ((d[i - 1] < 4) ? (int)d[i - 1] : 338) : 338; };   // x_i; 338 = p7P_MAXCODONS3 (degenerate / outside)
    for (int i = 2; i <= Lmax; i += 2) {
      ++pair;
      if (wv >= W) { lds_barrier(); chain_keepalive(s_ctl + 4, pair); lds_barrier(); continue; }   // a poller without a window
      const bool actA = job >= 0 && L >= 3 && i <= L, actB = job >= 0 && L >= 3 && i + 1 <= L;
      // ---- emission rows of the pair: codon lengths 2, 3, 4 ending at x_i (row A) and x_{i+1} (row B)
      const int xa = nuc(i), wa = nuc(i - 1), va = nuc(i - 2), ua = nuc(i - 3), xb = nuc(i + 1);
      const float *qa2 = p.rsc + (size_t)imin(xa * 84 + wa * 21, 337) * p.pitch;
      const float *qa3 = p.rsc + (size_t)imin(xa * 84 + wa * 21 + va * 5 + 1, 336) * p.pitch;
      const float *qa4 = p.rsc + (size_t)imin(xa * 84 + wa * 21 + va * 5 + ua + 2, 337) * p.pitch;
      const float *qb2 = p.rsc + (size_t)imin(xb * 84 + xa * 21, 337) * p.pitch;
      const float *qb3 = p.rsc + (size_t)imin(xb * 84 + xa * 21 + wa * 5 + 1, 336) * p.pitch;
      const float *qb4 = p.rsc + (size_t)imin(xb * 84 + xa * 21 + wa * 5 + va + 2, 337) * p.pitch;
      // ---- 1. everything of both rows that is parallel over the nodes
      const float mInA = wave_shr1(M2[C - 1], -INFINITY), iInA = wave_shr1(I2[C - 1], -INFINITY), dInA = wave_shr1(D2[C - 1], -INFINITY);
      const float mInB = wave_shr1(M1[C - 1], -INFINITY), iInB = wave_shr1(I1[C - 1], -INFINITY), dInB = wave_shr1(D1[C - 1], -INFINITY);
      float MA[C], IA[C], ivA[C], MB[C], IB[C], ivB[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1, nd = imin(node, M + 1), ne = imin(node, M);
        const float4 ta = *reinterpret_cast<const float4 *>(s_tf + nd * 8);
        const float4 tb = *reinterpret_cast<const float4 *>(s_tf + nd * 8 + 4);
        const bool in = node <= M;
        // (no branches in this loop: loads and stores are unconditional -- the slots past node M exist -- so that the log-sums of
        // a lane's C nodes, independent of each other, can be interleaved)
        const float la2 = qa2[ne], la3 = qa3[ne], la4 = qa4[ne], lb2 = qb2[ne], lb3 = qb3[ne], lb4 = qb4[ne];
        const float ea2 = in ? la2 : -INFINITY, ea3 = in ? la3 : -INFINITY, ea4 = in ? la4 : -INFINITY;
        const float eb2 = in ? lb2 : -INFINITY, eb3 = in ? lb3 : -INFINITY, eb4 = in ? lb4 : -INFINITY;
        // row A = i: from row i-2 and B(i-2) (:562-569); row 2 takes B(0) only (:503)
        const float mA = (c == 0) ? mInA : M2[c - 1], iA = (c == 0) ? iInA : I2[c - 1], dA = (c == 0) ? dInA : D2[c - 1];
        float a = LS(mA + ta.x, LS(iA + ta.y, LS(dA + ta.z, B2 + ta.w)));
        // (row 2 takes B(0) only (:503): rows 0 and 1 are -inf, and LS(-inf, x) = x exactly)
        ivA[c] = a;
        float mv = a + ea2;
        mv = LS(mv, iv_1[c] + ea3); mv = LS(mv, iv_2[c] + ea4);      // :571-574 (row 2: the IVX of rows 1, 0 are -inf)
        MA[c] = mv;
        const float insA = LS(M3[c] + tb.z, I3[c] + tb.w);
        IA[c] = (i > 2 && node < M) ? insA : -INFINITY;
        // row B = i+1: from row i-1 and B(i-1); its 3- and 4-nucleotide codons start in rows i and i-1
        const float mB = (c == 0) ? mInB : M1[c - 1], iB = (c == 0) ? iInB : I1[c - 1], dB = (c == 0) ? dInB : D1[c - 1];
        const float b = LS(mB + ta.x, LS(iB + ta.y, LS(dB + ta.z, B1 + ta.w)));
        ivB[c] = b;
        float mw = b + eb2;
        mw = LS(mw, a + eb3); mw = LS(mw, iv_1[c] + eb4);
        MB[c] = mw;
        const float insB = LS(M2[c] + tb.z, I2[c] + tb.w);
        IB[c] = (node < M) ? insB : -INFINITY;
        s_stage[((size_t)wv * 2 + 0) * stride + node] = mv; s_stage[((size_t)wv * 2 + 1) * stride + node] = mw;
      }
      lds_barrier();
      // ---- 2. the serial part, a lane per row: D(i,k) = LS(M(i,k-1) + tMD, D(i,k-1) + tDD), E(i) = LS(M(i,k), LS(D(i,k), E)) (:577-590)
      if (wv == 0 && lane < 2 * W) {
        float *st = s_stage + (size_t)lane * stride;
        float dch = -INFINITY, ech = -INFINITY;
        // the loop's own loads (M(i,k), the transitions) are a node ahead: what a node waits for is the chain's log-sums only
        // (slot M+1 of the row and of the transitions exists: the loads run a node ahead)
        FwdChainRegs r{ech, dch, st[1], s_tf[1 * 8 + 4], s_tf[1 * 8 + 5], lds_addr(st + 1), lds_addr(s_tf + 2 * 8 + 4)};   // tMD(k), tDD(k)
        fwd_chain_nodes(r, M, lds_addr(s_tbl), 15.999f);
        ech = r.e; dch = r.d;
        s_e[lane] = ech;
      }
      if (wv == 0) chain_done(s_ctl + 4, pair); else if (chain_poller(wv)) chain_keepalive(s_ctl + 4, pair);
      lds_barrier();
      // ---- 3. D and E back to the window's wave; special states of both rows (:592-603)
      float DA[C], DB[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        const int node = lane * C + c + 1, ne = imin(node, M);
        const float da = s_stage[((size_t)wv * 2 + 0) * stride + ne], db = s_stage[((size_t)wv * 2 + 1) * stride + ne];
        DA[c] = (node <= M) ? da : -INFINITY; DB[c] = (node <= M) ? db : -INFINITY;
      }
      const float EA = s_e[wv * 2 + 0], EB = s_e[wv * 2 + 1];
      float NA, JA, CA;
      if (i == 2) { NA = 0.f; JA = EA + tEL; CA = EA + tEM; }
      else { NA = N3 + tNL; JA = LS(J3 + tJL, EA + tEL); CA = LS(C3 + tCL, EA + tEM); }
      const float BA = LS(NA + tNM, JA + tJM);
      const float NB = N2 + tNL, JB = LS(J2 + tJL, EB + tEL), CB = LS(C2 + tCL, EB + tEM);
      const float BB = LS(NB + tNM, JB + tJM);
      if (xo && lane == 0) {
        if (actA) { float *r = xo + (size_t)i * 5; r[0] = EA; r[1] = NA; r[2] = JA; r[3] = BA; r[4] = CA; }
        if (actB) { float *r = xo + (size_t)(i + 1) * 5; r[0] = EB; r[1] = NB; r[2] = JB; r[3] = BB; r[4] = CB; }
      }
      if (actB) {                                               // both rows exist: the rings move by two
        N3 = N1; N2 = NA; N1 = NB; J3 = J1; J2 = JA; J1 = JB; C3 = C1; C2 = CA; C1 = CB; B2 = BA; B1 = BB;
#pragma unroll
        for (int c = 0; c < C; c++) {
          M3[c] = M1[c]; I3[c] = I1[c]; M2[c] = MA[c]; I2[c] = IA[c]; D2[c] = DA[c]; M1[c] = MB[c]; I1[c] = IB[c]; D1[c] = DB[c];
          iv_2[c] = ivA[c]; iv_1[c] = ivB[c];
        }
      } else if (actA) {                                        // the window's last row: only C(L), C(L-1), C(L-2) are still needed
        C3 = C2; C2 = C1; C1 = CA;
      }
    }
    if (job >= 0 && lane == 0) sc[job] = (L >= 3) ? LS(C1, LS(C2 + tCL, C3 + tCL)) + tCM : -INFINITY;
    __syncthreads();                                            // s_ctl is rewritten at the top
  }
#undef LS
