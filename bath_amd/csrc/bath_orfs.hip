// bath_orfs.hip -- six-frame translation and ORF finding for a block of DNA windows, and the length-sorted
// ORF work list that feeds the lane-per-ORF SSV kernel.
//
// Reference behaviour (easel esl_gencode_ProcessStart/ProcessPiece/ProcessEnd as driven by
// src/bathsearch.c:384-392 with do_watson/do_crick, minimum_length = 20, no initiator requirement): every
// maximal run of non-stop codons of at least <minlen> residues in each of the six frames of a window is one
// ORF; windows shorter than 15 nt are skipped (bathsearch.c:1066).
//
// GPU formulation.  A window is cut into tiles of 384 nt; a quarter wave (16 lanes x 24 nt) owns a tile, so the work
// is parallel over the total sequence length whatever the shape of the block (10^6 windows of 1 kb, or a few
// windows of 256 kb), loads are contiguous across lanes and every stream's residues leave as contiguous dwords.
//   orf_tile_kernel   The three bytes at position p are codon p/3 of forward frame p%3 and, on the other strand, a codon
//                     of reverse frame (n-p)%3 (runs of non-stop codons are the same whichever way a frame is walked,
//                     so reverse frames are scanned in memory order too).  Canonical ACGT codons are decoded by one
//                     24-bit multiply + bit-field extract + one 64-entry LDS table for both strands, degenerate codes by the
//                     general 18^3 table.  Per stream, the length of the stop-free run entering each lane's eight codons
//                     comes from a DPP running maximum over the tile's 16-lane row (the last stop before the lane); runs closed by two stops inside the tile are recorded as ORFs
//                     at once, the run touching the tile's left edge ("prefix") and the one open at its right edge
//                     ("suffix") are left in the tile summary.  Positions past the end of a stream count as stops.
//   orf_stitch_kernel one lane per (window, frame) walks the tile summaries and records the ORFs that cross tiles.
//   orf_scan_bins     turns the ORF length histogram into start offsets, longest ORFs first.
//   orf_sort_kernel   compacts the per-tile records into the dense work list ordered by length (block-local counting
//                     sort over a block's records read once by the whole block: one global atomic per block and non-empty bin).
// Amino stream of (w, sf):  aa + 2*off[w] + 96*w + sf*pitch(n),  pitch(n) = (n/3 + 16) & ~15   (closed form: no prefix sums)
#include <algorithm>
#include <climits>
#include <cstring>

#include "bath_common.hpp"
#include "bath_kernels.hpp"
#include "bath_launch.hpp"

namespace bath {

constexpr int kTileLanes = 16;                 // a quarter wave owns a tile: exactly one 16-lane DPP row
constexpr int kLaneCodons = 8;                 // codons per stream and lane
constexpr int kLaneNt = 3 * kLaneCodons;       // nucleotides per lane (it reads two more: its last codons run into the next lane's bytes)
constexpr int kTileCodons = kLaneCodons * kTileLanes;    // scan positions per stream and tile
constexpr int kTileNt = kLaneNt * kTileLanes;

struct OrfScanTables {
  const uint8_t *aa_full;   // [5832] (a*18+b)*18+c -> amino code, degenerate codons resolved (esl_gencode_GetTranslation)
  const uint8_t *aa64_fwd;  // [64] a<<4|b<<2|c for canonical codons
  const uint8_t *aa64_rev;  // [64] x0<<4|x1<<2|x2 of the three bytes in memory order -> amino code of the reverse-complement codon
  const uint8_t *comp;      // [18]
};

struct OrfTiles {
  const int4 *desc;           // [ntiles] {offset of the window in the DNA block / 16, window length, window, tile index within the window}
  const int32_t *tile_first;  // [nwin] first tile of each window
  int64_t ntiles;
};

struct OrfScanOut {
  uint8_t *aa;              // amino-acid streams
  uint2 *slots;             // [ntiles][cap] {first codon index within its stream, length | (strand*3+frame) << 28}
  int32_t *cnt;             // [ntiles] ORFs recorded per tile
  uint2 *cross;             // [ntiles*6] the ORF that ends at the first stop of (tile, frame) and began in an earlier tile; length 0: none
  int32_t *prefix, *suffix; // [ntiles*6] tile summaries: stop-free run at the left / right edge (kTileCodons: no stop in the tile)
  int *hist;                // [kOrfBins] ORF length histogram (lengths above the last bin are clamped into it)
  unsigned long long *n_orfs, *orf_res;
  int cap;
  int count;                // 0: leave the histogram and the two counters alone (orf_filter_kernel recounts what it keeps)
};

// One strand only (pli->strands) and / or initiation codons (bathsearch -m / -M): applied to the records of the two scan kernels
// before the sort.  Off in bathsearch's default configuration (both strands, any codon starts an ORF), where the pass is skipped.
struct OrfFilter {
  int strands;              // BATH_STRAND_*
  int using_initiators;     // -m or -M: ORFs start at an initiation codon, translated as M
  const uint8_t *is_init;   // [64] canonical codon (16a + 4b + c) -> may initiate
  const uint8_t *comp;      // [18] complement
};

__device__ __forceinline__ int orf_bin(int len) { return min(len, kOrfBins - 1); }

// Exclusive running maximum over the 16 lanes of a DPP row (lane 0 of a row gets <ident>): row_shr:1, then row_shr 1/2/4/8 of the
// shifted value.  5 VALU instructions once the identity is INT_MIN (the compiler folds each step into one v_max_i32_dpp; with
// another identity it emits mov + dpp-mov + max).  A tile is one row, so nothing crosses rows.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_or_ident(int v, int ident) { return __builtin_amdgcn_update_dpp(ident, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int row_excl_max_scan(int v, int ident) {
  int x = dpp_or_ident<0x111>(v, ident);                           // row_shr:1
  x = max(x, dpp_or_ident<0x111>(x, ident));                       // row_shr:1
  x = max(x, dpp_or_ident<0x112>(x, ident));                       // row_shr:2
  x = max(x, dpp_or_ident<0x114>(x, ident));                       // row_shr:4
  x = max(x, dpp_or_ident<0x118>(x, ident));                       // row_shr:8
  return x;
}

__global__ __launch_bounds__(256, 5) void orf_tile_kernel(SeqView dna, OrfTiles tiles, OrfScanTables tabs, OrfScanOut out, int minlen) {
  __shared__ int s_hist[kOrfBins];
  __shared__ __attribute__((aligned(16))) uint8_t s_full[5832 + 8];
  __shared__ uint16_t s_fr[64];                                // canonical codon -> forward amino acid | reverse-strand amino acid << 8, bit 7 of each = stop
  __shared__ uint8_t s_comp[32];
  __shared__ unsigned s_red[2];
  // per quarter wave, for the current tile: [0..5] prefix and [6..11] suffix of the six frames, [12] ORFs recorded.  The tile's
  // summary leaves as ONE store instruction of 13 lanes: the kernel is bound by the number of memory instructions it issues
  // (DESIGN 4.0), and twelve single-lane stores per tile cost as much there as twelve full ones.
  __shared__ int s_sum[256 / kTileLanes][16];
  for (int i = threadIdx.x; i < kOrfBins; i += blockDim.x) s_hist[i] = 0;
  for (int i = threadIdx.x; i < 5832; i += blockDim.x) s_full[i] = tabs.aa_full[i];
  if (threadIdx.x < 64) {
    const unsigned f = tabs.aa64_fwd[threadIdx.x], r = tabs.aa64_rev[threadIdx.x];
    s_fr[threadIdx.x] = (uint16_t)((f | (f == kStop ? 0x80u : 0u)) | ((r | (r == kStop ? 0x80u : 0u)) << 8));
  }
  if (threadIdx.x < 18) s_comp[threadIdx.x] = tabs.comp[threadIdx.x];
  if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
  __syncthreads();
  const int qw = threadIdx.x / kTileLanes;                     // quarter wave within the block
  const int i = threadIdx.x % kTileLanes;                      // lane within the tile
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  unsigned my_orfs = 0, my_res = 0;
  // Software pipeline over this wave's tiles (four per iteration, one per quarter wave): descriptors are fetched two tiles ahead
  // and the lane's 26 bytes of DNA one tile ahead, so the dependent loads (descriptor -> sequence data) of a tile are in flight
  // while the previous one computes.
  const int quarter = (threadIdx.x & 63) / kTileLanes;
  const int4 none = {0, 0, 0, 0};
  auto fetch_desc = [&](int64_t tb) { const int64_t t = tb + quarter; return t < tiles.ntiles ? tiles.desc[t] : none; };
  auto fetch_data = [&](const int4 &dsc, uint32_t (&D)[7]) {
    const int p0 = kTileNt * dsc.w + kLaneNt * i;
#pragma unroll
    for (int k = 0; k < 7; k++) D[k] = 0u;
    const uint8_t *d = dna.data + ((int64_t)(uint32_t)dsc.x << 4) + p0;   // 8-byte aligned: windows start on 16, p0 is a multiple of 8
    // no load starts at or past the window end, so none reaches further than 7 bytes beyond it
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (p0 + 8 * k < dsc.y) { const uint2 v = *reinterpret_cast<const uint2 *>(d + 8 * k); D[2 * k] = v.x; D[2 * k + 1] = v.y; }
    if (p0 + 24 < dsc.y) D[6] = *reinterpret_cast<const uint32_t *>(d + 24);
  };
  const int64_t tstep = nwaves * 4;
  int4 d_next = fetch_desc(wave0 * 4), d_next2 = fetch_desc(wave0 * 4 + tstep);
  uint32_t D_next[7];
  fetch_data(d_next, D_next);
  for (int64_t tb = wave0 * 4; tb < tiles.ntiles; tb += tstep) {
    const int64_t tile = tb + quarter;
    const int4 dsc = d_next;
    uint32_t D[7];
#pragma unroll
    for (int k = 0; k < 7; k++) D[k] = D_next[k];
    d_next = d_next2;
    d_next2 = fetch_desc(tb + 2 * tstep);
    fetch_data(d_next, D_next);
    const int n = dsc.y;                                       // n >= 15 for every window that has tiles; 0: no tile for this quarter wave
    const bool live = n > 0;
    const int w = dsc.z, T = dsc.w;
    const int64_t off = (int64_t)(uint32_t)dsc.x << 4;
    const int p0 = kTileNt * T + kLaneNt * i;
    if (i == 0) s_sum[qw][12] = 0;
    // ---- bytes past the window end read as 0 (they only feed positions that count as stops, but the padding between windows is
    // not a nucleotide code and would send the wave down the degenerate path): dword k keeps its low clamp(n - p0 - 4k, 0, 4) bytes
    const int rem8 = 8 * min(n - p0, 32);
#pragma unroll
    for (int k = 0; k < 7; k++) {
      const int t8 = min(max(rem8 - 32 * k, 0), 32);
      D[k] &= (uint32_t)((0xffffffffull << t8) >> 32);
    }
    const bool canonical = ((D[0] | D[1] | D[2] | D[3] | D[4] | D[5] | (D[6] & 0xffffu)) & 0xfcfcfcfcu) == 0u;
    // The 16-bit table entries of codon k (bytes k .. k+2 of the lane) stay whole, forward amino acid in the low byte and the
    // reverse strand's in the high byte, a stop flag in bit 7 of each.  Codon k belongs to phase k % 3 and is codon c = k / 3 of
    // that phase's streams; W[4 ph + c / 2] holds the entries of codons c, c + 1 (c even) in its low and high half.
    unsigned W[12];
    if (__all(canonical)) {
      unsigned e[24];
#pragma unroll
      for (int k = 0; k < 24; k++) {
        const unsigned t = (k % 4 == 0) ? D[k / 4] : __builtin_amdgcn_alignbyte(D[k / 4 + 1], D[k / 4], k % 4);
        // bytes x0,x1,x2 < 4 at bits 0,8,16: t * (2^21 + 2^11 + 2) has (x0<<4|x1<<2|x2) << 1, the byte offset of the codon's
        // 16-bit entry, at bits 16..22 (bit 16 is always 0) and nothing else there
        const unsigned boff = (__umul24(t, 0x200802u) >> 16) & 127u;
        e[k] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(s_fr) + boff);
      }
#pragma unroll
      for (int q = 0; q < 12; q++) W[q] = e[q / 4 + 6 * (q % 4)] | (e[q / 4 + 6 * (q % 4) + 3] << 16);
    } else {
      unsigned e[24];
#pragma unroll
      for (int k = 0; k < 24; k++) {
        const unsigned t = (k % 4 == 0) ? D[k / 4] : __builtin_amdgcn_alignbyte(D[k / 4 + 1], D[k / 4], k % 4);
        const int x0 = min((int)(t & 0xffu), 17), x1 = min((int)((t >> 8) & 0xffu), 17), x2 = min((int)((t >> 16) & 0xffu), 17);
        const unsigned f = s_full[(x0 * 18 + x1) * 18 + x2];
        const unsigned r = s_full[((int)s_comp[x2] * 18 + (int)s_comp[x1]) * 18 + (int)s_comp[x0]];
        e[k] = (f | (f == kStop ? 0x80u : 0u)) | ((r | (r == kStop ? 0x80u : 0u)) << 8);
      }
#pragma unroll
      for (int q = 0; q < 12; q++) W[q] = e[q / 4 + 6 * (q % 4)] | (e[q / 4 + 6 * (q % 4) + 3] << 16);
    }
    const int nvalid = live ? min(max(n - 2 - p0, 0), kLaneNt) : 0;      // positions p0 .. p0+nvalid-1 start a codon inside the window
    const int pitch = orf_stream_pitch(n);
    uint8_t *const abase = out.aa + (2 * off + 96 * (int64_t)w);
    const int u0 = kTileCodons * T + kLaneCodons * i;                    // scan index of the lane's first codon, every stream
    // A stream's eight residues are picked out of its four W words in the order they are stored: codons 0..7 for a forward stream,
    // 7..0 for a reverse one (its codon index runs against memory order).  Their flag bits 7, 15, .. 63 are the stream's stops, one
    // 64-bit mask in the same order.  Codons past the end of the stream count as stops: cv = how many of the eight exist
    // (x / 3 = x * 43 >> 7 for x < 128), the flags of the others are forced, from the top of the mask (forward) or its bottom (reverse).
    unsigned long long inv_f[3], inv_r[3];
    int cv[3];
#pragma unroll
    for (int ph = 0; ph < 3; ph++) {
      cv[ph] = ((nvalid - ph + 2) * 43) >> 7;
      inv_f[ph] = cv[ph] >= kLaneCodons ? 0ull : (0x8080808080808080ull << (8 * cv[ph]));
      inv_r[ph] = cv[ph] >= kLaneCodons ? 0ull : (0x8080808080808080ull >> (8 * cv[ph]));
    }
    // n = 3 q3 + r3 once per tile: the reverse frame of phase ph is (r3 - ph) mod 3 and that stream has q3 - (r3 < ph) codons,
    // without a division per stream
    const int q3 = n / 3, r3 = n - 3 * q3;
    uint2 *const slots = out.slots + tile * out.cap;                     // per tile, not per stream
    int *const prefix6 = &s_sum[qw][0], *const suffix6 = &s_sum[qw][6];
#pragma unroll
    for (int st = 0; st < 6; st++) {                                      // st: phase 0..2 forward, 3..5 the same phases on the other strand
      const int ph = st % 3;
      const bool rev = st >= 3;
      const int fr = r3 - ph + (r3 < ph ? 3 : 0);                         // reverse frame of phase ph in this window: (n - ph) mod 3
      const int sf = rev ? 3 + fr : ph;                                   // strand*3 + frame as reported
      const int C = q3 - 1 - (r3 < ph ? 1 : 0);                           // (n - 3 - fr - ph) / 3; reverse stream: codon index j = C - u
      // v_perm_b32 picks the forward (even) or the reverse-strand (odd) bytes of four codons out of two W words
      const unsigned lo = rev ? __builtin_amdgcn_perm(W[4 * ph + 3], W[4 * ph + 2], 0x01030507u) : __builtin_amdgcn_perm(W[4 * ph + 1], W[4 * ph + 0], 0x06040200u);
      const unsigned hi = rev ? __builtin_amdgcn_perm(W[4 * ph + 1], W[4 * ph + 0], 0x01030507u) : __builtin_amdgcn_perm(W[4 * ph + 3], W[4 * ph + 2], 0x06040200u);
      // stops in stored order (byte b is codon b of a forward stream, codon 7 - b of a reverse one), counting positions past the end
      const unsigned long long mf = (((unsigned long long)(hi & 0x80808080u) << 32) | (unsigned long long)(lo & 0x80808080u)) | (rev ? inv_r[ph] : inv_f[ph]);
      // ---- residues out: two dwords per lane when all eight codons exist
      const int so = sf * pitch + (rev ? C - u0 - (kLaneCodons - 1) : u0);     // 32-bit offset of the lane's first stored byte in this tile's window
      uint8_t *const ap = abase + so;
      const unsigned lo7 = lo & 0x7f7f7f7fu, hi7 = hi & 0x7f7f7f7fu;
      if (cv[ph] == kLaneCodons) {
        *reinterpret_cast<uint32_t *>(ap) = lo7;                            // a reverse stream's address has no alignment to speak of
        *reinterpret_cast<uint32_t *>(ap + 4) = hi7;
      } else if (cv[ph] > 0) {
        // a lane that is only partly inside the window: its cv residues are the low bytes of a forward stream's eight and the top
        // bytes of a reverse stream's, stored as 4 + 2 + 1 bytes (three store instructions at the most, not seven)
        unsigned long long v = ((unsigned long long)hi7 << 32) | lo7;
        uint8_t *q = ap;
        if (rev) { v >>= 8 * (kLaneCodons - cv[ph]); q += kLaneCodons - cv[ph]; }
        if (cv[ph] & 4) { *reinterpret_cast<uint32_t *>(q) = (uint32_t)v; v >>= 32; q += 4; }
        if (cv[ph] & 2) { *reinterpret_cast<uint16_t *>(q) = (uint16_t)v; v >>= 16; q += 2; }
        if (cv[ph] & 1) *q = (uint8_t)v;
      }
      // ---- length of the stop-free run entering this lane's eight codons: scan position of the last stop before them in the tile
      const bool any = mf != 0ull;
      const int b_top = (63 - (int)__clzll((long long)mf)) >> 3, b_bot = (__ffsll((long long)mf) - 1) >> 3;   // highest / lowest flagged byte (any only)
      const int c_last = rev ? kLaneCodons - 1 - b_bot : b_top;           // the lane's last and first stop, as codons 0..7
      const int c_first = rev ? kLaneCodons - 1 - b_top : b_bot;
      const int mine = any ? kLaneCodons * i + c_last : INT_MIN;          // scan position of this lane's last stop
      const int last = row_excl_max_scan(mine, INT_MIN);
      bool open = last < 0;                                               // no stop in the tile before this lane
      const int run_in = open ? kLaneCodons * i : kLaneCodons * i - 1 - last;
      auto record = [&](int u_stop, int len) {
        const int k = atomicAdd(&s_sum[qw][12], 1);
        slots[k] = make_uint2((unsigned)(rev ? C - u_stop + 1 : u_stop - len), (unsigned)len | ((unsigned)sf << 28));
        atomicAdd(&s_hist[orf_bin(len)], 1);
        my_orfs++; my_res += (unsigned)len;
      };
      if (minlen > kLaneCodons - 2) {
        // a run that starts after a stop inside these eight codons and ends at another is at most 6 long: only the lane's first
        // stop can close an ORF
        if (any) {
          const int len = run_in + c_first;
          if (open) { if (live) prefix6[sf] = len; }
          else if (live && len >= minlen) record(u0 + c_first, len);
        }
        if (live && i == kTileLanes - 1) {
          suffix6[sf] = any ? kLaneCodons - 1 - c_last : run_in + kLaneCodons;   // the run open at the tile's right edge
          if (open && !any) prefix6[sf] = kTileCodons;                     // no stop anywhere in the tile
        }
      } else {
        int len = run_in;
#pragma unroll
        for (int c = 0; c < kLaneCodons; c++) {
          if ((mf >> (8 * (rev ? kLaneCodons - 1 - c : c) + 7)) & 1ull) {
            if (open) { if (live) prefix6[sf] = len; open = false; }
            else if (live && len >= minlen) record(u0 + c, len);
            len = 0;
          } else len++;
        }
        if (live && i == kTileLanes - 1) {
          suffix6[sf] = len;
          if (open) prefix6[sf] = kTileCodons;
        }
      }
    }
    // every (tile, frame) got its prefix from exactly one lane and its suffix from lane 15; LDS operations of one wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (live && i < 13) {
      int *const dst = i < 6 ? out.prefix + tile * 6 + i : i < 12 ? out.suffix + tile * 6 + (i - 6) : out.cnt + tile;
      *dst = s_sum[qw][i];
    }
  }
  if (my_orfs) { atomicAdd(&s_red[0], my_orfs); atomicAdd(&s_red[1], my_res); }
  __syncthreads();
  if (!out.count) return;
  for (int k = threadIdx.x; k < kOrfBins; k += blockDim.x) if (s_hist[k]) atomicAdd(&out.hist[k], s_hist[k]);
  if (threadIdx.x == 0 && s_red[0]) { atomicAdd(out.n_orfs, (unsigned long long)s_red[0]); atomicAdd(out.orf_res, (unsigned long long)s_red[1]); }
}

// ORFs that cross tile edges: one lane per (window, frame) walks the summaries of the window's tiles
__global__ __launch_bounds__(256) void orf_stitch_kernel(SeqView dna, OrfTiles tiles, OrfScanOut out, int minlen) {
  __shared__ int s_hist[kOrfBins];
  __shared__ unsigned s_red[2];
  for (int i = threadIdx.x; i < kOrfBins; i += blockDim.x) s_hist[i] = 0;
  if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
  __syncthreads();
  unsigned my_orfs = 0, my_res = 0;
  const int64_t nstreams = dna.n * 6;
  for (int64_t sidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sidx < nstreams; sidx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w = sidx / 6;
    const int sf = (int)(sidx - w * 6);
    const int n = dna.len[w];
    if (n < 15) continue;
    const int nt = (n / 3) / kTileCodons + 1;
    const int64_t first = tiles.tile_first[w];
    const bool rev = sf >= 3;
    const int fr = rev ? sf - 3 : 0;
    const int ph = rev ? (n - fr) % 3 : sf;
    const int C = (n - 3 - fr - ph) / 3;
    int carry = 0;
    for (int T = 0; T < nt; T++) {
      const int64_t e = (first + T) * 6 + sf;
      const int p = out.prefix[e];
      if (p < kTileCodons) {
        const int len = carry + p;
        uint2 none = make_uint2(0u, 0u);
        if (len < minlen) out.cross[e] = none;
        else {
          const int u_stop = kTileCodons * T + p;
          out.cross[e] = make_uint2((unsigned)(rev ? C - u_stop + 1 : u_stop - len), (unsigned)len | ((unsigned)sf << 28));
          atomicAdd(&s_hist[orf_bin(len)], 1);
          my_orfs++; my_res += (unsigned)len;
        }
        carry = out.suffix[e];
      } else { carry += kTileCodons; out.cross[e] = make_uint2(0u, 0u); }
    }
  }
  if (my_orfs) { atomicAdd(&s_red[0], my_orfs); atomicAdd(&s_red[1], my_res); }
  __syncthreads();
  if (!out.count) return;
  for (int k = threadIdx.x; k < kOrfBins; k += blockDim.x) if (s_hist[k]) atomicAdd(&out.hist[k], s_hist[k]);
  if (threadIdx.x == 0 && s_red[0]) { atomicAdd(out.n_orfs, (unsigned long long)s_red[0]); atomicAdd(out.orf_res, (unsigned long long)s_red[1]); }
}

// The same for LONG windows (genome windows of 256 kb: ~680 tiles per window and frame), a WAVE per (window, frame): the lane
// walk above is a chain of dependent loads, one per tile (0.26 ms for a window whatever the block holds -- a tenth of a
// configs[3] query).  The run entering tile T comes from the nearest earlier tile that holds a stop: an exclusive running
// maximum of "index of a tile with a stop" over the wave's 64 tiles (DPP), that tile's suffix by one ds_bpermute, 128 codons
// for every stop-free tile in between; the run leaving the 64 tiles carries into the next 64.  Same records, same histogram.
__device__ __forceinline__ int wave_excl_max_scan(int v, int ident) {
  int x = dpp_or_ident<0x138>(v, ident);                           // wave_shr:1 (lane 0 gets the identity)
  x = max(x, dpp_or_ident<0x111>(x, ident));
  x = max(x, dpp_or_ident<0x112>(x, ident));
  x = max(x, dpp_or_ident<0x114>(x, ident));
  x = max(x, dpp_or_ident<0x118>(x, ident));
  x = max(x, dpp_or_ident<0x142, 0xa>(x, ident));                  // row_bcast:15
  x = max(x, dpp_or_ident<0x143, 0xc>(x, ident));                  // row_bcast:31
  return x;
}
__global__ __launch_bounds__(256) void orf_stitch_wave_kernel(SeqView dna, OrfTiles tiles, OrfScanOut out, int minlen) {
  __shared__ int s_hist[kOrfBins];
  __shared__ unsigned s_red[2];
  for (int i = threadIdx.x; i < kOrfBins; i += blockDim.x) s_hist[i] = 0;
  if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
  __syncthreads();
  unsigned my_orfs = 0, my_res = 0;
  const int lane = threadIdx.x & 63;
  const int64_t nstreams = dna.n * 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t sidx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; sidx < nstreams; sidx += nwaves) {
    const int64_t w = sidx / 6;
    const int sf = (int)(sidx - w * 6);
    const int n = dna.len[w];
    if (n < 15) continue;
    const int nt = (n / 3) / kTileCodons + 1;
    const int64_t first = tiles.tile_first[w];
    const bool rev = sf >= 3;
    const int fr = rev ? sf - 3 : 0;
    const int ph = rev ? (n - fr) % 3 : sf;
    const int C = (n - 3 - fr - ph) / 3;
    int carry_in = 0;
    for (int T0 = 0; T0 < nt; T0 += 64) {
      const int T = T0 + lane;
      const bool valid = T < nt;
      const int64_t e = (first + (valid ? T : 0)) * 6 + sf;
      const int p = valid ? out.prefix[e] : kTileCodons;
      const bool has = p < kTileCodons;
      const int sfx = has ? out.suffix[e] : 0;
      const int j = wave_excl_max_scan(has ? lane : -1, -1);           // the nearest earlier tile of these 64 that holds a stop
      const int sfx_j = __shfl(sfx, j < 0 ? 0 : j, 64);
      const int carry = (j >= 0) ? sfx_j + kTileCodons * (lane - j - 1) : carry_in + kTileCodons * lane;
      if (valid) {
        uint2 rec = make_uint2(0u, 0u);
        if (has) {
          const int len = carry + p;
          if (len >= minlen) {
            const int u_stop = kTileCodons * T + p;
            rec = make_uint2((unsigned)(rev ? C - u_stop + 1 : u_stop - len), (unsigned)len | ((unsigned)sf << 28));
            atomicAdd(&s_hist[orf_bin(len)], 1);
            my_orfs++; my_res += (unsigned)len;
          }
        }
        out.cross[e] = rec;
      }
      const int leave = has ? sfx : carry + kTileCodons;               // the run leaving this lane's tile
      carry_in = __shfl(leave, 63, 64);
    }
  }
  if (my_orfs) { atomicAdd(&s_red[0], my_orfs); atomicAdd(&s_red[1], my_res); }
  __syncthreads();
  if (!out.count) return;
  for (int k = threadIdx.x; k < kOrfBins; k += blockDim.x) if (s_hist[k]) atomicAdd(&out.hist[k], s_hist[k]);
  if (threadIdx.x == 0 && s_red[0]) { atomicAdd(out.n_orfs, (unsigned long long)s_red[0]); atomicAdd(out.orf_res, (unsigned long long)s_red[1]); }
}

// pli->strands and the initiation codons of -m / -M, on the records the scan kernels left (a lane per tile: its slots and its
// six crossing records).  A record of an excluded strand is cleared.  With initiators an ORF begins at the first initiation
// codon of its stop-free run (esl_gencode_ProcessPiece: a stop closes the frame's ORF, any other codon extends an open one, only an
// initiator opens one) and that codon reads M: the record is cut down -- and dropped if fewer than <minlen> residues remain --
// and the M is written into the amino-acid stream (the codons before it belong to no ORF).  A degenerate codon initiates only if
// every codon it stands for does (esl_gencode_IsInitiator).  The kernel counts what it keeps (histogram, ORFs, residues).
__global__ __launch_bounds__(256) void orf_filter_kernel(SeqView dna, OrfTiles tiles, OrfScanOut out, OrfFilter flt, int minlen) {
  __shared__ int s_hist[kOrfBins];
  __shared__ unsigned s_red[2];
  __shared__ uint8_t s_init[64], s_comp[32];
  for (int i = threadIdx.x; i < kOrfBins; i += blockDim.x) s_hist[i] = 0;
  if (threadIdx.x < 64) s_init[threadIdx.x] = flt.using_initiators ? flt.is_init[threadIdx.x] : 1;
  if (threadIdx.x < 18) s_comp[threadIdx.x] = flt.comp[threadIdx.x];
  if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
  __syncthreads();
  // members of a DNA code as a bit mask over A C G T ("ACGT-RYMKSWHBVDN*~")
  auto members = [](int x) -> unsigned {
    switch (x) {
      case 0: return 1u; case 1: return 2u; case 2: return 4u; case 3: return 8u;
      case 5: return 5u; case 6: return 10u; case 7: return 3u; case 8: return 12u; case 9: return 6u; case 10: return 9u;
      case 11: return 11u; case 12: return 14u; case 13: return 7u; case 14: return 13u; case 15: return 15u;
      default: return 0u;                                                   // gap, *, ~
    }
  };
  auto initiates = [&](int a, int b, int c) -> bool {
    if ((a | b | c) < 4) return s_init[16 * a + 4 * b + c] != 0;
    const unsigned ma = members(a), mb = members(b), mc = members(c);
    int n = 0;
    for (int x = 0; x < 4; x++) if (ma >> x & 1u)
      for (int y = 0; y < 4; y++) if (mb >> y & 1u)
        for (int z = 0; z < 4; z++) if (mc >> z & 1u) { if (!s_init[16 * x + 4 * y + z]) return false; n++; }
    return n > 0;
  };
  unsigned my_orfs = 0, my_res = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tiles.ntiles; t += (int64_t)gridDim.x * blockDim.x) {
    const int4 dsc = tiles.desc[t];
    const int n = dsc.y, w = dsc.z;
    if (n < 15) continue;
    const int64_t off = (int64_t)(uint32_t)dsc.x << 4;
    const uint8_t *x = dna.data + off;
    uint8_t *const abase = out.aa + (2 * off + 96 * (int64_t)w);
    const int pitch = orf_stream_pitch(n);
    const int c = out.cnt[t];
    uint2 *sl = out.slots + t * out.cap;
    for (int k = 0; k < c + 6; k++) {
      uint2 *rp = k < c ? sl + k : out.cross + t * 6 + (k - c);
      uint2 r = *rp;
      int len = (int)(r.y & 0x0fffffffu);
      if (len == 0) continue;
      const int sf = (int)(r.y >> 28);
      const bool rev = sf >= 3;
      if ((flt.strands == BATH_STRAND_TOPONLY && rev) || (flt.strands == BATH_STRAND_BOTTOMONLY && !rev)) { rp->y = 0u; continue; }
      if (flt.using_initiators) {
        int j = (int)r.x;
        const int jend = j + len;
        for (; j < jend; j++) {
          int a, b, cc;
          if (!rev) { const int p = sf + 3 * j; a = x[p]; b = x[p + 1]; cc = x[p + 2]; }
          else { const int q = (sf - 3) + 3 * j; a = s_comp[min((int)x[n - 1 - q], 17)]; b = s_comp[min((int)x[n - 2 - q], 17)]; cc = s_comp[min((int)x[n - 3 - q], 17)]; }
          if (initiates(min(a, 17), min(b, 17), min(cc, 17))) break;
        }
        len = jend - j;
        if (len < minlen || len <= 0) { rp->y = 0u; continue; }
        abase[sf * pitch + j] = 10;                                          // 'M' in "ACDEFGHIKLMNPQRSTVWY": the initiation codon's residue
        r.x = (unsigned)j; r.y = (unsigned)len | ((unsigned)sf << 28);
        *rp = r;
      }
      atomicAdd(&s_hist[orf_bin(len)], 1);
      my_orfs++; my_res += (unsigned)len;
    }
  }
  if (my_orfs) { atomicAdd(&s_red[0], my_orfs); atomicAdd(&s_red[1], my_res); }
  __syncthreads();
  for (int k = threadIdx.x; k < kOrfBins; k += blockDim.x) if (s_hist[k]) atomicAdd(&out.hist[k], s_hist[k]);
  if (threadIdx.x == 0 && s_red[0]) { atomicAdd(out.n_orfs, (unsigned long long)s_red[0]); atomicAdd(out.orf_res, (unsigned long long)s_red[1]); }
}

// counts -> start offsets, longest first; cursor[b * kOrfCursorStride] is the copy the sort kernel advances; total ORFs -> *n_total.
// One block of 256 threads, each owning 8 consecutive bins in longest-first order: a parallel scan, not a serial walk of the 2048
// bins (this single-block kernel waits for a CU beside the other part's SSV, and a serial chain there stretched it to over a ms).
__global__ __launch_bounds__(256) void orf_scan_bins(const int *__restrict__ hist, int *__restrict__ cursor, int *__restrict__ n_total) {
  constexpr int kPer = kOrfBins / 256;
  __shared__ int s_wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int c[kPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) { c[k] = hist[kOrfBins - 1 - (kPer * tid + k)]; sum += c[k]; }
  int x = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
  if (lane == 63) s_wsum[wv] = x;
  __syncthreads();
  int run = x - sum;
#pragma unroll
  for (int u = 0; u < 4; u++) run += u < wv ? s_wsum[u] : 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) { cursor[(kOrfBins - 1 - (kPer * tid + k)) * kOrfCursorStride] = run; run += c[k]; }
  if (tid == 255) *n_total = run;
}

// The work list: a counting sort by length bin, longest first, in blocks of kSortTiles consecutive tiles.  A block's records are
// one flat sequence -- tile by tile, its cnt[t] slot records then its six crossing records -- that the block's lanes walk
// together: consecutive lanes take consecutive records, so the slot regions and the crossing records are read by coalesced loads,
// once.  Each lane keeps its kSortRegs records in registers while a returning LDS atomic ranks them within their bin; the block
// then reserves its range in every non-empty bin with one global atomic and writes the records there.  A block whose records do
// not fit in kSortThreads * kSortRegs takes several rounds (a reservation per round).  Cleared records (length 0: crossing
// records without an ORF, and what orf_filter_kernel dropped) are skipped.
constexpr int kSortThreads = 1024;
constexpr int kSortTiles = 768;                                   // ~17 records per tile at the bench shape: one round per block
constexpr int kSortRegs = 16;
constexpr int kSortRound = kSortThreads * kSortRegs;

__global__ __launch_bounds__(kSortThreads) void orf_sort_kernel(OrfTiles tiles, const uint2 *__restrict__ slots, int cap, const int32_t *__restrict__ cnt,
                                                                const uint2 *__restrict__ cross, int *__restrict__ cursor, OrfRec *__restrict__ sorted) {
  __shared__ int s_bin[kOrfBins];                                 // per round: records per bin, then the block's start in that bin
  __shared__ int s_pre[kSortTiles + 1];                           // tile i's records are flat positions s_pre[i] .. s_pre[i+1]-1
  __shared__ int64_t s_wbase[kSortTiles];                         // amino-acid pool offset of the tile's window
  __shared__ int2 s_wp[kSortTiles];                               // {window, stream pitch}
  __shared__ uint16_t s_own[kSortRound];                          // flat position within the round -> tile
  __shared__ int s_wsum[kSortThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * kSortTiles;
  int e = 0;
  if (tid < kSortTiles && t0 + tid < tiles.ntiles) {
    const int64_t t = t0 + tid;
    const int4 dsc = tiles.desc[t];
    e = cnt[t] + 6;
    s_wbase[tid] = 2 * ((int64_t)(uint32_t)dsc.x << 4) + 96 * (int64_t)dsc.z;
    s_wp[tid] = make_int2(dsc.z, orf_stream_pitch(dsc.y));
  }
  for (int i = tid; i < kOrfBins; i += kSortThreads) s_bin[i] = 0;
  // block-wide exclusive prefix sum of the per-tile record counts
  int x = e;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
  if (lane == 63) s_wsum[wv] = x;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int u = 0; u < kSortThreads / 64; u++) { const int s = s_wsum[u]; before += u < wv ? s : 0; total += s; }
  const int pre = before + x - e;
  if (tid < kSortTiles) s_pre[tid] = pre;
  if (tid == 0) s_pre[kSortTiles] = total;
  for (int r0 = 0; r0 < total; r0 += kSortRound) {
    // owner of every flat position of the round: each tile's lane marks its own span
    if (tid < kSortTiles) {
      const int lo = max(pre, r0) - r0, hi = min(pre + e, r0 + kSortRound) - r0;
      for (int j = lo; j < hi; j++) s_own[j] = (uint16_t)tid;
    }
    __syncthreads();
    uint2 r[kSortRegs];
    int ti[kSortRegs];
#pragma unroll
    for (int k = 0; k < kSortRegs; k++) {
      const int j = r0 + k * kSortThreads + tid;
      r[k] = make_uint2(0u, 0u);
      ti[k] = -1;
      if (j < total) {
        const int i = s_own[j - r0];
        const int loc = j - s_pre[i], c = s_pre[i + 1] - s_pre[i] - 6;
        const int64_t t = t0 + i;
        r[k] = loc < c ? slots[t * cap + loc] : cross[t * 6 + (loc - c)];
        ti[k] = i;
      }
    }
    // rank within the block's share of the bin
#pragma unroll
    for (int k = 0; k < kSortRegs; k++) {
      const int len = (int)(r[k].y & 0x0fffffffu);
      if (len) ti[k] |= atomicAdd(&s_bin[orf_bin(len)], 1) << 10;
      else ti[k] = -1;
    }
    __syncthreads();
    for (int i = tid; i < kOrfBins; i += kSortThreads) {
      const int c = s_bin[i];
      if (c) s_bin[i] = atomicAdd(&cursor[i * kOrfCursorStride], c);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortRegs; k++) {
      if (ti[k] < 0) continue;
      const int i = ti[k] & 1023, rank = ti[k] >> 10;
      const int2 wp = s_wp[i];
      const int pos = s_bin[orf_bin((int)(r[k].y & 0x0fffffffu))] + rank;
      OrfRec rec;
      rec.aa_off = s_wbase[i] + (int64_t)(r[k].y >> 28) * wp.y + (int64_t)r[k].x; rec.w = wp.x; rec.len_sf = (int32_t)r[k].y;
      sorted[pos] = rec;
    }
    if (r0 + kSortRound < total) {                                // another round reuses s_bin and s_own
      __syncthreads();
      for (int i = tid; i < kOrfBins; i += kSortThreads) s_bin[i] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
size_t orf_aa_bytes(const bath_hip_seqs *dna) { return (size_t)(2 * dna->total_aligned + 96 * dna->n + 256); }
void orf_buffers_carve(OrfBuffers *ob, void *aa, void *slots, void *sorted, void *misc, size_t nent) {
  ob->aa = static_cast<uint8_t *>(aa); ob->slots = slots; ob->sorted = static_cast<OrfRec *>(sorted);
  ob->cross = misc;                                           // nent records of 8 bytes first (keeps them 8-byte aligned)
  ob->cnt = static_cast<int32_t *>(misc) + 2 * nent; ob->prefix = ob->cnt + nent; ob->suffix = ob->prefix + nent;
  ob->hist = reinterpret_cast<int *>(ob->suffix + nent); ob->cursor = ob->hist + kOrfBins; ob->ntotal = ob->cursor + kOrfBins * kOrfCursorStride;
}

int orf_slot_cap(int minlen) { return 6 * (kTileCodons / (std::max(minlen, 0) + 1) + 2); }   // six frames share a tile's record region

// tile -> window map of a DNA block, built once per block and kept with it
int orf_tiles_ensure(bath_hip_ctx *ctx, const bath_hip_seqs *dna) {
  if (dna->ntiles >= 0) return BATH_OK;
  std::vector<int32_t> first((size_t)std::max<int64_t>(dna->n, 1));
  std::vector<int4> desc;
  int64_t nt = 0;
  for (int64_t w = 0; w < dna->n; w++) {
    first[(size_t)w] = (int32_t)nt;
    const int n = dna->h_len[(size_t)w];
    const int k = n >= 15 ? (n / 3) / kTileCodons + 1 : 0;
    nt += k;
    if (nt >= (int64_t)INT32_MAX / 8 || (dna->h_off[(size_t)w] >> 4) > (int64_t)UINT32_MAX) { ctx->set_error("DNA block too large for one pipeline call: split it"); return BATH_EINVAL; }
    for (int T = 0; T < k; T++) desc.push_back(int4{(int)(uint32_t)(dna->h_off[(size_t)w] >> 4), n, (int)w, T});
  }
  if (desc.empty()) desc.push_back(int4{0, 0, 0, 0});
  BATH_HIP_TRY(ctx, hipMalloc((void **)&dna->d_tile_desc, desc.size() * sizeof(int4)));
  BATH_HIP_TRY(ctx, hipMalloc((void **)&dna->d_tile_first, first.size() * sizeof(int32_t)));
  BATH_HIP_TRY(ctx, hipMemcpy(dna->d_tile_desc, desc.data(), desc.size() * sizeof(int4), hipMemcpyHostToDevice));
  BATH_HIP_TRY(ctx, hipMemcpy(dna->d_tile_first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  dna->ntiles = nt;
  return BATH_OK;
}

// ---- translation tables ------------------------------------------------------------------------------------------
static bool dna_degen_has(int x, int y) {
  static const char *members[18] = {"A", "C", "G", "T", "", "AG", "CT", "AC", "GT", "CG", "AT", "ACT", "CGT", "ACG", "AGT", "ACGT", "", ""};
  static const char nt[] = "ACGT";
  return std::strchr(members[x], nt[y]) != nullptr;
}

// codon -> amino acid for all 18^3 digital codons: canonical codons through basic[]; degenerate codons
// give the amino acid all expansions agree on, else X (easel esl_gencode_GetTranslation semantics).
static void build_codon_table(const uint8_t basic[64], std::vector<uint8_t> &tab) {
  tab.assign(18 * 18 * 18, (uint8_t)kXaa);
  for (int a = 0; a < 18; a++) for (int b = 0; b < 18; b++) for (int c = 0; c < 18; c++) {
    int aa = -1; bool mixed = false;
    for (int x = 0; x < 4 && !mixed; x++) { if (!dna_degen_has(a, x)) continue;
      for (int y = 0; y < 4 && !mixed; y++) { if (!dna_degen_has(b, y)) continue;
        for (int z = 0; z < 4; z++) { if (!dna_degen_has(c, z)) continue;
          int v = basic[16 * x + 4 * y + z];
          if (aa == -1) aa = v; else if (aa != v) { mixed = true; break; }
        } } }
    tab[(a * 18 + b) * 18 + c] = (uint8_t)((mixed || aa == -1) ? kXaa : aa);
  }
}

int orf_tables_upload(bath_hip_ctx *ctx, int ncbi_table, OrfTablesDev *t, int initiator) {
  const int key = ncbi_table | (initiator << 16);
  t->using_initiators = initiator != BATH_INIT_ANY;
  if (ctx->orf_tables_id == key && ctx->scratch[Scratch::kOrfCodonTables].p) {            // still there from the last call: every query of a database pass asks again
    t->full = ctx->scratch[Scratch::kOrfCodonTables].as<uint8_t>(); t->fwd = t->full + 6144; t->rev = t->fwd + 64; t->comp = t->rev + 64; t->is_init = t->comp + 32;
    return BATH_OK;
  }
  uint8_t basic[64];
  if (bath_gencode_basic(ncbi_table, basic) != BATH_OK) { ctx->set_error("unknown NCBI translation table"); return BATH_EINVAL; }
  std::vector<uint8_t> host(6144 + 256, 0);
  std::vector<uint8_t> full;
  build_codon_table(basic, full);
  std::memcpy(host.data(), full.data(), full.size());
  uint8_t *fwd = host.data() + 6144, *rev = fwd + 64, *comp = rev + 64;
  for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) for (int c = 0; c < 4; c++) {
    fwd[a * 16 + b * 4 + c] = basic[16 * a + 4 * b + c];
    // memory-order bytes (x0,x1,x2) = (a,b,c): the reverse-strand codon is comp(x2), comp(x1), comp(x0)
    rev[a * 16 + b * 4 + c] = basic[16 * (3 - c) + 4 * (3 - b) + (3 - a)];
  }
  static const uint8_t kComp[18] = {3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 14, 13, 12, 11, 15, 16, 17};   // ACGT-RYMKSWHBVDN*~
  std::memcpy(comp, kComp, 18);
  if (bath_gencode_initiators(ncbi_table, initiator, comp + 32) != BATH_OK) { ctx->set_error("no initiation codons for this table / initiator mode"); return BATH_EINVAL; }
  DevBuf &b = ctx->scratch[Scratch::kOrfCodonTables];
  BATH_HIP_TRY(ctx, b.reserve(host.size()));
  BATH_HIP_TRY(ctx, hipMemcpyAsync(b.p, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->orf_tables_id = key;
  t->full = b.as<uint8_t>(); t->fwd = t->full + 6144; t->rev = t->fwd + 64; t->comp = t->rev + 64; t->is_init = t->comp + 32;
  return BATH_OK;
}

int launch_orf_scan(bath_hip_ctx *ctx, const bath_hip_seqs *dna, const OrfTablesDev &tt, int minlen, const OrfBuffers &b,
                    unsigned long long *d_n_orfs, unsigned long long *d_orf_res, int strands) {
  const int64_t ntiles = dna->ntiles;
  BATH_HIP_TRY(ctx, hipMemsetAsync(b.hist, 0, kOrfBins * sizeof(int), ctx->stream));
  OrfScanTables tabs{tt.full, tt.fwd, tt.rev, tt.comp};
  OrfTiles tiles{reinterpret_cast<const int4 *>(dna->d_tile_desc), dna->d_tile_first, ntiles};
  const bool filtered = strands != BATH_STRAND_BOTH || tt.using_initiators;   // not bathsearch's defaults: orf_filter_kernel edits the records and counts
  OrfScanOut out{b.aa, reinterpret_cast<uint2 *>(b.slots), b.cnt, reinterpret_cast<uint2 *>(b.cross), b.prefix, b.suffix, b.hist, d_n_orfs, d_orf_res, orf_slot_cap(minlen), filtered ? 0 : 1};
  const int cus = ctx->prop.multiProcessorCount;
  // persistent blocks: exactly as many as are resident at once, so that every block gets the same share of the tiles
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, orf_tile_kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + 15) / 16, (int64_t)cus * per_cu));
  hipLaunchKernelGGL(orf_tile_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dna->view(), tiles, tabs, out, minlen);
  static const int stitch_env = [] { const char *e = std::getenv("BATH_HIP_STITCH_WAVE"); return e ? std::atoi(e) : -1; }();   // 1 / 0: always / never the wave kernel (tests, A/B)
  const bool long_windows = stitch_env >= 0 ? stitch_env == 1 : ntiles > 32 * dna->n;                   // more than 32 tiles (12 kb) per window on average
  if (long_windows) {
    const int wblocks = (int)std::max<int64_t>(1, std::min<int64_t>((dna->n * 6 + 3) / 4, (int64_t)cus * 8));
    hipLaunchKernelGGL(orf_stitch_wave_kernel, dim3(wblocks), dim3(256), 0, ctx->stream, dna->view(), tiles, out, minlen);
  } else {
  const int sblocks = (int)std::max<int64_t>(1, std::min<int64_t>((dna->n * 6 + 255) / 256, (int64_t)cus * 8));
  hipLaunchKernelGGL(orf_stitch_kernel, dim3(sblocks), dim3(256), 0, ctx->stream, dna->view(), tiles, out, minlen);
  }
  if (filtered) {
    OrfFilter flt{strands, tt.using_initiators ? 1 : 0, tt.is_init, tt.comp};
    const int fblocks = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + 255) / 256, (int64_t)cus * 8));
    hipLaunchKernelGGL(orf_filter_kernel, dim3(fblocks), dim3(256), 0, ctx->stream, dna->view(), tiles, out, flt, minlen);
  }
  hipLaunchKernelGGL(orf_scan_bins, dim3(1), dim3(256), 0, ctx->stream, b.hist, b.cursor, b.ntotal);
  hipLaunchKernelGGL(orf_sort_kernel, dim3((unsigned)std::max<int64_t>(1, (ntiles + kSortTiles - 1) / kSortTiles)), dim3(kSortThreads), 0, ctx->stream, tiles,
                     reinterpret_cast<const uint2 *>(b.slots), out.cap, b.cnt, reinterpret_cast<const uint2 *>(b.cross), b.cursor, b.sorted);
  BATH_HIP_TRY(ctx, hipGetLastError());
  return BATH_OK;
}

}  // namespace bath

using namespace bath;

// esl_gencode_Process* as driven by bathsearch.c:384-392, for a whole block: the ORF list and residues, on the host.
extern "C" int bath_hip_translate_orfs(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int ncbi_table, int min_orf_len,
                                       const bath_orf **orfs, int64_t *n_orfs, const uint8_t **aa) {
  return bath_hip_translate_orfs_opts(ctx, dna, ncbi_table, min_orf_len, BATH_STRAND_BOTH, BATH_INIT_ANY, orfs, n_orfs, aa);
}

extern "C" int bath_hip_translate_orfs_opts(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int ncbi_table, int min_orf_len, int strands, int initiator,
                                            const bath_orf **orfs, int64_t *n_orfs, const uint8_t **aa) {
  if (!ctx || !dna || !orfs || !n_orfs || min_orf_len < 0 || strands < 0 || strands > 2 || initiator < 0 || initiator > 2) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  *orfs = nullptr; *n_orfs = 0;
  if (aa) *aa = nullptr;
  ctx->orfs.clear(); ctx->orf_aa.clear(); ctx->orf_work.clear();
  if (dna->n == 0) return BATH_OK;
  int st;
  OrfTablesDev tt{};
  if ((st = orf_tables_upload(ctx, ncbi_table, &tt, initiator)) != BATH_OK) return st;
  if ((st = orf_tiles_ensure(ctx, dna)) != BATH_OK) return st;
  int64_t max_orfs = 0;
  for (int64_t i = 0; i < dna->n; i++) if (dna->h_len[i] >= 15) max_orfs += 6 * (int64_t)((dna->h_len[i] / 3 + 1) / (min_orf_len + 1) + 1);
  const size_t nent = (size_t)dna->ntiles * 6;
  DevBuf &b_aa = ctx->scratch[Scratch::kOrfAminoPool], &b_slots = ctx->scratch[Scratch::kOrfSlots], &b_orfs = ctx->scratch[Scratch::kOrfRecords], &b_misc = ctx->scratch[Scratch::kOrfMisc];
  BATH_HIP_TRY(ctx, b_aa.reserve(orf_aa_bytes(dna)));
  BATH_HIP_TRY(ctx, b_slots.reserve(((size_t)dna->ntiles * (size_t)orf_slot_cap(min_orf_len) + 64) * 8));
  BATH_HIP_TRY(ctx, b_orfs.reserve((size_t)(max_orfs + 64) * sizeof(OrfRec)));
  BATH_HIP_TRY(ctx, b_misc.reserve((5 * nent + kOrfMiscInts) * sizeof(int32_t) + 64));
  OrfBuffers ob{};
  orf_buffers_carve(&ob, b_aa.p, b_slots.p, b_orfs.p, b_misc.p, nent);
  unsigned long long *d_ctr = reinterpret_cast<unsigned long long *>(ob.ntotal + 2);   // two counters nobody reads here
  BATH_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, 16, ctx->stream));
  if ((st = launch_orf_scan(ctx, dna, tt, min_orf_len, ob, d_ctr, d_ctr + 1, strands)) != BATH_OK) return st;
  int total = 0;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(&total, ob.ntotal, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<OrfRec> recs((size_t)total);
  std::vector<uint8_t> pool(orf_aa_bytes(dna));
  if (total > 0) BATH_HIP_TRY(ctx, hipMemcpy(recs.data(), ob.sorted, recs.size() * sizeof(OrfRec), hipMemcpyDeviceToHost));
  static_assert(sizeof(OrfRec) == sizeof(bath_orf_work), "bath_orf_work mirrors OrfRec");
  ctx->orf_work.resize((size_t)total);
  if (total > 0) std::memcpy(ctx->orf_work.data(), recs.data(), recs.size() * sizeof(OrfRec));
  BATH_HIP_TRY(ctx, hipMemcpy(pool.data(), ob.aa, pool.size(), hipMemcpyDeviceToHost));
  ctx->orfs.resize((size_t)total);
  for (int i = 0; i < total; i++) {
    const OrfRec &r = recs[(size_t)i];
    const int64_t w = r.w;
    const int sf = (int)((unsigned)r.len_sf >> 28), len = r.len_sf & 0x0fffffff;
    const int64_t stream = 2 * dna->h_off[w] + 96 * w + (int64_t)sf * orf_stream_pitch(dna->h_len[w]);
    bath_orf &o = ctx->orfs[(size_t)i];
    o.window = w; o.strand = sf / 3; o.frame = sf % 3; o.n = len;
    o.start = o.frame + 3 * (int32_t)(r.aa_off - stream) + 1; o.end = o.start + 3 * len - 1;
    o.aa_off = r.aa_off;                                     // device pool offset for now; rewritten below
  }
  std::sort(ctx->orfs.begin(), ctx->orfs.end(), [](const bath_orf &a, const bath_orf &b) {
    if (a.window != b.window) return a.window < b.window;
    if (a.strand != b.strand) return a.strand < b.strand;
    if (a.frame != b.frame) return a.frame < b.frame;
    return a.start < b.start;
  });
  for (bath_orf &o : ctx->orfs) {
    const int64_t src = o.aa_off;
    o.aa_off = (int64_t)ctx->orf_aa.size();
    ctx->orf_aa.insert(ctx->orf_aa.end(), pool.begin() + src, pool.begin() + src + o.n);
  }
  *orfs = ctx->orfs.data(); *n_orfs = total;
  if (aa) *aa = ctx->orf_aa.data();
  return BATH_OK;
}

extern "C" int bath_hip_orf_worklist(bath_hip_ctx *ctx, const bath_orf_work **list, int64_t *n) {
  if (!ctx || !list || !n) return BATH_EINVAL;
  *list = ctx->orf_work.data(); *n = (int64_t)ctx->orf_work.size();
  return BATH_OK;
}
