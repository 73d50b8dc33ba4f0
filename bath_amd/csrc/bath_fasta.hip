// bath_fasta.hip -- FASTA bytes -> digital targets -> DNA windows, on the device.
//
// The file's raw bytes arrive in chunks (bath_hip_fasta_feed) that may end anywhere.  A chunk is parsed in three launches:
//   (a) tile_agg_kernel: per 4 KB tile, with 16-byte loads, what the tile contributes whatever state it is entered in;
//   (b) tile_scan_kernel: one block walks the tile aggregates in order and fixes every tile's entry state (line state, records,
//       symbols, lines before it), the chunk's exit state and the first format error;
//   (c) tile_write_kernel: re-reads each tile, digitises through an LDS table and places every symbol with block prefix sums;
//       writes the record table (header byte range, first symbol).
// No launch hands work from one workgroup to another: everything a tile needs from the tiles before it comes from (b).
//
// The only state a byte's meaning depends on is its line's first byte other than blank space ("line char"): '>' makes the line
// a header, anything else a sequence line.  That state composes over spans as (has newline, first line char before the first
// newline, first line char after the last newline), an associative summary -- which is what (a) and (b) scan.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bath_common.hpp"

namespace {

constexpr int TILE = 4096;            // bytes per tile: 256 threads x 16 bytes
constexpr int TPB = 256;
constexpr int NONE = 256;             // "no line char yet"
constexpr int SCAN_THREADS = 1024;

__host__ __device__ inline bool is_blank(int b) { return b == ' ' || b == '\t' || b == '\r' || b == '\v' || b == '\f'; }

// DNA_SYMS = "ACGT-RYMKSWHBVDN*~", either case; U -> T, X -> N (bath_amd.digitize)
__host__ __device__ inline int dna_code(int b) {
  if (b >= 'a' && b <= 'z') b -= 32;
  switch (b) {
    case 'A': return 0;  case 'C': return 1;  case 'G': return 2;  case 'T': return 3;  case 'U': return 3;
    case '-': return 4;  case 'R': return 5;  case 'Y': return 6;  case 'M': return 7;  case 'K': return 8;
    case 'S': return 9;  case 'W': return 10; case 'H': return 11; case 'B': return 12; case 'V': return 13;
    case 'D': return 14; case 'N': return 15; case 'X': return 15; case '*': return 16; case '~': return 17;
    default: return 255;
  }
}

// span summary packed in 32 bits: bit 0 newline seen; bits 1-9 head (line char before the first newline); bits 10-18 tail (after the last)
__device__ inline uint32_t pack_sum(int nl, int head, int tail) { return (uint32_t)nl | (uint32_t)head << 1 | (uint32_t)tail << 10; }
__device__ inline int s_nl(uint32_t s) { return (int)(s & 1u); }
__device__ inline int s_head(uint32_t s) { return (int)((s >> 1) & 511u); }
__device__ inline int s_tail(uint32_t s) { return (int)((s >> 10) & 511u); }
__device__ inline uint32_t sum_identity() { return pack_sum(0, NONE, NONE); }
__device__ inline uint32_t combine(uint32_t a, uint32_t b) {      // span a, then span b
  const int nl = s_nl(a) | s_nl(b);
  const int head = s_nl(a) ? s_head(a) : (s_head(a) != NONE ? s_head(a) : s_head(b));
  const int tail = s_nl(b) ? s_tail(b) : (s_nl(a) ? (s_tail(a) != NONE ? s_tail(a) : s_head(b)) : NONE);
  return pack_sum(nl, head, tail);
}
__device__ inline int apply(uint32_t s, int c) { return s_nl(s) ? s_tail(s) : (c != NONE ? c : s_head(s)); }   // line char after the span

__device__ inline uint32_t byte_sum(int b) {
  if (b == '\n') return pack_sum(1, NONE, NONE);
  if (is_blank(b)) return sum_identity();
  return pack_sum(0, b, NONE);
}

struct TileAgg {
  uint32_t sum;           // the tile's span summary
  int32_t nl;             // newlines
  int32_t cnt_first;      // non-blank bytes before the first newline (the line the tile is entered in)
  int32_t nonblank_first; // the first of them (tile offset; TILE: none)
  int32_t bad_first;      // the first of them that is no symbol
  int32_t syms_rest, recs_rest;       // after the first newline: symbols, record starts
  int32_t bad_rest, seq_rest, rec_rest;   // ... first bad byte, first sequence byte, first record start (TILE: none)
};
struct TileEntry {
  int64_t syms, recs, lines;
  int32_t carry, pad;
};
struct FastaState {       // carried from chunk to chunk, on the device
  int64_t syms, recs, lines;
  int32_t carry, pad;
  int64_t err_off, err_line, err_rec;
  int32_t err_byte, err, pad2[2];
};

__device__ inline void load16(const uint8_t *p, int64_t avail, uint8_t (&b)[16], int &cnt) {
  if (avail >= 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);           // the chunk buffer is 16-byte aligned, tiles are 4096-byte
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 16; q++) b[q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
    cnt = 16;
  } else {
    cnt = avail > 0 ? (int)avail : 0;
#pragma unroll
    for (int q = 0; q < 16; q++) b[q] = q < cnt ? p[q] : (uint8_t)' ';
  }
}

// exclusive block scan of span summaries (Hillis-Steele over TPB threads)
__device__ uint32_t block_excl_sum(uint32_t v, uint32_t *lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const uint32_t o = t >= d ? lds[t - d] : sum_identity();
    __syncthreads();
    if (t >= d) lds[t] = combine(o, lds[t]);
    __syncthreads();
  }
  const uint32_t r = t > 0 ? lds[t - 1] : sum_identity();
  __syncthreads();
  return r;
}
__device__ int block_excl_add(int v, int *lds, int *total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const int o = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += o;
    __syncthreads();
  }
  const int r = lds[t] - v;
  *total = lds[TPB - 1];
  __syncthreads();
  return r;
}
__device__ int block_min(int v, int *lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) lds[threadIdx.x] = min(lds[threadIdx.x], lds[threadIdx.x + d]);
    __syncthreads();
  }
  const int r = lds[0];
  __syncthreads();
  return r;
}

// (a) what a tile contributes, for any entry state
__global__ __launch_bounds__(TPB) void tile_agg_kernel(const uint8_t *__restrict__ raw, int64_t n, TileAgg *__restrict__ agg) {
  __shared__ uint32_t ls[TPB];
  __shared__ int li[TPB];
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int off = threadIdx.x * 16;
  uint8_t b[16];
  int cnt;
  load16(raw + tile0 + off, n - tile0 - off, b, cnt);
  uint32_t mine = sum_identity();
  int nl = 0;
  for (int q = 0; q < cnt; q++) { mine = combine(mine, byte_sum(b[q])); nl += b[q] == '\n'; }
  const uint32_t pre = block_excl_sum(mine, ls);
  // walk: bytes before the tile's first newline belong to the entry line (unknown here), the rest are resolved in the tile
  bool first = !s_nl(pre);
  int c = s_tail(pre);
  int cnt_first = 0, nonblank_first = TILE, bad_first = TILE, syms = 0, recs = 0, bad_rest = TILE, seq_rest = TILE, rec_rest = TILE;
  for (int q = 0; q < cnt; q++) {
    const int x = b[q], pos = off + q;
    if (x == '\n') { first = false; c = NONE; continue; }
    if (is_blank(x)) continue;
    if (first) {
      cnt_first++;
      nonblank_first = min(nonblank_first, pos);
      if (dna_code(x) == 255) bad_first = min(bad_first, pos);
      continue;
    }
    if (c == NONE) {
      c = x;
      if (x == '>') { recs++; rec_rest = min(rec_rest, pos); continue; }
    }
    if (c == '>') continue;
    seq_rest = min(seq_rest, pos);
    if (dna_code(x) == 255) bad_rest = min(bad_rest, pos);
    else syms++;
  }
  int tot;
  TileAgg a;
  a.sum = 0;
  block_excl_add(nl, li, &tot); a.nl = tot;
  block_excl_add(cnt_first, li, &tot); a.cnt_first = tot;
  block_excl_add(syms, li, &tot); a.syms_rest = tot;
  block_excl_add(recs, li, &tot); a.recs_rest = tot;
  a.nonblank_first = block_min(nonblank_first, li);
  a.bad_first = block_min(bad_first, li);
  a.bad_rest = block_min(bad_rest, li);
  a.seq_rest = block_min(seq_rest, li);
  a.rec_rest = block_min(rec_rest, li);
  if (threadIdx.x == TPB - 1) a.sum = combine(pre, mine);
  if (threadIdx.x == TPB - 1) agg[blockIdx.x] = a;
}

// a tile's counts and first error, entered with line char <c> after <R> records
struct TileOut { int64_t syms, recs; int err; };
__device__ inline TileOut tile_resolve(const TileAgg &a, int c, int64_t R) {
  TileOut o{0, 0, TILE};
  const int L = c != NONE ? c : s_head(a.sum);
  int64_t rec_first = 0;
  if (L == '>') rec_first = (c == NONE) ? 1 : 0;
  else if (L != NONE) {
    o.syms += a.cnt_first - (a.bad_first < TILE ? 1 : 0);      // (an error stops the parse; the count is not used then)
    if (R == 0) o.err = min(o.err, a.nonblank_first);
    o.err = min(o.err, a.bad_first);
  }
  if (R + rec_first == 0 && a.seq_rest < a.rec_rest) o.err = min(o.err, a.seq_rest);
  o.err = min(o.err, a.bad_rest);
  o.syms += a.syms_rest;
  o.recs = rec_first + a.recs_rest;
  return o;
}

// (b) one block: entry state of every tile, the chunk's exit state, the first error (with its line and record)
__global__ __launch_bounds__(SCAN_THREADS) void tile_scan_kernel(const uint8_t *__restrict__ raw, int64_t n, int64_t file_off, const TileAgg *__restrict__ agg,
                                                                 int64_t ntiles, TileEntry *__restrict__ entry, FastaState *__restrict__ st) {
  __shared__ uint32_t s_sum[SCAN_THREADS];
  __shared__ int32_t s_carry[SCAN_THREADS];
  __shared__ int64_t s_syms[SCAN_THREADS], s_recs[SCAN_THREADS], s_lines[SCAN_THREADS];
  __shared__ long long s_err_tile;
  const int t = threadIdx.x;
  const int64_t per = (ntiles + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t t0 = min<int64_t>(ntiles, t * per), t1 = min<int64_t>(ntiles, t0 + per);
  uint32_t s = sum_identity();
  for (int64_t i = t0; i < t1; i++) s = combine(s, agg[i].sum);
  s_sum[t] = s;
  if (t == 0) s_err_tile = (long long)ntiles;
  __syncthreads();
  if (t == 0) {
    int c = st->carry;
    for (int k = 0; k < SCAN_THREADS; k++) { s_carry[k] = c; c = apply(s_sum[k], c); }
  }
  __syncthreads();
  {   // records, symbols, lines of my tiles (records decide the preamble check only, which does not change counts)
    int c = s_carry[t];
    int64_t sy = 0, re = 0, li = 0;
    for (int64_t i = t0; i < t1; i++) {
      const TileOut o = tile_resolve(agg[i], c, 1);
      sy += o.syms; re += o.recs; li += agg[i].nl;
      c = apply(agg[i].sum, c);
    }
    s_syms[t] = sy; s_recs[t] = re; s_lines[t] = li;
  }
  __syncthreads();
  if (t == 0) {
    int64_t sy = st->syms, re = st->recs, li = st->lines;
    for (int k = 0; k < SCAN_THREADS; k++) {
      const int64_t a = s_syms[k], b = s_recs[k], d = s_lines[k];
      s_syms[k] = sy; s_recs[k] = re; s_lines[k] = li;
      sy += a; re += b; li += d;
    }
  }
  __syncthreads();
  {
    int c = s_carry[t];
    int64_t sy = s_syms[t], re = s_recs[t], li = s_lines[t];
    for (int64_t i = t0; i < t1; i++) {
      entry[i] = TileEntry{sy, re, li, c, 0};
      const TileOut o = tile_resolve(agg[i], c, re);
      if (o.err < TILE) { atomicMin(&s_err_tile, (long long)i); break; }
      sy += o.syms; re += o.recs; li += agg[i].nl;
      c = apply(agg[i].sum, c);
    }
  }
  __syncthreads();
  if (t != 0) return;
  if (s_err_tile < ntiles) {
    // the byte, its line and record, by one walk over the tile
    const int64_t i = s_err_tile;
    const TileEntry e = entry[i];
    int c = e.carry;
    int64_t R = e.recs, line = e.lines + 1;
    const int64_t base = i * TILE, lim = min<int64_t>(n - base, TILE);
    for (int64_t q = 0; q < lim; q++) {
      const int x = raw[base + q];
      if (x == '\n') { c = NONE; line++; continue; }
      if (is_blank(x)) continue;
      if (c == NONE) { c = x; if (x == '>') { R++; continue; } }
      if (c == '>') continue;
      if (R == 0 || dna_code(x) == 255) {
        st->err = 1; st->err_off = file_off + base + q; st->err_line = line; st->err_rec = R - 1; st->err_byte = x;
        return;
      }
    }
    st->err = 1; st->err_off = -1; st->err_line = -1; st->err_rec = -1; st->err_byte = -1;      // (not reached: the aggregates said so)
    return;
  }
  if (ntiles > 0) {
    const TileEntry e = entry[ntiles - 1];
    const TileOut o = tile_resolve(agg[ntiles - 1], e.carry, e.recs);
    st->syms = e.syms + o.syms; st->recs = e.recs + o.recs; st->lines = e.lines + agg[ntiles - 1].nl;
    st->carry = apply(agg[ntiles - 1].sum, e.carry);
  }
}

// (c) digitise and place the symbols; the record table
__global__ __launch_bounds__(TPB) void tile_write_kernel(const uint8_t *__restrict__ raw, int64_t n, int64_t file_off, const TileEntry *__restrict__ entry,
                                                         uint8_t *__restrict__ codes, int64_t sym_base, int64_t *__restrict__ hdr_begin,
                                                         int64_t *__restrict__ hdr_end, int64_t *__restrict__ sym_start) {
  __shared__ uint32_t ls[TPB];
  __shared__ int li[TPB];
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)dna_code((int)threadIdx.x);
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int off = threadIdx.x * 16;
  const TileEntry e = entry[blockIdx.x];
  uint8_t b[16];
  int cnt;
  load16(raw + tile0 + off, n - tile0 - off, b, cnt);
  uint32_t mine = sum_identity();
  for (int q = 0; q < cnt; q++) mine = combine(mine, byte_sum(b[q]));
  const uint32_t pre = block_excl_sum(mine, ls);
  const int c0 = apply(pre, e.carry);
  int c = c0, ns = 0, nr = 0;
  for (int q = 0; q < cnt; q++) {
    const int x = b[q];
    if (x == '\n') { c = NONE; continue; }
    if (is_blank(x)) continue;
    if (c == NONE) { c = x; if (x == '>') { nr++; continue; } }
    if (c != '>') ns++;
  }
  int tot;
  const int sp = block_excl_add(ns, li, &tot);
  const int rp = block_excl_add(nr, li, &tot);
  int64_t sym = e.syms + sp, rec = e.recs + rp;        // global symbol index, records so far
  c = c0;
  for (int q = 0; q < cnt; q++) {
    const int x = b[q];
    const int64_t pos = file_off + tile0 + off + q;
    if (x == '\n') { if (c == '>') hdr_end[rec - 1] = pos; c = NONE; continue; }
    if (is_blank(x)) continue;
    if (c == NONE) {
      c = x;
      if (x == '>') { hdr_begin[rec] = pos + 1; sym_start[rec] = sym; rec++; continue; }
    }
    if (c == '>') continue;
    codes[sym - sym_base] = lut[x];
    sym++;
  }
}

// windows: one block per window, 16 bytes per thread and step; positions past the window's end get the padding byte of
// bath_hip_seqs_create (0x1d)
struct WinCopy { int64_t src, dst; int32_t n, padded; };
__global__ __launch_bounds__(TPB) void window_gather_kernel(const uint8_t *__restrict__ codes, const WinCopy *__restrict__ wins, uint8_t *__restrict__ data) {
  const WinCopy w = wins[blockIdx.x];
  const uint8_t *src = codes + w.src;
  uint8_t *dst = data + w.dst;
  for (int64_t j = (int64_t)threadIdx.x * 16; j < w.padded; j += TPB * 16) {
    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint32_t x = (j + q < w.n) ? src[j + q] : 0x1du;
      v[q >> 2] |= x << (8 * (q & 3));
    }
    *reinterpret_cast<uint4 *>(dst + j) = make_uint4(v[0], v[1], v[2], v[3]);   // windows start 16-byte aligned, padded to 16
  }
}

}  // namespace

struct bath_hip_fasta {
  bath_hip_ctx *ctx = nullptr;
  bath::DevBuf raw[2];                 // chunk bytes, two slots: the upload of chunk k+1 may run while chunk k is written out
  hipEvent_t ev_up = nullptr, ev_free[2] = {nullptr, nullptr};
  hipEvent_t ev_ready = nullptr;       // on the ingest stream after the last feed / finish: what another context's gather waits on
                                       // (release records nothing: its copy and hipFree are synchronous, done before d_codes is republished)
  std::mutex mu;                       // the host state below, for gathers of several contexts' threads (bath_hip_fasta_seqs_for)
  std::condition_variable cv_idle;     // gathers == 0
  int gathers = 0;                     // gathers between reading d_codes and the end of their kernel: release waits for none
  int slot = 0;
  bath::DevBuf agg, entry;
  uint8_t *d_codes = nullptr;          // symbols [sym_base, syms) of the file
  int64_t codes_cap = 0, sym_base = 0;
  int64_t *d_rec = nullptr;            // 3 x rec_cap: hdr_begin, hdr_end, sym_start
  int64_t rec_cap = 0;
  FastaState *d_state = nullptr;
  FastaState *h_state = nullptr;       // page-locked mirror
  int64_t fed = 0;                     // bytes fed
  bool failed = false, finished = false;
  std::vector<bath_fasta_record> recs; // host copy of the record table
  int64_t recs_valid = -1;             // records the host copy holds (-1: stale)
};

namespace {
int fasta_sync_records(bath_hip_fasta *f) {
  bath_hip_ctx *ctx = f->ctx;
  const int64_t R = f->h_state->recs;
  if (f->recs_valid == R) return BATH_OK;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<int64_t> h((size_t)std::max<int64_t>(R, 1) * 3);
  if (R > 0) {
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    BATH_HIP_TRY(ctx, hipMemcpy(h.data(), f->d_rec, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost));
    BATH_HIP_TRY(ctx, hipMemcpy(h.data() + R, f->d_rec + f->rec_cap, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost));
    BATH_HIP_TRY(ctx, hipMemcpy(h.data() + 2 * R, f->d_rec + 2 * f->rec_cap, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  f->recs.resize((size_t)R);
  for (int64_t r = 0; r < R; r++) {
    bath_fasta_record &x = f->recs[(size_t)r];
    x.hdr_begin = h[(size_t)r]; x.hdr_end = h[(size_t)(R + r)]; x.sym_start = h[(size_t)(2 * R + r)];
    if (x.hdr_end < 0) x.hdr_end = f->fed;                       // header still open (or ended by the end of the file)
    const int64_t next = r + 1 < R ? h[(size_t)(2 * R + r + 1)] : f->h_state->syms;
    x.length = next - x.sym_start;
  }
  f->recs_valid = R;
  return BATH_OK;
}

// grow a device buffer keeping its first <keep> bytes (ordered on the context's stream)
template <class T> int grow(bath_hip_ctx *ctx, T *&p, int64_t &cap, int64_t want, int64_t keep_elems, int parts = 1) {
  if (want <= cap) return BATH_OK;
  const int64_t ncap = std::max<int64_t>(want + want / 2, 1 << 16);
  T *q = nullptr;
  BATH_HIP_TRY(ctx, hipMalloc((void **)&q, (size_t)(ncap * parts) * sizeof(T)));
  if (p) {
    for (int k = 0; k < parts; k++)
      if (keep_elems > 0) BATH_HIP_TRY(ctx, hipMemcpyAsync(q + k * ncap, p + k * cap, (size_t)keep_elems * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(p);
  }
  p = q; cap = ncap;
  return BATH_OK;
}
}  // namespace

extern "C" int bath_hip_fasta_create(bath_hip_ctx *ctx, bath_hip_fasta **ret) {
  *ret = nullptr;
  if (!ctx) return BATH_EINVAL;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  bath_hip_fasta *f = new bath_hip_fasta();
  f->ctx = ctx;
  auto init = [&]() -> int {
    BATH_HIP_TRY(ctx, hipMalloc((void **)&f->d_state, sizeof(FastaState)));
    BATH_HIP_TRY(ctx, hipHostMalloc((void **)&f->h_state, sizeof(FastaState), hipHostMallocDefault));
    std::memset(f->h_state, 0, sizeof(FastaState));
    f->h_state->carry = NONE;
    f->h_state->err_off = f->h_state->err_line = f->h_state->err_rec = -1;
    BATH_HIP_TRY(ctx, hipMemcpy(f->d_state, f->h_state, sizeof(FastaState), hipMemcpyHostToDevice));
    BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&f->ev_up, hipEventDisableTiming));
    for (auto &e : f->ev_free) BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    BATH_HIP_TRY(ctx, hipEventCreateWithFlags(&f->ev_ready, hipEventDisableTiming));
    return BATH_OK;
  };
  if (int st = init(); st != BATH_OK) { bath_hip_fasta_destroy(f); return st; }
  *ret = f;
  return BATH_OK;
}

extern "C" void bath_hip_fasta_destroy(bath_hip_fasta *f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->ctx->copy_stream) (void)hipStreamSynchronize(f->ctx->copy_stream);
  for (auto &r : f->raw) r.release();
  f->agg.release(); f->entry.release();
  if (f->d_codes) (void)hipFree(f->d_codes);
  if (f->d_rec) (void)hipFree(f->d_rec);
  if (f->d_state) (void)hipFree(f->d_state);
  if (f->h_state) (void)hipHostFree(f->h_state);
  if (f->ev_up) (void)hipEventDestroy(f->ev_up);
  for (auto e : f->ev_free) if (e) (void)hipEventDestroy(e);
  if (f->ev_ready) (void)hipEventDestroy(f->ev_ready);
  delete f;
}

extern "C" int bath_hip_fasta_feed(bath_hip_fasta *f, const void *bytes, int64_t n) {
  if (!f || n < 0 || (n > 0 && !bytes)) return BATH_EINVAL;
  bath_hip_ctx *ctx = f->ctx;
  if (f->failed) { ctx->set_error("FASTA input: the handle stopped at a format error"); return BATH_EINVAL; }
  if (f->finished) { ctx->set_error("FASTA input: bytes fed after the end of the file"); return BATH_EINVAL; }
  if (n == 0) return BATH_OK;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->copy_stream) BATH_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  const int s = f->slot;
  f->slot ^= 1;
  // the slot's previous chunk must be written out before its bytes are replaced
  BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, f->ev_free[s], 0));
  if (f->raw[s].cap < (size_t)n + 16) {
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    BATH_HIP_TRY(ctx, f->raw[s].reserve((size_t)n + 16));
  }
  const uint8_t *d_raw = (const uint8_t *)f->raw[s].p;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(f->raw[s].p, bytes, (size_t)n, hipMemcpyHostToDevice, ctx->copy_stream));
  BATH_HIP_TRY(ctx, hipEventRecord(f->ev_up, ctx->copy_stream));
  BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, f->ev_up, 0));
  const int64_t ntiles = (n + TILE - 1) / TILE;
  if (ntiles > INT32_MAX) { ctx->set_error("FASTA chunk too large"); return BATH_EINVAL; }
  BATH_HIP_TRY(ctx, f->agg.reserve((size_t)ntiles * sizeof(TileAgg)));
  BATH_HIP_TRY(ctx, f->entry.reserve((size_t)ntiles * sizeof(TileEntry)));
  hipLaunchKernelGGL(tile_agg_kernel, dim3((unsigned)ntiles), dim3(TPB), 0, ctx->stream, d_raw, n, (TileAgg *)f->agg.p);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, d_raw, n, f->fed, (const TileAgg *)f->agg.p, ntiles,
                     (TileEntry *)f->entry.p, f->d_state);
  BATH_HIP_TRY(ctx, hipGetLastError());
  const int64_t syms0 = f->h_state->syms, recs0 = f->h_state->recs;
  BATH_HIP_TRY(ctx, hipMemcpyAsync(f->h_state, f->d_state, sizeof(FastaState), hipMemcpyDeviceToHost, ctx->stream));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the upload is done too: <bytes> is free
  f->recs_valid = -1;
  if (f->h_state->err) {
    f->failed = true;
    f->fed += n;
    char m[160];
    std::snprintf(m, sizeof m, "FASTA format error at byte %lld (line %lld): %s", (long long)f->h_state->err_off, (long long)f->h_state->err_line,
                  f->h_state->err_rec < 0 ? "sequence data before the first header" : "illegal character");
    ctx->set_error(m);
    BATH_HIP_TRY(ctx, hipEventRecord(f->ev_free[s], ctx->stream));
    return BATH_EINVAL;
  }
  // room for the chunk's symbols and records (the device wrote the counts: no host pass over the bytes)
  if (int st = grow(ctx, f->d_codes, f->codes_cap, f->h_state->syms - f->sym_base + 16, syms0 - f->sym_base); st != BATH_OK) return st;
  if (int st = grow(ctx, f->d_rec, f->rec_cap, f->h_state->recs, recs0, 3); st != BATH_OK) return st;
  if (f->h_state->recs > recs0)      // headers still open read -1 (another thread may close one in this launch: no kernel writes it)
    BATH_HIP_TRY(ctx, hipMemsetAsync(f->d_rec + f->rec_cap + recs0, 0xff, (size_t)(f->h_state->recs - recs0) * sizeof(int64_t), ctx->stream));
  hipLaunchKernelGGL(tile_write_kernel, dim3((unsigned)ntiles), dim3(TPB), 0, ctx->stream, d_raw, n, f->fed, (const TileEntry *)f->entry.p,
                     f->d_codes, f->sym_base, f->d_rec, f->d_rec + f->rec_cap, f->d_rec + 2 * f->rec_cap);
  BATH_HIP_TRY(ctx, hipGetLastError());
  BATH_HIP_TRY(ctx, hipEventRecord(f->ev_free[s], ctx->stream));
  BATH_HIP_TRY(ctx, hipEventRecord(f->ev_ready, ctx->stream));
  f->fed += n;
  return BATH_OK;
}

extern "C" int bath_hip_fasta_finish(bath_hip_fasta *f) {
  if (!f) return BATH_EINVAL;
  if (f->failed) return BATH_EINVAL;
  std::lock_guard<std::mutex> g(f->mu);
  f->finished = true;
  BATH_HIP_TRY(f->ctx, hipSetDevice(f->ctx->device));
  BATH_HIP_TRY(f->ctx, hipStreamSynchronize(f->ctx->stream));
  BATH_HIP_TRY(f->ctx, hipEventRecord(f->ev_ready, f->ctx->stream));
  f->recs_valid = -1;
  return fasta_sync_records(f);
}

extern "C" int64_t bath_hip_fasta_count(bath_hip_fasta *f) { return f ? f->h_state->recs : -1; }
extern "C" int64_t bath_hip_fasta_symbols(bath_hip_fasta *f) { return f ? f->h_state->syms : -1; }

extern "C" int bath_hip_fasta_records(bath_hip_fasta *f, int64_t lo, int64_t n, bath_fasta_record *out) {
  if (!f || lo < 0 || n < 0 || lo + n > f->h_state->recs) return BATH_EINVAL;
  std::lock_guard<std::mutex> g(f->mu);
  if (int st = fasta_sync_records(f); st != BATH_OK) return st;
  if (n > 0) std::memcpy(out, f->recs.data() + lo, (size_t)n * sizeof(bath_fasta_record));
  return BATH_OK;
}

extern "C" int bath_hip_fasta_error(const bath_hip_fasta *f, int64_t *offset, int64_t *line, int64_t *record, int32_t *byte) {
  if (!f) return BATH_EINVAL;
  if (!f->failed) return BATH_ENORESULT;
  *offset = f->h_state->err_off; *line = f->h_state->err_line; *record = f->h_state->err_rec; *byte = f->h_state->err_byte;
  return BATH_OK;
}

extern "C" int64_t bath_hip_fasta_windows(bath_hip_fasta *f, int64_t lo, int64_t hi, int32_t max_length, int32_t block_length,
                                          bath_fasta_window *out, int64_t cap) {
  if (!f || lo < 0 || hi < lo || hi > f->h_state->recs || max_length < 1 || block_length < 1) return -1;
  std::lock_guard<std::mutex> g(f->mu);
  if (fasta_sync_records(f) != BATH_OK) return -1;
  const int64_t C = 3 * (int64_t)max_length;
  int64_t k = 0;
  for (int64_t r = lo; r < hi; r++) {                  // dist.split_targets
    const int64_t L = f->recs[(size_t)r].length;
    int64_t pos = 0;
    while (true) {
      const int64_t c = pos == 0 ? 0 : C;
      const int64_t n_new = std::min<int64_t>(block_length, L - pos);
      if (k < cap && out) out[k] = bath_fasta_window{r, pos - c, (int32_t)(n_new + c), (int32_t)c};
      k++;
      pos += n_new;
      if (pos >= L) break;
    }
  }
  return k;
}

namespace {
// The windows <w> of <f> as a block of <ctx>: the owner's own context (bath_hip_fasta_seqs) or another one of the same device
// (bath_hip_fasta_seqs_for: <shared>).  The handle's host tables are read under its mutex; the gather runs on <ctx>'s stream and is
// complete when the call returns; f->gathers counts the calls between those two points, which bath_hip_fasta_release waits for.
int fasta_gather(bath_hip_ctx *ctx, bath_hip_fasta *f, const bath_fasta_window *w, int64_t n, bath_hip_seqs **ret, bool shared) {
  std::vector<WinCopy> cp((size_t)std::max<int64_t>(n, 1));
  bath_hip_seqs *sq = new bath_hip_seqs();
  sq->ctx = ctx; sq->n = n;
  sq->h_off.resize((size_t)n); sq->h_len.resize((size_t)n); sq->h_context.resize((size_t)n);
  int64_t pos = 0;
  bool any_context = false;
  const uint8_t *d_codes = nullptr;
  std::unique_lock<std::mutex> lock(f->mu);
  if (int st = fasta_sync_records(f); st != BATH_OK) {
    if (shared) ctx->set_error("FASTA targets: the record table could not be read: " + f->ctx->err);
    delete sq;
    return st;
  }
  for (int64_t i = 0; i < n; i++) {
    const bath_fasta_window &x = w[i];
    const bool ok = x.target >= 0 && x.target < (int64_t)f->recs.size() && x.n >= 0 && x.context >= 0 && x.context <= x.n && x.start0 >= 0 &&
                    x.start0 + x.n <= f->recs[(size_t)x.target].length && f->recs[(size_t)x.target].sym_start + x.start0 >= f->sym_base;
    if (!ok) { delete sq; ctx->set_error("window outside its target, or its codes were released"); return BATH_EINVAL; }
    sq->h_off[(size_t)i] = pos; sq->h_len[(size_t)i] = x.n; sq->h_context[(size_t)i] = x.context;
    any_context |= x.context > 0;
    sq->maxlen = std::max(sq->maxlen, x.n);
    sq->total += x.n;
    const int32_t padded = (x.n + 15) / 16 * 16;
    cp[(size_t)i] = WinCopy{f->recs[(size_t)x.target].sym_start + x.start0 - f->sym_base, pos, x.n, padded};
    pos += padded;
  }
  sq->total_aligned = pos;
  d_codes = f->d_codes;
  f->gathers++;
  lock.unlock();
  auto build = [&]() -> int {
    const size_t bytes = (size_t)pos + 64;
    BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (shared) BATH_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, f->ev_ready, 0));   // the codes are written: ingest stream -> this one
    BATH_HIP_TRY(ctx, hipMalloc((void **)&sq->d_data, bytes));
    BATH_HIP_TRY(ctx, hipMalloc((void **)&sq->d_off, (size_t)std::max<int64_t>(n, 1) * sizeof(int64_t)));
    BATH_HIP_TRY(ctx, hipMalloc((void **)&sq->d_len, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t)));
    BATH_HIP_TRY(ctx, hipMemsetAsync(sq->d_data + pos, 0x1d, 64, ctx->stream));
    if (n > 0) {
      WinCopy *d_cp = nullptr;
      BATH_HIP_TRY(ctx, hipMalloc((void **)&d_cp, (size_t)n * sizeof(WinCopy)));
      BATH_HIP_TRY(ctx, hipMemcpyAsync(d_cp, cp.data(), (size_t)n * sizeof(WinCopy), hipMemcpyHostToDevice, ctx->stream));
      BATH_HIP_TRY(ctx, hipMemcpyAsync(sq->d_off, sq->h_off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
      BATH_HIP_TRY(ctx, hipMemcpyAsync(sq->d_len, sq->h_len.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
      if (n > INT32_MAX) { ctx->set_error("too many windows in one block"); return BATH_EINVAL; }
      hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)n), dim3(TPB), 0, ctx->stream, d_codes, d_cp, sq->d_data);
      BATH_HIP_TRY(ctx, hipGetLastError());
      BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipFree(d_cp);
    }
    if (any_context) {
      BATH_HIP_TRY(ctx, hipMalloc((void **)&sq->d_context, (size_t)n * sizeof(int32_t)));
      BATH_HIP_TRY(ctx, hipMemcpy(sq->d_context, sq->h_context.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    } else {
      sq->h_context.clear();
    }
    BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BATH_OK;
  };
  const int st = build();
  if (st != BATH_OK) (void)hipStreamSynchronize(ctx->stream);      // nothing of this call reads the codes any more
  lock.lock();
  if (--f->gathers == 0) f->cv_idle.notify_all();
  lock.unlock();
  if (st != BATH_OK) { bath_hip_seqs_destroy(sq); return st; }
  *ret = sq;
  return BATH_OK;
}
}  // namespace

extern "C" int bath_hip_fasta_seqs(bath_hip_fasta *f, const bath_fasta_window *w, int64_t n, bath_hip_seqs **ret) {
  *ret = nullptr;
  if (!f || n < 0 || (n > 0 && !w)) return BATH_EINVAL;
  return fasta_gather(f->ctx, f, w, n, ret, false);
}

extern "C" int bath_hip_fasta_seqs_for(bath_hip_ctx *consumer, bath_hip_fasta *f, const bath_fasta_window *w, int64_t n, bath_hip_seqs **ret) {
  if (ret) *ret = nullptr;
  if (!consumer || !f || !ret || n < 0 || (n > 0 && !w)) return BATH_EINVAL;
  if (consumer->device != f->ctx->device) { consumer->set_error("FASTA targets of another device"); return BATH_EINVAL; }
  return fasta_gather(consumer, f, w, n, ret, consumer != f->ctx);
}

extern "C" int bath_hip_fasta_codes(bath_hip_fasta *f, int64_t target, int64_t start, int64_t n, uint8_t *out) {
  if (!f || n < 0) return BATH_EINVAL;
  bath_hip_ctx *ctx = f->ctx;
  std::lock_guard<std::mutex> g(f->mu);
  if (int st = fasta_sync_records(f); st != BATH_OK) return st;
  if (target < 0 || target >= (int64_t)f->recs.size() || start < 0 || start + n > f->recs[(size_t)target].length ||
      f->recs[(size_t)target].sym_start + start < f->sym_base) { ctx->set_error("codes outside the target"); return BATH_EINVAL; }
  if (n == 0) return BATH_OK;
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));      // a worker thread renders: the copy below is from this context's device
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  BATH_HIP_TRY(ctx, hipMemcpy(out, f->d_codes + (f->recs[(size_t)target].sym_start + start - f->sym_base), (size_t)n, hipMemcpyDeviceToHost));
  return BATH_OK;
}

extern "C" int bath_hip_fasta_release(bath_hip_fasta *f, int64_t lo) {
  if (!f || lo < 0 || lo > f->h_state->recs) return BATH_EINVAL;
  bath_hip_ctx *ctx = f->ctx;
  std::unique_lock<std::mutex> lock(f->mu);
  f->cv_idle.wait(lock, [&] { return f->gathers == 0; });          // no gather in flight reads the codes freed below
  if (int st = fasta_sync_records(f); st != BATH_OK) return st;
  const int64_t base = lo < (int64_t)f->recs.size() ? f->recs[(size_t)lo].sym_start : f->h_state->syms;
  if (base <= f->sym_base) return BATH_OK;
  const int64_t keep = f->h_state->syms - base;
  uint8_t *q = nullptr;
  const int64_t cap = std::max<int64_t>(keep + keep / 2, 1 << 16);
  BATH_HIP_TRY(ctx, hipSetDevice(ctx->device));
  BATH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  BATH_HIP_TRY(ctx, hipMalloc((void **)&q, (size_t)cap));
  if (keep > 0) BATH_HIP_TRY(ctx, hipMemcpy(q, f->d_codes + (base - f->sym_base), (size_t)keep, hipMemcpyDeviceToDevice));
  (void)hipFree(f->d_codes);
  f->d_codes = q; f->codes_cap = cap; f->sym_base = base;
  return BATH_OK;
}
