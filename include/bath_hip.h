/* bath_hip.h -- C ABI of the MI355X (gfx950) backend for BATH's bathsearch DP hot path.
 *
 * This is the drop-in boundary: the reference selects its DP backend at build time through the
 * impl_* directory contract (src/hmmer.h:1044-1052, src/Makefile.in:39) and every kernel there has
 * the shape  int f(const ESL_DSQ *dsq, int L, const PROFILE *om, MATRIX *ox, float *opt_sc)
 * (src/impl_sse/impl_sse.h:408-553).  A GPU cannot be fed one target per call, so each entry
 * point below is the BATCHED form of the reference function named in its comment: same inputs
 * (digital sequences, 1..L, easel codes), same outputs (nat scores, easel status codes
 * eslOK=0 / eslERANGE=16 / eslENORESULT=19), one array element per target.  INTEGRATION.md shows the
 * impl_hip/ shims that bind these to the reference's single-target prototypes.
 *
 * Plain C types only.  All pointers are HOST pointers unless the name ends in _dev.
 * Every function returns 0 (BATH_OK) or an easel-compatible error code; bath_hip_last_error()
 * returns a message.  There is no CPU fallback: if no gfx950 device is usable, bath_hip_init fails.
 */
#ifndef BATH_HIP_H
#define BATH_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BATH_OK          0
#define BATH_EFAIL       1
#define BATH_EMEM        5
#define BATH_EFORMAT     7
#define BATH_EINVAL     11
#define BATH_ERANGE     16   /* eslERANGE: filter score overflow (score = +inf) / Forward range error */
#define BATH_ENORESULT  19   /* eslENORESULT: SSV cannot decide, full MSV needed                      */
#define BATH_ENODEVICE  40

#define BATH_KP_AMINO   29   /* easel amino alphabet "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~" */
#define BATH_K_AMINO    20
#define BATH_KP_DNA     18   /* easel DNA alphabet   "ACGT-RYMKSWHBVDN*~"            */
#define BATH_NEVPARAM    8   /* MMU MLAMBDA VMU VLAMBDA FTAU FLAMBDA FTAUFS3 FTAUFS5 (hmmer.h:67) */
#define BATH_FTAU        4
#define BATH_FLAMBDA     5
#define BATH_FTAUFS3     6

typedef struct bath_hip_ctx      bath_hip_ctx;      /* one GPU + one HIP stream (a reference "worker", bathsearch.c:34-52) */
typedef struct bath_hip_oprofile bath_hip_oprofile; /* device-resident P7_OPROFILE  (impl_sse.h:75)   */
typedef struct bath_hip_fsprofile bath_hip_fsprofile; /* device-resident P7_FS_OPROFILE (impl_sse.h:200) */
typedef struct bath_hip_seqs     bath_hip_seqs;     /* device-resident block of digital sequences (ESL_SQ_BLOCK) */

/* ------------------------------------------------------------------------------------------
 * Host-side model objects (generic layer the impl boundary consumes).
 * ------------------------------------------------------------------------------------------ */

/* P7_HMM as read from a BATH3/f file (p7_hmmfile.c:1342 read_asc30hmm). */
typedef struct {
  int32_t M, max_length, ct;
  float   fsprob;
  float  *t;        /* [(M+1)*7]  MM MI MD IM II DM DD   */
  float  *mat;      /* [(M+1)*20]                         */
  float  *ins;      /* [(M+1)*20]                         */
  float   compo[BATH_K_AMINO];
  float   evparam[BATH_NEVPARAM];
  char    name[128];
  char    acc[64];  /* ACC line, "" when absent                                              */
  char   *consensus;/* [M+2] consensus residue per node, consensus[0] = ' ' (P7_HMM.consensus): the file's CONS column,
                     * or p7_hmm_SetConsensus's rule when the file has none (p7_hmm.c: most probable residue,
                     * upper case if its probability is >= 0.5)                                */
  char   *rf;       /* [M+2] reference annotation per node (P7_HMM.rf, "RF yes"), rf[0] = ' '; NULL when the model has none */
  char   *cs;       /* [M+2] consensus structure annotation (P7_HMM.cs, "CS yes"); NULL when the model has none            */
} bath_hmm;

/* P7_PROFILE (hmmer.h:338): what p7_oprofile_Convert() reads. */
typedef struct {
  int32_t M, L, max_length;
  float   nj;
  float  *tsc;      /* [M*8]  order MM IM DM BM MD DD MI II (hmmer.h:221), BM stored off by one */
  float  *rsc;      /* [Kp][(M+1)*2]  match at [x][2k], insert at [x][2k+1]                     */
  float   xsc[4][2];/* [E N J C][LOOP MOVE]                                                     */
  float   evparam[BATH_NEVPARAM];
  float   compo[BATH_K_AMINO];
} bath_profile;

/* P7_FS_PROFILE (hmmer.h:371): what p7_fs_oprofile_Convert() reads. */
typedef struct {
  int32_t M, L, max_length, codon_lengths, maxcodons;
  float   nj, fsprob;
  float  *tsc;      /* [M*8]                                   */
  float  *rsc;      /* [(maxcodons+Kp)][M+1]  rsc[codon][k]    */
  uint8_t *codons;  /* [(M+1)][maxcodons] argmax amino acid    */
  uint8_t *indel_pos;
  float   xsc[4][2];
  float   evparam[BATH_NEVPARAM];
  float   compo[BATH_K_AMINO];
} bath_fs_profile;

int  bath_hmmfile_count(const char *path);
int  bath_hmmfile_read(const char *path, int index, bath_hmm **ret);            /* p7_hmmfile.c:1342 */
void bath_hmm_destroy(bath_hmm *hmm);
int  bath_gencode_basic(int ncbi_table, uint8_t basic[64]);                     /* gcode->basic[16a+4b+c] */
int  bath_profile_config(const bath_hmm *hmm, int L, bath_profile **ret);       /* p7_ProfileConfig, modelconfig.c:48 (p7_LOCAL, Swiss-Prot bg) */
void bath_profile_destroy(bath_profile *gm);
int  bath_fs_profile_config(const bath_hmm *hmm, const uint8_t basic[64], int codon_lengths, int L_amino,
                            bath_fs_profile **ret);                             /* p7_ProfileConfig_fs, modelconfig.c:220 */
void bath_fs_profile_destroy(bath_fs_profile *gm);

/* ------------------------------------------------------------------------------------------
 * Device context.
 * ------------------------------------------------------------------------------------------ */
int         bath_hip_init(int device, bath_hip_ctx **ctx);          /* impl_Init(), impl_sse.h:559 */
void        bath_hip_finalize(bath_hip_ctx *ctx);
const char *bath_hip_last_error(const bath_hip_ctx *ctx);
int         bath_hip_synchronize(bath_hip_ctx *ctx);
/* Release the lanes, side contexts and side streams the context created lazily for the concurrency inside its calls (created
 * again on demand).  For a context that will sit idle while other contexts of the process work: its streams hold hardware
 * queues.  Results of earlier calls on the context are invalid afterwards. */
int         bath_hip_trim(bath_hip_ctx *ctx);
void       *bath_hip_stream(bath_hip_ctx *ctx);                      /* hipStream_t, for event timing */
/* Frameshift recursions.  1 (the default): every sum along the model -- D(i,k), E(i), Backward's B(i) -- runs node by node in the
 * reference's order (generic_fwdback_frameshift.c:340-365, :577-590, :1279-1283), so every table log-sum has the reference's
 * operands: scores, special-state rows and matrices are BIT-IDENTICAL to the generic reference (the north star's 1e-4 with
 * room to spare) and every frameshift-branch domain has the reference's coordinates exactly.
 * 0 = "fast": the same table log-sums associated by wavefront scans in the multihit recursions (3-codon parsers, the regions'
 * Forward), ~1.3x faster on the bench's --fs pass.  WARNING: the fast mode is OUTSIDE the parity contract and CHANGES RESULTS, not
 * only the last digits of scores: window scores move by up to ~1e-3 nats (beyond 1e-4 relative for scores near zero), so a window
 * at a threshold may take the other branch, region boundaries may shift by a step and a clustered region's stochastic traces take
 * other turns -- on the bench's block 89 of 4789 domains come out with OTHER COORDINATES (bench.py: fs.fast.domains_identical_to_
 * strict_mode).  Use it for throughput estimates or pre-screening, never where hit lists are compared with the reference's.
 * Applies to the pipeline entry points and to BATH_LOGSUM_CONTEXT. */
int         bath_hip_set_fs_strict(bath_hip_ctx *ctx, int on);
/* Odds-ratio mode of the 3-codon parsers.  1: the pipeline entry points (bath_hip_pipeline_frameshift, _frameshift_domains) run their
 * 3-codon Forward and Backward parsers in BATH_LOGSUM_ODDS, and BATH_LOGSUM_CONTEXT on the fs3 entry points means BATH_LOGSUM_ODDS;
 * every other stage (envelopes, the regions' Forward, decoding, optimal accuracy) runs as bath_hip_set_fs_strict selects.
 * 0 (the default): no change.  The first odds-mode call for a 3-codon profile builds its odds-ratio tables on the device. */
int         bath_hip_set_fs_odds(bath_hip_ctx *ctx, int on);
/* Which kernel scores the Forward stage of the filter cascade (bath_hip_pipeline_filters and what builds on it).  0 (the default):
 * fwd_group_kernel, four targets per wave, for a model of up to 160 nodes when the stage's special-state rows are not kept for the
 * domain stage, whatever the block's size; the wave-per-target kernel otherwise.  1: the same, and it stays so if the default ever
 * gains a rule of its own (what tests ask for).  2: never.  The two kernels' scores agree within the Forward parser's contract
 * (1e-4 relative / 2e-4 absolute nats), not bit for bit.  BATH_EINVAL for a null ctx or another mode. */
int         bath_hip_set_fwd_group(bath_hip_ctx *ctx, int mode);
/* Odds-ratio mode of the 5-codon Forward and Backward.  1: the envelopes' Forward and Backward (bath_hip_fs5_envelopes[_x] with
 * BATH_LOGSUM_CONTEXT, the pipeline's envelope batches) and the regions' multihit Forward (the domain stage, bath_hip_fs5_forward_full)
 * run in fp32 odds ratios with sparse rescaling, as the reference's p7_Forward_Frameshift / p7_Backward_Frameshift (impl_sse/
 * fwdback_fs.c:2054, :2634); it takes precedence over bath_hip_set_fs_strict for these stages.  Decoding, optimal accuracy, null2 and
 * the traces read the matrices as before (log value + the running scale).  c5_compat = 1 is refused (BATH_EINVAL) while it is on.
 * Contract: scores within 1e-3 + 1e-4 |s| nats of EXACT log-space arithmetic, matrix cells and special-state rows within 2e-3 +
 * 2e-4 |v| where the exact value is above -60 and within 60 nats of its row's largest; values about 87 nats below the running scale
 * flush to zero in fp32 and come back as -inf.  NOT bit-identical to strict: a domain at a threshold may move.
 * 0 (the default): no change.  An explicit BATH_LOGSUM_ODDS on the fs5 entry points stays refused.  The reference's whole --fs
 * arithmetic is bath_hip_set_fs_odds(ctx, 1) plus bath_hip_set_fs5_odds(ctx, 1).  A null ctx returns BATH_EINVAL. */
int         bath_hip_set_fs5_odds(bath_hip_ctx *ctx, int on);
/* How the frameshift branch samples the 200 stochastic tracebacks of a multi-domain region (region_trace_ensemble_frameshift,
 * p7_domaindef.c:891-958).
 *   BATH_ENSEMBLE_SERIAL (0, the default): one random-number stream per region, trace t starts where trace t-1 stopped drawing; on
 *     host threads, from Forward matrices the kernel streams into page-locked host memory.  The reference's order of draws.
 *   BATH_ENSEMBLE_STREAMS_HOST (1): trace t starts from the state the region's generator has after t * 2^20 steps (trace 0 where
 *     the serial stream starts), and the walk uses its own expf / logf (IEEE double arithmetic, the same float on host and device);
 *     on host threads.  The twin of mode 2: same traces, same segments, same envelopes.
 *   BATH_ENSEMBLE_STREAMS_DEVICE (2): the same walks as 200 lanes of fs_ensemble_kernel, one block per region, on matrices that stay
 *     in device memory; only statuses and segments come back.
 * Modes 1 and 2 sample the same posterior with other random numbers than mode 0: envelopes agree with mode 0's as two seeds of
 * mode 0 agree with each other, not bit for bit.  A region outside the stream rule (4 (4 (Lr + M) + 64) >= 2^20) takes the serial
 * path; in mode 2 a region with a trace of more than 8 segments takes mode 1's.  bath_hip_fs_ensemble_counters counts both (since
 * the context was created), and the bytes of Forward matrices mode 2 did not send to the host.  The standard branch's ensemble
 * (region_trace_ensemble) has a switch of its own, bath_hip_set_std_ensemble.  Unknown mode or null ctx: BATH_EINVAL. */
#define BATH_ENSEMBLE_SERIAL 0
#define BATH_ENSEMBLE_STREAMS_HOST 1
#define BATH_ENSEMBLE_STREAMS_DEVICE 2
int         bath_hip_set_fs_ensemble(bath_hip_ctx *ctx, int mode);
int         bath_hip_fs_ensemble_counters(bath_hip_ctx *ctx, int64_t *bound_fallbacks, int64_t *overflow_fallbacks, int64_t *matrix_bytes_kept);
/* The same choice for the STANDARD branch's multi-domain regions (region_trace_ensemble, p7_domaindef.c:766-850, with
 * p7_StochasticTrace): a plain search, and the windows of an --fs search that take the standard branch.  Same modes, same stream rule
 * (trace t starts t * 2^20 steps into the region's generator; a region with 4 (4 (Lr + M) + 64) >= 2^20 takes the serial path):
 *   BATH_ENSEMBLE_SERIAL (0, the default): today's path -- host threads, Forward matrices streamed into page-locked host memory.
 *   BATH_ENSEMBLE_STREAMS_HOST (1): a stream per trace, the E state's sum in ascending node order; host threads.  The twin of mode 2.
 *   BATH_ENSEMBLE_STREAMS_DEVICE (2): the same walks as 200 lanes of std_ensemble_kernel, one block per region, on matrices that stay
 *     in device memory; statuses, segments and the 2-bit M / I / D path codes inside them come back in one copy.
 * The walk has no transcendental (the matrix holds scaled probabilities), so modes 1 and 2 give the same traces bit for bit; the null2
 * contributions of the traces (p7_Null2_ByTrace) are computed on the host from segments and path codes by one piece of code for both,
 * and clustering is unchanged.  Against mode 0 the envelopes agree as two seeds of mode 0 agree.  In mode 2 a region with a trace of
 * more than 8 segments takes mode 1's walk on a copy of its matrix (more than 64: the serial one).  A region with a trace that is not
 * ok has no envelopes, as a failed serial ensemble has none.  bath_hip_std_ensemble_counters: regions (since the context was
 * created) that took the serial path from a stream mode, and that went from the kernel to the host twin; each region counts once;
 * kernel_regions: the regions std_ensemble_kernel walked. */
int         bath_hip_set_std_ensemble(bath_hip_ctx *ctx, int mode);
int         bath_hip_std_ensemble_counters(bath_hip_ctx *ctx, int64_t *serial_fallbacks, int64_t *twin_fallbacks, int64_t *kernel_regions);
/* Measurement aid: 1 = the envelope stage (bath_hip_fs5_envelopes and the domain stage's batches) runs its Backward wavefront AFTER the
 * Forward wavefront on the same stream instead of beside it, so that a kernel's HIP-event span is its time alone on the chip
 * (bench.py: fs.roofline.alone); 0 = side by side (the default); -1 = whatever BATH_HIP_FS_SERIAL says.  Results do not change. */
int         bath_hip_set_fs_serial(bath_hip_ctx *ctx, int on);

/* ------------------------------------------------------------------------------------------
 * Optimized profile (P7_OPROFILE surface).
 * ------------------------------------------------------------------------------------------ */
int  bath_hip_oprofile_convert(bath_hip_ctx *ctx, const bath_profile *gm, bath_hip_oprofile **ret); /* p7_oprofile_Convert, p7_oprofile.c:1091 */
void bath_hip_oprofile_destroy(bath_hip_oprofile *om);
/* P7_OPROFILE.consensus (impl_sse.h:128), consensus[1..M] as in bath_hmm: needed only for the hits' percent identity. */
int  bath_hip_oprofile_set_consensus(bath_hip_oprofile *om, const char *consensus);
int  bath_hip_oprofile_M(const bath_hip_oprofile *om);

/* Scalars of the limited-precision score systems (impl_sse.h:79-96), for L as configured by
 * p7_oprofile_ReconfigLength(om, L) (p7_oprofile.c:1261). */
typedef struct {
  uint8_t tbm_b, tec_b, tjb_b, base_b, bias_b;
  float   scale_b;
  int16_t xw[4][2];
  float   scale_w;
  int16_t base_w, ddbound_w;
  float   xf[4][2];
} bath_oprofile_scalars;
int  bath_hip_oprofile_scalars(const bath_hip_oprofile *om, int L, bath_oprofile_scalars *out);
/* p7_oprofile_GetSSVEmissionScoreArray (p7_oprofile.c:1507): arr[(M+1)*Kp], arr[k*Kp+x] */
int  bath_hip_oprofile_get_ssv_scores(const bath_hip_oprofile *om, uint8_t *arr);
/* unstriped views for parity tests: rw[Kp*(M+1)], tw[(M+1)*8] (MM IM DM BM MD DD MI II), rf, tf likewise */
int  bath_hip_oprofile_get_vit(const bath_hip_oprofile *om, int16_t *rw, int16_t *tw);
int  bath_hip_oprofile_get_fwd(const bath_hip_oprofile *om, float *rf, float *tf);

/* ------------------------------------------------------------------------------------------
 * Sequence blocks.  dsq holds n sequences back to back, sequence i = dsq[offsets[i] .. offsets[i+1]),
 * residues only (no sentinels), easel digital codes.
 * ------------------------------------------------------------------------------------------ */
int     bath_hip_seqs_create(bath_hip_ctx *ctx, const uint8_t *dsq, const int64_t *offsets, int64_t n, bath_hip_seqs **ret);
void    bath_hip_seqs_destroy(bath_hip_seqs *sq);
int64_t bath_hip_seqs_count(const bath_hip_seqs *sq);
/* The block as it lies on the device, copied to the host (for checks and tools): up to <cap> bytes of its data -- every sequence
 * at its offset, padded to 16 with 0x1d, 64 more padding bytes behind the last -- and, where the pointer is not NULL, the <n>
 * offsets, lengths and contexts (zeros when none are set).  Returns the number of data bytes the block holds, -1 on an error. */
int64_t bath_hip_seqs_read(const bath_hip_seqs *sq, uint8_t *data, int64_t cap, int64_t *offsets, int32_t *lengths, int32_t *context);
/* Windows of a long target (esl_sqio_ReadWindow with context, bathsearch.c:1099): context[i] = ESL_SQ.C of window i, the
 * leading nucleotides that also ended the previous window.  ORFs inside the context are skipped (p7_pipeline.c:1635-1637)
 * and only the new residues are counted in stats->nres (bathsearch.c:1258).  NULL clears it. */
int  bath_hip_seqs_set_context(bath_hip_seqs *sq, const int32_t *context);

/* Streamed blocks: what a host that feeds the GPU block after block uses instead of bath_hip_seqs_create.  The block arrives
 * in 2 bits per nucleotide (A, C, G, T = 0..3, nucleotide j of a sequence in bits 2(j%4).. of its byte j/4; every sequence starts
 * on a byte boundary, sequences back to back), 4x less to move over PCIe than the byte-per-nucleotide form; positions holding
 * any other code (degenerate nucleotides) come as an exception list.  bath_hip_seqs_create_packed lays the block out from its
 * offsets (in nucleotides) once; bath_hip_seqs_upload_packed queues the transfer of new content on the context's copy stream
 * and returns at once when <packed> is page-locked memory (bath_hip_host_alloc), so that the upload of the next block overlaps
 * the cascade of the current one; bath_hip_seqs_upload_wait orders the context's streams after the transfer and expands the
 * block on the device to the layout every kernel reads.  The block keeps its shape (offsets, lengths, contexts) across uploads. */
void *bath_hip_host_alloc(size_t bytes);
void  bath_hip_host_free(void *p);
int   bath_hip_seqs_create_packed(bath_hip_ctx *ctx, const int64_t *offsets, int64_t n, bath_hip_seqs **ret);
int   bath_hip_seqs_upload_packed(bath_hip_seqs *sq, const uint8_t *packed, const int64_t *exc_seq, const int32_t *exc_pos,
                                  const uint8_t *exc_code, int64_t n_exc);
int   bath_hip_seqs_upload_wait(bath_hip_seqs *sq);

/* ------------------------------------------------------------------------------------------
 * FASTA ingest on the device (bath_fasta.hip).  The raw bytes of a FASTA file go to HBM as they are, in chunks that may end
 * anywhere; kernels find the records, drop line breaks, digitise (the product's DNA alphabet, as bath_amd.digitize) and keep the
 * codes of every record resident.  Windows of the records (esl_sqio_ReadWindow: block_length new nucleotides after a context of
 * 3 * max_length) are then gathered from those codes into a bath_hip_seqs with its ESL_SQ.C context set.
 *
 * Rules: a record starts at a '>' that is the first byte of its line other than space, \t, \r, \v, \f; its header runs to the
 * end of that line.  In sequence lines those bytes and \n are skipped; ACGT-RYMKSWHBVDN*~ in either case are symbols, U reads T
 * and X reads N; any other byte, and anything but blank lines before the first record, is an error (bath_hip_fasta_error).
 * ------------------------------------------------------------------------------------------ */
typedef struct bath_hip_fasta bath_hip_fasta;
typedef struct {
  int64_t hdr_begin, hdr_end;   /* header bytes [hdr_begin, hdr_end) in the file: after the '>', up to the line's \n (excluded) */
  int64_t sym_start;            /* the record's first symbol in the stream of all the file's symbols */
  int64_t length;               /* nucleotides */
} bath_fasta_record;
typedef struct {
  int64_t target, start0;       /* window = record <target>[start0 : start0 + n] (0-based) */
  int32_t n, context;           /* its first <context> nucleotides are the previous window's (ESL_SQ.C) */
} bath_fasta_window;
int     bath_hip_fasta_create(bath_hip_ctx *ctx, bath_hip_fasta **ret);
void    bath_hip_fasta_destroy(bath_hip_fasta *f);
/* the next <n> bytes of the file: uploaded on the context's copy stream (asynchronously from page-locked memory), parsed on its
 * stream.  <bytes> may be reused when the call returns.  BATH_EINVAL on a format error: see bath_hip_fasta_error; the context
 * stays usable, the handle takes no more bytes. */
int     bath_hip_fasta_feed(bath_hip_fasta *f, const void *bytes, int64_t n);
int     bath_hip_fasta_finish(bath_hip_fasta *f);                       /* end of file: closes the last record */
int64_t bath_hip_fasta_count(bath_hip_fasta *f);                        /* records so far (the last may still be open) */
int64_t bath_hip_fasta_symbols(bath_hip_fasta *f);                      /* symbols so far */
int     bath_hip_fasta_records(bath_hip_fasta *f, int64_t lo, int64_t n, bath_fasta_record *out);
/* the first format error: its byte offset in the file, 1-based line, 0-based record (-1: before the first record), the byte */
int     bath_hip_fasta_error(const bath_hip_fasta *f, int64_t *offset, int64_t *line, int64_t *record, int32_t *byte);
/* the windows of records [lo, hi) (dist.split_targets): their number; written to <out> when <cap> allows */
int64_t bath_hip_fasta_windows(bath_hip_fasta *f, int64_t lo, int64_t hi, int32_t max_length, int32_t block_length, bath_fasta_window *out, int64_t cap);
/* a block of the given windows, laid out as bath_hip_seqs_create lays out sequences, with their contexts set */
int     bath_hip_fasta_seqs(bath_hip_fasta *f, const bath_fasta_window *w, int64_t n, bath_hip_seqs **ret);
/* The same block for another context of the handle's device: a search that runs several queries side by side, one context and one
 * host thread each, over one resident copy of the targets.  The block belongs to <consumer> (allocated for it, laid out as
 * bath_hip_fasta_seqs lays it out, contexts set; destroyed like any other); the gather runs on <consumer>'s stream, after that
 * stream has waited on an event recorded on the ingest stream behind the last feed / finish, and is complete when the call returns.
 * Ownership and ordering: the handle, its codes and its tables stay the creating context's.  Once the handle is finished, or
 * between two feeds, any number of host threads may call this at once, each with its own <consumer>, beside records / windows /
 * codes / seqs calls: the handle's host tables are read under a mutex inside it.  feed and finish must not run beside them.
 * bath_hip_fasta_release waits for every gather in flight before it frees codes, so the caller need not synchronise the
 * consumers first; blocks returned earlier are copies and stay valid.  Destroy the handle only after the last such call returned.
 * Errors are <consumer>'s (bath_hip_last_error(consumer)); the handle stays usable.  <consumer> may be the handle's own context. */
int     bath_hip_fasta_seqs_for(bath_hip_ctx *consumer, bath_hip_fasta *f, const bath_fasta_window *w, int64_t n, bath_hip_seqs **ret);
/* codes [start, start + n) of record <target> to the host (the windows of reported hits, for their alignments) */
int     bath_hip_fasta_codes(bath_hip_fasta *f, int64_t target, int64_t start, int64_t n, uint8_t *out);
/* drop the codes of the records before <lo> from device memory (a file streamed through a budget); their windows are gone.
 * Waits for the gathers of other contexts that are in flight (bath_hip_fasta_seqs_for). */
int     bath_hip_fasta_release(bath_hip_fasta *f, int64_t lo);

/* ------------------------------------------------------------------------------------------
 * Filter kernels, batched.  Each target i is scored exactly as the reference would after
 * p7_oprofile_ReconfigLength(om, L_i) (p7_pipeline.c:1644).  sc[n] nats, status[n] easel codes.
 * ------------------------------------------------------------------------------------------ */
int bath_hip_ssvfilter(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status);      /* p7_SSVFilter, ssvfilter.c:876 */
int bath_hip_msvfilter(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status);      /* p7_MSVFilter, msvfilter.c:74  */
int bath_hip_vitfilter(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status);      /* p7_ViterbiFilter, vitfilter.c:83 */
int bath_hip_forward_parser(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status); /* p7_ForwardParser, fwdback.c:132 */
/* The same scores by the group kernel of the cascade's Forward stage (fwd_group_kernel: a quarter wave per target, four targets of
 * a length-sorted list per wave; models of up to 160 nodes, BATH_EINVAL beyond).  Not bit-identical to bath_hip_forward_parser: the
 * cells' arithmetic is the same, the D scan and the sum over the model associate differently.  Contract: status equal, scores
 * within 1e-4 relative / 2e-4 absolute nats of p7_ForwardParser. */
int bath_hip_fwdparser_group(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *sc, int32_t *status);
/* p7_bg_NullOne + p7_bg_FilterScore (p7_bg.c:356,491) with p7_bg_SetFilter(bg, M, om->compo): nullsc[n], filtersc[n] */
int bath_hip_bias_filter(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, float *nullsc, float *filtersc);
/* p7_ForwardParser followed by p7_BackwardParser (fwdback.c:132,236) with the special-state rows p7_domaindef reads:
 * for target i, (L_i+1) rows of {E,N,J,B,C,SCALE} (P7_OMX xmx, impl_sse.h:253-262) at xmx_offsets[i] floats in fwd_xmx and
 * bck_xmx (either may be NULL).  Backward is scaled by Forward's per-row factors (fwdback.c:660-675).  Scores in nats;
 * status eslOK / eslERANGE per target (may be NULL). */
int bath_hip_fwdback_parser(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, const int64_t *xmx_offsets,
                            float *fwd_sc, float *bck_sc, int32_t *fwd_status, int32_t *bck_status, float *fwd_xmx, float *bck_xmx);

/* p7_ViterbiFilter_BATH (vitfilter.c:286) and p7_SSVFilter_BATH (msvfilter.c:250) over a block: the filter plus the hit windows
 * (P7_HMM_WINDOW, hmmer.h:998: position n in the target, last model node k, length; score only from the SSV variant) that
 * p7_pli_BuildDNAWindows and the local-composition re-filter read.  filtersc[n]: the bias-filter score of every target;
 * P: the P-value threshold (pli->F2 / pli->F1).  *wins is owned by ctx (valid until the next call), ordered by target, then
 * by position.  As in the pipeline each target is scored with the profile configured for its own length.
 * bath_hip_vitfilter_bath takes the cascade's own path: a batch of at least BATH_HIP_LANE_MIN_NT / 3 residues (default 150 M nt) of a
 * model of up to 224 nodes is sorted by length and scored by the lane-per-target kernel, its targets beyond 128 residues by the
 * wave-per-target kernel beside it; smaller batches by the wave-per-target kernel.  bath_hip_kernel_times then holds one span,
 * named after the kernel that ran: "vit_lane_kernel<NR>" or "vit_wave_kernel". */
typedef struct {
  int64_t target;                  /* index of the sequence in the block */
  int32_t n, k, length;
  float   score;
} bath_hmm_window;
int bath_hip_vitfilter_bath(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, const float *filtersc, double P,
                            float *sc, int32_t *status, const bath_hmm_window **wins, int64_t *nwins);
int bath_hip_ssvfilter_bath(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, double P,
                            const bath_hmm_window **wins, int64_t *nwins);

/* ------------------------------------------------------------------------------------------
 * The filter cascade of p7_Pipeline_BATH (p7_pipeline.c:1632-1791) over a block of DNA windows:
 * six-frame translation (esl_gencode_Process*, bathsearch.c:384-392), MSV, bias, Viterbi, Forward.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  double  F1, F2, F3, F4;         /* p7_pipeline.c:219-222 */
  int32_t do_biasfilter, fs_pipe, min_orf_len, ncbi_table;
  /* pli->nres on entry: the residues this search counted before the block's first window, both strands (bathsearch.c:1071,
   * :1084, :1258, :1268 add a window's W per strand before the window is searched).  The domain stage drops / flags a hit by
   * P * nres_running / max_length > E with the count AT THE HIT'S WINDOW AND STRAND (p7_domaindef.c:1033, p7_pipeline.c:1079,
   * :1246), so the hits of a block do not depend on how a search is cut into blocks as long as every block is told where it
   * starts; 0 for a search's first (or only) block. */
  int64_t nres_before;
  /* The rest of the option state p7_pipeline_Create_BATH keeps and the hot path reads (p7_pipeline.c:94-234; bathsearch.c:718-719,
   * :831-833).  bath_pipeline_params_default sets bathsearch's defaults; INTEGRATION.md section 4 maps each field to its pli-> member. */
  int32_t do_null2;               /* pli->do_null2: 1; --nonull2 clears it (:199, :213).  0: a hit's bias correction is 0 (:1063-1066, :1230-1233) */
  int32_t std_pipe;               /* pli->std_pipe: 1; --fsonly clears it (:107).  0: P_tot = 1 in the branch decision and a window that does not
                                   * take the frameshift branch is dropped (:1457, :1480)                                                          */
  int32_t strands;                /* pli->strands: BATH_STRAND_BOTH (0), _TOPONLY (--strand plus), _BOTTOMONLY (--strand minus); only the strands
                                   * searched are translated and counted in nres (bathsearch.c:1069, :1082, :1256, :1267)                          */
  int32_t initiator;              /* which codons may start an ORF (bathsearch.c:718-719): BATH_INIT_ANY (0, the default: esl_gencode_SetInitiatorAny),
                                   * BATH_INIT_TABLE (-M: the codon table's own start codons), BATH_INIT_AUG (-m: esl_gencode_SetInitiatorOnlyAUG).
                                   * With -m / -M the initiation codon is translated as M (esl_gencode_WorkstateCreate: using_initiators)           */
  int32_t inc_by_E;               /* pli->inc_by_E: 1; --incT clears it (:165-175).  The domain stage's early tests go by THIS flag, not by_E:
                                   * 1: drop / flag by P * Z > E (p7_domaindef.c:1034; :1080, :1247); 0: no early drop, flag by bit score >= T       */
  int32_t seed;                   /* --seed (:98): 42.  Every region's stochastic-trace ensemble starts from it (do_reseeding, p7_domaindef.c:781,
                                   * :904); 0: one arbitrary seed per process, the generator runs on from region to region (:140-143)                */
  double  T;                      /* pli->T: -T, 0.0 when not given (:148, :155); the early test's bit-score threshold when inc_by_E is 0           */
} bath_pipeline_params;
#define BATH_STRAND_BOTH       0
#define BATH_STRAND_TOPONLY    1
#define BATH_STRAND_BOTTOMONLY 2
#define BATH_INIT_ANY   0
#define BATH_INIT_TABLE 1
#define BATH_INIT_AUG   2

typedef struct {                   /* one per ORF that passed the MSV filter (P <= F1) */
  int64_t window;                  /* index of the DNA window in the block                               */
  int32_t strand, frame;           /* 0 top / 1 bottom; 0..2                                             */
  int32_t start, end;              /* 1-based nt coords on that strand (start<end), as esl_gencode gives */
  int32_t n;                       /* ORF length in aa                                                   */
  int32_t stage;                   /* 1 failed bias, 2 failed Vit, 3 failed Fwd, 4 passed (F3, or F4 if fs_pipe) */
  int32_t msv_status, vit_status;
  float   usc, nullsc, filtersc, vfsc, fwdsc;
  double  P;                       /* P-value at the stage where the ORF stopped                         */
} bath_orf_result;

typedef struct {                   /* pipeline counters, hmmer.h:1115-1128 */
  int64_t nres, n_orfs;
  int64_t n_past_msv, n_past_bias, n_past_vit, n_past_fwd;
  int64_t pos_past_msv, pos_past_bias, pos_past_vit, pos_past_fwd;
  int64_t cells_msv, cells_vit, cells_fwd;     /* sum of L*M per stage (Mc/s numerator, msvfilter.c:563) */
} bath_pipeline_stats;

/* Six-frame translation of a block of DNA windows: esl_gencode_ProcessStart/Piece/End as driven by
 * bathsearch.c:384-392 (both strands, no initiator requirement; windows < 15 nt skipped, bathsearch.c:1066).
 * Every maximal run of non-stop codons of >= min_orf_len residues is one ORF. */
typedef struct {
  int64_t window;                  /* index in the block                                                   */
  int32_t strand, frame;           /* 0 = as given, 1 = reverse complement; frame 0..2                      */
  int32_t start, end;              /* 1-based nt coordinates on that strand (orfsq->start/end convention)   */
  int32_t n;                       /* residues                                                              */
  int64_t aa_off;                  /* residues of this ORF are aa[aa_off .. aa_off+n)                       */
} bath_orf;
/* On return *orfs (sorted by window, strand, frame, start) and *aa are owned by ctx, valid until the next call. */
int  bath_hip_translate_orfs(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int ncbi_table, int min_orf_len,
                             const bath_orf **orfs, int64_t *n_orfs, const uint8_t **aa);
/* ... for one strand only and / or with initiation codons (bath_pipeline_params.strands, .initiator) */
int  bath_hip_translate_orfs_opts(bath_hip_ctx *ctx, const bath_hip_seqs *dna, int ncbi_table, int min_orf_len, int strands, int initiator,
                                  const bath_orf **orfs, int64_t *n_orfs, const uint8_t **aa);
/* The length-sorted ORF work list the last bath_hip_translate_orfs[_opts] call built on the device, as the sort left it: longest
 * first (lengths from 2047 up share the first bin), the order within a bin not defined.  aa_off is the ORF's offset in the
 * device's amino-acid stream pool, len_sf = residues | (strand*3 + frame) << 28.  Owned by ctx, valid until the next call. */
typedef struct {
  int64_t aa_off;
  int32_t window;
  int32_t len_sf;
} bath_orf_work;
int  bath_hip_orf_worklist(bath_hip_ctx *ctx, const bath_orf_work **list, int64_t *n);
/* gcode->is_initiator[16 a + 4 b + c] (easel codes A C G T = 0..3) under <initiator>; the table's own start codons are NCBI's
 * (gc.prt "sncbieaa" line); easel's copy is not in the reference tree, so BATH_INIT_TABLE is parity-unpinned */
int  bath_gencode_initiators(int ncbi_table, int initiator, uint8_t is_init[64]);

void bath_pipeline_params_default(bath_pipeline_params *p, int fs_pipe);
/* Runs the cascade on every window of <dna>, both strands.  On return *results points to an array of
 * *n_results records owned by ctx (valid until the next call); pass NULL to skip the copy-out. */
int  bath_hip_pipeline_filters(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna,
                               const bath_pipeline_params *params, bath_pipeline_stats *stats,
                               const bath_orf_result **results, int64_t *n_results);
/* Device time of the stages of the last bath_hip_pipeline_filters call, ms (HIP events on ctx's stream).
 * names[i] are static strings. */
int  bath_hip_pipeline_timings(const bath_hip_ctx *ctx, int max, const char **names, float *ms, int64_t *launches);

/* Device time of every kernel of the stages AFTER the cascade (3-codon parsers, region heuristics, 5-codon envelope kernels,
 * tracebacks) launched by the last bath_hip_pipeline_frameshift_domains call, aggregated by kernel name: HIP events on the stream
 * each kernel ran on.  cells = DP cells (rows x nodes) the launches covered, bytes = their algorithmic HBM traffic (the matrix
 * bytes the kernel must read and write).  Returns the number of entries written (<= max). */
typedef struct {
  const char *name;                /* static string */
  float   ms;
  int64_t launches;
  double  cells, bytes;
} bath_kernel_time;
int  bath_hip_kernel_times(bath_hip_ctx *ctx, int max, bath_kernel_time *out);

/* The frameshift pipeline (bathsearch --fs) up to the decision which branch a DNA window takes:
 * the cascade with F4 at the Forward stage (p7_pipeline.c:1774-1789), then p7_pli_BuildDNAWindows (:462-572) and the
 * per-window part of p7_pli_Frameshift (:1368-1464): summed ORF score, window null / bias scores
 * (p7_bg_fs_NullOne, p7_bg_fs_FilterScore), p7_ForwardParser_Frameshift_3Codons, and the P-value comparison.
 * Domain definition after the decision is not part of this library yet. */
typedef struct {
  int64_t window;                  /* sequence index in the block                                            */
  int32_t strand;                  /* 0 = as given, 1 = reverse complement                                    */
  int32_t n, length;               /* window start (1-based on that strand) and length, nt (P7_HMM_WINDOW n, length) */
  int32_t orf_cnt, k_min, k_max;   /* ORFs with P <= F4 inside the window; model range of their hit windows   */
  float   tot_orfsc;               /* log-sum of the ORFs' (Forward - null) scores, nats (:1408)             */
  float   nullsc, filtersc, fwdsc; /* of the DNA window: null, bias-filter and frameshift Forward scores      */
  double  P_tot, P_min, P_fs, P_null;
  int32_t branch;                  /* 1: frameshift branch (:1464); 2: standard branch (:1479); 0: neither (--fsonly, :1480) */
} bath_fs_window;
/* <om_fs3> is the 3-codon frameshift profile.  stats->pos_past_fwd counts as the reference does in this mode
 * (:1468, :1490).  *fs_windows is owned by ctx, valid until the next call; results/n_results as in
 * bath_hip_pipeline_filters (may be NULL). */
int  bath_hip_pipeline_frameshift(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3,
                                  const bath_hip_seqs *dna, const bath_pipeline_params *params, bath_pipeline_stats *stats,
                                  const bath_orf_result **results, int64_t *n_results,
                                  const bath_fs_window **fs_windows, int64_t *n_fs_windows);

/* ... and what the frameshift branch does next (p7_pipeline.c:1469-1476): p7_BackwardParser_Frameshift_3Codons,
 * p7_domaindef_ByPosteriorHeuristics_Frameshift_BATH (p7_domaindef.c:301) with rescore_isolated_domain_frameshift (:993)
 * for single-domain regions, and the scores p7_pli_postDomainDef_Frameshift_BATH (p7_pipeline.c:1005) gives the hit.
 * Multi-domain regions are resolved by stochastic-trace clustering (p7_domaindef.c:396-455); *n_clustered_regions counts them
 * (ddef->nclustered; the name predates that stage). */
typedef struct {
  int64_t window;                  /* sequence index in the block                                              */
  int32_t strand;
  int32_t fs_window;               /* index into the fs_windows array                                          */
  int32_t ienv, jenv, iali, jali;  /* nt coordinates on the sequence, as P7_DOMAIN ienv/jenv/iali/jali (:1035-1049) */
  int32_t ihmm, jhmm;              /* first / last model node of the optimal-accuracy alignment                */
  float   envsc, oasc;             /* envelope Forward score (nats), expected number of correctly aligned residues */
  float   domcorrection, dombias;  /* null2 correction and the bias term derived from it, nats (:1064)          */
  float   bitscore, pre_score;     /* the hit's score in bits (hit->score) and before the null2 correction       */
  double  lnP;
  int32_t reported;                /* exp(lnP) * Z <= E_report, Z = nres of the block / max_length (:1080)      */
  int32_t n_shifted_codons;        /* match states of the alignment that emit a quasi-codon (length != 3)        */
  /* what --tblout prints of the alignment display (p7_alidisplay.c:538-935, 937-1245) */
  int32_t n_stops;                 /* aligned codons that are stop codons (ad->stops)                            */
  float   pid;                     /* percent of alignment columns whose residue is the consensus residue (ad->pid); 0 without a consensus */
  int32_t ali_columns;             /* ad->N: trace states from the first to the last match state                  */
  int64_t cigar_off;               /* the --cigar string starts at bath_hip_domain_cigars(ctx) + cigar_off        */
} bath_fs_domain;
const char *bath_hip_domain_cigars(const bath_hip_ctx *ctx);   /* NUL-terminated strings, valid until the next pipeline call */

/* P7_DOMAIN.tr: the optimal-accuracy trace of every domain of the last bath_hip_pipeline_hits / _frameshift_domains call, with its
 * posterior probabilities, as rescore_isolated_domain_frameshift / _bath keep it (p7_domaindef.c:1171, :1330) and as
 * p7_alidisplay_fs_Create / _nonfs_Create (p7_alidisplay.c:538, :937) and p7_tophits_TabularFrameshifts read it -- what the
 * alignment blocks of the default output and --fstblout are made from.  tr[d] belongs to domains[d] of that call.
 * Per trace state z = tr[d].off .. tr[d].off + tr[d].N - 1, in the reference's conventions (p7_trace_fs_AppendWithPP, p7_trace.c:2303;
 * p7_trace_fs_Convert, :405):
 *   st[z]  BATH_T_M / BATH_T_D / BATH_T_I (p7T_M, p7T_D, p7T_I; hmmer.h:487)
 *   k[z]   model node
 *   i[z]   M, I: the codon's LAST nucleotide, 1-based in windowsq -- the DNA window the domain was defined on: nucleotide
 *          win_start + i - 1 of the strand read (for a hit of the plain pipeline windowsq is the ORF's own stretch of DNA,
 *          p7_pipeline.c:1755); D: what the reference leaves there (the envelope's start - 1 in the frameshift branch, 0 in the standard one)
 *   c[z]   M: the (quasi-)codon's length 1..5 (always 3 in the standard branch); 0 otherwise
 *   pp[z]  M, I: the state's posterior probability; D: 0
 * The states are those from the first to the last match state (ad->N of them): the N / B / E / C flanks of the reference's trace carry
 * nothing any caller on this path reads (both alidisplay constructors and TabularFrameshifts start at the first M) and are not
 * materialised.  The arrays are owned by ctx and valid until its next pipeline call. */
#define BATH_T_M 1
#define BATH_T_D 2
#define BATH_T_I 3
typedef struct {
  int64_t off;                     /* first state of this trace in the arrays                                           */
  int32_t N;                       /* states (alignment columns, ad->N)                                                  */
  int32_t win_start;               /* windowsq->start on the strand read, 1-based                                        */
  int32_t orf_start;               /* standard branch: orfsq->start on the strand read (its first codon reads M under -m / -M); 0 in the frameshift branch */
  int32_t frameshift;              /* 1: a domain of the frameshift branch (p7_alidisplay_fs_Create), 0: of the standard branch (_nonfs_Create) */
} bath_domain_trace;
int bath_hip_domain_traces(bath_hip_ctx *ctx, const bath_domain_trace **tr, int64_t *n_traces,
                           const int8_t **st, const int32_t **k, const int32_t **i, const int8_t **c, const float **pp);

/* The alignment block of a hit as the default output prints it under "Alignment:" (p7_alidisplay_fs_Create / _nonfs_Create,
 * p7_alidisplay.c:538-1243, and p7_alidisplay_Print_BATH, :3757-4110, as p7_tophits_Domains calls it: p7_tophits.c:1394), from one
 * trace of bath_hip_domain_traces: the optional CS / RF lines, the model's consensus, the match line, the translation, the codons
 * (a quasi-codon's missing or extra nucleotides marked as the reference marks them), the optional frame line and the posterior
 * probability line, in blocks of (textw - names - coordinates) / 5 columns.  Host code; nothing here touches the GPU.
 *   st .. pp      the arrays of bath_hip_domain_traces, already offset to this trace (st + tr->off, ...)
 *   window_dsq    windowsq: window_dsq[i - 1] is nucleotide i of the strand read (digital), <window_len> of them -- for a domain d
 *                 of a block: the strand's nucleotides from tr->win_start on
 *   gm_fs5 / gm   the 5-codon frameshift profile (frameshift branch) / the standard profile (standard branch); the other may be NULL
 *   basic         the codon table (bath_gencode_basic), standard branch
 * Returns the text's size in bytes (without a terminating NUL) and copies at most <cap> of them to <buf>; < 0 on error. */
typedef struct {
  const char *hmm_name, *seq_name;   /* ad->hmmname, ad->sqname (the caller substitutes accessions under --acc)            */
  const char *consensus;             /* bath_hmm.consensus                                                                  */
  const char *rf, *cs;               /* bath_hmm.rf / .cs or NULL                                                           */
  int32_t M;
  int64_t sqfrom, sqto;              /* ad->sqfrom / ad->sqto: the hit's iali / jali on the sequence                       */
  int32_t textw;                     /* --textw (150); <= 0: one block of unlimited width (--notextw)                       */
  int32_t show_frameline;            /* --frameline                                                                         */
  int32_t initiator;                 /* bath_pipeline_params.initiator: under -m / -M an ORF's first codon reads M          */
} bath_alidisplay_opts;
int64_t bath_alidisplay_print(const bath_domain_trace *tr, const int8_t *st, const int32_t *k, const int32_t *i, const int8_t *c, const float *pp,
                              const uint8_t *window_dsq, int32_t window_len, const bath_fs_profile *gm_fs5, const bath_profile *gm,
                              const uint8_t basic[64], const bath_alidisplay_opts *opts, char *buf, int64_t cap);
int  bath_hip_pipeline_frameshift_domains(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3,
                                          const bath_hip_fsprofile *om_fs5, const bath_hip_seqs *dna, const bath_pipeline_params *params,
                                          double E_report, bath_pipeline_stats *stats,
                                          const bath_fs_window **fs_windows, int64_t *n_fs_windows,
                                          const bath_fs_domain **domains, int64_t *n_domains, int64_t *n_clustered_regions);

/* The standard pipeline (bathsearch without --fs) after the Forward filter (p7_pipeline.c:1741-1771): p7_BackwardParser,
 * p7_domaindef_ByPosteriorHeuristics_BATH (p7_domaindef.c:491) with rescore_isolated_domain_bath (:1194) for single-domain
 * regions, p7_pli_postDomainDef_BATH (p7_pipeline.c:1172).  One bath_fs_domain per hit (fs_window = -1,
 * n_shifted_codons = 0).  Multi-domain regions are resolved by stochastic-trace clustering (p7_domaindef.c:539-583);
 * *n_clustered_regions counts them (ddef->nclustered). */
int  bath_hip_pipeline_hits(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *dna,
                            const bath_pipeline_params *params, double E_report, bath_pipeline_stats *stats,
                            const bath_fs_domain **domains, int64_t *n_domains, int64_t *n_clustered_regions);

/* Full-matrix forms over a block of amino-acid targets (the batched twins of impl_sse's single-target functions):
 *   bath_hip_forward_full  <- p7_Forward (fwdback.c:94): Forward matrices (L_i+1) x (M+1) x {M,D,I} (odds ratios, scaled per row
 *       like the parser) back to back in <dp>, special-state rows (L_i+1) x {E,N,J,B,C,SCALE} in <xmx> (either may be NULL).
 *       cfg_len[n] (or NULL: each target's own length) is the length the profile is configured for
 *       (p7_oprofile_ReconfigLength / ReconfigMultihit, p7_domaindef.c:560 uses the ORF's saved length for a region);
 *       unihit != 0: p7_oprofile_ReconfigUnihit.  This is what p7_StochasticTrace walks.
 *   bath_hip_std_envelopes <- p7_Forward + p7_Backward + p7_Decoding + p7_OptimalAccuracy + p7_Null2_ByExpectation on envelopes
 *       (rescore_isolated_domain_bath, p7_domaindef.c:1194-1262; unihit, L = L_i): scores, null2[Kp], posterior matrices <pp>
 *       and optimal-accuracy matrices <oa> in the Forward matrix layout, posterior / OA special-state rows (L_i+1) x {E,N,J,B,C}
 *       in <ppx> / <oax> (any of the four may be NULL).
 *   bath_hip_std_envelopes_fill: the same with the domain stage's choice of kernels made by the caller -- fill 0: one lane per
 *       envelope does everything (bath_hip_std_envelopes); 1: std_envelope_fill_kernel<C>, a wave per envelope, for the model's C,
 *       then the traceback; 2: std_envelope_fill_mw_kernel<C>, a block of four waves per envelope.  1 and 2 take models of up to
 *       1024 nodes (BATH_ERANGE beyond).  The matrices are those the stage's traceback reads; row 0 of <pp> is not part of them. */
typedef struct {
  float   fwdsc, bcksc, oasc;
  int32_t fwd_status, bck_status, ok;       /* ok == 0: numeric range error in decoding (eslERANGE), the domain is dropped */
  float   null2[BATH_KP_AMINO];
} bath_std_result;
int bath_hip_forward_full(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, const int32_t *cfg_len, int unihit,
                          float *sc, int32_t *status, float *dp, float *xmx);
int bath_hip_std_envelopes(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, bath_std_result *res,
                           float *pp, float *oa, float *ppx, float *oax);
int bath_hip_std_envelopes_fill(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *sq, bath_std_result *res,
                                float *pp, float *oa, float *ppx, float *oax, int fill);

/* ------------------------------------------------------------------------------------------
 * Hit list of a search and its tabular output (P7_TOPHITS; host code).
 * What bathsearch does after its workers finish (bathsearch.c:868-921): p7_tophits_ComputeEvalues_BATH
 * (p7_tophits.c:789), SortBySeqidxAndAlipos (:379), RemoveDuplicates (:816), SortBySortkey (:345), Threshold (:914),
 * p7_tophits_TabularTargets (:1603) for --tblout and p7_tophits_TabularFrameshifts (:1428) for --fstblout.
 * ------------------------------------------------------------------------------------------ */
typedef struct bath_tophits bath_tophits;
bath_tophits *bath_tophits_create(void);
void bath_tophits_destroy(bath_tophits *th);
/* One hit per domain with reported != 0 (the pipeline's own E-value test, p7_pipeline.c:1080,1246).  <cigars> is
 * bath_hip_domain_cigars(ctx) or NULL; the block's sequence w has global index seqidx0 + w, name seq_names[w], length
 * seq_lens[w]; seq_accs / seq_descs may be NULL. */
int  bath_tophits_add(bath_tophits *th, const bath_fs_domain *dom, int64_t n, const char *cigars, int64_t seqidx0,
                      const char *const *seq_names, const char *const *seq_accs, const char *const *seq_descs, const int64_t *seq_lens);
/* <nres>: residues searched, both strands (sum of the pipelines' nres); E: reporting threshold (-E, default 10). */
int  bath_tophits_finalize(bath_tophits *th, int64_t nres, int max_length, double E);
/* Reporting / inclusion by bit score (p7_pli_TargetReportable / p7_pli_TargetIncludable, p7_pipeline.c:583-603), before finalize:
 * by_E = 0 (-T): a hit is reported when score >= T instead of exp(lnP) <= E; inc_by_E = 0 (--incT): included when score >= incT
 * instead of exp(lnP) <= incE.  Defaults: both by E. */
void bath_tophits_set_score_thresholds(bath_tophits *th, int by_E, double T, int inc_by_E, double incT);
/* The residue count bathsearch hands p7_tophits_ComputeEvalues_BATH (bathsearch.c:868-881): with -Z <x> it is 1e6 * x, doubled when
 * both strands are searched, whatever was searched; without, the sum of the workers' pli->nres.  Pass the result to
 * bath_tophits_finalize as <nres>. */
int64_t bath_search_space_residues(int Z_is_set, double Z_megabases, int strands, int64_t nres_searched);
int64_t bath_tophits_count(const bath_tophits *th);       /* hits held, reported or not */
int64_t bath_tophits_reported(const bath_tophits *th);
#define BATH_HIT_REPORTED  1
#define BATH_HIT_DUPLICATE 4
/* The rank-th hit in the current sort order (by E-value after finalize); dom->lnP is the E-value's log after finalize. */
int  bath_tophits_get(const bath_tophits *th, int64_t rank, bath_fs_domain *dom, int64_t *seqidx, int32_t *flags);
/* Returns the table's size in bytes and copies at most <cap> of them to <buf>. */
/* p7_tophits_Targets (:1073): the "Scores for complete hits" block of the main output; textw = --textw (120; <= 0 unlimited). */
int64_t bath_tophits_targets(const bath_tophits *th, int fs_pipe, int textw, char *buf, int64_t cap);
/* Head of the rank-th hit's entry under "Annotation for each hit" (p7_tophits_Domains, :1256-1378): ">> name", the two header
 * lines and the hit's line; 0 for a hit that is not reported.  The alignment block itself is not produced. */
int64_t bath_tophits_domain_annotation(const bath_tophits *th, int64_t rank, int M, int fs_pipe, char *buf, int64_t cap);
/* p7_pli_Statistics (p7_pipeline.c:1836): the "Internal pipeline statistics summary" block without its two timing lines. */
int64_t bath_tophits_pipeline_statistics(const bath_tophits *th, const bath_pipeline_stats *stats, const bath_pipeline_params *params,
                                         int64_t nmodels, int64_t nnodes, int64_t nseqs, char *buf, int64_t cap);
void bath_tophits_set_inclusion(bath_tophits *th, double incE);   /* --incE, default 0.01; before finalize */
#define BATH_HIT_INCLUDED  2
int64_t bath_tophits_tabular_targets(const bath_tophits *th, const char *qname, const char *qacc, int M, int fs_pipe,
                                     int show_cigar, int show_header, char *buf, int64_t cap);

/* --fstblout: where a coding region is broken (p7_tophits_TabularFrameshifts, p7_tophits.c:1428-1582).  Host code.
 * bath_trace_frameshift_rows: the rows of one hit, from its trace as bath_hip_domain_traces / bath_hits_traces give it (st .. c
 *   already offset to this trace), window_dsq / window_len as bath_alidisplay_print takes them, the 5-codon frameshift profile and
 *   the hit's iali / jali on the sequence.  Walking the states with ali_pos = 1 at the first match state:
 *     M on a quasi-codon of 1 / 2 nt   'D', length 2 / 1        M on 4 / 5 nt   'I', length 1 / 2
 *     M on a stop codon                'S', length 0  (the renderer's rule for ad->codon == 6)
 *   then ali_pos += the codon's length; I: no row, even on a stop codon, ali_pos += 3; D: no row, no advance.  So a hit can have
 *   fewer 'S' rows than its n_stops, which counts the stops of insert states too.  ali_start is ali_pos before the advance,
 *   seq_start = iali + ali_pos - 1 (iali < jali) or iali - ali_pos + 1.  A trace with frameshift == 0 has no rows.
 *   Returns the number of rows and writes at most <cap> of them to <rows> (which may be NULL); < 0 on error.
 * bath_tophits_tabular_frameshifts: the table of every hit with BATH_HIT_REPORTED in the list's current order; the rows of the
 *   r-th of them are rows[row_off[r] .. row_off[r + 1]), n_reported = bath_tophits_reported(th).  Column widths as --tblout's, over
 *   every hit of the list.  The two header lines are written when show_header is set AND the list holds a hit of any kind, as the
 *   reference does: a first query without hits leaves the file without a header.  The E-value is --tblout's.
 *   Returns the table's size in bytes and copies at most <cap> of them to <buf>; < 0 on error. */
typedef struct {
  char    type;                      /* 'D' nucleotides missing from the codon, 'I' extra nucleotides in it, 'S' a stop codon */
  int32_t length;                    /* nucleotides missing / extra; 0 for 'S'                                                 */
  int32_t ali_start;                 /* 1-based position in the alignment's own nucleotides                                    */
  int64_t seq_start;                 /* the same position on the target sequence                                               */
} bath_fs_row;
int64_t bath_trace_frameshift_rows(const bath_domain_trace *tr, const int8_t *st, const int32_t *k, const int32_t *i, const int8_t *c,
                                   const uint8_t *window_dsq, int32_t window_len, const bath_fs_profile *gm_fs5, int64_t iali, int64_t jali,
                                   bath_fs_row *rows, int64_t cap);
int64_t bath_tophits_tabular_frameshifts(const bath_tophits *th, const char *qname, const char *qacc, const bath_fs_row *rows,
                                         const int64_t *row_off, int64_t n_reported, int show_header, char *buf, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * One search on several GPUs from a C host: the hit list as a byte stream and the division of the work.
 * Host code; the host's own transport (MPI, RCCL, sockets) moves the bytes.
 *
 * Hits between processes.  The reference ships a hit as p7_hit_Serialize writes it (src/p7_hit.c:174-411; read back by
 * p7_hit_Deserialize, :411-640): a self-delimiting record -- its own size first, every fixed-width field in NETWORK byte order, a
 * byte of presence flags, optional strings NUL-terminated -- followed by its domain and alignment.  The same scheme here:
 *   stream  := u32 magic "BHIT" | u32 version (1) | u64 n_hits | n_hits x hit
 *   hit     := u32 size of this record | i64 window | i32 strand, fs_window, ienv, jenv, iali, jali, ihmm, jhmm | f32 envsc, oasc,
 *              domcorrection, dombias, bitscore, pre_score | f64 lnP | i32 reported, n_shifted_codons, n_stops | f32 pid |
 *              i32 ali_columns | u8 flags (1: CIGAR present, 2: trace present) | [cigar, NUL-terminated] |
 *              [i32 N, win_start, orf_start, frameshift | N x (u8 st, u8 c, i32 k, i32 i, f32 pp)]
 * all integers and IEEE floats big-endian (esl_hton32 / esl_hton64 as p7_hit.c applies them).
 * bath_hits_serialize returns the stream's size in bytes and writes it to <buf> when <buf> is not NULL and <cap> suffices (-1: bad
 * arguments or <cap> too small); <cigars> is bath_hip_domain_cigars(ctx) or NULL; <tr> .. <pp> are bath_hip_domain_traces' outputs
 * or all NULL (hits without their traces: enough for --tblout, not for the alignment blocks).
 * ------------------------------------------------------------------------------------------ */
typedef struct bath_hits bath_hits;                 /* a deserialized hit list; owns its arrays */
int64_t bath_hits_serialize(const bath_fs_domain *dom, int64_t n, const char *cigars, const bath_domain_trace *tr,
                            const int8_t *st, const int32_t *k, const int32_t *i, const int8_t *c, const float *pp,
                            uint8_t *buf, int64_t cap);
int     bath_hits_deserialize(const uint8_t *buf, int64_t nbytes, bath_hits **ret);     /* BATH_EFORMAT for a stream that is not one */
int64_t bath_hits_stream_size(const uint8_t *buf, int64_t nbytes);   /* bytes of the stream starting at buf (streams may lie back to back in a message); -1: not a stream */
void    bath_hits_destroy(bath_hits *h);
int64_t bath_hits_count(const bath_hits *h);
bath_fs_domain *bath_hits_domains(bath_hits *h);    /* cigar_off points into bath_hits_cigars(); -1: the hit came without one */
const char *bath_hits_cigars(const bath_hits *h, int64_t *nbytes);
int     bath_hits_traces(const bath_hits *h, const bath_domain_trace **tr, const int8_t **st, const int32_t **k, const int32_t **i,
                         const int8_t **c, const float **pp);                           /* BATH_EINVAL when the stream carried none */
/* p7_tophits_Merge from a byte stream (bathsearch.c:884-888): the hits of another rank join <th>.  <window_shift> is added to every
 * hit's window index (a rank that searched windows [lo, hi) of the search numbers them from 0); <n_seqs> is the length of the
 * seq_* arrays: a hit whose shifted window is not in [0, n_seqs) -- a damaged or mismatched stream, a wrong shift -- is refused with
 * BATH_EFORMAT and nothing is added; the rest as bath_tophits_add. */
int     bath_tophits_add_serialized(bath_tophits *th, const uint8_t *buf, int64_t nbytes, int64_t window_shift, int64_t n_seqs, int64_t seqidx0,
                                    const char *const *seq_names, const char *const *seq_accs, const char *const *seq_descs, const int64_t *seq_lens);

/* Division of the work, the same on every rank without communication.
 * bath_dist_shard_range: rank r's contiguous share [lo, hi) of n units (windows of one search over the ranks: configs[1], [2], [4]).
 * bath_dist_items: a multi-query job (bathsearch's loop over an HMM database, bathsearch.c:737-844; configs[3]) as (query, window
 *   group) items: query q's windows [0, n_q) in g_q consecutive groups, g_q = round(cost_q / sum of costs x T) clipped to [1, n_q],
 *   T = max(queries, items_per_rank x world); costs NULL: g_q = ceil(items_per_rank x world / queries) for every query.  A useful
 *   cost is windows x (M + 150).  Returns the number of items; writes at most <cap>.
 * bath_dist_deal: owner rank of every item, longest processing time first onto the least loaded rank (ties: earlier item, lower rank). */
typedef struct { int32_t query; int64_t lo, hi; } bath_dist_item;
void    bath_dist_shard_range(int64_t n, int rank, int world, int64_t *lo, int64_t *hi);
int64_t bath_dist_items(const int64_t *n_windows_by_query, const double *costs_by_query, int n_queries, int world, int items_per_rank,
                        bath_dist_item *items, int64_t cap);
int     bath_dist_deal(const double *costs, int64_t n_items, int world, int32_t *owner);

/* ------------------------------------------------------------------------------------------
 * Frameshift kernels (P7_FS_OPROFILE surface), batched over DNA windows.
 * ------------------------------------------------------------------------------------------ */
#define BATH_LOGSUM_TABLE 0   /* emulate p7_FLogsum's 0.001-nat truncating table (logsum.c:105) */
#define BATH_LOGSUM_EXACT 1   /* exact log(1+exp(x))                                            */
#define BATH_LOGSUM_TABLE_SERIAL 2 /* the table, sums along the model in the reference's serial order: bit-identical to generic_fwdback_frameshift.c */
#define BATH_LOGSUM_CONTEXT 3 /* whatever bath_hip_set_fs_strict selected for the context: TABLE_SERIAL unless switched to the fast mode
                                 (fs3 entry points: ODDS when bath_hip_set_fs_odds switched it on; fs5 entry points: the
                                 5-codon odds-ratio kernels when bath_hip_set_fs5_odds switched them on) */
/* BATH_LOGSUM_ODDS (3-codon parsers only; the fs5 entry points answer BATH_EINVAL): what the reference's bathsearch --fs runs,
 * p7_{Forward,Backward}Parser_Frameshift_3Codons (impl_sse/fwdback_fs.c:97, :565) -- the recursion in fp32 odds ratios (expf of the
 * profile's scores), no log-sum table, every value of the recursion rescaled together when E(i) (Backward: B(i)) passes 1e4.
 * Contract: scores within 1e-3 + 1e-4 |s| nats of EXACT log-space arithmetic (the reference's own SIMD-vs-generic bar with exact
 * log-sums, fwdback_fs.c:3189-3191), the special-state rows (log value + the accumulated scale, the layout of every mode) within
 * 2e-3 + 2e-4 |v| where the exact value is above -60 (Backward: within 40 nats of its row's largest value); values that far below
 * the scale flush to zero in fp32 and come back as -inf.  A window whose C(L) terms underflow (the reference's eslERANGE) scores -inf.
 * NOT bit-identical to the generic reference: against the strict mode's table log-sums scores differ by up to ~1e-2 nats on long
 * windows, so a window at a threshold may take the other branch and a domain may move. */
#define BATH_LOGSUM_ODDS 4

int  bath_hip_fsprofile_convert(bath_hip_ctx *ctx, const bath_fs_profile *gm_fs, bath_hip_fsprofile **ret); /* p7_fs_oprofile_Convert, p7_fs_oprofile.c:221 */
void bath_hip_fsprofile_destroy(bath_hip_fsprofile *om);

/* p7_ForwardParser_Frameshift_3Codons (fwdback_fs.c:97) / p7_GForwardParser_Frameshift_3Codons
 * (generic_fwdback_frameshift.c:451): per window i, after p7_fs_oprofile_ReconfigLength(om, L_i/3).
 * xmx (optional) receives the special-state rows: for window i, (L_i+1)*5 floats {E,N,J,B,C} at xmx_offsets[i]. */
int bath_hip_fs3_forward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, int logsum_mode,
                                float *sc, float *xmx, const int64_t *xmx_offsets);
int bath_hip_fs3_backward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om3, const bath_hip_seqs *dna, int logsum_mode,
                                 float *sc, float *xmx, const int64_t *xmx_offsets);  /* fwdback_fs.c:565 / generic :1422 */

/* Envelope rescoring (p7_domaindef.c:993-1082): p7_Forward_Frameshift + p7_Backward_Frameshift +
 * p7_Decoding_Frameshift + p7_OptimalAccuracy_Frameshift fill + p7_Null2_fs_ByExpectation, one
 * envelope per sequence of <dna>, unihit profile reconfigured to L_i/3.
 * c5_compat: 1 = generic_fwdback_frameshift.c:324 ring aliasing for 5-nt codons, 0 = fwdback_fs.c:1464. */
typedef struct {
  float fwdsc, bcksc, oasc;
  float null2[BATH_KP_AMINO];
} bath_fs5_result;
int bath_hip_fs5_envelopes(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                           bath_fs5_result *res,
                           float *pp /* optional: posterior matrices, (L_i+1)*(M+1)*8 floats at pp_offsets[i] */, const int64_t *pp_offsets,
                           float *oa /* optional: OA matrices (L_i+1)*(M+1)*3 */, const int64_t *oa_offsets);

/* bath_hip_fs5_envelopes with the special-state rows as well: posterior rows <ppx> and optimal-accuracy rows <oax>,
 * (L_i+1) x {E,N,J,B,C} per envelope, back to back (either may be NULL). */
int bath_hip_fs5_envelopes_x(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int logsum_mode, int c5_compat,
                             bath_fs5_result *res, float *pp, float *oa, float *ppx, float *oax);
/* p7_Forward_Frameshift in the MULTIHIT configuration of amino length <cfg_len_amino> (p7_domaindef.c:411-414: the model's saved
 * length): sc[n]; Forward matrices (L_i+1) x (M+1) x {D, I, M_C0, M_C1..M_C5} in <fwd>, special-state rows (L_i+1) x {E,N,J,B,C}
 * in <xmx>, back to back (either may be NULL).  This is what p7_StochasticTrace_Frameshift walks. */
int bath_hip_fs5_forward_full(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int cfg_len_amino,
                              float *sc, float *fwd, float *xmx);

/* The score of bath_hip_fs5_forward_full and nothing else (p7_Forward_Frameshift in the multihit local configuration of
 * <cfg_len_amino>; what p7_fs_Tau_5codons needs of p7_ForwardParser_Frameshift_5Codons): no DP matrix and no special-state row goes
 * to global memory.  sc[n]; a window shorter than 5 nt scores -inf.  Always the strict arithmetic (serial table log-sums, bit-identical
 * to the generic reference): bath_hip_set_fs_strict and bath_hip_set_fs5_odds do not reach this entry point. */
int bath_hip_fs5_forward_parser(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int cfg_len_amino, float *sc);
/* The same score in the reference's arithmetic: the multihit score of bath_hip_fs5_forward_full under bath_hip_set_fs5_odds, bit for
 * bit, and nothing else (the 5-codon odds-ratio Forward instantiated without its stores; what p7_fs_Tau_5codons gets from
 * p7_ForwardParser_Frameshift_5Codons, impl_sse/fwdback_fs.c).  sc[n]; -inf for a window shorter than 5 nt and for an overflow (the
 * reference's eslERANGE), never NaN.  Always odds ratios, whatever the context's switches say.  BATH_EINVAL for a 3-codon profile. */
int bath_hip_fs5_forward_parser_odds(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *dna, int cfg_len_amino, float *sc);

/* ------------------------------------------------------------------------------------------
 * Frameshift calibration (bathconvert.c:128-169): the FS3 / FS5 Forward taus by simulation, and MAXL.
 * ------------------------------------------------------------------------------------------ */
/* The sample stream of p7_fs_Tau_3codons / _5codons (evalues.c:633-643): N sequences; for each, L draws of esl_rnd_FChoose over the
 * 20 frequencies <f> (NULL: the Swiss-Prot background; used as they stand, a roll beyond their sum is drawn again), then L draws of
 * esl_rnd_Roll over the codons of each residue in p7_codontable_Create's order.  dna: N x 3L codes 0..3.  *rng_state: the "fast"
 * generator's state (bath_selftest_rng_jump(seed, 0, &state) right after seeding), in and out: the reference carries one generator,
 * seeded with 42, through all the models of a file.  BATH_EINVAL: unknown table, or a drawn residue without a codon in it.  Host only. */
int bath_calib_sample(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, uint8_t *dna);
/* esl_gumbel_FitComplete: maximum-likelihood Gumbel on complete data (Newton-Raphson on Lawless 4.1.6 from a method-of-moments start,
 * one step past easel's |f| < 1e-5; mu from 4.1.5).  BATH_ENORESULT: no convergence.  Host only, double. */
int    bath_gumbel_fit_complete(const double *x, int n, double *mu, double *lambda);
double bath_gumbel_invcdf(double p, double mu, double lambda);
/* tau = invcdf(1 - tailp; fit of xv) + log(tailp) / lambda_model (evalues.c:658) */
int    bath_calib_tau(const double *xv, int n, double lambda_model, double tailp, double *tau);
float  bath_bg_fs_nullone(int L_amino);                    /* p7_bg_SetLength(bg, L) + p7_bg_fs_NullOne (p7_bg.c:189, :377) */
int    bath_hmm_max_length(const bath_hmm *hmm, double emit_thresh);   /* p7_Builder_MaxLength (p7_builder.c:678); -1 without a model */
/* p7_fs_Tau_3codons then p7_fs_Tau_5codons of one model (bathconvert.c:147-161): the two frameshift profiles at length L, N sampled
 * sequences each (the 3-codon fit's first, from the same generator), bath_hip_fs3_forward_parser (strict) and
 * bath_hip_fs5_forward_parser, xv[i] = (sc - nullsc) / ln 2, the fits.  xv3 / xv5 (NULL or [N]): the bit scores.  Nothing is redrawn:
 * the reference's redraw is for its odds-ratio parser's overflow, which log space does not have (bath_hip_calibrate_fs_arith below runs
 * that arithmetic, with the redraw).  BATH_ERANGE: a sequence without a path (L below two codons). */
int bath_hip_calibrate_fs(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                          double *tau3, double *tau5, double *xv3, double *xv5);
/* The reference's redraw loop (evalues.c:633-649, :728-744, with their `i--; continue`) around a batch scoring callback: sequences
 * are drawn one after another from the carried generator (bath_calib_sample's stream), a sequence whose score is not finite is
 * discarded and the next one is drawn from where the generator stands after it, until N scores are kept:
 * xv[i] = (sc - nullsc) / ln 2 (float difference, double quotient).  score(user, dna, n, L3, sc): n sequences of L3 = 3L codes back to
 * back, sc[n] out, BATH_OK or an error that ends the fit.  Each call scores what is still missing.  *n_redrawn (or NULL): sequences
 * discarded; more than N of them in one fit returns BATH_ERANGE (the reference would loop for ever).  *rng_state ends where the
 * serial loop's generator ends and is left alone on error.  Host only. */
typedef int (*bath_calib_score_fn)(void *user, const uint8_t *dna, int n, int L3, float *sc);
int bath_calib_fit_scores(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, bath_calib_score_fn score, void *user,
                          float nullsc, double *xv, int *n_redrawn);
/* bath_hip_calibrate_fs in a chosen arithmetic.  BATH_ARITH_STRICT: that call's result, bit for bit.  BATH_ARITH_ODDS3: the 3-codon
 * scores from bath_hip_fs3_forward_parser in BATH_LOGSUM_ODDS.  BATH_ARITH_ODDS: also the 5-codon scores from
 * bath_hip_fs5_forward_parser_odds -- what the reference's bathconvert runs.  The odds modes go through bath_calib_fit_scores;
 * redrawn[2] (or NULL): sequences discarded in the 3-codon and the 5-codon fit.  The context's switches are neither read nor changed. */
#define BATH_ARITH_STRICT 0
#define BATH_ARITH_ODDS3  1
#define BATH_ARITH_ODDS   2
int bath_hip_calibrate_fs_arith(bath_hip_ctx *ctx, const bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, int L, int N, double tailp,
                                double *tau3, double *tau5, double *xv3, double *xv5, int arith, int *redrawn);
/* Several models per launch.  One model's 2 x N windows leave most of the device idle for the length of a window's row chain; a batch
 * gives every parser launch the windows of all its models.
 * bath_calib_sample_batch: the stream that n_models successive bath_hip_calibrate_fs calls draw, in their order -- model 0's 3-codon
 * set, model 0's 5-codon set, model 1's 3-codon set, ... each model with its own table; dna[n_models][2][N][3L].  *rng_state is left
 * alone on error (BATH_EINVAL: an unknown table, or a drawn residue without a codon in a model's table).  Host only.
 * bath_hip_calibrate_fs_batch: defined by what it equals -- n_models successive bath_hip_calibrate_fs calls with the state carried:
 * tau3[n_models], tau5[n_models], xv3 / xv5 (NULL or [n_models * N]) and the final state are the same bits.  Strict arithmetic only
 * (the odds modes' redraw makes a model's stream depend on the scores of the model before it).  1 <= n_models <= BATH_CALIB_BATCH_MAX.
 * All samples are drawn first, the 2 x n_models profiles built on host threads and uploaded, the models grouped by kernel tiling, one
 * launch per parser and per tiling present (fs3_fwd_batch_kernel, fs5_fwd_parser_batch_kernel: the spans bath_hip_kernel_times reports
 * afterwards), the 5-codon launches beside the 3-codon ones, one synchronize, then the fits.  All or nothing: on any error (its message
 * names the model's position in the batch, from 0) no output is written, *rng_state is unchanged and the context stays usable.
 * BATH_EINVAL: a model beyond the frameshift kernels' 1280 nodes, an unknown table, n_models out of range, L < 2, N < 2;
 * BATH_ERANGE: a sequence without a path, as in the single call. */
#define BATH_CALIB_BATCH_MAX 64
int bath_calib_sample_batch(uint32_t *rng_state, const float *f, const int *ncbi_tables, int n_models, int L, int N, uint8_t *dna);
int bath_hip_calibrate_fs_batch(bath_hip_ctx *ctx, const bath_hmm *const *hmms, const int *ncbi_tables, int n_models,
                                uint32_t *rng_state, int L, int N, double tailp,
                                double *tau3, double *tau5, double *xv3, double *xv5);
/* Fits from given generator states (bathfetch: the reference fits only what it fetches when the file has an index, every key from a
 * fresh generator, and carries one generator through the whole file when it has none, bathfetch.c:282-347).
 * bath_calib_skip: advances *rng_state exactly as n_sets successive bath_calib_sample calls with these arguments would, and stores
 * nothing: what a model that is passed over costs the carried generator (n_sets = 2: its 3-codon and its 5-codon set).  BATH_EINVAL
 * where bath_calib_sample returns it; *rng_state is left alone then.  Host only.
 * bath_hip_calibrate_fs_batch_at: defined by what it equals -- for every k, bath_hip_calibrate_fs of hmms[k] with ncbi_tables[k] from a
 * state equal to states_in[k]: tau3[k], tau5[k], xv3 / xv5 (NULL or [n_models * N]) and states_out[k], the state behind the model's
 * 5-codon set, are the same bits.  Models with one (states_in[k], ncbi_tables[k]) read one pair of sample sets, drawn once and held
 * once on the device; otherwise the launches are bath_hip_calibrate_fs_batch's.  Strict arithmetic only.  The same refusals, all or
 * nothing, messages by position in the batch. */
int bath_calib_skip(uint32_t *rng_state, const float *f, int ncbi_table, int L, int N, int n_sets);
int bath_hip_calibrate_fs_batch_at(bath_hip_ctx *ctx, const bath_hmm *const *hmms, const int *ncbi_tables, int n_models,
                                   const uint32_t *states_in, uint32_t *states_out, int L, int N, double tailp,
                                   double *tau3, double *tau5, double *xv3, double *xv5);

/* ------------------------------------------------------------------------------------------
 * Single-sequence models (bathbuild on an unaligned protein file; p7_SingleBuilder, p7_builder.c:501-569) and their calibration
 * (p7_Calibrate, evalues.c:64-199).  The model is host code; calibration runs the filters and parsers above on sampled sequences.
 * ------------------------------------------------------------------------------------------ */
/* The score system of p7_builder_LoadScoreSystem / _SetScoreSystem: a substitution matrix -- the built-in named <mx_name> (NULL:
 * BLOSUM62, the only one; bath_scorematrix_builtin gives its NCBI-format text or NULL) or, when <mxfile> is not NULL, an NCBI-format
 * file -- turned into conditional probabilities P(b | a) against the Swiss-Prot background widened to double
 * (esl_scorematrix_ProbifyGivenBG: lambda solves sum_ab f_a f_b exp(lambda s_ab) = 1; esl_scorematrix_JointToConditionalOnQuery),
 * with the gap-open and gap-extend probabilities.  On failure <errbuf> holds the reference's message: BATH_EFAIL an unknown
 * built-in or an unreadable file, BATH_EFORMAT a file that is not a matrix, BATH_EINVAL a matrix without a positive root for lambda. */
typedef struct bath_scoresystem bath_scoresystem;
const char *bath_scorematrix_builtin(const char *name);
int    bath_scoresystem_create(const char *mx_name, const char *mxfile, double popen, double pextend, bath_scoresystem **ret,
                               char *errbuf, int errlen);
void   bath_scoresystem_destroy(bath_scoresystem *s);
double bath_scoresystem_lambda(const bath_scoresystem *s);
int    bath_scoresystem_conditionals(const bath_scoresystem *s, double *Q /* [20][20], row = the query's residue */);
/* p7_Seqmodel + p7_hmm_SetComposition + p7_hmm_SetConsensus(hmm, sq) for the residues dsq[0 .. n) (codes 0..19 only: the caller has
 * stripped non-residues and refused degenerate codes): match emissions of node k are row dsq[k-1] narrowed to float, inserts the
 * background, transitions from popen / pextend with node M's special cases (seqmodel.c:59-82), the consensus the sequence itself.
 * evparam unset, max_length -1, fsprob 0.01, ct as given.  BATH_ERANGE: a name of more than 127 bytes (bath_hmm.name would cut it).  The model is in memory as the reference's is when it calibrates it. */
int    bath_hmm_from_sequence(const bath_scoresystem *s, const uint8_t *dsq, int n, const char *name, int ct, bath_hmm **ret);
double bath_hmm_mean_match_relent(const bath_hmm *hmm);   /* p7_MeanMatchRelativeEntropy (modelstats.c:80), bits per match state */
/* p7_MeanPositionRelativeEntropy (modelstats.c:163), bathstat's re/pos: match emissions weighted by match occupancy, plus the cost of
 * the transitions into each node; 0 without a model */
double bath_hmm_mean_position_relent(const bath_hmm *hmm);
double bath_hmm_lambda(const bath_hmm *hmm);           /* p7_Lambda (evalues.c:244): ln 2 + 1.44 / (M * relent); 0 without a model */
/* p7_hmmfile_WriteASCII(fp, p7_BATH_3f, hmm) (p7_hmmfile.c:565-689): the whole model's text, fields in the reference's order and
 * widths.  What bath_hmm does not hold comes as arguments: NSEQ (> 0), EFFN (>= 0), DESC, DATE and the command log, one line per
 * command (NULL or "": the line is left out).  The STATS block is written when the model is calibrated (evparam set); a calibrated
 * model whose two frameshift taus are unset (bath_hip_calibrate_std) is written as the reference writes hmm->fs == FALSE
 * (p7_hmmfile.c:620-623): the three standard STATS lines and CODON TABLE, without the FS3, FS5 and FRAMESHIFT PROB lines.  Returns the
 * text's size in bytes and copies at most <cap> of them to <buf>; < 0 on error. */
int64_t bath_hmm_write_ascii(const bath_hmm *hmm, int nseq, double eff_nseq, const char *desc, const char *date, const char *comlog,
                             char *buf, int64_t cap);
/* esl_rsq_xfIID as p7_MSVMu / p7_ViterbiMu / p7_Tau call it (evalues.c:317, :386, :556): N sequences of L residues, aa[N * L] codes
 * 0..19, from the generator state carried in *rng_state (bath_calib_sample's stream without the codons).  Host only. */
int bath_calib_sample_amino(uint32_t *rng_state, const float *f, int L, int N, uint8_t *aa);
int bath_gumbel_fit_complete_loc(const double *x, int n, double lambda, double *mu);   /* esl_gumbel_FitCompleteLoc; host only */
/* The three standard sample sets of a calibration, resident on the device: EmN x EmL, EvN x EvL and EfN x EfL residues drawn in
 * that order from *rng_state (advanced past them), with the device buffers a model's three fits need.  They depend on nothing a
 * kernel computes, and a builder that reseeds its generator for every model (--seed other than 0) draws the same three for every
 * model: make them once per run and hand them to every bath_hip_calibrate call.  Owned by the caller; destroy before the context. */
typedef struct bath_hip_calib_samples bath_hip_calib_samples;
int  bath_hip_calib_samples_create(bath_hip_ctx *ctx, uint32_t *rng_state, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN,
                                   bath_hip_calib_samples **ret);
void bath_hip_calib_samples_destroy(bath_hip_calib_samples *s);
/* p7_Calibrate: lambda (p7_Lambda), then the MSV mu (p7_MSVMu: the MSV filter, SSV first, on EmN sequences of length EmL; an
 * overflow scores maxsc, evalues.c:305; esl_gumbel_FitCompleteLoc at lambda), the Viterbi mu (p7_ViterbiMu, :374), the Forward tau
 * (p7_Tau: bath_calib_tau at tail mass Eft), each sequence scored at its own length, xv = (sc - null1) / ln 2; then the FS3 and FS5
 * taus as bath_hip_calibrate_fs_arith fits them in <arith>, at L = EfL, N = EfN, from the same generator.  The sets are drawn in that
 * order.  <samples> NULL: the three standard sets are drawn from *rng_state for this call (a generator carried from model to model,
 * --seed 0); else they are <samples> -- which must have been drawn from the state *rng_state holds, for this context, with these
 * lengths and counts (BATH_EINVAL otherwise) -- and the frameshift fits go on from where those draws ended.  The model's three
 * filters are queued before the first synchronize and their scores come back together.  On success hmm->evparam holds all eight
 * values and *rng_state the generator after the last draw; on failure both are as they were.  xv: NULL or EmN + EvN + 3 EfN bit
 * scores (MSV, Viterbi, Forward, FS3, FS5); redrawn: as bath_hip_calibrate_fs_arith's.  bath_hip_kernel_times afterwards: this
 * model's launches ("calib_msv", "calib_vit", "calib_fwd" and the frameshift parsers). */
int  bath_hip_calibrate(bath_hip_ctx *ctx, bath_hmm *hmm, int ncbi_table, uint32_t *rng_state, bath_hip_calib_samples *samples,
                        int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, int arith, double *xv, int *redrawn);
/* bath_hip_calibrate of several models per kernel launch, for a builder that reseeds its generator for every model: every model
 * starts from the state *rng_state holds, so all of them read the three sets of <samples> (required) and, with the one table of
 * the run, the same two frameshift sets drawn behind them -- five shared sample sets against n_models models.  Per standard filter
 * and per kernel tiling present one launch scores its set against the models of that tiling (a block reads its model at
 * blockIdx.y); the two frameshift parsers follow as bath_hip_calibrate_fs_batch launches them, every model on the one pair of
 * sets; one synchronize, then the fits.  Defined by what it equals: n_models calls of bath_hip_calibrate(ctx, hmms[k], ncbi_table,
 * &copy_of_state, samples, ..., BATH_ARITH_STRICT, xv_k, NULL), each from the same state -- the eight evparam floats of every
 * model bit for bit, xv (NULL, or [n_models][EmN + EvN + 3 EfN] bit scores) bit for bit, *rng_state what one such call leaves.
 * Strict arithmetic only (the odds modes' redraw makes a model's stream depend on its scores).  1 <= n_models <=
 * BATH_CALIB_BATCH_MAX.  BATH_EINVAL before anything is drawn, launched or written: n_models out of range, a missing model or
 * M < 1, a model beyond the frameshift kernels' 1280 nodes (the message names its position in the batch), an unknown table,
 * <samples> missing or not drawn from *rng_state for this context with these lengths and counts.  All or nothing: on any failure
 * no model's evparam, *rng_state and xv are touched, and the context stays usable.  bath_hip_kernel_times afterwards: the batch's
 * launches, "msv_wave_batch_kernel", "vit_wave_batch_kernel", "fwd_wave_batch_kernel", "fs3_fwd_batch_kernel" and
 * "fs5_fwd_parser_batch_kernel", one per tiling present. */
int  bath_hip_calibrate_batch(bath_hip_ctx *ctx, bath_hmm *const *hmms, int n_models, int ncbi_table, uint32_t *rng_state,
                              bath_hip_calib_samples *samples, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv);
/* The standard half of the two calls above: what p7_Calibrate does for a model without hmm->fs (evalues.c:124-155), as the
 * reference's search-time builder runs it when neither --fs nor --hmmout is given (p7_search_builder.c:182).  Lambda, the MSV mu, the
 * Viterbi mu and the Forward tau exactly as bath_hip_calibrate / bath_hip_calibrate_batch fit them -- evparam[0..5] bit for bit,
 * the same launches -- and nothing else: no frameshift sample is drawn, no frameshift parser launched, no translation table read,
 * and on success evparam[6] and evparam[7] hold the unset value (-99999).  *rng_state ends where the three standard draws end; with
 * <samples> that is the state behind them.  xv: NULL or, per model, EmN + EvN + EfN bit scores (MSV, Viterbi, Forward).  The other
 * rules are those of the full calls (<samples> as there, required by the batch call; all or nothing; the batch call names a failing
 * model's position), but the limit is the filter cascade's 2048 nodes, not the frameshift kernels' 1280.  bath_hip_kernel_times
 * afterwards: "calib_msv", "calib_vit", "calib_fwd"; for the batch call the three "*_wave_batch_kernel" names, one per tiling. */
int  bath_hip_calibrate_std(bath_hip_ctx *ctx, bath_hmm *hmm, uint32_t *rng_state, bath_hip_calib_samples *samples,
                            int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv);
int  bath_hip_calibrate_std_batch(bath_hip_ctx *ctx, bath_hmm *const *hmms, int n_models, uint32_t *rng_state,
                                  bath_hip_calib_samples *samples, int EmL, int EmN, int EvL, int EvN, int EfL, int EfN, double Eft, double *xv);

/* The multi-domain region stage on its own: the multihit Forward of every sequence of <regions> (each one region, configuration
 * length 100 as the pipeline's) and its trace ensemble in the context's bath_hip_set_fs_ensemble mode.  Per region r:
 *   region_status[r]  0 = ok, 1 = no valid traces (Forward underflow, an impossible state, the step cap): no envelopes;
 *   trace_status      [n][200] or NULL: 0 ok, 1 impossible state, 2 step cap, 3 segment overflow (modes 1, 2; zeros in mode 0);
 *   seg, seg_off      records (trace, i, j, k, m) in region coordinates, trace by trace in p7_trace_fs_Index's order; region r's
 *                     are seg_off[r] .. seg_off[r+1] (modes 1, 2; none in mode 0, whose walk keeps no segments);
 *   env, env_off      envelopes (i, j) in region coordinates, ordered by start, before the pipeline's length >= 15 rule.
 * At most max_seg / max_env records are written; the offsets count all of them (BATH_ERANGE when either did not fit). */
int bath_hip_fs5_region_ensembles(bath_hip_ctx *ctx, const bath_hip_fsprofile *om5, const bath_hip_seqs *regions, uint32_t seed,
                                  int32_t *region_status, int32_t *trace_status, int32_t *seg, int64_t max_seg, int64_t *seg_off,
                                  int32_t *env, int64_t max_env, int64_t *env_off);

/* The standard branch's multi-domain region stage on its own: the multihit Forward of every sequence of <regions> (amino acids, each
 * one region; model configured for length cfg_len[r], or the region's own length when cfg_len is NULL) and its trace ensemble in
 * the context's bath_hip_set_std_ensemble mode.  Outputs as bath_hip_fs5_region_ensembles's, in region coordinates, with segments in
 * p7_trace_Index's order, plus env_n2corr: per envelope the sum of the ensemble's per-residue null2 log odds over it (the domain's
 * null2 correction, p7_domaindef.c:1270-1272).  An empty region (Forward score -inf) has status 1 and nothing is walked. */
int bath_hip_std_region_ensembles(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_seqs *regions, const int32_t *cfg_len, uint32_t seed,
                                  int32_t *region_status, int32_t *trace_status, int32_t *seg, int64_t max_seg, int64_t *seg_off,
                                  int32_t *env, float *env_n2corr, int64_t max_env, int64_t *env_off);

/* ------------------------------------------------------------------------------------------
 * Self-test hooks (host only, no GPU): the pieces of easel the multi-domain branch restates -- esl_randomness_CreateFast /
 * esl_random (p7_pipeline.c:140: the "fast" generator, x <- 69069 x + 1 on a Jenkins-mixed seed) and esl_vec_FNorm +
 * esl_rnd_FChoose as p7_StochasticTrace calls them (stotrace.c:165-300) -- so that tests can hold them against independent
 * implementations of the published algorithms.
 * ------------------------------------------------------------------------------------------ */
int bath_selftest_rng_stream(uint32_t seed, int n, double *out);                          /* the first n values of esl_random() after seeding */
int bath_selftest_fchoose(uint32_t seed, const float *p, int n, int draws, int32_t *out); /* draws x (copy p, esl_vec_FNorm, esl_rnd_FChoose) from one stream */
/* region_trace_ensemble_frameshift (p7_domaindef.c:891-958: 200 stochastic tracebacks through a region's multihit 5-codon Forward
 * matrix, single-linkage clustering) as the pipeline runs it on the host, on caller-supplied matrices: fwd (Lr+1) x (M+1) x
 * {D, I, M, C1..C5}, fx (Lr+1) x {E,N,J,B,C}, tsc the generic [M][8] log transitions; env: n_env x {i, j} in window nucleotides. */
/* p7_spensemble_Cluster + the removal of dominated clusters on caller-supplied segments (idx: the sample a segment came from) */
int bath_selftest_cluster_segments(int n, const int32_t *idx, const int32_t *i, const int32_t *j, const int32_t *k, const int32_t *m,
                                   int nsamples, int fs, int32_t *env, int max_env, int32_t *n_env);
int bath_selftest_fs_ensemble(int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr, const float *fwd, const float *fx,
                              int32_t *env, int max_env, int32_t *n_env);
/* ... with the region's seed (bath_selftest_fs_ensemble uses 42) */
int bath_selftest_fs_ensemble_seeded(int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr, const float *fwd, const float *fx,
                                     uint32_t seed, int32_t *env, int max_env, int32_t *n_env);
/* The host twin of BATH_ENSEMBLE_STREAMS_DEVICE (= what BATH_ENSEMBLE_STREAMS_HOST runs) on caller-supplied matrices, no GPU needed.
 * region_status: 0 ok, 1 no valid traces; trace_status[200] or NULL; seg: up to max_seg records (trace, i, j, k, m) in region
 * coordinates, *n_seg all of them; env: up to max_env (i, j) pairs in window coordinates (shifted by ireg - 1), *n_env all of them.
 * BATH_ERANGE: the region is outside the stream rule, or a trace has more than 64 segments (the pipeline then runs the serial ensemble). */
int bath_selftest_fs_ensemble_streams(int M, const float *tsc, float xNL, float xNM, float xE, int ireg, int Lr, const float *fwd, const float *fx,
                                      uint32_t seed, int32_t *region_status, int32_t *trace_status, int32_t *seg, int max_seg, int32_t *n_seg,
                                      int32_t *env, int max_env, int32_t *n_env);
/* The standard branch's ensemble on caller-supplied tables and matrices, no GPU needed: tf [M+1][8], rf [>= 20][M+1] (odds ratios of
 * the optimized profile), pmove / tEL / tEM of its multihit configuration, res[Lr], fwd (Lr+1) x (M+1) x {M, D, I}, fx (Lr+1) x
 * {E, N, J, B, C, SCALE}.  mode 0 or 1 (BATH_ERANGE in mode 1: outside the stream rule or more than 64 segments in a trace).
 * n2sc[Lr] or NULL: per-residue null2 log odds; the other outputs as bath_selftest_fs_ensemble_streams's, region coordinates. */
int bath_selftest_std_ensemble(int mode, int M, const float *tf, const float *rf, float pmove, float tEL, float tEM, const uint8_t *res, int Lr,
                               const float *fwd, const float *fx, uint32_t seed, int32_t *region_status, int32_t *trace_status,
                               int32_t *seg, int max_seg, int32_t *n_seg, float *n2sc, int32_t *env, int max_env, int32_t *n_env);
/* one walk of the standard branch's stream modes from generator state <rng_state>: *status, seg[max_seg][4] = (i, j, k, m) first domain first */
int bath_selftest_std_ens_walk(int M, const float *tf, float pmove, float tEL, float tEM, int Lr, const float *fwd, const float *fx, uint32_t rng_state,
                               int32_t *status, int32_t *seg, int max_seg, int32_t *n_seg);
int bath_selftest_rng_jump(uint32_t seed, uint64_t n, uint32_t *state);   /* the generator's state n steps after seeding, by jump-ahead: value n - 1 of bath_selftest_rng_stream is state / 2^32 */
int bath_selftest_compo_terms(int base_b, float scale_b, float *terms /* [20][256] */);   /* the local-composition filter's term table bg_f[x] * expf((base_b - s) / scale_b), by the host build of the function the profile's kernel compiles */
/* (needs the GPU) the cascade's counting sort of a work list by length: targets 0..n-1 of lengths lens[], sorted[n] longest first (ties in any order), *n_longer: the number of targets longer than T */
int bath_selftest_len_sort(bath_hip_ctx *ctx, int n, const int32_t *lens, int T, int32_t *sorted, int32_t *n_longer);
int bath_selftest_compute_units(const bath_hip_ctx *ctx);   /* the device's compute units: the cascade sizes its decision kernels' grids by them (4 blocks of 256 threads each), and a test its blocks by that */
int bath_selftest_ens_explog(int n,const float *x, float *e, float *l);  /* the stream modes' own expf / logf (host build of the source the kernel compiles); either output may be NULL */
/* (need the GPU) The frameshift stage's DNA-window builder and branch decision on their own (bath_fs_windows.hip), from lists a test
 * makes up in place of what a cascade leaves.  A lane = one cascade lane's F4 survivors and their hit windows, ids the lane's own. */
typedef struct { int64_t window, aa_off; double P; int32_t cand, sf, startj, len; float fwdsc, nullsc; int64_t fxoff; } bath_fs_cand;   /* sf = strand * 3 + frame; startj: first codon of the frame's stream */
typedef struct { int32_t cand, n, k, length; float score; } bath_fs_hitwin;                                                            /* P7_HMM_WINDOW of candidate <cand> */
typedef struct { const bath_fs_cand *cands; const bath_fs_hitwin *wins; int32_t n_c, n_w, cand_base; int64_t first_window, dpool; } bath_fs_lane;
typedef struct {                   /* an F4 survivor in the builder's order, with the DNA window it asks for */
  int64_t w, aa_off; double P;
  int32_t cand, strand, start, end, n; float fwd_null;
  int32_t wb, we;                  /* we > wb: a hit window of the ORF was found */
  int32_t dw_n, dw_len, dw_k, kmin, kmax, g0, g1, pad_;
} bath_fs_orf;
typedef struct { int64_t src_off, dst_off; int32_t seq_n, start, len, strand, kmin, kmax; } bath_fs_windesc;   /* a window's gather descriptor */
typedef struct { int32_t n_orfs, nw, maxlen, pad_; int64_t pool_bytes, total; } bath_fs_winbuild;
/* driver 0: the lists uploaded as given, then the kernels; driver 1: the lists ordered and merged as the pipeline's host path does, then
 * the host build.  F3, std_pipe: of the search.  Only the lengths and offsets of <dna> are read.  Returns the build's status
 * (BATH_ENORESULT: the kernels hand the block back; nothing is written then) and, the stream synchronized, the whole product: hdr, the
 * ordered ORFs [sum n_c], and per window (at most sum n_c) the record, its group grp[2 i], grp[2 i + 1] (a range of orfs), pool offset,
 * length and descriptor (read back from the device copy). */
int bath_selftest_fs_windows(bath_hip_ctx *ctx, const bath_hip_oprofile *om, const bath_hip_fsprofile *om_fs3, const bath_hip_seqs *dna, double F3, int std_pipe,
                             int driver, const bath_fs_lane *lanes, int nlanes, int nc_total, bath_fs_winbuild *hdr, bath_fs_orf *orfs,
                             bath_fs_window *windows, int32_t *grp, int64_t *voff, int32_t *vlen, bath_fs_windesc *desc);
/* the branch decision over records[nw] (in: as a build leaves them; out: completed) from bias[nw][2][3], the three frames' Forward scores of
 * the bias filter HMM under the model's and the local composition, and fsc[nw], the windows' Forward scores.  driver 0: fsw_decide_kernel;
 * driver 1: the host loop a host-built block takes. */
int bath_selftest_fs_decide(bath_hip_ctx *ctx, const bath_hip_fsprofile *om_fs3, bath_fs_window *records, int nw, const float *bias, const float *fsc,
                            int do_biasfilter, int std_pipe, double F3, int driver);

#ifdef __cplusplus
}
#endif
#endif /* BATH_HIP_H */
