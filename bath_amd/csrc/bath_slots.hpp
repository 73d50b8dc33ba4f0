// bath_slots.hpp -- the names of a context's long-lived buffers: device scratch (bath_hip_ctx::scratch) and page-locked staging
// (bath_hip_ctx::stage).  One enumerator per role, grouped by stage in pipeline order; the two enums are the record of who owns what.
//
// Sharing.  `kB = kA` directly behind kA: the two roles live in ONE allocation, and the comment says what keeps them apart.  What all
// of them rest on: one host thread drives a context at a time, and every entry point and every stage named below ends with a
// synchronize of the context's stream (side stream joined first) before it returns -- so roles of different calls never overlap on
// one context.  Work that runs beside other work has a context of its own (the cascade's lanes, ctx->aux / aux2 / aux3), with its
// own arrays.  A role with no alias has its allocation to itself.  A new stage takes a new enumerator; an alias needs that comment.
#pragma once
#include <type_traits>

namespace bath {

enum class Scratch : int {
  // ---- translation pass (bath_orfs.hip; bath_pipeline.hip carves the same four for the cascade)
  kOrfCodonTables,          // the NCBI table's codon tables, kept while ctx->orf_tables_id names it
  kOrfAminoPool,            // the amino-acid streams of every ORF: the pool every later stage of the call reads (ctx->fs_std_pool)
  kOrfSlots,                // per-tile ORF slots
  kOrfRecords,              // the length-sorted work list
  kOrfMisc,                 // counts, cross-tile pieces, histogram, cursors
  // ---- filter cascade (bath_pipeline.hip: run_filters)
  kSsvScoreTable,           // the profile's SSV score table + background frequencies, kept while ctx->tabs_uid names the profile
  kCascadeWork,             // candidate arrays, to-do lists, hit windows, counters (PipelineWork); read by the records and survivor stages
  kFilterBathWork = kCascadeWork,   // bath_hip_vitfilter_bath / bath_hip_ssvfilter_bath: calls of their own, a cascade pass lays the buffer out afresh
  kLocalCompoSums,          // 20 sums per candidate for the local-composition re-filter
  kCascadeFwdRows,          // the Forward parser's special-state rows of the F3 survivors (ctx->fwd_rows_kept), until the next cascade call
  kCascadeFwdRowOffsets,    // ... where, by candidate (ctx->fwd_rows_off)
  // ---- ORF records and survivor lists (bath_records.hip; bath_pipeline.hip: select_survivors)
  kRecordKeys,              // sort keys and indices, both halves of the radix sort
  kRecordSortTemp,          // rocprim's temporary storage
  kRecords,                 // the records (ctx->d_records), until the next cascade call
  kSurvivorSelect,          // a lane's F4 survivors and their hit windows
  // ---- frameshift pipeline: DNA windows, bias filter, branch decision (bath_fs_windows.hip, bath_fs_stage.hip)
  kFsWindowPadding,         // the profile's window padding fractions, kept while ctx->fsw_pad_uid names the profile
  kFsWindowWork,            // the device-side window builder's workspace
  kFsWindowResult,          // what a build leaves: header, view arrays, ordered ORFs, groups, window records, descriptors (ResLayout)
  kFsWindowPool,            // the windows' nucleotides (fs_gather_view_built)
  kFsWindowBias,            // the bias filter's six terms per window (side stream; joined before fs_decide reads them)
  kFsWindowLenTerms,        // the decision's length terms, as uploaded from ctx->fsw_len_terms
  // ---- 3-codon frameshift parsers and regions (bath_frameshift.hip, bath_fs_chain.hip)
  kFsJobList,               // windows by decreasing length + job counters (fs_schedule), for every frameshift launch of a call
  kChainBatchesFwd,         // chain_batches for the Forward chain kernel
  kChainBatchesBwd,         // ... for the Backward one, which may run on the side stream beside Forward: its own buffer
  kChainFwdHistory,         // fs3_fwd_chain_mem_kernel's row history
  kFs3FwdScores,            // Forward scores of the windows (Backward's behind them); fs_decide reads them on the device
  kFs3FwdRows,              // Forward special-state rows
  kFs5TraceOut = kFs3FwdRows,       // fs5_envelopes_ex's trace records: a later call; the parsers and fs3_regions synchronize before they return
  kStdTraceOffsets = kFs3FwdRows,   // std_domains' trace column offsets: the standard branch runs after that synchronize, or on ctx->aux
  kFs3RowOffsets,           // the rows' offsets
  kFs5TraceSteps = kFs3RowOffsets,  // fs5_envelopes_ex's dense trace columns: a later call, as kFs5TraceOut
  kFs3BwdRows,              // Backward special-state rows (fs3_regions)
  kFs5OaRows = kFs3BwdRows,         // fs5_envelopes_ex's optimal-accuracy special-state rows: a later call, as kFs5TraceOut
  kFs3RegionWork,           // fs_regions_kernel's three floats per row
  kEnvTraceColumns = kFs3RegionWork,   // the envelopes' trace columns, either branch: fs3_regions has synchronized; the branches share a context only one after the other
  kFs3RegionList,           // the regions of every window (fs3_regions copies them to the host and synchronizes)
  kEnvFwdMatrix = kFs3RegionList,   // Forward matrices of an envelope / region batch, either branch: behind fs3_regions' synchronize
  kFsKeptFwdRows,           // the decision stage's Forward rows of every window (fs3_forward_scores), for fs3_regions of the domain stage; ctx->fs_keep_xoff
  kFsKeptFwdRowOffsets,     // ... the offsets of the windows fs3_regions was given
  // ---- frameshift domain stage: regions, ensembles (bath_domaindef.hip, bath_fs_ensemble.hip)
  kFsGatherPool,            // nucleotides of the regions / envelopes of a batch (fs_gather_view)
  kFsGatherDesc,            // ... their descriptors and view arrays
  kFsRegionFwdMatrix,       // device ensemble: the regions' Forward matrices stay here while envelope batches use kEnvFwdMatrix
  kFsRegionFwdRows,         // ... and their special-state rows
  kFsEnsembleStates,        // fs_ensemble_kernel's start states
  kFsEnsembleOut,           // ... its statuses and segments
  // ---- envelopes: full Forward / Backward, decoding, optimal accuracy, traces (bath_fs_envelopes.hip: fs5_envelopes_ex; bath_std_domains.hip: std_domains)
  kEnvBwdMatrix,            // Backward matrices (posteriors after decoding)
  kFs5OaMatrix,             // optimal-accuracy matrices of the 5-codon model
  kEnvFwdRows,              // Forward special-state rows beside kEnvFwdMatrix (fs5_envelopes_ex, fs5_region_forward, bath_hip_forward_full)
  kStdPosteriorRows = kEnvFwdRows,  // standard branch: posterior rows (its Forward rows are kStdFwdRows); batches of the two branches are calls of their own
  kEnvBwdRows,              // Backward special-state rows of the 5-codon envelopes
  kStdOaRows = kEnvBwdRows,         // standard branch: optimal-accuracy rows; as kStdPosteriorRows
  kEnvOffsets,              // the batch's matrix and row offsets
  kEnvScores,               // Forward / Backward / OA scores of the batch (and statuses: bath_hip_forward_full)
  kStdEnvOut = kEnvScores,          // standard branch: StdEnvOut records (its scores are kStdScores); as kStdPosteriorRows
  kEnvNull2Work,            // per-envelope sums behind null2
  kEnvNull2,                // null2 scores
  kFs5RowDenominators,      // the rows' normalising factors when the posterior matrix is not stored
  kFs5FwdRing,              // wavefront Forward's ring (bath_fs_wavefront.hip)
  kFs5BwdRing,              // wavefront Backward's ring; Backward runs on the side stream beside Forward
  kFs5BwdTerms,             // ... its terms
  kFs5BwdTermOffsets,       // ... and their offsets
  // ---- standard branch's domain stage and the stand-alone filter entry points (bath_std_domains.hip, bath_filters.hip): the entry
  // points are the same stages run alone, so they name the same buffers
  kFilterOrder,             // targets by length (bath_hip_ssvfilter / msvfilter / vitfilter)
  kStdViewArrays = kFilterOrder,    // std_domains: a batch's offsets, row offsets and lengths; the filter entry points are calls of their own
  kFilterSsvRaw,            // SSV's 16-bit results before classification
  kStdScores,               // scores of the batch in flight (Forward's, Backward's behind them)
  kStdStatus,               // ... and statuses
  kMsvTodo,                 // bath_hip_msvfilter: the targets SSV left undecided
  kFwdbackRowOffsets = kMsvTodo,    // bath_hip_fwdback_parser: row offsets; a call of its own
  kStdRegionWork = kMsvTodo,        // std_domains: std_regions_kernel's three floats per row; a call of its own
  kFwdGroupWork,            // bath_hip_fwdparser_group: the work list, its copy sorted by length, the sort's bins, the list's length
  kBiasFilterScores,        // bath_hip_bias_filter: the filter scores
  kStdRegionList = kBiasFilterScores,     // std_domains: the ORFs' regions; a call of its own
  kStdRegionCfgLen = kBiasFilterScores,   // the multi-domain regions' configuration lengths: std_domains has copied the region list out and synchronized ("parsers + regions")
  kStdFwdRows,              // Forward special-state rows of the batch in flight (ORFs, then regions, then envelopes: a synchronize between)
  kStdBwdRows,              // Backward special-state rows
  kStdKeptRowSource,        // where the survivors' rows lie in kCascadeFwdRows (copy_rows_kernel)
  kStdRegionFwdMatrix,      // device ensemble: the multi-domain regions' Forward matrices
  kStdEnsembleUpload,       // std_ensemble_kernel: job list, path offsets, start states
  kStdEnsembleOut,          // ... statuses, segments, path codes
  // ---- frameshift calibration of several models per launch (bath_calibrate.hip: bath_hip_calibrate_fs_batch)
  kCalibBatchWork,          // a job counter per (model, parser), the job order, the models' descriptors (FsBatchModel), the windows' scores
  // ---- the standard filters of several models per launch (bath_calibrate.hip: bath_hip_calibrate_batch; bath_calib_batch.hip)
  kCalibStdBatchWork,       // the models' descriptors (StdBatchModel), every model's scores and statuses; beside kCalibBatchWork in one call
  kCount
};

// Page-locked staging for small tables a launch uploads and small results it brings back: an asynchronous copy from or to here needs
// no synchronize before the local it was built in goes away.  One role per call site; a site is refilled by its context only after
// the stage that used it has synchronized its stream.  The multi-domain regions' matrices, which host threads walk, live here too.
enum class Pinned : int {
  kFsJobOrder,              // fs_schedule's job order, up
  kChainBatchesFwd,         // chain_batches for Forward, up
  kChainBatchesBwd,         // ... for Backward (side stream), up
  kFs5BwdTermOffsets,       // wavefront Backward's term offsets, up
  kStdUploads,              // std_domains: every small upload of a stage, back to back
  kStdDownloads,            // ... and its downloads
  kStdRegionMatrices,       // std_region_stage: the multi-domain regions' Forward matrices, written by the kernel, read by the ensemble threads
  kStdRegionRows,           // ... their special-state rows, then their residues
  kFsWindowResult,          // regions A and B of Scratch::kFsWindowResult, down (device build); the whole product (host build)
  kFsDecideDown,            // fs_decide: the completed window records (device build) or the bias terms (host build), down
  kFsRegionMatrices,        // fs5_region_forward: the regions' Forward matrices, written by the kernel (coherent) or copied down, read by the ensemble threads
  kFsRegionRows,            // ... their special-state rows, then the done flags and the scores
  kFsEnsembleStates,        // fs_ensemble_kernel's start states, up
  kFsEnsembleOut,           // ... its statuses, segments and the regions' scores, down
  kStdEnsembleUpload,       // std_ensemble_kernel's upload
  kStdEnsembleOut,          // ... and its results, down
  kCalibBatchUpload,        // bath_hip_calibrate_fs_batch, bath_hip_calibrate_batch: zeroed counters, job order and descriptors, up
  kCalibStdBatchUpload,     // bath_hip_calibrate_batch: the standard filters' descriptors, up (in flight beside kCalibBatchUpload)
  kCount
};

// An array indexed by one of the enums above and by nothing else.
template <class E, class B>
struct SlotArray {
  B b[(int)E::kCount];
  B &operator[](E e) { return b[(int)e]; }
  B *begin() { return b; }
  B *end() { return b + (int)E::kCount; }
};
static_assert(!std::is_invocable_v<decltype(&SlotArray<Scratch, int>::operator[]), SlotArray<Scratch, int> &, int> &&
              !std::is_invocable_v<decltype(&SlotArray<Scratch, int>::operator[]), SlotArray<Scratch, int> &, Pinned>,
              "a slot is named by its own enum: no integer, no enumerator of the other array");

}  // namespace bath
