// xflow-amd: host launchers of the gfx950 kernels (implemented in *.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "xflow/backend.h"

namespace xflow {
namespace hip {

// kernels_dedup.hip
void launch_dedup(const u64* keys, int64_t nnz, ScratchView s, DedupOut o, hipStream_t st);
void launch_remap_pos(u32* pos, int64_t nnz, const u32* inv, u32 none, hipStream_t st);
void launch_partition_counts(const ScratchView& s, const u32* chunk_offsets,
                             const int64_t* n_uniq, int64_t* counts, int64_t seq, hipStream_t st);

// kernels_pull.hip
void launch_table_pull(const PullArgs& a, hipStream_t st);

// kernels_apply.hip
void launch_table_apply(const ApplyArgs& a, hipStream_t st);
void launch_owner_group(const OwnerGroupArgs& a, hipStream_t st);

// kernels_exchange.hip
void launch_gather_grads(const GatherGradArgs& a, hipStream_t st);
void launch_scatter_rows(const float* src, float* dst, const u32* map, const int64_t* n_dev,
                         int64_t n_max, int width, float* zero_out, int zero_width,
                         hipStream_t st);
// CSR exchange: exclusive scan (out[n] = total; tiles: n_max / 4096 + 2 words)
void launch_scan_u32(const u32* in, u32* out, const int64_t* n_dev, int64_t n_max, u32* tiles,
                     hipStream_t st);
void launch_csr_pack(const u32* off, const u32* cnt, const void* src, const u32* doff,
                     const int64_t* n_dev, int64_t n_max, void* dst, int entry_bytes,
                     hipStream_t st);
void launch_csr_totals(const int64_t* counts, int world, bool encoded, const u32* doff,
                       int64_t* totals, hipStream_t st);

// kernels_table.hip
void launch_fill_u64(u64* p, u64 v, size_t n, hipStream_t st);
void launch_upload_small(void* dst, const void* src, size_t bytes, hipStream_t st);
void launch_download_small(void* host_dst, const void* src, size_t bytes, hipStream_t st);
void launch_snapshot(HostSnap* dst, const u32* mon, unsigned long long seq, hipStream_t st);
void launch_table_clear(const TableView& t, hipStream_t st);
void launch_table_export(const TableView& t, u64* keys_out, u32* words_out, int64_t max_rows,
                         unsigned long long* counter, hipStream_t st);
void launch_table_import(const TableView& t, const u64* keys, const u32* words, int64_t n,
                         hipStream_t st);
void launch_table_prefill(const TableView& t, int64_t n, u64 seed, hipStream_t st);
// growth: split segments [s0, s0 + k) (marks: (k << seg_log2) / 64 words of scratch)
void launch_table_split(const TableView& t, u64 s0, u64 k, u64* marks, hipStream_t st);
// pruning: drop the slot_prunable keys of segments [s0, s0 + k), adding their
// number to *count (marks as for the split); then *size -= *count,
// *total += *count
void launch_table_prune(const TableView& t, const OptSpec& o, float max_n, u64 s0, u64 k,
                        u64* marks, unsigned long long* count, hipStream_t st);
void launch_table_prune_finish(unsigned long long* size, unsigned long long* total,
                               const unsigned long long* count, hipStream_t st);
void launch_table_nonzero(const TableView& t, const OptSpec& o, unsigned long long* counter,
                          hipStream_t st);
// delta checkpoints: the touched-key filter of 2^L bits (delta_bit, common.h)
void launch_delta_mark(u32* bits, int L, const u64* keys, const int64_t* n_dev, int64_t n_host,
                       int64_t n_max, hipStream_t st);
void launch_table_export_marked(const TableView& t, const u32* bits, int L, u64* keys_out,
                                u32* words_out, int64_t max_rows, unsigned long long* counter,
                                hipStream_t st);
void launch_delta_popcount(const u32* bits, int L, unsigned long long* counter, hipStream_t st);
// serving snapshots: the slot_exported keys and their P resolved weights
void launch_table_export_weights(const TableView& t, const OptSpec& o, u64* keys_out,
                                 float* weights_out, int64_t max_rows,
                                 unsigned long long* counter, hipStream_t st);
// serving deltas: the marked keys (the filter bit alone) and their P resolved weights
void launch_table_export_weights_marked(const TableView& t, const OptSpec& o, const u32* bits,
                                        int L, u64* keys_out, float* weights_out,
                                        int64_t max_rows, unsigned long long* counter,
                                        hipStream_t st);

// kernels_refresh.hip: a serving delta into a frozen table.  Upsert n unique
// (key, P weights) entries, flagging dirty[segment] = 1 where the weights
// written read as an absent key's; then, over segments [s0, s0 + k), drop the
// slots of flagged segments that read as absent (marks as for the split),
// adding their number to *dropped and the flagged segments to *swept
void launch_frozen_upsert(const TableView& t, const OptSpec& o, const u64* keys,
                          const float* weights, int64_t n, u32* dirty, hipStream_t st);
void launch_frozen_sweep(const TableView& t, const OptSpec& o, u64 s0, u64 k, const u32* dirty,
                         u64* marks, unsigned long long* dropped, unsigned long long* swept,
                         hipStream_t st);

// kernels_serve.hip
void launch_serve_lr(const ServeLrArgs& a, hipStream_t st);
void launch_serve_model(const ServeArgs& a, hipStream_t st);  // FM, MVM

// kernels_layout.hip
void launch_unpack_block(const UnpackArgs& a, hipStream_t st);
void launch_field_major(const void* src, void* dst, int64_t rows, int F, int elem_bytes, bool widen,
                        hipStream_t st);

// kernels_shuffle.hip (ShuffleArgs): fixed width in one pass; CSR as lengths +
// labels, launch_scan_u32 of a.len into a.row_ptr, then the entries
void launch_shuffle_fixed(const ShuffleArgs& a, hipStream_t st);
void launch_shuffle_len(const ShuffleArgs& a, hipStream_t st);
void launch_shuffle_gather(const ShuffleArgs& a, hipStream_t st);

// kernels_cross.hip (CrossArgs, one launch each): a row-major fixed-width
// source, a field-major one, a CSR one
void launch_cross_fixed(const CrossArgs& a, hipStream_t st);
void launch_cross_cols(const CrossArgs& a, hipStream_t st);
void launch_cross_csr(const CrossArgs& a, hipStream_t st);

// kernels_model.hip (the kernels: kernels_lr / _fm / _mvm / _reduce / _reduce_vec .hip)
void launch_forward_backward(const FwdArgs& a, hipStream_t st);
void launch_slice_masks(const BatchView& b, const u32* pos, u32* tmask, hipStream_t st);

// kernels_parse.hip
void launch_parse_text(const TextParseArgs& a, hipStream_t st);

// kernels_eval.hip
void launch_eval_metrics(const float* pctr, const float* labels, int64_t n, EvalMetrics* out,
                         hipStream_t st);
// per-group AUC counts and calibration (GroupedEval); table: optional per-group sums
void launch_eval_grouped(const float* pctr, const float* labels, const u64* groups, int64_t n,
                         GroupedEval* out, GroupTable* table, hipStream_t st);
void launch_row_group_keys(const BatchView& b, int field, u64* out, hipStream_t st);

// kernels_synth.hip
void launch_synth(const SynthArgs& a, hipStream_t st);

}  // namespace hip
}  // namespace xflow
