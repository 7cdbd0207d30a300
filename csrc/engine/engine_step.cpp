// xflow-amd: the step planner, the single-rank training step and evaluation.
#include <algorithm>
#include <cmath>

#include "xflow/engine.h"

namespace xflow {

void Engine::set_reduction(FwdArgs& fa) const {
  fa.trash_pos = (u32)scratch_.cap;
  if (!red_pairs_) return;
  if (rec_on_) fa.red_records = rec_count_;
  if (red_vmax_) {  // (MVM: two alternating words, see FwdArgs::red_vmax)
    fa.red_vmax = red_vmax_ + vmax_parity_;
    fa.red_vmax_next = red_vmax_ + (vmax_parity_ ^ 1);
    fa.red_dup = red_vmax_ + 2 + vmax_parity_;
    fa.red_dup_next = red_vmax_ + 2 + (vmax_parity_ ^ 1);
    if (mdup_rec_) {
      fa.mdup.rec = mdup_rec_;
      fa.mdup.vmax = red_vmax_ + 4;
      fa.mdup.n = red_vmax_ + 6;
      fa.mdup.acc = mdup_acc_;
      fa.mdup.claim = mdup_claim_;
      fa.mdup.cap = (int64_t)mdup_claim_.capacity();
      fa.mdup.ew = mdup_ew_;
    }
    vmax_parity_ ^= 1;
  }
  fa.red_bcap = ws_->bcap;
  fa.red_cap = scratch_.cap;
  fa.red_nsub = red_nsub_;
  fa.red_pairs = red_pairs_;
  fa.red_sorted = red_sorted_;
  fa.red_sorted_words = (int64_t)red_sorted_.capacity();
  fa.red_hist = red_hist_;
  fa.red_tot = red_tot_;
  fa.red_count = red_count_;
  fa.red_groups = red_groups_;
  fa.red_nb = red_nb_;
  fa.red_maxb = red_maxb_;
  fa.red_rowv = red_rowv_;
}

PullArgs Engine::pull_args(const u64* keys, const int64_t* n_dev, int64_t n, bool insert,
                           u32* out_slot) const {
  PullArgs pa;
  pa.table = table_;
  pa.opt = cfg_.opt;
  pa.keys = keys;
  pa.n_dev = n_dev;
  pa.n_host = n_dev ? 0 : n;
  pa.n_max = n;
  pa.insert = insert;
  pa.out_slot = out_slot;
  return pa;
}

ApplyArgs Engine::apply_args(const u64* keys, const u32* slots, const int64_t* n_dev, int64_t n,
                             int S) const {
  ApplyArgs aa;
  aa.table = table_;
  aa.opt = cfg_.opt;
  aa.keys = keys;
  aa.slots = slots;
  aa.n_dev = n_dev;
  aa.n_host = n_dev ? 0 : n;
  aa.n_max = n;
  aa.S = S;
  aa.pstride = pstride();
  aa.P = cfg_.model.P();
  aa.fm_D = cfg_.model.v_dim;
  return aa;
}

FwdArgs Engine::train_fwd_args(const BatchView& b, const u32* pos, int S) const {
  FwdArgs fa;
  fa.batch = b;
  fa.pos = pos;
  fa.wpull = wpull_;
  fa.grad = grad_;
  fa.stats = stats_;
  fa.model = cfg_.model;
  fa.S = S;
  fa.fx_bad = overflow_;
  fa.fm_vals = fm_vals_;
  set_reduction(fa);
  return fa;
}

FwdArgs Engine::eval_fwd_args(const BatchView& b, float* pctr) const {
  FwdArgs fa;
  fa.batch = b;
  fa.pos = ws_->pos;
  fa.wpull = wpull_;
  fa.pctr = pctr;
  fa.stats = stats_ + 1;
  fa.model = cfg_.model;
  fa.fm_vals = fm_vals_;
  return fa;
}

int Engine::slices_of(const BatchView& b) const {
  if (b.slice_rows <= 0 || b.rows <= 0) return 1;
  return (int)((b.rows + b.slice_rows - 1) / b.slice_rows);
}

const int32_t* Engine::slice_rows_dev(const BatchView& b, int S) {
  if (b.rows == cached_rows_ && b.slice_rows == cached_slice_rows_ && S == cached_S_)
    return slice_rows_;
  const int ng = slice_groups(S);
  // (a growth waits for the stream: the old normalisers may still be read)
  slice_rows_.reserve(*be_, (size_t)ng * kSliceGroup, (size_t)ng * kSliceGroup);
  const int64_t sr = b.slice_rows > 0 ? b.slice_rows : b.rows;
  for (int g = 0; g < ng; ++g) {
    int32_t h[kSliceGroup];
    const int n = ng == 1 ? S : kSliceGroup;
    for (int l = 0; l < n; ++l) {
      const int64_t s = (int64_t)g * kSliceGroup + l;
      int64_t rem = s < S ? b.rows - s * sr : 0;
      rem = rem < 0 ? 0 : rem;
      // an empty slice has no gradient rows; 1 keeps 0/rows finite
      h[l] = (int32_t)(rem < sr ? (rem > 0 ? rem : 1) : sr);
    }
    // (no host wait)
    be_->upload_small(slice_rows_ + (int64_t)g * kSliceGroup, h, sizeof(int32_t) * n);
  }
  cached_S_ = S;
  cached_rows_ = b.rows;
  cached_slice_rows_ = b.slice_rows;
  return slice_rows_;
}

BatchView Engine::group_view(const BatchView& b, int S, int k, const u32*& pos) const {
  if (slice_groups(S) == 1) return b;
  const int64_t sr = b.slice_rows > 0 ? b.slice_rows : b.rows;
  int64_t r0 = (int64_t)k * kSliceGroup * sr;
  r0 = r0 < b.rows ? r0 : b.rows;
  int64_t n = (int64_t)kSliceGroup * sr;
  n = n < b.rows - r0 ? n : b.rows - r0;
  BatchView g = b;
  g.rows = n;
  if (b.row_ptr) {  // CSR: occurrence indices stay absolute
    g.row_ptr = b.row_ptr + r0;
    g.labels = b.labels + r0;
    return g;  // (g.nnz: the whole batch's, an upper bound; no kernel reads it)
  }
  // fixed width: row-major (r, j) at r*npr + j, field-major at j*col_stride + r
  const int64_t off = b.col_stride > 0 ? r0 : r0 * b.nnz_per_row;
  g.keys = b.keys + off;
  if (b.fgid) g.fgid = b.fgid + off;
  g.labels = b.labels + r0;
  g.nnz = n * b.nnz_per_row;
  pos += off;
  return g;
}

void Engine::ensure_inv() {
  if (ws_->inv) return;
  // + the trash slot's entry (and padding to a 16-slot compaction group): no
  // unique index, so reductions skip it
  ws_->inv.alloc(*be_, scratch_.cap + 16);
  be_->memset(ws_->inv + scratch_.cap, 0xFF, 16 * sizeof(u32));
}

void Engine::dedup_(const BatchView& b, int parts, u64* uniq_keys_out, bool want_inv,
                    int64_t* n_copy, bool lead) {
  if (b.nnz > cfg_.max_nnz) throw std::invalid_argument("batch nnz exceeds max_nnz");
  if (b.rows > cfg_.max_rows) throw std::invalid_argument("batch rows exceed max_rows");
  if (b.col_stride > 0 && (b.row_ptr || b.col_stride < b.rows || b.nnz != b.rows * b.nnz_per_row))
    throw std::invalid_argument("field-major batch needs fixed nnz_per_row and col_stride >= rows");
  if (b.nnz == 0) {
    // rows without occurrences: no keys.  The backends' dedup writes the
    // unique count only when it runs over occurrences, so it is cleared here
    // (a count left from the batch before would pull, insert and flag that
    // batch's keys again)
    be_->memset(ws_->n_uniq, 0, sizeof(int64_t));
    return;
  }
  // table-ordered unique lists (ScratchView::home_bits) on the one-owner GPU path
  const int hb = be_->is_gpu() && parts == 1
                     ? table_.seg_log2 + table_.level + (table_.split > 0 ? 1 : 0)
                     : 0;
  if (parts != scratch_.parts || hb != scratch_.home_bits) {
    // slots depend on the partitioning / home bits: start from an empty scratch table
    be_->fill_u64(scratch_.keys, kEmptyKey, scratch_.cap);
    be_->memset(scratch_.claims, 0, sizeof(unsigned long long));
    scratch_.parts = parts;
    scratch_.home_bits = hb;
  }
  // (n_uniq is written, not accumulated, by both backends' dedup)
  if (++scratch_.epoch > kStampEpochs) {
    // byte stamps wrap: clear them (0 marks never-stamped slots) and the
    // spill mark, which holds an epoch of the previous cycle
    scratch_.epoch = 1;
    be_->memset(scratch_.stamps, 0, scratch_.cap);
    if (scratch_.ctl) {
      const unsigned long long z = 0ull;
      be_->upload_small(scratch_.ctl + 4, &z, sizeof(z));
    }
  }
  scratch_.grow = 0.0f;
  if (scratch_.ctl && nnz_seen_ > 0 && b.nnz > nnz_seen_)
    scratch_.grow = (float)((double)b.nnz / (double)nnz_seen_);
  if (b.nnz > nnz_seen_) nnz_seen_ = b.nnz;
  DedupOut o;
  o.pos = ws_->pos;
  o.uniq_keys = uniq_keys_out ? uniq_keys_out : uniq_keys_;
  o.uniq_pos = ws_->uniq_pos;
  o.n_uniq = ws_->n_uniq;
  o.overflow = overflow_;
  o.block_counts = block_counts_;
  o.inv = want_inv ? ws_->inv.get() : nullptr;
  o.n_uniq_copy = n_copy;
  o.cap_out = ws_->bcap;
  o.lead = lead;
  be_->dedup(b.keys, b.nnz, scratch_, o);
}

const char* grad_path_name(GradPath g) {
  switch (g) {
    case GradPath::kCsr: return "csr";
    case GradPath::kUniqueLR: return "unique_lr";
    case GradPath::kUniqueFmBC: return "unique_fm_bc";
    case GradPath::kUniqueRows: return "unique_rows";
    case GradPath::kSlotSums: return "slot_sums";
    case GradPath::kSlotRows: return "slot_rows";
  }
  return "?";
}

StepInputs Engine::step_inputs() const {
  StepInputs in;
  in.gpu = be_->is_gpu();
  in.remaps = be_->remaps_positions();
  in.red_pairs = red_pairs_ != nullptr;
  in.red_rowv = red_rowv_ != nullptr;
  in.fm_vals = fm_vals_;
  in.csr = cfg_.csr;
  in.sum_slices = cfg_.sum_slices;
  in.kind = cfg_.model.kind;
  in.fm_math = cfg_.model.fm_math;
  in.L = table_.L;
  in.scratch_cap = (double)scratch_.cap;
  in.max_nnz = (double)cfg_.max_nnz;
  in.max_rows = (double)cfg_.max_rows;
  in.pstride = pstride();
  in.slice_cap = slice_cap_;
  in.kdim = cfg_.model.kernel_dim();
  in.lead_handoff = cfg_.lead_handoff;
  in.red_rank = cfg_.red_rank;
  in.red_local = cfg_.red_local;
  in.red_apply = cfg_.red_apply;
  return in;
}

StepPlan plan_step(const StepInputs& in, int S) {
  constexpr double k32 = 4294967295.0;  // (32-bit dest * width bounds)
  StepPlan p;
  p.S = S;
  const TableLayout& L = in.L;
  const bool lr16_slot = in.kind == kLR && L.lr16();
  // CSR: several ordered slices of LR-FTRL 16-byte slots or reference FM, on
  // unique-index positions; dests = unique * 2^sl + slice inside one bucket
  // and in 32 bits
  // standard FM / MVM: full-row entries from the vector records' scatter-
  // free form (k_red_csr_vec; MVM's vector is its D-wide T, NV = D)
  const bool fm_std = in.kind == kFM && in.fm_math == kFmStandard;
  const bool mvm = in.kind == kMVM && in.kdim >= 2;
  const int vnv = fm_std ? 1 + in.kdim : in.kdim;  // (vector records' NV)
  const bool std_ok = (fm_std || mvm) && in.gpu && in.red_rowv &&
                      std::ceil(in.max_rows / fmstd_block(vnv - 1)) <= kSegMaxGroups;
  // below these slice counts the slice-group layouts win (same-box A/B at the
  // bench batch, profiles/r5_ab.txt #27: LR S = 4 499.8 vs 533.7, standard FM
  // S = 4 266.2 vs 270.4, MVM S = 2 182.9 vs 273.1; reference FM ties at S = 2)
  const int csr_min = (in.kind == kLR || fm_std) ? 8 : 4;
  if (in.csr && S >= csr_min && !in.sum_slices && in.red_pairs && in.remaps &&
      (lr16_slot || in.fm_vals || std_ok)) {
    int sl = 0;
    while ((1 << sl) < S) ++sl;
    const int nv = in.fm_vals ? 2 : (std_ok ? vnv : 1);
    if (sl <= red_shift(nv) && in.max_nnz * (double)(1 << sl) < k32) {
      p.csr_slog2 = sl;
      p.csr_rows = std_ok;
      p.grad = GradPath::kCsr;
      return p;
    }
  }
  p.groups = Engine::slice_groups(S);
  // (slice groups always run the masked multi-slice paths: every group has >= 2 slices)
  p.Sf = p.groups > 1 ? Engine::kSliceGroup : S;
  p.masks = p.Sf > 1 && !in.sum_slices;
  // LR-FTRL on 16-byte slots, bucket reduction: the reduction writes
  // normalised gradients in unique order (through the compaction's slot ->
  // unique index map; S > 1: [unique][slice] plus the slice bits) and the
  // apply takes (n, z) from the pull, so it reads nothing at random and
  // writes the slot once
  const bool lr16_ok = in.gpu && lr16_slot && in.red_pairs && in.scratch_cap < k32;
  // unique-index positions: pulled rows, gradient destinations and every
  // gradient / mask buffer in unique order -- the reductions span the unique
  // keys (S x that with S slices), not the 4x-headroom scratch slots.  The
  // remap pass costs ~40 us per 10.2 M occurrences; same-box A/B
  // (profiles/r4_unique_positions_ab.txt): a win with several slices (FM-8
  // std S = 8 143 -> 222 M samples/s, FM-8 S = 8 +1.9 %, LR S = 8 +0.8 %),
  // for standard FM (+10.5 %) and MVM (live +13 %, degenerate +2.3 %), a loss
  // for one-slice LR (-5.1 %) and reference FM (-1.4 %)
  p.upos = in.remaps && in.red_pairs &&
           (p.Sf > 1 || in.kind == kMVM || (in.kind == kFM && in.fm_math == kFmStandard));
  // slice bits from the reduction (dest * pstride in 32 bits)
  const double key_bound = p.upos ? in.max_nnz : in.scratch_cap;
  const bool red_masks = in.red_pairs && key_bound * in.slice_cap * in.pstride < k32 &&
                         (in.kind == kLR || in.kind == kFM ||
                          (in.kind == kMVM && in.red_rowv && in.kdim >= 2));
  p.lr16 = lr16_ok && (p.Sf == 1 || (p.masks && red_masks));
  // summed slices: slot-indexed sums (packed apply), still the (n, z) stash
  p.lr16s = lr16_ok && p.Sf > 1 && !p.lr16;
  // several slices on the reduction path: unique-order [unique][slice]
  // gradients plus the slice bits the reduction writes; the pull clears the
  // bits, the apply reads only the present slices
  p.uqm = p.masks && red_masks;
  // reference FM: the normalised (B, C) sums land in unique order
  p.fmu = in.fm_vals && (p.Sf == 1 || p.uqm);
  // compact reference-FM rows of a grouped step: the (B, C) of later groups
  // expand with the PULLED weights, not the table's (updated by the earlier
  // groups), so the pull keeps the per-parameter weights
  p.fm_keep_w = in.fm_vals && p.groups > 1;
  // MVM (one slice) and standard-math FM (any slices) on their reduction
  // paths: the per-key gradient rows land in unique order too (a dense apply
  // read instead of slot-indexed rows the apply had to zero after reading)
  const bool rows_ok = in.gpu && in.red_pairs && key_bound * in.pstride * in.slice_cap < k32;
  // (kdim >= 2, here and in red_masks: an Engine never has red_rowv at width
  // 1, so this only matters to callers of the bare plan_step who pass it)
  p.mvmu = rows_ok && p.Sf == 1 && in.kind == kMVM && in.red_rowv && in.kdim >= 2;
  p.fsu = rows_ok && (p.Sf == 1 || p.uqm) && in.kind == kFM && in.fm_math == kFmStandard;
  p.rowu = p.mvmu || p.fsu;
  // FTRL with several params per key on the packed apply: the pull stashes
  // every key's (n, z) in unique order for the first group's apply
  p.grpst = in.gpu && L.opt == kFTRL && L.P > 1;
  // the unique-order outputs of a multi-slice step and their slice bits
  p.uq = p.Sf > 1 && (p.lr16 || p.fmu || p.fsu);
  p.grad = p.lr16 ? GradPath::kUniqueLR
           : p.fmu ? GradPath::kUniqueFmBC
           : p.rowu ? GradPath::kUniqueRows
           : p.lr16s ? GradPath::kSlotSums
           : GradPath::kSlotRows;
  // The leader handoff: one-slice LR on the bucket reduction with slot
  // positions (nothing between the dedup and k_lr_lead reads pos), a
  // field-major batch of whole kLeadTile-row tiles no wider than the
  // kernel's register rows, slots below the follower bit.  Does not change
  // the gradient layout.
  p.lead = in.lead_handoff && in.gpu && in.kind == kLR && S == 1 && in.red_pairs && !p.upos &&
           in.field_major && in.rows >= kLeadTile && std::fmod(in.rows, (double)kLeadTile) == 0.0 &&
           in.fields >= 1.0 && in.fields <= kLeadMaxFields && in.scratch_cap < 2147483648.0;
  // Ranked reduction outputs: the one-slice steps whose bucket reduction
  // (k_red_sum) writes unique-order outputs from slot positions -- LR with or
  // without the handoff, reference FM's (B, C).  The dedup then writes no
  // slot -> unique map.  Does not change the gradient layout.
  p.red_rank = in.red_rank && in.gpu && S == 1 && in.red_pairs && !p.upos && (p.lr16 || p.fmu);
  // Bucket-sorted producer regions: exactly the handoff steps (k_lr_lead is
  // the one producer that holds every record's bucket before its backward).
  // Does not change the gradient layout.
  p.red_local = in.red_local && p.lead;
  // FTRL inside the reduction: the bucket-sorted handoff steps whose sums are
  // ranked -- one slice, one group, 16-byte FTRL slots.  Does not change the
  // gradient layout (the unique-order array is just never materialised).
  p.red_apply = in.red_apply && p.red_local && p.red_rank && p.lr16;
  return p;
}

// Several slices, one pass: dedup -> pull (stash) -> one producer pass over
// every slice with dests unique * 2^slog2 + slice -> the CSR reduction (only
// the touched (key, slice) pairs) -> one apply whose per-key chains push the
// slices in order.  Replaces the slice groups' per-group sums and applies.
void Engine::train_step_csr(const BatchView& b, int S, int slog2) {
  const int32_t* srows = slice_rows_dev(b, S);
  const bool fm = fm_vals_;
  // standard FM / MVM: full-row entries (k_red_csr_vec), applied by the packed CSR apply
  const bool rows = csr_full_rows();
  const int ew = rows ? csr_row_words(table_.L.P) : 0;
  float* stash = fm || rows ? grp_nz_.ensure(*be_, 2 * (size_t)cfg_.max_nnz * table_.L.P)
                            : lr_nz_.ensure(*be_, 2 * (size_t)cfg_.max_nnz);
  PullArgs pa = begin_fused_step(b, true, true);
  pa.out_nz = stash;
  be_->table_pull(pa);

  // (entries normalised by the reduction; reference FM: B and C before the
  // expansion, as the slice-group path and the multi-rank send buffer do)
  csr_forward_backward(b, slog2, srows, true);

  ApplyArgs aa = apply_args(uniq_keys_, uniq_slot_, ws_->n_uniq, b.nnz, S);
  aa.fm_compact = fm;
  aa.nz_stash = stash;
  aa.csr_off = csr_off_;
  aa.csr_cnt = csr_cnt_;
  aa.csr_ent = rows ? static_cast<const void*>(csr_vent_.get()) : red_pairs_.get();
  aa.csr_ew = ew;
  // (a chain has at most S entries: with S <= 16 nothing is ever deferred)
  aa.csr_long = S > 16 ? csr_long_list(b.nnz) : nullptr;
  aa.csr_long_cap = (int64_t)csr_long_.capacity();
  attach_snapshot(aa);
  be_->table_apply(aa);
  end_step();
}

void Engine::csr_forward_backward(const BatchView& b, int slog2, const int32_t* srows,
                                  bool normalise) {
  csr_off_.ensure(*be_, (size_t)cfg_.max_nnz);  // (the CSR arrays' one allocation site)
  csr_cnt_.ensure(*be_, (size_t)cfg_.max_nnz);
  FwdArgs fa = train_fwd_args(b, ws_->pos, 1 << slog2);
  fa.agg_ok = true;  // (dests below max_nnz * 2^slog2 < 2^32: csr_slog2)
  fa.red_nuq = ws_->n_uniq;
  fa.fm_compact = fm_vals_;
  fa.red_csr.off = csr_off_;
  fa.red_csr.cnt = csr_cnt_;
  fa.red_csr.ent = red_pairs_;
  fa.red_csr.slog2 = slog2;
  fa.red_csr.rows = normalise ? srows : nullptr;
  if (csr_full_rows()) {  // full-row entries
    const int ew = csr_row_words(table_.L.P);
    fa.red_csr.ent = csr_vent_.ensure(*be_, (size_t)cfg_.max_nnz * ew);
    fa.red_csr.P = table_.L.P;
    fa.red_csr.ew = ew;
  }
  be_->forward_backward(fa);
  ++csr_steps_;
}

u32* Engine::csr_long_list(int64_t n) {
  if (!be_->is_gpu()) return nullptr;
  // (wave-private lists: n plus a grid-stride iteration of every wave's keys,
  // <= 8192 x 4 waves x 64, and the per-wave counts)
  // (+ the dense list of n, the offsets and the scan tiles)
  const int64_t need = 2 * n + (int64_t)(2u << 20) + 4 * 65536;
  csr_long_.reserve(*be_, (size_t)need, (size_t)(need + n / 4));
  return csr_long_;
}

void Engine::csr_debug(std::vector<u32>& off, std::vector<u32>& cnt, std::vector<u32>& words) {
  off.clear();
  cnt.clear();
  words.clear();
  if (!csr_off_) return;
  const int64_t n = n_unique();
  off.resize((size_t)n);
  cnt.resize((size_t)n);
  be_->copy_d2h(off.data(), csr_off_, sizeof(u32) * (size_t)n);
  be_->copy_d2h(cnt.data(), csr_cnt_, sizeof(u32) * (size_t)n);
  u64 end = 0;
  for (int64_t i = 0; i < n; ++i) end = std::max<u64>(end, (u64)off[i] + cnt[i]);
  // (full-row entries, MVM's too, are in csr_vent_: csr_forward_backward)
  const bool rows = csr_vent_ && csr_full_rows();
  const int w = rows ? csr_row_words(table_.L.P) : csr_entry_bytes() / 4;
  words.resize((size_t)end * w);
  if (end) be_->copy_d2h(words.data(), rows ? static_cast<const void*>(csr_vent_.get()) : red_pairs_.get(),
                         sizeof(u32) * (size_t)end * w);
}

std::vector<u64> Engine::unique_keys() {
  std::vector<u64> k((size_t)n_unique());
  if (!k.empty()) be_->copy_d2h(k.data(), uniq_keys_, sizeof(u64) * k.size());
  return k;
}

Engine::RedGeometry Engine::red_geometry(int S, int64_t nuq) {
  RedGeometry g;
  const bool fm_std = cfg_.model.kind == kFM && cfg_.model.fm_math == kFmStandard;
  const bool mvm = cfg_.model.kind == kMVM && cfg_.model.kernel_dim() >= 2;
  const int kd = cfg_.model.kernel_dim();
  const int nv = fm_vals_ ? 2 : (fm_std ? 1 + kd : (mvm ? kd : 1));
  int sl = 0;
  while ((1 << sl) < S) ++sl;
  g.base = red_shift(nv);
  g.maxb = red_maxb_ > 0 ? red_maxb_ : kRedMaxBuckets;
  g.nsub = red_nsub_;
  g.nb = red_nb_;
  g.nuq = nuq >= 0 ? nuq : n_unique();
  // RedGeom::shift and RedGeom::active (csrc/hip/model_common.h), dests = unique << sl
  const u64 dests = (u64)g.nuq << sl;
  int sh = g.base;
  while (((dests + (1ull << sh) - 1) >> sh) > (u64)kRedMaxBuckets) ++sh;
  if (g.maxb > kRedMaxBuckets && sh - g.base >= 2)
    while (sh > g.base && ((dests + (1ull << (sh - 1)) - 1) >> (sh - 1)) <= (u64)g.maxb) --sh;
  const int min_shift = csr_full_rows() ? kCsrVecMinShift : 0;
  g.shift = sh < min_shift ? min_shift : sh;
  const u64 n = (dests + (1ull << g.shift) - 1) >> g.shift;
  g.needed = (int64_t)n;  // (beyond nb: the step's dests do not fit the allocated buckets)
  g.buckets = n < (u64)g.nb ? (int)n : g.nb;
  return g;
}

void Engine::train_step(const BatchView& b) {
  refuse_frozen("train_step");
  stale_stashes();  // the table changes: server stashes are stale
  use_worker_set(0);
  const int S = slices_of(b);
  if (S > cfg_.max_slices) throw std::invalid_argument("batch has more slices than max_slices");
  if (cfg_.sum_slices && slice_groups(S) > 1)
    throw std::invalid_argument("sum_slices: at most 32 slices per step (ordered pushes: any count)");
  // every layout decision, made once (plan_step)
  const StepPlan P = plan(S, b.rows, b.nnz_per_row, !b.row_ptr && b.col_stride > 0 && b.col_stride == b.rows);
  if (P.grad == GradPath::kCsr) {
    train_step_csr(b, S, P.csr_slog2);
    return;
  }
  const int ng = P.groups;
  const int ps = pstride();
  const bool masks = P.masks;
  const int32_t* srows = slice_rows_dev(b, S);
  const bool uqm = P.uqm, fm_keep_w = P.fm_keep_w, uq = P.uq, upos = P.upos;
  // (dest * ps in 32 bits over unique indices or scratch slots, see plan_step)
  const double key_bound = upos ? (double)cfg_.max_nnz : (double)scratch_.cap;
  // The unique-order gradient output, if the plan has one: the reduction
  // writes it (through the slot -> unique map unless positions are unique
  // indices already), the pull zeroes it, the apply reads it densely and
  // neither maps nor clears it.
  struct {
    float* buf = nullptr;
    int width = 0;            // floats per (key, slice)
    bool normalised = false;  // the reduction divides by the slice's rows (else the apply does)
    bool pull_zeroes = true;  // (the slice bits instead when several slices run: uq)
  } uo;
  const size_t un = (size_t)cfg_.max_nnz;
  if (P.red_apply) {
    // (never materialised: the reduction pushes each sum where it would store it)
    uo = {nullptr, 1, true, false};
  } else if (P.lr16) {
    uo = {lr_grad_.ensure(*be_, un * slice_cap_), 1, true, true};
  } else if (P.fmu) {  // (B, C) normalised before the expansion: 2 divisions a key, not P
    uo = {fm_grad_.ensure(*be_, 2 * un * slice_cap_), 2, true, true};
  } else if (P.rowu) {
    // (one-slice standard FM: every unique key's row is written by the
    // reduction -- each occurrence leaves a record, k_fm_std_red -- so the
    // pull need not zero them)
    uo = {row_grad_.ensure(*be_, un * ps * (P.fsu ? slice_cap_ : 1)), ps, false,
          !(P.fsu && P.Sf == 1)};
  }
  // the (n, z) the pull stashes in unique order for the first group's apply
  float* nz = P.lr16 || P.lr16s ? lr_nz_.ensure(*be_, 2 * un)
              : P.grpst         ? grp_nz_.ensure(*be_, 2 * un * table_.L.P)
                                : nullptr;
  if (fm_keep_w) fm_w_.ensure(*be_, un * ps);
  if (uq) lr_mask_.ensure(*be_, un);

  PullArgs pa = begin_fused_step(b, upos || (uo.buf && !P.red_rank), upos, P.lead);
  if (fm_keep_w) pa.out_w = fm_w_;
  pa.out_nz = nz;
  if (uo.buf && uo.pull_zeroes) {
    pa.zero_out = uo.buf;
    pa.zero_width = uo.width;
  }
  if (uq) {  // S > 1: only a key's present slices are read, so only its bits need clearing
    pa.zero_out = reinterpret_cast<float*>(lr_mask_.get());
    pa.zero_width = 1;
  }
  be_->table_pull(pa);

  for (int k = 0; k < ng; ++k) {
    const u32* posk = ws_->pos;
    const BatchView bk = group_view(b, S, k, posk);
    const int Sg = group_slices(S, k);
    const int32_t* srk = srows + (int64_t)k * kSliceGroup;
    // a later group's unique-order slice bits start from zero again: the
    // pull cleared them for the first group, each group's apply clears the
    // bits it read (ApplyArgs::masks_clear); a later group's apply reads the
    // table, which the earlier groups updated, instead of the pull's stash
    const bool stash = k == 0;

    FwdArgs fa = train_fwd_args(bk, posk, Sg);
    fa.agg_ok = key_bound * Sg * ps < 4294967295.0;  // (32-bit dest * ps, see rows_ok)
    if (upos) fa.red_nuq = ws_->n_uniq;
    fa.lead = P.lead;  // (one group, one slice: the whole batch's positions)
    fa.red_local = P.red_local;
    // slice bits from the reduction (unique order with the outputs, else
    // slot-indexed), else per occurrence
    if (uq) fa.red_masks = lr_mask_;
    else if (uqm) fa.red_masks = tmask_;
    else if (masks) be_->slice_masks(bk, posk, tmask_);
    // reference-math FM on the GPU reduction path: (B, C) rows, expanded by the apply
    fa.fm_compact = fa.red_pairs && fa.agg_ok && cfg_.model.kind == kFM &&
                    cfg_.model.fm_math == kFmReference;
    if (fm_vals_ && !fa.fm_compact) throw std::logic_error("train_step: compact FM rows need the reduction");
    if (uo.buf || P.red_apply) {
      fa.red_out = uo.buf;
      // (unique-index positions: the outputs' rows are the dests' own)
      fa.red_inv = upos || P.red_rank ? nullptr : ws_->inv.get();
      if (P.red_rank) {  // (the stamps and chunk offsets the dedup above left)
        fa.red_rank_offs = block_counts_;
        fa.red_rank_stamps = scratch_.stamps;
        fa.red_rank_epoch = scratch_.epoch;
      }
      if (uo.normalised) fa.red_rows = srk;
    }
    if (P.red_apply) {
      // the apply's inputs: the reduction's launch is the step's last (one
      // group), and carries the snapshot the apply's would
      fa.red_apply_words = table_.words;
      fa.red_apply_slots = uniq_slot_;
      fa.red_apply_nz = nz;
      fa.red_apply_ftrl = cfg_.opt.ftrl;
      attach_snapshot(fa, b.nnz);
    }
    be_->forward_backward(fa);
    if (P.red_apply) continue;

    ApplyArgs aa = apply_args(uniq_keys_, uniq_slot_, ws_->n_uniq, b.nnz, Sg);
    aa.sum_slices = cfg_.sum_slices;
    aa.fm_compact = fa.fm_compact;
    if (fm_keep_w) aa.pulled = fm_w_;
    aa.nz_stash = stash ? nz : nullptr;  // (unique order, as the apply's entries)
    if (uo.buf) {  // already in unique order, zeroed by the next pull
      aa.grads = uo.buf;
      aa.gstride = uo.width;
      aa.slice_rows = uo.normalised ? nullptr : srk;
    } else {  // slot- or unique-indexed rows of raw sums
      aa.grads = grad_;
      aa.grad_map = upos ? nullptr : ws_->uniq_pos.get();
      aa.zero_after = true;
      aa.slice_rows = srk;
    }
    if (uq) {  // present slices by the unique-order bits (cleared by the next pull)
      aa.masks = lr_mask_;
      aa.masks_clear = k + 1 < ng;  // (for the next group's reduction)
    } else if (masks) {
      aa.masks = tmask_;
      aa.masks_rw = tmask_;
    }
    attach_snapshot(aa);
    be_->table_apply(aa);
  }
  end_step();
}

PullArgs Engine::begin_fused_step(const BatchView& b, bool want_inv, bool upos, bool lead) {
  if (want_inv) ensure_inv();
  // (leader-encoded positions are not slots: nothing may remap them)
  if (lead && upos) throw std::logic_error("begin_fused_step: leader handoff with unique positions");
  dedup_(b, 1, nullptr, want_inv, nullptr, lead);
  ws_->inv_valid = false;  // (the sharded step's send order is not this one)
  if (upos) be_->remap_pos(ws_->pos, b.nnz, ws_->inv, (u32)scratch_.cap);
  guard_inserts(b.nnz);  // (<= nnz new keys; may grow the table first)
  // (delta checkpoints: every apply of the step pushes these keys only)
  delta_mark(uniq_keys_, ws_->n_uniq, b.nnz);
  PullArgs pa = pull_args(uniq_keys_, ws_->n_uniq, b.nnz, true, uniq_slot_);
  pa.admit = admit_;
  pa.out_vals = wpull_;
  pa.out_map = upos ? nullptr : ws_->uniq_pos.get();
  pa.pstride = pstride();
  pa.fm_vals = fm_vals_;
  return pa;
}

void Engine::eval_step(const BatchView& b, float* pctr) {
  // (a frozen LR table: lookup and score in one launch, but for the batch
  // sizes at which the three launches measured faster)
  if (serve_lr_ && !(b.rows >= cfg_.serve_unfused_lo && b.rows < cfg_.serve_unfused_hi)) {
    ServeLrArgs sa;
    sa.table = table_;
    sa.batch = b;
    sa.pctr = pctr;
    sa.stats = stats_ + 1;
    be_->serve_lr(sa);
    return;
  }
  // (frozen FM / MVM likewise, with a window of their own; fm_vals_: the
  // forward below would sum compact value rows, so the kernel does)
  if (serve_model_ &&
      !(b.rows >= cfg_.serve_unfused_latent_lo && b.rows < cfg_.serve_unfused_latent_hi)) {
    ServeArgs sa;
    sa.table = table_;
    sa.batch = b;
    sa.pctr = pctr;
    sa.stats = stats_ + 1;
    sa.model = cfg_.model;
    sa.opt = cfg_.opt;
    sa.fm_vals = fm_vals_;
    be_->serve_model(sa);
    return;
  }
  use_worker_set(0);
  dedup_(b);
  PullArgs pa = pull_args(uniq_keys_, ws_->n_uniq, b.nnz, false, uniq_slot_);
  pa.out_vals = wpull_;
  pa.out_map = ws_->uniq_pos;
  pa.pstride = pstride();
  pa.fm_vals = fm_vals_;
  be_->table_pull(pa);
  be_->forward_backward(eval_fwd_args(b, pctr));
}

}  // namespace xflow
