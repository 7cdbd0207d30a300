// xflow-amd: Engine implementation (device agnostic; talks to a Backend).
#include <cstdlib>
#include "xflow/engine.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <fstream>
#include <stdexcept>
#include <string>

namespace xflow {

namespace {

uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

constexpr char kMagic[8] = {'X', 'F', 'L', 'O', 'W', 'T', 'B', '1'};
constexpr char kServingMagic[8] = {'X', 'F', 'L', 'O', 'W', 'S', 'W', '1'};

// XFLOW_NO_MONITOR=1: no per-step capacity snapshot (A/B of the monitor's
// cost only; growth then relies on exact-size reads, overflow on the
// epoch-end check)
bool monitor_disabled() {
  static const bool off = std::getenv("XFLOW_NO_MONITOR") != nullptr;
  return off;
}

}  // namespace

// Every argument check, before anything is allocated.
const EngineConfig& Engine::validated(const EngineConfig& cfg) {
  if (cfg.table_log2_cap < 4 || cfg.table_log2_cap > 31)
    throw std::invalid_argument("table_log2_cap must be in [4, 31]");
  if (!(cfg.grow_load > 0.0 && cfg.grow_load < 1.0))
    throw std::invalid_argument("grow_load must be in (0, 1)");
  if (cfg.monitor_lag < 0 || cfg.monitor_lag >= kSnaps)
    throw std::invalid_argument("monitor_lag must be in [0, 63]");
  if (cfg.max_slices < 1) throw std::invalid_argument("max_slices must be >= 1");
  if (cfg.model.kind != kLR && (cfg.model.v_dim < 1 || cfg.model.v_dim > 32))
    throw std::invalid_argument("v_dim must be in [1, 32]");
  if (cfg.admit_min_count < 1 || cfg.admit_min_count > 255)
    throw std::invalid_argument("admit_min_count must be in [1, 255]");
  if (cfg.admit_log2 != 0 && (cfg.admit_log2 < kAdmitBlockLog2 || cfg.admit_log2 > kAdmitMaxLog2))
    throw std::invalid_argument("admit_log2 must be 0 (automatic) or in [6, 32]");
  if (cfg.delta_log2 != 0 && (cfg.delta_log2 < kDeltaMinLog2 || cfg.delta_log2 > kDeltaMaxLog2))
    throw std::invalid_argument("delta_log2 must be 0 (automatic) or in [10, 34]");
  if (next_pow2((uint64_t)((double)cfg.max_nnz * cfg.scratch_factor) + 1) > (1ull << 31))
    throw std::invalid_argument("max_nnz too large");
  if (cfg.opt.kind != kFTRL && cfg.opt.kind != kSGD && cfg.opt.kind != kFrozen)
    throw std::invalid_argument("optimizer kind must be 0 (FTRL), 1 (SGD) or 2 (frozen)");
  if (cfg.opt.kind == kFrozen) {
    if (cfg.opt.frozen_from != kFTRL && cfg.opt.frozen_from != kSGD)
      throw std::invalid_argument("frozen_from must be 0 (FTRL) or 1 (SGD)");
    // (read-only: nothing is admitted and nothing is tracked)
    if (cfg.admit_min_count > 1)
      throw std::runtime_error("admit_min_count > 1: this engine holds a serving snapshot "
                               "(frozen, read-only): it admits no keys");
    if (cfg.delta_track)
      throw std::runtime_error("delta_track: this engine holds a serving snapshot (frozen, "
                               "read-only): it has no deltas to save");
  }
  // (the FM / MVM window: both bounds negative -- the model's measured default
  // -- or both given)
  if ((cfg.serve_unfused_latent_lo < 0) != (cfg.serve_unfused_latent_hi < 0))
    throw std::invalid_argument("serve_unfused_latent: give both bounds, or both negative "
                                "for the model's default");
  return cfg;
}

void Engine::refuse_frozen(const char* what) const {
  if (frozen())
    throw std::runtime_error(std::string(what) + ": this engine holds a serving snapshot "
                             "(frozen, read-only weights): it cannot be trained, pruned or "
                             "saved as a training checkpoint");
}

Engine::Engine(const EngineConfig& cfg) : cfg_(validated(cfg)) {
  // buffers hold one slice group (more slices per step run group by group)
  slice_cap_ = cfg_.max_slices < kSliceGroup ? cfg_.max_slices : kSliceGroup;
  be_ = cfg_.device >= 0 ? make_hip_backend(cfg_.device) : make_cpu_backend();
  Backend& be = *be_;
  // the device kernels' latent widths: any other v_dim runs padded (inert
  // padded dims, ModelSpec::pad_dim)
  cfg_.model.pad_dim = 0;
  if (be.is_gpu() && cfg_.model.kind != kLR &&
      device_latent_width(cfg_.model.v_dim) != cfg_.model.v_dim)
    cfg_.model.pad_dim = device_latent_width(cfg_.model.v_dim);

  // persistent table
  table_.L = TableLayout::make(cfg_.model, cfg_.opt);
  log2_cap_ = cfg_.table_log2_cap;
  max_log2_cap_ = cfg_.max_log2_cap > 0 ? (cfg_.max_log2_cap < 31 ? cfg_.max_log2_cap : 31) : 31;
  if (max_log2_cap_ < log2_cap_) max_log2_cap_ = log2_cap_;
  if (!(cfg_.grow_start > 0.0 && cfg_.grow_start < cfg_.grow_load))
    cfg_.grow_start = 0.75 * cfg_.grow_load;
  // geometry (backend.h TableView): segments of at most 2^kMaxSegLog2 (2^20) slots
  table_.seg_log2 = log2_cap_ < kMaxSegLog2 ? log2_cap_ : kMaxSegLog2;
  table_.level = log2_cap_ - table_.seg_log2;
  table_.split = 0;
  table_.cap = 1ull << log2_cap_;
  const u64 seg = 1ull << table_.seg_log2;
  table_.probe_limit = seg < kMaxProbe ? seg : kMaxProbe;
  max_segs_ = cfg_.table_grow ? (1ull << max_log2_cap_) >> table_.seg_log2 : table_.cap >> table_.seg_log2;
  table_bytes_ = (size_t)table_.cap * table_.L.stride * sizeof(u32);
  table_.words = static_cast<u32*>(
      be.table_reserve((size_t)(max_segs_ << table_.seg_log2) * table_.L.stride * sizeof(u32),
                       max_segs_ > (table_.cap >> table_.seg_log2)));
  table_range_.e = this;  // (from here on the range is released on unwinding)
  table_.words = static_cast<u32*>(be.table_commit(table_.words, table_bytes_));
  // one 16-byte block {size, overflow[2]}: a step's snapshot is one copy
  overflow_ = mon_.alloc_zero(be, 4) + 2;
  table_.size = reinterpret_cast<unsigned long long*>(mon_.get());
  table_.overflow = overflow_ + 1;
  be.table_clear(table_);
  // feature admission: the counting filter (EngineConfig::admit_min_count)
  if (cfg_.admit_min_count > 1) {
    const int top = cfg_.table_grow ? max_log2_cap_ : log2_cap_;
    admit_.log2 = cfg_.admit_log2 ? cfg_.admit_log2 : (top + 1 < kAdmitMaxLog2 ? top + 1 : kAdmitMaxLog2);
    if (admit_.log2 < kAdmitBlockLog2) admit_.log2 = kAdmitBlockLog2;
    admit_.min_count = cfg_.admit_min_count;
    admit_.counters = admit_counters_.alloc_zero(be, (size_t)1 << admit_.log2);
  }
  // delta checkpoints: the touched-key filter (EngineConfig::delta_track)
  if (cfg_.delta_track) {
    const int top = cfg_.table_grow ? max_log2_cap_ : log2_cap_;
    delta_log2_ = cfg_.delta_log2 ? cfg_.delta_log2
                                  : (top + 2 < kDeltaMaxLog2 ? top + 2 : kDeltaMaxLog2);
    if (delta_log2_ < kDeltaMinLog2) delta_log2_ = kDeltaMinLog2;
    delta_bits_.alloc_zero(be, (size_t)1 << (delta_log2_ - 5));
  }
  std::memset(snaps_.alloc(be, kSnaps), 0, sizeof(HostSnap) * kSnaps);

  // per-step dedup scratch
  const int64_t nnz = cfg_.max_nnz;
  scratch_.cap = next_pow2((uint64_t)((double)nnz * cfg_.scratch_factor) + 1);
  scratch_.keys = scratch_keys_.alloc(be, scratch_.cap);
  be.fill_u64(scratch_.keys, kEmptyKey, scratch_.cap);
  scratch_.stamps = scratch_stamps_.alloc_zero(be, scratch_.cap);
  scratch_.claims = scratch_claims_.alloc_zero(be, 1);
  // Rebuild once half full: one more step adds at most max_nnz <= cap/factor
  // keys, so the load factor stays below 0.5 + 1/factor.
  scratch_.rebuild_at = scratch_.cap / 2;
  scratch_.epoch = 0;
  if (be.is_gpu()) {
    // adaptive active capacity (ScratchView::ctl): starts at the allocation
    scratch_.ctl = scratch_ctl_.alloc(be, kScratchCtlWords);
    unsigned long long c0[kScratchCtlWords] = {scratch_.cap};
    static_assert(kScratchCtlWords >= 8, "ScratchView::ctl[0..7]");
    be.copy_h2d(scratch_.ctl, c0, sizeof(c0));
    scratch_.carry = cfg_.scratch_carry;
  }
  block_counts_.alloc(be, scratch_.cap / 4096 + 1);

  const int ps = cfg_.model.pstride();
  uniq_keys_.alloc(be, nnz);
  uniq_slot_.alloc(be, nnz);
  use_worker_set(0);
  // slot-indexed buffers carry one extra row: the trash slot (index cap) that
  // a dedup probe overflow sends its occurrences to (flagged, never applied)
  const uint64_t rows1 = scratch_.cap + 1;
  grad_.alloc_zero(be, rows1 * slice_cap_ * ps);
  tmask_.alloc_zero(be, rows1);
  // atomic-free gradient reduction (FwdArgs::red_*): LR (1 value per key) and
  // reference-math FM (2 values per key, 16-byte records)
  const bool fm_ref = cfg_.model.kind == kFM && cfg_.model.fm_math == kFmReference;
  // standard FM: vector records (dest, 1 + D sums) per (key, slice, column)
  // and workgroup (k_fm_std_red), at most one per occurrence
  const bool fm_std = cfg_.model.kind == kFM && cfg_.model.fm_math == kFmStandard;
  // (MVM: the reduction sums the D-wide T = loss*M rows, which the kernels
  // have for D >= 2; width 1 aggregates in LDS / by atomics, dispatch_mvm)
  const bool mvm = cfg_.model.kind == kMVM && cfg_.model.kernel_dim() >= 2;
  if (be.is_gpu() && (cfg_.model.kind == kLR || fm_ref || fm_std || mvm)) {
    // values per record: 1 (LR), 2 (reference FM), the vector records of
    // standard FM (1 + D) and MVM (D: per-row T = loss*M sums)
    const bool vec = fm_std || mvm;
    const int kd = cfg_.model.kernel_dim();
    const int nv = fm_ref ? 2 : (fm_std ? 1 + kd : (mvm ? kd : 1));
    const int shift = red_shift(nv);
    // u64 words per record slot: nv for LR / reference FM, the vector record otherwise
    const int recw = vec ? vec_rec_words(nv) / 2 : nv;
    const int group_rows = fm_ref ? kFmGroupRows : (vec ? kFmStdMinGroupRows : kLrGroupRows);
    // (the trash slot's occurrences are never reduced: FwdArgs::trash_pos)
    // Buckets of 2^shift dests at the allocated capacity; beyond
    // kRedMaxBuckets the device widens the buckets (FwdArgs::red_bcap) and
    // sums a wide bucket with red_nsub workgroups -- only when the adaptive
    // scratch has grown that far (bench shape: S = 8 at 2^23 active slots
    // stays at 4096 buckets of 2^14).
    uint64_t dests = scratch_.cap * (uint64_t)slice_cap_;
    // A CSR step reduces every slice at once, not one slice group: its dests
    // are unique << slog2, up to max_nnz << slog2(max_slices).  Wherever
    // plan_step takes the CSR path the buckets cover that too (a dest past
    // the allocated buckets has no cursor in k_red_scatter).
    {
      int sl = 0;
      while ((1 << sl) < cfg_.max_slices) ++sl;
      const uint64_t csr_dests = (uint64_t)cfg_.max_nnz << sl;
      if (cfg_.csr && sl <= shift && csr_dests < 4294967295ull && csr_dests > dests) dests = csr_dests;
    }
    // vector records: the producer's larger bucket cap where its LDS allows
    // (vec_red_max_buckets) and the batch fits the scatter-free form
    const int vd = nv - 1;  // k_fm_std_red<vd>: NV = 1 + vd
    const int maxb = vec && (cfg_.max_rows + fmstd_block(vd) - 1) / fmstd_block(vd) <= kSegMaxGroups
                         ? vec_red_max_buckets(vd)
                         : kRedMaxBuckets;
    red_maxb_ = vec ? maxb : 0;
    int nb = (int)((dests + (1ull << shift) - 1) >> shift);
    int nsub = 1;
    while ((uint64_t)nb > (uint64_t)maxb * nsub) nsub <<= 1;
    if (nsub > 1) nb = maxb;
    red_nsub_ = nsub;
    if (nb <= maxb && dests < (1ull << 32)) {
      const int64_t groups = (cfg_.max_rows + group_rows - 1) / group_rows;
      red_nb_ = nb;
      red_pairs_.alloc(be, (size_t)nnz * recw);
      red_sorted_.alloc(be, (size_t)nnz * recw);
      red_hist_.alloc(be, (size_t)nb * groups);
      red_tot_.alloc(be, 2 * (size_t)nb + 2);
      red_count_.alloc(be, groups);
      red_groups_ = (int)groups;
      // MVM: T = loss*M per row; standard FM: (loss, loss*vs) per row (k_fm_std_fwd)
      if (mvm || fm_std) red_rowv_.alloc(be, (size_t)cfg_.max_rows * ps);
      if (mvm) {
        // (vmax, dup flag, dup |c| max, dup record count: two alternating words each)
        red_vmax_.alloc_zero(be, 8);
        // repeated-field rows' records and fixed-point sums (MvmDup, backend.h)
        const int D = cfg_.model.kernel_dim();
        mdup_ew_ = csr_row_words(D);
        mdup_rec_.alloc(be, (size_t)nnz * mdup_ew_);
        mdup_acc_.alloc(be, (size_t)nnz * D);
        mdup_claim_.alloc(be, (size_t)nnz);
      }
    }
  }
  // reference-math FM with the GPU reduction: compact (w, Σv, Σv^2, 0) value rows
  fm_vals_ = red_pairs_ && fm_ref;
  vstride_ = fm_vals_ ? 4 : ps;
  serve_lr_ = frozen() && cfg_.serve_fused && cfg_.model.kind == kLR && be.serves_lr();
  serve_model_ = frozen() && cfg_.serve_fused && be.serves_models() &&
                 (cfg_.model.kind == kMVM ||
                  (cfg_.model.kind == kFM &&
                   !(cfg_.model.fm_math == kFmStandard && cfg_.model.fm_mfma)));
  if (cfg_.serve_unfused_latent_lo < 0) {  // (validated: then both are)
    // the model's measured window (EngineConfig::serve_unfused_latent_lo).
    // cfg_ holds the window in force from here on, not the caller's (-1, -1):
    // serve_unfused_latent() and eval_step read it
    cfg_.serve_unfused_latent_lo = 0;
    cfg_.serve_unfused_latent_hi =
        cfg_.model.kind == kMVM ? INT64_MAX
                                : (cfg_.model.fm_math == kFmReference ? 512 : 0);
  }
  wpull_.alloc(be, rows1 * vstride_);
  be.memset(wpull_ + scratch_.cap * vstride_, 0, sizeof(float) * vstride_);
  stats_.alloc_zero(be, 2);
  if (!be.partitioned_dedup()) bucket_ws_.alloc(be, 512);  // (Backend::bucket's cursors)
  slice_rows_.alloc(be, kSliceGroup);

  st_keys_.alloc(be, nnz);
  st_fgid_.alloc(be, nnz);
  st_rowptr_.alloc(be, cfg_.max_rows + 1);
  st_labels_.alloc(be, cfg_.max_rows);
  be.synchronize();
}

Engine::~Engine() { be_->synchronize(); }  // (the members release the table range and the buffers)

void Engine::use_worker_set(int wb) {
  if (wb < 0 || wb > 1) throw std::invalid_argument("worker buffer set must be 0 or 1");
  ws_ = &wset_[wb];
  if (ws_->pos) return;
  // first use: set 0 by the constructor, set 1 by the pipelined sharded step
  // (pos last: a set whose allocation threw half way is allocated again)
  Backend& be = *be_;
  const int64_t nnz = cfg_.max_nnz;
  ws_->uniq_pos.alloc(be, nnz);
  if (!be.partitioned_dedup()) ws_->send_pos.alloc(be, nnz);  // (Backend::bucket's output)
  ws_->n_uniq.alloc_zero(be, 1);
  ws_->bcap.alloc_zero(be, 1);
  ws_->pos.alloc(be, nnz);
}

// The GPU reduction path sees every (key, slice) that occurs (a record per
// column-table entry, or per occurrence), so it can write the slice bits:
// every model on its bucket-reduction path.
bool Engine::reduction_masks(bool unique_positions) const {
  // (dest * pstride in 32 bits: dests = unique index x slices with unique-
  // index positions, at most max_nnz keys -- else scratch slot x slices)
  const double keys = unique_positions ? (double)cfg_.max_nnz : (double)scratch_.cap;
  if (!red_pairs_ || keys * slice_cap_ * pstride() >= 4294967295.0) return false;
  return cfg_.model.kind == kLR || cfg_.model.kind == kFM ||
         (cfg_.model.kind == kMVM && red_rowv_ != nullptr);
}

std::vector<int64_t> Engine::parse_text(const char* text, int64_t n, u64* keys, int32_t* fgid,
                                        int32_t* row_ptr, float* labels, int64_t max_rows,
                                        int64_t max_nnz, int64_t row_mod) {
  const int64_t need = text_ws_words(n);
  text_ws_.reserve(*be_, (size_t)need, (size_t)(need + need / 4));
  text_counts_.ensure(*be_, 8);
  TextParseArgs a;
  a.text = text;
  a.n = n;
  a.keys = keys;
  a.fgid = fgid;
  a.row_ptr = row_ptr;
  a.labels = labels;
  a.max_rows = max_rows;
  a.max_nnz = max_nnz;
  a.max_lines = text_max_lines(n);
  a.ws = text_ws_;
  a.ws_words = (int64_t)text_ws_.capacity();
  a.row_mod = row_mod;
  a.counts = text_counts_;
  be_->parse_text(a);
  long long c[7];
  be_->copy_d2h(c, text_counts_, sizeof(c));
  if (c[5]) throw std::runtime_error("parse_text: more lines than n/2 + 2 (a block of empty lines?)");
  if (c[0] > max_rows || c[1] > max_nnz)
    throw std::runtime_error("parse_text: the block holds more rows / features than the arrays");
  return {c[0], c[1], c[0] > 0 ? c[2] : 0, c[3], c[6]};
}

void Engine::shuffle_rows(const BatchView& src, u64 seed, u64* keys, int32_t* fgid, float* labels,
                          int32_t* row_ptr, bool field_major_out, int key_bytes) {
  if (src.col_stride > 0)
    throw std::invalid_argument("shuffle_rows: a field-major source (row-major or CSR only)");
  if (src.rows > cfg_.max_rows) throw std::invalid_argument("shuffle_rows: batch rows exceed max_rows");
  if (src.nnz > cfg_.max_nnz) throw std::invalid_argument("shuffle_rows: batch nnz exceeds max_nnz");
  ShuffleArgs a;
  a.src = src;
  a.key_bytes = key_bytes;
  a.seed = seed;
  a.keys = keys;
  a.fgid = fgid;
  a.labels = labels;
  a.row_ptr = row_ptr;
  a.field_major_out = field_major_out;
  // (the workspace of the CSR form: allocated on the first CSR call, never again)
  if (src.row_ptr && be_->is_gpu()) a.len = shuf_len_.ensure(*be_, (size_t)cfg_.max_rows + 1);
  be_->shuffle_rows(a);
}

void Engine::cross_rows(const CrossArgs& a) {
  const int64_t out_nnz = a.src.nnz + (int64_t)(a.spec.n > 0 ? a.spec.n : 0) * a.src.rows;
  if (a.src.rows > cfg_.max_rows) throw std::invalid_argument("cross_rows: batch rows exceed max_rows");
  if (out_nnz > cfg_.max_nnz)
    throw std::invalid_argument("cross_rows: nnz + crosses * rows exceeds max_nnz");
  be_->cross_rows(a);  // (check_cross_args: the spec, the layouts, int32)
}

void Engine::count_records(bool on) {
  if (on && !rec_count_) rec_count_.alloc_zero(*be_, 1);
  rec_on_ = on;
}

int64_t Engine::take_records() {
  if (!rec_count_) return -1;
  unsigned long long n = 0;
  be_->copy_d2h(&n, rec_count_, sizeof(n));
  be_->memset(rec_count_, 0, sizeof(n));
  return (int64_t)n;
}

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


// log2 of the padded slice count when a step of S slices takes the CSR path
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

void Engine::w_forward_backward_csr(const BatchView& b, const float* pulled, int64_t n_send,
                                    int S_global, int wb, bool pack, u32* cnt_out, void* ent_out,
                                    const int64_t* counts, int world, bool encoded,
                                    int64_t* totals_out) {
  use_worker_set(wb);
  const int St = S_global > 0 ? S_global : slices_of(b);
  const int sl = csr_slog2(St);
  if (sl < 0 || St < slices_of(b) || St > cfg_.max_slices)
    throw std::invalid_argument("w_forward_backward_csr: S_global off the CSR path");
  // (a rank out of data -- a batch of 0 rows -- still takes part: no keys,
  // zero entries per owner)
  if (b.nnz > 0 && !ws_->inv_valid)
    throw std::logic_error("w_forward_backward_csr: needs the partitioned dedup's inv");
  // unique-index (= send-order) positions, and the pulled rows (send order)
  // as the forward's value rows; the trash slot's row stays zero
  be_->remap_pos(ws_->pos, b.nnz, ws_->inv, (u32)scratch_.cap);
  be_->scatter_rows(pulled, wpull_, nullptr, nullptr, n_send, vstride_);
  // (rows per slice: the worker normalises, the owner does not know them)
  csr_forward_backward(b, sl, slice_rows_dev(b, St), true);
  last_nsend_ = n_send;
  if (!pack) return;
  csr_doff_.ensure(*be_, (size_t)cfg_.max_nnz + 1);
  be_->scan_u32(csr_cnt_, csr_doff_, ws_->n_uniq, cfg_.max_nnz);
  be_->csr_pack(csr_off_, csr_cnt_, csr_full_rows() ? static_cast<const void*>(csr_vent_.get()) : red_pairs_.get(),
                csr_doff_, ws_->n_uniq, cfg_.max_nnz, ent_out, csr_entry_bytes());
  be_->copy_d2d(cnt_out, csr_cnt_, sizeof(u32) * (size_t)n_send);
  be_->csr_totals(counts, world, encoded, csr_doff_, totals_out);
}

template <typename Source>
void Engine::apply_by_source(const ApplyArgs& base, const std::vector<int64_t>& src_offsets,
                             int buf, bool stash, const char* need_weights, Source source) {
  const SrvBuf& sb = srv_[buf];
  size_t first_src = 0;
  while (first_src + 1 < src_offsets.size() && src_offsets[first_src + 1] <= src_offsets[first_src])
    ++first_src;
  for (size_t src = 0; src + 1 < src_offsets.size(); ++src) {
    const int64_t o = src_offsets[src], c = src_offsets[src + 1] - o;
    if (c <= 0) continue;
    ApplyArgs aa = base;
    aa.keys = base.keys + o;
    aa.slots = base.slots + o;
    aa.n_host = c;
    aa.n_max = c;
    source(aa, o, c);
    if (aa.fm_compact) {
      aa.pulled = pulled_weights(buf, o);
      // compact value rows carry no per-parameter weights: a later source
      // would expand its (B, C) with weights the earlier sources updated
      if (!aa.pulled && src > first_src) throw std::logic_error(need_weights);
    }
    // the first source applied sees the state its pull saw; a key sent by
    // several sources is updated by the earlier ones, so later sources re-read
    if (stash) aa.nz_stash = sb.nz + 2 * o;  // (a fresh stash exists: s_pull)
    stash = false;
    attach_snapshot(aa);
    be_->table_apply(aa);
  }
}

void Engine::s_apply_csr(const u64* recv_keys, const u32* recv_cnt, const void* recv_ent,
                         const std::vector<int64_t>& src_offsets, int S, int buf) {
  refuse_frozen("s_apply_csr");
  if (buf < 0 || buf >= kSrvBufs) throw std::invalid_argument("server buffer must be in [0, kSrvBufs)");
  SrvBuf& sb = srv_[buf];
  sb.keys = nullptr;  // applied: no slot remap needed after a growth
  bool stash = sb.nz_fresh;
  stale_stashes();
  const u32* off = csr_off_;
  const u32* cnt = csr_cnt_;
  const void* ent = csr_full_rows() ? static_cast<const void*>(csr_vent_.get()) : red_pairs_.get();
  const int64_t n = src_offsets.empty() ? 0 : src_offsets.back();
  if (n > sb.n) throw std::invalid_argument("s_apply_csr: offsets beyond pull");
  mark_stale_buffer(sb, recv_keys, n);
  if (recv_cnt) {  // received entries: offsets by a scan of the counts
    csr_roff_.reserve(*be_, (size_t)n + 1, (size_t)(n + n / 4 + 1024));
    be_->scan_u32(recv_cnt, csr_roff_, nullptr, n);
    off = csr_roff_;
    cnt = recv_cnt;
    ent = recv_ent;
  }
  ApplyArgs base = apply_args(recv_keys, sb.slots, nullptr, 0, S);
  base.fm_compact = fm_vals_;
  base.csr_ew = csr_full_rows() ? csr_row_words(table_.L.P) : 0;
  base.csr_ent = ent;
  apply_by_source(base, src_offsets, buf, stash,
                  "s_apply_csr: compact FM rows of several sources need s_pull's weights",
                  [&](ApplyArgs& aa, int64_t o, int64_t c) {
                    // (entries normalised by the workers; entry indices are global)
                    aa.csr_off = off + o;
                    aa.csr_cnt = cnt + o;
                    aa.csr_long = S > 16 ? csr_long_list(c) : nullptr;
                    aa.csr_long_cap = (int64_t)csr_long_.capacity();
                  });
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

// the device arrays of push_host / pull_host: exactly n keys when they grow
void Engine::ensure_host_staging(int64_t n) {
  if (!host_keys_dev_.reserve(*be_, (size_t)n, (size_t)n)) return;  // (waited for the stream)
  host_vals_dev_.alloc(*be_, (size_t)n * cfg_.model.P());
  host_slots_dev_.alloc(*be_, (size_t)n);
}

void Engine::push_host(const std::vector<u64>& keys, const std::vector<float>& grads) {
  refuse_frozen("push");
  stale_stashes();  // the table changes: server stashes are stale
  const int64_t n = (int64_t)keys.size();
  const int P = cfg_.model.P();
  if ((int64_t)grads.size() != n * P) throw std::invalid_argument("push_host: grads != keys*P");
  if (n == 0) return;
  guard_inserts(n);
  ensure_host_staging(n);
  be_->copy_h2d(host_keys_dev_, keys.data(), sizeof(u64) * n);
  be_->copy_h2d(host_vals_dev_, grads.data(), sizeof(float) * n * P);
  delta_mark(host_keys_dev_, nullptr, n);
  // (no admission filter: explicit pushes insert regardless; no values read)
  be_->table_pull(pull_args(host_keys_dev_, nullptr, n, true, host_slots_dev_));
  // Pushes of one call are applied one key at a time in order; duplicate keys
  // inside one call are applied sequentially by separate launches.
  ApplyArgs aa = apply_args(host_keys_dev_, host_slots_dev_, nullptr, 1, 1);
  aa.pstride = P;  // (host rows are P wide, not padded to the kernels' latent width)
  for (int64_t i = 0; i < n; ++i) {
    aa.slots = host_slots_dev_ + i;
    aa.grads = host_vals_dev_ + i * P;
    be_->table_apply(aa);
  }
  be_->synchronize();
}

void Engine::prefill(int64_t n, uint64_t seed) {
  if (n > 0) guard_inserts(n);  // (may grow the table first)
  if (n < 0 || (uint64_t)n > table_.cap - table_.cap / 16)
    throw std::invalid_argument("prefill: at most 15/16 of the table's slots");
  stale_stashes();
  if (n > 0) delta_needs_full_ = true;  // (inserts that bypass marking)
  be_->table_prefill(table_, n, seed);
  be_->synchronize();
  (void)table_size();  // (re-bases the capacity monitor)
}

std::vector<float> Engine::pull_host(const std::vector<u64>& keys) {
  const int64_t n = (int64_t)keys.size();
  const int P = cfg_.model.P();
  std::vector<float> out((size_t)n * P);
  if (n == 0) return out;
  ensure_host_staging(n);
  be_->copy_h2d(host_keys_dev_, keys.data(), sizeof(u64) * n);
  PullArgs pa = pull_args(host_keys_dev_, nullptr, n, false, host_slots_dev_);
  pa.out_vals = host_vals_dev_;
  pa.pstride = P;  // (host rows: P wide, no compact FM value rows)
  be_->table_pull(pa);
  be_->copy_d2h(out.data(), host_vals_dev_, sizeof(float) * n * P);
  return out;
}

// ---------------------------------------------------------------------------
// multi-rank phases
// ---------------------------------------------------------------------------
void Engine::w_prepare(const BatchView& b, int world, int64_t* counts_out, u64* send_keys_out,
                       int wb, int64_t seq) {
  // (the partitioned dedup is the backend's only way to group keys by owner)
  if (be_->partitioned_dedup() && (world < 1 || world > kMaxParts))
    throw std::runtime_error("w_prepare: world size " + std::to_string(world) + " outside [1, " +
                             std::to_string(kMaxParts) + "]");
  if (world <= 1) seq = -1;  // (no exchange to check)
  use_worker_set(wb);
  if (slices_of(b) > cfg_.max_slices)
    throw std::invalid_argument("batch has more slices than max_slices");
  if (b.nnz == 0) {
    // nothing to send; a batch without rows (a rank out of data) sends -1
    // counts, which tell the receivers "no data from this source" (the loop
    // ends when every source says so, ShardedEngine.train_step)
    const int64_t c = b.rows == 0 ? -1 : 0;
    be_->fill_u64(reinterpret_cast<u64*>(counts_out), (u64)(seq >= 0 ? encode_count(c, seq) : c),
                  (size_t)(world > 0 ? world : 1));
    be_->memset(ws_->n_uniq, 0, sizeof(int64_t));
    ws_->inv_valid = false;
    ws_->send_map = ws_->uniq_pos;
    return;
  }
  if (be_->partitioned_dedup()) {
    // owner-partitioned scratch: the slot-ordered unique list is the send
    // order already; counts are range counts (one range at world 1).  ws_->inv
    // (slot -> send index) lets the LR backward write the send buffer directly.
    if (red_pairs_ && (cfg_.model.kind == kLR || fm_vals_ || csr_full_rows())) ensure_inv();
    dedup_(b, world, send_keys_out, true, world == 1 ? counts_out : nullptr);
    ws_->inv_valid = ws_->inv != nullptr;
    if (world > 1) be_->partition_counts(scratch_, block_counts_, ws_->n_uniq, counts_out, seq);
    ws_->send_map = ws_->uniq_pos;
    return;
  }
  dedup_(b);
  ws_->inv_valid = false;
  BucketArgs ba;
  ba.uniq_keys = uniq_keys_;
  ba.uniq_pos = ws_->uniq_pos;
  ba.n_dev = ws_->n_uniq;
  ba.n_max = b.nnz;
  ba.world = world;
  ba.counts = counts_out;
  ba.send_keys = send_keys_out;
  ba.send_pos = ws_->send_pos;
  ba.scratch = bucket_ws_;
  ba.seq = seq;
  be_->bucket(ba);
  ws_->send_map = ws_->send_pos;
  // (slice masks are built in w_forward_backward with the step's global S)
}

void Engine::ensure_server_capacity(int64_t n, int buf) {
  if (buf < 0 || buf >= kSrvBufs) throw std::invalid_argument("server buffer must be in [0, kSrvBufs)");
  SrvBuf& sb = srv_[buf];
  const size_t cap = (size_t)(n + n / 4 + 1024);
  if (n <= 0 || !sb.slots.reserve(*be_, (size_t)n, cap)) return;  // (waited for the stream)
  if (lr16_layout()) sb.nz.alloc(*be_, 2 * cap);
}

bool Engine::lr16_layout() const {
  const TableLayout& L = table_.L;
  return be_->is_gpu() && L.lr16();
}

void Engine::w_forward(const BatchView& b, const float* pulled, int64_t n_send, float* pctr,
                       int wb) {
  use_worker_set(wb);
  be_->scatter_rows(pulled, wpull_, ws_->send_map, nullptr, n_send, vstride_);
  be_->forward_backward(eval_fwd_args(b, pctr));
}

void Engine::s_pull(const u64* recv_keys, int64_t n, float* out_vals, bool insert, int buf,
                    const std::vector<int64_t>& src_offsets, bool keep_weights) {
  if (insert) refuse_frozen("s_pull(insert=True)");
  ensure_server_capacity(n, buf);
  SrvBuf& sb = srv_[buf];
  sb.n = n;
  sb.vals = out_vals;
  sb.w_valid = false;
  sb.grp = SrcGroups();
  // (kept until the buffer's s_apply: a table growth re-probes its slots)
  sb.keys = insert && n > 0 ? recv_keys : nullptr;
  if (n == 0) return;
  if (insert) {
    guard_inserts(n);
    group_entries(recv_keys, n, buf, src_offsets);
    // (delta checkpoints: the buffer's applies push these keys; one that runs
    // after a delta_clear marks them again, mark_stale_buffer)
    delta_mark(recv_keys, nullptr, n);
  }
  sb.delta_gen = insert ? delta_gen_ : ~0ull;
  PullArgs pa = pull_args(recv_keys, nullptr, n, insert, sb.slots);
  if (insert) pa.admit = admit_;
  pa.out_vals = out_vals;
  pa.pstride = pstride();
  pa.fm_vals = fm_vals_;
  // Compact FM value rows carry no per-parameter weights: an apply that runs
  // after other table updates (the staleness-k step), or source by source
  // because the owner grouping was skipped (world > kMaxGroupSources, or the
  // other buffers' registrations were dropped on an owner-scratch resize),
  // needs the weights the workers' gradients refer to.
  const int nsrc = (int)src_offsets.size() - 1;
  int active = 0;
  for (int s2 = 0; s2 < nsrc; ++s2) active += src_offsets[s2 + 1] > src_offsets[s2];
  if (fm_vals_ && insert && (keep_weights || (!sb.grp.oidx && active > 1))) {
    sb.w.reserve(*be_, (size_t)n * pstride(), (size_t)(n + n / 4 + 1024) * pstride());
    pa.out_w = sb.w;
    sb.w_valid = true;
  }
  pa.out_nz = sb.nz;
  sb.nz_fresh = sb.nz != nullptr;
  be_->table_pull(pa);
}

// Owner grouping of the received entries (several sources with keys this
// step, GPU backend): one registration per (key, source) in an owner scratch
// table, so that s_apply runs once over all sources.  The scratch keeps keys
// across steps and is cleared once the entries registered since the last
// clear (an upper bound of its keys) could exceed half of it; it is sized to
// 4x the step's entries, so the load stays below 0.75.
bool Engine::group_entries(const u64* recv_keys, int64_t n, int buf,
                           const std::vector<int64_t>& offs) {
  // (EngineConfig::owner_group: grouping is opt-in)
  const int nsrc = (int)offs.size() - 1;
  if (cfg_.owner_group != 1) return false;
  if (!be_->owner_grouping() || nsrc < 2 || nsrc > kMaxGroupSources) return false;
  if (offs.front() != 0 || offs.back() != n) throw std::invalid_argument("s_pull: source offsets");
  int active = 0;
  for (int s = 0; s < nsrc; ++s) {
    if (offs[s + 1] < offs[s]) throw std::invalid_argument("s_pull: source offsets");
    active += offs[s + 1] > offs[s];
  }
  if (active < 2) return false;  // one source: the per-source apply is one launch already
  const u64 want = next_pow2((uint64_t)n * 4);
  if (want > (1ull << 32)) throw std::invalid_argument("s_pull: too many received keys to group");
  if (want > own_keys_.capacity() || nsrc != own_nsrc_) {
    // (re)size: the other buffer's registrations are dropped with the arrays
    // (its apply then runs source by source)
    be_->synchronize();
    const u64 cap = want > own_keys_.capacity() ? want : own_keys_.capacity();
    for (SrvBuf& b : srv_) {
      b.own_idx.reset();
      b.grp = SrcGroups();
    }
    own_nsrc_ = nsrc;
    own_keys_.alloc(*be_, cap);
    be_->fill_u64(own_keys_, kEmptyKey, cap);
    own_fill_ = 0;
  }
  const u64 own_cap = own_keys_.capacity();
  SrvBuf& sb = srv_[buf];
  if (!sb.own_idx) sb.own_idx.alloc_zero(*be_, own_cap * (u64)own_nsrc_);  // epoch 0: never valid
  sb.own_pos.reserve(*be_, (size_t)n, (size_t)(n + n / 4 + 1024));
  if (own_fill_ + n > (int64_t)(own_cap / 2)) {
    be_->fill_u64(own_keys_, kEmptyKey, own_cap);
    own_fill_ = 0;
  }
  own_fill_ += n;
  if (++own_epoch_ == 0) own_epoch_ = 1;
  OwnerGroupArgs ga;
  ga.keys = recv_keys;
  ga.n = n;
  ga.okeys = own_keys_;
  ga.ocap = own_cap;
  ga.opos = sb.own_pos;
  ga.oidx = sb.own_idx;
  ga.g.nsrc = nsrc;
  ga.g.epoch = own_epoch_;
  for (int s = 0; s <= nsrc; ++s) ga.g.offs[s] = offs[s];
  ga.overflow = overflow_;
  be_->owner_group(ga);
  sb.grp = ga.g;
  sb.grp.opos = sb.own_pos;
  sb.grp.oidx = sb.own_idx;
  return true;
}

void Engine::w_forward_backward(const BatchView& b, const float* pulled, int64_t n_send,
                                float* grads_out, u32* masks_out, int S_global, int wb,
                                int group) {
  use_worker_set(wb);
  // All ranks of a step must agree on the gradient row width (S*pstride):
  // S_global (>= this batch's slices) lets a rank with a short or empty batch
  // emit the same layout; its extra slices carry no rows and no mask bits.
  const int St = S_global > 0 ? S_global : slices_of(b);
  if (St < slices_of(b) || St > cfg_.max_slices)
    throw std::invalid_argument("w_forward_backward: S_global out of range");
  const int ng = slice_groups(St);
  if (group < 0 || group >= ng) throw std::invalid_argument("w_forward_backward: slice group");
  if (ng > 1 && cfg_.sum_slices)
    throw std::invalid_argument("sum_slices: at most 32 slices per step (ordered pushes: any count)");
  // slice group `group` of the step: its rows, its slices (>= 2 when grouped)
  const u32* posk = ws_->pos;
  const BatchView bk = group_view(b, St, group, posk);
  const int S = group_slices(St, group);
  const int ps = pstride();
  const bool masks = S > 1 && !cfg_.sum_slices;
  const int32_t* srows = slice_rows_dev(b, St) + (int64_t)group * kSliceGroup;
  const bool direct = ws_->inv_valid && red_pairs_ && S == 1 &&
                      (cfg_.model.kind == kLR || fm_vals_) &&
                      (double)scratch_.cap * S * ps < 4294967295.0;
  // the direct path's send buffer is zeroed by the scatter; the pulled rows
  // are placed once per step (every group reads the same ones)
  if (group == 0)
    be_->scatter_rows(pulled, wpull_, ws_->send_map, nullptr, n_send, vstride_,
                      direct ? grads_out : nullptr, grad_width());
  FwdArgs fa = train_fwd_args(bk, posk, S);
  fa.agg_ok = (double)scratch_.cap * S * pstride() < 4294967295.0;
  if (masks && reduction_masks(false)) fa.red_masks = tmask_;
  else if (masks) be_->slice_masks(bk, posk, tmask_);
  fa.fm_compact = sharded_fm_compact() && fa.agg_ok;
  if (sharded_fm_compact() && !fa.fm_compact)
    throw std::logic_error("w_forward_backward: compact FM rows need the reduction path");
  if (direct) {
    if (!fa.red_pairs || !fa.agg_ok) throw std::logic_error("direct send path without reduction");
    // the bucket reduction writes the normalised send buffer (no gather)
    fa.red_out = grads_out;
    fa.red_inv = ws_->inv;
    fa.red_rows = srows;
    be_->forward_backward(fa);
    last_nsend_ = n_send;
    return;
  }
  be_->forward_backward(fa);
  GatherGradArgs ga;
  ga.grad = grad_;
  ga.grad_rw = grad_;
  ga.tmask = masks ? tmask_.get() : nullptr;
  ga.tmask_rw = masks ? tmask_.get() : nullptr;
  ga.map = ws_->send_map;
  ga.n_max = n_send;
  ga.S = S;
  ga.pstride = ps;
  ga.slice_rows = srows;
  ga.width = grad_width();
  ga.out = grads_out;
  ga.out_mask = masks ? masks_out : nullptr;
  be_->gather_grads(ga);
  last_nsend_ = n_send;
}

void Engine::s_apply(const u64* recv_keys, const float* recv_grads, const u32* recv_masks,
                     const std::vector<int64_t>& src_offsets, int S, int buf) {
  refuse_frozen("s_apply");
  if (buf < 0 || buf >= kSrvBufs) throw std::invalid_argument("server buffer must be in [0, kSrvBufs)");
  SrvBuf& sb = srv_[buf];
  sb.keys = nullptr;  // applied: no slot remap needed after a growth
  const int gw = grad_width();
  // (the grouped apply pushes every source of a key at once: its stash stays
  // valid; source by source only the first launch takes it, apply_by_source)
  bool stash = sb.nz_fresh;
  stale_stashes();
  mark_stale_buffer(sb, recv_keys, src_offsets.empty() ? 0 : src_offsets.back());
  ApplyArgs base = apply_args(recv_keys, sb.slots, nullptr, 0, S);
  base.grads = const_cast<float*>(recv_grads);
  base.masks = recv_masks;
  base.gstride = gw;
  base.fm_compact = sharded_fm_compact();
  base.sum_slices = cfg_.sum_slices;
  const SrcGroups& g = sb.grp;
  bool same = g.oidx && (int)src_offsets.size() == g.nsrc + 1;
  for (int s = 0; same && s <= g.nsrc; ++s) same = src_offsets[s] == g.offs[s];
  // (other offsets, e.g. one source at a time for a grouped-slice step: per source below)
  if (same) {
    const int64_t n = g.offs[g.nsrc];
    if (n > sb.n) throw std::invalid_argument("s_apply: offsets beyond pull");
    ApplyArgs aa = base;
    aa.n_host = n;
    aa.n_max = n;
    if (aa.fm_compact) aa.pulled = pulled_weights(buf, 0);
    if (stash) aa.nz_stash = sb.nz;
    aa.grp = g;
    attach_snapshot(aa);
    be_->table_apply(aa);
    return;
  }
  apply_by_source(base, src_offsets, buf, stash,
                  "s_apply: compact FM rows of several sources need the grouped "
                  "apply or s_pull(keep_weights)",
                  [&](ApplyArgs& aa, int64_t off, int64_t cnt) {
                    if (off + cnt > sb.n) throw std::invalid_argument("s_apply: offsets beyond pull");
                    aa.grads = base.grads + off * (int64_t)S * gw;
                    if (recv_masks) aa.masks = recv_masks + off;
                  });
}

// Per-parameter pre-step weights of buffer entries from `off` for the compact
// FM apply: full pulled rows, or the owner's kept weights, or none (the apply
// then takes the slot's current weights -- valid while no other update ran).
const float* Engine::pulled_weights(int buf, int64_t off) const {
  const SrvBuf& sb = srv_[buf];
  if (!fm_vals_) return sb.vals + off * (int64_t)pstride();
  if (sb.w_valid) return sb.w + off * (int64_t)pstride();
  return nullptr;
}

// The dedup scratch is epoch-stamped and persistent: nothing to release; the
// step's capacity snapshot is queued here.
void Engine::w_finish() { end_step(); }

// ---------------------------------------------------------------------------
// table capacity management
// ---------------------------------------------------------------------------

// Consume the recorded snapshots in order (each event completes after the
// older ones: one stream); wait_upto >= 0 waits for snapshots up to that
// sequence number.  A snapshot with an overflow flag raises: keys were
// dropped (table: no slot within the probe bound; dedup or owner scratch:
// full), so the run is invalid -- fail within monitor_lag steps, not at
// epoch end.
bool Engine::snap_ready(int64_t seq) const {
  const volatile unsigned long long* p = &snaps_[seq % kSnaps].word;
  const unsigned long long want = (unsigned long long)seq & ((1ull << (64 - kSnapSeqShift)) - 1);
  return (*p >> kSnapSeqShift) == want;
}

// The next snapshot rides on this apply launch (its first wave stores it):
// valid as long as no insert is queued between it and end_step.
template <typename Args>
void Engine::attach_snapshot_to(Args& a, int64_t n_max) {
  if (!be_->is_gpu() || monitor_disabled() || n_max <= 0) return;
  const int64_t seq = snap_seq_ + 1;
  if (seq - 1 - snap_seen_ >= kSnaps) poll_snapshots(seq - kSnaps);  // (ring slot reuse)
  a.snap = &snaps_[seq % kSnaps];
  a.snap_mon = mon_;
  a.snap_seq = (unsigned long long)seq;
  snap_carried_ = true;
}
void Engine::attach_snapshot(ApplyArgs& aa) { attach_snapshot_to(aa, aa.n_max); }
// (a reduction that applies, FwdArgs::red_apply_*: n_max = the batch's occurrences)
void Engine::attach_snapshot(FwdArgs& fa, int64_t n_max) { attach_snapshot_to(fa, n_max); }

void Engine::poll_snapshots(int64_t wait_upto) {
  while (snap_seen_ < snap_seq_) {
    const int64_t seq = snap_seen_ + 1;  // (sequence numbers start at 1)
    const int i = (int)(seq % kSnaps);
    if (!snap_ready(seq)) {
      if (seq > wait_upto) break;
      ++monitor_waits_;
      const auto t0 = std::chrono::steady_clock::now();
      for (int spin = 0; !snap_ready(seq); ++spin) {
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
        else std::this_thread::yield();
      }
      monitor_wait_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    const unsigned long long w = *reinterpret_cast<volatile unsigned long long*>(&snaps_[i].word);
    const int64_t size = (int64_t)(w & 0xFFFFFFFFull);
    const bool ovf0 = (w >> 32) & 1ull, ovf1 = (w >> 33) & 1ull, bad = (w >> 34) & 1ull;
    known_size_ = size;
    known_adds_ = snap_adds_[i];
    ++snap_seen_;
    if (bad && !ovf0 && !ovf1)
      throw std::runtime_error(
          "xflow: non-finite or out-of-range prediction / gradient sum (the model diverged); "
          "the step's values were clamped");
    if (ovf0 || ovf1) {
      char msg[320];
      std::snprintf(msg, sizeof(msg),
                    "xflow: %s overflow -- keys were dropped (table: %lld keys in %llu slots%s); "
                    "raise the capacity (table_log2_cap / max_log2_cap, max_nnz)",
                    ovf1 ? "parameter table" : "dedup/owner scratch", (long long)size,
                    (unsigned long long)table_.cap, cfg_.table_grow ? "" : ", growth disabled");
      throw std::runtime_error(msg);
    }
  }
}

// Close the next snapshot: it is the one an apply of this step carries, or
// a tiny kernel writes it now; its insert bound is everything queued so far.
void Engine::close_snapshot() {
  const int64_t seq = snap_seq_ + 1;
  if (!snap_carried_) {
    if (seq - 1 - snap_seen_ >= kSnaps) poll_snapshots(seq - kSnaps);  // (ring slot reuse)
    be_->snapshot(&snaps_[seq % kSnaps], mon_, (unsigned long long)seq);
  }
  snap_carried_ = false;
  snap_adds_[seq % kSnaps] = queued_adds_;
  snap_seq_ = seq;
}

void Engine::end_step() {
  if (monitor_disabled()) return;
  close_snapshot();
  // bounded run-ahead: the snapshot monitor_lag steps back must be in
  poll_snapshots(snap_seq_ - cfg_.monitor_lag);
}

// Before an inserting pull of n keys (at most n new): grow the table so that
// the growth schedule (EngineConfig::grow_start / grow_load) holds for an
// upper bound of its size -- the last snapshot's size plus every insert bound
// queued since.  No host sync: a split is queued device work (split_to).
void Engine::guard_inserts(int64_t n) {
  if (n <= 0) return;
  // an apply outside a step (e.g. a staleness-k flush) carried a snapshot:
  // close it before these inserts, which it does not include
  if (snap_carried_) close_snapshot();
  poll_snapshots(-1);
  if (cfg_.table_grow) {
    const double bound = (double)(known_size_ + (queued_adds_ - known_adds_) + n);
    const u64 N = table_.cap >> table_.seg_log2;
    const u64 want = segments_for(bound, cfg_.grow_start, cfg_.grow_load);
    if (want > N) {
      // paced: twice what the schedule asks for this call's n keys (and at
      // least ~64 MB of segments), so a schedule that fell behind catches up
      // over several calls instead of one burst -- unless the fullest
      // segments would pass kHardLoad
      const size_t seg_bytes = ((size_t)1 << table_.seg_log2) * table_.L.stride * sizeof(u32);
      const u64 before = segments_for(bound - (double)n, cfg_.grow_start, cfg_.grow_load);
      u64 pace = 2 * (want - (before < want ? before : want)) + 1;
      const u64 floor_pace = seg_bytes >= (64u << 20) ? 1 : (u64)((64u << 20) / seg_bytes);
      if (pace < floor_pace) pace = floor_pace;
      const double hl = cfg_.grow_load > kHardLoad ? cfg_.grow_load : kHardLoad;
      const u64 hard = segments_for(bound, hl, hl);
      u64 target = want < N + pace ? want : N + pace;
      if (hard > target) target = hard;
      split_to(target);
    }
  }
  queued_adds_ += n;
}

// Segments the schedule wants for `keys` keys: at level L with s segments
// split, a segment not yet split holds keys / 2^L (uniform hashing) at load
// u = keys / (2^L * G); the schedule splits 2^L * (u - grow_start) /
// (grow_load - grow_start) of them (all by u = grow_load, when the level is
// complete and u halves).  u0 == u1: the segments that keep every load <= u1
// (whole levels).  Capped at 2^max_log2_cap slots.
u64 Engine::segments_for(double keys, double u0, double u1) const {
  const int g = table_.seg_log2;
  const double G = (double)(1ull << g);
  u64 N = table_.cap >> g;
  while (N < max_segs_) {
    int L = 0;
    while ((2ull << L) <= N) ++L;
    const u64 P = 1ull << L, s = N - P;
    const double u = keys / ((double)P * G);
    if (u <= u0) break;
    u64 want = u >= u1 ? P : (u64)std::ceil((double)P * (u - u0) / (u1 - u0));  // (u0 < u < u1)
    if (want > P) want = P;
    if (want <= s) break;
    N = P + want;
  }
  return N < max_segs_ ? N : max_segs_;
}

// Split segments (level by level, in launches of at most 2^28 slots) until the
// table has nseg segments: commit the new segments' memory at the end of the
// range, clear them, split their source segments (Backend::table_split).
// Slots of the moved keys change: pulled-but-not-applied server buffers are
// looked up again, queued on the stream.
void Engine::split_to(u64 nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  const int g = table_.seg_log2;
  const u64 G = 1ull << g;
  const size_t seg_bytes = (size_t)G * table_.L.stride * sizeof(u32);
  const u64 per_launch = g >= 28 ? 1 : (1ull << (28 - g));
  if (nseg > max_segs_) nseg = max_segs_;
  bool grew = false;
  while ((table_.cap >> g) < nseg) {
    const u64 N = table_.cap >> g, P = 1ull << table_.level, s0 = table_.split;
    u64 k = nseg - N;
    if (k > P - s0) k = P - s0;
    if (k > per_launch) k = per_launch;
    const size_t bytes = (size_t)(N + k) * seg_bytes;
    const size_t have = be_->table_committed();
    if (bytes > have) {
      const size_t fr = be_->free_memory();
      // (a re-allocating backend needs the whole new table next to the old one)
      const size_t need = be_->table_in_place() ? bytes - have : bytes;
      if (fr < need + (size_t)(256u << 20)) {
        if (grew) break;  // (what fits was added; the inserts run at a higher load)
        char msg[256];
        std::snprintf(msg, sizeof(msg),
                      "xflow: table growth to %llu slots needs %.2f GB more, %.2f GB free on the device",
                      (unsigned long long)((N + k) << g), need / 1e9, fr / 1e9);
        throw std::runtime_error(msg);
      }
    }
    table_.words = static_cast<u32*>(be_->table_commit(table_.words, bytes));
    TableView fresh = table_;
    fresh.words = table_.words + (size_t)(N << g) * table_.L.stride;
    fresh.cap = k << g;
    be_->table_clear(fresh);
    table_.cap = (N + k) << g;
    table_.split = s0 + k;
    be_->table_split(table_, s0, k);
    if (table_.split == P) {
      ++table_.level;
      table_.split = 0;
    }
    table_bytes_ = (size_t)table_.cap * table_.L.stride * sizeof(u32);
    splits_ += (int64_t)k;
    grew = true;
  }
  if (grew) {
    ++growths_;
    remap_server_slots();
  }
  grow_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

size_t Engine::table_committed() const { return be_->table_committed(); }

// Explicit growth to at least 2^lg slots (normally automatic).
void Engine::grow_table(int lg) {
  if (lg > 31) throw std::invalid_argument("grow_table: at most 2^31 slots (32-bit slot indices)");
  if (lg < table_.seg_log2 || (1ull << lg) <= table_.cap) return;
  if (lg > max_log2_cap_) throw std::invalid_argument("grow_table: beyond max_log2_cap");
  poll_snapshots(-1);
  split_to((1ull << lg) >> table_.seg_log2);
}

// Slots of pulled-but-not-yet-applied server buffers point into the old
// table: look their keys up again (all present, no insert).
void Engine::remap_server_slots() {
  for (SrvBuf& sb : srv_) {
    if (!sb.keys || sb.n <= 0) continue;
    PullArgs pa = pull_args(sb.keys, nullptr, sb.n, false, sb.slots);
    pa.pstride = pstride();
    be_->table_pull(pa);
  }
}

// ---------------------------------------------------------------------------
LossStats Engine::read_stats(bool reset, int which) {
  if (which < 0 || which > 1) throw std::invalid_argument("read_stats: which must be 0 or 1");
  LossStats h;
  be_->copy_d2h(&h, stats_ + which, sizeof(h));
  if (reset) be_->memset(stats_ + which, 0, sizeof(LossStats));
  return h;
}

int64_t Engine::n_unique() {
  int64_t n = 0;
  be_->copy_d2h(&n, ws_->n_uniq, sizeof(n));
  return n;
}

int64_t Engine::table_size() {
  unsigned long long n = 0;
  be_->copy_d2h(&n, table_.size, sizeof(n));  // (stream-synchronising: every queued insert is in)
  known_size_ = (int64_t)n;
  known_adds_ = queued_adds_;
  return (int64_t)n;
}

// Drop every key that meets the pruning rule (slot_prunable, types.h).  Not
// part of a step: call it between steps (epoch ends, before a model ships).
// Slots of the staying keys change, so pulled-but-not-applied server buffers
// are looked up again: an entry whose key was dropped gets the absent slot and
// its push is skipped, like a not-admitted key's.  The admission filter is not
// touched.  Capacity is not given back: the point is a lower load, shorter
// chains and later growth.
int64_t Engine::prune(float max_n) {
  refuse_frozen("prune");
  if (std::isnan(max_n)) throw std::invalid_argument("prune: max_n must not be NaN");
  if (snap_carried_) close_snapshot();  // (as guard_inserts: it predates the prune)
  poll_snapshots(snap_seq_);
  if (!pruned_dev_) pruned_dev_.alloc_zero(*be_, 1);
  be_->table_prune(table_, cfg_.opt, max_n, pruned_dev_);
  unsigned long long total = 0;
  be_->copy_d2h(&total, pruned_dev_, sizeof(total));  // (synchronising)
  (void)table_size();  // (re-bases the capacity monitor)
  stale_stashes();
  remap_server_slots();
  const int64_t dropped = (int64_t)total - pruned_keys_;
  pruned_keys_ = (int64_t)total;
  if (dropped > 0) delta_needs_full_ = true;  // (a delta cannot say "this key left")
  return dropped;
}

std::vector<uint8_t> Engine::admit_counts(const std::vector<u64>& keys) {
  std::vector<uint8_t> out(keys.size(), 0);
  if (!admit_.counters) return out;
  for (size_t i = 0; i < keys.size(); ++i) {
    const AdmitPos p = admit_pos(sanitize_key(keys[i]), admit_.log2);
    uint8_t c0 = 0, c1 = 0;
    be_->copy_d2h(&c0, admit_.counters + p.c0, 1);  // (synchronising)
    be_->copy_d2h(&c1, admit_.counters + p.c1, 1);
    out[i] = c0 < c1 ? c0 : c1;
  }
  return out;
}

void Engine::admit_export(uint8_t* dst) {
  if (admit_.counters) be_->copy_d2h(dst, admit_.counters, admit_bytes());
}

void Engine::admit_import(const uint8_t* src) {
  if (!admit_.counters) throw std::runtime_error("admit_import: admission is off");
  be_->synchronize();
  be_->copy_h2d(admit_.counters, src, admit_bytes());
  be_->synchronize();
}

std::vector<u32> Engine::server_slots(int buf) {
  if (buf < 0 || buf >= kSrvBufs) throw std::invalid_argument("server buffer must be in [0, kSrvBufs)");
  const SrvBuf& sb = srv_[buf];
  std::vector<u32> out((size_t)(sb.n > 0 ? sb.n : 0));
  if (!out.empty()) be_->copy_d2h(out.data(), sb.slots, sizeof(u32) * out.size());
  return out;
}

int64_t Engine::scratch_capacity() {
  if (!scratch_.ctl) return (int64_t)scratch_.cap;
  unsigned long long c = 0;
  be_->copy_d2h(&c, scratch_.ctl, sizeof(c));
  return (int64_t)c;  // ctl[0]: the capacity the next batch is deduplicated with
}

int64_t Engine::batch_capacity() {
  if (!scratch_.ctl) return (int64_t)scratch_.cap;
  unsigned long long c = 0;
  be_->copy_d2h(&c, ws_->bcap, sizeof(c));
  return (int64_t)c;  // (FwdArgs::red_bcap: the allocation when the batch spilled)
}

ScratchStats Engine::scratch_stats() {
  ScratchStats s;
  unsigned long long claims = 0;
  be_->copy_d2h(&claims, scratch_.claims, sizeof(claims));
  s.occupancy = (int64_t)claims;
  s.capacity = (int64_t)scratch_.cap;
  if (scratch_.ctl) {
    unsigned long long c[kScratchCtlWords];
    be_->copy_d2h(c, scratch_.ctl, sizeof(c));
    s.capacity = (int64_t)c[0];
    s.rebuilds = (int64_t)c[6];
    s.carried = (int64_t)c[7];
  }
  return s;
}

bool Engine::overflowed() {
  u32 o[2] = {0, 0};
  be_->copy_d2h(o, overflow_, sizeof(o));
  return o[0] || o[1];
}

BatchView Engine::synth_batch(const SynthArgs& a0, int64_t slice_rows) {
  SynthArgs a = a0;
  if (a.rows > cfg_.max_rows || a.rows * a.fields > cfg_.max_nnz)
    throw std::invalid_argument("synth batch exceeds engine capacity");
  if (a.col_stride > 0 && (a.col_stride < a.rows || (!a0.keys && a.col_stride != a.rows)))
    throw std::invalid_argument("synth: col_stride must be >= rows (== rows for staging)");
  // caller-provided outputs (e.g. torch tensors) or the engine's staging buffers
  a.keys = a0.keys ? a0.keys : st_keys_;
  a.labels = a0.labels ? a0.labels : st_labels_;
  if (!a0.fgid) a.fgid = cfg_.model.kind == kMVM ? st_fgid_.get() : nullptr;
  be_->synth_batch(a);
  BatchView b;
  b.keys = a.keys;
  b.labels = a.labels;
  b.fgid = a.fgid;
  b.rows = a.rows;
  b.nnz = a.rows * a.fields;
  b.nnz_per_row = a.fields;
  b.slice_rows = slice_rows;
  b.col_stride = a.col_stride;
  return b;
}

BatchView Engine::stage_host_batch(const BatchView& h) {
  if (h.rows > cfg_.max_rows || h.nnz > cfg_.max_nnz)
    throw std::invalid_argument("host batch exceeds engine capacity");
  BatchView b = h;
  be_->copy_h2d(st_keys_, h.keys, sizeof(u64) * h.nnz);
  b.keys = st_keys_;
  if (h.row_ptr) {
    be_->copy_h2d(st_rowptr_, h.row_ptr, sizeof(int32_t) * (h.rows + 1));
    b.row_ptr = st_rowptr_;
  }
  if (h.fgid) {
    be_->copy_h2d(st_fgid_, h.fgid, sizeof(int32_t) * h.nnz);
    b.fgid = st_fgid_;
  }
  be_->copy_h2d(st_labels_, h.labels, sizeof(float) * h.rows);
  b.labels = st_labels_;
  return b;
}

BatchView Engine::stage_host_batch_async(const BatchView& h) {
  if (h.rows > cfg_.max_rows || h.nnz > cfg_.max_nnz)
    throw std::invalid_argument("host batch exceeds engine capacity");
  const int s = astage_next_;
  astage_next_ ^= 1;
  StageSet& d = aset_[s];
  if (!d.keys) {
    d.keys.alloc(*be_, cfg_.max_nnz);
    d.rowptr.alloc(*be_, cfg_.max_rows + 1);
    d.fgid.alloc(*be_, cfg_.max_nnz);
    d.labels.alloc(*be_, cfg_.max_rows);
  }
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t bk = sizeof(u64) * h.nnz, br = h.row_ptr ? sizeof(int32_t) * (h.rows + 1) : 0,
               bf = h.fgid ? sizeof(int32_t) * h.nnz : 0, bl = sizeof(float) * h.rows;
  const size_t ok = 0, orp = up(bk), of = orp + up(br), ol = of + up(bf);
  be_->stage_begin(s);
  char* pin = static_cast<char*>(be_->stage_pinned(s, ol + up(bl)));
  std::memcpy(pin + ok, h.keys, bk);
  if (br) std::memcpy(pin + orp, h.row_ptr, br);
  if (bf) std::memcpy(pin + of, h.fgid, bf);
  std::memcpy(pin + ol, h.labels, bl);
  be_->stage_copy(s, d.keys, ok, bk);
  if (br) be_->stage_copy(s, d.rowptr, orp, br);
  if (bf) be_->stage_copy(s, d.fgid, of, bf);
  be_->stage_copy(s, d.labels, ol, bl);
  be_->stage_commit(s);
  astage_last_ = s;
  BatchView b = h;
  b.keys = d.keys;
  b.row_ptr = h.row_ptr ? d.rowptr.get() : nullptr;
  b.fgid = h.fgid ? d.fgid.get() : nullptr;
  b.labels = d.labels;
  return b;
}

void Engine::stage_release() {
  if (astage_last_ >= 0) be_->stage_release(astage_last_);
}

// ---------------------------------------------------------------------------
// checkpoint
// ---------------------------------------------------------------------------
// Checkpoint transfers stream through two pinned staging buffers: a table of
// 1e9 LR keys is 16 GB of keys + state, and a pageable copy of it (plus the
// zero-fill of the destination) ran at ~2.6 GB/s (profiles/r3s3_table_ops.txt).
constexpr size_t kStageChunk = 64u << 20;

// host memcpy of one staged chunk, split over a few threads (a single thread
// copies well below the DMA rate)
static void par_copy(void* dst, const void* src, size_t bytes) {
  constexpr size_t kPiece = 8u << 20;
  const size_t parts = bytes / kPiece;
  if (parts < 2) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const size_t nt = parts < 8 ? parts : 8, per = (bytes + nt - 1) / nt;
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) {
    const size_t o = t * per;
    if (o >= bytes) break;
    const size_t n = bytes - o < per ? bytes - o : per;
    th.emplace_back([=] { std::memcpy((char*)dst + o, (const char*)src + o, n); });
  }
  std::memcpy(dst, src, per < bytes ? per : bytes);
  for (std::thread& x : th) x.join();
}

template <typename Sink>
void Engine::d2h_stream(const void* src, size_t bytes, Sink sink) {
  if (bytes == 0) return;
  for (auto& p : stage_io_) p.ensure(*be_, kStageChunk);
  const char* s = static_cast<const char*>(src);
  int cur = 0;
  be_->copy_d2h_async(stage_io_[0].get(), s, bytes < kStageChunk ? bytes : kStageChunk);
  be_->synchronize();
  for (size_t off = 0; off < bytes;) {
    const size_t len = bytes - off < kStageChunk ? bytes - off : kStageChunk;
    const size_t nxt = off + len;
    if (nxt < bytes)  // the next chunk's DMA runs while the host consumes this one
      be_->copy_d2h_async(stage_io_[cur ^ 1].get(), s + nxt,
                          bytes - nxt < kStageChunk ? bytes - nxt : kStageChunk);
    sink(stage_io_[cur].get(), off, len);
    be_->synchronize();
    off = nxt;
    cur ^= 1;
  }
}

template <typename Fill>
void Engine::h2d_stream(void* dst, size_t bytes, Fill fill) {
  if (bytes == 0) return;
  for (auto& p : stage_io_) p.ensure(*be_, kStageChunk);
  char* d = static_cast<char*>(dst);
  int cur = 0;
  for (size_t off = 0; off < bytes;) {
    const size_t len = bytes - off < kStageChunk ? bytes - off : kStageChunk;
    fill(stage_io_[cur].get(), off, len);  // overlaps the previous chunk's DMA
    be_->synchronize();              // (that DMA read the other buffer)
    be_->copy_h2d_async(d + off, stage_io_[cur].get(), len);
    off += len;
    cur ^= 1;
  }
  be_->synchronize();
}

void Engine::export_into(u64* keys, u32* words, int64_t n) {
  const int W = state_words();
  if (n != table_size()) throw std::invalid_argument("export_into: n must equal table_size()");
  if (n == 0) return;
  DeviceBuffer<u64> dk(*be_, n);
  DeviceBuffer<u32> dw(*be_, n * W);
  if (be_->table_export(table_, dk, dw, n) != n)
    throw std::runtime_error("export_table: live slot count mismatch");
  d2h_stream(dk, sizeof(u64) * n, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)keys + o, c, b);
  });
  d2h_stream(dw, sizeof(u32) * n * W, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)words + o, c, b);
  });
}

void Engine::export_table(std::vector<u64>& keys, std::vector<u32>& words) {
  const int64_t n = table_size();
  keys.resize((size_t)n);
  words.resize((size_t)n * state_words());
  export_into(keys.data(), words.data(), n);
}

// device arrays of n (key, state) pairs -> the table
void Engine::table_from_device(const u64* dk, const u32* dw, int64_t n) {
  delta_needs_full_ = true;  // (import_from / load: states set without marking)
  be_->table_import(table_, dk, dw, n);
  be_->synchronize();
  (void)table_size();  // (re-bases the capacity monitor)
}

void Engine::import_from(const u64* keys, const u32* words, int64_t n) {
  stale_stashes();  // the table changes: server stashes are stale
  const int W = state_words();
  if (n <= 0) return;
  guard_inserts(n);
  DeviceBuffer<u64> dk(*be_, n);
  DeviceBuffer<u32> dw(*be_, n * W);
  h2d_stream(dk, sizeof(u64) * n, [&](void* c, size_t o, size_t b) {
    par_copy(c, (const char*)keys + o, b);
  });
  h2d_stream(dw, sizeof(u32) * n * W, [&](void* c, size_t o, size_t b) {
    par_copy(c, (const char*)words + o, b);
  });
  table_from_device(dk, dw, n);
}

void Engine::import_table(const std::vector<u64>& keys, const std::vector<u32>& words) {
  const int64_t n = (int64_t)keys.size();
  if ((int64_t)words.size() != n * state_words())
    throw std::invalid_argument("import_table: size mismatch");
  import_from(keys.data(), words.data(), n);
}

// Shard file: the device export streams chunk by chunk from the staging
// buffers to the file (no whole-table host copy).
void Engine::save(const std::string& path) {
  refuse_frozen("save");
  const int W = state_words();
  const int64_t n = table_size();
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + path);
  bool ok = true;
  int32_t hdr[8] = {1, cfg_.model.kind, cfg_.model.v_dim, table_.L.P,
                    table_.L.p_w, table_.L.opt, table_.L.stride, 0};
  const uint64_t un = (uint64_t)n;
  ok = ok && std::fwrite(kMagic, 1, 8, f) == 8;
  ok = ok && std::fwrite(hdr, sizeof(hdr), 1, f) == 1;
  ok = ok && std::fwrite(&un, sizeof(un), 1, f) == 1;
  if (n > 0 && ok) {
    DeviceBuffer<u64> dk(*be_, n);
    DeviceBuffer<u32> dw(*be_, n * W);
    if (be_->table_export(table_, dk, dw, n) != n) {
      std::fclose(f);
      throw std::runtime_error("export_table: live slot count mismatch");
    }
    auto put = [&](const void* c, size_t, size_t b) {
      ok = ok && std::fwrite(c, 1, b, f) == b;
    };
    d2h_stream(dk, sizeof(u64) * n, put);
    d2h_stream(dw, sizeof(u32) * n * W, put);
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("write failed: " + path);
}

// ---------------------------------------------------------------------------
// delta checkpoints (EngineConfig::delta_track)
// ---------------------------------------------------------------------------
int64_t Engine::delta_count() {
  if (!delta_bits_) throw std::runtime_error("delta_count: delta tracking is off");
  return be_->table_export_marked(table_, delta_bits_, delta_log2_, nullptr, nullptr, 0);
}

int64_t Engine::delta_to_device(DeviceBuffer<u64>& dk, DeviceBuffer<u32>& dw) {
  const int64_t n = delta_count();
  if (n == 0) return 0;
  dk.alloc(*be_, (size_t)n);
  dw.alloc(*be_, (size_t)n * state_words());
  if (be_->table_export_marked(table_, delta_bits_, delta_log2_, dk, dw, n) != n)
    throw std::runtime_error("delta_export: marked key count changed between the passes");
  return n;
}

void Engine::delta_export(std::vector<u64>& keys, std::vector<u32>& words) {
  if (!delta_bits_) throw std::runtime_error("delta_export: delta tracking is off");
  const int W = state_words();
  DeviceBuffer<u64> dk;
  DeviceBuffer<u32> dw;
  const int64_t n = delta_to_device(dk, dw);
  keys.resize((size_t)n);
  words.resize((size_t)n * W);
  if (n == 0) return;
  d2h_stream(dk, sizeof(u64) * n, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)keys.data() + o, c, b);
  });
  d2h_stream(dw, sizeof(u32) * n * W, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)words.data() + o, c, b);
  });
}

// Engine::save's format with hdr[7] = 1; the device buffers hold the delta only.
void Engine::save_delta(const std::string& path) {
  refuse_frozen("save_delta");
  if (!delta_bits_) throw std::runtime_error("save_delta: delta tracking is off");
  const int W = state_words();
  DeviceBuffer<u64> dk;
  DeviceBuffer<u32> dw;
  const int64_t n = delta_to_device(dk, dw);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + path);
  int32_t hdr[8] = {1, cfg_.model.kind, cfg_.model.v_dim, table_.L.P,
                    table_.L.p_w, table_.L.opt, table_.L.stride, 1};
  const uint64_t un = (uint64_t)n;
  bool ok = std::fwrite(kMagic, 1, 8, f) == 8;
  ok = ok && std::fwrite(hdr, sizeof(hdr), 1, f) == 1;
  ok = ok && std::fwrite(&un, sizeof(un), 1, f) == 1;
  if (n > 0 && ok) {
    auto put = [&](const void* c, size_t, size_t b) {
      ok = ok && std::fwrite(c, 1, b, f) == b;
    };
    d2h_stream(dk, sizeof(u64) * n, put);
    d2h_stream(dw, sizeof(u32) * n * W, put);
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("write failed: " + path);
}

// ---------------------------------------------------------------------------
// serving snapshots
// ---------------------------------------------------------------------------
int64_t Engine::export_weights_count() {
  return be_->table_export_weights(table_, cfg_.opt, nullptr, nullptr, 0);
}

int64_t Engine::weights_to_device(DeviceBuffer<u64>& dk, DeviceBuffer<float>& dw) {
  const int64_t n = export_weights_count();
  if (n == 0) return 0;
  dk.alloc(*be_, (size_t)n);
  dw.alloc(*be_, (size_t)n * table_.L.P);
  if (be_->table_export_weights(table_, cfg_.opt, dk, dw, n) != n)
    throw std::runtime_error("export_weights: key count changed between the passes");
  return n;
}

void Engine::export_weights(std::vector<u64>& keys, std::vector<float>& weights) {
  const int P = table_.L.P;
  DeviceBuffer<u64> dk;
  DeviceBuffer<float> dw;
  const int64_t n = weights_to_device(dk, dw);
  keys.resize((size_t)n);
  weights.resize((size_t)n * P);
  if (n == 0) return;
  d2h_stream(dk, sizeof(u64) * n, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)keys.data() + o, c, b);
  });
  d2h_stream(dw, sizeof(float) * n * P, [&](const void* c, size_t o, size_t b) {
    par_copy((char*)weights.data() + o, c, b);
  });
}

int64_t Engine::save_serving(const std::string& path) {
  const int P = table_.L.P;
  DeviceBuffer<u64> dk;
  DeviceBuffer<float> dw;
  const uint64_t total = (uint64_t)table_size();
  const int64_t n = weights_to_device(dk, dw);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + path);
  const int32_t hdr[6] = {cfg_.model.kind, cfg_.model.v_dim, cfg_.model.fm_math,
                          cfg_.model.mvm_math, P,
                          frozen() ? cfg_.opt.frozen_from : cfg_.opt.kind};
  const uint64_t un = (uint64_t)n;
  bool ok = std::fwrite(kServingMagic, 1, 8, f) == 8;
  ok = ok && std::fwrite(hdr, sizeof(hdr), 1, f) == 1;
  ok = ok && std::fwrite(&total, sizeof(total), 1, f) == 1;
  ok = ok && std::fwrite(&un, sizeof(un), 1, f) == 1;
  if (n > 0 && ok) {
    auto put = [&](const void* c, size_t, size_t b) {
      ok = ok && std::fwrite(c, 1, b, f) == b;
    };
    d2h_stream(dk, sizeof(u64) * n, put);
    d2h_stream(dw, sizeof(float) * n * P, put);
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("write failed: " + path);
  return n;
}

void Engine::import_weights(const u64* keys, const float* weights, int64_t n) {
  if (!frozen())
    throw std::runtime_error("import_weights: only a frozen engine (a serving snapshot) "
                             "stores resolved weights");
  if (n <= 0) return;
  // (a frozen slot's state words: the P weights' bits, then the 16-byte padding)
  const int W = state_words(), P = table_.L.P;
  std::vector<u32> words((size_t)n * W, 0u);
  for (int64_t i = 0; i < n; ++i)
    std::memcpy(words.data() + (size_t)i * W, weights + (size_t)i * P, sizeof(float) * P);
  import_from(keys, words.data(), n);
}

void Engine::delta_clear() {
  delta_needs_full_ = false;
  if (!delta_bits_) return;
  be_->memset(delta_bits_, 0, sizeof(u32) * ((size_t)1 << (delta_log2_ - 5)));
  ++delta_gen_;
}

DeltaStats Engine::delta_stats() {
  DeltaStats s;
  if (!delta_bits_) return s;
  s.log2 = delta_log2_;
  s.bits_set = be_->delta_popcount(delta_bits_, delta_log2_);
  s.needs_full = delta_needs_full_;
  return s;
}

void Engine::load(const std::string& path) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  char magic[8];
  int32_t hdr[8];
  uint64_t n = 0;
  bool ok = std::fread(magic, 1, 8, f) == 8 && std::fread(hdr, sizeof(hdr), 1, f) == 1 &&
            std::fread(&n, sizeof(n), 1, f) == 1;
  if (!ok || std::memcmp(magic, kMagic, 8) != 0) {
    std::fclose(f);
    throw std::runtime_error("bad checkpoint " + path);
  }
  if (hdr[1] != cfg_.model.kind || hdr[3] != table_.L.P || hdr[5] != table_.L.opt ||
      hdr[6] != table_.L.stride) {
    std::fclose(f);
    throw std::runtime_error("checkpoint layout does not match this model/optimizer");
  }
  const int W = state_words();
  stale_stashes();
  if (n > 0) {
    guard_inserts((int64_t)n);
    DeviceBuffer<u64> dk(*be_, n);
    DeviceBuffer<u32> dw(*be_, n * W);
    auto get = [&](void* c, size_t, size_t b) { ok = ok && std::fread(c, 1, b, f) == b; };
    h2d_stream(dk, sizeof(u64) * n, get);
    h2d_stream(dw, sizeof(u32) * n * W, get);
    if (ok) table_from_device(dk, dw, (int64_t)n);
  }
  std::fclose(f);
  if (!ok) throw std::runtime_error("truncated checkpoint " + path);
}

}  // namespace xflow
