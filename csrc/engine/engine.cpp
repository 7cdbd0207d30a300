// xflow-amd: Engine construction, host push / pull and the small accessors.
#include <cstring>

#include "engine_detail.h"
#include "xflow/engine.h"

namespace xflow {

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

}  // namespace xflow
