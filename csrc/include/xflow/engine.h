// xflow-amd: Engine — one rank's sparse CTR trainer state and step pipeline.
//
// A rank plays both ps-lite roles of the reference at once:
//   worker  (lr_worker.cc / fm_worker.cc / mvm_worker.cc): dedups a batch's
//           keys, forward/backward over its rows, produces per-(key, slice)
//           gradient sums;
//   server  (ftrl.h / sgd.h via server.h): owns a shard of the HBM hash table
//           and answers pulls / applies pushes for the keys it owns.
// Single-rank training fuses both (train_step); multi-rank training drives the
// phase methods from the distributed layer with sparse all-to-alls between
// them (xflow_amd/parallel/sparse_a2a.py).
#pragma once

#include <memory>
#include <utility>
#include <string>
#include <vector>

#include "xflow/backend.h"
#include "xflow/device_buffer.h"

namespace xflow {

struct EngineConfig {
  ModelSpec model;
  OptSpec opt;
  int table_log2_cap = 20;     // slots = 2^table_log2_cap (<= 2^31)
  int64_t max_rows = 1 << 16;  // per step
  int64_t max_nnz = 1 << 22;   // per step
  // slices per step (any count: a step of more than kSliceGroup slices runs
  // its slices in groups of kSliceGroup over one dedup + pull, see train_step)
  int max_slices = 1;
  bool sum_slices = false;     // apply Σ_s g_s once instead of ordered per-slice pushes
  double scratch_factor = 2.5;  // dedup scratch capacity = pow2 >= factor * max_nnz
  int device = -1;             // -1 => CPU backend, else HIP device ordinal
  // Table capacity management (the reference's store is an unbounded
  // unordered_map, ftrl.h:54-56,84).  Before every inserting pull the engine
  // bounds the table's size from below-lagging device snapshots plus the
  // inserts queued since (each at most the pull's key count), and grows the
  // table by segment splits (TableView, backend.h) on a schedule that keeps
  // the fullest segments' load <= grow_load: with u = the load of a segment
  // not yet split at this level, the first 2^level * (u - grow_start) /
  // (grow_load - grow_start) segments are split.  A split is stream-ordered
  // device work on one segment plus one new segment of memory -- no host
  // sync, no copy of the table -- up to 2^max_log2_cap slots.
  // table_grow = false keeps the capacity fixed: an insert that finds no slot
  // flags the overflow, and the next step start raises within monitor_lag
  // steps of it.
  bool table_grow = true;
  double grow_load = 0.8;
  double grow_start = 0.6;     // (< grow_load; else 3/4 of it)
  int max_log2_cap = 0;        // 0 => 31, and what the device's free memory allows
  // steps the host may run ahead of the device before it waits for a
  // snapshot (bounds both the growth bound's slack and fail-fast latency)
  int monitor_lag = 2;
  // Owner apply of a multi-source sharded step (GPU): 0 = one launch per
  // source in source order (default), 1 = one grouped launch (k_owner_group
  // registration + leader apply).  Per source measured faster for every
  // model in the emulated 8-GPU step (device us per rank-step, LR 617 vs
  // 687, FM-8 846 vs 893, MVM-10 1082 vs 1184:
  // profiles/r3s3_w8_owner_apply_ab.txt).
  int owner_group = 0;
  // Steps of several slices on the GPU for LR-FTRL / reference FM: CSR
  // gradients (one reduction and one apply of the touched (key, slice)
  // pairs, Engine::train_step_csr) -- else slice groups of kSliceGroup
  // (the same pushes, dense per-group buffers; also what a slice count the
  // CSR dests cannot address falls back to)
  bool csr = true;
  // Feature admission (McMahan et al. 2013, §4 "probabilistic feature
  // inclusion"; AdmitView, backend.h): a training pull inserts a key only
  // once a blocked counting filter in front of the table has seen it
  // admit_min_count times (1..255; 1 = off: every pull inserts, no filter
  // exists).  A sighting is one entry of an inserting training pull
  // (train_step: the step's unique keys; s_pull: every received entry) whose
  // key is not in the table.  Until then the key reads its absent weight and
  // its gradient is dropped.  Lookups (eval_step, pull_host, s_pull without
  // insert) neither count nor consult the filter; push_host, import and
  // prefill insert regardless of it.  admit_log2: log2 of the filter's bytes
  // (6..32), 0 = min(32, the table's largest log2 capacity + 1).  The filter
  // is allocated once and never grows.
  int admit_min_count = 1;
  int admit_log2 = 0;
  // The leader handoff (StepPlan::lead): on for the steps it
  // covers; false keeps the column-hashing k_lr everywhere (the A/B switch --
  // the results are bit-equal either way).
  bool lead_handoff = true;
  // Carry-over rebuilds of the GPU dedup scratch (ScratchView::carry, DESIGN
  // §3): a rebuild at an unchanged capacity keeps the batch's own keys.
  // false: every rebuild frees the whole table (the A/B switch -- the results
  // are bit-equal either way).
  bool scratch_carry = true;
  // Unique-order reduction outputs ranked from the dedup stamps
  // (StepPlan::red_rank) on the steps that covers; false keeps the
  // compaction's slot -> unique map everywhere (the A/B switch -- the results
  // are bit-equal either way).
  bool red_rank = true;
  // Bucket-sorted producer regions (StepPlan::red_local) on the
  // leader-handoff steps: the reduction runs without its scan and scatter
  // passes.  false keeps them everywhere (the A/B switch -- the results are
  // bit-equal either way).
  bool red_local = true;
  // FTRL applied inside the bucket reduction (StepPlan::red_apply)
  // on the bucket-sorted handoff steps with ranked outputs: the thread that
  // would store a key's normalised sum pushes it instead, so the step has no
  // unique-order gradient array and no apply launch.  false keeps both (the
  // A/B switch -- the results are bit-equal either way).
  bool red_apply = true;
  // Delta checkpoints (docs/DESIGN.md §2): a filter of 2^delta_log2 bits in
  // device memory, indexed by key hash (delta_bit, common.h), in which every
  // key whose state may have changed is marked -- by a launch of its own
  // behind every inserting pull (the fused step, s_pull(insert), push_host);
  // save_delta / delta_export write only the table's keys whose bit is set.
  // A collision can only add an untouched key; a touched key is never
  // missed.  Lookups never mark.  delta_log2: 10..34, 0 = min(34, the
  // table's largest log2 capacity + 2).  The filter is allocated once and
  // never grows.  false: no filter exists and no launch is added.
  bool delta_track = false;
  int delta_log2 = 0;
  // A frozen engine (OptSpec::kind == kFrozen: a serving snapshot)
  // scores batches with the model's one-launch lookup-and-score kernel
  // (Backend::serve_lr, Backend::serve_model) where the backend has one; false
  // -- or standard FM with fm_mfma -- runs eval_step's dedup -> pull -> forward
  // as on a training engine (the A/B switch).  Ignored by engines that are
  // not frozen.
  bool serve_fused = true;
  // ... except for batches of serve_unfused_lo <= rows < serve_unfused_hi,
  // which take the three-launch path (tests/test_serving_snapshot.py holds
  // the two paths to the same bits).  profiles/serve.txt (tools/serve_bench.py,
  // rows x 39 fields): the one-launch kernel is ahead at 1, 8, 16 and 32 rows
  // and from 256 rows up, and 6 % behind at 64 and 128 rows (0.0400 against
  // 0.0378 ms, 0.0418 against 0.0395) -- one or two waves walk their rows'
  // dependent probe rounds alone.  The window is [first size measured behind,
  // first size measured ahead again).  lo >= hi: always one launch.
  int64_t serve_unfused_lo = 64;
  int64_t serve_unfused_hi = 256;
  // The same window for FM and MVM (the LR window above was measured for LR
  // and holds for LR only); (0, 0): always one launch.  Negative (the
  // default): the model's own measured window -- the families differ badly
  // (profiles/serve.txt, FM-8 and MVM-10, rows x 39 fields):
  //   reference FM  [0, 512): its unfused path gathers compact 16-byte value
  //                 rows and is 7 to 24 % ahead up to 256 rows (0.0338 against
  //                 0.0363 ms at 1 row, 0.0441 against 0.0545 at 32), within
  //                 2 % at 512; the kernel is 30 % ahead at 1024 and 4096
  //                 rows and 16 % at 262144
  //   standard FM   [0, 0): the kernel is level at 32 rows and 2 to 28 %
  //                 ahead everywhere else
  //   MVM           every size: the kernel never won (0.0696 against 0.0458
  //                 ms at 1 row, 0.4531 against 0.3306 at 262144); it ships
  //                 for serve_unfused_rows_latent=(0, 0) and is off by default
  // Engine::serve_unfused_latent() reports the window in force.
  int64_t serve_unfused_latent_lo = -1;
  int64_t serve_unfused_latent_hi = -1;
};

// Engine::delta_stats
struct DeltaStats {
  int log2 = 0;            // log2 of the filter's bits (0: tracking off)
  int64_t bits_set = 0;    // popcount of the filter
  bool needs_full = false; // the table changed in a way a delta cannot carry
};

// The dedup scratch's counters (Engine::scratch_stats).  The CPU backend has
// a fixed capacity and counts no rebuilds: it reports its capacity and the
// keys claimed since its last clear.
struct ScratchStats {
  int64_t capacity = 0;   // active capacity (ScratchView::ctl[0])
  // the rebuild counter: occupied slots with carry-over, else the keys
  // claimed since the last rebuild
  int64_t occupancy = 0;
  int64_t rebuilds = 0;   // rebuilds the compaction decided (ctl[6])
  int64_t carried = 0;    // keys the last of them kept (ctl[7]; 0: a full clear)
};

// What the single-rank step's gradient layout depends on (Engine::step_inputs)
struct StepInputs {
  bool gpu = false;        // HIP backend
  bool remaps = false;     // Backend::remaps_positions (unique-index positions)
  bool red_pairs = false;  // the bucket reduction's buffers exist
  bool red_rowv = false;   // ... and its vector records (MVM)
  bool fm_vals = false;    // reference FM on value rows: compact (B, C) gradients
  bool csr = true;         // EngineConfig::csr
  bool sum_slices = false;
  int kind = kLR;  // ModelKind
  int fm_math = kFmReference;  // FmMath
  TableLayout L;
  double scratch_cap = 0.0, max_nnz = 0.0, max_rows = 0.0;
  int pstride = 1, slice_cap = 1;
  int kdim = 1;  // latent width of the kernels (ModelSpec::kernel_dim)
  // the leader handoff's inputs: the switch and the batch's shape (the only
  // per-batch inputs; Engine::plan(S) without a batch leaves rows at 0: off)
  bool lead_handoff = true;  // EngineConfig::lead_handoff
  bool field_major = false;  // fixed width, col_stride == rows
  double rows = 0.0, fields = 0.0;
  bool red_rank = true;  // EngineConfig::red_rank
  bool red_local = true;  // EngineConfig::red_local
  bool red_apply = true;  // EngineConfig::red_apply
};

// Where a step's gradients land, one per step:
//   kCsr        CSR entries of the touched (key, slice) pairs (S > 1, LR-FTRL 16-byte
//               slots, reference FM, or the full rows of standard FM and MVM): one
//               reduction, one chain apply
//   kUniqueLR   LR-FTRL normalised sums in unique order ([unique][slice] + slice bits)
//   kUniqueFmBC reference-FM normalised (B, C) in unique order
//   kUniqueRows full gradient rows in unique order (standard FM any S, MVM S = 1)
//   kSlotSums   LR-FTRL summed slices, slot-indexed (sum_slices)
//   kSlotRows   slot- or position-indexed rows the apply gathers and zeroes (CPU, fallbacks)
enum class GradPath : int { kCsr = 0, kUniqueLR, kUniqueFmBC, kUniqueRows, kSlotSums, kSlotRows };
const char* grad_path_name(GradPath g);

// The step's layout decisions, made once by plan_step (a pure function of
// StepInputs and S: unit-tested over the whole input space on the CPU) and
// only read by Engine::train_step.  Field meanings at their use there.
struct StepPlan {
  int S = 1, groups = 1, Sf = 1;  // slices, slice groups, slices per group
  int csr_slog2 = -1;             // kCsr: log2 of the padded slice count
  bool csr_rows = false;          // kCsr of full-row entries (standard FM, MVM)
  GradPath grad = GradPath::kSlotRows;
  bool masks = false;     // ordered per-slice pushes read slice bits
  bool upos = false;      // unique-index positions (Backend::remap_pos)
  bool lr16 = false;      // kUniqueLR
  bool lr16s = false;     // kSlotSums
  bool uqm = false;       // slice bits from the reduction
  bool fmu = false;       // kUniqueFmBC
  bool fm_keep_w = false; // the pull keeps per-parameter weights (grouped compact FM)
  bool mvmu = false, fsu = false, rowu = false;  // kUniqueRows (MVM, standard FM, either)
  bool grpst = false;     // the pull stashes (n, z) of multi-parameter FTRL keys
  bool uq = false;        // unique-order slice bits (S > 1 on a unique-order layout)
  // the leader handoff: the dedup writes leader-encoded positions
  // (DedupOut::lead) and k_lr_lead consumes them
  bool lead = false;
  // one-slice LR / reference FM on slot positions: k_red_sum ranks its
  // unique-order outputs from the stamps and the compaction's chunk offsets
  // (FwdArgs::red_rank_*), the compaction writes no slot -> unique map
  bool red_rank = false;
  // with lead: k_lr_lead writes its records sorted by bucket and the sums read
  // them in place (FwdArgs::red_local): no k_red_scan, no k_red_scatter
  bool red_local = false;
  // with red_local, red_rank and lr16 (one slice, one group, FTRL on 16-byte
  // slots, slot positions, ranked outputs): k_red_sum_local pushes each key's
  // sum itself (FwdArgs::red_apply_*): no lr_grad_, no table_apply
  bool red_apply = false;
};

StepPlan plan_step(const StepInputs& in, int S);

class Engine {
 public:
  explicit Engine(const EngineConfig& cfg);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  const EngineConfig& config() const { return cfg_; }
  Backend& backend() { return *be_; }
  bool is_gpu() const { return be_->is_gpu(); }
  void set_stream(void* s) { be_->set_stream(s); }
  void synchronize() { be_->synchronize(); }

  // ---- single-rank fused step -------------------------------------------
  // Batch pointers are backend memory (device pointers on the HIP backend).
  void train_step(const BatchView& b);
  // Forward only; pctr (backend memory, may be null) receives predictions.
  // Keys are looked up without insertion.
  void eval_step(const BatchView& b, float* pctr);

  // Push explicit gradients (host arrays) to keys, like the reference's
  // initialisation pushes (lr_worker.cc:180-182, fm_worker.cc:248-252).
  void push_host(const std::vector<u64>& keys, const std::vector<float>& grads);
  // Insert n synthetic keys no batch touches (Backend::table_prefill):
  // occupancy-realistic benchmarks of a long run's table.
  void prefill(int64_t n, uint64_t seed);
  // Backend::download_small on the engine's stream
  void download_small(void* host_dst, const void* src, size_t bytes) {
    be_->download_small(host_dst, src, bytes);
  }
  // Pull current values (host) of keys without inserting them.
  std::vector<float> pull_host(const std::vector<u64>& keys);

  // ---- multi-rank phases --------------------------------------------------
  // Worker phases take a worker buffer set wb (0/1): the dedup positions, send
  // map and counts of a prepared batch live there, so the next batch can be
  // prepared (deduplicated, counts exchanged) while the current one is still
  // in its forward/backward -- the pipelined sharded step.
  // worker: dedup the batch and group its unique keys by owner rank.
  // counts_out: backend int64[world]; send_keys_out: backend u64[>= n_unique].
  // seq (world > 1): the caller's prepare sequence number, carried in the
  // counts (encode_count) so that peers detect a rank that skipped a step.
  void w_prepare(const BatchView& b, int world, int64_t* counts_out, u64* send_keys_out,
                 int wb = 0, int64_t seq = -1);
  // server: probe/insert n received keys, write pulled rows (pstride floats)
  // into out_vals (backend memory), remember slots for s_apply.
  // buf selects one of two server slot buffers (pipelined steps alternate).
  // src_offsets (world+1 entries, optional): the sources' ranges of the
  // received keys; with several sources the GPU backend groups the entries by
  // key here so that s_apply is one launch.
  // keep_weights: also keep the per-parameter pulled weights for the apply
  // (needed when other updates reach the table between this pull and its
  // apply, i.e. the staleness-1 step, with compact FM value rows)
  void s_pull(const u64* recv_keys, int64_t n, float* out_vals, bool insert = true, int buf = 0,
              const std::vector<int64_t>& src_offsets = {}, bool keep_weights = false);
  // worker: forward only from pulled rows (sharded evaluation); pctr may be null.
  void w_forward(const BatchView& b, const float* pulled, int64_t n_send, float* pctr, int wb = 0);
  // worker: place pulled rows (in send order) into the pos-indexed buffer,
  // run forward/backward, then emit normalised gradients in send order.
  // grads_out: [n_send][S*pstride]; masks_out: [n_send] (used when S>1).
  // S_global > kSliceGroup: slice group `group` only (its rows, group_slices
  // slices: grads_out [n_send][group_slices*width]); every group reads the
  // same pulled rows, and the groups' pushes are applied in group order.
  void w_forward_backward(const BatchView& b, const float* pulled, int64_t n_send,
                          float* grads_out, u32* masks_out, int S_global = 0, int wb = 0,
                          int group = 0);
  // ---- the CSR exchange (several slices, GPU: LR-FTRL / reference FM) ----
  // log2 of the padded slice count when a step of S slices runs its gradients
  // as CSR entries (-1: the dense slice-group layout)
  int csr_slog2(int S) const { return plan(S).csr_slog2; }
  // the single-rank step's layout for S slices (plan_step on this engine)
  StepInputs step_inputs() const;
  StepPlan plan(int S) const { return plan_step(step_inputs(), S); }
  // ... for a batch of this shape (the leader handoff depends on it)
  StepPlan plan(int S, int64_t rows, int64_t fields, bool field_major) const {
    StepInputs in = step_inputs();
    in.rows = (double)rows;
    in.fields = (double)fields;
    in.field_major = field_major;
    return plan_step(in, S);
  }
  // bytes of one CSR entry: LR (slice | value) 8, reference FM (slice, B, C)
  // 12, standard FM a full row (csr_row_words)
  int csr_entry_bytes() const {
    return csr_full_rows() ? 4 * csr_row_words(table_.L.P) : (fm_vals_ ? 12 : 8);
  }
  bool csr_full_rows() const {
    return (cfg_.model.kind == kFM && cfg_.model.fm_math == kFmStandard) ||
           (cfg_.model.kind == kMVM && cfg_.model.kernel_dim() >= 2);
  }
  // worker: forward/backward of every slice of the step at once.  pack:
  // entries packed densely in send order into ent_out (cnt_out: entries per
  // key, u32 [n_send]; totals_out: entries per owner, from the step's owner
  // key counts `counts` (encoded: world > 1)); else they stay in the engine's
  // CSR layout (world 1, read in place by s_apply_csr with null arrays).
  void w_forward_backward_csr(const BatchView& b, const float* pulled, int64_t n_send,
                              int S_global, int wb, bool pack, u32* cnt_out, void* ent_out,
                              const int64_t* counts, int world, bool encoded, int64_t* totals_out);
  // server: apply received CSR gradients source by source: recv_cnt [n] per
  // key, entries of all sources back to back (null recv_cnt: the worker's own
  // entries of this step, world 1)
  void s_apply_csr(const u64* recv_keys, const u32* recv_cnt, const void* recv_ent,
                   const std::vector<int64_t>& src_offsets, int S, int buf = 0);
  // server: apply received gradients source by source (deterministic order).
  // src_offsets has world+1 entries delimiting each source's rows.
  void s_apply(const u64* recv_keys, const float* recv_grads, const u32* recv_masks,
               const std::vector<int64_t>& src_offsets, int S, int buf = 0);
  // worker: release the per-step dedup scratch.
  void w_finish();

  // AUC / logloss sums of n predictions in backend memory (labels 0/1 floats),
  // computed on the device: only the scalars come back (base.h:84-110)
  EvalMetrics eval_metrics(const float* pctr, const float* labels, int64_t n) {
    return be_->eval_metrics(pctr, labels, n);
  }
  // per-group AUC counts and calibration of n predictions split by groups[n]
  // (GroupedEval, backend.h); table: optional per-group sums in key order
  GroupedEval eval_grouped(const float* pctr, const float* labels, const u64* groups, int64_t n,
                           GroupTable* table = nullptr) {
    return be_->eval_grouped(pctr, labels, groups, n, table);
  }
  // out[r] = the key row r is grouped by for `field` (Backend::row_group_keys)
  void row_group_keys(const BatchView& b, int field, u64* out) {
    if (!b.fgid && b.row_ptr)
      throw std::invalid_argument("row_group_keys: a CSR batch needs its field ids (fgid)");
    be_->row_group_keys(b, field, out);
  }

  // Per-epoch row shuffling (Backend::shuffle_rows, ShuffleArgs): destination
  // row i of the outputs (backend memory) receives row shuffle_index(i, rows,
  // seed) of src, a CSR or fixed-width row-major batch within max_rows /
  // max_nnz; a field-major source is refused.  Fixed width: keys of key_bytes
  // 4 are zero-extended, field_major_out writes [F][rows] (row_ptr unused).
  // Queued on the engine's stream: no allocation after the first CSR call,
  // no host sync.
  void shuffle_rows(const BatchView& src, u64 seed, u64* keys, int32_t* fgid, float* labels,
                    int32_t* row_ptr, bool field_major_out, int key_bytes = 8);

  // Feature crosses (Backend::cross_rows, CrossArgs): every row of the source
  // gains a.spec.n cross keys.  rows and nnz + crosses * rows must lie within
  // max_rows / max_nnz (and int32).  Queued on the engine's stream: one
  // launch, no allocation, no host sync.
  void cross_rows(const CrossArgs& a);

  // ---- stats / introspection -------------------------------------------
  // which = 0: training forward passes, 1: eval_step passes.
  LossStats read_stats(bool reset, int which = 0);
  int64_t n_unique();            // unique keys of the last prepared batch (syncs)
  int64_t table_size();          // occupied slots (syncs)
  int64_t scratch_capacity();    // active dedup scratch capacity (adaptive on the GPU; syncs)
  // slots the last batch's compaction and reduction covered: the capacity it
  // was deduplicated with, or the whole allocation when it spilled (syncs)
  int64_t batch_capacity();
  ScratchStats scratch_stats();  // (syncs: tests and tools only)
  uint64_t table_capacity() const { return table_.cap; }
  size_t table_bytes() const { return table_bytes_; }
  bool overflowed();
  // capacity management (EngineConfig::table_grow): growths (split launches)
  // and segments split so far, host waits the monitor needed, and an explicit
  // growth to at least 2^log2_cap slots
  int64_t table_growths() const { return growths_; }
  // steps (fused or worker-side) whose several slices ran on the CSR path
  int64_t csr_steps() const { return csr_steps_; }
  // host copies of the last CSR step's per-key (off, cnt) and its entry words
  // (tests / debugging; syncs)
  void csr_debug(std::vector<u32>& off, std::vector<u32>& cnt, std::vector<u32>& words);
  // the unique keys of the last fused step, in unique order (which slot a key
  // gets is a CAS race, so the order is the step's own; tests; syncs)
  std::vector<u64> unique_keys();
  // the bucket geometry a CSR step of S slices has at the last batch's unique
  // count: RedGeom::shift / active on the host (tests assert the branch of
  // k_red_csr / k_red_csr_vec a case reaches; syncs)
  struct RedGeometry {
    int base = 0, shift = 0, buckets = 0, maxb = 0, nsub = 1, nb = 0;
    int64_t nuq = 0, needed = 0;
  };
  // (nuq < 0: the last batch's unique count)
  RedGeometry red_geometry(int S, int64_t nuq = -1);
  int64_t table_splits() const { return splits_; }
  // feature admission: the filter's bytes (0: off) and log2 of them, the
  // estimates min(c0, c1) of keys' sightings, the whole filter to / from
  // host memory of admit_bytes() bytes (checkpoints), and the slots a server
  // buffer's last s_pull recorded (tests / diagnostics).  All but the first
  // two sync.
  size_t admit_bytes() const { return admit_.counters ? (size_t)1 << admit_.log2 : 0; }
  int admit_log2() const { return admit_.counters ? admit_.log2 : 0; }
  std::vector<uint8_t> admit_counts(const std::vector<u64>& keys);
  void admit_export(uint8_t* dst);
  void admit_import(const uint8_t* src);
  std::vector<u32> server_slots(int buf);
  // geometry: {segment slots log2, level, split, segments}
  std::vector<int64_t> table_geometry() const {
    return {table_.seg_log2, table_.level, (int64_t)table_.split,
            (int64_t)(table_.cap >> table_.seg_log2)};
  }
  // device bytes committed to the table's range (>= table_bytes())
  size_t table_committed() const;
  // seconds of host time the growth calls took (mapping + launches)
  double grow_seconds() const { return grow_s_; }
  int64_t monitor_waits() const { return monitor_waits_; }
  // host seconds spent blocked on the monitor's run-ahead bound (the device
  // was monitor_lag steps behind): subtracted from the host's issue time
  double monitor_wait_seconds() const { return monitor_wait_s_; }
  // gradient-reduction records written by the producers since the last call
  // (counting on: one atomic per producer workgroup; off: -1).  Syncs.
  void count_records(bool on);
  int64_t take_records();
  void grow_table(int log2_cap);
  // Drop the keys whose weights are all exactly zero (slot_prunable, types.h:
  // with FTRL also every n <= max_n; max_n < 0: no bound) and re-pack the
  // keys that stay.  Returns the number dropped (syncs); pruned_keys() is the
  // running total.  Only LR is prediction-neutral: a dropped FM / MVM key
  // reads as never seen again (its latents take the lazy init).
  int64_t prune(float max_n = -1.0f);
  int64_t pruned_keys() const { return pruned_keys_; }
  // queue a snapshot of (table size, overflow flags) behind the step's
  // work; called at the end of every training step (fused or sharded)
  void end_step();
  // exactly non-zero (key, param) weights of this table shard (L1 sparsity)
  int64_t nonzero_weights() { return be_->table_nonzero(table_, cfg_.opt); }
  int pstride() const { return cfg_.model.pstride(); }
  // floats per pulled value row (pull outputs, the values exchange, the
  // forward's gather): pstride, or 4 for reference-math FM on the GPU
  // reduction path ((w, Σv, Σv^2, 0), FwdArgs::fm_vals)
  int value_width() const { return vstride_; }
  // floats per (key, slice) in the multi-rank gradient exchange: pstride, or
  // 2 for reference-math FM on the GPU reduction path ((B, C) rows, expanded
  // by the owner with the values it served)
  int grad_width() const { return sharded_fm_compact() ? 2 : pstride(); }
  int slices_of(const BatchView& b) const;
  // Hogwild slices beyond kSliceGroup per step (the reference's default is
  // hardware_concurrency threads per block, lr_worker.h:40-41): the step's
  // slices run in groups of kSliceGroup -- one dedup + pull for the whole
  // step (every slice reads the same weights), then per group a
  // forward/backward over the group's rows and an apply of its pushes in
  // slice order, so the pushes of all S slices are applied in global slice
  // order: the same semantics as one S-slice step.  A group of one slice
  // runs as two (masked path; the second slice has no rows).
  static constexpr int kSliceGroup = 32;
  static int slice_groups(int S) { return S <= kSliceGroup ? 1 : (S + kSliceGroup - 1) / kSliceGroup; }
  static int group_slices(int S, int group) {
    if (S <= kSliceGroup) return S;
    const int n = S - group * kSliceGroup;
    return n >= kSliceGroup ? kSliceGroup : (n < 2 ? 2 : n);
  }

  // ---- checkpoint ------------------------------------------------------
  // Host copies of every live slot: keys + (stride-2) state words each.
  void export_table(std::vector<u64>& keys, std::vector<u32>& words);
  void import_table(const std::vector<u64>& keys, const std::vector<u32>& words);
  // The same into / from caller memory of n keys and n * state_words()
  // words (n = table_size() for export), streamed through two pinned
  // staging buffers so the DMA of one chunk overlaps the host copy of the
  // previous one.
  void export_into(u64* keys, u32* words, int64_t n);
  void import_from(const u64* keys, const u32* words, int64_t n);
  int state_words() const { return table_.L.stride - 2; }
  const TableLayout& layout() const { return table_.L; }
  // Binary shard file: header + keys + state words.
  void save(const std::string& path);
  void load(const std::string& path);
  // ---- serving snapshots (docs/DESIGN.md §2) -----------------------------
  // The keys whose weights differ from what an absent key reads
  // (slot_exported, types.h) and their P resolved fp32 weights each: a count
  // pass, device buffers of exactly that size, then the export -- the peak
  // extra device memory is the snapshot, not the table.  Syncs.
  int64_t export_weights_count();
  void export_weights(std::vector<u64>& keys, std::vector<float>& weights);
  // The same as a file: magic "XFLOWSW1", int32 {model kind, v_dim, fm_math,
  // mvm_math, P, source optimiser kind}, u64 keys of this table, u64 n, keys
  // u64[n], weights f32[n][P].  Returns n.
  int64_t save_serving(const std::string& path);
  // Insert n (key, P weights) pairs into this frozen engine's table (the
  // import path with words = weight bits); throws on any other engine.
  void import_weights(const u64* keys, const float* weights, int64_t n);
  // this engine holds a serving snapshot: read-only, every training entry
  // point, prune and the training checkpoints throw
  bool frozen() const { return cfg_.opt.kind == kFrozen; }
  // The model's one-launch kernel is available and switched on
  // (EngineConfig::serve_fused; frozen, a backend that has it, not standard FM
  // with fm_mfma).  Which batch sizes eval_step gives it is the window's
  // business: serve_unfused_lo/hi for LR, serve_unfused_latent() for FM and
  // MVM.  With the default window a frozen MVM engine reports true here and
  // never launches k_serve_mvm, and reference FM launches k_serve_fm only
  // from 512 rows.
  bool serve_fused() const { return serve_lr_ || serve_model_; }
  // FM / MVM: batches of first <= rows < second take the unfused path
  std::pair<int64_t, int64_t> serve_unfused_latent() const {
    return {cfg_.serve_unfused_latent_lo, cfg_.serve_unfused_latent_hi};
  }
  // ---- serving deltas (docs/DESIGN.md §2) -----------------------------------
  // Producer, on a training engine with delta_track: (key, P resolved weights)
  // of every key of the table whose touched-key bit is set -- the keys that
  // now read as an absent key included (those entries are the deletions; no
  // flag marks them).  Count pass, device buffers of exactly that size, then
  // the export, as export_weights.  All three throw with tracking off and on a
  // frozen engine; none of them clears the filter.  Sync.
  int64_t serving_delta_count();
  void export_weights_delta(std::vector<u64>& keys, std::vector<float>& weights);
  // The same as a file: magic "XFLOWSD1", then save_serving's header fields
  // and arrays.  Returns n.
  int64_t save_serving_delta(const std::string& path);
  // Consumer, on a frozen engine only (throws elsewhere): upsert the n entries,
  // then sweep out every slot that reads as absent (Backend::frozen_upsert /
  // frozen_sweep).  Keys must be unique within one call after sanitize_key (a
  // slot then has one writer; the CPU backend checks it in the debug build).
  // Stream-ordered on the engine's stream: an eval_step queued before the call
  // sees the old model whole, one queued after it the new model whole.
  // Capacity first, before any launch: the table holds at most its size + n
  // keys afterwards; when that passes grow_load of the slots the table may
  // grow to (table_grow = false: of the slots it has) the call throws with the
  // table untouched, else the table grows by splits as before any insert.
  // Syncs (the counts come back).
  struct DeltaApplied {
    int64_t inserted = 0, overwritten = 0;  // entries whose key was new / present
    int64_t dropped = 0;         // slots the sweep freed
    int64_t segments_swept = 0;  // segments the sweep read
    double upsert_seconds = 0.0, sweep_seconds = 0.0;  // the two steps, each waited for
  };
  DeltaApplied apply_weights_delta(const u64* keys, const float* weights, int64_t n);
  // ---- delta checkpoints (EngineConfig::delta_track) ----------------------
  // The table's keys whose filter bit is set: their number (a count pass;
  // syncs), host copies of them and their state words (count pass, device
  // buffers of exactly that size, the staged transfer of export_into), and
  // the same as a shard file in save's format whose spare header word
  // hdr[7] = 1 marks a delta.  All three throw with tracking off.
  int64_t delta_count();
  void delta_export(std::vector<u64>& keys, std::vector<u32>& words);
  void save_delta(const std::string& path);
  // zero the filter and reset needs_full: the next delta holds what changes
  // from here on (no-op with tracking off)
  void delta_clear();
  // needs_full: set by what a delta cannot express or what bypasses marking
  // -- a prune that dropped a key, import_from / import_table / load, prefill
  DeltaStats delta_stats();
  // (the two host-side fields of delta_stats, without its popcount pass)
  int delta_log2() const { return delta_log2_; }
  bool delta_needs_full() const { return delta_bits_ && delta_needs_full_; }

  // libffm text block (backend memory, 16-byte aligned) -> CSR arrays in
  // backend memory, on the device (Backend::parse_text).  Returns {rows,
  // occurrences, shortest row, longest row, occurrences of the first rows -
  // rows % row_mod rows}; syncs once (the counts).  Throws when the block
  // holds more rows / occurrences than the arrays (max_rows / max_nnz).
  std::vector<int64_t> parse_text(const char* text, int64_t n, u64* keys, int32_t* fgid,
                                  int32_t* row_ptr, float* labels, int64_t max_rows,
                                  int64_t max_nnz, int64_t row_mod = 1);

  // Synthetic Criteo-shaped batch into engine-owned staging buffers.
  BatchView synth_batch(const SynthArgs& a, int64_t slice_rows);
  // Copy a host CSR batch into engine-owned staging buffers.
  BatchView stage_host_batch(const BatchView& host);
  // Asynchronous, double-buffered variant (the native trainer's input path):
  // the host arrays are copied into a pinned buffer and sent on the
  // backend's copy queue while earlier steps run; the compute queue waits
  // for them.  Call stage_release() after queueing the steps that read the
  // returned batch, before staging the batch after the next one.
  BatchView stage_host_batch_async(const BatchView& host);
  void stage_release();

 private:
  static const EngineConfig& validated(const EngineConfig& cfg);  // throws on a bad argument
  EngineConfig cfg_;
  std::unique_ptr<Backend> be_;  // first: every buffer below is destroyed before the backend
  TableView table_;
  // The table's address range (Backend::table_reserve; table_.words is its
  // base, which moves when a backend re-allocates on commit): released when
  // the engine -- or its constructor, throwing -- unwinds.
  struct TableRange {
    Engine* e = nullptr;
    ~TableRange() {
      if (e) e->be_->table_release(e->table_.words);
    }
  } table_range_;
  // (table_.size / overflow, admit_.counters and scratch_'s arrays alias the
  // owned buffers mon_, admit_counters_ and scratch_*_)
  AdmitView admit_;              // counters == null: admission off
  size_t table_bytes_ = 0;
  ScratchView scratch_;
  DeviceBuffer<unsigned char> admit_counters_;
  // delta checkpoints: the touched-key filter (null: tracking off)
  DeviceBuffer<u32> delta_bits_;
  int delta_log2_ = 0;
  bool delta_needs_full_ = false;
  uint64_t delta_gen_ = 0;  // delta_clear() calls so far
  // queue the marks of n keys (*n_dev when set) behind the stream's work
  void delta_mark(const u64* keys, const int64_t* n_dev, int64_t n) {
    if (delta_bits_) be_->delta_mark(delta_bits_, delta_log2_, keys, n_dev, n, n);
  }
  DeviceBuffer<u64> scratch_keys_;
  DeviceBuffer<unsigned char> scratch_stamps_;
  DeviceBuffer<unsigned long long> scratch_claims_, scratch_ctl_;

  // chunked device<->host transfer through the staging pair (export / save,
  // import / load): sink(host chunk, byte offset, bytes) consumes each chunk
  // while the next one is in flight; fill(host chunk, offset, bytes)
  // produces each chunk while the previous one uploads
  template <typename Sink>
  void d2h_stream(const void* src, size_t bytes, Sink sink);
  template <typename Fill>
  void h2d_stream(void* dst, size_t bytes, Fill fill);
  // engine_io.cpp: an export's (keys, values) on the device -- every live
  // slot, the delta's, the serving weights' (count pass, then buffers of
  // exactly that size) -- and its way to host memory or into a file behind a
  // header; import_from's and load's upload of n pairs, which differ in the fill
  struct Pairs;
  template <typename Pass>
  Pairs export_pairs(int64_t n, int width, const char* changed, Pass pass);
  Pairs full_to_device();
  Pairs delta_to_device();
  Pairs weights_to_device();
  Pairs weights_delta_to_device();
  void pairs_to_host(const Pairs& p, void* keys, void* vals);
  void pairs_to_file(const Pairs& p, const std::string& path, const void* hdr, size_t hbytes);
  template <typename Fill>
  bool import_pairs(int64_t n, Fill fill);
  DeviceBuffer<char, Mem::kStaging> stage_io_[2];
  void ensure_host_staging(int64_t n);  // push_host / pull_host device arrays of n keys
  void ensure_server_capacity(int64_t n, int buf = 0);
  // worker buffer sets (see w_prepare); ws_ is the current one
  struct WorkerSet {
    DeviceBuffer<u32> pos;        // [max_nnz]
    DeviceBuffer<u32> uniq_pos;   // [max_nnz]
    DeviceBuffer<u32> inv;        // [scratch cap] slot -> send index (partitioned dedup, LR)
    DeviceBuffer<int64_t> n_uniq;  // [1]
    DeviceBuffer<u32> send_pos;   // [max_nnz] (only without the partitioned dedup)
    const u32* send_map = nullptr;  // send order -> scratch slot (send_pos or uniq_pos)
    bool inv_valid = false;       // inv describes the batch of the last w_prepare
    DeviceBuffer<unsigned long long> bcap;  // scratch capacity of the set's batch (device)
  };
  WorkerSet wset_[2];
  WorkerSet* ws_ = &wset_[0];
  void use_worker_set(int wb);  // switches ws_; a set is allocated on first use
  // owner grouping for the one-launch multi-source apply (Backend::owner_group)
  DeviceBuffer<u64> own_keys_;   // owner scratch
  int64_t own_fill_ = 0;         // entries registered since the last clear (upper bound of keys)
  int own_nsrc_ = 0;             // row stride of SrvBuf::own_idx
  u32 own_epoch_ = 0;
  bool group_entries(const u64* recv_keys, int64_t n, int buf,
                     const std::vector<int64_t>& src_offsets);
  // per-slice normalisers, kSliceGroup entries per slice group (group k's
  // local slice s at [k * kSliceGroup + s])
  const int32_t* slice_rows_dev(const BatchView& b, int S);
  // rows of slice group k of a batch of S slices, and the matching dedup
  // positions (a row-range view: same layout, offset pointers)
  BatchView group_view(const BatchView& b, int S, int k, const u32*& pos) const;
  int slice_cap_ = 1;            // slices per group the buffers are sized for
  // parts > 1: owner-partitioned scratch (ScratchView::parts); uniq_keys_out
  // redirects the unique-key list (the sharded step's send buffer)
  void dedup_(const BatchView& b, int parts = 1, u64* uniq_keys_out = nullptr,
              bool want_inv = false, int64_t* n_copy = nullptr, bool lead = false);
  bool sharded_fm_compact() const {
    return red_pairs_ && cfg_.model.kind == kFM && cfg_.model.fm_math == kFmReference &&
           (double)scratch_.cap * slice_cap_ * pstride() < 4294967295.0;
  }
  bool fm_vals_ = false;
  int vstride_ = 1;
  bool serve_lr_ = false;  // frozen LR on a backend with serve_lr, serve_fused on
  // frozen FM / MVM on a backend with serve_model, serve_fused on (not
  // standard FM with fm_mfma: that forward sums a row in another association)
  bool serve_model_ = false;
  // throws "<what>: this engine holds a serving snapshot ..." when frozen
  void refuse_frozen(const char* what) const;
  const float* pulled_weights(int buf, int64_t off) const;

  // worker buffers (backend memory)
  DeviceBuffer<u64> uniq_keys_;    // [max_nnz]
  DeviceBuffer<u32> uniq_slot_;    // [max_nnz]
  DeviceBuffer<u32> block_counts_; // dedup compaction workspace
  DeviceBuffer<u32> mon_;          // [4]: table size (u64), overflow_ (below)
  u32* overflow_ = nullptr;        // [2]: scratch, table (= mon_ + 2)
  DeviceBuffer<float> wpull_;      // [scratch_cap * pstride]
  DeviceBuffer<float> grad_;       // [scratch_cap * slice_cap * pstride]
  DeviceBuffer<u32> tmask_;        // [scratch_cap]
  // HIP LR gradient reduction workspace (FwdArgs::red_*), null when unused
  DeviceBuffer<u64> red_pairs_;
  DeviceBuffer<u64> red_sorted_;
  DeviceBuffer<u32> red_hist_;
  DeviceBuffer<u32> red_tot_;
  DeviceBuffer<u32> red_count_;
  DeviceBuffer<float> red_rowv_;    // MVM: per-row loss*M (FwdArgs::red_rowv)
  DeviceBuffer<float> lr_grad_;     // LR-FTRL fused step: unique-order gradients [max_nnz][slice_cap]
  DeviceBuffer<float> lr_nz_;       // LR-FTRL fused step: pulled (n, z) [max_nnz][2]
  int64_t nnz_seen_ = 0;          // most occurrences in one batch (ScratchView::grow)
  DeviceBuffer<u32> lr_mask_;       // LR-FTRL fused step, S > 1: unique-order slice bits [max_nnz]
  DeviceBuffer<float> fm_grad_;     // reference FM fused step: unique-order (B, C) [max_nnz][2]
  DeviceBuffer<float> row_grad_;    // MVM / standard FM fused step (one slice): unique-order rows [max_nnz][pstride]
  DeviceBuffer<float> fm_w_;        // reference FM, grouped step: pulled per-parameter weights [max_nnz][pstride]
  int red_nb_ = 0;
  int red_nsub_ = 1;
  int red_maxb_ = 0;  // FwdArgs::red_maxb
  int red_groups_ = 0;  // FwdArgs::red_groups
  void set_reduction(FwdArgs& fa) const;
  // Kernel arguments are filled here and nowhere else: each builder sets what
  // every caller of its struct sets, a call site then adds only what is its
  // own.  Counts: *n_dev entries (at most n) when n_dev is set, else n.
  PullArgs pull_args(const u64* keys, const int64_t* n_dev, int64_t n, bool insert,
                     u32* out_slot) const;
  // (fm_D is read by compact-FM applies only)
  ApplyArgs apply_args(const u64* keys, const u32* slots, const int64_t* n_dev, int64_t n,
                       int S) const;
  // training forward/backward of S slices; calls set_reduction (once per forward)
  FwdArgs train_fwd_args(const BatchView& b, const u32* pos, int S) const;
  // forward only (eval_step, w_forward): eval stats, optional predictions
  FwdArgs eval_fwd_args(const BatchView& b, float* pctr) const;
  // The fused step's prologue: dedup (want_inv: with the slot -> unique index
  // map) -> unique-index positions (upos) -> growth guard; returns the
  // inserting pull over the unique keys for the caller to complete and launch.
  PullArgs begin_fused_step(const BatchView& b, bool want_inv, bool upos, bool lead = false);
  // The owner's per-source applies of server buffer buf: base (keys / slots at
  // entry 0) offset to every non-empty source of src_offsets in order, the
  // pull's (n, z) stash handed to the first launch only, compact FM rows of a
  // later source refused without kept weights (logic_error need_weights).
  // source(aa, first entry, entries) adds the source's own arguments.
  template <typename Source>
  void apply_by_source(const ApplyArgs& base, const std::vector<int64_t>& src_offsets, int buf,
                       bool stash, const char* need_weights, Source source);
  // CSR gradients (CsrOut): the single-rank step of several slices, LR-FTRL on
  // 16-byte slots or compact reference-FM rows -- one producer pass, one
  // reduction and one apply for any slice count
  DeviceBuffer<u32> csr_off_;      // [max_nnz]
  DeviceBuffer<u32> csr_cnt_;      // [max_nnz]
  DeviceBuffer<float> csr_vent_;   // standard FM / MVM: full-row entries [max_nnz][csr_row_words(P)]
  // MVM: repeated-field rows' records and fixed-point sums (MvmDup, backend.h)
  DeviceBuffer<float> mdup_rec_;
  DeviceBuffer<long long> mdup_acc_;
  DeviceBuffer<u32> mdup_claim_;
  int mdup_ew_ = 0;
  int64_t csr_steps_ = 0;
  void train_step_csr(const BatchView& b, int S, int slog2);
  DeviceBuffer<u32> csr_doff_;     // [max_nnz + 1] dense offsets (worker pack)
  StreamBuffer<u32> csr_long_;     // [1 + max keys] the applies' deferred long chains
  u32* csr_long_list(int64_t n);
  StreamBuffer<u32> csr_roff_;     // received entries' offsets (server)
  // the forward/backward both CSR entry points run: producer pass over every
  // slice with dests unique * 2^slog2 + slice, CSR reduction into csr_*_
  void csr_forward_backward(const BatchView& b, int slog2, const int32_t* srows, bool normalise);
  bool reduction_masks(bool unique_positions) const;
  void ensure_inv();
  DeviceBuffer<LossStats> stats_;  // [1]
  DeviceBuffer<int64_t> bucket_ws_;  // [2*256] (only without the partitioned dedup)
  DeviceBuffer<int32_t> slice_rows_;  // [kSliceGroup per slice group]
  int64_t cached_rows_ = -1, cached_slice_rows_ = -1;
  int cached_S_ = -1;
  int64_t last_nsend_ = 0;

  // async staging sets (stage_host_batch_async)
  struct StageSet {
    DeviceBuffer<u64> keys;
    DeviceBuffer<int32_t> rowptr;
    DeviceBuffer<int32_t> fgid;
    DeviceBuffer<float> labels;
  };
  StageSet aset_[2];
  int astage_next_ = 0, astage_last_ = -1;
  // staging batch buffers (backend memory)
  DeviceBuffer<u64> st_keys_;
  DeviceBuffer<int32_t> st_rowptr_;
  DeviceBuffer<int32_t> st_fgid_;
  DeviceBuffer<float> st_labels_;

  // Server buffers: a pipelined step with staleness k applies a buffer's
  // pushes after the next k pulls (parallel/async_p2p.py), so k + 1 are live.
 public:
  // (the asynchronous parameter server keeps one per (source, ring slot))
  static constexpr int kSrvBufs = 64;
 private:
  struct SrvBuf {
    DeviceBuffer<u32> slots;     // table slot of each received key (s_pull)
    int64_t n = 0;
    const u64* keys = nullptr;   // the received keys (slots re-probed after a table growth)
    // LR-FTRL 16-byte slots: (n, z) as pulled, and whether no apply has
    // touched the table since that pull (then the first source's apply takes
    // its state from here instead of re-reading the table)
    DeviceBuffer<float> nz;
    bool nz_fresh = false;
    const float* vals = nullptr;  // s_pull outputs (fm_compact apply)
    DeviceBuffer<float> w;        // s_pull(keep_weights) per-param weights
    bool w_valid = false;
    DeviceBuffer<u32> own_pos;    // owner grouping of the buffer's entries
    DeviceBuffer<u64> own_idx;
    SrcGroups grp;                // grp.oidx != null: s_pull grouped this buffer
    uint64_t delta_gen = 0;       // delta_gen_ when s_pull marked the buffer's keys
  };
  SrvBuf srv_[kSrvBufs];
  void stale_stashes() {
    for (SrvBuf& b : srv_) b.nz_fresh = false;
  }
  // Delta checkpoints: every apply follows an inserting s_pull of the same
  // keys into the same buffer, which marked them -- unless delta_clear ran in
  // between (a save between a pipelined step's pull and its apply) or the
  // pull did not insert: then the apply marks its n keys itself.
  void mark_stale_buffer(SrvBuf& sb, const u64* keys, int64_t n) {
    if (!delta_bits_ || sb.delta_gen == delta_gen_ || n <= 0) return;
    delta_mark(keys, nullptr, n < sb.n ? n : sb.n);
    sb.delta_gen = delta_gen_;
  }
  bool lr16_layout() const;

  // capacity monitor (EngineConfig::table_grow): a ring of pinned snapshots
  // (HostSnap: table size, overflow flags, sequence number), one per step,
  // written by the step's apply kernel (or a tiny kernel when the step has
  // none) and polled by the host -- no event, no extra launch; each comes
  // with the cumulative insert bound queued before it
  static constexpr int kSnaps = 64;
  HostBuffer<HostSnap> snaps_;      // pinned host [kSnaps]
  int64_t snap_adds_[kSnaps] = {};
  bool snap_carried_ = false;       // an apply since the last inserts carries the next snapshot
  bool snap_ready(int64_t seq) const;
  void close_snapshot();
  void attach_snapshot(ApplyArgs& aa);
  void attach_snapshot(FwdArgs& fa, int64_t n_max);
  template <typename Args>
  void attach_snapshot_to(Args& a, int64_t n_max);
  int64_t snap_seq_ = 0;            // snapshots recorded
  int64_t snap_seen_ = 0;           // snapshots consumed (all older ones complete)
  int64_t known_size_ = 0;          // table size at the last consumed snapshot (or sync)
  int64_t known_adds_ = 0;          // cumulative insert bound queued before it
  int64_t queued_adds_ = 0;         // cumulative insert bound queued so far
  int64_t growths_ = 0, splits_ = 0, monitor_waits_ = 0;
  DeviceBuffer<unsigned long long> pruned_dev_;  // [1] keys dropped by prune(), cumulative
  int64_t pruned_keys_ = 0;
  double grow_s_ = 0.0;
  u64 max_segs_ = 0;                // segments of 2^max_log2_cap slots
  double monitor_wait_s_ = 0.0;
  DeviceBuffer<float> grp_nz_;                   // FM / MVM FTRL: the pull's (n, z) stash [unique][P]
  DeviceBuffer<unsigned long long> rec_count_;  // (count_records) device counter
  DeviceBuffer<u32> red_vmax_;                   // MVM: per-step scale words [2], dup words [2]
  DeviceBuffer<u32> text_ws_;                    // parse_text workspace
  DeviceBuffer<long long> text_counts_;          // parse_text counts [7]
  DeviceBuffer<u32> shuf_len_;                   // shuffle_rows (CSR): the rows' lengths [max_rows + 1]
  mutable int vmax_parity_ = 0;
  bool rec_on_ = false;
  int log2_cap_ = 0, max_log2_cap_ = 31;
  void poll_snapshots(int64_t wait_upto);
  void guard_inserts(int64_t n);   // before an inserting pull of <= n new keys
  void remap_server_slots();
  // segment count the growth schedule (u0 = grow_start, u1 = grow_load) wants
  u64 segments_for(double keys, double u0, double u1) const;
  // load of the fullest segments at which growth stops pacing itself
  static constexpr double kHardLoad = 0.9;
  void split_to(u64 nseg);              // split segments until there are nseg

  DeviceBuffer<u64> host_keys_dev_;   // push_host / pull_host staging
  DeviceBuffer<float> host_vals_dev_;
  DeviceBuffer<u32> host_slots_dev_;
};

}  // namespace xflow
