// xflow-amd: table capacity (monitor, segment splits, growth), prune and admission.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "xflow/engine.h"

namespace xflow {

// XFLOW_NO_MONITOR=1: no per-step capacity snapshot (A/B of the monitor's
// cost only; growth then relies on exact-size reads, overflow on the
// epoch-end check)
static bool monitor_disabled() {
  static const bool off = std::getenv("XFLOW_NO_MONITOR") != nullptr;
  return off;
}

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

}  // namespace xflow
