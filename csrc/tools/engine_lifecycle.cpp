// xflow-amd: `engine_lifecycle` -- Engine construction, growth and destruction
// on the CPU backend, for the host sanitizers (scripts/sanitize_host.sh:
// AddressSanitizer + UBSan with leak detection).  It walks the paths that
// allocate, grow or free engine memory and destroys the engine after each
// group, so a buffer nobody owns shows up as a leak.  No data files.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "xflow/engine.h"

using namespace xflow;

namespace {

constexpr int64_t kRows = 128;
constexpr int kFields = 8;

EngineConfig config(int kind, int fm_math = kFmReference, int admit_min_count = 1) {
  EngineConfig c;
  c.model.kind = kind;
  c.model.v_dim = 4;
  c.model.fm_math = fm_math;
  c.table_log2_cap = 10;
  c.max_log2_cap = 14;
  c.max_rows = kRows;
  c.max_nnz = kRows * kFields;
  c.max_slices = 8;
  c.admit_min_count = admit_min_count;
  return c;
}

BatchView batch(Engine& e, int slices, uint64_t step) {
  static const std::vector<uint64_t> vocab(kFields, 500);
  static const std::vector<float> zipf(kFields, 1.1f);
  SynthArgs a;
  a.rows = kRows;
  a.fields = kFields;
  a.vocab = vocab.data();
  a.zipf_s = zipf.data();
  a.hash_space = 1 << 16;
  a.seed = 7;
  a.step = step;
  return e.synth_batch(a, kRows / slices);
}

void check(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(std::string("engine_lifecycle: ") + what);
}

// a constructor that rejects its arguments must leave nothing behind
void rejected(const EngineConfig& c, const char* what) {
  try {
    Engine e(c);
  } catch (const std::invalid_argument&) {
    return;
  }
  check(false, what);
}

// a few steps of 1 and of 8 slices, one evaluation
void train(const EngineConfig& c) {
  Engine e(c);
  for (uint64_t step = 0; step < 3; ++step) {
    e.train_step(batch(e, 1, step));
    e.train_step(batch(e, 8, step));
  }
  std::vector<float> pctr(kRows);
  e.eval_step(batch(e, 1, 9), pctr.data());
  check(e.table_size() > 0 && !e.overflowed(), "training left no keys");
}

// the second, larger call of each pair grows the host staging arrays / both server buffers
void growth() {
  Engine e(config(kLR));
  for (int n : {3, 300}) {
    std::vector<u64> keys(n);
    for (int i = 0; i < n; ++i) keys[i] = 1000 + 7 * (u64)i;
    e.push_host(keys, std::vector<float>(n, 0.5f));
    check((int)e.pull_host(keys).size() == n, "pull_host size");
  }
  for (int64_t n : {16, 700}) {
    std::vector<u64> keys(n);
    for (int64_t i = 0; i < n; ++i) keys[i] = 5000 + 3 * (u64)i;
    std::vector<float> vals(n * e.value_width()), grads(n * e.grad_width(), 0.25f);
    for (int buf = 0; buf < 2; ++buf) {
      e.s_pull(keys.data(), n, vals.data(), true, buf);
      e.s_apply(keys.data(), grads.data(), nullptr, {0, n}, 1, buf);
    }
  }
}

void worker_sets() {
  Engine e(config(kLR));
  std::vector<int64_t> counts(1);
  std::vector<u64> send(e.config().max_nnz);
  for (int wb : {0, 1, 0}) {
    e.w_prepare(batch(e, 1, wb), 1, counts.data(), send.data(), wb);
    check(e.n_unique() > 0, "w_prepare found no keys");
  }
}

void round_trip() {
  Engine a(config(kFM)), b(config(kFM));
  a.train_step(batch(a, 1, 0));
  std::vector<u64> keys;
  std::vector<u32> words;
  a.export_table(keys, words);
  b.import_table(keys, words);
  check(!keys.empty() && b.table_size() == a.table_size(), "table round trip");
}

// a prune round: prefilled (zero-state) keys leave, trained keys with a
// non-zero weight stay and keep their values; a pulled-but-unapplied server
// buffer is looked up again; the table keeps working afterwards
void prune_round(EngineConfig c) {
  // (MVM: latent values of order 1 keep the field products, and so the
  // gradients and weights, away from exactly 0)
  if (c.model.kind == kMVM) c.opt.v_init_scale = 1.0f;
  Engine e(c);
  e.prefill(300, 11);
  for (uint64_t step = 0; step < 3; ++step) e.train_step(batch(e, 1, step));
  std::vector<u64> keys;
  std::vector<u32> words;
  e.export_table(keys, words);
  const std::vector<float> before = e.pull_host(keys);
  const int64_t n0 = e.table_size();
  const int64_t n = 64;
  std::vector<u64> sk(n);
  for (int64_t i = 0; i < n; ++i) sk[i] = (1ull << 20) + 5 * (u64)i;  // (no batch key: hash_space 2^16)
  std::vector<float> vals(n * e.value_width()), grads(n * e.grad_width(), 0.25f);
  e.s_pull(sk.data(), n, vals.data(), true, 0);  // (inserted with zero state: they leave too)
  const int64_t dropped = e.prune(0.0f);
  check(dropped >= 300 && e.table_size() == n0 + n - dropped, "prune count");
  check(e.pruned_keys() == dropped && e.prune() >= 0, "prune total");
  e.s_apply(sk.data(), grads.data(), nullptr, {0, n}, 1, 0);
  check(!e.overflowed(), "prune overflowed");
  const int P = e.config().model.P();
  const std::vector<float> after = e.pull_host(keys);
  std::vector<u64> k2;
  e.export_table(k2, words);
  size_t kept = 0;
  for (size_t i = 0; i < keys.size(); ++i) {
    bool zero = true;
    for (int p = 0; p < P; ++p) zero = zero && before[i * P + p] == 0.0f;
    if (zero) continue;  // (may have left)
    ++kept;
    for (int p = 0; p < P; ++p) check(after[i * P + p] == before[i * P + p], "prune moved a value");
  }
  check(kept > 0 && k2.size() >= kept, "prune kept nothing");
  for (uint64_t step = 3; step < 5; ++step) e.train_step(batch(e, 8, step));
  check(e.table_size() > 0 && !e.overflowed(), "training after a prune");
}

}  // namespace

int main() {
  try {
    rejected(config(kLR, kFmReference, 0), "admit_min_count = 0 was accepted");
    EngineConfig bad = config(kLR, kFmReference, 2);
    bad.admit_log2 = 3;
    rejected(bad, "admit_log2 = 3 was accepted");
    train(config(kLR));
    train(config(kFM));
    train(config(kFM, kFmStandard));
    train(config(kMVM));
    train(config(kLR, kFmReference, 2));  // (with the admission filter)
    growth();
    worker_sets();
    round_trip();
    prune_round(config(kLR));
    prune_round(config(kFM));
    prune_round(config(kMVM));
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "%s\n", ex.what());
    return 1;
  }
  std::puts("engine_lifecycle: ok");
  return 0;
}
