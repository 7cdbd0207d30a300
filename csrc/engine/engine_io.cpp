// xflow-amd: checkpoints -- table export / import, the training shard file
// and its delta, serving snapshots.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "xflow/engine.h"

namespace xflow {

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

namespace {

constexpr char kMagic[8] = {'X', 'F', 'L', 'O', 'W', 'T', 'B', '1'};
constexpr char kServingMagic[8] = {'X', 'F', 'L', 'O', 'W', 'S', 'W', '1'};
constexpr char kServingDeltaMagic[8] = {'X', 'F', 'L', 'O', 'W', 'S', 'D', '1'};

// A training shard's first 48 bytes; u64 keys[n], u32 words[n][stride - 2] follow
struct ShardHeader {
  char magic[8];
  int32_t w[8];  // 1, model kind, v_dim, P, p_w, optimiser, slot stride, 1 for a delta
  uint64_t n;
};
static_assert(sizeof(ShardHeader) == 48, "no padding");
ShardHeader shard_header(const ModelSpec& m, const TableLayout& L, int64_t n, bool delta) {
  ShardHeader h = {{}, {1, m.kind, m.v_dim, L.P, L.p_w, L.opt, L.stride, delta}, (uint64_t)n};
  std::memcpy(h.magic, kMagic, 8);
  return h;
}

// A checkpoint file, closed on every way out: an export, an allocation or a
// backend copy may throw while it is open.
struct File {
  File(const std::string& path, const char* mode) : path(path), f(std::fopen(path.c_str(), mode)) {
    if (!f) throw std::runtime_error("cannot open " + path);
  }
  File(const File&) = delete;
  ~File() { if (f) std::fclose(f); }
  bool write(const void* p, size_t n) { return ok = ok && std::fwrite(p, 1, n, f) == n; }
  bool read(void* p, size_t n) { return ok = ok && std::fread(p, 1, n, f) == n; }
  void finish() {  // a writer's last call: the close can fail too
    ok = (std::fclose(std::exchange(f, nullptr)) == 0) && ok;
    if (!ok) throw std::runtime_error("write failed: " + path);
  }
  const std::string path;
  std::FILE* f;
  bool ok = true;  // every write / read so far was whole
};

}  // namespace

// An export on the device: n keys, vbytes of state words or f32 weight bits
struct Engine::Pairs {
  DeviceBuffer<u64> k;
  DeviceBuffer<u32> v;
  int64_t n = 0;
  size_t vbytes = 0;
};

// buffers of exactly n entries, then the export pass, which must find n again
template <typename Pass>
Engine::Pairs Engine::export_pairs(int64_t n, int width, const char* changed, Pass pass) {
  Pairs p;
  if (n == 0) return p;
  p.n = n;
  p.vbytes = sizeof(u32) * n * width;
  p.k.alloc(*be_, (size_t)n);
  p.v.alloc(*be_, (size_t)n * width);
  if (pass(p.k.get(), p.v.get()) != n) throw std::runtime_error(changed);
  return p;
}

Engine::Pairs Engine::full_to_device() {
  const int64_t n = table_size();
  return export_pairs(n, state_words(), "export_table: live slot count mismatch",
                      [&](u64* k, u32* v) { return be_->table_export(table_, k, v, n); });
}

void Engine::pairs_to_host(const Pairs& p, void* keys, void* vals) {
  auto to = [](void* d) {  // (the sink into host memory at d)
    return [d](const void* c, size_t o, size_t b) { par_copy((char*)d + o, c, b); };
  };
  d2h_stream(p.k, sizeof(u64) * p.n, to(keys));
  d2h_stream(p.v, p.vbytes, to(vals));
}

void Engine::pairs_to_file(const Pairs& p, const std::string& path, const void* hdr, size_t hbytes) {
  File f(path, "wb");
  f.write(hdr, hbytes);
  // (chunk by chunk from the staging buffers: no whole-table host copy)
  auto put = [&](const void* c, size_t, size_t b) { f.write(c, b); };
  d2h_stream(p.k, sizeof(u64) * p.n, put);
  d2h_stream(p.v, p.vbytes, put);
  f.finish();
}

void Engine::export_into(u64* keys, u32* words, int64_t n) {
  if (n != table_size()) throw std::invalid_argument("export_into: n must equal table_size()");
  pairs_to_host(full_to_device(), keys, words);
}

void Engine::export_table(std::vector<u64>& keys, std::vector<u32>& words) {
  const Pairs p = full_to_device();
  keys.resize((size_t)p.n);
  words.resize((size_t)p.n * state_words());
  pairs_to_host(p, keys.data(), words.data());
}

// n (key, state) pairs into the table: fill(words, chunk, byte offset, bytes)
// stages the key array (words = false), then the state words; false from it (a
// short file) leaves the table as it was, and is returned
template <typename Fill>
bool Engine::import_pairs(int64_t n, Fill fill) {
  stale_stashes();  // the table changes: server stashes are stale
  if (n <= 0) return true;
  guard_inserts(n);
  DeviceBuffer<u64> dk(*be_, n);
  DeviceBuffer<u32> dw(*be_, n * state_words());
  bool ok = true;
  h2d_stream(dk, sizeof(u64) * n, [&](void* c, size_t o, size_t b) { ok = ok && fill(false, c, o, b); });
  h2d_stream(dw, sizeof(u32) * n * state_words(),
             [&](void* c, size_t o, size_t b) { ok = ok && fill(true, c, o, b); });
  if (!ok) return false;
  delta_needs_full_ = true;  // (states set without marking)
  be_->table_import(table_, dk, dw, n);
  be_->synchronize();
  (void)table_size();  // (re-bases the capacity monitor)
  return true;
}

void Engine::import_from(const u64* keys, const u32* words, int64_t n) {
  import_pairs(n, [=](bool w, void* c, size_t o, size_t b) {
    par_copy(c, (w ? (const char*)words : (const char*)keys) + o, b);
    return true;
  });
}

void Engine::import_table(const std::vector<u64>& keys, const std::vector<u32>& words) {
  const int64_t n = (int64_t)keys.size();
  if ((int64_t)words.size() != n * state_words())
    throw std::invalid_argument("import_table: size mismatch");
  import_from(keys.data(), words.data(), n);
}

void Engine::save(const std::string& path) {
  refuse_frozen("save");
  const Pairs p = full_to_device();
  const ShardHeader h = shard_header(cfg_.model, table_.L, p.n, false);
  pairs_to_file(p, path, &h, sizeof(h));
}

void Engine::load(const std::string& path) {
  File f(path, "rb");
  ShardHeader h;
  const ShardHeader want = shard_header(cfg_.model, table_.L, 0, false);
  if (!f.read(&h, sizeof(h)) || std::memcmp(h.magic, want.magic, 8) != 0 ||
      h.n > (uint64_t)INT64_MAX)  // (a count no table holds)
    throw std::runtime_error("bad checkpoint " + path);
  for (int i : {1, 3, 5, 6})  // (model kind, P, optimiser, slot stride)
    if (h.w[i] != want.w[i])
      throw std::runtime_error("checkpoint layout does not match this model/optimizer");
  if (!import_pairs((int64_t)h.n, [&](bool, void* c, size_t, size_t b) { return f.read(c, b); }))
    throw std::runtime_error("truncated checkpoint " + path);
}

int64_t Engine::delta_count() {
  if (!delta_bits_) throw std::runtime_error("delta_count: delta tracking is off");
  return be_->table_export_marked(table_, delta_bits_, delta_log2_, nullptr, nullptr, 0);
}

Engine::Pairs Engine::delta_to_device() {
  const int64_t n = delta_count();
  return export_pairs(n, state_words(), "delta_export: marked key count changed between the passes",
                      [&](u64* k, u32* v) {
                        return be_->table_export_marked(table_, delta_bits_, delta_log2_, k, v, n);
                      });
}

void Engine::delta_export(std::vector<u64>& keys, std::vector<u32>& words) {
  if (!delta_bits_) throw std::runtime_error("delta_export: delta tracking is off");
  const Pairs p = delta_to_device();
  keys.resize((size_t)p.n);
  words.resize((size_t)p.n * state_words());
  pairs_to_host(p, keys.data(), words.data());
}

// Engine::save's format with hdr[7] = 1; the device buffers hold the delta only.
void Engine::save_delta(const std::string& path) {
  refuse_frozen("save_delta");
  if (!delta_bits_) throw std::runtime_error("save_delta: delta tracking is off");
  const Pairs p = delta_to_device();
  const ShardHeader h = shard_header(cfg_.model, table_.L, p.n, true);
  pairs_to_file(p, path, &h, sizeof(h));
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

int64_t Engine::export_weights_count() {
  return be_->table_export_weights(table_, cfg_.opt, nullptr, nullptr, 0);
}

Engine::Pairs Engine::weights_to_device() {
  const int64_t n = export_weights_count();
  return export_pairs(n, table_.L.P, "export_weights: key count changed between the passes",
                      [&](u64* k, u32* v) {
                        return be_->table_export_weights(table_, cfg_.opt, k, (float*)v, n);
                      });
}

void Engine::export_weights(std::vector<u64>& keys, std::vector<float>& weights) {
  const Pairs p = weights_to_device();
  keys.resize((size_t)p.n);
  weights.resize((size_t)p.n * table_.L.P);
  pairs_to_host(p, keys.data(), weights.data());
}

namespace {

// A serving file's first 48 bytes (a snapshot's or a delta's, by the magic);
// u64 keys[n], f32 weights[n][P] follow
struct ServingHeader {
  char magic[8];
  int32_t w[6];  // model kind, v_dim, fm_math, mvm_math, P, source optimiser
  uint64_t total, n;  // keys of the source table, entries of this file
};
static_assert(sizeof(ServingHeader) == 48, "no padding");
ServingHeader serving_header(const char* magic, const EngineConfig& c, int P, int64_t total,
                             int64_t n) {
  ServingHeader h = {{}, {c.model.kind, c.model.v_dim, c.model.fm_math, c.model.mvm_math, P,
                          c.opt.kind == kFrozen ? c.opt.frozen_from : c.opt.kind},
                     (uint64_t)total, (uint64_t)n};
  std::memcpy(h.magic, magic, 8);
  return h;
}

}  // namespace

int64_t Engine::save_serving(const std::string& path) {
  const int64_t total = table_size();
  const Pairs p = weights_to_device();
  const ServingHeader h = serving_header(kServingMagic, cfg_, table_.L.P, total, p.n);
  pairs_to_file(p, path, &h, sizeof(h));
  return p.n;
}

int64_t Engine::serving_delta_count() {
  refuse_frozen("serving_delta_count");
  if (!delta_bits_) throw std::runtime_error("serving_delta_count: delta tracking is off");
  return be_->table_export_weights_marked(table_, cfg_.opt, delta_bits_, delta_log2_, nullptr,
                                          nullptr, 0);
}

Engine::Pairs Engine::weights_delta_to_device() {
  const int64_t n = serving_delta_count();
  return export_pairs(n, table_.L.P,
                      "export_weights_delta: marked key count changed between the passes",
                      [&](u64* k, u32* v) {
                        return be_->table_export_weights_marked(table_, cfg_.opt, delta_bits_,
                                                                delta_log2_, k, (float*)v, n);
                      });
}

void Engine::export_weights_delta(std::vector<u64>& keys, std::vector<float>& weights) {
  refuse_frozen("export_weights_delta");
  if (!delta_bits_) throw std::runtime_error("export_weights_delta: delta tracking is off");
  const Pairs p = weights_delta_to_device();
  keys.resize((size_t)p.n);
  weights.resize((size_t)p.n * table_.L.P);
  pairs_to_host(p, keys.data(), weights.data());
}

int64_t Engine::save_serving_delta(const std::string& path) {
  refuse_frozen("save_serving_delta");
  if (!delta_bits_) throw std::runtime_error("save_serving_delta: delta tracking is off");
  const int64_t total = table_size();
  const Pairs p = weights_delta_to_device();
  const ServingHeader h = serving_header(kServingDeltaMagic, cfg_, table_.L.P, total, p.n);
  pairs_to_file(p, path, &h, sizeof(h));
  return p.n;
}

Engine::DeltaApplied Engine::apply_weights_delta(const u64* keys, const float* weights,
                                                 int64_t n) {
  if (!frozen())
    throw std::runtime_error("apply_weights_delta: only a frozen engine (a serving snapshot) "
                             "takes serving deltas");
  DeltaApplied r;
  if (n <= 0) return r;
  // capacity, before anything changes: every entry may be a new key
  const int64_t size0 = table_size();
  const double room = cfg_.grow_load * (double)(max_segs_ << table_.seg_log2);
  if ((double)size0 + (double)n > room) {
    char msg[320];
    std::snprintf(msg, sizeof(msg),
                  "apply_weights_delta: %lld keys + %lld entries would pass the load bound %.2f "
                  "of %llu slots%s; the table is unchanged",
                  (long long)size0, (long long)n, cfg_.grow_load,
                  (unsigned long long)(max_segs_ << table_.seg_log2),
                  cfg_.table_grow ? "" : " (growth disabled)");
    throw std::runtime_error(msg);
  }
  const int P = table_.L.P;
  DeviceBuffer<u64> dk(*be_, (size_t)n);
  DeviceBuffer<float> dw(*be_, (size_t)n * P);
  auto from = [](const void* s) {
    return [s](void* c, size_t o, size_t b) { par_copy(c, (const char*)s + o, b); };
  };
  h2d_stream(dk, sizeof(u64) * n, from(keys));
  h2d_stream(dw, sizeof(float) * n * P, from(weights));
  guard_inserts(n);  // (may split segments first)
  stale_stashes();   // the table changes: server stashes are stale
  const u64 nseg = table_.cap >> table_.seg_log2;
  DeviceBuffer<u32> dirty;
  dirty.alloc_zero(*be_, (size_t)nseg);
  DeviceBuffer<unsigned long long> stats;
  stats.alloc_zero(*be_, 3);
  using clock = std::chrono::steady_clock;
  be_->synchronize();
  const auto t0 = clock::now();
  be_->frozen_upsert(table_, cfg_.opt, dk, dw, n, dirty);
  be_->synchronize();
  const auto t1 = clock::now();
  be_->frozen_sweep(table_, cfg_.opt, dirty, stats);
  unsigned long long st[3] = {};
  be_->copy_d2h(st, stats, sizeof(st));  // (synchronising)
  r.sweep_seconds = std::chrono::duration<double>(clock::now() - t1).count();
  r.upsert_seconds = std::chrono::duration<double>(t1 - t0).count();
  const int64_t size1 = table_size();  // (re-bases the capacity monitor)
  // (slots of the staying keys changed; a frozen engine has no pulled-but-not-
  // applied server buffer to look up again: s_pull(insert) refuses it)
  r.dropped = (int64_t)st[0];
  r.segments_swept = (int64_t)st[1];
  r.inserted = size1 + r.dropped - size0;
  r.overwritten = n - r.inserted;
  if (overflowed())
    throw std::runtime_error("apply_weights_delta: an entry found no slot within the probe "
                             "bound -- the table dropped keys of this delta");
  return r;
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

}  // namespace xflow
