// xflow-amd: batches into backend memory -- parsed text, shuffles, crosses, synthetic and staged rows.
#include <cstring>

#include "xflow/engine.h"

namespace xflow {

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

}  // namespace xflow
