// xflow-amd: the multi-rank worker (w_*) and owner (s_*) phases of a sharded step.
#include "engine_detail.h"
#include "xflow/engine.h"

namespace xflow {

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

}  // namespace xflow
