// xflow-amd: LR forward + backward (k_lr, k_lr_lead) and its dispatch (gfx950).
// Reference math: lr_worker.cc:121-143 (loss), :100-119 (gradient).
#include "model_common.h"

namespace xflow {
namespace hip {

// Backward of one column: exact LDS aggregation, then the LDS-only barrier
// and the flush of the table (global atomics left in flight, or pairs).
template <int LOG2>
__device__ __forceinline__ void lr_column(ColumnAgg<1, LOG2>& agg, int j, bool has, u32 dest,
                                          float loss, float* __restrict__ grad) {
  const int t = j & 1;
  if (has) agg.add(t, agg.insert(t, dest), 0, loss);
  lds_barrier();
  agg.flush(t, grad);
}

// LR: one lane per row, the sum order is the row's feature order (bitwise
// equal to the CPU backend).  BLOCK rows per workgroup: larger workgroups
// aggregate mid-frequency keys better (Criteo-shaped batch: 4.29 M global
// atomics at 256 rows, 2.95 M at 1024 rows, for 10.2 M occurrences).
template <bool kGrad, bool kAgg, int BLOCK, bool kRed = false>
__global__ void __launch_bounds__(BLOCK) k_lr(FwdArgs a) {
  XF_KT_DECL;
  constexpr int LOG2 = ilog2c(2 * BLOCK);
  // the reduction's column tables: 4 x BLOCK slots (a column's load <= 1/4:
  // short probe chains -- the insert is a chain of dependent LDS CASes, and
  // the barrier waits for the longest); the workgroup owns its CU anyway
  constexpr int LOG2R = ilog2c(4 * BLOCK);
  constexpr int C = kLrRegCols;
  constexpr bool kCol = kAgg && !kRed;  // column tables with global atomics
  __shared__ u32 s_tag[kCol ? 2 : 1][kCol ? (1 << LOG2) : 1];
  __shared__ float s_acc[kCol ? 2 : 1][kCol ? (1 << LOG2) : 1];
  __shared__ long long s_fx[kRed ? 2 : 1][kRed ? (1 << LOG2R) : 1];
  __shared__ int s_wmax[BLOCK / kWave];
  __shared__ u32 s_tag32[kRed ? 2 : 1][kRed ? (1 << LOG2R) : 1];
  __shared__ unsigned short s_list[kRed ? 2 : 1][kRed ? (1 << LOG2R) / 2 : 1];
  __shared__ u32 s_hist[kRed ? kRedMaxBuckets : 1];
  __shared__ u32 s_nlist[3];
  XF_DASSERT(!a.lead);  // (leader-encoded positions: k_lr_lead only)
  const BatchView& b = a.batch;
  const u32* __restrict__ pos = a.pos;
  const float* __restrict__ wp = a.wpull;
  int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool active = r < b.rows;
  RowSpan rs;
  if (active) rs = row_span(b, r);
  const int len = rs.len;
  // (the unused aggregator of an instantiation points at a 1-element array)
  ColumnAgg<1, LOG2> agg{reinterpret_cast<u32(*)[1 << LOG2]>(&s_tag[0][0]),
                         reinterpret_cast<float(*)[1 << LOG2]>(&s_acc[0][0])};
  if constexpr (kCol) agg.init();
  ListAgg<LOG2R> lagg{reinterpret_cast<u32(*)[1 << LOG2R]>(&s_tag32[0][0]),
                      reinterpret_cast<long long(*)[1 << LOG2R]>(&s_fx[0][0]),
                      reinterpret_cast<unsigned short(*)[(1 << LOG2R) / 2]>(&s_list[0][0]),
                     s_nlist, s_hist, nullptr};
  if constexpr (kRed) {
    // the workgroup's pair region starts at its first row's first occurrence
    // (published to the other waves by the barrier below)
    const int64_t r0 = (int64_t)blockIdx.x * BLOCK;
    lagg.region = a.red_pairs + (b.row_ptr ? (int64_t)b.row_ptr[r0] : r0 * b.nnz_per_row);
    lagg.init(red_active(a, red_shift(1)));
    lagg.shift = red_geom(a).shift(red_shift(1));
#ifdef XFLOW_KTIMING
    lagg.kt_acc_ = kt_acc_;
    lagg.kt_cur_ = &kt_;
#endif
  }
  // block-uniform longest row: selects the register path and bounds the
  // backward column walk
  int maxlen;
  if (!b.row_ptr) {
    maxlen = (int)b.nnz_per_row;
    if constexpr (kAgg) __syncthreads();
  } else {
    int m = wave_max(len);
    if (threadIdx.x % kWave == 0) s_wmax[threadIdx.x / kWave] = m;
    __syncthreads();
    maxlen = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / kWave; ++w) maxlen = max(maxlen, s_wmax[w]);
  }
  StatAcc st;
  float loss = 0.0f;
  const u32 s = active ? (u32)slice_of(b, r, a.S) : 0u;
  const u32 S = (u32)a.S;
  XF_KT(0);
  if (maxlen <= C) {
    u32 pv[C];
#pragma unroll
    for (int j = 0; j < C; ++j) pv[j] = j < len ? pos[rs.at(j)] : 0u;
    float wv[C];
#pragma unroll
    for (int j = 0; j < C; ++j) wv[j] = j < len ? wp[pv[j]] : 0.0f;
    if (active) {
      float wx = 0.0f;
#pragma unroll
      for (int j = 0; j < C; ++j)
        if (j < len) wx += wv[j];
      float p = sigmoid_ref(wx);
      float y = b.labels[r];
      loss = p - y;
      if (a.pctr) a.pctr[r] = p;
      st.add(p, y);
    }
    XF_KT(1);
    if constexpr (kGrad) {
      if constexpr (!kAgg) {
#pragma unroll
        for (int j = 0; j < C; ++j)
          if (j < len) atomicAdd(&a.grad[pv[j] * S + s], loss);
      } else {
#pragma unroll
        for (int j = 0; j < C; ++j) {
          if (j >= maxlen) continue;
          if constexpr (kRed) lagg.column(j, j < len && pv[j] != a.trash_pos, pv[j] * S + s, loss);
          else lr_column<LOG2>(agg, j, j < len, pv[j] * S + s, loss, a.grad);
        }
      }
    }
    XF_KT(2);
  } else {
    if (active) {
      float wx = 0.0f;
      int j = 0;
      for (; j + 4 <= len; j += 4) {
        u32 p0 = pos[rs.at(j)], p1 = pos[rs.at(j + 1)], p2 = pos[rs.at(j + 2)],
            p3 = pos[rs.at(j + 3)];
        float w0 = wp[p0], w1 = wp[p1], w2 = wp[p2], w3 = wp[p3];
        wx += w0;
        wx += w1;
        wx += w2;
        wx += w3;
      }
      for (; j < len; ++j) wx += wp[pos[rs.at(j)]];
      float p = sigmoid_ref(wx);
      float y = b.labels[r];
      loss = p - y;
      if (a.pctr) a.pctr[r] = p;
      st.add(p, y);
    }
    if constexpr (kGrad) {
      if constexpr (!kAgg) {
        for (int j = 0; j < len; ++j) atomicAdd(&a.grad[pos[rs.at(j)] * S + s], loss);
      } else {
        PosStream ps(pos, rs, len, a.trash_pos);
        for (int j0 = 0; j0 < maxlen; j0 += kPosChunk) {
          ps.prefetch(j0 + kPosChunk);
#pragma unroll
          for (int q = 0; q < kPosChunk; ++q) {
            const int j = j0 + q;
            if (j >= maxlen) break;
            const u32 pj = ps.get(q);
            const u32 dest = pj * S + s;
            if constexpr (kRed) lagg.column(j, pj != a.trash_pos, dest, loss);
            else lr_column<LOG2>(agg, j, j < len, dest, loss, a.grad);
          }
          ps.advance();
        }
      }
    }
  }
  if constexpr (kRed) {
    __syncthreads();
    if (threadIdx.x == 0) {
      a.red_count[blockIdx.x] = lagg.total();
      if (a.red_records) atomicAdd(a.red_records, (unsigned long long)lagg.total());
    }
    for (int i = threadIdx.x, n = red_active(a, red_shift(1)); i < n; i += BLOCK)
      a.red_hist[(size_t)i * gridDim.x + blockIdx.x] = s_hist[i];
  }
  st.bad |= lagg.bad;
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
  XF_KT(3);
  XF_KT_FLUSH();
}

// LR on leader-encoded positions (FwdArgs::lead): the dedup's tile -- one
// field of kLeadTile consecutive rows -- is this workgroup's column, and its
// grouping arrives in pos (a leader's slot, or kLeadBit | the leader's row in
// the tile), so no column is hashed a second time (no ListAgg).
//   forward   a leader gathers wpull[slot] and publishes the word in LDS at
//             its own row, kPosChunk columns per barrier (two buffers); a
//             follower reads its leader's word (same-address LDS reads
//             broadcast).  The row's sum order stays f = 0..F-1.
//   backward  a follower adds its fixed-point loss to acc[leader row] (two
//             buffers alternate, one LDS-only barrier per column); after the
//             barrier a leader adds its own, zeroes the entry and writes the
//             record (slot, sum) exactly as ListAgg's claimer does, so the
//             workgroup's region holds the same record set in another order.
// Rows of at most kLrRegCols features, S = 1, every row of the grid live.
//
// kLocal (FwdArgs::red_local): the region is written sorted by bucket, so the
// reduction needs neither k_red_scan nor k_red_scatter (k_red_sum_local reads
// the (workgroup, bucket) segments in place).  Every leader's slot is in pv
// before the forward's first use of a gathered weight, so the leaders are
// counted per bucket under that latency; a scan of the counts gives each
// bucket's first record of the region, and in the backward a leader takes its
// record index from its bucket's cursor (a returning LDS add before the
// column's barrier) instead of the workgroup's running count.  The tail writes
// start << 16 | count per bucket to red_hist (lead_seg).  The record set is
// what the other form writes; their order inside a segment is a race, as their
// order in the region already was.
template <bool kLocal>
__global__ void __launch_bounds__(kLeadTile) k_lr_lead(FwdArgs a) {
  XF_KT_DECL;
  constexpr int BLOCK = kLeadTile;
  constexpr int C = kLrRegCols;
  constexpr int Q = kPosChunk;
  constexpr int kFx = FxBits<1>::kFx;
  constexpr u32 kIdx = (u32)BLOCK - 1u;
  __shared__ float s_w[2][Q][BLOCK];
  __shared__ long long s_acc[2][BLOCK];
  __shared__ u32 s_hist[kRedMaxBuckets];
  __shared__ u32 s_cur[kLocal ? kRedMaxBuckets : 1];  // (kLocal) next record of each bucket
  __shared__ u32 s_n;
  static_assert(kRedMaxBuckets % BLOCK == 0, "the cursor scan: whole lanes");
  const BatchView& b = a.batch;
  const u32* __restrict__ pos = a.pos;
  const float* __restrict__ wp = a.wpull;
  const int t = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * BLOCK + t;
  XF_DASSERT(a.lead && a.S == 1 && r < b.rows && b.col_stride == b.rows && !b.row_ptr);
  const int len = (int)b.nnz_per_row;
  XF_DASSERT(len <= C);
  u64* __restrict__ region = a.red_pairs + (int64_t)blockIdx.x * BLOCK * len;
  const int nb = red_active(a, red_shift(1));
  const int shift = red_geom(a).shift(red_shift(1));
  s_acc[0][t] = 0ll;
  s_acc[1][t] = 0ll;
  for (int i = t; i < nb; i += BLOCK) s_hist[i] = 0u;
  if (t == 0) s_n = 0u;
  if constexpr (kLocal) lds_barrier();  // (s_hist is zero before the first count below)
  XF_KT(0);
  // every position load, then every leader's gather, in flight at once
  u32 pv[C];
#pragma unroll
  for (int j = 0; j < C; ++j) pv[j] = j < len ? pos[(int64_t)j * b.col_stride + r] : kLeadBit;
  float wv[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    XF_DASSERT((pv[j] & kLeadBit) || pv[j] <= a.trash_pos);
    wv[j] = pv[j] & kLeadBit ? 0.0f : wp[pv[j]];
  }
  if constexpr (kLocal) {
    // the emitting leaders per bucket, counted while the gathers are in flight
    // (a column past the row's length holds kLeadBit)
#pragma unroll
    for (int j = 0; j < C; ++j)
      if (!(pv[j] & kLeadBit) && pv[j] != a.trash_pos) {
        XF_DASSERT((int)(pv[j] >> shift) < nb);
        atomicAdd(&s_hist[pv[j] >> shift], 1u);
      }
  }
#pragma unroll
  for (int j0 = 0; j0 < C; j0 += Q) {
    if (j0 >= len) continue;  // (block-uniform)
    const int buf = (j0 / Q) & 1;
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (j0 + q < len && !(pv[j0 + q] & kLeadBit)) s_w[buf][q][t] = wv[j0 + q];
    // (buffer buf is written again two chunks on, after the next barrier:
    // every read of this chunk is before that barrier)
    lds_barrier();
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (j0 + q < len && (pv[j0 + q] & kLeadBit)) wv[j0 + q] = s_w[buf][q][pv[j0 + q] & kIdx];
  }
  u32 nrec = 0;  // (kLocal) the workgroup's records
  if constexpr (kLocal) {
    // the counts are complete (the forward has had a barrier): each bucket's
    // first record index, lane t scanning buckets [kPer t, kPer t + kPer)
    constexpr int kPer = kRedMaxBuckets / BLOCK;
    u32 c[kPer], sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      c[q] = kPer * t + q < nb ? s_hist[kPer * t + q] : 0u;
      sum += c[q];
    }
    u32 ex = block_exclusive_scan<BLOCK>(sum, &nrec);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      if (kPer * t + q < nb) s_cur[kPer * t + q] = ex;
      ex += c[q];
    }
    XF_DASSERT(nrec <= (u32)BLOCK * (u32)len);
  }
  StatAcc st;
  float wx = 0.0f;
#pragma unroll
  for (int j = 0; j < C; ++j)
    if (j < len) wx += wv[j];
  const float p = sigmoid_ref(wx);
  const float y = b.labels[r];
  const float loss = p - y;
  if (a.pctr) a.pctr[r] = p;
  st.add(p, y);
  XF_KT(1);
  u32 bad = 0;
  const long long v = fx_from<kFx>(fx_clamp<kFx>(loss, bad));
  // (the init's s_acc / s_hist / s_n stores are ordered by the forward's barrier)
  if constexpr (kLocal) lds_barrier();  // (the cursors, before the first column takes one)
#pragma unroll
  for (int j = 0; j < C; ++j) {
    if (j >= len) continue;  // (block-uniform)
    const int tb = j & 1;
    const u32 pj = pv[j];
    const bool follows = (pj & kLeadBit) != 0u;
    // a trash-slot leader (a full scratch table) emits nothing, as ListAgg
    const bool emits = !follows && pj != a.trash_pos;
    if (follows)
      atomicAdd(reinterpret_cast<unsigned long long*>(&s_acc[tb][pj & kIdx]), (unsigned long long)v);
    u32 idx = 0;
    if constexpr (kLocal) {
      if (emits) idx = atomicAdd(&s_cur[pj >> shift], 1u);
    } else {
      const unsigned long long m = __ballot(emits);
      if (m) {
        const int lane = lane_id();
        const int first = __ffsll((long long)m) - 1;
        u32 base = 0;
        if (lane == first) base = atomicAdd(&s_n, (u32)__popcll(m));
        idx = __shfl(base, first) + (u32)__popcll(m & ((1ull << lane) - 1ull));
      }
      if (emits) {
        XF_DASSERT((int)(pj >> shift) < kRedMaxBuckets);
        atomicAdd(&s_hist[pj >> shift], 1u);
      }
    }
    XF_KT(4);
    lds_barrier();
    XF_KT(5);
    if (!follows) {
      const long long sum = v + s_acc[tb][t];
      s_acc[tb][t] = 0ll;
      if (emits) {
        XF_DASSERT(idx < (u32)BLOCK * (u32)len);
        region[idx] = (u64)pj | ((u64)__float_as_uint((float)fx_to_double<kFx>(sum)) << 32);
      }
    }
    XF_KT(6);
  }
  __syncthreads();
  if constexpr (!kLocal) nrec = s_n;
  if (t == 0) {
    a.red_count[blockIdx.x] = nrec;
    if (a.red_records) atomicAdd(a.red_records, (unsigned long long)nrec);
  }
  for (int i = t; i < nb; i += BLOCK) {
    // (kLocal: the bucket's cursor has passed its last record)
    u32 h = s_hist[i];
    if constexpr (kLocal) h = lead_seg(s_cur[i] - h, h);
    a.red_hist[(size_t)i * gridDim.x + blockIdx.x] = h;
  }
  st.bad |= bad;
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
  XF_KT(3);
  XF_KT_FLUSH();
}

void dispatch_lr(const FwdArgs& a, hipStream_t st) {
  const bool grad = a.grad != nullptr;
  const int grid = (int)((a.batch.rows + kBlock - 1) / kBlock);
  // LDS aggregation needs every destination index to fit a u32 tag
  constexpr int kLrBlock = 1024;
  const int g = (int)((a.batch.rows + kLrBlock - 1) / kLrBlock);
  const bool red = grad && red_path(a, kRedMaxBuckets);
  if (a.red_out && !(red && (a.S == 1 || a.red_masks)))
    throw std::runtime_error("red_out needs the LR bucket reduction (S > 1: with slice bits)");
  if (a.red_masks && a.S > 1 && !red)
    throw std::runtime_error("red_masks need the LR bucket reduction");
  if (a.red_local && !a.lead)
    throw std::runtime_error("red_local: the LR leader handoff only (plan_step)");
  if (a.lead) {
    // leader-encoded positions (DedupOut::lead): one workgroup per dedup
    // tile row block, whatever the batch size (no narrow_rows)
    const BatchView& b = a.batch;
    if (!red || a.S != 1 || a.red_masks || a.red_nuq || a.red_csr.cnt || b.row_ptr ||
        b.col_stride != b.rows || b.rows % kLeadTile || b.nnz_per_row > kLrRegCols ||
        b.nnz_per_row < 1 || a.trash_pos >= kLeadBit)
      throw std::runtime_error("LR leader handoff: not a step it covers (plan_step)");
    const int gr = (int)(b.rows / kLeadTile);
    if (a.red_local) hipLaunchKernelGGL(k_lr_lead<true>, dim3(gr), dim3(kLeadTile), 0, st, a);
    else hipLaunchKernelGGL(k_lr_lead<false>, dim3(gr), dim3(kLeadTile), 0, st, a);
#ifdef XFLOW_KTIMING
    ktime_dump("lr lead (init forward - tail add barrier flush)", 7, st);
#endif
    launch_reduction<1>(a, gr, kLeadTile, st);
  } else if (red) {
    const int R = narrow_rows(a, kLrGroupRows);
    const int gr = (int)((a.batch.rows + R - 1) / R);
    launch_rows(R, [&](auto r) {
      hipLaunchKernelGGL((k_lr<true, true, decltype(r)::value, true>), dim3(gr), dim3(R), 0, st, a);
    });
#ifdef XFLOW_KTIMING
    ktime_dump("lr (init forward walk-other tail insert barrier flush)", 7, st);
#endif
    launch_reduction<1>(a, gr, R, st);
  } else if (grad && a.agg_ok)
    hipLaunchKernelGGL((k_lr<true, true, kLrBlock>), dim3(g), dim3(kLrBlock), 0, st, a);
  else if (grad)
    hipLaunchKernelGGL((k_lr<true, false, kBlock>), dim3(grid), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((k_lr<false, false, kBlock>), dim3(grid), dim3(kBlock), 0, st, a);
}

}  // namespace hip
}  // namespace xflow
