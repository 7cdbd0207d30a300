// xflow-amd: vector-record reduction of the standard-FM and MVM gradients,
// its CSR form and MVM's repeated-field passes (gfx950).  The launcher starts
// its producers itself, so they are here too: k_fm_std_red and k_fm_std_fwd.
#include "model_common.h"

namespace xflow {
namespace hip {

// Standard-math FM (Rendle) on the atomic-free reduction.  The occurrence
// gradient has 1+D components (loss; loss*(vs_k - v_k)), all of them needed
// per key.  Each column's contributions are summed per (key, slice) in an LDS
// table with 1+D fixed-point accumulators per slot (one insert per
// occurrence; 1+D integer atomics for every occurrence after the slot's
// first; deterministic), and the flush emits one vector
// record (dest, 1+D sums) per (key, slice, column) -- 48 bytes at D = 8 --
// which k_red_scan / k_red_scatter partition by dest bucket and
// k_red_sum_vec sums into the slot-indexed gradient rows.  Before: LDS column
// tables flushed with (1+D) global float atomics per (key, column,
// workgroup), 1.15 ms of a 1.6 ms FM-8 step.
// One LDS table (flushed, then a barrier, per column): 2x the rows of a
// double-buffered table for the same LDS -- larger workgroups aggregate hot
// keys over more rows (A/B: 128 rows per workgroup -21 %, 256 -> 512 below)
// (fmstd_block: backend.h)

// kSeg (the scatter-free form, launch_fmstd_reduction): a pre-pass counts the
// workgroup's occurrences per bucket -- an upper bound of its records there --
// and the flush writes each record into its bucket's sub-range of the
// workgroup region (LDS cursor), so the region leaves the kernel already
// partitioned by bucket; the sub-range starts go to red_sorted (as u32
// [bucket][workgroup]) and k_red_sum_vec<D, true> reads a bucket's records
// straight from the producers' regions -- no k_red_scatter pass over the
// (48-byte) records.
// kSplit: the forward ran in k_fm_std_fwd (its own high-occupancy launch: this
// kernel's LDS tables leave a CU two waves per SIMD for the row gathers), which
// left (loss, loss*vs_k) per row in red_rowv -- the same floats the fused form
// computes here, so both forms sum identical fixed-point values.
// kScaled (MVM): T = loss*M spans many orders of magnitude (a product over
// fields), beyond any one static fixed-point scale: the int64 sums use the
// step's scale (fx_scale_bits of FwdArgs::red_vmax, set by the forward).

template <int D, int BLOCK, bool kSeg = false, bool kSplit = false, bool kScaled = false>
__global__ void __launch_bounds__(BLOCK) k_fm_std_red(FwdArgs a) {
  XF_KT_DECL;
  constexpr int PS = fm_ps(D);
  constexpr int NV = 1 + D;
  static_assert(BLOCK == fmstd_block(D), "producer block");
  // (not a power of two: 2.75 x BLOCK at D = 8 with int32 sums)
  constexpr u32 kSlots = (u32)(kScaled ? fmstd_slots(D) : fmstd_slots32(D));
  constexpr u32 kFree = 0xffffffffu;  // (no dest: dest < trash_pos * S)
  constexpr int kFx = FxBits<1>::kFx;
  // Column accumulators.  kScaled (MVM): int64 at the step's scale.  Else
  // int32 at a per-workgroup, per-component scale: a column adds at most one
  // value per row (BLOCK of them), each below 2^31 / BLOCK once scaled by the
  // workgroup's largest |value| of that component, so no sum overflows -- and
  // an int32 LDS atomic touches one bank where an int64 one touched two (the
  // random-slot atomics were 64 % bank-conflict cycles, profiles/r5_fmstd_pmc.txt).
  // Order-free integer sums either way: deterministic.
  using Acc = typename std::conditional<kScaled, long long, int>::type;
  // slot tags: the claiming dest, kFree once its claimer has flushed it
  __shared__ u32 s_tag[kSlots];
  __shared__ Acc s_acc[1][kSlots * NV];
  __shared__ int s_fxc[NV];
  __shared__ float s_cmax[NV][BLOCK / kWave];
  const int fxs = kScaled ? fx_scale_bits(a.red_vmax, fx_head_bits(a.batch.rows)) : kFx;
  // a slot some occurrence joined (added to) this column; its claimer flushes it
  __shared__ unsigned char s_join[kSlots];
  constexpr int kMaxB = vec_red_max_buckets(D);
  // per-bucket counts, then (kSeg) each bucket's record cursor in the region
  __shared__ u32 s_hist[kMaxB];
  __shared__ u32 s_total;
  __shared__ int s_wmax[BLOCK / kWave];
  const BatchView& b = a.batch;
  const u32* __restrict__ pos = a.pos;
  const float4* __restrict__ wp4 = reinterpret_cast<const float4*>(a.wpull);
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool active = r < b.rows;
  RowSpan rs;
  if (active) rs = row_span(b, r);
  const int len = rs.len;
  const int64_t r0 = (int64_t)blockIdx.x * BLOCK;
  using Rec = typename VecRedRec<NV>::T;
  constexpr int W = vec_rec_words(NV);
  Rec* region = reinterpret_cast<Rec*>(a.red_pairs) +
                (b.row_ptr ? (int64_t)b.row_ptr[r0] : r0 * b.nnz_per_row);
  const RedGeom geom = red_geom(a);
  const int shift = geom.shift(red_shift(NV));
  for (int i = threadIdx.x; i < kSlots; i += BLOCK) {
    s_tag[i] = kFree;
    s_join[i] = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) s_acc[0][i * NV + c] = (Acc)0;
  }
  for (int i = threadIdx.x, n = geom.active(shift, a.red_nb); i < n; i += BLOCK) s_hist[i] = 0u;
  if (threadIdx.x == 0) s_total = 0u;
  int maxlen;
  if (!b.row_ptr) {
    maxlen = b.nnz_per_row;
    __syncthreads();
  } else {
    const int m = wave_max(len);
    if (threadIdx.x % kWave == 0) s_wmax[threadIdx.x / kWave] = m;
    __syncthreads();
    maxlen = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / kWave; ++w) maxlen = max(maxlen, s_wmax[w]);
  }
  XF_KT(0);
  const u32 S = (u32)a.S;
  const u32 sl = active ? (u32)slice_of(b, r, a.S) : 0u;
  // kSplit: the row's vector (FM: loss, loss*vs_k; MVM: T_k = loss*M_k); a
  // one-slice MVM step emits nothing for an all-zero one (a zero contribution
  // -- every unique key is pushed anyway), several slices need every
  // occurrence (the records' presence gives the slice bits), and so does
  // standard FM: every unique key then has a record and the reduction writes
  // every unique-order row (the pull does not zero them, Engine::train_step)
  float t[PS];
  bool live = active;
  if (kSplit && active) {
    const float4* rv = reinterpret_cast<const float4*>(a.red_rowv + (size_t)r * PS);
#pragma unroll
    for (int q = 0; q < PS / 4; ++q) {
      const float4 v4 = rv[q];
      t[4 * q] = v4.x;
      t[4 * q + 1] = v4.y;
      t[4 * q + 2] = v4.z;
      t[4 * q + 3] = v4.w;
    }
    bool nz = false;
#pragma unroll
    for (int c = 0; c < NV; ++c) nz |= t[c] != 0.0f;
    live = nz || S > 1u || !kScaled;
  }
  constexpr int kPer = kMaxB / BLOCK;
  // kSeg: this thread's buckets' sub-range starts kept for the tail (when
  // they fit a few registers; else re-read from red_sorted)
  constexpr bool kRegStart = kSeg && kPer <= 8;
  u32 sstart[kRegStart ? kPer : 1];
  if constexpr (kSeg) {
    // occurrences per bucket (s_hist, zeroed above) -> sub-range starts (the cursors)
    const PosStream pp(pos, rs, live ? len : 0, a.trash_pos, false);
    for (int j0 = 0; j0 < maxlen; j0 += kPosChunk) {
      u32 pv[kPosChunk], ok;
      pp.fetch(pv, ok, j0);
#pragma unroll
      for (int q = 0; q < kPosChunk; ++q)
        if (((ok >> q) & 1u) && pv[q] != a.trash_pos)
          atomicAdd(&s_hist[(pv[q] * S + sl) >> shift], 1u);
    }
    __syncthreads();
    const int nb = geom.active(shift, a.red_nb);
    u32 c[kPer], sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int i = (int)threadIdx.x * kPer + q;
      c[q] = i < nb ? s_hist[i] : 0u;
      sum += c[q];
    }
    u32 tot;
    u32 ex = block_exclusive_scan<BLOCK>(sum, &tot);
    u32* sub_out = reinterpret_cast<u32*>(a.red_sorted);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int i = (int)threadIdx.x * kPer + q;
      if (i < nb) {
        sub_out[(size_t)i * gridDim.x + blockIdx.x] = ex;
        s_hist[i] = ex;  // now the record cursor
      }
      if constexpr (kRegStart) sstart[q] = ex;
      ex += c[q];
    }
    __syncthreads();
  }
  XF_KT(1);
  StatAcc st;
  float loss = 0.0f;
  float vs[D];  // (kSplit: loss*vs_k)
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  if (kSplit && active) {
    loss = t[0];
#pragma unroll
    for (int k = 0; k < D; ++k) vs[k] = t[1 + k];
  } else if (active) {
    float wx = 0.0f, vp = 0.0f;
    for (int j = 0; j < len; ++j) {
      const float4* src = wp4 + (size_t)pos[rs.at(j)] * (PS / 4);
      float w[PS];
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) {
        const float4 v4 = src[q];
        w[4 * q] = v4.x;
        w[4 * q + 1] = v4.y;
        w[4 * q + 2] = v4.z;
        w[4 * q + 3] = v4.w;
      }
      wx += w[0];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        vs[k] += w[1 + k];
        vp += w[1 + k] * w[1 + k];
      }
    }
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) sq += vs[k] * vs[k];
    const float p = sigmoid_ref(wx + 0.5f * (sq - vp));
    const float lab = b.labels[r];
    loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
  }
  const int lane = lane_id();
  u32 written = 0, bad = 0;
  // the column walk's positions arrive a chunk ahead (PosStream)
  PosStream ps(pos, rs, live ? len : 0, a.trash_pos);
  // the row's fixed-point values, the same for every column: converted once
  // (factorised: Σ loss*(vs_k - v_k) = C_k - v_k*B with B = Σ loss and C_k =
  // Σ loss*vs_k -- v_k is the key's pulled value, one per step -- so the
  // column walk needs no second gather of the pulled row; k_red_sum_vec
  // expands C - v*B once per dest)
  Acc rowv[NV];
  if constexpr (kScaled) {  // (kSplit: the row's vector, |.| <= the step's vmax)
    rowv[0] = fx_from_rt(loss, fxs);
#pragma unroll
    for (int k = 0; k < D; ++k) rowv[1 + k] = fx_from_rt(vs[k], fxs);
  } else {
    // per-component scale from the workgroup's largest |value| (see s_acc)
    float f[NV];
    f[0] = loss;
#pragma unroll
    for (int k = 0; k < D; ++k) f[1 + k] = kSplit ? vs[k] : loss * vs[k];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      float m = f[c] == f[c] ? fabsf(f[c]) : INFINITY;
      if (!(m <= 3.0e38f)) bad = 1u;  // non-finite: a diverged model (flagged, read as 0)
      m = wave_max(m <= 3.0e38f ? m : 0.0f);
      if (lane_id() == 0) s_cmax[c][threadIdx.x / kWave] = m;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
      float m = 0.0f;
#pragma unroll
      for (int w = 0; w < BLOCK / kWave; ++w) m = fmaxf(m, s_cmax[threadIdx.x][w]);
      int e = 0;
      if (m > 0.0f) frexpf(m, &e);  // m < 2^e
      constexpr int kHead = ilog2c(BLOCK) + 1;  // (BLOCK terms, plus rounding slack)
      const int fx = 31 - kHead - e;
      s_fxc[threadIdx.x] = fx < -100 ? -100 : (fx > 100 ? 100 : fx);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const double d = ldexp((double)f[c], s_fxc[c]);
      rowv[c] = (d == d && fabs(d) < 2.1e9) ? (int)__builtin_rint(d) : 0;
    }
  }
  // Per column: insert (claim a free slot, or find the dest's); an occurrence
  // that found its (key, slice) already claimed adds its NV values to the slot
  // and marks it joined; a claimer reserves its record's place right away.
  // After a barrier each claimer frees its slot and writes the record -- its
  // own values plus, if joined, the slot's sums (then zeroed) -- so the next
  // column starts on an empty table: the insert is one CAS against kFree per
  // probe step (no read first, no stale tags), and a key alone in its column
  // (25-35 % of the occurrences at the Criteo shape) costs one CAS, one flag
  // read and one tag write -- no accumulator traffic.
  int fxc[NV];  // (the workgroup's scales, out of LDS once)
#pragma unroll
  for (int c = 0; c < NV; ++c) fxc[c] = kScaled ? 0 : s_fxc[c];
  XF_KT(2);
  for (int j0 = 0; j0 < maxlen; j0 += kPosChunk) {
    ps.prefetch(j0 + kPosChunk);
#pragma unroll
    for (int q = 0; q < kPosChunk; ++q) {
      if (j0 + q >= maxlen) break;
      const u32 pj = ps.get(q);
      const bool has = pj != a.trash_pos;
      const u32 dest = pj * S + sl;
      bool claimed = false;
      u32 h = 0;
      if (has) {
        h = (u32)(((u64)(dest * 0x9E3779B1u) * kSlots) >> 32);
        while (true) {  // <= BLOCK keys per column in > BLOCK free slots: terminates
          const u32 old = atomicCAS(&s_tag[h], kFree, dest);
          if (old == kFree) {
            claimed = true;
            break;
          }
          if (old == dest) break;
          h = h + 1 == kSlots ? 0u : h + 1;
        }
      }
      if (has && !claimed) {
        Acc* acc = &s_acc[0][h * NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
          if constexpr (kScaled)
            atomicAdd(reinterpret_cast<unsigned long long*>(&acc[c]), (unsigned long long)rowv[c]);
          else
            atomicAdd(&acc[c], rowv[c]);
        }
        s_join[h] = 1;
      }
      u32 idx = 0;
      if constexpr (kSeg) {  // the record's place in its bucket's sub-range
        if (claimed) idx = atomicAdd(&s_hist[dest >> shift], 1u);
      } else {  // the record's index in the workgroup region
        const unsigned long long m = __ballot(claimed);
        if (m) {
          const int leader = __ffsll((long long)m) - 1;
          u32 base = 0;
          if (lane == leader) base = atomicAdd(&s_total, (u32)__popcll(m));
          idx = __shfl(base, leader) + (u32)__popcll(m & ((1ull << lane) - 1ull));
        }
        if (claimed) atomicAdd(&s_hist[dest >> shift], 1u);
      }
      XF_KT(3);
      lds_barrier();
      XF_KT(4);
      if (claimed) {
        s_tag[h] = kFree;
        Acc* acc = &s_acc[0][h * NV];
        Acc sum[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) sum[c] = rowv[c];
        if (s_join[h]) {
          s_join[h] = 0;
#pragma unroll
          for (int c = 0; c < NV; ++c) {
            sum[c] += acc[c];
            acc[c] = (Acc)0;
          }
        }
        u32 wv[W];
        wv[0] = dest;
#pragma unroll
        for (int c = 0; c < NV; ++c)
          wv[1 + c] = __float_as_uint(kScaled ? (float)fx_to_double_rt((long long)sum[c], fxs)
                                              : (float)ldexp((double)sum[c], -fxc[c]));
#pragma unroll
        for (int c = 1 + NV; c < W; ++c) wv[c] = 0u;
        Rec rec;
#pragma unroll
        for (int u = 0; u < W / 4; ++u)
          rec.q[u] = make_uint4(wv[4 * u], wv[4 * u + 1], wv[4 * u + 2], wv[4 * u + 3]);
        region[idx] = rec;
        if constexpr (kSeg) ++written;
      }
      XF_KT(5);
      lds_barrier();  // (one table: freed before the next column inserts)
      XF_KT(6);
    }
    ps.advance();
  }
  if constexpr (kSeg) {  // (the non-kSeg count is s_total already)
    const u32 wsum = wave_sum_u32(written);
    if (lane == 0 && wsum) atomicAdd(&s_total, wsum);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    written = s_total;
    a.red_count[blockIdx.x] = written;
    if (a.red_records) atomicAdd(a.red_records, (unsigned long long)written);
  }
  // (kSeg: the cursor ends at the bucket's start in the region + its records;
  // the starts are still in the registers of the pre-pass's bucket mapping)
  if constexpr (kRegStart) {
    const int nb = geom.active(shift, a.red_nb);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int i = (int)threadIdx.x * kPer + q;
      if (i < nb) a.red_hist[(size_t)i * gridDim.x + blockIdx.x] = s_hist[i] - sstart[q];
    }
  } else {
    const u32* sub_start = reinterpret_cast<const u32*>(a.red_sorted);
    for (int i = threadIdx.x, n = geom.active(shift, a.red_nb); i < n; i += BLOCK) {
      const size_t at = (size_t)i * gridDim.x + blockIdx.x;
      a.red_hist[at] = kSeg ? s_hist[i] - sub_start[at] : s_hist[i];
    }
  }
  st.bad |= bad;
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
  XF_KT(7);
  XF_KT_FLUSH();
}

// Sums of a bucket's vector records: units of kR dests (as k_red_sum) with
// (1+D) int64 accumulators per dest in LDS; every dest a record reached gets
// its whole gradient row (pad components 0) -- the rows are the step's
// (slot, slice) gradients the apply reads.
// kSeg: no scatter pass -- bucket bk's records are the producers' sub-ranges
// (k_fm_std_red<.., true>): segment g holds hist[bk][g+1] - hist[bk][g]
// records (hist: k_red_scan's exclusive prefix over the workgroups, tot[bk]
// the total) at region(g) + subs[bk][g]; record i of the bucket is found by a
// binary search of the LDS-staged prefix.
// (kSegMaxGroups: backend.h)
// G: segment-table capacity (groups); 512 keeps the rank-8 form at 76 KB of
// LDS, two workgroups per CU (the per-unit phases are latency chains)
// kMvm: the records are MVM's per-row T = loss*M sums (NV = 1 + D = the MVM
// latent dim) and the final gradient is g_k += Σ T_k / (1 + v_k), none where
// v_k == 0 (mvm_worker.cc:137-170: the occurrence's field sum S is the key's
// own v in a row without repeated fields); added to the rows (a repeated-field
// row's gradients arrive there by atomics first).
template <int D, bool kSeg = false, int G = kSegMaxGroups, bool kMvm = false>
__global__ void __launch_bounds__(kRedBlock) k_red_sum_vec(const void* __restrict__ sorted,
                                                           const u32* __restrict__ start,
                                                           float* __restrict__ grad,
                                                           RedGeom geom, int nb,
                                                           float* __restrict__ out,
                                                           const u32* __restrict__ inv,
                                                           const float* __restrict__ wpull,
                                                           int S, SegSrc sg,
                                                           u32* __restrict__ masks,
                                                           const u32* __restrict__ vmax,
                                                           const u32* __restrict__ dup = nullptr) {
  constexpr int NV = 1 + D;
  constexpr int PS = fm_ps(D);
  constexpr int kShift = red_shift(NV);
  constexpr u32 kR = 1u << kShift;
  constexpr int kFx = FxBits<1>::kFx;
  constexpr int W = vec_rec_words(NV);
  using Rec = typename VecRedRec<NV>::T;
  __shared__ long long acc[kR * NV];
  // MVM: the step's fixed-point scale (k_fm_std_red kScaled)
  const int fxs = kMvm ? fx_scale_bits(vmax, geom.fx_head) : kFx;
  // MVM: no repeated-field row added to the rows this step -- they hold the
  // pull's zeros, so the epilogue stores without reading them
  const bool rows_zero = kMvm && dup && *dup == 0u;
  __shared__ u32 seen[kR / 32];
  __shared__ u32 s_pre[kSeg ? G : 1];
  __shared__ u32 s_seg[kSeg ? G : 1];
  const Rec* src = static_cast<const Rec*>(sorted);
  const int shift = geom.shift(kShift);
  const u32 act = (u32)geom.active(shift, nb);
  // A workgroup takes whole buckets: a bucket wider than a unit (several
  // slices' dests) is summed unit after unit by the same workgroup, so its
  // segment table is staged once (per unit, the staging -- two loads per
  // producer workgroup -- cost more than the records at 32 slices)
  const u32 nsubs = 1u << (shift - kShift);
  for (u32 bk = blockIdx.x; bk < act; bk += gridDim.x) {
    u32 beg, end;
    if constexpr (kSeg) {
      beg = 0;
      end = sg.tot[bk];
    } else {
      beg = start[bk];
      end = start[bk + 1];
    }
    if (beg == end) continue;  // (block-uniform)
    if constexpr (kSeg) {
      // segment g: records [s_pre[g], s_pre[g+1]) of the bucket, at s_seg[g] + i
      const size_t row0 = (size_t)bk * sg.groups;
      for (int g = threadIdx.x; g < sg.groups; g += kRedBlock) {
        const int64_t r0 = (int64_t)g * sg.rows_per_group;
        const u32 base = (u32)(sg.b.row_ptr ? sg.b.row_ptr[r0] : r0 * sg.b.nnz_per_row);
        const u32 p = sg.hist[row0 + g];
        s_pre[g] = p;
        s_seg[g] = base + sg.subs[row0 + g] - p;
      }
    }
  for (u32 sub = 0; sub < nsubs; ++sub) {
    const u64 lo = ((u64)bk << shift) + ((u64)sub << kShift);
    for (u32 i = threadIdx.x; i < kR * NV; i += kRedBlock) acc[i] = 0ll;
    for (u32 i = threadIdx.x; i < kR / 32; i += kRedBlock) seen[i] = 0u;
    lds_barrier();
    for (u32 i = beg + threadIdx.x; i < end; i += kRedBlock) {
      u32 ri = i;
      if constexpr (kSeg) {
        int l0 = 0, l1 = sg.groups;  // first g with s_pre[g] > i
        while (l0 < l1) {
          const int m = (l0 + l1) >> 1;
          if (s_pre[m] <= i) l0 = m + 1;
          else l1 = m;
        }
        ri = s_seg[l0 - 1] + i;
      }
      const Rec r = src[ri];
      const u64 l = (u64)r.q[0].x - lo;
      if (l >= kR) continue;  // (another sub-unit's dest)
      u32 wv[W];
#pragma unroll
      for (int q = 0; q < W / 4; ++q) {
        wv[4 * q] = r.q[q].x;
        wv[4 * q + 1] = r.q[q].y;
        wv[4 * q + 2] = r.q[q].z;
        wv[4 * q + 3] = r.q[q].w;
      }
      long long* ap = acc + l * NV;
#pragma unroll
      for (int c = 0; c < NV; ++c)
        atomicAdd(reinterpret_cast<unsigned long long*>(&ap[c]),
                  (unsigned long long)fx_from_rt(__uint_as_float(wv[1 + c]), fxs));
      atomicOr(&seen[l >> 5], 1u << (l & 31));
    }
    lds_barrier();
    for (u32 l = threadIdx.x; l < kR; l += kRedBlock) {
      if (!((seen[l >> 5] >> (l & 31)) & 1u)) continue;
      if constexpr (kMvm) {
        const u64 slot = (lo + l) / (u64)S;
        float* row = grad + (lo + l) * PS;
        if (out) {
          const u32 u = uix(inv, slot);
          if (u == 0xFFFFFFFFu) continue;
          row = out + ((u64)u * (u64)S + (lo + l - slot * (u64)S)) * PS;
        }
        // (whole rows as dwordx4: the pulled v, the row's earlier atomics)
        const float4* w4 = reinterpret_cast<const float4*>(wpull + slot * PS);
        float4* r4 = reinterpret_cast<float4*>(row);
        float w[PS], o[PS];
#pragma unroll
        for (int q = 0; q < PS / 4; ++q) {
          const float4 a4 = w4[q], b4 = rows_zero ? make_float4(0.f, 0.f, 0.f, 0.f) : r4[q];
          w[4 * q] = a4.x, w[4 * q + 1] = a4.y, w[4 * q + 2] = a4.z, w[4 * q + 3] = a4.w;
          o[4 * q] = b4.x, o[4 * q + 1] = b4.y, o[4 * q + 2] = b4.z, o[4 * q + 3] = b4.w;
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) {
          const long long t = acc[l * NV + c];
          if (t != 0 && w[c] != 0.0f) o[c] += (float)(fx_to_double_rt(t, fxs) / (1.0 + (double)w[c]));
        }
#pragma unroll
        for (int q = 0; q < PS / 4; ++q) r4[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        continue;
      }
      // (B, C_0..C_{D-1}) -> g_w = B, g_v[k] = C_k - v_k*B (k_fm_std_red)
      const double B = fx_to_double_rt(acc[l * NV], fxs);
      const float4* v4 = reinterpret_cast<const float4*>(wpull + ((lo + l) / (u64)S) * PS);
      float o[PS];
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) {
        const float4 v = v4[q];
        o[4 * q] = v.x;
        o[4 * q + 1] = v.y;
        o[4 * q + 2] = v.z;
        o[4 * q + 3] = v.w;
      }
      o[0] = (float)B;
#pragma unroll
      for (int c = 1; c < PS; ++c)
        o[c] = c < NV ? (float)(fx_to_double_rt(acc[l * NV + c], fxs) - (double)o[c] * B) : 0.0f;
      float* row = grad + (lo + l) * PS;
      if (out) {  // the unique-order row (FwdArgs::red_out); S > 1: [unique][slice]
        const u64 slot = (lo + l) / (u64)S;
        const u32 u = uix(inv, slot);
        if (u == 0xFFFFFFFFu) continue;
        row = out + ((u64)u * (u64)S + (lo + l - slot * (u64)S)) * PS;
      }
      float4* g4 = reinterpret_cast<float4*>(row);
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) g4[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
    // S > 1: each slot's slice bits from the records' presence (every
    // occurrence leaves a record, so a slice that touched the key is present
    // even with a zero gradient -- it still pushes, like the reference's slice)
    if (masks) unit_masks<kR>(seen, lo, (u64)S, masks, out ? inv : nullptr);
    lds_barrier();  // (the next unit reinitialises what this one read)
  }
  }
}

// One-workgroup exclusive scan of n u32 counts (n + 1 outputs, the last the
// total): the CSR entries' base of every bucket from its record total.
__global__ void __launch_bounds__(kRedBlock) k_scan_small(const u32* __restrict__ in, int nb,
                                                        u32* __restrict__ out, RedGeom geom,
                                                        int base) {
  const int n = geom.active(geom.shift(base), nb);  // (k_red_scan's buckets)
  u32 carry = 0;
  for (int c0 = 0; c0 < n; c0 += kRedBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < n ? in[i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kRedBlock>(v, &t);
    if (i < n) out[i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// CSR form of the standard-FM vector reduction (several slices, dests =
// unique * 2^slog2 + slice): only the touched (key, slice) pairs become
// entries (slice, g_w, g_v_0 .. g_v_{D-1}) -- expanded with the pulled v
// (g_w = B, g_v = C - v*B, fm_worker.cc:159-202 in Rendle's form) and divided
// by the slice's rows -- in (key, slice) order, with each key's (off, cnt):
// the per-key push chains of the reference's per-slice pushes
// (fm_worker.cc:241-242) in one apply.  Per bucket and window of 2^15 dests:
// (1) a presence bitmap of the records' dests, (2) its prefix popcounts --
// the rank of a present dest is its entry index, (3) the keys' (off, cnt)
// from the bitmap, (4) the records' fixed-point sums accumulated at their
// rank (1024 ranks at a time, NV int64 each in LDS), then expanded and
// written.  Only distinct present dests take LDS, so the many-slice dest
// space (2^slog2 per key) costs one pass over the records, not one per
// 2^10-dest unit as the dense rows did.
constexpr int kCsrVecWin = 15;
// kMvm: the records are MVM's per-row T = loss*M sums (scaled fixed point,
// k_red_sum_vec<.., kMvm>) and an entry is g_k = Σ T_k / (1 + v_k), 0 where
// v_k == 0 (mvm_worker.cc:137-170); rows with a repeated field are added
// after, by the MvmDup passes (k_mdup_*).
template <int D, int G, bool kMvm = false>
__global__ void __launch_bounds__(kRedBlock) k_red_csr_vec(const void* __restrict__ recs, RedGeom geom,
                                                         int nb, SegSrc sg,
                                                         const u32* __restrict__ estart,
                                                         CsrOut co, const float* __restrict__ wpull,
                                                         const u32* __restrict__ vmax) {
  constexpr int NV = 1 + D;
  constexpr int PS = fm_ps(D);
  constexpr int kShift = red_shift(NV);
  // ranks per accumulation chunk: NV int64 each in <= 120 KB of LDS (one
  // workgroup per CU; a bucket holds ~500-1000 distinct dests, so at 1024
  // ranks one chunk -- one second pass over the records -- covers it: 512
  // at MVM-10's NV = 10 took a third pass, 332 vs 213 us for FM-8)
  constexpr u32 kR = (120 * 1024 / (8 * NV) < 2048 ? 120 * 1024 / (8 * NV) : 2048) & ~63u;
  constexpr u32 kWords = 1u << (kCsrVecWin - 5);
  static_assert(kWords == kRedBlock, "one bitmap word per thread");
  constexpr int kFx = FxBits<1>::kFx;
  using Rec = typename VecRedRec<NV>::T;
  __shared__ long long acc[kR * NV];
  __shared__ u32 bits[kWords];
  __shared__ u32 wscan[kWords];
  __shared__ u32 rdest[kR];
  __shared__ u32 s_pre[G];
  __shared__ u32 s_seg[G];
  __shared__ u32 s_tot;
  const Rec* src = static_cast<const Rec*>(recs);
  const int shift = geom.shift(kShift);
  const u32 act = (u32)geom.active(shift, nb);
  const int sl = co.slog2;
  const u32 smask = (1u << sl) - 1u;
  const int ew = co.ew, P = co.P;
  float* ent = static_cast<float*>(co.ent);
  const int tid = (int)threadIdx.x;
  const int fxs = kMvm ? fx_scale_bits(vmax, geom.fx_head) : kFx;
  for (u32 bk = blockIdx.x; bk < act; bk += gridDim.x) {
    const u32 nrec = sg.tot[bk];
    if (nrec == 0) continue;  // (block-uniform)
    const size_t row0 = (size_t)bk * sg.groups;
    for (int g = tid; g < sg.groups; g += kRedBlock) {
      const int64_t r0 = (int64_t)g * sg.rows_per_group;
      const u32 base = (u32)(sg.b.row_ptr ? sg.b.row_ptr[r0] : r0 * sg.b.nnz_per_row);
      const u32 pf = sg.hist[row0 + g];
      s_pre[g] = pf;
      s_seg[g] = base + sg.subs[row0 + g] - pf;
    }
    auto rec_at = [&](u32 i) -> const Rec& {
      int l0 = 0, l1 = sg.groups;  // first g with s_pre[g] > i
      while (l0 < l1) {
        const int m = (l0 + l1) >> 1;
        if (s_pre[m] <= i) l0 = m + 1;
        else l1 = m;
      }
      return src[s_seg[l0 - 1] + i];
    };
    u32 ebase = estart[bk];
    const u64 blo = (u64)bk << shift;
    const u64 bhi = blo + (1ull << shift);
    for (u64 lo = blo; lo < bhi; lo += 1ull << kCsrVecWin) {
      // (1) presence
      bits[tid] = 0u;
      lds_barrier();
      for (u32 i = tid; i < nrec; i += kRedBlock) {
        const u64 l = (u64)rec_at(i).q[0].x - lo;
        if (l < (1ull << kCsrVecWin)) atomicOr(&bits[l >> 5], 1u << (l & 31));
      }
      lds_barrier();
      // (2) ranks
      u32 tot;
      const u32 ex = block_exclusive_scan<kRedBlock>((u32)__popc(bits[tid]), &tot);
      wscan[tid] = ex;
      if (tid == 0) s_tot = tot;
      lds_barrier();
      const u32 ndist = s_tot;
      if (ndist == 0) continue;  // (block-uniform)
      auto rank = [&](u32 l) {
        return wscan[l >> 5] + (u32)__popc(bits[l >> 5] & ((1u << (l & 31)) - 1u));
      };
      // (3) the keys' (off, cnt): the window holds 2^(15 - slog2) keys whole
      for (u32 k = tid; k < (1u << (kCsrVecWin - sl)); k += kRedBlock) {
        const u32 l0 = k << sl;
        u32 cnt;
        if (sl >= 5) {
          cnt = 0;
          for (u32 w = l0 >> 5; w < (l0 + (1u << sl)) >> 5; ++w) cnt += (u32)__popc(bits[w]);
        } else {
          cnt = (u32)__popc((bits[l0 >> 5] >> (l0 & 31)) & ((1u << (1u << sl)) - 1u));
        }
        if (cnt) {
          const u32 u = (u32)((lo + l0) >> sl);
          co.off[u] = ebase + rank(l0);
          co.cnt[u] = cnt;
        }
      }
      // (4) sums at the ranks, kR ranks at a time
      for (u32 c0 = 0; c0 < ndist; c0 += kR) {
        for (u32 i = tid; i < kR * NV; i += kRedBlock) acc[i] = 0ll;
        lds_barrier();
        for (u32 i = tid; i < nrec; i += kRedBlock) {
          const Rec& rr = rec_at(i);
          const u64 l = (u64)rr.q[0].x - lo;
          if (l >= (1ull << kCsrVecWin)) continue;
          const u32 r = rank((u32)l) - c0;
          if (r >= kR) continue;
          const Rec r4 = rr;
          u32 wv[vec_rec_words(NV)];
#pragma unroll
          for (int q = 0; q < vec_rec_words(NV) / 4; ++q) {
            wv[4 * q] = r4.q[q].x;
            wv[4 * q + 1] = r4.q[q].y;
            wv[4 * q + 2] = r4.q[q].z;
            wv[4 * q + 3] = r4.q[q].w;
          }
          rdest[r] = wv[0];  // (every record of the rank writes the same dest)
          long long* ap = acc + r * NV;
#pragma unroll
          for (int c = 0; c < NV; ++c)
            atomicAdd(reinterpret_cast<unsigned long long*>(&ap[c]),
                      (unsigned long long)fx_from_rt(__uint_as_float(wv[1 + c]), fxs));
        }
        lds_barrier();
        const u32 nr = min(kR, ndist - c0);
        for (u32 t = tid; t < nr; t += kRedBlock) {
          const u32 d = rdest[t];
          const u32 u = d >> sl, s = d & smask;
          const double rows = co.rows ? (double)co.rows[s] : 1.0;
          const float* v = wpull + (u64)u * PS;
          float* e = ent + (u64)(ebase + c0 + t) * (u32)ew;
          e[0] = __uint_as_float(s);
          if constexpr (kMvm) {
#pragma unroll
            for (int c = 0; c < NV; ++c) {
              const long long tc = acc[t * NV + c];
              if (c < P)
                e[1 + c] = tc != 0 && v[c] != 0.0f
                               ? (float)(fx_to_double_rt(tc, fxs) / (1.0 + (double)v[c]) / rows)
                               : 0.0f;
            }
          } else {
            const double B = fx_to_double_rt(acc[t * NV], fxs);
            e[1] = (float)(B / rows);
#pragma unroll
            for (int c = 1; c < NV; ++c)
              if (c < P) e[1 + c] = (float)((fx_to_double_rt(acc[t * NV + c], fxs) - (double)v[c] * B) / rows);
          }
        }
        lds_barrier();  // (the next chunk reinitialises what this one read)
      }
      ebase += ndist;
    }
  }
}

// MVM rows with a repeated field (MvmDup): three order-free passes after the
// reduction.  (1) resolve each record's target -- CSR: its (key, slice)
// entry, found among the key's entries (every occurrence left a record, so
// it exists) -- and zero the target's accumulators and claim; (2) add the
// records' components in fixed point at the step's scale (the forward's
// largest |c|; 2^head of them fit int64); (3) the first record of a target
// adds the sums to the row / entry once (entries divided by the slice's rows,
// as the entry itself is).  Integer sums: deterministic in any order.
__global__ void __launch_bounds__(kBlock) k_mdup_prep(MvmDup m, CsrOut co, int D, int max_n) {
  const u32 n = min(*m.n, (u32)min<int64_t>(max_n, m.cap));
  const bool csr = co.cnt != nullptr;
  const int sl = co.slog2;
  const u32 smask = (1u << sl) - 1u;
  const float* ent = static_cast<const float*>(co.ent);
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float* r = m.rec + (size_t)i * m.ew;
    u32 t = __float_as_uint(r[0]);
    if (csr) {
      const u32 u = t >> sl, s = t & smask;
      const u32 o = co.off[u], c = co.cnt[u];
      u32 e = o;
      while (e < o + c && __float_as_uint(ent[(size_t)e * co.ew]) != s) ++e;
      t = e < o + c ? e : 0xFFFFFFFFu;
      r[0] = __uint_as_float(t);
    }
    if (t == 0xFFFFFFFFu || (int64_t)t >= m.cap) continue;
    for (int k = 0; k < D; ++k) m.acc[(size_t)t * D + k] = 0ll;
    m.claim[t] = 0u;
  }
}

__global__ void __launch_bounds__(kBlock) k_mdup_acc(MvmDup m, int D, int head, int max_n) {
  const u32 n = min(*m.n, (u32)min<int64_t>(max_n, m.cap));
  const int fxs = fx_scale_bits(m.vmax, head);
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* r = m.rec + (size_t)i * m.ew;
    const u32 t = __float_as_uint(r[0]);
    if (t == 0xFFFFFFFFu || (int64_t)t >= m.cap) continue;
    for (int k = 0; k < D; ++k)
      atomicAdd(reinterpret_cast<unsigned long long*>(&m.acc[(size_t)t * D + k]),
                (unsigned long long)fx_from_rt(r[1 + k], fxs));
  }
}

__global__ void __launch_bounds__(kBlock) k_mdup_fin(MvmDup m, CsrOut co, float* __restrict__ out,
                                                     int PS, int D, int head, int max_n) {
  const u32 n = min(*m.n, (u32)min<int64_t>(max_n, m.cap));
  const int fxs = fx_scale_bits(m.vmax, head);
  const bool csr = co.cnt != nullptr;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 t = __float_as_uint(m.rec[(size_t)i * m.ew]);
    if (t == 0xFFFFFFFFu || (int64_t)t >= m.cap) continue;
    if (atomicExch(&m.claim[t], 1u) != 0u) continue;  // (one adder per target)
    const long long* ac = m.acc + (size_t)t * D;
    if (csr) {
      float* e = static_cast<float*>(co.ent) + (size_t)t * co.ew;
      const u32 s = __float_as_uint(e[0]);
      const double rows = co.rows ? (double)co.rows[s] : 1.0;
      for (int k = 0; k < co.P && k + 1 < co.ew && k < D; ++k)
        e[1 + k] += (float)(fx_to_double_rt(ac[k], fxs) / rows);
    } else {
      float* row = out + (size_t)t * PS;
      for (int k = 0; k < D; ++k) row[k] += (float)fx_to_double_rt(ac[k], fxs);
    }
  }
}

// the step's record count and scale back to 0 once the passes read them (a
// step without a forward -- 0 rows -- must find them 0, whatever the parity)
__global__ void k_mdup_done(u32* n, u32* vmax) {
  *n = 0u;
  *vmax = 0u;
}

static void launch_mdup(const FwdArgs& a, int D, hipStream_t st) {
  const int64_t nmax = a.batch.nnz < a.mdup.cap ? a.batch.nnz : a.mdup.cap;
  const int g = (int)std::min<int64_t>(2048, (nmax + kBlock - 1) / kBlock + 1);
  const int head = fx_head_bits(a.batch.nnz);
  CsrOut co = a.red_csr.cnt ? a.red_csr : CsrOut();
  hipLaunchKernelGGL(k_mdup_prep, dim3(g), dim3(kBlock), 0, st, a.mdup, co, D, (int)nmax);
  hipLaunchKernelGGL(k_mdup_acc, dim3(g), dim3(kBlock), 0, st, a.mdup, D, head, (int)nmax);
  hipLaunchKernelGGL(k_mdup_fin, dim3(g), dim3(kBlock), 0, st, a.mdup, co, a.red_out,
                     D == 1 ? 1 : (D + 3) & ~3, D, head, (int)nmax);  // (mvm_ps)
  hipLaunchKernelGGL(k_mdup_done, dim3(1), dim3(1), 0, st, a.mdup.n, a.mdup.vmax);
}

// Standard-math FM forward of the split form (k_fm_std_red<.., kSplit>): one
// lane per row, the same sums in the same order as the fused kernel; writes
// (loss, loss*vs_0 .. loss*vs_{D-1}, pad) per row to red_rowv.
template <int D>
__global__ void __launch_bounds__(kBlock) k_fm_std_fwd(FwdArgs a) {
  constexpr int PS = fm_ps(D);
  const BatchView& b = a.batch;
  const u32* __restrict__ pos = a.pos;
  const float4* __restrict__ wp4 = reinterpret_cast<const float4*>(a.wpull);
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  StatAcc st;
  if (r < b.rows) {
    const RowSpan rs = row_span(b, r);
    float vs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) vs[k] = 0.0f;
    float wx = 0.0f, vp = 0.0f;
    for (int j = 0; j < rs.len; ++j) {
      const float4* src = wp4 + (size_t)pos[rs.at(j)] * (PS / 4);
      float w[PS];
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) {
        const float4 v4 = src[q];
        w[4 * q] = v4.x;
        w[4 * q + 1] = v4.y;
        w[4 * q + 2] = v4.z;
        w[4 * q + 3] = v4.w;
      }
      wx += w[0];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        vs[k] += w[1 + k];
        vp += w[1 + k] * w[1 + k];
      }
    }
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) sq += vs[k] * vs[k];
    const float p = sigmoid_ref(wx + 0.5f * (sq - vp));
    const float lab = b.labels[r];
    const float loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
    float o[PS];
    o[0] = loss;
#pragma unroll
    for (int c = 1; c < PS; ++c) o[c] = c <= D ? loss * vs[c - 1] : 0.0f;
    float4* t4 = reinterpret_cast<float4*>(a.red_rowv + (size_t)r * PS);
#pragma unroll
    for (int q = 0; q < PS / 4; ++q) t4[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  }
  flush_stats<kBlock>(st, a.stats, a.fx_bad);
}

// Vector-record reduction of NV = 1 + D sums per (key, slice): standard FM
// (rows (loss, loss*vs_k) from k_fm_std_fwd, expanded with the pulled v) or,
// kMvm, MVM (rows T_k = loss*M_k from k_mvm2<.., kRed>, divided by 1 + v_k).
template <int D, bool kMvm>
void launch_vec_reduction(const FwdArgs& a, hipStream_t st) {
  constexpr int BLOCK = fmstd_block(D);
  constexpr int NV = 1 + D;
  if (kMvm && (!a.red_rowv || !a.red_vmax))
    throw std::runtime_error("MVM vector reduction needs red_rowv and red_vmax");
  const int groups = (int)((a.batch.rows + BLOCK - 1) / BLOCK);
  const RedGeom geom = red_geom(a);
  const u32 grid = std::min<u32>((u32)(a.red_nb * a.red_nsub), (u32)device_cus());
  if (a.red_out && a.S != 1 && !a.red_masks)
    throw std::runtime_error("vector-record red_out with several slices needs the slice bits");
  u32* masks = a.S > 1 ? a.red_masks : nullptr;
  // scatter-free form: the sub-range starts ([nb][groups] u32) live in red_sorted
  // (XFLOW_FMSTD_SEG=0: the dense producer region + k_red_scatter instead, an A/B switch)
  static const bool seg_on = [] {
    const char* e = std::getenv("XFLOW_FMSTD_SEG");
    return !(e && e[0] == '0');
  }();
  const bool seg = seg_on && groups <= kSegMaxGroups &&
                   (int64_t)a.red_nb * groups <= 2 * a.red_sorted_words &&
                   a.red_sorted_words * 8 / (vec_rec_words(NV) * 4) < (1ll << 32);
  if (a.red_maxb > vec_red_max_buckets(D) || (!seg && a.red_maxb > kRedMaxBuckets))
    throw std::runtime_error("vector reduction: bucket cap beyond the producer's");
  const bool split = a.red_rowv != nullptr;
  // (one slice: the rows' only other writer is k_mvm2's repeated-field atomics)
  const u32* dup = kMvm && a.S == 1 ? a.red_dup : nullptr;
  if (a.red_csr.cnt) {  // several slices as CSR entries (Engine::train_step_csr)
    if (!seg || !split || a.red_out || !a.red_nuq || a.S != (1 << a.red_csr.slog2) ||
        (kMvm && !a.mdup.rec) ||
        a.red_csr.slog2 > red_shift(NV) || a.red_csr.P > NV || a.red_csr.P < 1 ||
        a.red_csr.ew < csr_row_words(a.red_csr.P))
      throw std::runtime_error("CSR vector reduction: split scatter-free form, unique positions, "
                               "S = 2^slog2 <= 2^shift, full-row entries (MVM: dup records)");
  }
#ifdef XFLOW_KTIMING
  ktime_dump("fmstd (init prepass rowv insert bar1 flush bar2 tail)", 8, st);
#endif
  if (split && !kMvm)
    hipLaunchKernelGGL(k_fm_std_fwd<D>, dim3((int)((a.batch.rows + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, st, a);
  if (a.red_csr.cnt) {
    hipLaunchKernelGGL((k_fm_std_red<D, BLOCK, true, true, kMvm>), dim3(groups), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_red_scan, dim3(a.red_nb), dim3(kBlock), 0, st, a.red_hist, groups,
                       a.red_tot, geom, red_shift(NV));
    u32* estart = a.red_tot + a.red_nb + 1;  // (nb + 1 words: the scatter's starts, unused here)
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(kRedBlock), 0, st, a.red_tot, a.red_nb, estart,
                       geom, red_shift(NV));
    const SegSrc sg{a.red_hist, a.red_tot, reinterpret_cast<const u32*>(a.red_sorted), a.batch,
                    BLOCK, groups};
    const u32 g2 = std::min<u32>((u32)a.red_nb, (u32)device_cus());
    if (groups <= 512)
      hipLaunchKernelGGL((k_red_csr_vec<D, 512, kMvm>), dim3(g2), dim3(kRedBlock), 0, st,
                         static_cast<const void*>(a.red_pairs), geom, a.red_nb, sg, estart,
                         a.red_csr, a.wpull, a.red_vmax);
    else
      hipLaunchKernelGGL((k_red_csr_vec<D, kSegMaxGroups, kMvm>), dim3(g2), dim3(kRedBlock), 0, st,
                         static_cast<const void*>(a.red_pairs), geom, a.red_nb, sg, estart,
                         a.red_csr, a.wpull, a.red_vmax);
    if (kMvm && a.mdup.rec) launch_mdup(a, NV, st);  // (rows with a repeated field)
    return;
  }
  if (seg) {
    if (split) hipLaunchKernelGGL((k_fm_std_red<D, BLOCK, true, true, kMvm>), dim3(groups), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_fm_std_red<D, BLOCK, true>), dim3(groups), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_red_scan, dim3(a.red_nb), dim3(kBlock), 0, st, a.red_hist, groups,
                       a.red_tot, geom, red_shift(NV));
    const SegSrc sg{a.red_hist, a.red_tot, reinterpret_cast<const u32*>(a.red_sorted), a.batch,
                    BLOCK, groups};
    if (groups <= 512) {
      const u32 grid2 = std::min<u32>((u32)(a.red_nb * a.red_nsub), 2u * (u32)device_cus());
      hipLaunchKernelGGL((k_red_sum_vec<D, true, 512, kMvm>), dim3(grid2), dim3(kRedBlock), 0, st,
                         static_cast<const void*>(a.red_pairs), nullptr, a.grad, geom, a.red_nb,
                         a.red_out, a.red_inv, a.wpull, a.S, sg, masks, a.red_vmax, dup);
    } else {
      hipLaunchKernelGGL((k_red_sum_vec<D, true, kSegMaxGroups, kMvm>), dim3(grid), dim3(kRedBlock), 0, st,
                         static_cast<const void*>(a.red_pairs), nullptr, a.grad, geom, a.red_nb,
                         a.red_out, a.red_inv, a.wpull, a.S, sg, masks, a.red_vmax, dup);
    }
    if (kMvm && a.mdup.rec && a.red_out) launch_mdup(a, NV, st);  // (rows with a repeated field)
    return;
  }
  if (split) hipLaunchKernelGGL((k_fm_std_red<D, BLOCK, false, true, kMvm>), dim3(groups), dim3(BLOCK), 0, st, a);
  else hipLaunchKernelGGL((k_fm_std_red<D, BLOCK>), dim3(groups), dim3(BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_red_scan, dim3(a.red_nb), dim3(kBlock), 0, st, a.red_hist, groups,
                     a.red_tot, geom, red_shift(NV));
  u32* start = a.red_tot + a.red_nb + 1;
  hipLaunchKernelGGL((k_red_scatter<NV, VecRedRec<NV>>), dim3(groups), dim3(kRedBlock), 0, st,
                     a.batch, BLOCK, static_cast<const void*>(a.red_pairs), a.red_count,
                     a.red_hist, a.red_tot, start, a.red_nb, static_cast<void*>(a.red_sorted),
                     geom);
  hipLaunchKernelGGL((k_red_sum_vec<D, false, kSegMaxGroups, kMvm>), dim3(grid), dim3(kRedBlock), 0, st,
                     static_cast<const void*>(a.red_sorted), start, a.grad, geom, a.red_nb,
                     a.red_out, a.red_inv, a.wpull, a.S, SegSrc{}, masks, a.red_vmax, dup);
  if (kMvm && a.mdup.rec && a.red_out) launch_mdup(a, NV, st);  // (rows with a repeated field)
}
#define XF_VEC_RED(D)                                                       \
  template void launch_vec_reduction<D, false>(const FwdArgs&, hipStream_t); \
  template void launch_vec_reduction<D - 1, true>(const FwdArgs&, hipStream_t);
// (FM's v_dim; MVM's width 2.. as D - 1 -- width 1 has no vector reduction)
XF_VEC_RED(2) XF_VEC_RED(4) XF_VEC_RED(8) XF_VEC_RED(10) XF_VEC_RED(16) XF_VEC_RED(32)
template void launch_vec_reduction<1, false>(const FwdArgs&, hipStream_t);
#undef XF_VEC_RED

}  // namespace hip
}  // namespace xflow
