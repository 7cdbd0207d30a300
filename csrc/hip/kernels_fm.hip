// xflow-amd: FM forward + backward and its dispatch (gfx950): the full-row
// kernel (k_fm), the reference-math producers of the scalar reduction
// (k_fm_red, k_fm_vals) and the matrix-core forward (k_fm_fwd_mfma).  The
// standard-math producers (k_fm_std_red, k_fm_std_fwd) live with their
// launcher in kernels_reduce_vec.hip.
// Reference math: fm_worker.cc:159-202 (loss), :126-157 (gradient)  [kFmReference]
#include "model_common.h"

namespace xflow {
namespace hip {

// FM: one lane per row; the pulled row [w, v_0..v_{D-1}, pad] is read as
// PS/4 dwordx4 loads.  Backward: the P = 1+D gradient components of every
// occurrence are summed per (key, slice) exactly in the per-column LDS tables
// (vector accumulators), then flushed with one global atomic per non-zero
// component -- hot keys cost one atomic per workgroup instead of one per row.
template <int D, bool kGrad, bool kAgg>
__global__ void __launch_bounds__(fm_block(D)) k_fm(FwdArgs a) {
  constexpr int PS = fm_ps(D);
  constexpr int BLOCK = fm_block(D);
  constexpr int LOG2 = ilog2c(2 * BLOCK);
  __shared__ u32 s_tag[kAgg ? 2 : 1][kAgg ? (1 << LOG2) : 1];
  __shared__ float s_acc[kAgg ? 2 : 1][kAgg ? (1 << LOG2) * PS : 1];
  __shared__ int s_maxlen;
  const BatchView& b = a.batch;
  const bool standard = a.model.fm_math == kFmStandard;
  const u32* __restrict__ pos = a.pos;
  const float4* __restrict__ wp4 = reinterpret_cast<const float4*>(a.wpull);
  int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool active = r < b.rows;
  RowSpan rs;
  StatAcc st;
  float loss = 0.0f, vsum = 0.0f;
  float vs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  if (active) {
    rs = row_span(b, r);
    float wx = 0.0f, vp = 0.0f;
    for (int j = 0; j < rs.len; ++j) {
      float w[PS];
      const float4* src = wp4 + (size_t)pos[rs.at(j)] * (PS / 4);
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) {
        float4 v4 = src[q];
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
    float y;
    if (standard) {
      float sq = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) sq += vs[k] * vs[k];
      y = wx + 0.5f * (sq - vp);
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) vsum += vs[k];
      y = wx + (vsum * vsum - vp);
    }
    float p = sigmoid_ref(y);
    float lab = b.labels[r];
    loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
  }
  if (kGrad) {
    const u32 s = active ? (u32)slice_of(b, r, a.S) : 0u;
    const u32 S = (u32)a.S;
    const float gw = standard ? loss : loss * (float)a.model.v_dim;  // (real D: padded dims are inert)
    auto contrib = [&](u32 p, float* c) {
      const float4* src = wp4 + (size_t)p * (PS / 4);
      float w[PS];
#pragma unroll
      for (int q = 0; q < PS / 4; ++q) {
        float4 v4 = src[q];
        w[4 * q] = v4.x;
        w[4 * q + 1] = v4.y;
        w[4 * q + 2] = v4.z;
        w[4 * q + 3] = v4.w;
      }
      c[0] = gw;
#pragma unroll
      for (int k = 0; k < D; ++k) c[1 + k] = loss * ((standard ? vs[k] : vsum) - w[1 + k]);
    };
    if constexpr (!kAgg) {
      for (int j = 0; j < rs.len; ++j) {
        const u32 p = pos[rs.at(j)];
        float c[1 + D];
        contrib(p, c);
        float* g = a.grad + ((size_t)p * S + s) * PS;
#pragma unroll
        for (int k = 0; k < 1 + D; ++k) atomicAdd(&g[k], c[k]);
      }
    } else {
      ColumnAgg<PS, LOG2> agg{s_tag, s_acc};
      if (threadIdx.x == 0) s_maxlen = 0;
      agg.init();
      __syncthreads();
      const int len = rs.len;
      if (len > 0) atomicMax(&s_maxlen, len);
      __syncthreads();
      const int maxlen = s_maxlen;
      for (int j = 0; j < maxlen; ++j) {
        const int t = j & 1;
        if (j < len) {
          const u32 p = pos[rs.at(j)];
          float c[1 + D];
          contrib(p, c);
          const int h = agg.insert(t, p * S + s);
#pragma unroll
          for (int k = 0; k < 1 + D; ++k) agg.add(t, h, k, c[k]);
        }
        __syncthreads();
        agg.flush(t, a.grad);
      }
    }
  }
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
}

// Reference-math FM on the atomic-free reduction path.  The gradient of key i
// in row r is loss_r*D for w and loss_r*(vsum_r - v_ik) for v (fm_worker.cc:
// 126-157), so per (key, slice) only B = Σ loss and C = Σ loss*vsum need
// summing -- two LDS atomics per occurrence instead of 1+D -- and k_red_sum
// expands them with the pulled v: g_w = D*B, g_v[k] = C - v_k*B.
template <int D, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_fm_red(FwdArgs a) {
  constexpr int PS = fm_ps(D);
  constexpr int LOG2 = ilog2c(2 * BLOCK);
  __shared__ u32 s_tag32[2][1 << LOG2];
  __shared__ long long s_acc[2][(1 << LOG2) * 2];
  __shared__ unsigned short s_list[2][BLOCK];
  __shared__ u32 s_hist[kRedMaxBuckets];
  __shared__ u32 s_nlist[3];
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
  u64* region = reinterpret_cast<u64*>(reinterpret_cast<uint3*>(a.red_pairs) +
                                       (b.row_ptr ? (int64_t)b.row_ptr[r0]
                                                  : r0 * b.nnz_per_row));
  ListAgg<LOG2, 2> lagg{s_tag32, s_acc, s_list, s_nlist, s_hist, region};
  lagg.init(red_active(a, red_shift(2)));
  lagg.shift = red_geom(a).shift(red_shift(2));
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
  StatAcc st;
  float loss = 0.0f, vsum = 0.0f;
  if (active) {
    float vs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) vs[k] = 0.0f;
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
#pragma unroll
    for (int k = 0; k < D; ++k) vsum += vs[k];
    const float p = sigmoid_ref(wx + (vsum * vsum - vp));
    const float lab = b.labels[r];
    loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
  }
  const u32 s = active ? (u32)slice_of(b, r, a.S) : 0u;
  const u32 S = (u32)a.S;
  const float lv = loss * vsum;
  PosStream ps(pos, rs, len, a.trash_pos);
  for (int j0 = 0; j0 < maxlen; j0 += kPosChunk) {
    ps.prefetch(j0 + kPosChunk);
#pragma unroll
    for (int q = 0; q < kPosChunk; ++q) {
      if (j0 + q >= maxlen) break;
      const u32 pj = ps.get(q);
      lagg.column(j0 + q, pj != a.trash_pos, pj * S + s, loss, lv);
    }
    ps.advance();
  }
  __syncthreads();
  if (threadIdx.x == 0) {
      a.red_count[blockIdx.x] = lagg.total();
      if (a.red_records) atomicAdd(a.red_records, (unsigned long long)lagg.total());
    }
  for (int i = threadIdx.x, n = red_active(a, red_shift(2)); i < n; i += BLOCK)
    a.red_hist[(size_t)i * gridDim.x + blockIdx.x] = s_hist[i];
  st.bad |= lagg.bad;
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
}

// Reference-math FM on compact value rows (FwdArgs::fm_vals): each feature's
// pulled row is (w, Σ_k v_k, Σ_k v_k^2, 0), one dwordx4 -- the reference's
// y = Σ w + (Σ_f Σ_k v)^2 - Σ_f Σ_k v^2 (fm_worker.cc:159-202) needs nothing
// else, and its backward only Σ loss and Σ loss*vsum per key (k_fm_red).
// A third of the gather traffic of the full-row kernel, independent of D.
template <int BLOCK, bool kGrad>
__global__ void __launch_bounds__(BLOCK) k_fm_vals(FwdArgs a) {
  // one column table of 4 x BLOCK slots (load <= 1/4: short probe chains) in
  // the LDS of two alternating 2 x BLOCK ones, at one more barrier per column
  constexpr int LOG2 = ilog2c(4 * BLOCK);
  __shared__ u32 s_tag32[1][kGrad ? (1 << LOG2) : 1];
  __shared__ long long s_acc[1][kGrad ? (1 << LOG2) * 2 : 1];
  __shared__ unsigned short s_list[1][kGrad ? (1 << LOG2) / 2 : 1];
  __shared__ u32 s_hist[kGrad ? kRedMaxBuckets : 1];
  __shared__ u32 s_nlist[3];
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
  ListAgg<LOG2, 2, 1> lagg{reinterpret_cast<u32(*)[1 << LOG2]>(&s_tag32[0][0]),
                           reinterpret_cast<long long(*)[(1 << LOG2) * 2]>(&s_acc[0][0]),
                           reinterpret_cast<unsigned short(*)[(1 << LOG2) / 2]>(&s_list[0][0]),
                           s_nlist, s_hist, nullptr};
  int maxlen = 0;
  if constexpr (kGrad) {
    lagg.region = reinterpret_cast<u64*>(reinterpret_cast<uint3*>(a.red_pairs) +
                                         (b.row_ptr ? (int64_t)b.row_ptr[r0] : r0 * b.nnz_per_row));
    lagg.init(red_active(a, red_shift(2)));
    lagg.shift = red_geom(a).shift(red_shift(2));
    if (!b.row_ptr) {
      maxlen = b.nnz_per_row;
      __syncthreads();
    } else {
      const int m = wave_max(len);
      if (threadIdx.x % kWave == 0) s_wmax[threadIdx.x / kWave] = m;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < BLOCK / kWave; ++w) maxlen = max(maxlen, s_wmax[w]);
    }
  }
  StatAcc st;
  float loss = 0.0f, vsum = 0.0f;
  if (active) {
    float wx = 0.0f, vp = 0.0f;
    int j = 0;
    for (; j + 4 <= len; j += 4) {  // four independent row loads in flight
      float4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = wp4[pos[rs.at(j + u)]];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wx += q[u].x;
        vsum += q[u].y;
        vp += q[u].z;
      }
    }
    for (; j < len; ++j) {
      const float4 q = wp4[pos[rs.at(j)]];
      wx += q.x;
      vsum += q.y;
      vp += q.z;
    }
    const float p = sigmoid_ref(wx + (vsum * vsum - vp));
    const float lab = b.labels[r];
    loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
  }
  if constexpr (kGrad) {
    const u32 s = active ? (u32)slice_of(b, r, a.S) : 0u;
    const u32 S = (u32)a.S;
    const float lv = loss * vsum;
    PosStream ps(pos, rs, len, a.trash_pos);
    for (int j0 = 0; j0 < maxlen; j0 += kPosChunk) {
      ps.prefetch(j0 + kPosChunk);
#pragma unroll
      for (int q = 0; q < kPosChunk; ++q) {
        if (j0 + q >= maxlen) break;
        const u32 pj = ps.get(q);
        lagg.column(j0 + q, pj != a.trash_pos, pj * S + s, loss, lv);
      }
      ps.advance();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      a.red_count[blockIdx.x] = lagg.total();
      if (a.red_records) atomicAdd(a.red_records, (unsigned long long)lagg.total());
    }
    for (int i = threadIdx.x, n = red_active(a, red_shift(2)); i < n; i += BLOCK)
      a.red_hist[(size_t)i * gridDim.x + blockIdx.x] = s_hist[i];
  }
  st.bad |= lagg.bad;
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
}

// ---------------------------------------------------------------------------
// Standard-math FM forward on the matrix cores (v_mfma_f32_16x16x4_f32), the
// row-indicator form of DESIGN.md section 6: a wave owns 16 rows; for every
// (row quad m, field f) one MFMA adds, for the 4 rows of the quad, the
// field's latent row v (columns 0..D-1) and its squares (columns D..2D-1) to
// the 16 x 16 accumulator tile D[row][column]:
//   A[i][q] = (i == 4m + q)       (one-hot: 4 of the 64 A entries are 1)
//   B[q][c] = v[row 4m+q, f][c], v^2[..][c - D]
// so D[i][k] = sum_f v_ik = vs_k and D[i][D+k] = sum_f v_ik^2, exact f32 adds
// in field order (fmaf chain).  y = sum_f w + 0.5 sum_k (vs_k^2 - sum_f v^2)
// (Rendle's sum trick; fm_math = standard).  An honest A/B against the VALU
// forward (one lane per row) -- see profiles/r2_fm_mfma_ab.txt: 15/16 of each
// MFMA's work multiplies by the zero entries of A, so the matrix-core form
// needs 4*F instructions per 16 rows where the VALU form spends F*D FMAs per
// row; both are bound by the gather of the pulled rows.
// Selected for forward-only standard FM with ModelSpec::fm_mfma.
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <int D>
__global__ void __launch_bounds__(256) k_fm_fwd_mfma(FwdArgs a) {
  static_assert(2 * D <= 16, "one 16-column tile: D <= 8");
  constexpr int PS = fm_ps(D);
  const BatchView& b = a.batch;
  const int lane = lane_id();
  const int q = lane >> 4, c = lane & 15;
  const int64_t r0 = ((int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) * 16;
  int F = b.nnz_per_row;
  if (b.row_ptr) {  // longest row of the wave's 16
    int len = 0;
    const int64_t r = r0 + (lane & 15);
    if (lane < 16 && r < b.rows) len = (int)(b.row_ptr[r + 1] - b.row_ptr[r]);
    F = wave_max(len);
  }
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float wx[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // lanes with c == 0: w sums of rows 4m+q
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int64_t row = r0 + 4 * m + q;
    RowSpan rs;
    if (row < b.rows) rs = row_span(b, row);
    const float av = (c == 4 * m + q) ? 1.0f : 0.0f;  // A[i = c][k = q]
    for (int f = 0; f < F; ++f) {
      float bv = 0.0f, w = 0.0f;
      if (f < rs.len) {
        const float* src = a.wpull + (size_t)a.pos[rs.at(f)] * PS;
        w = src[0];
        const float v = c < D ? src[1 + c] : (c < 2 * D ? src[1 + c - D] : 0.0f);
        bv = c < D ? v : v * v;
      }
      wx[m] += w;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
  }
  // D[row = 4*(lane>>4) + reg][col = lane & 15]: per row, sum over the 16 columns
  float t[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float x = acc[reg];
    t[reg] = c < D ? x * x : (c < 2 * D ? -x : 0.0f);
  }
  // (vs_k^2 terms first, then the squares: same association on every lane)
#pragma unroll
  for (int o = 1; o < 16; o <<= 1)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) t[reg] += __shfl_xor(t[reg], o);
  // lane 16*g + 0 holds rows 4g .. 4g+3; their w sums sit in lanes (q = reg, c = 0), index m = g
  StatAcc st;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int g = lane >> 4;
    float wxs = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float x = __shfl(wx[m], 16 * reg);  // lane (q = reg, c = 0)
      if (m == g) wxs = x;
    }
    const int64_t row = r0 + 4 * g + reg;
    if (c == 0 && row < b.rows) {
      const float p = sigmoid_ref(wxs + 0.5f * t[reg]);
      const float lab = b.labels[row];
      if (a.pctr) a.pctr[row] = p;
      st.add(p, lab);
    }
  }
  flush_stats<256>(st, a.stats, a.fx_bad);
}

template <bool kGrad>
void dispatch_fm(const FwdArgs& a, hipStream_t st) {
  const bool agg = kGrad && a.agg_ok;
  const bool red = kGrad && a.model.fm_math == kFmReference && red_path(a, kRedMaxBuckets);
  if (a.fm_compact && !red) throw std::runtime_error("fm_compact needs the FM reduction path");
  if (a.red_masks && a.S > 1 && a.model.fm_math == kFmReference && !red)
    throw std::runtime_error("red_masks need the FM reduction path");
  if (!kGrad && a.model.fm_math == kFmStandard && a.model.fm_mfma) {
    const int g = (int)((a.batch.rows + 63) / 64);  // 4 waves x 16 rows
    switch (a.model.kernel_dim()) {
      case 1: hipLaunchKernelGGL(k_fm_fwd_mfma<1>, dim3(g), dim3(256), 0, st, a); break;
      case 2: hipLaunchKernelGGL(k_fm_fwd_mfma<2>, dim3(g), dim3(256), 0, st, a); break;
      case 4: hipLaunchKernelGGL(k_fm_fwd_mfma<4>, dim3(g), dim3(256), 0, st, a); break;
      case 8: hipLaunchKernelGGL(k_fm_fwd_mfma<8>, dim3(g), dim3(256), 0, st, a); break;
      default: throw std::runtime_error("FM MFMA forward: v_dim 1, 2, 4 or 8");
    }
    return;
  }
  if (a.fm_vals) {
    if (a.model.fm_math != kFmReference) throw std::runtime_error("fm_vals: reference math only");
    constexpr int R = kFmGroupRows;
    const int gr = (int)((a.batch.rows + R - 1) / R);
    if (kGrad) {
      if (!red || !a.fm_compact) throw std::runtime_error("fm_vals: needs the compact reduction");
      const int Rn = narrow_rows(a, R);
      const int gn = (int)((a.batch.rows + Rn - 1) / Rn);
      launch_rows(Rn, [&](auto r) {
        hipLaunchKernelGGL((k_fm_vals<decltype(r)::value, true>), dim3(gn), dim3(Rn), 0, st, a);
      });
      launch_reduction<2>(a, gn, Rn, st);
    } else {
      hipLaunchKernelGGL((k_fm_vals<R, false>), dim3(gr), dim3(R), 0, st, a);
    }
    return;
  }
  // standard math: per-component records through the LR reduction pipeline
  const bool red_std = kGrad && a.model.fm_math == kFmStandard && red_path(a, red_cap(a));
  if (a.red_masks && a.S > 1 && a.model.fm_math == kFmStandard && !red_std)
    throw std::runtime_error("red_masks need the standard-FM reduction path");
  if (a.red_out && a.model.fm_math == kFmStandard && !red_std)
    throw std::runtime_error("standard FM red_out needs the vector-record reduction");
  switch (a.model.kernel_dim()) {
#define XF_FM_CASE(DD)                                                                   \
  case DD: {                                                                             \
    constexpr int B = fm_block(DD);                                                      \
    int g = (int)((a.batch.rows + B - 1) / B);                                           \
    if (red_std) {                                                                       \
      launch_vec_reduction<DD>(a, st);                                                 \
    } else if (red) {                                                                    \
      constexpr int R = kFmGroupRows;                                                    \
      const int gr = (int)((a.batch.rows + R - 1) / R);                                  \
      hipLaunchKernelGGL((k_fm_red<DD, R>), dim3(gr), dim3(R), 0, st, a);                \
      launch_reduction<2>(a, gr, R, st);                                                 \
    } else if (agg) {                                                                    \
      hipLaunchKernelGGL((k_fm<DD, kGrad, true>), dim3(g), dim3(B), 0, st, a);           \
    } else {                                                                             \
      hipLaunchKernelGGL((k_fm<DD, kGrad, false>), dim3(g), dim3(B), 0, st, a);          \
    }                                                                                    \
    break;                                                                               \
  }
    XF_FM_CASE(1) XF_FM_CASE(2) XF_FM_CASE(4) XF_FM_CASE(8) XF_FM_CASE(10) XF_FM_CASE(16)
    XF_FM_CASE(32)
#undef XF_FM_CASE
    default:
      throw std::runtime_error("FM: unsupported v_dim (1,2,4,8,10,16,32)");
  }
}
template void dispatch_fm<true>(const FwdArgs&, hipStream_t);
template void dispatch_fm<false>(const FwdArgs&, hipStream_t);

}  // namespace hip
}  // namespace xflow
