// xflow-amd: candidate pools of models with feature crosses (gfx950): the
// kernels of PoolRowsArgs and PoolSubsetArgs with spec.n > 0.  docs/DESIGN.md §2.
//
// A pair (request q, pool row n) is scored as the model scores the row context
// ++ candidate ++ the spec's cross keys of that row.  The pool's decomposition
// survives: the base is k_pool_subset's chain on the two resident vectors, and
// a cross adds terms of its own table entry alone (PoolSubsetArgs, backend.h).
// A cross whose fields all occur in the context is folded into the context's
// vector once per request; any other costs the pair a few operand reads, one
// hash and one probe.  What the kernels need of a row beside its vector is
// its operand row (row_operands): 1 + nu u64 words, the `seen` mask and the
// raw key of the first occurrence of every distinct operand field (CrossMap).
//
//   k_pool_rows_lr_x / k_pool_rows_fm_x<D>   rows -> vectors and operand rows
//     k_pool_rows_*'s design: a workgroup of 4 waves, a wave per row, lane l
//     sums occurrences l, l + 64, .. through the serve kernels' chunked probe.
//     Operands: per chunk of 64 occurrences lane l loads the field id of
//     occurrence j0 + l; a ballot per distinct field not seen yet gives the
//     chunk's lowest matching lane, i.e. the first occurrence (chunks ascend),
//     and lane u keeps field u's index.  The walk ends with the row or when
//     every field is seen.  Lane u < nu then loads that key and stores word
//     1 + u, lane 0 stores the mask.  fold: lane j, j below the number of
//     complete crosses, collects the j-th complete cross's operands from the
//     lanes that hold them (shuffles), hashes it and adds its probe to its own
//     partial before rank_allsum, as k_rank_*_x continues the context partial.
//     Without fold the sums, the butterfly, the finish and the store are
//     k_pool_rows_*'s: the same bits.  LDS: 16 keys per wave, 512 B.
//
//   k_pool_subset_lr_x / k_pool_subset_fm_x<D, STD, STAGE>
//     k_pool_subset's geometry and request walk: 256 threads take 256
//     consecutive entries, a wave 64, a lane one; the wave finds the request
//     of its first entry by binary search and walks on.  q comes from the
//     walk's counter and an index outside [0, N) or an entry no request owns
//     reads nothing and stores +0.0f: no value of req_ptr or index is an
//     address unchecked.
//     The steps run in the order 2, 3, 4, 1, 5: the probe keeps up to four
//     slots of 36 words in registers and the vectors take 2 W more, so the
//     vectors are read once the probes are done (D = 32: 2 waves per SIMD
//     instead of 1); no value depends on the order.
//     1. vectors   as k_pool_subset reads them, staged through the wave's LDS
//        region or direct; the base chain is its chain.
//     2. operands  the context's operand row is read by the lane itself
//        (lanes of a request share the address).  The pool's rows are a gather
//        of 64 random rows of 8 (1 + nu) bytes: from 1 + nu = 3 words on they
//        go through the wave's region as the vectors do -- word t = lane + 64 j
//        belongs to row t / (1 + nu), so consecutive lanes read consecutive
//        words of one row -- and lane l reads row l back.  Rows are kept at an
//        odd stride of 8-byte words: no bank conflict on the way back.  A
//        region holds 1024 words, so G = min(64, 1024 / stride) rows go per
//        pass (all 64 up to 15 fields; 15 at the 64 fields of a full spec) and
//        only the lanes of a pass hash.  The vectors reuse the region behind
//        the last pass's barrier.  Every barrier is reached by every thread.
//     3. keys      the lane hashes its incomplete crosses in spec order into
//        its column of the wave's xk[c][lane], lane-consecutive 8-byte words.
//     4. probes    that column is a RowSpan of step 64 through serve_lr_sum /
//        rank_fm_sum<D>: eight probes in flight (four for D > 10), chains,
//        probe_limit, absent keys and lazy inits are theirs.  The sums start
//        from 0.0f apart from the base.
//     5. finish    PoolSubsetArgs' formula, sigmoid_ref, a coalesced store.
// An element depends on its own context row, pool row and the table alone.
// VALU, not the matrix cores, for kernels_pool_subset.hip's reason: a wave's
// entries are unrelated pairs.  No atomics, no scratch memory.
// LDS (dynamic) per workgroup: 2 KB per cross for xk, plus four regions of
// max(256 W bytes if the vectors are staged, 8 * G * stride): 16 crosses over
// 64 fields at W = 36 take 32 KB + 36 KB, over the 64 KB a launch gets without
// asking, so that one case reads its vectors directly (the same bits) and
// takes 32 KB + 32 KB: 2 workgroups per CU's 160 KB.  13 pair crosses over 26
// fields: 26 KB + 32 KB (W = 36: 36 KB), 2 per CU; one pair cross at W = 12:
// 2 KB + 6 KB, where registers set the occupancy, not LDS.
#include "pool_common.h"

namespace xflow {
namespace hip {

constexpr int kPoolOpsRegionWords = 1024;  // u64 words of a wave's operand staging region

// The operand row of the wave's row r, stored to a.ops: returns the `seen`
// mask (wave-uniform); myop is this lane's word (lane u < nu: field u's).
__device__ __forceinline__ u64 pool_row_operands(const PoolRowsArgs& a, const CrossMap& m,
                                                 int64_t r, int lane, u64& myop) {
  const BatchView& b = a.batch;
  const RowSpan rs = row_span(b, r);
  const u64 all = m.nu >= 64 ? ~0ull : (1ull << m.nu) - 1ull;
  u64 seen = 0;
  int first = -1;  // lane u: the index of field u's first occurrence
  for (int j0 = 0; j0 < rs.len && seen != all; j0 += kWave) {
    const int32_t g = j0 + lane < rs.len ? b.fgid[rs.at(j0 + lane)] : -1;  // (operand fields are >= 0)
    for (int u = 0; u < m.nu; ++u) {
      if ((seen >> u) & 1ull) continue;
      const u64 hit = __ballot(g == m.ufield[u]);
      if (hit) {
        seen |= 1ull << u;
        if (lane == u) first = j0 + __builtin_ctzll(hit);
      }
    }
  }
  myop = first >= 0 ? b.keys[rs.at(first)] : kNoGroup;
  u64* out = a.ops + r * (int64_t)(1 + m.nu);
  if (lane < m.nu) out[1 + lane] = myop;
  if (lane == 0) out[0] = seen;
  return seen;
}

// fold: lane j below the number of complete crosses hashes the j-th of them
// into cxk[j] (the wave's 16 keys); returns the lane's span there
__device__ __forceinline__ RowSpan pool_row_fold(const PoolRowsArgs& a, const CrossMap& m, u64 seen,
                                                 u64 myop, int lane, u64* cxk) {
  const CrossSpec& x = a.spec;
  int ncomp = 0, myc = -1;
  for (int c = 0; c < x.n; ++c) {
    const u64 need = cross_need(x, m, c);
    if ((seen & need) == need) {
      if (lane == ncomp) myc = c;
      ++ncomp;
    }
  }
  const int cc = myc >= 0 ? myc : 0;
  u64 ops[kMaxCrossArity];
  int32_t fs[kMaxCrossArity];
#pragma unroll
  for (int k = 0; k < kMaxCrossArity; ++k) {  // (every lane shuffles)
    ops[k] = __shfl((unsigned long long)myop, (int)m.slot_u[kMaxCrossArity * cc + k]);
    fs[k] = x.field[cc][k];
  }
  RowSpan xs;
  xs.base = lane;
  xs.len = 0;
  if (myc >= 0) {  // (myc >= 0: lanes 0 .. ncomp - 1, ncomp <= 16)
    cxk[lane] = cross_key(fs, ops, x.arity[cc]);
    xs.len = 1;
  }
  return xs;
}

__global__ void __launch_bounds__(kPoolRowWaves * kWave) k_pool_rows_lr_x(PoolRowsArgs a,
                                                                          CrossMap m) {
  __shared__ u64 s_cxk[kPoolRowWaves * kMaxCrosses];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t r = (int64_t)blockIdx.x * kPoolRowWaves + wave;
  if (r >= a.batch.rows) return;  // (wave-uniform; no barrier below)
  float wx = 0.0f;
  serve_lr_sum(a.table, a.batch.keys, pool_lane_span(row_span(a.batch, r), lane), wx);
  u64 myop;
  const u64 seen = pool_row_operands(a, m, r, lane, myop);
  if (a.fold) {
    u64* cxk = s_cxk + wave * kMaxCrosses;
    const RowSpan xs = pool_row_fold(a, m, seen, myop, lane, cxk);
    serve_lr_sum(a.table, cxk, xs, wx);
  }
  wx = rank_allsum(wx);
  constexpr int W = 4;
  if (lane < W) a.vec[r * W + lane] = lane == 0 ? wx : 0.0f;
}

template <int D>
__global__ void __launch_bounds__(kPoolRowWaves * kWave) k_pool_rows_fm_x(PoolRowsArgs a,
                                                                          CrossMap m) {
  __shared__ u64 s_cxk[kPoolRowWaves * kMaxCrosses];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t r = (int64_t)blockIdx.x * kPoolRowWaves + wave;
  if (r >= a.batch.rows) return;  // (wave-uniform; no barrier below)
  float vs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  float wx = 0.0f, vp = 0.0f;
  rank_fm_sum<D>(a.table, a.opt, a.batch.keys, pool_lane_span(row_span(a.batch, r), lane), wx, vs,
                 vp);
  u64 myop;
  const u64 seen = pool_row_operands(a, m, r, lane, myop);
  if (a.fold) {
    u64* cxk = s_cxk + wave * kMaxCrosses;
    const RowSpan xs = pool_row_fold(a, m, seen, myop, lane, cxk);
    rank_fm_sum<D>(a.table, a.opt, cxk, xs, wx, vs, vp);
  }
  pool_rows_fm_store<D>(a, r, lane, wx, vs, vp);
}

// How a pool_subset launch with crosses uses its dynamic LDS
struct PoolCrossGeom {
  int stride = 0;   // u64 words between staged operand rows (odd); 0: every lane loads its own
  int G = kWave;    // operand rows of a wave per pass
  int region = 0;   // bytes of a wave's staging region
};

// D = 0: LR.  STD: standard FM (Dk = D), else reference FM (Dk = 1).
template <int D, bool STD, bool STAGE>
__global__ void __launch_bounds__(kBlock) k_pool_subset_x(PoolSubsetArgs a, CrossMap m,
                                                          PoolCrossGeom geo) {
  constexpr int Dk = D == 0 ? 0 : (STD ? D : 1), KP = (Dk + 3) & ~1;
  constexpr int W = pool_subset_width(KP), Q = W / 4;
  constexpr bool kStaged = STAGE && Q > 1;
  constexpr int DX = D > 0 ? D : 1;
  static_assert(Q == 1 || Q % 2 == 1 || Q == 2, "the swizzle covers Q = 2 only");
  extern __shared__ __align__(16) unsigned char pool_cross_mem[];
  const CrossSpec& x = a.spec;
  const float g = D > 0 && !STD ? 2.0f : 1.0f;  // pool_gain
  const int OW = 1 + m.nu;
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  u64* xk = reinterpret_cast<u64*>(pool_cross_mem) + (size_t)wave * x.n * kWave;  // [C][64]
  unsigned char* region = pool_cross_mem + (size_t)x.n * kBlock * 8 + (size_t)wave * geo.region;
  const int64_t w0 = (int64_t)blockIdx.x * kBlock + (int64_t)wave * kWave;  // the wave's first entry
  const int64_t e = w0 + lane;
  const int64_t wend = w0 + kWave < a.M ? w0 + kWave : a.M;

  // the request of this lane's entry (wave-uniform walk)
  int64_t q = -1;
  if (w0 < a.M) {
    int64_t l0 = 0, l1 = a.R;  // first request that ends past the wave's first entry
    while (l0 < l1) {
      const int64_t mid = (l0 + l1) >> 1;
      if ((int64_t)a.req_ptr[mid + 1] > w0) l1 = mid;
      else l0 = mid + 1;
    }
    for (int64_t r = l0; r < a.R; ++r) {
      const int64_t lo = a.req_ptr[r], hi = a.req_ptr[r + 1];
      if (lo >= wend) break;
      if (e >= lo && e < hi) q = r;
    }
  }
  int i = e < a.M ? a.index[e] : -1;  // -1: no row to read
  if (i < 0 || i >= a.N || q < 0) i = -1;

  // 2. and 3. the pool's operand rows, G of the wave's 64 per pass; the lanes
  // of a pass hash their incomplete crosses
  int nx = 0;
  const bool staged = geo.stride > 0;
  u64* srow = reinterpret_cast<u64*>(region);
  for (int g0 = 0; g0 < kWave; g0 += geo.G) {  // (uniform trip count)
    const int gn = kWave - g0 < geo.G ? kWave - g0 : geo.G;
    if (staged) {
      for (int t0 = 0; t0 < gn * OW; t0 += kWave) {  // (uniform: every lane shuffles)
        const int t = t0 + lane;
        const bool on = t < gn * OW;
        const int r = on ? t / OW : 0, w = t - r * OW;
        const int ri = __shfl(i, g0 + r);
        if (on) srow[r * geo.stride + w] = ri >= 0 ? a.pool_ops[(int64_t)ri * OW + w] : 0ull;
      }
      __syncthreads();
    }
    if (i >= 0 && lane >= g0 && lane < g0 + gn) {
      const u64* qrow = a.ctx_ops + q * OW;
      const u64* nrow = staged ? srow + (lane - g0) * geo.stride : a.pool_ops + (int64_t)i * OW;
      const u64 sq = qrow[0], sn = nrow[0];
      for (int c = 0; c < x.n; ++c) {
        const u64 need = cross_need(x, m, c);
        if ((sq & need) == need) continue;  // (inside the context's vector)
        u64 ops[kMaxCrossArity];
#pragma unroll
        for (int k = 0; k < kMaxCrossArity; ++k) {
          u64 v = kNoGroup;
          if (k < x.arity[c]) {
            const int u = m.slot_u[kMaxCrossArity * c + k];
            if ((sq >> u) & 1ull) v = qrow[1 + u];
            else if ((sn >> u) & 1ull) v = nrow[1 + u];
          }
          ops[k] = v;
        }
        xk[nx * kWave + lane] = cross_key(x.field[c], ops, x.arity[c]);
        ++nx;
      }
    }
    if (staged) __syncthreads();  // (the pass is read)
  }

  // 4. the probes of the lane's column, before the vectors are read: the
  // probe's slots and the vectors are never in registers together
  RowSpan xs;
  xs.base = lane;
  xs.step = kWave;
  xs.len = nx;
  float X[DX];
#pragma unroll
  for (int k = 0; k < DX; ++k) X[k] = 0.0f;
  float xw = 0.0f, xp = 0.0f;
  if constexpr (D == 0) serve_lr_sum(a.table, xk, xs, xw);
  else rank_fm_sum<D>(a.table, a.opt, xk, xs, xw, X, xp);

  // 1. the vectors and the base chain
  const float4* pool4 = reinterpret_cast<const float4*>(a.pool);
  float bv[W];
  if constexpr (kStaged) {
    float4* mine = reinterpret_cast<float4*>(region);  // (the operand passes end in a barrier)
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int t = lane + kWave * j, r = t / Q, p = t % Q;
      const int ri = __shfl(i, r);
      mine[pool_subset_slot<Q>(r, p)] =
          ri >= 0 ? pool4[(int64_t)ri * Q + p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // (every thread of the workgroup is here)
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const float4 v = mine[pool_subset_slot<Q>(lane, p)];
      bv[4 * p] = v.x, bv[4 * p + 1] = v.y, bv[4 * p + 2] = v.z, bv[4 * p + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const float4 v = i >= 0 ? pool4[(int64_t)i * Q + p] : make_float4(0.f, 0.f, 0.f, 0.f);
      bv[4 * p] = v.x, bv[4 * p + 1] = v.y, bv[4 * p + 2] = v.z, bv[4 * p + 3] = v.w;
    }
  }
  if (e >= a.M) return;  // (no barrier below)
  float out = 0.0f;
  if (i >= 0) {
    const float4* ctx4 = reinterpret_cast<const float4*>(a.ctx) + q * Q;
    float av[W];
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const float4 v = ctx4[p];
      av[4 * p] = v.x, av[4 * p + 1] = v.y, av[4 * p + 2] = v.z, av[4 * p + 3] = v.w;
    }
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < Dk + 2; ++k)  // (constant k: av and bv stay in registers)
      acc = __fmaf_rn(pool_operand(av, k, Dk, true, g), pool_operand(bv, k, Dk, false, g), acc);
    // 5. the finish (PoolSubsetArgs)
    float y;
    if constexpr (D == 0) {
      y = __fadd_rn(acc, xw);
    } else if constexpr (STD) {
      float t2 = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) t2 = __fmaf_rn(__fadd_rn(av[1 + k], bv[1 + k]), X[k], t2);
      y = __fadd_rn(__fadd_rn(acc, rank_fm_finish<DX>(kFmStandard, xw, X, xp)), t2);
    } else {
      float sx = 0.0f;  // (rank_fm_finish's own sum)
#pragma unroll
      for (int k = 0; k < D; ++k) sx = __fadd_rn(sx, X[k]);
      const float t2 = __fmul_rn(__fmul_rn(2.0f, __fadd_rn(av[1], bv[1])), sx);
      y = __fadd_rn(__fadd_rn(acc, rank_fm_finish<DX>(a.model.fm_math, xw, X, xp)), t2);
    }
    out = sigmoid_ref(y);
  }
  a.pctr[e] = out;
}

void launch_pool_rows_cross(const PoolRowsArgs& a, hipStream_t st) {
  const CrossMap m = cross_map(a.spec);
  const dim3 g((unsigned)((a.batch.rows + kPoolRowWaves - 1) / kPoolRowWaves));
  const dim3 blk(kPoolRowWaves * kWave);
  if (a.model.kind == kLR) {
    hipLaunchKernelGGL(k_pool_rows_lr_x, g, blk, 0, st, a, m);
  } else {
    switch (a.model.kernel_dim()) {
#define XF_POOL_CASE(DD) \
  case DD: hipLaunchKernelGGL(k_pool_rows_fm_x<DD>, g, blk, 0, st, a, m); break;
      XF_POOL_CASE(1) XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(8) XF_POOL_CASE(10)
      XF_POOL_CASE(16) XF_POOL_CASE(32)
#undef XF_POOL_CASE
      default:
        throw std::runtime_error("pool_rows: unsupported v_dim (1,2,4,8,10,16,32)");
    }
  }
  XF_HIP_CHECK(hipGetLastError());
}

template <int D, bool STD>
static void pool_subset_cross(const PoolSubsetArgs& a, const CrossMap& m, hipStream_t st) {
  constexpr int Dk = D == 0 ? 0 : (STD ? D : 1), W = pool_subset_width((Dk + 3) & ~1);
  PoolCrossGeom geo;
  const int OW = 1 + m.nu;
  if (OW >= 3) {
    geo.stride = OW | 1;
    geo.G = std::min(kWave, kPoolOpsRegionWords / geo.stride);
    geo.region = geo.G * geo.stride * 8;
  }
  const size_t xk = (size_t)a.spec.n * kBlock * 8;
  const int vec_region = kWave * W * 4;
  // (over the 64 KB of a plain launch: the vectors are read directly, the same bits)
  const bool stage = a.stage && W > 4 &&
                     xk + (size_t)(kBlock / kWave) * std::max(geo.region, vec_region) <= 64 * 1024;
  if (stage) geo.region = std::max(geo.region, vec_region);
  geo.region = (geo.region + 15) & ~15;
  const size_t lds = xk + (size_t)(kBlock / kWave) * geo.region;
  const dim3 grid((unsigned)((a.M + kBlock - 1) / kBlock)), blk(kBlock);
  if constexpr (W > 4) {
    if (stage) {
      hipLaunchKernelGGL((k_pool_subset_x<D, STD, true>), grid, blk, lds, st, a, m, geo);
      return;
    }
  }
  hipLaunchKernelGGL((k_pool_subset_x<D, STD, false>), grid, blk, lds, st, a, m, geo);
}

void launch_pool_subset_cross(const PoolSubsetArgs& a, hipStream_t st) {
  const CrossMap m = cross_map(a.spec);
  if (pool_width(a.model) != pool_subset_width((pool_dk(a.model) + 3) & ~1))
    throw std::runtime_error("pool_subset: unsupported v_dim (1,2,4,8,10,16,32)");
  if (a.model.kind == kLR) {
    pool_subset_cross<0, false>(a, m, st);
  } else {
    const bool standard = a.model.fm_math == kFmStandard;
    switch (a.model.kernel_dim()) {
#define XF_POOL_CASE(DD)                                  \
  case DD:                                                \
    if (standard) pool_subset_cross<DD, true>(a, m, st);  \
    else pool_subset_cross<DD, false>(a, m, st);          \
    break;
      XF_POOL_CASE(1) XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(8) XF_POOL_CASE(10)
      XF_POOL_CASE(16) XF_POOL_CASE(32)
#undef XF_POOL_CASE
      default:
        throw std::runtime_error("pool_subset: unsupported v_dim (1,2,4,8,10,16,32)");
    }
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
