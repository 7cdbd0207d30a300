// xflow-amd: candidate pools (gfx950): R contexts scored against a resident
// pool of N candidates as one GEMM on the matrix cores.  docs/DESIGN.md §2.
//
// Both models decompose over the split of a row into a context r and a
// candidate i (PoolRowsArgs, backend.h): with c_x the model's own logit of a
// part alone, y(r, i) = c_r + c_i + g * <u_r, u_i>, where u is empty (LR), the
// latent sums vs[0..D) (standard FM, g = 1) or their sum (reference FM, g = 2).
// A part is 1 + Dk floats, a pool an [N, W] matrix computed once per model
// version, and a request touches the table for its context's keys alone.
//
//   k_pool_rows_lr / k_pool_rows_fm<D>   rows -> vectors {c, u, +0.0f ..}
//     A workgroup of 4 waves, one wave per row.  Lane l takes the row's
//     occurrences l, l + 64, .. through the serve kernels' chunked probe
//     (chains, probe_limit, absent keys and lazy inits are theirs) and sums
//     them in ascending order from 0.0f; rank_allsum's fixed butterfly leaves
//     the row's sums, the same bits, in every lane; lane 0 finishes them as
//     the model finishes a row (rank_fm_finish) and lane j < W stores word j
//     (the sums are in every lane: one coalesced store per row in place of
//     lane 0's W).  A vector is a
//     function of the row's keys in their order alone.
//
//   k_pool_score<KP>   pctr[R][N] = sigmoid_ref(A x B), v_mfma_f32_32x32x2_f32
//     A[q][..] = {g * u_q, c_q, 1, 0 ..}, B[..][i] = {u_i, 1, c_i, 0 ..}, K
//     padded with zeros on both sides to KP = Dk + 2 rounded up to the
//     instruction's 2.  A workgroup of 4 waves owns 128 consecutive candidates,
//     a wave 32 of them: its B operand (lane l: candidate l % 32, k = 2s + l / 32)
//     is read from global memory once into KP / 2 registers and kept.  The
//     workgroup walks blocks of 32 requests: their A operand is staged in LDS
//     as [k][32] (a wave's read of one k is 32 consecutive floats, no bank
//     conflict) and every wave runs KP / 2 MFMAs into its 32 x 32 accumulator.
//     M = requests, N = candidates: accumulator register v of a lane is the
//     score of request 8 * (v / 4) + 4 * (l / 32) + v % 4 against candidate
//     l % 32, so each register is stored by 32 lanes as 32 consecutive floats
//     of one request's row.  The epilogue is sigmoid_ref on the registers whose
//     request exists; padded requests and candidates are computed and never
//     stored (their epilogue is skipped: it costs more than the product).
//     The request blocks are also spread over gridDim.y, so that a small pool
//     under many requests still fills the device; which workgroup computes a
//     block changes no bit.
//     An element is the chain acc = fma(A[q][k], B[k][i], acc) over k = 0 ..
//     KP - 1 from 0.0f inside the matrix unit: it depends on its own request
//     row and candidate column alone, never on R, N, the tile or the rest of
//     the call.  Out-of-range rows read nothing and store nothing.
// No atomics, no scratch memory.
#include "pool_common.h"
#include "rank_common.h"

namespace xflow {
namespace hip {

constexpr int kPoolTileN = 128;    // candidates per workgroup of k_pool_score
constexpr int kPoolTargetGrid = 2048;  // workgroups wanted before gridDim.y stops growing

__global__ void __launch_bounds__(kPoolRowWaves * kWave) k_pool_rows_lr(PoolRowsArgs a) {
  const int lane = threadIdx.x % kWave;
  const int64_t r = (int64_t)blockIdx.x * kPoolRowWaves + threadIdx.x / kWave;
  if (r >= a.batch.rows) return;  // (wave-uniform)
  float wx = 0.0f;
  serve_lr_sum(a.table, a.batch.keys, pool_lane_span(row_span(a.batch, r), lane), wx);
  wx = rank_allsum(wx);
  constexpr int W = 4;
  if (lane < W) a.vec[r * W + lane] = lane == 0 ? wx : 0.0f;
}

template <int D>
__global__ void __launch_bounds__(kPoolRowWaves * kWave) k_pool_rows_fm(PoolRowsArgs a) {
  const int lane = threadIdx.x % kWave;
  const int64_t r = (int64_t)blockIdx.x * kPoolRowWaves + threadIdx.x / kWave;
  if (r >= a.batch.rows) return;  // (wave-uniform)
  float vs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) vs[k] = 0.0f;
  float wx = 0.0f, vp = 0.0f;
  rank_fm_sum<D>(a.table, a.opt, a.batch.keys, pool_lane_span(row_span(a.batch, r), lane), wx, vs,
                 vp);
  pool_rows_fm_store<D>(a, r, lane, wx, vs, vp);
}

template <int KP>
__global__ void __launch_bounds__(kBlock) k_pool_score(PoolScoreArgs a, int W, int Dk, float g) {
  static_assert(KP % 2 == 0 && kBlock / kWave * 32 == kPoolTileN, "K steps of 2; 4 waves x 32");
  constexpr int KS = KP / 2;
  __shared__ float s_a[KP * kPoolTileM];  // [k][request of the block]
  const int lane = threadIdx.x % kWave, j = lane & 31, h = lane >> 5;
  const int64_t n = (int64_t)blockIdx.x * kPoolTileN + (threadIdx.x / kWave) * 32 + j;
  const bool n_on = n < a.N;
  float bv[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    bv[s] = n_on ? pool_operand(a.pool + n * W, 2 * s + h, Dk, false, g) : 0.0f;
  const int64_t blocks = (a.R + kPoolTileM - 1) / kPoolTileM;
  for (int64_t rb = blockIdx.y; rb < blocks; rb += gridDim.y) {  // (uniform trip count)
    const int64_t r0 = rb * kPoolTileM;
    __syncthreads();  // the block before is read
    for (int e = threadIdx.x; e < KP * kPoolTileM; e += kBlock) {
      const int64_t r = r0 + (e & 31);
      s_a[e] = r < a.R ? pool_operand(a.ctx + r * W, e >> 5, Dk, true, g) : 0.0f;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[(2 * s + h) * kPoolTileM + j], bv[s], acc, 0,
                                                 0, 0);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t r = r0 + 8 * (v / 4) + 4 * h + (v % 4);
      if (r < a.R && n_on) a.pctr[r * a.N + n] = sigmoid_ref(acc[v]);
    }
  }
}

void launch_pool_rows(const PoolRowsArgs& a, hipStream_t st) {
  if (!pool_check(a)) return;
  if (a.spec.n != 0) return launch_pool_rows_cross(a, st);  // kernels_pool_cross.hip
  const dim3 g((unsigned)((a.batch.rows + kPoolRowWaves - 1) / kPoolRowWaves));
  const dim3 blk(kPoolRowWaves * kWave);
  if (a.model.kind == kLR) {
    hipLaunchKernelGGL(k_pool_rows_lr, g, blk, 0, st, a);
  } else {
    switch (a.model.kernel_dim()) {
#define XF_POOL_CASE(DD) \
  case DD: hipLaunchKernelGGL(k_pool_rows_fm<DD>, g, blk, 0, st, a); break;
      XF_POOL_CASE(1) XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(8) XF_POOL_CASE(10)
      XF_POOL_CASE(16) XF_POOL_CASE(32)
#undef XF_POOL_CASE
      default:
        throw std::runtime_error("pool_rows: unsupported v_dim (1,2,4,8,10,16,32)");
    }
  }
  XF_HIP_CHECK(hipGetLastError());
}

void launch_pool_score(const PoolScoreArgs& a, hipStream_t st) {
  if (!pool_check(a)) return;
  const int Dk = pool_dk(a.model), W = pool_width(a.model);
  const float g = pool_gain(a.model);
  const int64_t gx = (a.N + kPoolTileN - 1) / kPoolTileN;
  const int64_t blocks = (a.R + kPoolTileM - 1) / kPoolTileM;
  const int64_t gy = std::min<int64_t>(std::min<int64_t>(blocks, 65535),
                                       std::max<int64_t>(1, kPoolTargetGrid / gx));
  const dim3 grid((unsigned)gx, (unsigned)gy), blk(kBlock);
  switch ((Dk + 2 + 1) & ~1) {
#define XF_POOL_CASE(KP) \
  case KP: hipLaunchKernelGGL(k_pool_score<KP>, grid, blk, 0, st, a, W, Dk, g); break;
    XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(6) XF_POOL_CASE(10) XF_POOL_CASE(12)
    XF_POOL_CASE(18) XF_POOL_CASE(34)
#undef XF_POOL_CASE
    default:
      throw std::runtime_error("pool_score: unsupported v_dim (1,2,4,8,10,16,32)");
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
