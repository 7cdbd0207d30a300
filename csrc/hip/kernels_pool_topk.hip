// xflow-amd: candidate pools, top-k (gfx950): every context's best k candidates
// of a resident pool, selected next to the accumulators -- the R x N scores are
// never stored (PoolTopkArgs, backend.h; docs/DESIGN.md §2).
//
// A candidate's word is eval_key_bits(pctr) << 32 | ~index, the format
// k_topk_tile writes to its partial lists: unique within a request, descending
// word order is the order of TopkArgs, and 0 sorts below every real word (an
// index is below 2^31) and pads.  pctr is sigmoid_ref of k_pool_score's own
// chain: the same v_mfma_f32_32x32x2_f32 steps over the same pool_operand
// words in the same k order, so a score has the bits k_pool_score would have
// stored.  The selection is on that word, never on the logit.
//
//   k_pool_topk_strip<KP>   grid = groups of mq requests x strips of candidates
//     The roles of k_pool_score are swapped: the group's requests are staged
//     once in LDS as the A operand [k][32] (rows >= mq are zero and have no
//     epilogue -- the product is cheap, the lists are what is scarce) and the
//     strip streams past in steps of 128 candidates, 32 per wave: lane l reads
//     word 2s + l / 32 of candidate l % 32 into register s and the wave runs
//     the KP / 2 MFMAs.  With mq <= 8 the group's scores are accumulator
//     registers 0 .. 3: request 4 * (l / 32) + v against candidate l % 32.
//     lists   the group's requests share 4096 words of LDS, a region of
//             2^lg >= max(2 k, 512) words each (mq = 4096 >> lg: 8 up to k =
//             256, then 4, 2).  Words [0, k) of a region are the request's
//             best so far, sorted; [k, k + n) the survivors since (pending);
//             the rest are zeros or earlier losers -- real words of the same
//             request, which a later sort may see again without harm.  tau is
//             the region's word k - 1 at its last compress (0 before: fewer
//             than k seen).
//     filter  a word survives iff it is above its request's tau.  One ballot
//             per accumulator register gives both requests' survivor masks;
//             the waves' counts meet in s_cnt across one barrier, and a word
//             goes to pending[n + survivors of lower waves + survivors in
//             lower lanes]: a fixed place, no atomics.
//     compress  when a request's pending could overflow in the next step (n +
//             128 > region - k; from the counts alone, at a barrier) the
//             workgroup sorts, in one bitonic network over LDS, every region
//             that is more than half full, and each takes its new tau.
//     output  a last compress of every region with pending words; the first k
//             words of a region then go to partial[request][strip][0 .. k) --
//             or, with one strip, straight to idx / score.
//   k_pool_topk_merge   one workgroup per request: k_topk_merge's rounds over
//     topk_sort, the best k so far next to 4096 / k - 1 strip lists per round;
//     writes idx / score and their padding from the final words (the score is
//     the word's high half: sigmoid_ref returns a positive float or NaN, so a
//     key of 0 under a real word is a NaN).
// A word below tau can never be among its request's best k -- k larger words of
// the same request exist -- so every list holds exactly the best of what it
// has seen, whatever the strips, the groups or the grid; the merge sorts unique
// words.  No atomics, no float arithmetic after the epilogue, no scratch memory.
#include "kernels.h"
#include "pool_common.h"
#include "topk_common.h"

namespace xflow {
namespace hip {

namespace {

constexpr int kPtWords = kPoolTopkWords;
constexpr int kPtStep = kPoolTopkStep;
constexpr int kPtRows = 8;  // most requests of a group: regions of 512 words
constexpr int kPtRegs = 4;  // the accumulator registers that hold their scores
static_assert(kPtStep == kBlock / kWave * 32 && kPtWords == kTopkT && kPtRows == 2 * kPtRegs,
              "4 waves x 32 candidates; rows 4 * (l / 32) + v of registers v < 4");

struct PoolTopkLaunch {
  PoolTopkArgs a;
  int W, Dk;
  float g;
  int lg, mq;  // words per region 1 << lg, requests per group
  int64_t strip, strips;
};

// idx / score of a final word
__device__ __forceinline__ void pool_topk_store(const PoolTopkArgs& a, int64_t at, u64 w) {
  const u32 key = (u32)(w >> 32);
  a.idx[at] = w ? (int32_t)~(u32)w : -1;
  a.score[at] = __uint_as_float(w == 0 || key != 0 ? key : 0x7fc00000u);
}

// Sorts descending every region that holds more than half of its pending words
// (last: any), sets its tau and empties its pending list.  Every thread calls it.
__device__ __forceinline__ void pool_topk_compress(u64* s_list, int* s_n, u64* s_tau, int lg, int k,
                                                   bool last) {
  const int tid = threadIdx.x, region = 1 << lg, cap = region - k;
  for (int kk = 2; kk <= region; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
#pragma unroll
      for (int e = 0; e < kPtWords / 2 / kBlock; ++e) {  // (a region is 256 pairs or more: uniform)
        const int pr = e * kBlock + tid;
        const int i = ((pr & ~(jj - 1)) << 1) | (pr & (jj - 1));
        const int c = s_n[i >> lg];
        if (last ? c == 0 : 2 * c <= cap) continue;
        const bool desc = (i & (region - 1) & kk) == 0;
        const u64 x = s_list[i], y = s_list[i | jj];
        if ((x < y) == desc) {
          s_list[i] = y;
          s_list[i | jj] = x;
        }
      }
      __syncthreads();
    }
  }
  if (tid < kPtRows) {
    const int c = s_n[tid];
    if (last ? c != 0 : 2 * c > cap) {  // (never a row without a region: its count is 0)
      s_tau[tid] = s_list[(tid << lg) + k - 1];
      s_n[tid] = 0;
    }
  }
  __syncthreads();
}

template <int KP>
__global__ void __launch_bounds__(kBlock) k_pool_topk_strip(PoolTopkLaunch p) {
  static_assert(KP % 2 == 0, "K steps of 2");
  constexpr int KS = KP / 2;
  __shared__ u64 s_list[kPtWords];
  __shared__ float s_a[KP * kPoolTileM];  // [k][request of the group]
  __shared__ u64 s_tau[kPtRows];
  __shared__ int s_n[kPtRows];
  __shared__ int s_cnt[kBlock / kWave][kPtRows];
  const PoolTopkArgs& a = p.a;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, j = lane & 31, h = lane >> 5;
  const int64_t si = (int64_t)blockIdx.x % p.strips, r0 = (int64_t)blockIdx.x / p.strips * p.mq;
  const int cap = (1 << p.lg) - a.k;
  const int64_t n0 = si * p.strip;
  const int64_t n1 = n0 + p.strip < a.N ? n0 + p.strip : a.N;
  for (int e = tid; e < kPtWords; e += kBlock) s_list[e] = 0;
  for (int e = tid; e < KP * kPoolTileM; e += kBlock) {
    const int m = e & 31;
    s_a[e] = m < p.mq && r0 + m < a.R
                 ? pool_operand(a.ctx + (r0 + m) * p.W, e >> 5, p.Dk, true, p.g)
                 : 0.0f;
  }
  if (tid < kPtRows) {
    s_tau[tid] = 0;
    s_n[tid] = 0;
  }
  __syncthreads();
  for (int64_t nb = n0; nb < n1; nb += kPtStep) {  // (uniform trip count)
    const int64_t n = nb + wave * 32 + j;
    const bool n_on = n < n1;
    float bv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
      bv[s] = n_on ? pool_operand(a.pool + n * p.W, 2 * s + h, p.Dk, false, p.g) : 0.0f;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[(2 * s + h) * kPoolTileM + j], bv[s], acc, 0,
                                                 0, 0);
    u64 wd[kPtRegs];   // this lane's survivors (0: none)
    u32 mine[kPtRegs]; // the survivor mask of its request in this wave
    bool any = false;
#pragma unroll
    for (int v = 0; v < kPtRegs; ++v) {
      const int m = 4 * h + v;
      u64 w = 0;
      if (n_on && m < p.mq && r0 + m < a.R)
        w = (u64)eval_key_bits(sigmoid_ref(acc[v])) << 32 | (u32)~(u32)n;
      const bool keep = w > s_tau[m];  // (a real word is above 0)
      const u64 b = __ballot(keep);
      mine[v] = h ? (u32)(b >> 32) : (u32)b;
      if (j == 0) s_cnt[wave][m] = __popc(mine[v]);
      wd[v] = keep ? w : 0;
      any = any || b != 0;
    }
    __syncthreads();
    if (any) {  // (wave-uniform)
#pragma unroll
      for (int v = 0; v < kPtRegs; ++v) {
        if (wd[v] == 0) continue;
        const int m = 4 * h + v;
        int off = s_n[m] + __popc(mine[v] & ((1u << j) - 1u));
        for (int w2 = 0; w2 < wave; ++w2) off += s_cnt[w2][m];
        XF_DASSERT(off < cap);
        s_list[(m << p.lg) + a.k + off] = wd[v];
      }
    }
    __syncthreads();
    bool full = false;
    if (tid < kPtRows) {
      int t = s_n[tid];
#pragma unroll
      for (int w2 = 0; w2 < kBlock / kWave; ++w2) t += s_cnt[w2][tid];
      s_n[tid] = t;
      full = t + kPtStep > cap;  // the next step could overflow it
    }
    if (__syncthreads_or(full)) pool_topk_compress(s_list, s_n, s_tau, p.lg, a.k, false);
  }
  pool_topk_compress(s_list, s_n, s_tau, p.lg, a.k, true);
  for (int m = 0; m < p.mq && r0 + m < a.R; ++m) {
    const int64_t r = r0 + m;
    for (int e = tid; e < a.k; e += kBlock) {
      const u64 w = s_list[(m << p.lg) + e];
      if (p.strips == 1) pool_topk_store(a, r * a.k + e, w);
      else a.partial[(r * p.strips + si) * a.k + e] = w;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_pool_topk_merge(PoolTopkArgs a, int64_t strips) {
  __shared__ u64 lds[kTopkT];
  const int64_t q = blockIdx.x;
  const u32 k = (u32)a.k, S = (u32)kTopkT / k;  // (>= 4)
  const u64* lists = a.partial + q * strips * k;
  const u32 rel0 = threadIdx.x * kTopkPer;
  u64 v[kTopkPer];
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e) v[e] = 0;
  // words [0, k): the best so far; [s k, (s + 1) k), s >= 1: the list of strip sb + s - 1
  for (int64_t sb = 0; sb < strips; sb += S - 1) {
    const int64_t n = strips - sb < (int64_t)(S - 1) ? strips - sb : (int64_t)(S - 1);
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e) {
      const u32 p = rel0 + e, s = p / k, off = p - s * k;
      if (s == 0) continue;
      v[e] = (int64_t)s <= n ? lists[(sb + s - 1) * k + off] : 0;
    }
    topk_sort(v, topk_pow2((n + 1) * (int64_t)k), lds);
  }
#pragma unroll
  for (int e = 0; e < kTopkPer; ++e)
    if (rel0 + e < k) pool_topk_store(a, q * k + rel0 + e, v[e]);
}

}  // namespace

void launch_pool_topk(const PoolTopkArgs& a, hipStream_t st) {
  if (!pool_check(a)) return;
  const PoolTopkGeom g = pool_topk_geom(a.R, a.N, a.k, a.strip);
  if (g.strips > 1 && !a.partial)
    throw std::runtime_error("pool_topk: more than one strip needs the scratch");
  if (g.groups > 0x7fffffffll / g.strips)
    throw std::runtime_error("pool_topk: too many workgroups (requests / group * strips)");
  PoolTopkLaunch p;
  p.a = a;
  p.W = pool_width(a.model);
  p.Dk = pool_dk(a.model);
  p.g = pool_gain(a.model);
  p.lg = g.lg_region;
  p.mq = g.mq;
  p.strip = g.strip;
  p.strips = g.strips;
  const dim3 grid((unsigned)(g.groups * g.strips)), blk(kBlock);
  switch ((p.Dk + 2 + 1) & ~1) {
#define XF_POOL_CASE(KP) \
  case KP: hipLaunchKernelGGL(k_pool_topk_strip<KP>, grid, blk, 0, st, p); break;
    XF_POOL_CASE(2) XF_POOL_CASE(4) XF_POOL_CASE(6) XF_POOL_CASE(10) XF_POOL_CASE(12)
    XF_POOL_CASE(18) XF_POOL_CASE(34)
#undef XF_POOL_CASE
    default:
      throw std::runtime_error("pool_topk: unsupported v_dim (1,2,4,8,10,16,32)");
  }
  if (g.strips > 1)
    hipLaunchKernelGGL(k_pool_topk_merge, dim3((unsigned)a.R), blk, 0, st, a, g.strips);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
