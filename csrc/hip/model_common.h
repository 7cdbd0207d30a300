// xflow-amd: device code shared by the model kernels (kernels_lr / kernels_fm /
// kernels_mvm / kernels_reduce / kernels_reduce_vec / kernels_model .hip).
// Included by .hip files only.  The build has no relocatable device code, so
// every __device__ function a kernel calls is defined here or in the kernel's
// own file; the host launchers that cross files are declared at the end.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "kernels.h"
#include "hip_util.h"

namespace xflow {
namespace hip {

// Diagnostic build only (-DXFLOW_KTIMING): per-phase shader-clock cycles of
// the column-walk producers (k_fm_std_red, k_lr), summed over waves (each
// wave accumulates in registers, lane 0 adds them once), printed every 25
// launches (ktime_dump).  Each file that times a kernel has its own counters
// and reads them back in its own ktime_dump.
#ifdef XFLOW_KTIMING
static __device__ unsigned long long g_ktime[16];
#define XF_KT_DECL                  \
  unsigned long long kt_acc_[8] = {}; \
  unsigned long long kt_ = clock64()
#define XF_KT(p)                                  \
  do {                                            \
    const unsigned long long n_ = clock64();      \
    kt_acc_[p] += n_ - kt_;                       \
    kt_ = n_;                                     \
  } while (0)
#define XF_KT_FLUSH()                                                    \
  do {                                                                   \
    if (lane_id() == 0) {                                                \
      for (int p_ = 0; p_ < 8; ++p_) atomicAdd(&g_ktime[p_], kt_acc_[p_]); \
      atomicAdd(&g_ktime[15], 1ull);                                     \
    }                                                                    \
  } while (0)
static void ktime_dump(const char* what, int nphase, hipStream_t st) {
  static int calls = 0;
  if (++calls % 25) return;
  unsigned long long t[16];
  XF_HIP_CHECK(hipStreamSynchronize(st));
  XF_HIP_CHECK(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_ktime), sizeof(t)));
  const double w = (double)(t[15] ? t[15] : 1);
  std::fprintf(stderr, "[ktime] %s waves %llu  cycles/wave:", what, t[15]);
  for (int p = 0; p < nphase; ++p) std::fprintf(stderr, " p%d %.0f", p, t[p] / w);
  std::fprintf(stderr, "\n");
}
#else
#define XF_KT_DECL (void)0
#define XF_KT(p) (void)0
#define XF_KT_FLUSH() (void)0
#endif

// unique index of a gradient row: through the slot -> unique map, or the row
// itself when the positions already are unique indices (inv == null)
__device__ __forceinline__ u32 uix(const u32* inv, u64 x) { return inv ? inv[x] : (u32)x; }

__device__ __forceinline__ int slice_of(const BatchView& b, int64_t r, int S) {
  if (b.slice_rows <= 0) return 0;
  int64_t s = r / b.slice_rows;
  return (int)(s < S ? s : S - 1);
}

// Bucket geometry of this step's gradient reduction (FwdArgs::red_bcap):
// the smallest shift >= base that keeps ceil(dests / 2^shift) within
// kRedMaxBuckets, dests = (batch scratch capacity) * S.
// (kCsrVecMinShift: backend.h, next to Engine::red_geometry's host copy of shift())
struct RedGeom {
  const unsigned long long* bcap;
  u64 cap;
  int S;
  // unique-index positions (FwdArgs::red_nuq): dests = unique * S + s lie
  // below the batch's unique count times S
  const int64_t* nuq;
  int maxb;  // bucket cap (FwdArgs::red_maxb)
  int fx_head;  // scaled fixed point (MVM): fx_head_bits of the batch's rows
  // smallest bucket shift: the CSR vector reduction (k_red_csr_vec) takes
  // buckets of 2^kCsrVecMinShift dests -- fewer, fuller buckets amortise its
  // per-bucket phases, and the producer writes fewer per-bucket counts
  int min_shift;
  __device__ __forceinline__ u64 rows() const {
    return nuq ? (u64)*nuq : (bcap ? (u64)*bcap : cap);
  }
  __device__ __forceinline__ int shift(int base) const {
    const u64 dests = rows() * (u64)S;
    int sh = base;
    while (((dests + (1ull << sh) - 1) >> sh) > (u64)kRedMaxBuckets) ++sh;
    // a larger cap (vector records) only where a bucket would otherwise span
    // four or more LDS units: at two, the extra buckets' per-(bucket,
    // workgroup) counts and offsets cost more than the records' second read
    // (FM-8 std --slices 8 -1.2 %, --slices 64 +5.5 %: profiles/r4_negative_ab.txt)
    if (maxb > kRedMaxBuckets && sh - base >= 2)
      while (sh > base && ((dests + (1ull << (sh - 1)) - 1) >> (sh - 1)) <= (u64)maxb) --sh;
    return sh < min_shift ? min_shift : sh;
  }
  // buckets this step's dests reach (of the nb allocated for the full
  // capacity): producers, scans and sums skip the rest
  __device__ __forceinline__ int active(int shift, int nb) const {
    const u64 dests = rows() * (u64)S;
    const u64 n = (dests + (1ull << shift) - 1) >> shift;
    return n < (u64)nb ? (int)n : nb;
  }
};

__host__ __device__ inline RedGeom red_geom(const FwdArgs& a) {
  const int S = a.S;
  return RedGeom{a.red_bcap, a.red_cap, S, a.red_nuq, a.red_maxb > 0 ? a.red_maxb : kRedMaxBuckets,
                 fx_head_bits(a.batch.rows), a.red_csr.cnt && a.red_csr.ew > 0 ? kCsrVecMinShift : 0};
}

__device__ __forceinline__ int red_active(const FwdArgs& a, int base) {
  const RedGeom g = red_geom(a);
  return g.active(g.shift(base), a.red_nb);
}

// Per-row loss statistics, reduced per workgroup then one f64 atomic each.
struct StatAcc {
  double ln = 0, l2 = 0, rows = 0, pos = 0;
  u32 bad = 0;  // a non-finite / out-of-range prediction or gradient input (FwdArgs::fx_bad)
  __device__ void add(float p, float y) {
    bad |= !(p >= 0.0f && p <= 1.0f) ? 1u : 0u;
    float pc = fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f);
    ln += (y > 0.5f) ? -(double)logf(pc) : -(double)logf(1.0f - pc);
    l2 += (y > 0.5f) ? (double)log2f(p) : (double)log2f(1.0f - p);
    rows += 1.0;
    pos += (y > 0.5f) ? 1.0 : 0.0;
  }
};

template <int BLOCK>
__device__ void flush_stats(StatAcc a, LossStats* out, u32* bad_flag = nullptr) {
  if (bad_flag && __ballot(a.bad != 0u) && threadIdx.x % kWave == 0) atomicOr(bad_flag, 2u);
  if (!out) return;
  __shared__ double red[4][BLOCK / kWave];
  a.ln = wave_sum(a.ln);
  a.l2 = wave_sum(a.l2);
  a.rows = wave_sum(a.rows);
  a.pos = wave_sum(a.pos);
  int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
  if (l == 0) {
    red[0][w] = a.ln;
    red[1][w] = a.l2;
    red[2][w] = a.rows;
    red[3][w] = a.pos;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double s = 0;
    for (int i = 0; i < BLOCK / kWave; ++i) s += red[threadIdx.x][i];
    double* dst = threadIdx.x == 0 ? &out->ln_loss
                  : threadIdx.x == 1 ? &out->log2_lik
                  : threadIdx.x == 2 ? &out->rows
                                     : &out->positives;
    if (s != 0.0) atomicAdd(dst, s);
  }
}

// Exact per-column gradient aggregation in LDS.
//
// CTR keys are heavily skewed: in the Criteo-shaped batch the top 1000 keys
// carry ~60% of all occurrences, so per-occurrence global float atomics
// serialise on a few hot addresses.  The backward therefore walks a workgroup's
// rows column by column (occurrence j of every row = field j for fixed-width
// CTR rows and for field-ordered libffm lines): a column has at most kBlock
// occurrences, which are summed exactly in an LDS open-addressing table of
// 2*kBlock slots (load <= 0.5, never overflows), then flushed with one global
// atomic per distinct key.  Two tables alternate so one barrier per column
// suffices: column j inserts into table j&1 while the flush of table (j-1)&1
// by other waves completes before the next barrier.
constexpr u32 kColEmpty = 0xFFFFFFFFu;

// LOG2 = log2(table slots) = log2(2 * workgroup size)
template <int PS, int LOG2>
struct ColumnAgg {
  static constexpr int kSlots = 1 << LOG2;
  u32 (*tag)[kSlots];
  float (*acc)[kSlots * PS];

  __device__ __forceinline__ void init() {
    for (int i = threadIdx.x; i < kSlots; i += blockDim.x) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        tag[t][i] = kColEmpty;
#pragma unroll
        for (int c = 0; c < PS; ++c) acc[t][i * PS + c] = 0.0f;
      }
    }
  }
  // slot of `dest` in table t (claimed on first use); a column inserts at most
  // kSlots/2 keys, so the probe always terminates
  __device__ __forceinline__ int insert(int t, u32 dest) {
    u32 h = (dest * 0x9E3779B1u) >> (32 - LOG2);
    while (true) {  // (one CAS against an empty slot per probe step, no read first)
      const u32 old = atomicCAS(&tag[t][h], kColEmpty, dest);
      if (old == kColEmpty || old == dest) return (int)h;
      h = (h + 1) & (kSlots - 1);
    }
  }
  __device__ __forceinline__ void add(int t, int h, int c, float g) {
    atomicAdd(&acc[t][h * PS + c], g);
  }
  // one global atomic per (distinct key, non-zero component); resets the
  // table.  Consecutive lanes take consecutive components of a key's gradient
  // row, so a wave's atomics land on a few contiguous PS*4-byte segments
  // instead of 64 scattered rows.
  __device__ __forceinline__ void flush(int t, float* __restrict__ grad) {
    if constexpr (PS == 1) {
      for (int i = threadIdx.x; i < kSlots; i += blockDim.x) {
        u32 d = tag[t][i];
        if (d == kColEmpty) continue;
        float v = acc[t][i];
        if (v != 0.0f) atomicAdd(&grad[d], v);
        acc[t][i] = 0.0f;
        tag[t][i] = kColEmpty;
      }
    } else {
      for (int e = threadIdx.x; e < kSlots * PS; e += blockDim.x) {
        const int i = e / PS, c = e - i * PS;
        u32 d = tag[t][i];
        if (d == kColEmpty) continue;
        float v = acc[t][e];
        if (v != 0.0f) atomicAdd(&grad[(size_t)d * PS + c], v);
        acc[t][e] = 0.0f;
      }
      __syncthreads();  // every lane has read the tags before they are reset
      for (int i = threadIdx.x; i < kSlots; i += blockDim.x) tag[t][i] = kColEmpty;
    }
  }
};

// Column aggregation for the atomic-free LR backward (PS == 1), double
// buffered (column j uses table j & 1, one barrier per column).  Per column:
// every occurrence inserts its dest -- one CAS against kFree per probe step --
// and so claims a slot or finds it claimed; one that found it claimed adds
// its values to the slot and marks it joined; a claimer takes its record's
// index from the workgroup's running count and counts it in the LDS histogram
// of dest >> kRedShift that drives the reduction kernels below.  After the
// barrier each claimer frees its slot and writes its record -- its own
// values, plus the slot's sums if joined (then zeroed) -- so the table is
// empty again when column j + 2 reuses it.  A key alone in its column (most
// of the long-tail occurrences) costs one CAS, one flag read and one tag
// write: no accumulator traffic, no slot list.
// NV = values aggregated per key: 1 (LR: Σ loss) or 2 (reference-math FM:
// Σ loss and Σ loss*vsum, expanded to the 1+D gradient in k_red_sum).
// Records: NV == 1 -> u64 (dest | value << 32), NV == 2 -> uint3 (dest, v0, v1):
// 12 bytes, dwordx3 accesses (a quarter less traffic than padded uint4 records).
// kTabs = 1: one table, freed before the next column inserts (a second
// barrier per column) -- twice the slots in the same LDS.
template <int LOG2, int NV = 1, int kTabs = 2>
struct ListAgg {
  static constexpr int kSlots = 1 << LOG2;
  static constexpr int kShift = red_shift(NV);
  static constexpr int kFx = FxBits<NV>::kFx;
  static constexpr u32 kFree = 0xffffffffu;  // (no dest: dest < trash_pos * S)
  u32 (*tag)[kSlots];
  long long (*acc)[kSlots * NV];  // fixed-point sums (deterministic, see fx_from)
  unsigned short (*list)[kSlots / 2];  // (storage of the joined flags: kSlots bytes per table)
  u32* nlist;   // [0]: the workgroup's records so far
  u32* hist;    // [red_nb]
  u64* region;  // this workgroup's pair region
  int shift = kShift;  // bucket = dest >> shift (RedGeom: runtime, >= kShift)
  u32 bad = 0;   // a clamped fixed-point input (see fx_clamp), OR-ed into the stats flag
#ifdef XFLOW_KTIMING
  unsigned long long* kt_acc_ = nullptr;  // (the kernel's phase counters: 4 insert, 5 barrier, 6 flush)
  unsigned long long* kt_cur_ = nullptr;
#define XF_KTL(p)                                  \
  do {                                             \
    if (kt_acc_) {                                 \
      const unsigned long long n_ = clock64();     \
      kt_acc_[p] += n_ - *kt_cur_;                 \
      *kt_cur_ = n_;                               \
    }                                              \
  } while (0)
#else
#define XF_KTL(p) (void)0
#endif

  __device__ __forceinline__ unsigned char* joined(int t) {
    return reinterpret_cast<unsigned char*>(&list[t][0]);
  }
  __device__ __forceinline__ void init(int nb) {
    for (int i = threadIdx.x; i < kSlots; i += blockDim.x) {
#pragma unroll
      for (int tt = 0; tt < kTabs; ++tt) {
        tag[tt][i] = kFree;
        joined(tt)[i] = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[tt][i * NV + v] = 0ll;
      }
    }
    for (int i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x == 0) nlist[0] = 0u;
  }
  // records written by the workgroup (after its last column and a barrier)
  __device__ __forceinline__ u32 total() const { return nlist[0]; }
  // at most kSlots/2 keys per column in an empty table: the probe terminates
  __device__ __forceinline__ int insert(int t, u32 dest, bool& claimed) {
    u32 h = (dest * 0x9E3779B1u) >> (32 - LOG2);
    while (true) {
      const u32 old = atomicCAS(&tag[t][h], kFree, dest);
      if (old == kFree) {
        claimed = true;
        return (int)h;
      }
      if (old == dest) return (int)h;
      h = (h + 1) & (kSlots - 1);
    }
  }
  // called by every lane of the workgroup (wave-uniform control flow)
  __device__ __forceinline__ void column(int j, bool has, u32 dest, float loss,
                                         float loss2 = 0.0f) {
    const int t = kTabs == 2 ? (j & 1) : 0;
    bool claimed = false;
    int h = 0;
    long long v[NV];
    v[0] = 0ll;
    if constexpr (NV > 1) v[1] = 0ll;
    if (has) {
      h = insert(t, dest, claimed);
      v[0] = fx_from<kFx>(fx_clamp<kFx>(loss, bad));
      if constexpr (NV > 1) v[1] = fx_from<kFx>(fx_clamp<kFx>(loss2, bad));
    }
    if (has && !claimed) {
#pragma unroll
      for (int c = 0; c < NV; ++c)
        atomicAdd(reinterpret_cast<unsigned long long*>(&acc[t][h * NV + c]), (unsigned long long)v[c]);
      joined(t)[h] = 1;
    }
    const unsigned long long m = __ballot(claimed);
    u32 idx = 0;
    if (m) {
      const int lane = lane_id();
      const int leader = __ffsll((long long)m) - 1;
      u32 base = 0;
      if (lane == leader) base = atomicAdd(&nlist[0], (u32)__popcll(m));
      idx = __shfl(base, leader) + (u32)__popcll(m & ((1ull << lane) - 1ull));
    }
    if (claimed) {
      XF_DASSERT((int)(dest >> shift) < kRedMaxBuckets);
      atomicAdd(&hist[dest >> shift], 1u);
    }
    XF_KTL(4);
    lds_barrier();
    XF_KTL(5);
    if (claimed) {
      tag[t][h] = kFree;
      if (joined(t)[h]) {
        joined(t)[h] = 0;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
          v[c] += acc[t][h * NV + c];
          acc[t][h * NV + c] = 0ll;
        }
      }
      const float v0 = (float)fx_to_double<kFx>(v[0]);
      if constexpr (NV == 1) {
        region[idx] = (u64)dest | ((u64)__float_as_uint(v0) << 32);
      } else {
        const float v1 = (float)fx_to_double<kFx>(v[1]);
        reinterpret_cast<uint3*>(region)[idx] =
            make_uint3(dest, __float_as_uint(v0), __float_as_uint(v1));
      }
    }
    XF_KTL(6);
    if constexpr (kTabs == 1) lds_barrier();  // (freed before the next column inserts)
  }
};

constexpr int ilog2c(int v) { return v <= 1 ? 0 : 1 + ilog2c(v / 2); }

// A row's dedup positions, column by column, kPosChunk columns per load
// batch: a chunk's loads are issued together (one memory latency per chunk)
// and the next chunk's are issued before this chunk's columns run, so the
// column walks below -- a chain of LDS round trips and barriers per column --
// never wait on a global load.  (A load issued and consumed inside the walk
// costs a full memory latency per column: the barriers' memory clobber keeps
// the compiler from hoisting it, and the records' conditional stores make its
// vmcnt wait a vmcnt(0).)  Every lane loads from a valid address (pos[0]
// outside its row) and the row bounds select trash_pos at the use.
constexpr int kPosChunk = 8;
struct PosStream {
  const u32* __restrict__ pos;
  RowSpan rs;
  int len;
  u32 trash;
  u32 cur[kPosChunk], nxt[kPosChunk];
  u32 okc = 0, okn = 0;
  __device__ __forceinline__ PosStream(const u32* p, const RowSpan& r, int n, u32 tr,
                                       bool prime = true)
      : pos(p), rs(r), len(n), trash(tr) {
    if (prime) fetch(cur, okc, 0);
  }
  __device__ __forceinline__ void fetch(u32 (&dst)[kPosChunk], u32& ok, int j0) const {
    ok = 0u;
#pragma unroll
    for (int q = 0; q < kPosChunk; ++q) {
      const bool v = j0 + q < len;
      dst[q] = pos[v ? rs.at(j0 + q) : 0];
      ok |= (u32)v << q;
    }
  }
  __device__ __forceinline__ void prefetch(int j0) { fetch(nxt, okn, j0); }
  __device__ __forceinline__ u32 get(int q) const { return (okc >> q) & 1u ? cur[q] : trash; }
  __device__ __forceinline__ void advance() {
#pragma unroll
    for (int q = 0; q < kPosChunk; ++q) cur[q] = nxt[q];
    okc = okn;
  }
};

// Rows of at most kLrRegCols features keep their dedup positions in registers:
// every pos load of a row is issued before the first use (one memory latency
// instead of one per 4 features), and the backward column walk reuses them
// instead of re-reading pos.  Longer rows take the streaming path.
constexpr int kLrRegCols = 40;
static_assert(kLeadMaxFields <= kLrRegCols, "k_lr_lead's register rows");

// FM: pulled row = [w, v_0 .. v_{D-1}, pad] (pstride floats)
constexpr int fm_ps(int D) { return ((1 + D) + 3) & ~3; }
constexpr int fm_block(int D) { return fm_ps(D) <= 12 ? 256 : (fm_ps(D) <= 20 ? 128 : 64); }

// MVM: pulled row = [v_0 .. v_{D-1}, pad]
constexpr int mvm_ps(int D) { return D == 1 ? 1 : (D + 3) & ~3; }
constexpr int mvm_block(int D) { return mvm_ps(D) <= 12 ? 256 : (mvm_ps(D) <= 20 ? 128 : 64); }
constexpr int mvm_block_for(int D, bool red) { return red ? kMvmGroupRows : mvm_block(D); }

template <int PS>
__device__ __forceinline__ void load_row(const float* __restrict__ wp, u32 p, float (&w)[PS]) {
  if constexpr (PS % 4 == 0) {
    const float4* src = reinterpret_cast<const float4*>(wp) + (size_t)p * (PS / 4);
#pragma unroll
    for (int q = 0; q < PS / 4; ++q) {
      const float4 v4 = src[q];
      w[4 * q] = v4.x;
      w[4 * q + 1] = v4.y;
      w[4 * q + 2] = v4.z;
      w[4 * q + 3] = v4.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < PS; ++c) w[c] = wp[(size_t)p * PS + c];
  }
}

constexpr int kRedBlock = 1024;
constexpr int kRedUnroll = 4;

// record of one (dest, NV values) partial sum; NV >= 3: standard-FM vector
// records (dest, v_0 .. v_{NV-1}, pad) of vec_rec_words(NV) words
template <int W>
struct VecRec {
  uint4 q[W / 4];
};
template <int NV> struct VecRedRec {
  using T = VecRec<vec_rec_words(NV)>;
  __device__ static u32 dest(const T& r) { return r.q[0].x; }
};
template <int NV> struct RedRec;
template <> struct RedRec<1> {
  using T = u64;
  __device__ static u32 dest(T r) { return (u32)r; }
};
template <> struct RedRec<2> {
  using T = uint3;
  __device__ static u32 dest(T r) { return r.x; }
};

// (defined here: the scalar and the vector reduction each instantiate their own record types)
template <int NV, typename R = RedRec<NV>>
__global__ void __launch_bounds__(kRedBlock) k_red_scatter(BatchView b, int rows_per_group,
                                                           const void* __restrict__ pairs,
                                                           const u32* __restrict__ count,
                                                           const u32* __restrict__ hist,
                                                           const u32* __restrict__ tot,
                                                           u32* __restrict__ start, int nb,
                                                           void* __restrict__ sorted,
                                                           RedGeom geom) {
  using T = typename R::T;
  const int kShift = geom.shift(red_shift(NV));
  __shared__ u32 cur[kRedMaxBuckets];
  const int g = blockIdx.x, groups = gridDim.x;
  nb = geom.active(kShift, nb);
  u32 carry = 0;
  for (int c0 = 0; c0 < nb; c0 += kRedBlock) {
    const int i = c0 + (int)threadIdx.x;
    const u32 v = i < nb ? tot[i] : 0u;
    u32 t;
    const u32 ex = block_exclusive_scan<kRedBlock>(v, &t);
    if (i < nb) {
      cur[i] = carry + ex + hist[(size_t)i * groups + g];
      if (g == 0) start[i] = carry + ex;
    }
    carry += t;
  }
  if (g == 0 && threadIdx.x == 0) start[nb] = carry;
  __syncthreads();
  const int64_t r0 = (int64_t)g * rows_per_group;
  const T* src = static_cast<const T*>(pairs) +
                 (b.row_ptr ? (int64_t)b.row_ptr[r0] : r0 * b.nnz_per_row);
  T* dst = static_cast<T*>(sorted);
  const u32 n = count[g];
  // kRedUnroll independent load -> LDS rank -> store chains per lane
  for (u32 i0 = threadIdx.x; i0 < n; i0 += kRedUnroll * kRedBlock) {
    T pr[kRedUnroll];
#pragma unroll
    for (int q = 0; q < kRedUnroll; ++q) {
      const u32 i = i0 + (u32)q * kRedBlock;
      if (i < n) pr[q] = src[i];
    }
    u32 p[kRedUnroll];
#pragma unroll
    for (int q = 0; q < kRedUnroll; ++q)
      if (i0 + (u32)q * kRedBlock < n) {
        XF_DASSERT((int)(R::dest(pr[q]) >> kShift) < nb);
        p[q] = atomicAdd(&cur[R::dest(pr[q]) >> kShift], 1u);
      }
#pragma unroll
    for (int q = 0; q < kRedUnroll; ++q)
      if (i0 + (u32)q * kRedBlock < n) dst[p[q]] = pr[q];
  }
}

// Final gradient rows.  NV == 1: grad[dest] = Σ (LR).  NV == 2: reference-math
// FM (fm_worker.cc:126-157), per (key, slice) dest = slot*S + s with B = Σ loss
// and C = Σ loss*vsum: g_w = D*B, g_v[k] = Σ loss*(vsum - v_k) = C - v_k*B.
struct RedFinal {
  float* grad;
  const float* wpull;  // [slot][ps] pulled rows (NV == 2)
  int S, ps, D;
  float* out;          // NV == 1 send-order output (FwdArgs::red_out), or null
  const u32* inv;
  const int32_t* rows;
  bool compact;        // NV == 2: store (B, C) only (FwdArgs::fm_compact)
  u32* masks;          // slice-presence bits (FwdArgs::red_masks; unique order with out), or null
  // (out, S == 1) the unique index from the compaction's chunk offsets and
  // the stamps instead of inv (FwdArgs::red_rank_*); rk_offs null: through inv
  const u32* rk_offs = nullptr;
  const unsigned char* rk_stamps = nullptr;
  const unsigned long long* rk_cap = nullptr;  // slots the compaction covered (FwdArgs::red_bcap)
  u32 rk_epoch = 0;
  // (k_red_sum_local, rk_offs, no out) FTRL in place of the store
  // (FwdArgs::red_apply_*): the table's words, and in unique order the keys'
  // table slots and pulled (n, z); ap_slots null: off
  u32* ap_words = nullptr;
  const u32* ap_slots = nullptr;
  const float2* ap_nz = nullptr;
  FtrlParams ap_fp;
};

// Slice bits of one slot from the presence bitmap: its dests slot*S + s that
// fall in [lo, lo + kR).
template <u32 kR>
__device__ __forceinline__ u32 slot_bits(const u32* pbits, u64 slot, u64 S, u64 lo) {
  u32 bits = 0;
  for (u64 s = 0; s < S; ++s) {
    const u64 d = slot * S + s;
    if (d >= lo && d < lo + kR && ((pbits[(d - lo) >> 5] >> ((d - lo) & 31)) & 1u))
      bits |= 1u << s;
  }
  return bits;
}

// Slice bits of every slot whose dests slot*S + s meet the unit [lo, lo + kR),
// from the unit's presence bitmap (bit l: dest lo + l has records): one plain
// store per slot inside the unit, an atomic OR for a slot straddling its edge
// (S not dividing kR; the masks start zeroed).  masks are indexed by slot, or
// by the slot's unique index (inv != null: unique-order outputs).
template <u32 kR>
__device__ __forceinline__ void unit_masks(const u32* pbits, u64 lo, u64 S, u32* __restrict__ masks,
                                           const u32* __restrict__ inv) {
  const u64 s0 = lo / S, s1 = (lo + kR + S - 1) / S;
  for (u64 slot = s0 + threadIdx.x; slot < s1; slot += blockDim.x) {
    const u32 bits = slot_bits<kR>(pbits, slot, S, lo);
    if (!bits) continue;
    u64 m = slot;
    if (inv) {
      m = inv[slot];
      if (m == 0xFFFFFFFFu) continue;  // (the trash slot)
    }
    if (slot * S >= lo && slot * S + S <= lo + kR) masks[m] = bits;
    else atomicOr(&masks[m], bits);
  }
}

// Bucket-sorted producer regions (FwdArgs::red_local, k_lr_lead<true> ->
// k_red_sum_local): red_hist[bucket][workgroup] holds the bucket's segment of
// the workgroup's region, first record << 16 | records.  A region has at most
// kLeadTile x kLeadMaxFields records.
static_assert(kLeadTile * kLeadMaxFields < (1 << 16), "lead_seg packs two 16-bit fields");
__device__ __forceinline__ u32 lead_seg(u32 start, u32 count) { return start << 16 | count; }
struct LeadSegs {
  const u64* pairs = nullptr;  // the producers' regions, gcap records apart
  const u32* hist = nullptr;   // [nb][groups] lead_seg words
  u32 groups = 0, gcap = 0;
  // per unit (k_red_sum_local): the bucket's row of hist, whether it has
  // records at all, and the form of the sums (block-uniform)
  const u32* row = nullptr;
  bool any = false, dense = false;
  // segment g of the row, clamped to the region
  __device__ __forceinline__ void seg(u32 word, u32& off, u32& cnt) const {
    off = word >> 16;
    cnt = word & 0xFFFFu;
    off = off < gcap ? off : gcap;
    cnt = cnt < gcap - off ? cnt : gcap - off;
  }
};

struct SegSrc {
  const u32* hist;   // [nb][groups] exclusive prefix (k_red_scan)
  const u32* tot;    // [nb]
  const u32* subs;   // [nb][groups] sub-range start in the workgroup region
  BatchView b;
  int rows_per_group, groups;
};

// Rows per producer workgroup on the reduction path: the model's R, or --
// when the batch fills at most an eighth of the CUs (a slice group of a step
// of 256 slices or more) -- halved (down to 128) until it fills them, within
// the workgroups the reduction's buffers hold.  A producer's time is its
// column walk, nearly independent of its rows; narrower workgroups aggregate
// less, so the records' sums cost more (A/B, profiles/r4_negative_ab.txt 13:
// LR --slices 256 +5.5 %, --slices 64 -1.5 % when narrowed to fill the CUs).
inline int narrow_rows(const FwdArgs& a, int R) {
  const int64_t rows = a.batch.rows;
  auto groups = [&](int r) { return (rows + r - 1) / r; };
  if (a.red_groups <= 0 || groups(R) * 8 > device_cus()) return R;
  while (R > 128 && groups(R) < device_cus() && groups(R / 2) <= a.red_groups) R /= 2;
  return R;
}

// "This step is on the bucket-reduction path" (up to max_buckets buckets).
inline bool red_path(const FwdArgs& a, int max_buckets) {
  return a.agg_ok && a.red_pairs && a.red_nb > 0 && a.red_nb <= max_buckets;
}
// bucket cap of the vector-record reductions (FwdArgs::red_maxb)
inline int red_cap(const FwdArgs& a) { return a.red_maxb > 0 ? a.red_maxb : kRedMaxBuckets; }

// Calls f(std::integral_constant<int, R>) for the producer's rows per
// workgroup (narrow_rows: 1024, 512, 256 or 128), so f can name R as a
// template argument of the kernel it launches.
template <typename F>
inline void launch_rows(int R, F&& f) {
  switch (R) {
    case 1024: f(std::integral_constant<int, 1024>{}); break;
    case 512: f(std::integral_constant<int, 512>{}); break;
    case 256: f(std::integral_constant<int, 256>{}); break;
    default: f(std::integral_constant<int, 128>{}); break;
  }
}

// kernels_reduce.hip (launch_reduction: NV = 1, 2)
__global__ void k_red_scan(u32* __restrict__ hist, int groups, u32* __restrict__ tot, RedGeom geom,
                           int base);
template <int NV>
void launch_reduction(const FwdArgs& a, int groups, int rows_per_group, hipStream_t st);
// kernels_reduce_vec.hip (D = 1, 2, 4, 8, 10, 16, 32; kMvm: D = the MVM width - 1)
template <int D, bool kMvm = false>
void launch_vec_reduction(const FwdArgs& a, hipStream_t st);
// kernels_lr.hip, kernels_fm.hip, kernels_mvm.hip
void dispatch_lr(const FwdArgs& a, hipStream_t st);
template <bool kGrad>
void dispatch_fm(const FwdArgs& a, hipStream_t st);
template <bool kGrad>
void dispatch_mvm(const FwdArgs& a, hipStream_t st);

}  // namespace hip
}  // namespace xflow
