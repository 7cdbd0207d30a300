// xflow-amd: push of the HBM-resident sparse parameter store (gfx950).
// Replaces the Push of the ps-lite KVServer + unordered_map store of the
// reference (ftrl.h:38-152, server.h:20-35):
//
//   table_apply  per-coordinate FTRL-Proximal / SGD push (one lane per key for
//                LR, one lane group per key for multi-parameter models),
//                contributions applied in (slice) order -> deterministic.
//
// and the owner grouping of a multi-source step's received entries
// (k_owner_group), which the one-launch multi-source applies read.
#include "table_common.h"

namespace xflow {
namespace hip {

#define XF_APPLY_SNAPSHOT(a) \
  if ((a).snap) store_snapshot((a).snap, (a).snap_mon, (a).snap_seq)

// LR-FTRL, one slice, 16-byte slots: read (n,z) as one dwordx2, write it back.
// One key per lane, grid-stride: measured faster than issuing four keys per
// lane up front (54 vs 49 us for 850 K keys) -- twice the waves in flight hide
// the dependent slot -> state chain better than per-lane ILP.
template <bool kSlices>
__global__ void __launch_bounds__(kBlock) k_apply_lr16(ApplyArgs a) {
  XF_APPLY_SNAPSHOT(a);
  int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const FtrlParams fp = a.opt.ftrl;
  if constexpr (kSlices) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      // unique-order [key][slice] normalised sums: the present slices' pushes
      // in slice order (the CPU backend's Hogwild order); a key no slice of
      // this group touched is skipped before any table access
      const u32 m0 = a.masks[i];
      if (!m0) continue;
      if (a.masks_clear) const_cast<u32*>(a.masks)[i] = 0u;
      u32 slot = a.slots[i];
      if (slot == kNoSlot) continue;
      float2* st = reinterpret_cast<float2*>(a.table.words + (u64)slot * 4 + 2);
      // (the pull's stash for the step's first group; later groups read the
      // state the earlier ones wrote)
      float2 nz = a.nz_stash ? reinterpret_cast<const float2*>(a.nz_stash)[i] : *st;
      const float* g = a.grads + (size_t)i * a.S;
      float sn = sqrtf(nz.x);
      for (u32 m = m0; m; m &= m - 1) {
        const float w = ftrl_weight_sn(nz.y, sn, fp);
        ftrl_push_sn(nz.x, nz.y, sn, w, g[__ffs(m) - 1], fp);
      }
      *st = nz;
    }
  } else {
    // the next key's loads are issued before this key's stores: on gfx9
    // vmcnt also counts stores, so a load issued after them would wait for
    // their completion as well
    struct In {
      u32 slot, row;
      float raw;
      float2 nz;
    };
    auto load = [&](int64_t i) {
      In x;
      x.slot = a.slots[i];
      x.row = a.grad_map ? a.grad_map[i] : (u32)i;
      x.raw = a.grads[x.row];
      x.nz = make_float2(0.0f, 0.0f);
      if (x.slot != kNoSlot)
        x.nz = a.nz_stash ? reinterpret_cast<const float2*>(a.nz_stash)[i]
                          : *reinterpret_cast<const float2*>(a.table.words + (u64)x.slot * 4 + 2);
      return x;
    };
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    In nx;
    if (i < n) nx = load(i);
    for (; i < n; i += stride) {
      const In x = nx;
      if (i + stride < n) nx = load(i + stride);
      if (a.zero_after) a.grads[x.row] = 0.0f;
      if (x.slot == kNoSlot) continue;
      float2 nz = x.nz;
      const float w = ftrl_weight(nz.y, nz.x, fp);
      const float g = norm_grad(x.raw, a.slice_rows, 0);
      ftrl_push(nz.x, nz.y, w, g, fp);
      *reinterpret_cast<float2*>(a.table.words + (u64)x.slot * 4 + 2) = nz;
    }
  }
}

// LR-FTRL, 16-byte slots, CSR gradients (ApplyArgs::csr_*, one launch for
// every slice of the step): a key's entries are its slices' normalised sums in
// slice order -- the reference's per-slice pushes of only the keys a slice
// touched (lr_worker.cc:162-175) -- applied as a chain on (n, z) held in
// registers (sqrt(n) carried), the slot written once.  The first entries of
// the next keys are loaded before this key's chain.
constexpr int kCsrChunk = 8;  // CSR entries a lane loads at once
// Chains longer than this run in a second launch over the deferred keys
constexpr u32 kCsrShortChain = 16;

// Geometry of the deferral lists (ApplyArgs::csr_long, in u32 words) of a
// launch of W waves that each visit kpi keys per iteration of the grid-stride
// loop over at most n_max keys:
//   [counts W][regions W x R][offsets W + 1][dense list <= n_max][scan tiles]
// with R = the keys one wave visits.  k_csr_gather and the host's capacity
// check take it from here.  The apply kernels keep the same arithmetic on
// their own loop stride (CsrDefer, CsrDense below): built on this struct they
// compiled to other register counts.  The debug build (XF_DASSERT) checks
// them against it in every launch.
struct CsrLists {
  u64 W, R, n;
  XF_HD CsrLists(int64_t n_max, u32 waves, int kpi) : W(waves), n((u64)n_max) {
    const int64_t stride = (int64_t)waves * kpi;
    R = (u64)kpi * (u64)((n_max + stride - 1) / stride);
  }
  XF_HD u64 regions() const { return W; }
  XF_HD u64 offsets() const { return W + W * R; }
  XF_HD u64 dense() const { return offsets() + W + 1; }
  XF_HD u64 tiles() const { return dense() + n; }
};

// (debug build) the offsets CsrDefer and CsrDense use are CsrLists'
__device__ __forceinline__ bool csr_lists_agree(int64_t n_max, int64_t stride, int kpi, u32 waves,
                                                u64 R) {
  const CsrLists g(n_max, waves, kpi);
  return stride == (int64_t)waves * kpi && R == g.R && waves == g.regions() &&
         waves + (u64)waves * R == g.offsets() && g.offsets() + waves + 1 == g.dense();
}

// Wave-private deferral lists: wave w owns region w and writes its count to
// [w]; the second launch has the same grid and takes its own wave's list -- no
// global counter (a single one serialised ~10^4 atomics per step at one L2
// channel)
// (stride = waves * kpi: CsrLists' W, R, regions())
struct CsrDefer {
  u32* list = nullptr;
  u32 gw = 0, waves = 0;
  u64 R = 0;
  __device__ __forceinline__ CsrDefer(u32* l, int64_t n_max, int64_t stride, int kpi) : list(l) {
    gw = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    waves = gridDim.x * (blockDim.x / kWave);
    R = (u64)kpi * (u64)((n_max + stride - 1) / stride);
    XF_DASSERT(csr_lists_agree(n_max, stride, kpi, waves, R));
  }
  __device__ __forceinline__ u32* region() const { return list + waves + (u64)gw * R; }
};
// After the first pass the counts are scanned into offsets (waves + 1) and
// the regions gathered into one dense list, so the second pass packs 64 long
// chains per wave (a wave-private list holds ~2 of them: lanes idle)
// (CsrLists' offsets() and dense())
struct CsrDense {
  const u32* offs;
  const u32* list;
  __device__ __forceinline__ CsrDense(const u32* l, const CsrDefer& d)
      : offs(l + d.waves + (u64)d.waves * d.R), list(offs + d.waves + 1) {}
};

// one wave per source region: its deferred keys to their dense positions
__global__ void __launch_bounds__(kBlock) k_csr_gather(u32* __restrict__ l, int64_t n_max,
                                                       int kpi, u32 waves) {
  const u32 w = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (w >= waves) return;
  const CsrLists g(n_max, waves, kpi);
  const u32* offs = l + g.offsets();
  u32* dense = l + g.dense();
  const u32* src = l + g.regions() + (u64)w * g.R;
  const u32 c = l[w], o = offs[w];
  for (u32 k = lane_id(); k < c; k += kWave) dense[o + k] = src[k];
}

// kLong: the second launch (entries of the deferred list), else the first
template <bool kLong>
__global__ void __launch_bounds__(kBlock) k_apply_lr16_csr(ApplyArgs a) {
  if (!kLong) XF_APPLY_SNAPSHOT(a);
  const int64_t stride0 = (int64_t)gridDim.x * blockDim.x;
  const CsrDefer df(a.csr_long, a.n_max, stride0, kWave);
  __shared__ u32 s_def[kBlock / kWave];
  const int wib = threadIdx.x / kWave, lane = lane_id();
  if (!kLong && lane == 0) s_def[wib] = 0u;
  // (pass 2: the dense list of every wave's deferred keys, csr_dense)
  const CsrDense dn(a.csr_long, df);
  const int64_t n = kLong ? (int64_t)dn.offs[df.waves] : dev_count(a.n_dev, a.n_host, a.n_max);
  const u32* __restrict__ lst = dn.list;
  const int64_t stride = stride0;
  const FtrlParams fp = a.opt.ftrl;
  const u64* __restrict__ ent = static_cast<const u64*>(a.csr_ent);
  struct In {
    u32 key, slot, off, cnt;
    u64 e0;
    float2 nz;
  };
  auto load = [&](int64_t j) {
    In x;
    const int64_t i = kLong ? (int64_t)lst[j] : j;
    x.key = (u32)i;
    x.slot = a.slots[i];
    x.off = a.csr_off[i];
    x.cnt = a.csr_cnt[i];
    x.e0 = x.cnt ? ent[x.off] : 0ull;
    x.nz = make_float2(0.0f, 0.0f);
    if (x.slot != kNoSlot && x.cnt && (kLong || !a.csr_long || x.cnt <= kCsrShortChain))
      x.nz = a.nz_stash ? reinterpret_cast<const float2*>(a.nz_stash)[i]
                        : *reinterpret_cast<const float2*>(a.table.words + (u64)x.slot * 4 + 2);
    return x;
  };
  // (pass 2: few keys -- the hot ones -- each a long latency-bound chain:
  // consecutive keys go to consecutive workgroups, so they spread over every
  // CU and several waves share each SIMD, instead of packing 64 per wave
  // onto the first few CUs)
  int64_t i = kLong ? (int64_t)threadIdx.x * gridDim.x + blockIdx.x
                    : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  In nx;
  if (i < n) nx = load(i);
  for (; i < n; i += stride) {
    const In x = nx;
    if (i + stride < n) nx = load(i + stride);
    if (!kLong && a.csr_long && x.slot != kNoSlot && x.cnt > kCsrShortChain) {
      df.region()[atomicAdd(&s_def[wib], 1u)] = x.key;  // (LDS counter of this wave)
      continue;
    }
    if (x.slot == kNoSlot || !x.cnt) continue;
    float2 nz = x.nz;
    float sn = sqrtf(nz.x);
    auto push = [&](u64 e) {
      const float w = ftrl_weight_sn(nz.y, sn, fp);
      ftrl_push_sn(nz.x, nz.y, sn, w, __uint_as_float((u32)(e >> 32)), fp);
    };
    push(x.e0);
    // the chain's values (the entries' high words) C at a time, all C loads
    // in flight together: indices past the chain are clamped to its last
    // entry, not predicated -- a predicated load is a branch around it and
    // the compiler then waits on each one before the next
    const u32* __restrict__ hv = reinterpret_cast<const u32*>(ent) + 1;
    const u32 last = x.off + x.cnt - 1;
    auto chain = [&](auto cc) {
      constexpr int C = decltype(cc)::value;
      for (u32 j = 1; j < x.cnt; j += C) {
        float e[C];
#pragma unroll
        for (int q = 0; q < C; ++q) e[q] = __uint_as_float(hv[2 * (u64)min(x.off + j + q, last)]);
#pragma unroll
        for (int q = 0; q < C; ++q)
          if (j + q < x.cnt) {
            const float w = ftrl_weight_sn(nz.y, sn, fp);
            ftrl_push_sn(nz.x, nz.y, sn, w, e[q], fp);
          }
      }
    };
    if (!kLong) chain(std::integral_constant<int, 4>());
    else chain(std::integral_constant<int, kCsrChunk>());
    *reinterpret_cast<float2*>(a.table.words + (u64)x.slot * 4 + 2) = nz;
  }
  // (every lane has left the loop: lane 0, the wave's last, saw every defer)
  if (!kLong && a.csr_long && lane == 0) a.csr_long[df.gw] = s_def[wib];
}

__global__ void __launch_bounds__(kBlock) k_apply_generic(ApplyArgs a) {
  XF_APPLY_SNAPSHOT(a);
  int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const TableView& t = a.table;
  const TableLayout& L = t.L;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int S = a.S, ps = a.pstride, P = a.P;
  const u32 all = (S >= 32) ? 0xFFFFFFFFu : ((1u << S) - 1u);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32 slot = a.slots[i];
    u32 row = a.grad_map ? a.grad_map[i] : (u32)i;
    float* g = a.grads + (size_t)row * S * ps;
    u32 m = a.masks ? a.masks[row] : all;
    if (slot != kNoSlot) {
      u32* sp = t.words + (u64)slot * L.stride;
      u64 key = *reinterpret_cast<u64*>(sp);
      if (a.sum_slices) {
        for (int p = 0; p < P; ++p) {
          float acc = 0.0f;
          for (int s = 0; s < S; ++s)
            if (m & (1u << s)) acc += norm_grad(g[s * ps + p], a.slice_rows, s);
          slot_push(sp, key, p, acc, L, a.opt);
        }
        if (L.has_flag) sp[L.flag_word] = 1u;
      } else {
        for (int s = 0; s < S; ++s) {
          if (!(m & (1u << s))) continue;
          for (int p = 0; p < P; ++p)
            slot_push(sp, key, p, norm_grad(g[s * ps + p], a.slice_rows, s), L, a.opt);
          if (L.has_flag) sp[L.flag_word] = 1u;
        }
      }
    }
    if (a.zero_after) {
      for (int j = 0; j < S * ps; ++j) g[j] = 0.0f;
      if (a.masks_rw) a.masks_rw[row] = 0u;
    }
  }
}

// ---- one-launch multi-source apply (ApplyArgs::grp) ------------------------
__device__ __forceinline__ int group_src(const SrcGroups& g, int64_t i) {
  int s = 0;
  while (s + 1 < g.nsrc && i >= g.offs[s + 1]) ++s;
  return s;
}

// Entry i leads its key when no earlier source sent the key this step; then
// row = the key's (slot, source) registrations and src0 = i's source.
__device__ __forceinline__ bool group_leader(const SrcGroups& g, int64_t i, const u64*& row,
                                             int& src0) {
  const u32 so = g.opos[i];
  if (so == kNoSlot) return false;  // owner scratch overflow (flagged by k_owner_group)
  row = g.oidx + (u64)so * (u64)g.nsrc;
  src0 = group_src(g, i);
  for (int s = 0; s < src0; ++s)
    if ((u32)(row[s] >> 32) == g.epoch) return false;
  return true;
}

// Registration of every received entry under (owner-scratch slot of its key,
// source).  The owner scratch persists across steps (hot keys keep their
// slot); stale registrations carry older epochs.
__global__ void __launch_bounds__(kBlock) k_owner_group(OwnerGroupArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const u64 key = sanitize_key(a.keys[i]);
  const u64 mask = a.ocap - 1;
  u64 s = fmix64(key) & mask;
  u32 slot = kNoSlot;
  for (u64 c = 0; c < a.ocap; ++c) {
    const u64 cur = a.okeys[s];
    if (cur == key) {
      slot = (u32)s;
      break;
    }
    if (cur == kEmptyKey) {
      const u64 prev = atomicCAS(reinterpret_cast<unsigned long long*>(&a.okeys[s]),
                                 (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (prev == kEmptyKey || prev == key) {
        slot = (u32)s;
        break;
      }
    }
    s = (s + 1) & mask;
  }
  a.opos[i] = slot;
  if (slot == kNoSlot) {
    *a.overflow = 1u;
    return;
  }
  a.oidx[(u64)slot * (u64)a.g.nsrc + (u64)group_src(a.g, i)] = ((u64)a.g.epoch << 32) | (u32)i;
}

void launch_owner_group(const OwnerGroupArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  if (a.g.nsrc < 1 || a.g.nsrc > kMaxGroupSources) throw std::runtime_error("owner_group: nsrc");
  if (a.ocap == 0 || (a.ocap & (a.ocap - 1))) throw std::runtime_error("owner_group: ocap");
  hipLaunchKernelGGL(k_owner_group, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, st, a);
  XF_HIP_CHECK(hipGetLastError());
}

// LR-FTRL, one slice, 16-byte slots, all sources in one launch: the leader
// entry of a key takes (n, z) from its pull stash (or the table), pushes each
// source's gradient in source order and writes the slot once.
__global__ void __launch_bounds__(kBlock) k_apply_lr16_multi(ApplyArgs a) {
  XF_APPLY_SNAPSHOT(a);
  const int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const FtrlParams fp = a.opt.ftrl;
  const SrcGroups& g = a.grp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64* row;
    int src0;
    if (!group_leader(g, i, row, src0)) continue;
    const u32 slot = a.slots[i];
    if (slot == kNoSlot) continue;
    float2* st = reinterpret_cast<float2*>(a.table.words + (u64)slot * 4 + 2);
    float2 nz = a.nz_stash ? reinterpret_cast<const float2*>(a.nz_stash)[i] : *st;
    float sn = sqrtf(nz.x);
    for (int s = src0; s < g.nsrc; ++s) {
      const u64 v = row[s];
      if ((u32)(v >> 32) != g.epoch) continue;
      const float gr = a.grads[(u32)v];
      const float w = ftrl_weight_sn(nz.y, sn, fp);
      ftrl_push_sn(nz.x, nz.y, sn, w, gr, fp);
    }
    *st = nz;
  }
}

// Multi-parameter apply on packed lane groups (packed_lane: P lanes per key,
// lane p owns parameter p's optimizer state), so a wave touches a few
// contiguous slots instead of 64 scattered ones.  Every lane reads the
// "pushed" flag before lane 0 of the group writes it (one group never
// straddles a wave: program order); latent params use their lazy init value
// until the key's first push.  With a.grp (several sources) the group of a
// key's leader entry applies the (source, slice) contributions in that
// order; other entries skip.
// (7 waves per SIMD: <= 72 VGPRs without spills -- 77 at the default gave 6;
// 8 waves spills: FM-8 +1.7 % / -1 %, profiles/r2_s3_fm_pull_apply_pipeline.txt)
// kSl: a step of several slices (S > 1), whose keys take chains of pushes
template <bool kSl>
__global__ void __launch_bounds__(kBlock, 7) k_apply_group(ApplyArgs a) {
  XF_APPLY_SNAPSHOT(a);
  const int64_t n = dev_count(a.n_dev, a.n_host, a.n_max);
  const TableLayout& L = a.table.L;
  const int S = a.S, ps = a.pstride, gs = a.gstride ? a.gstride : ps;
  const u32 all = (S >= 32) ? 0xFFFFFFFFu : ((1u << S) - 1u);
  const PackedLane pl = packed_lane(L.P);
  const int p = pl.p;
  const bool multi = a.grp.oidx != nullptr;
  const bool ftrl = L.opt == kFTRL;
  int64_t i = pl.on ? pl.first : n;
  // (row words loaded an iteration ahead: another entry's slot -- keys are
  // unique per launch, and of a key's entries only the leader writes)
  RowPipe pipe;
  pipe.stride = pl.stride;
  pipe.n = n;
  if (ftrl && a.nz_stash) {  // (the pull's (n, z): the row is only written)
    pipe.stash = reinterpret_cast<const float2*>(a.nz_stash);
    pipe.keys = a.keys;
  }
  pipe.start(a.slots, a.table.words, i, p, L);
  // one source, one slice: the key's gradient row joins the pipeline too
  // (row index two iterations ahead, the lane's value(s) one ahead)
  const bool gpipe = !kSl && !multi && S == 1 && !a.masks && !a.sum_slices;
  auto grad_row = [&](int64_t k) -> u32 { return a.grad_map ? a.grad_map[k] : (u32)k; };
  auto grad_val = [&](u32 r) -> float2 {
    const float* g = a.grads + (size_t)r * gs;
    return a.fm_compact ? *reinterpret_cast<const float2*>(g) : make_float2(g[p], 0.0f);
  };
  u32 gr_cur = 0, gr_nx = 0;
  float2 gv_nx = make_float2(0.0f, 0.0f);
  if (gpipe && i < n) {
    gr_cur = grad_row(i);
    if (i + pl.stride < n) gr_nx = grad_row(i + pl.stride);
    gv_nx = grad_val(gr_cur);
  }
  for (; i < n; i += pl.stride) {
    RowPre rp;
    const u32 slot = pipe.next(a.slots, a.table.words, i, p, L, rp);
    float2 gv = make_float2(0.0f, 0.0f);
    u32 grow_i = 0;
    if (gpipe) {
      gv = gv_nx;
      grow_i = gr_cur;
      gr_cur = gr_nx;
      if (i + pl.stride < n) gv_nx = grad_val(gr_cur);
      if (i + 2 * pl.stride < n) gr_nx = grad_row(i + 2 * pl.stride);
    }
    const u64* grow = nullptr;
    int src0 = 0, nsrc = 1;
    if (multi) {
      if (!group_leader(a.grp, i, grow, src0)) continue;  // uniform over the key's lanes
      nsrc = a.grp.nsrc;
    }
    XF_DASSERT(slot == kNoSlot || slot < a.table.cap);
    if (slot != kNoSlot) {
      u32* sp = a.table.words + (u64)slot * L.stride;
      const u64 key = rp.key;
      bool pushed = rp.flag != 0u;
      float n0 = rp.s0, z0 = rp.s1;  // FTRL (n, z); SGD w
      // current weight; w_next caches it between pushes and is recomputed
      // only when another push follows (the closed form is the bulk of this
      // kernel's instructions: one push per key -- S = 1 -- evaluates it once)
      float w_next = state_weight(key, pushed, n0, z0, p, L, a.opt);
      bool stale = false;
      // (several slices: sqrtf(n) carried through the key's pushes)
      float sn = kSl && ftrl ? sqrtf(n0) : 0.0f;
      auto push = [&](float gv) {
        if constexpr (kSl) {
          if (stale) w_next = ftrl ? ftrl_weight_sn(z0, sn, a.opt.ftrl) : n0;
          if (ftrl) ftrl_push_sn(n0, z0, sn, w_next, gv, a.opt.ftrl);
          else n0 = w_next - a.opt.sgd.lr * gv;
        } else {
          if (stale) w_next = state_weight(key, true, n0, z0, p, L, a.opt);
          if (ftrl) ftrl_push(n0, z0, w_next, gv, a.opt.ftrl);
          else n0 = w_next - a.opt.sgd.lr * gv;
        }
        pushed = true;
        stale = true;
      };
      // compact reference-math FM rows (B, C): expand with the pre-step
      // (pulled) weight, the float recipe k_red_sum<2> uses for full rows
      const float w_pre = a.fm_compact ? (a.pulled ? a.pulled[(size_t)i * ps + p] : w_next) : 0.0f;
      u32 any = 0;
      if (gpipe) {
        any = 1u;
        const float raw = !a.fm_compact ? gv.x
                          : (p == 0 ? (float)a.fm_D * gv.x : gv.y - w_pre * gv.x);
        push(norm_grad(raw, a.slice_rows, 0));
        nsrc = 0;  // (the per-source loop below is skipped)
      }
      for (int sc = src0; sc < nsrc; ++sc) {
        u32 e = (u32)i;
        if (multi) {
          const u64 v = grow[sc];
          if ((u32)(v >> 32) != a.grp.epoch) continue;
          e = (u32)v;
        }
        const u32 row = a.grad_map ? a.grad_map[e] : e;
        const float* g = a.grads + (size_t)row * S * gs;
        const u32 m = a.masks ? a.masks[row] : all;
        if (a.masks_clear && p == 0) const_cast<u32*>(a.masks)[row] = 0u;
        any |= m;
        auto raw_of = [&](int s) -> float {
          if (!a.fm_compact) return g[s * gs + p];
          const float Bv = g[s * gs], Cv = g[s * gs + 1];
          return p == 0 ? (float)a.fm_D * Bv : Cv - w_pre * Bv;
        };
        if (a.sum_slices) {
          float acc = 0.0f;
          for (int s = 0; s < S; ++s)
            if (m & (1u << s)) acc += norm_grad(raw_of(s), a.slice_rows, s);
          if (m) push(acc);
        } else {
          for (int s = 0; s < S; ++s)
            if (m & (1u << s)) push(norm_grad(raw_of(s), a.slice_rows, s));
        }
      }
      if (ftrl) *reinterpret_cast<float2*>(sp + 2 + 2 * p) = make_float2(n0, z0);
      else sp[2 + p] = __float_as_uint(n0);
      if (L.has_flag && p == 0 && any) sp[L.flag_word] = 1u;
    }
    if (!multi && a.zero_after) {
      const u32 row = gpipe ? grow_i : (a.grad_map ? a.grad_map[i] : (u32)i);
      float* g = a.grads + (size_t)row * S * gs;
      const int w = a.fm_compact ? 2 : ps;
      for (int s = 0; s < S; ++s)
        for (int c = p; c < w; c += L.P) g[s * gs + c] = 0.0f;
      if (p == 0 && a.masks_rw) a.masks_rw[row] = 0u;
    }
  }
}

// CSR apply of compact reference-FM rows on packed lane groups (P lanes per
// key, lane p owns param p): the key's entries (slice, B, C), normalised by
// the reduction, expand with its pre-step weight (g_w = D*B, g_v = C - v*B,
// fm_worker.cc:126-157) and push in slice order.  The key's lanes load its
// entries cooperatively -- lane p holds entry c*P + p of chunk c, each push
// takes (B, C) from lane q % P by ds_bpermute -- so a chain of cnt entries
// costs ceil(cnt / P) loads, the next chunk in flight while one is consumed,
// instead of cnt dependent loads per lane.  Two-stage pipeline over the
// grid-stride loop: slot and (off, cnt) two iterations ahead, the row words
// and the first chunk one ahead.  kLong: the second launch, over the dense
// list of the deferred long chains.
// kRows (standard FM, ApplyArgs::csr_ew): full-row entries (slice, g_0 ..
// g_{P-1}) -- lane p reads its own component, kCsrRowChunk entries at a time
// (clamped, all in flight), the key's lanes together one entry's row.
constexpr int kCsrRowChunk = 4;
template <bool kLong, bool kRows = false>
__global__ void __launch_bounds__(kBlock) k_apply_group_csr(ApplyArgs a) {
  if (!kLong) XF_APPLY_SNAPSHOT(a);
  const TableLayout& L = a.table.L;
  const int ps = a.pstride;
  const PackedLane pl = packed_lane(L.P);
  const CsrDefer cdf(a.csr_long, a.n_max, pl.stride, pl.K);
  const CsrDense dn(a.csr_long, cdf);
  __shared__ u32 s_def[kBlock / kWave];
  const int wib = threadIdx.x / kWave;
  if (!kLong && a.csr_long && lane_id() == 0) s_def[wib] = 0u;
  const int64_t n = kLong ? (int64_t)dn.offs[cdf.waves] : dev_count(a.n_dev, a.n_host, a.n_max);
  const int p = pl.p;
  const u32 P = (u32)L.P;
  const int gbase = lane_id() - p;  // the key group's first lane
  const bool ftrl = L.opt == kFTRL;
  // (B, C) of entry e: words 3e + 1, 3e + 2 of the uint3 entries
  const float* __restrict__ ebc = static_cast<const float*>(a.csr_ent) + 1;
  const float2* stash = ftrl ? reinterpret_cast<const float2*>(a.nz_stash) : nullptr;
  // the lane's entry of the chunk at c0 (past the chain: clamped to its last
  // entry, read but never used -- no branch around the load)
  auto chunk = [&](u32 off, u32 cnt, u32 c0) {
    const float* q = ebc + 3 * (u64)(off + min(c0 + (u32)p, cnt - 1u));
    return make_float2(q[0], q[1]);
  };
  struct A {  // stage A: independent loads
    u32 i, slot, off, cnt;
  };
  // (kRows) the lane's component of entry e
  const float* __restrict__ eg = static_cast<const float*>(a.csr_ent) + 1 + p;
  const u32 ew = (u32)a.csr_ew;
  auto rows_chunk = [&](u32 off, u32 cnt, u32 q0, float (&e)[kCsrRowChunk]) {
#pragma unroll
    for (int k = 0; k < kCsrRowChunk; ++k) e[k] = eg[(u64)(off + min(q0 + (u32)k, cnt - 1u)) * ew];
  };
  struct B {  // stage B: the row words and the first chunk
    RowPre r;
    float2 c0;
    float r0[kCsrRowChunk];
  };
  auto stage_a = [&](int64_t j) {
    A x;
    x.i = kLong ? dn.list[j] : (u32)j;
    x.slot = a.slots[x.i];
    x.off = a.csr_off[x.i];
    x.cnt = a.csr_cnt[x.i];
    return x;
  };
  auto stage_b = [&](const A& x) {
    B y;
    y.r = stash ? row_stash(stash, a.keys, x.i, p, L.P) : row_pre(a.table.words, x.slot, p, L);
    if constexpr (kRows) {
      if (x.cnt) rows_chunk(x.off, x.cnt, 0u, y.r0);
    } else {
      y.c0 = x.cnt ? chunk(x.off, x.cnt, 0u) : make_float2(0.0f, 0.0f);
    }
    return y;
  };
  // (kLong: packed like pass 1 -- spreading the long chains one key group
  // per wave, as k_apply_lr16_csr does, measured 10 % slower at S = 256)
  int64_t j = pl.on ? pl.first : n;
  const int64_t st = pl.stride;
  A a0, a1;
  B b0;
  if (j < n) a0 = stage_a(j);
  if (j + st < n) a1 = stage_a(j + st);
  if (j < n) b0 = stage_b(a0);
  for (; j < n; j += st) {
    const A x = a0;
    const B y = b0;
    a0 = a1;
    if (j + st < n) b0 = stage_b(a0);
    if (j + 2 * st < n) a1 = stage_a(j + 2 * st);
    if (x.slot == kNoSlot || !x.cnt) continue;
    if (!kLong && a.csr_long && x.cnt > kCsrShortChain) {  // (uniform over the key's lanes)
      if (p == 0) cdf.region()[atomicAdd(&s_def[wib], 1u)] = x.i;
      continue;
    }
    float n0 = y.r.s0, z0 = y.r.s1;
    const float w0 = state_weight(y.r.key, y.r.flag != 0u, n0, z0, p, L, a.opt);
    float w_next = w0, sn = ftrl ? sqrtf(n0) : 0.0f;
    bool stale = false;
    auto push = [&](float g) {
      if (stale) w_next = ftrl ? ftrl_weight_sn(z0, sn, a.opt.ftrl) : n0;
      if (ftrl) ftrl_push_sn(n0, z0, sn, w_next, g, a.opt.ftrl);
      else n0 = w_next - a.opt.sgd.lr * g;
      stale = true;
    };
    if constexpr (kRows) {
      float e[kCsrRowChunk];
#pragma unroll
      for (int k = 0; k < kCsrRowChunk; ++k) e[k] = y.r0[k];
      for (u32 q0 = 0; q0 < x.cnt; q0 += kCsrRowChunk) {
        float nx[kCsrRowChunk];
        if (q0 + kCsrRowChunk < x.cnt) rows_chunk(x.off, x.cnt, q0 + kCsrRowChunk, nx);
#pragma unroll
        for (int k = 0; k < kCsrRowChunk; ++k)
          if (q0 + k < x.cnt) push(e[k]);
#pragma unroll
        for (int k = 0; k < kCsrRowChunk; ++k) e[k] = nx[k];
      }
      u32* sp = a.table.words + (u64)x.slot * L.stride;
      if (ftrl) *reinterpret_cast<float2*>(sp + 2 + 2 * p) = make_float2(n0, z0);
      else sp[2 + p] = __float_as_uint(n0);
      if (L.has_flag && p == 0) sp[L.flag_word] = 1u;
      continue;
    }
    const float w_pre = a.pulled ? a.pulled[(size_t)x.i * ps + p] : w0;
    float2 cur = y.c0;
    float2 nxt = x.cnt > P ? chunk(x.off, x.cnt, P) : make_float2(0.0f, 0.0f);
    u32 r = 0;  // q % P
    for (u32 q = 0; q < x.cnt; ++q) {
      if (r == P) {  // (uniform over the key's lanes)
        r = 0;
        cur = nxt;
        if (q + P < x.cnt) nxt = chunk(x.off, x.cnt, q + P);
      }
      const int src = (gbase + (int)r) << 2;
      const float Bv = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(cur.x)));
      const float Cv = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(cur.y)));
      ++r;
      push(p == 0 ? (float)a.fm_D * Bv : Cv - w_pre * Bv);
    }
    u32* sp = a.table.words + (u64)x.slot * L.stride;
    if (ftrl) *reinterpret_cast<float2*>(sp + 2 + 2 * p) = make_float2(n0, z0);
    else sp[2 + p] = __float_as_uint(n0);
    if (L.has_flag && p == 0) sp[L.flag_word] = 1u;
  }
  // (lane 0 -- key group 0, the wave's first key of every iteration -- is the
  // last to leave the loop)
  if (!kLong && a.csr_long && lane_id() == 0) a.csr_long[cdf.gw] = s_def[wib];
}

// A CSR apply: the first pass over every key (short chains applied, long ones
// deferred to the wave's list), then -- with deferral lists -- the scan of the
// waves' counts, the gather into the dense list and the second pass over it.
// Both passes run on `grid` workgroups, `per` keys per wave and iteration.
static void launch_csr_passes(void (*first)(ApplyArgs), void (*second)(ApplyArgs), int grid,
                              int per, const ApplyArgs& a, hipStream_t st) {
  const u32 waves = (u32)grid * (kBlock / kWave);
  const CsrLists g(a.n_max, waves, per);  // (n_max, as the kernels' CsrDefer)
  if (a.csr_long && g.tiles() + waves / 4096 + 8 > (u64)a.csr_long_cap)
    throw std::runtime_error("CSR apply: deferral list too small");
  hipLaunchKernelGGL(first, dim3(grid), dim3(kBlock), 0, st, a);
  if (!a.csr_long) return;
  launch_scan_u32(a.csr_long, a.csr_long + g.offsets(), nullptr, waves, a.csr_long + g.tiles(), st);
  hipLaunchKernelGGL(k_csr_gather, dim3((waves + 3) / 4), dim3(kBlock), 0, st, a.csr_long, a.n_max,
                     per, waves);
  hipLaunchKernelGGL(second, dim3(grid), dim3(kBlock), 0, st, a);
}

void launch_table_apply(const ApplyArgs& a, hipStream_t st) {
  if (a.n_max <= 0) return;
  const TableLayout& L = a.table.L;
  int grid = grid_for(a.n_dev ? a.n_max : a.n_host);
  const int64_t nm = a.n_dev ? a.n_max : a.n_host;
  const bool lr16_slot = L.lr16() && a.pstride == 1;
  const bool lr16 = lr16_slot && a.S == 1 && !a.masks;
  // S > 1 on unique-order sums and slice bits (Engine::train_step's fused LR step)
  const bool lr16_slices = lr16_slot && a.S > 1 && a.masks && !a.masks_rw && !a.grad_map &&
                           !a.zero_after && !a.sum_slices && !a.slice_rows && !a.grp.oidx;
  if (a.nz_stash && !a.keys && !a.grp.oidx && L.P > 1)
    throw std::runtime_error("table_apply: a stash needs the entries' keys");
  if (a.csr_cnt) {
    if (a.zero_after || a.sum_slices || a.grp.oidx || a.grad_map || a.slice_rows)
      throw std::runtime_error("CSR apply: bad arguments (entries come normalised)");
    const int g2 = lr16_slot ? grid : packed_grid(nm, L.P);
    const int per = lr16_slot ? kWave : kWave / L.P;  // keys per wave per iteration
    if (lr16_slot) {
      launch_csr_passes(k_apply_lr16_csr<false>, k_apply_lr16_csr<true>, g2, per, a, st);
    } else if (a.fm_compact && L.P <= kWave && !a.csr_ew) {
      launch_csr_passes(k_apply_group_csr<false>, k_apply_group_csr<true>, g2, per, a, st);
    } else if (a.csr_ew >= csr_row_words(L.P) && !a.fm_compact && L.P <= kWave) {
      launch_csr_passes(k_apply_group_csr<false, true>, k_apply_group_csr<true, true>, g2, per, a,
                        st);
    } else {
      throw std::runtime_error("CSR apply: LR-FTRL 16-byte slots, compact reference-FM rows or full rows");
    }
  } else if (a.grp.oidx) {
    if (a.zero_after) throw std::runtime_error("multi-source apply: bad arguments");
    if (lr16) hipLaunchKernelGGL(k_apply_lr16_multi, dim3(grid), dim3(kBlock), 0, st, a);
    else if (a.S > 1)
      hipLaunchKernelGGL(k_apply_group<true>, dim3(packed_grid(nm, L.P)), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(k_apply_group<false>, dim3(packed_grid(nm, L.P)), dim3(kBlock), 0, st, a);
  } else if (lr16) {
    hipLaunchKernelGGL(k_apply_lr16<false>, dim3(grid), dim3(kBlock), 0, st, a);
  } else if (lr16_slices) {
    hipLaunchKernelGGL(k_apply_lr16<true>, dim3(grid), dim3(kBlock), 0, st, a);
  } else if ((a.pstride >= 2 || (L.P == 1 && a.nz_stash)) && L.P <= kWave) {
    // (LR with several slices and the pull's stash: one lane per key, packed)
    if (a.S > 1)
      hipLaunchKernelGGL(k_apply_group<true>, dim3(packed_grid(nm, L.P)), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(k_apply_group<false>, dim3(packed_grid(nm, L.P)), dim3(kBlock), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_apply_generic, dim3(grid), dim3(kBlock), 0, st, a);
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
