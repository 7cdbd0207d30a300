// xflow-amd: one-launch scoring from a frozen table (gfx950): LR (k_serve_lr)
// and, further down, FM and MVM (k_serve_fm, k_serve_mvm).
//
// A serving snapshot of an LR model (docs/DESIGN.md §2) is a small read-only
// table of 16-byte slots {key, w, pad}: it sits in L2 / the Infinity Cache,
// and a request's cost is then the launches of dedup -> pull -> forward, not
// their memory traffic.  k_serve_lr does the whole request in one launch: a
// lane owns a row, probes the table for every occurrence of it directly and
// sums the weights in occurrence order -- the order the forward kernels sum a
// row's pulled weights in (k_lr), so the prediction is the same function of
// the same floats.  No scratch, no atomics on the result: deterministic.
//
// One lane per row favours field-major batches: there a wave's key loads of
// one field are contiguous, while row-major and CSR keys of neighbouring
// lanes lie a row apart (uncoalesced, served by L1 / L2), and one long CSR
// row keeps its lane busy while the wave's others idle.  Correct in every
// layout; tools/serve_bench.py measures fixed-width rows of 39 fields only.
#include "model_common.h"

namespace xflow {
namespace hip {

// Occurrences a lane keeps in flight: their key loads are issued together,
// then their home-slot loads (one dwordx4 each), before any is resolved --
// as in k_pull_lr16, memory-level parallelism is what matters.  A chain that
// continues past the home slot (rare at the snapshot's load <= 0.5) is
// walked slot by slot.
constexpr int kServeItems = 8;
// one wave per workgroup: a lane's work is a chain of dependent round trips,
// so small batches should spread over as many CUs as they have waves
constexpr int kServeBlock = kWave;

__global__ void __launch_bounds__(kServeBlock) k_serve_lr(ServeLrArgs a) {
  const BatchView& b = a.batch;
  const TableView& t = a.table;
  const uint4* slots = reinterpret_cast<const uint4*>(t.words);
  const int64_t r = (int64_t)blockIdx.x * kServeBlock + threadIdx.x;
  const bool active = r < b.rows;
  StatAcc st;
  if (active) {
    const RowSpan rs = row_span(b, r);
    float wx = 0.0f;
    for (int j0 = 0; j0 < rs.len; j0 += kServeItems) {
      u64 key[kServeItems], s[kServeItems];
      uint4 v[kServeItems];
#pragma unroll
      for (int q = 0; q < kServeItems; ++q) {
        const bool on = j0 + q < rs.len;
        key[q] = on ? sanitize_key(b.keys[rs.at(j0 + q)]) : 0ull;
        s[q] = table_home(t, fmix64(key[q]));
      }
#pragma unroll
      for (int q = 0; q < kServeItems; ++q)
        if (j0 + q < rs.len) v[q] = slots[s[q]];
#pragma unroll
      for (int q = 0; q < kServeItems; ++q) {
        if (j0 + q >= rs.len) continue;
        float w = 0.0f;  // an absent key adds 0.0f
        uint4 cur = v[q];
        u64 sq = s[q];
        // slots at distance >= probe_limit are never examined (bounded chains)
        for (u64 c = 0; c < t.probe_limit; ++c) {
          const u64 k = (u64)cur.x | ((u64)cur.y << 32);
          if (k == key[q]) {
            w = __uint_as_float(cur.z);
            break;
          }
          if (k == kEmptyKey) break;
          sq = table_next(t, sq);
          cur = slots[sq];
        }
        wx += w;
      }
    }
    const float p = sigmoid_ref(wx);
    if (a.pctr) a.pctr[r] = p;
    if (a.stats) st.add(p, b.labels[r]);
  }
  flush_stats<kServeBlock>(st, a.stats);
}

void launch_serve_lr(const ServeLrArgs& a, hipStream_t st) {
  const TableLayout& L = a.table.L;
  if (L.opt != kFrozen || L.P != 1 || L.stride != 4)
    throw std::runtime_error("serve_lr: needs a frozen LR table (16-byte slots)");
  if (a.batch.rows <= 0) return;
  if (a.batch.rows > 0x7fffffffll * kServeBlock) throw std::runtime_error("serve_lr: too many rows");
  const int64_t g = (a.batch.rows + kServeBlock - 1) / kServeBlock;
  hipLaunchKernelGGL(k_serve_lr, dim3((unsigned)g), dim3(kServeBlock), 0, st, a);
  XF_HIP_CHECK(hipGetLastError());
}


// ---------------------------------------------------------------------------
// FM and MVM: the same request shape on slots of 2 + P words {key, w_0 ..
// w_{P-1}, pad}.  A lane keeps N occurrences in flight: their key loads, then
// the first dwordx4 of their home slots (the key and the first two weights),
// then -- once every chain is walked -- the rest of the N resolved slots, so a
// chunk of N occurrences costs two dependent round trips whatever the slot
// width.  The arithmetic on the weights is the unfused forward's, operation
// for operation (docs/DESIGN.md §2): the build has no floating-point
// contraction (k_fm, k_fm_vals, k_pull_values and k_mvm2 multiply and add
// separately -- checked in their ISA), and the products below say so
// explicitly.  A key that is not in the table reads absent_weight, the pull's
// own rule; the kernel-width padding (v_dim 3 runs at 4) reads 0.0f as the
// pull writes it.
// ---------------------------------------------------------------------------
// words of the widest slot that holds nw weights, and the occurrences in
// flight per lane: the resolved slots stay in registers (N * SW words)
constexpr int serve_sw(int nw) { return (2 + nw + 3) & ~3; }
constexpr int serve_items(int nw) { return serve_sw(nw) <= 16 ? 8 : 4; }

template <int NW>  // weights per key at the kernel width (FM 1 + D, MVM D)
struct ServeProbe {
  static constexpr int SW = serve_sw(NW), Q = SW / 4, N = serve_items(NW);
  u64 key[N];
  uint4 w4[N][Q];  // the key's slot, or what was loaded on the way (absent)
  u32 hit = 0;     // bit q: key[q] is in the table

  // occurrences j0 .. j0 + C - 1 of the row (those past its end: off) into
  // items 0 .. C - 1; C = 1: one probe (MVM's untuned product orders)
  template <int C = N>
  __device__ __forceinline__ void load(const TableView& t, const BatchView& b, const RowSpan& rs,
                                       int j0) {
    const uint4* slots = reinterpret_cast<const uint4*>(t.words);
    const u64 q4 = (u64)(t.L.stride / 4);
    u64 s[C];
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const bool on = j0 + q < rs.len;
      key[q] = on ? sanitize_key(b.keys[rs.at(j0 + q)]) : 0ull;
      s[q] = table_home(t, fmix64(key[q]));
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
      w4[q][0] = make_uint4(0u, 0u, 0u, 0u);
      if (j0 + q < rs.len) w4[q][0] = slots[s[q] * q4];
    }
    hit = 0u;
#pragma unroll
    for (int q = 0; q < C; ++q) {
      if (!(j0 + q < rs.len)) continue;
      uint4 cur = w4[q][0];
      u64 sq = s[q];
      // slots at distance >= probe_limit are never examined (bounded chains)
      for (u64 c = 0; c < t.probe_limit; ++c) {
        const u64 k = (u64)cur.x | ((u64)cur.y << 32);
        if (k == key[q]) {
          hit |= 1u << q;
          w4[q][0] = cur;
          s[q] = sq;
          break;
        }
        if (k == kEmptyKey) break;
        sq = table_next(t, sq);
        cur = slots[sq * q4];
      }
    }
#pragma unroll
    for (int q = 0; q < C; ++q)
#pragma unroll
      for (int i = 1; i < Q; ++i) {
        w4[q][i] = make_uint4(0u, 0u, 0u, 0u);
        if (((hit >> q) & 1u) && (u64)i < q4) w4[q][i] = slots[s[q] * q4 + (u64)i];
      }
  }

  // the NW weights of item q (the same q in every lane): the slot's P, or an
  // absent key's, then the padding
  __device__ __forceinline__ void weights(int q, const TableLayout& L, const OptSpec& o,
                                          float (&w)[NW]) const {
    u64 k = 0ull;
    bool found = false;
    u32 sw[SW];
#pragma unroll
    for (int i = 0; i < SW; ++i) sw[i] = 0u;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (q == i) {
        k = key[i];
        found = ((hit >> i) & 1u) != 0u;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          sw[4 * j] = w4[i][j].x;
          sw[4 * j + 1] = w4[i][j].y;
          sw[4 * j + 2] = w4[i][j].z;
          sw[4 * j + 3] = w4[i][j].w;
        }
      }
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (found && i < L.P) ? __uint_as_float(sw[2 + i]) : 0.0f;
    if (!found) {
      // (one copy of the lazy init's code: a loop over the real params)
#pragma unroll 1
      for (int p = 0; p < L.P; ++p) {
        const float v = absent_weight(k, p, L, o);
#pragma unroll
        for (int i = 0; i < NW; ++i)
          if (i == p) w[i] = v;
      }
    }
  }
};

// FM.  Full rows (k_fm): per occurrence wx += w, then vs[k] += v_k and
// vp += v_k * v_k for k in order; standard math sums vs[k]^2 in k order.
// Compact reference rows (ServeArgs::fm_vals; k_pull_values -> k_fm_vals):
// per key sv = Σ_k v_k and qv = Σ_k v_k^2 over its real params in order, per
// occurrence wx += w, vsum += sv, vp += qv -- not the same float.
template <int D>
__global__ void __launch_bounds__(kServeBlock) k_serve_fm(ServeArgs a) {
  constexpr int NW = 1 + D;
  using Probe = ServeProbe<NW>;
  const BatchView& b = a.batch;
  const TableView& t = a.table;
  const bool standard = a.model.fm_math == kFmStandard;
  const bool compact = a.fm_vals;
  const int64_t r = (int64_t)blockIdx.x * kServeBlock + threadIdx.x;
  const bool active = r < b.rows;
  StatAcc st;
  if (active) {
    const RowSpan rs = row_span(b, r);
    float vs[D];
#pragma unroll
    for (int k = 0; k < D; ++k) vs[k] = 0.0f;
    float wx = 0.0f, vp = 0.0f, vsum = 0.0f;
    Probe pr;
    for (int j0 = 0; j0 < rs.len; j0 += Probe::N) {
      pr.load(t, b, rs, j0);
#pragma unroll 1
      for (int q = 0; q < Probe::N; ++q) {
        if (j0 + q >= rs.len) break;
        float w[NW];
        pr.weights(q, t.L, a.opt, w);
        wx = __fadd_rn(wx, w[0]);
        if (compact) {
          float sv = 0.0f, qv = 0.0f;
#pragma unroll
          for (int k = 0; k < D; ++k)
            if (1 + k < t.L.P) {
              sv = __fadd_rn(sv, w[1 + k]);
              qv = __fadd_rn(qv, __fmul_rn(w[1 + k], w[1 + k]));
            }
          vsum = __fadd_rn(vsum, sv);
          vp = __fadd_rn(vp, qv);
        } else {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            vs[k] = __fadd_rn(vs[k], w[1 + k]);
            vp = __fadd_rn(vp, __fmul_rn(w[1 + k], w[1 + k]));
          }
        }
      }
    }
    float y;
    if (standard) {
      float sq = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) sq = __fadd_rn(sq, __fmul_rn(vs[k], vs[k]));
      y = __fadd_rn(wx, __fmul_rn(0.5f, __fsub_rn(sq, vp)));
    } else {
      if (!compact) {
#pragma unroll
        for (int k = 0; k < D; ++k) vsum = __fadd_rn(vsum, vs[k]);
      }
      y = __fadd_rn(wx, __fsub_rn(__fmul_rn(vsum, vsum), vp));
    }
    const float p = sigmoid_ref(y);
    if (a.pctr) a.pctr[r] = p;
    if (a.stats) st.add(p, b.labels[r]);
  }
  flush_stats<kServeBlock>(st, a.stats);
}

// MVM (k_mvm2's forward): the row's field mask and its `complete` test, then
// the product over fields [0, G) in one of three orders -- a sorted row of
// unique fields in occurrence order (the chunked probe), an unsorted one by
// field id, a row with a repeated or >= 64 field id by per-field sums.  The
// last two probe the table once per (field, occurrence): correct, not tuned.
template <int D>
__global__ void __launch_bounds__(kServeBlock) k_serve_mvm(ServeArgs a) {
  using Probe = ServeProbe<D>;
  const BatchView& b = a.batch;
  const TableView& t = a.table;
  const bool compat = a.model.mvm_math == kMvmCompat;
  const int64_t r = (int64_t)blockIdx.x * kServeBlock + threadIdx.x;
  const bool active = r < b.rows;
  StatAcc st;
  if (active) {
    const RowSpan rs = row_span(b, r);
    const int len = rs.len;
    unsigned long long mask = 0ull;
    bool dup = false, sorted = true;
    int maxf = 0;
    for (int j = 0; j < len; ++j) {
      const int f = b.fgid[rs.at(j)];
      if (j > 0 && f <= maxf) sorted = false;
      maxf = max(maxf, f);
      if (f < 0 || f >= 64) {
        dup = true;
      } else {
        if ((mask >> f) & 1ull) dup = true;
        mask |= 1ull << f;
      }
    }
    const int G = compat ? maxf : maxf + 1;
    bool complete;  // every field g < G occurs (else some S[g] = 0 and M = 0)
    if (dup || G > 64) {
      complete = true;
      for (int g = 0; g < G && complete; ++g) {
        bool found = false;
        for (int j = 0; j < len && !found; ++j) found = b.fgid[rs.at(j)] == g;
        complete = found;
      }
    } else {
      const unsigned long long need = G >= 64 ? ~0ull : ((1ull << G) - 1ull);
      complete = (mask & need) == need;
    }
    float M[D];
#pragma unroll
    for (int k = 0; k < D; ++k) M[k] = complete ? 1.0f : 0.0f;
    Probe pr;
    if (complete) {
      if (!dup && sorted) {
        bool more = true;
        for (int j0 = 0; j0 < len && more; j0 += Probe::N) {
          pr.load(t, b, rs, j0);
#pragma unroll 1
          for (int q = 0; q < Probe::N; ++q) {
            if (j0 + q >= len || b.fgid[rs.at(j0 + q)] >= G) {
              more = false;
              break;
            }
            float w[D];
            pr.weights(q, t.L, a.opt, w);
#pragma unroll
            for (int k = 0; k < D; ++k) M[k] = __fmul_rn(M[k], w[k]);
          }
        }
      } else if (!dup) {
        for (int g = 0; g < G; ++g) {
          int jj = 0;
          while (b.fgid[rs.at(jj)] != g) ++jj;
          float w[D];
          pr.template load<1>(t, b, rs, jj);
          pr.weights(0, t.L, a.opt, w);
#pragma unroll
          for (int k = 0; k < D; ++k) M[k] = __fmul_rn(M[k], w[k]);
        }
      } else {
        for (int g = 0; g < G; ++g) {
          float S[D];
#pragma unroll
          for (int k = 0; k < D; ++k) S[k] = 0.0f;
          for (int j = 0; j < len; ++j) {
            if (b.fgid[rs.at(j)] != g) continue;
            float w[D];
            pr.template load<1>(t, b, rs, j);
            pr.weights(0, t.L, a.opt, w);
#pragma unroll
            for (int k = 0; k < D; ++k) S[k] = __fadd_rn(S[k], w[k]);
          }
#pragma unroll
          for (int k = 0; k < D; ++k) M[k] = __fmul_rn(M[k], S[k]);
        }
      }
    }
    float y = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) y = __fadd_rn(y, M[k]);
    const float p = sigmoid_ref(y);
    if (a.pctr) a.pctr[r] = p;
    if (a.stats) st.add(p, b.labels[r]);
  }
  flush_stats<kServeBlock>(st, a.stats);
}

void launch_serve_model(const ServeArgs& a, hipStream_t st) {
  const TableLayout& L = a.table.L;
  const ModelSpec& m = a.model;
  if (m.kind != kFM && m.kind != kMVM)
    throw std::runtime_error("serve_model: FM or MVM (LR: serve_lr)");
  if (L.opt != kFrozen || L.has_flag || L.sp != 1 || L.P != m.P() || L.p_w != m.p_w() ||
      L.stride != ((2 + L.P + 3) & ~3))
    throw std::runtime_error("serve_model: needs the model's frozen table (2 + P words per slot)");
  if (m.kind == kFM && m.fm_math == kFmStandard && m.fm_mfma)
    throw std::runtime_error("serve_model: fm_mfma sums a row another way (the unfused path)");
  if (a.fm_vals && !(m.kind == kFM && m.fm_math == kFmReference))
    throw std::runtime_error("serve_model: fm_vals is reference-math FM");
  if (a.batch.rows <= 0) return;
  if (m.kind == kMVM && !a.batch.fgid && a.batch.nnz > 0)
    throw std::runtime_error("MVM needs field ids (fgid)");
  if (a.batch.rows > 0x7fffffffll * kServeBlock) throw std::runtime_error("serve_model: too many rows");
  const dim3 g((unsigned)((a.batch.rows + kServeBlock - 1) / kServeBlock)), blk(kServeBlock);
  switch (m.kernel_dim()) {
#define XF_SERVE_CASE(DD)                                                    \
  case DD:                                                                   \
    if (m.kind == kFM) hipLaunchKernelGGL(k_serve_fm<DD>, g, blk, 0, st, a); \
    else hipLaunchKernelGGL(k_serve_mvm<DD>, g, blk, 0, st, a);              \
    break;
    XF_SERVE_CASE(1) XF_SERVE_CASE(2) XF_SERVE_CASE(4) XF_SERVE_CASE(8) XF_SERVE_CASE(10)
    XF_SERVE_CASE(16) XF_SERVE_CASE(32)
#undef XF_SERVE_CASE
    default:
      throw std::runtime_error("serve_model: unsupported v_dim (1,2,4,8,10,16,32)");
  }
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
