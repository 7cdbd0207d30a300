// xflow-amd: one-launch LR scoring from a frozen table (gfx950).
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

}  // namespace hip
}  // namespace xflow
