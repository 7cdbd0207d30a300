// xflow-amd: MVM forward + backward (k_mvm2) and its dispatch (gfx950).
// MVM, one lane per row with register-resident latent sums.  Each occurrence's
// pulled row [v_0..v_{D-1}, pad] is read with dwordx4 loads once per pass; the
// per-field sums S[g][k] are the occurrence's own v when every field occurs at
// most once in the row (CTR rows; checked per row with a 64-bit field mask),
// otherwise they are summed over the row's occurrences of that field.  The
// backward aggregates each occurrence's D-vector per (key, slice) in the LDS
// column tables (vector flush) instead of D global atomics per occurrence.
// Reference math: mvm_worker.cc:137-218 (product over fields [0, G), G = maxf
// (compat) or maxf + 1 (fixed); gradient loss*M_k/(1+S) when S != 0).
#include "model_common.h"

namespace xflow {
namespace hip {

template <int D, bool kGrad, bool kAgg, bool kRed = false>
__global__ void __launch_bounds__(mvm_block_for(D, kRed)) k_mvm2(FwdArgs a) {
  constexpr int PS = mvm_ps(D);
  constexpr int BLOCK = mvm_block_for(D, kRed);
  constexpr int LOG2 = ilog2c(2 * BLOCK);
  __shared__ u32 s_tag[kAgg ? 2 : 1][kAgg ? (1 << LOG2) : 1];
  __shared__ float s_acc[kAgg ? 2 : 1][kAgg ? (1 << LOG2) * PS : 1];
  __shared__ int s_wmax[BLOCK / kWave];
  const BatchView& b = a.batch;
  const bool compat = a.model.mvm_math == kMvmCompat;
  const u32* __restrict__ pos = a.pos;
  const float* __restrict__ wp = a.wpull;
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool active = r < b.rows;
  RowSpan rs;
  if (active) rs = row_span(b, r);
  const int len = rs.len;
  // fields of the row: mask of those < 64, duplicate / out-of-mask flags
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
  // sum of the row's latent rows of field f, component-wise (slow path)
  auto field_sum = [&](int f, float (&S)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) S[k] = 0.0f;
    for (int j = 0; j < len; ++j) {
      if (b.fgid[rs.at(j)] != f) continue;
      float w[PS];
      load_row<PS>(wp, pos[rs.at(j)], w);
#pragma unroll
      for (int k = 0; k < D; ++k) S[k] += w[k];
    }
  };
  float M[D];
  float y = 0.0f;
  StatAcc st;
  float loss = 0.0f;
  if (active) {
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
#pragma unroll
    for (int k = 0; k < D; ++k) M[k] = complete ? 1.0f : 0.0f;
    if (complete) {
      if (!dup && sorted) {
        // occurrence order = field order g = 0..G-1 (the reference's product order)
        for (int j = 0; j < len; ++j) {
          if (b.fgid[rs.at(j)] >= G) break;
          float w[PS];
          load_row<PS>(wp, pos[rs.at(j)], w);
#pragma unroll
          for (int k = 0; k < D; ++k) M[k] *= w[k];
        }
      } else if (!dup) {
        for (int g = 0; g < G; ++g) {
          int jj = 0;
          while (b.fgid[rs.at(jj)] != g) ++jj;
          float w[PS];
          load_row<PS>(wp, pos[rs.at(jj)], w);
#pragma unroll
          for (int k = 0; k < D; ++k) M[k] *= w[k];
        }
      } else {
        for (int g = 0; g < G; ++g) {
          float S[D];
          field_sum(g, S);
#pragma unroll
          for (int k = 0; k < D; ++k) M[k] *= S[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) y += M[k];
    const float p = sigmoid_ref(y);
    const float lab = b.labels[r];
    loss = p - lab;
    if (a.pctr) a.pctr[r] = p;
    st.add(p, lab);
  }
  if constexpr (kGrad) {
    const u32 s = active ? (u32)slice_of(b, r, a.S) : 0u;
    const u32 S = (u32)a.S;
    // gradient of the row's j-th occurrence
    auto contrib = [&](int j, float (&c)[D]) {
      float Sf[D];
      if (!dup) {
        float w[PS];
        load_row<PS>(wp, pos[rs.at(j)], w);
#pragma unroll
        for (int k = 0; k < D; ++k) Sf[k] = w[k];
      } else {
        field_sum(b.fgid[rs.at(j)], Sf);
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
        c[k] = (Sf[k] == 0.0f) ? 0.0f
                               : (float)((double)loss * ((double)M[k] / (1.0 + (double)Sf[k])));
    };
    if constexpr (kRed) {
      // Dup-free rows: S of an occurrence is the key's own v, so the gradient
      // factorises as T_k/(1+v_k) with T = loss*M per row: the row's T goes
      // to red_rowv and the vector-record reduction (k_fm_std_red<D-1, ..,
      // kSplit> + k_red_sum_vec<.., kMvm>) sums T per (key, slice) and
      // divides once.  Rows with a repeated field (S = field sum): global
      // atomics, and T = 0 (their occurrences still leave records, for the
      // slice bits of a multi-slice step).
      float tmax = 0.0f;  // |T| of the row (the step's fixed-point scale)
      if (active) {
        float* t = a.red_rowv + (size_t)r * PS;
#pragma unroll
        for (int k = 0; k < PS; ++k) {
          const float v = (!dup && k < D) ? loss * M[k] : 0.0f;
          t[k] = v;
          // (a non-finite T maxes to inf: fx_scale_bits then keeps the
          // static 2^44 scale and the clamp flags the step)
          tmax = fmaxf(tmax, v == v ? fabsf(v) : INFINITY);
        }
      }
      {
        __shared__ float s_tmax[BLOCK / kWave];
        tmax = wave_max(tmax);
        if (threadIdx.x % kWave == 0) s_tmax[threadIdx.x / kWave] = tmax;
        __syncthreads();
        if (threadIdx.x == 0) {
          float m = 0.0f;
#pragma unroll
          for (int w = 0; w < BLOCK / kWave; ++w) m = fmaxf(m, s_tmax[w]);
          if (m > 0.0f) atomicMax(a.red_vmax, __float_as_uint(m));  // (>= 0: bits order as values)
          if (!(m <= 3.0e38f)) atomicOr(a.fx_bad, 2u);  // non-finite T: a diverged model
          if (blockIdx.x == 0) *a.red_vmax_next = 0u;  // (the next step's word)
          if (blockIdx.x == 0 && a.red_dup_next) *a.red_dup_next = 0u;

        }
      }
      // repeated-field rows on the unique-row / CSR outputs: fixed-point
      // records for the order-free passes after the reduction (MvmDup)
      const bool md = a.mdup.rec && (a.red_out || a.red_csr.cnt);
      // (one flag write per wave with a repeated-field row added by atomics: FwdArgs::red_dup)
      if (a.red_dup && !md && __ballot(active && dup) && lane_id() == 0) atomicOr(a.red_dup, 1u);
      float cmax = 0.0f;
      if (active && dup && md) {
        const int ew = a.mdup.ew;
        for (int j = 0; j < len; ++j) {
          float c[D];
          contrib(j, c);
          const u32 pj = pos[rs.at(j)];
          if (pj == a.trash_pos) continue;
          // target: the (key, slice) dest (CSR; resolved to its entry later)
          // or the key's unique-order row
          const u32 tgt = a.red_csr.cnt ? pj * S + s : uix(a.red_inv, pj);
          if (tgt == 0xFFFFFFFFu) continue;
          const u32 at = atomicAdd(a.mdup.n, 1u);
          if (at >= (u32)a.mdup.cap) continue;  // (cannot happen: <= one per occurrence)
          float* rec = a.mdup.rec + (size_t)at * ew;
          rec[0] = __uint_as_float(tgt);
#pragma unroll
          for (int k = 0; k < D; ++k) {
            rec[1 + k] = c[k];
            cmax = fmaxf(cmax, c[k] == c[k] ? fabsf(c[k]) : INFINITY);
          }
        }
      } else if (active && dup) {
        for (int j = 0; j < len; ++j) {
          float c[D];
          contrib(j, c);
          const u32 pj = pos[rs.at(j)];
          float* g = a.grad + ((size_t)pj * S + s) * PS;
          if (a.red_out) {  // (one slice: the unique-order rows the reduction adds to)
            const u32 o = uix(a.red_inv, pj);
            if (o == 0xFFFFFFFFu) continue;
            g = a.red_out + (size_t)o * PS;
          }
#pragma unroll
          for (int k = 0; k < D; ++k) atomicAdd(&g[k], c[k]);
        }
      }
      if (md) {  // (every lane: the wave's largest |c| sets the step's scale)
        cmax = wave_max(cmax);
        if (lane_id() == 0 && cmax > 0.0f) {
          atomicMax(a.mdup.vmax, __float_as_uint(fminf(cmax, 3.4e38f)));
          if (!(cmax <= 3.0e38f)) atomicOr(a.fx_bad, 2u);  // non-finite: a diverged model
        }
      }
    } else if constexpr (!kAgg) {
      for (int j = 0; j < len; ++j) {
        float c[D];
        contrib(j, c);
        float* g = a.grad + ((size_t)pos[rs.at(j)] * S + s) * PS;
#pragma unroll
        for (int k = 0; k < D; ++k) atomicAdd(&g[k], c[k]);
      }
    } else {
      ColumnAgg<PS, LOG2> agg{s_tag, s_acc};
      agg.init();
      const int m = wave_max(len);
      if (threadIdx.x % kWave == 0) s_wmax[threadIdx.x / kWave] = m;
      __syncthreads();
      int maxlen = 0;
#pragma unroll
      for (int w = 0; w < BLOCK / kWave; ++w) maxlen = max(maxlen, s_wmax[w]);
      for (int j = 0; j < maxlen; ++j) {
        const int t = j & 1;
        if (j < len) {
          float c[D];
          contrib(j, c);
          const int h = agg.insert(t, pos[rs.at(j)] * S + s);
#pragma unroll
          for (int k = 0; k < D; ++k) agg.add(t, h, k, c[k]);
        }
        __syncthreads();
        agg.flush(t, a.grad);
      }
    }
  }
  flush_stats<BLOCK>(st, a.stats, a.fx_bad);
}

template <bool kGrad>
void dispatch_mvm(const FwdArgs& a, hipStream_t st) {
  const bool agg = kGrad && a.agg_ok;
  const bool red = kGrad && a.red_rowv && red_path(a, red_cap(a));
  if (a.red_masks && a.S > 1 && !(red && a.model.kernel_dim() >= 2))
    throw std::runtime_error("red_masks need the MVM reduction path");
  switch (a.model.kernel_dim()) {
#define XF_MVM_CASE(DD)                                                                  \
  case DD: {                                                                             \
    constexpr int B = mvm_block(DD);                                                     \
    const int g = (int)((a.batch.rows + B - 1) / B);                                     \
    if (a.red_out && !(red && DD >= 2))                                                  \
      throw std::runtime_error("MVM red_out needs the bucket reduction");                \
    if (red && DD >= 2) {                                                                \
      constexpr int R = kMvmGroupRows;                                                   \
      const int gr = (int)((a.batch.rows + R - 1) / R);                                  \
      hipLaunchKernelGGL((k_mvm2<DD, kGrad, false, true>), dim3(gr), dim3(R), 0, st, a); \
      launch_vec_reduction<(DD >= 2 ? DD - 1 : 1), true>(a, st);                          \
    } else if (agg) {                                                                    \
      hipLaunchKernelGGL((k_mvm2<DD, kGrad, true>), dim3(g), dim3(B), 0, st, a);         \
    } else {                                                                             \
      hipLaunchKernelGGL((k_mvm2<DD, kGrad, false>), dim3(g), dim3(B), 0, st, a);        \
    }                                                                                    \
    break;                                                                               \
  }
    XF_MVM_CASE(1) XF_MVM_CASE(2) XF_MVM_CASE(4) XF_MVM_CASE(8) XF_MVM_CASE(10) XF_MVM_CASE(16)
    XF_MVM_CASE(32)
#undef XF_MVM_CASE
    default:
      throw std::runtime_error("MVM: unsupported v_dim (1,2,4,8,10,16,32)");
  }
}
template void dispatch_mvm<true>(const FwdArgs&, hipStream_t);
template void dispatch_mvm<false>(const FwdArgs&, hipStream_t);

}  // namespace hip
}  // namespace xflow
