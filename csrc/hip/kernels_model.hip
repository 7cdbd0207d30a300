// xflow-amd: fused forward + backward kernels for LR / FM / MVM (gfx950):
// the entry point.  The kernels and their dispatch are in kernels_lr.hip,
// kernels_fm.hip and kernels_mvm.hip, the gradient reductions in
// kernels_reduce.hip and kernels_reduce_vec.hip, what they share in
// model_common.h.
//
// One lane per row.  The pulled parameters of the batch's unique keys live in
// a dense buffer indexed by the key's dedup-scratch slot (`wpull[pos]`), so a
// row gathers its features with one dependent load each and never touches the
// persistent table.  The loss-weighted gradient contributions are added
// (un-normalised, like the reference's running sums) into `grad[pos][slice]`;
// the per-slice division by row count happens when the gradients are pushed.
//
// Reference math:
//   LR   lr_worker.cc:121-143 (loss), :100-119 (gradient)
//   FM   fm_worker.cc:159-202 (loss), :126-157 (gradient)      [kFmReference]
//   MVM  mvm_worker.cc:172-218 (loss), :137-170 (gradient)
#include "model_common.h"

namespace xflow {
namespace hip {

void launch_forward_backward(const FwdArgs& a, hipStream_t st) {
  if (a.batch.rows <= 0) return;
  const bool grad = a.grad != nullptr;
  switch (a.model.kind) {
    case kLR:
      dispatch_lr(a, st);
      break;
    case kFM:
      if (a.lead) throw std::runtime_error("leader-encoded positions: LR only");
      if (grad) dispatch_fm<true>(a, st);
      else dispatch_fm<false>(a, st);
      break;
    case kMVM:
      // (a batch without occurrences has no field ids to point at)
      if (a.lead) throw std::runtime_error("leader-encoded positions: LR only");
      if (!a.batch.fgid && a.batch.nnz > 0) throw std::runtime_error("MVM needs field ids (fgid)");
      if (grad) dispatch_mvm<true>(a, st);
      else dispatch_mvm<false>(a, st);
      break;
    default:
      throw std::runtime_error("unknown model kind");
  }
  XF_HIP_CHECK(hipGetLastError());
}

__global__ void k_slice_masks(BatchView b, const u32* __restrict__ pos, u32* __restrict__ tmask,
                              int S) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.rows) return;
  const RowSpan rs = row_span(b, r);
  u32 bit = 1u << slice_of(b, r, S);
  for (int j = 0; j < rs.len; ++j) atomicOr(&tmask[pos[rs.at(j)]], bit);
}

void launch_slice_masks(const BatchView& b, const u32* pos, u32* tmask, hipStream_t st) {
  if (b.rows <= 0) return;
  int S = b.slice_rows > 0 ? (int)((b.rows + b.slice_rows - 1) / b.slice_rows) : 1;
  hipLaunchKernelGGL(k_slice_masks, dim3((int)((b.rows + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, b, pos, tmask, S);
  XF_HIP_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace xflow
