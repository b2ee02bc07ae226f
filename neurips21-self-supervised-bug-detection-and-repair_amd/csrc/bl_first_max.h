// First-maximum search over a model's flat fp32 output, shared by the kernels that judge `predict` minibatches on the device
// (bl_report.hip, bl_evaluate.hip).  Values are read as fp64 through int32 indices; a candidate is a (value, index) pair with
// index -1 = "none yet"; NaNs never enter a search (the callers apply the rule for a NaN in front themselves).  Every
// reduction is a fixed tree: wave butterfly, then the waves in wave order.
#pragma once
#include "bl_common.h"

namespace {
__device__ __forceinline__ double rp_load(const float* src, int64_t n_src, int32_t j) {
  // an index outside src (the host never sends one) reads as NaN instead of out of bounds
  return (j >= 0 && (int64_t)j < n_src) ? (double)src[j] : __builtin_nan("");
}

__device__ __forceinline__ int32_t rp_at(const int32_t* a, int64_t n, int64_t i, int32_t otherwise) {
  return (i >= 0 && i < n) ? a[i] : otherwise;
}

// Candidate (value, index) a replaces b in a first-maximum search: greater value, or the same value earlier.  NaNs never enter.
__device__ __forceinline__ bool rp_better(double va, int ia, double vb, int ib) { return ib < 0 || va > vb || (va == vb && ia < ib); }

__device__ __forceinline__ void rp_wave_argmax(double& v, int& i) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, BL_WAVE);
    const int oi = __shfl_xor(i, o, BL_WAVE);
    if (oi >= 0 && rp_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}
}  // namespace
