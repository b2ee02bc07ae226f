// What the forward-only service kernels share (bl_report.hip, bl_evaluate.hip, bl_confidence.hip, bl_distill.hip, bl_selfsup.hip,
// bl_ensemble.hip, bl_varmisuse_predict.hip; bl_dedup.hip for the offsets): they read segments of a model's flat fp32 output
// through CSR offsets and int32 indices, work in fp64, and must give the same bits on every run.  The contract, stated once:
//
//   Offsets  A CSR offset is clamped into [0, hi] and a row's length is never negative, so a malformed offset array (the host
//            never sends one) reads nothing out of bounds.  bl_load_f64 / bl_at_i32 check the index they are given likewise.
//   Sums     Fixed trees, no atomics.  bl_wave_sum_f64: the xor butterfly, strides BL_WAVE / 2 .. 1.  bl_block_sum_f64: that,
//            then the waves' sums added in wave order.  bl_tree_sum_f64: one value per thread in LDS, halved from stride
//            THREADS / 2 down to 1.  What a thread adds up BEFORE the call is its caller's business (stride order everywhere).
//   Maxima   A candidate is a (value, index) pair, index -1 = "none yet"; bl_better is the one ordering: greater value, or the
//            same value at the lower index, so a search returns the FIRST maximum whatever the geometry.  NaNs never enter a
//            search: the caller leaves them out and applies its own rule for a NaN in front (Python's max() keeps it).
//            The value type is the caller's: fp64 everywhere but in bl_ensemble.hip, which searches the fp32 values as they
//            are (widening is exact and keeps the order, and only the index leaves that search).
//   Barriers bl_block_sum_f64 and bl_block_argmax synchronise BEFORE they write their LDS scratch ("the previous use has been
//            read") and once after; they do not synchronise on the way out.  So back-to-back calls on the same scratch are safe,
//            every thread of the workgroup must make the call, and a caller that writes the scratch itself afterwards needs its
//            own barrier.  bl_tree_sum_f64 ends on a barrier; its result is s_acc[0].
//
// Everything here is inline, so a file's `#pragma clang fp contract(off)` governs the copies compiled into it.
#pragma once
#include "bl_common.h"

namespace {
// ---- offsets and loads ----
__device__ __forceinline__ int64_t bl_clamp_off(int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : (v > hi ? hi : v); }

// row `row` of a CSR offset array over hi entries: its clamped start in `begin`, its length (>= 0) returned
template <class Off>
__device__ __forceinline__ int64_t bl_csr_row(const Off* off, int64_t row, int64_t hi, int64_t& begin) {
  begin = bl_clamp_off(off[row], hi);
  const int64_t end = bl_clamp_off(off[row + 1], hi);
  return end > begin ? end - begin : 0;
}

__device__ __forceinline__ double bl_load_f64(const float* src, int64_t n_src, int32_t j) {
  // an index outside src (the host never sends one) reads as NaN instead of out of bounds
  return (j >= 0 && (int64_t)j < n_src) ? (double)src[j] : __builtin_nan("");
}

__device__ __forceinline__ int32_t bl_at_i32(const int32_t* a, int64_t n, int64_t i, int32_t otherwise) {
  return (i >= 0 && i < n) ? a[i] : otherwise;
}

// a log-probability that stands for a probability above 0: false for -inf and for NaN
__device__ __forceinline__ bool bl_has_prob(double l) { return l > -__builtin_huge_val(); }

// ---- sums ----
__device__ __forceinline__ double bl_wave_sum_f64(double v) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, BL_WAVE);
  return v;
}

// sum over a workgroup of WAVES waves, the same value in every thread.  s_red: WAVES entries.
template <int WAVES>
__device__ __forceinline__ double bl_block_sum_f64(double v, double* s_red) {
  v = bl_wave_sum_f64(v);
  __syncthreads();  // s_red may still be read from the previous reduction
  if (threadIdx.x % BL_WAVE == 0) s_red[threadIdx.x / BL_WAVE] = v;
  __syncthreads();
  double t = s_red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t += s_red[w];
  return t;
}

// sum of one value per thread of a workgroup of THREADS threads (a power of two); afterwards s_acc[0] holds it.  s_acc: THREADS entries.
template <int THREADS>
__device__ __forceinline__ void bl_tree_sum_f64(double acc, double* s_acc) {
  s_acc[threadIdx.x] = acc;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
    __syncthreads();
  }
}

// ---- first maxima ----
// Candidate (value, index) a replaces b: b is "none yet", a's value is greater, or it is the same value earlier.
template <class T>
__device__ __forceinline__ bool bl_better(T va, int ia, T vb, int ib) {
  return ib < 0 || va > vb || (va == vb && ia < ib);
}

template <class T>
__device__ __forceinline__ void bl_wave_argmax(T& v, int& i) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const T ov = __shfl_xor(v, o, BL_WAVE);
    const int oi = __shfl_xor(i, o, BL_WAVE);
    if (oi >= 0 && bl_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}

// the workgroup's first maximum from every thread's candidate; all threads return the same pair.  s_v / s_i: WAVES entries.
template <int WAVES>
__device__ __forceinline__ void bl_block_argmax(double& v, int& i, double* s_v, int* s_i) {
  const int lane = threadIdx.x % BL_WAVE, wave = threadIdx.x / BL_WAVE;
  bl_wave_argmax(v, i);
  __syncthreads();  // the previous use of s_v / s_i has been read
  if (lane == 0) {
    s_v[wave] = v;
    s_i[wave] = i;
  }
  __syncthreads();
  v = s_v[0];
  i = s_i[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w)
    if (s_i[w] >= 0 && bl_better(s_v[w], s_i[w], v, i)) {
      v = s_v[w];
      i = s_i[w];
    }
}
}  // namespace
