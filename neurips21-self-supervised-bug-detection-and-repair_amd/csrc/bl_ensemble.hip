// Ensemble combine: M members' per-sample predictions -> one ensemble prediction, in fp64, on the device.
//
// Replaces the combination half of reference buglab/models/ensemble/wrapper.py:33-89 (`EnsembleWrapper.predict` and
// `_avg_ensembling`), which loops over Python dicts with np.logaddexp one sample at a time.  The members' forward passes
// have already run on the same minibatch; their flat outputs [loc | text | var | swap] (fp32) are concatenated in `src`, and
// the host has turned each member's un-batching rule (buglab/models/basemodel.py::prediction_layout) into gather indices in one
// canonical layout per sample: locations = np.unique(reference_nodes) ascending then NO_BUG, rewrites by original index.
//
// One launch, one workgroup per sample (4 waves):
//   consensus only: wave w computes the first-maximum location of members w, w + 4, ... (bl_wave_argmax of bl_segment_f64.h,
//                   NaN as Python's `max` treats it), results in LDS;
//   every kind:     the threads stride over the sample's location and rewrite entries; each entry folds the present members
//                   in member order: r = a_0 + w, r = logaddexp(r, a_m + w), w = -log(M') -- numpy's logaddexp, in fp64.
// No atomics, a fixed member order: results are bit-identical from run to run.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int EN_THREADS = 256;
constexpr int EN_WAVES = EN_THREADS / BL_WAVE;

// numpy's npy_logaddexp: equal inputs (infinities of one sign included) -> x + ln 2; a NaN input -> NaN
__device__ __forceinline__ double en_logaddexp(double x, double y) {
  if (x == y) return x + 0.693147180559945309417232121458176568;
  const double t = x - y;
  if (t > 0) return x + log1p(exp(-t));
  if (t <= 0) return y + log1p(exp(t));
  return t;
}

// value of entry i of member m; an index outside src (the host never sends one) reads as NaN instead of out of bounds
__device__ __forceinline__ float en_load(const float* src, int64_t n_src, const int32_t* idx, int64_t total, int m, int64_t pos) {
  const int32_t j = idx[(int64_t)m * total + pos];
  return (j >= 0 && (int64_t)j < n_src) ? src[j] : __builtin_nanf("");
}

__global__ __launch_bounds__(EN_THREADS) void ensemble_combine_kernel(const float* __restrict__ src, int64_t n_src,
                                                                      const int32_t* __restrict__ loc_idx,
                                                                      const int32_t* __restrict__ loc_off, int64_t total_loc,
                                                                      const int32_t* __restrict__ rw_idx,
                                                                      const int32_t* __restrict__ rw_off, int64_t total_rw, int M,
                                                                      int kind, double* __restrict__ out_loc,
                                                                      double* __restrict__ out_rw) {
  __shared__ int s_active[BL_ENSEMBLE_MAX_MEMBERS];
  __shared__ int s_arg[BL_ENSEMBLE_MAX_MEMBERS];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  int64_t l0, r0;
  const int64_t nloc = bl_csr_row(loc_off, b, total_loc, l0), nrw = bl_csr_row(rw_off, b, total_rw, r0);

  // a member is absent from a sample when its gather indices there are -1 (the host writes all of them or none)
  if (tid < M) s_active[tid] = nloc > 0 && loc_idx[(int64_t)tid * total_loc + l0] >= 0;
  __syncthreads();

  if (kind == BL_ENSEMBLE_CONSENSUS) {
    // Python's max(d, key=d.get) over the canonical order: the first element starts as the best and a later one replaces it
    // only if strictly greater.  So a NaN first element wins; a later NaN never does; among the rest the first maximum wins.
    for (int m = wave; m < M; m += EN_WAVES) {
      if (!s_active[m]) continue;  // wave-uniform
      float bv = 0.0f;
      int bi = -1;
      for (int64_t i = lane; i < nloc; i += BL_WAVE) {
        const float v = en_load(src, n_src, loc_idx, total_loc, m, l0 + i);
        if (v == v && bl_better(v, (int)i, bv, bi)) {
          bv = v;
          bi = (int)i;
        }
      }
      bl_wave_argmax(bv, bi);
      if (lane == 0) {
        const float first = en_load(src, n_src, loc_idx, total_loc, m, l0);
        s_arg[m] = (first != first || bi < 0) ? 0 : bi;  // a NaN in front wins
      }
    }
    __syncthreads();
  }

  int count = 0, first_member = -1, agree = 1;
  for (int m = 0; m < M; ++m) {
    if (!s_active[m]) continue;
    if (first_member < 0) first_member = m;
    else if (kind == BL_ENSEMBLE_CONSENSUS && s_arg[m] != s_arg[first_member]) agree = 0;
    ++count;
  }
  const double nan = __builtin_nan("");
  if (count == 0) {  // no member predicts this sample (the host skips such samples): NaN, never a made-up value
    for (int64_t i = tid; i < nloc; i += EN_THREADS) out_loc[l0 + i] = nan;
    for (int64_t i = tid; i < nrw; i += EN_THREADS) out_rw[r0 + i] = nan;
    return;
  }
  if (!agree) {  // wrapper.py:77-79: every location -inf, NO_BUG 0, the first present member's rewrites unchanged
    for (int64_t i = tid; i < nloc; i += EN_THREADS) out_loc[l0 + i] = i == nloc - 1 ? 0.0 : -__builtin_huge_val();
    for (int64_t i = tid; i < nrw; i += EN_THREADS) out_rw[r0 + i] = (double)en_load(src, n_src, rw_idx, total_rw, first_member, r0 + i);
    return;
  }
  const double w = -log((double)count);  // wrapper.py:84 (-log(1) = -0.0: one member passes through unchanged)
  for (int64_t i = tid; i < nloc; i += EN_THREADS) {
    double r = (double)en_load(src, n_src, loc_idx, total_loc, first_member, l0 + i) + w;
    for (int m = first_member + 1; m < M; ++m)
      if (s_active[m]) r = en_logaddexp(r, (double)en_load(src, n_src, loc_idx, total_loc, m, l0 + i) + w);
    out_loc[l0 + i] = r;
  }
  for (int64_t i = tid; i < nrw; i += EN_THREADS) {
    double r = (double)en_load(src, n_src, rw_idx, total_rw, first_member, r0 + i) + w;
    for (int m = first_member + 1; m < M; ++m)
      if (s_active[m]) r = en_logaddexp(r, (double)en_load(src, n_src, rw_idx, total_rw, m, r0 + i) + w);
    out_rw[r0 + i] = r;
  }
}
}  // namespace

extern "C" int bl_ensemble_combine(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                                   const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, int32_t M, int32_t B, int32_t kind,
                                   double* out_loc, double* out_rw, void* stream) {
  BL_CHECK_ARG(M >= 1, "bl_ensemble_combine: M = %d members, need at least 1", (int)M);
  BL_CHECK_ARG(kind == BL_ENSEMBLE_AVG || kind == BL_ENSEMBLE_CONSENSUS, "bl_ensemble_combine: unknown kind %d", (int)kind);
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_loc >= 0 && total_rw >= 0,
               "bl_ensemble_combine: negative size (B %d, n_src %lld, total_loc %lld, total_rw %lld)", (int)B, (long long)n_src,
               (long long)total_loc, (long long)total_rw);
  BL_CHECK_RANGE(M <= BL_ENSEMBLE_MAX_MEMBERS, "bl_ensemble_combine: M = %d members, at most %d supported", (int)M,
                 BL_ENSEMBLE_MAX_MEMBERS);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32((int64_t)M * total_loc) && bl_fits_int32((int64_t)M * total_rw),
                 "bl_ensemble_combine: index space beyond int32 (n_src %lld, M x total_loc %lld, M x total_rw %lld)", (long long)n_src,
                 (long long)M * total_loc, (long long)M * total_rw);
  BL_CHECK_ARG(loc_off && rw_off, "bl_ensemble_combine: null offset pointer");
  BL_CHECK_ARG(B == 0 || (src && loc_idx && out_loc), "bl_ensemble_combine: null src / loc_idx / out_loc");
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && out_rw), "bl_ensemble_combine: null rw_idx / out_rw with %lld rewrite entries",
               (long long)total_rw);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(ensemble_combine_kernel, dim3(B), dim3(EN_THREADS), 0, (hipStream_t)stream, src, n_src, loc_idx, loc_off, total_loc,
                     rw_idx, rw_off, total_rw, (int)M, (int)kind, out_loc, out_rw);
  BL_LAUNCH_CHECK("bl_ensemble_combine");
  return BL_OK;
}
