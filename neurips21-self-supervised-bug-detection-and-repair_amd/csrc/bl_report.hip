// Bug reports: the device half of buglab/models/visualize.py -- what decides WHETHER and WHERE a sample appears in the report.
//
// Replaces the per-sample Python of reference buglab/models/visualize.py:75-144 (predicted location, best rewrite per code
// range, the sample's confidence, the "mistake" flag) and :151-170 (--only-incorrect, the sort by confidence, top k), which the
// reference runs on dicts and lists after copying every log-probability to the host and after rendering every snippet.  Here the
// model's flat output [loc | text | var | swap] (fp32, as it sits on the device after the forward) is read through int32 indices
// the host derived in the collate worker (buglab/models/_report.py::report_indices), and only the verdicts go back.
//
// fp64 on purpose (as bl_selfsup.hip): the reference's values are Python floats made from fp32 numbers.  Every output is a
// selected fp32 value or ONE fp64 sum of two of them, so there is no rounding to argue about.
//
// bl_report_summarize  one workgroup (4 waves) per sample.
//   1  predicted location: first maximum over the sample's location entries in the order the host sends (the key order of the
//      dict `predict` yields), by the rule of Python's max(): the first entry stays unless a later one is GREATER -- so a NaN
//      in front wins, a NaN elsewhere never does.  Threads stride over the entries; bl_block_argmax.
//   2  the waves stride over the sample's range groups; the lanes of a wave stride over the group's rewrites, which the host
//      lists group by group (grp_rw, a stable sort of the rewrites by group: the CSR form of rw_grp), so neither the number of
//      rewrites nor of groups is bounded by LDS.  Per group: the first maximum (same rule), best_range_logprob = loc + max.
//      Each wave keeps the maximum of best_range_logprob over the SHOWN groups it met, and the wave that meets the target's
//      group works out that group's verdict.
//   3  wave results are combined in wave order; thread 0 writes the sample's outputs.
// bl_report_order      one thread per sample, keys in LDS tiles: rank = number of kept samples that come before it in the order
//   of Python's stable sorted(key=-key): greater key first, input order on ties (so -inf keys come last, in input order; NaN
//   keys, which Python cannot order, come after those, in input order).  rank < k (or k <= 0) -> out[rank] = index.  O(n^2)
//   comparisons, exact, no atomics.  Without by_confidence the rank is the number of kept samples in front: a compaction.
// Plain vector loads and stores only; bit-identical from run to run.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int RP_THREADS = 256;
constexpr int RP_WAVES = RP_THREADS / BL_WAVE;

__global__ __launch_bounds__(RP_THREADS) void report_summarize_kernel(
    const float* __restrict__ src, int64_t n_src, const int32_t* __restrict__ loc_idx, const int32_t* __restrict__ loc_off,
    int64_t total_loc, const int32_t* __restrict__ rw_idx, const int32_t* __restrict__ rw_off, int64_t total_rw,
    const int32_t* __restrict__ rw_eq_target, const int32_t* __restrict__ grp_rw, const int32_t* __restrict__ grp_rw_off,
    const int32_t* __restrict__ grp_loc, const int32_t* __restrict__ grp_shown, const int32_t* __restrict__ grp_off,
    int64_t total_grp, const int32_t* __restrict__ tgt_grp, const int32_t* __restrict__ ground_loc,
    const int32_t* __restrict__ nobug_idx, int32_t* __restrict__ out_best_rw, double* __restrict__ out_best_range,
    int32_t* __restrict__ out_sample_i, double* __restrict__ out_sample_d, int B) {
  __shared__ double s_v[RP_WAVES];
  __shared__ int s_i[RP_WAVES];
  __shared__ double s_max[RP_WAVES];
  __shared__ int s_tgt[RP_WAVES];  // -1: this wave did not meet the target's group; else 0 / 1 = that group's verdict
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  int64_t l0, g0;
  const int n_loc = (int)bl_csr_row(loc_off, b, total_loc, l0);
  const int64_t r0 = bl_clamp_off(rw_off[b], total_rw);
  const int64_t n_grp = bl_csr_row(grp_off, b, total_grp, g0);

  // ---- 1: the predicted location
  double bv = 0.0;
  int bi = -1;
  for (int i = tid; i < n_loc; i += RP_THREADS) {
    const double v = bl_load_f64(src, n_src, loc_idx[l0 + i]);
    if (v == v && bl_better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
  bl_block_argmax<RP_WAVES>(bv, bi, s_v, s_i);
  int pred = bi < 0 ? 0 : bi;  // nothing but NaNs: Python's max() keeps the first
  if (n_loc > 0) {
    const double first = bl_load_f64(src, n_src, loc_idx[l0]);
    if (first != first) pred = 0;
  }

  // ---- 2: the range groups
  const int tg = tgt_grp[b];
  double wmax = -__builtin_huge_val();
  int wtgt = -1;
  for (int64_t g = g0 + wave; g < g0 + n_grp; g += RP_WAVES) {  // uniform over the wave
    int64_t q0;
    const int64_t n_q = bl_csr_row(grp_rw_off, g, total_rw, q0);
    double gv = 0.0;
    int gi = -1;  // position in grp_rw: ascending = by original rewrite index within the group
    for (int64_t q = q0 + lane; q < q0 + n_q; q += BL_WAVE) {
      const double v = bl_load_f64(src, n_src, bl_at_i32(rw_idx, total_rw, grp_rw[q], -1));
      if (v == v && bl_better(v, (int)(q - q0), gv, gi)) {
        gv = v;
        gi = (int)(q - q0);
      }
    }
    bl_wave_argmax(gv, gi);
    if (n_q > 0) {
      const double first = bl_load_f64(src, n_src, bl_at_i32(rw_idx, total_rw, grp_rw[q0], -1));
      if (first != first || gi < 0) {
        gv = first == first ? gv : first;
        gi = 0;
      }
    }
    const int32_t rw = gi >= 0 ? grp_rw[q0 + gi] : -1;  // the rewrite's place among the minibatch's rewrites
    const int gl = grp_loc[g];                          // the group's node: a position among the sample's location entries
    const double locv = (gl >= 0 && gl < n_loc) ? bl_load_f64(src, n_src, loc_idx[l0 + gl]) : __builtin_nan("");
    const double best = gi >= 0 ? locv + gv : __builtin_nan("");
    const bool shown = grp_shown[g] != 0;
    if (lane == 0) {
      out_best_rw[g] = rw >= 0 ? (int32_t)(rw - r0) : -1;
      out_best_range[g] = best;
    }
    if (shown && best > wmax) wmax = best;
    if (shown && tg >= 0 && g - g0 == (int64_t)tg)
      wtgt = (gl != pred) ? 1 : (bl_at_i32(rw_eq_target, total_rw, rw, 0) == 0 ? 1 : 0);
  }
  if (lane == 0) {
    s_max[wave] = wmax;
    s_tgt[wave] = wtgt;
  }
  __syncthreads();

  // ---- 3: the sample's verdict
  if (tid == 0) {
    double pl = s_max[0];
    int wrong = ground_loc[b] != pred ? 1 : 0;
#pragma unroll
    for (int w = 0; w < RP_WAVES; ++w) {
      if (s_max[w] > pl) pl = s_max[w];
      if (s_tgt[w] >= 0) wrong = s_tgt[w];
    }
    out_sample_i[b] = pred;
    out_sample_i[B + b] = pred == n_loc - 1 ? 1 : 0;
    out_sample_i[2 * B + b] = wrong;
    out_sample_d[b] = pl;
    out_sample_d[B + b] = bl_load_f64(src, n_src, nobug_idx[b]);
  }
}

// sample j (key kj) comes before sample i (key ki) in the report
__device__ __forceinline__ bool rp_before(double kj, int64_t j, double ki, int64_t i, bool by_confidence) {
  if (!by_confidence) return j < i;
  const bool nj = kj != kj, ni = ki != ki;
  if (nj || ni) return (!nj && ni) || (nj && ni && j < i);
  return kj > ki || (kj == ki && j < i);
}

__global__ __launch_bounds__(RP_THREADS) void report_order_kernel(const double* __restrict__ keys, const int32_t* __restrict__ keep,
                                                                  int64_t n, int64_t k, int by_confidence, int32_t* __restrict__ out,
                                                                  int32_t* __restrict__ out_count) {
  __shared__ double s_key[RP_THREADS];
  __shared__ int s_keep[RP_THREADS];
  const int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
  const bool live = i < n;
  const double ki = live ? keys[i] : 0.0;
  const bool keep_i = live && keep[i] != 0;
  int64_t rank = 0, kept = 0;
  for (int64_t t0 = 0; t0 < n; t0 += RP_THREADS) {
    const int64_t j = t0 + threadIdx.x;
    __syncthreads();  // the previous tile has been read
    s_key[threadIdx.x] = j < n ? keys[j] : 0.0;
    s_keep[threadIdx.x] = j < n ? (keep[j] != 0 ? 1 : 0) : 0;
    __syncthreads();
    const int m = (int)(n - t0 < RP_THREADS ? n - t0 : RP_THREADS);
    for (int t = 0; t < m; ++t) {
      const int kj = s_keep[t];
      kept += kj;
      rank += (kj && rp_before(s_key[t], t0 + t, ki, i, by_confidence != 0)) ? 1 : 0;
    }
  }
  const int64_t shown = (k > 0 && k < kept) ? k : kept;
  if (i == 0) out_count[0] = (int32_t)shown;
  if (keep_i && rank < shown) out[rank] = (int32_t)i;  // rank < kept <= n: inside out
}
}  // namespace

extern "C" int bl_report_summarize(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                                   const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, const int32_t* rw_eq_target,
                                   const int32_t* grp_rw, const int32_t* grp_rw_off, const int32_t* grp_loc, const int32_t* grp_shown,
                                   const int32_t* grp_off, int64_t total_grp, const int32_t* tgt_grp, const int32_t* ground_loc,
                                   const int32_t* nobug_idx, int32_t B, int32_t* out_best_rw, double* out_best_range,
                                   int32_t* out_sample_i, double* out_sample_d, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_loc >= 0 && total_rw >= 0 && total_grp >= 0,
               "bl_report_summarize: negative size (B %d, n_src %lld, total_loc %lld, total_rw %lld, total_grp %lld)", (int)B,
               (long long)n_src, (long long)total_loc, (long long)total_rw, (long long)total_grp);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32(total_loc) && bl_fits_int32(total_rw) && bl_fits_int32(total_grp),
                 "bl_report_summarize: index space beyond int32 (n_src %lld, total_loc %lld, total_rw %lld, total_grp %lld)",
                 (long long)n_src, (long long)total_loc, (long long)total_rw, (long long)total_grp);
  BL_CHECK_ARG(B == 0 || (src && loc_off && rw_off && grp_off && tgt_grp && ground_loc && nobug_idx),
               "bl_report_summarize: null src / loc_off / rw_off / grp_off / tgt_grp / ground_loc / nobug_idx");
  BL_CHECK_ARG(B == 0 || (out_sample_i && out_sample_d), "bl_report_summarize: null out_sample_i / out_sample_d");
  BL_CHECK_ARG(total_loc == 0 || loc_idx, "bl_report_summarize: null loc_idx with %lld location entries", (long long)total_loc);
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && rw_eq_target && grp_rw), "bl_report_summarize: null rw_idx / rw_eq_target / grp_rw with %lld rewrites",
               (long long)total_rw);
  BL_CHECK_ARG(total_grp == 0 || (grp_rw_off && grp_loc && grp_shown && out_best_rw && out_best_range),
               "bl_report_summarize: null grp_rw_off / grp_loc / grp_shown / out_best_rw / out_best_range with %lld groups",
               (long long)total_grp);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(report_summarize_kernel, dim3(B), dim3(RP_THREADS), 0, (hipStream_t)stream, src, n_src, loc_idx, loc_off, total_loc,
                     rw_idx, rw_off, total_rw, rw_eq_target, grp_rw, grp_rw_off, grp_loc, grp_shown, grp_off, total_grp, tgt_grp,
                     ground_loc, nobug_idx, out_best_rw, out_best_range, out_sample_i, out_sample_d, (int)B);
  BL_LAUNCH_CHECK("bl_report_summarize");
  return BL_OK;
}

extern "C" int bl_report_order(const double* keys, const int32_t* keep, int64_t n, int64_t k, int32_t by_confidence, int32_t* out,
                               int32_t* out_count, void* stream) {
  BL_CHECK_ARG(n >= 0, "bl_report_order: negative size (n %lld)", (long long)n);
  BL_CHECK_RANGE(n <= (int64_t)BL_REPORT_MAX_SAMPLES, "bl_report_order: n = %lld samples, at most %lld supported", (long long)n,
                 (long long)BL_REPORT_MAX_SAMPLES);
  BL_CHECK_ARG(out_count, "bl_report_order: null out_count");
  BL_CHECK_ARG(n == 0 || (keys && keep && out), "bl_report_order: null keys / keep / out");
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(out_count, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) {
      bl_set_error("bl_report_order: clearing out_count failed: %s", hipGetErrorString(e));
      return (int)e;
    }
    return BL_OK;
  }
  hipLaunchKernelGGL(report_order_kernel, dim3((unsigned)((n + RP_THREADS - 1) / RP_THREADS)), dim3(RP_THREADS), 0, (hipStream_t)stream,
                     keys, keep, n, k, (int)by_confidence, out, out_count);
  BL_LAUNCH_CHECK("bl_report_order");
  return BL_OK;
}
