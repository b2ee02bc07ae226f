// Self-supervision services: the device half of bug selection and of detector scoring, in fp64 from the fp32 flat output.
//
// Replaces the arithmetic of reference buglab/controllers/bugselectorserver.py:22-28, 120-150 (per-rewrite log-probability,
// temperature / epsilon distribution, `num_rewrites_per_sample` rewrites drawn without replacement) and of
// buglab/controllers/detectordatascoringworker.py:118-130 (the log-probability a detector gives to the true fix), which the
// reference does in Python on one request at a time after copying every prediction value to the host.  Here the model's flat
// output [loc | text | var | swap] (fp32, as it sits on the device after the forward) is read through int32 indices the host
// derived from buglab/models/basemodel.py::prediction_layout, and only the answers go back.
//
// fp64 on purpose (as bl_ensemble_combine): the reference's values are Python floats made from fp32 numbers.
//
// bl_score_targets   one thread per sample: out[b] = src[tgt_loc[b]] (+ src[tgt_rw[b]] when tgt_rw[b] >= 0).
// bl_selector_sample one workgroup (4 waves) per sample; the threads stride over the sample's n_b + 1 entries (its rewrites by
//                    original index, then NO_BUG), so n_b is not bounded by LDS:
//   pass 1  g_i, written to out_logprob; z = sum_i exp(g_i / T)          (bl_block_sum_f64)
//   pass 2  p_i = exp(g_i / T) / z, or 1 / (n_b + 1) when u_eps[b] < epsilon; entropy; number of entries with p_i > 0;
//           Gumbel key_i = log p_i - log(-log u_i), kept in LDS for the first SS_KEY_CACHE entries and recomputed beyond
//   draws   k_b = min(K, #{p_i > 0}) rounds of a block arg-max over the keys that come after the previous winner in the order
//           (key descending, index ascending): the k_b largest keys, ties to the lower index.
// No max subtraction in the softmax: exp(g / T) is computed as the reference computes it, so an overflow or a sum of zero gives
// the reference's inf / nan.  0 * log 0 is nan in the entropy, as in NumPy.  No atomics; the reductions are bl_segment_f64.h's:
// bit-identical from run to run.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / BL_WAVE;
constexpr int SS_KEY_CACHE = 2048;  // 16 KiB of LDS; longer samples recompute the keys of the entries beyond

__global__ __launch_bounds__(SS_THREADS) void score_targets_kernel(const float* __restrict__ src, int64_t n_src,
                                                                   const int32_t* __restrict__ tgt_loc,
                                                                   const int32_t* __restrict__ tgt_rw, int B,
                                                                   double* __restrict__ out) {
  const int b = blockIdx.x * SS_THREADS + threadIdx.x;
  if (b >= B) return;
  const double loc = bl_load_f64(src, n_src, tgt_loc[b]);
  const int32_t r = tgt_rw[b];
  out[b] = r >= 0 ? loc + bl_load_f64(src, n_src, r) : loc;
}

// (key, index) a comes before b: larger key, then lower index
__device__ __forceinline__ bool ss_before(double ka, int ia, double kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

__device__ __forceinline__ double ss_key(double p, double u) {
  const double k = log(p) - log(-log(u));
  return k == k ? k : -__builtin_huge_val();  // a uniform outside (0, 1) (the caller never sends one) sorts last
}

__global__ __launch_bounds__(SS_THREADS) void selector_sample_kernel(
    const float* __restrict__ src, int64_t n_src, const int32_t* __restrict__ rw_idx, const int32_t* __restrict__ rw_loc_idx,
    const int32_t* __restrict__ rw_off, int64_t total_rw, const int32_t* __restrict__ nobug_idx, const double* __restrict__ u_eps,
    const double* __restrict__ u, double temperature, double epsilon, int K, double* __restrict__ out_logprob,
    double* __restrict__ out_p, double* __restrict__ out_entropy, int32_t* __restrict__ out_selected) {
  __shared__ double s_key[SS_KEY_CACHE];
  __shared__ double s_red[SS_WAVES];
  __shared__ double s_bk[SS_WAVES];
  __shared__ int s_bi[SS_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t r0;
  const int n = (int)bl_csr_row(rw_off, b, total_rw, r0);  // candidate rewrites; entry n is NO_BUG
  const int64_t e0 = r0 + b;                                // the sample's n + 1 entries in out_logprob / out_p / u
  double* lp = out_logprob + e0;
  double* pp = out_p + e0;
  const double* uu = u + e0;

  double z = 0.0;
  for (int i = tid; i <= n; i += SS_THREADS) {
    const double g = i < n ? bl_load_f64(src, n_src, rw_idx[r0 + i]) + bl_load_f64(src, n_src, rw_loc_idx[r0 + i])
                           : bl_load_f64(src, n_src, nobug_idx[b]);
    lp[i] = g;
    z += exp(g / temperature);
  }
  z = bl_block_sum_f64<SS_WAVES>(z, s_red);

  const bool uniform = u_eps[b] < epsilon;
  const double p_uniform = 1.0 / (double)(n + 1);
  double ent = 0.0, cnt = 0.0;
  for (int i = tid; i <= n; i += SS_THREADS) {  // the thread reads back the log-probabilities it wrote itself
    const double p = uniform ? p_uniform : exp(lp[i] / temperature) / z;
    pp[i] = p;
    ent += p * log(p);
    cnt += p > 0.0 ? 1.0 : 0.0;
    if (i < SS_KEY_CACHE) s_key[i] = p > 0.0 ? ss_key(p, uu[i]) : __builtin_nan("");  // NaN: not eligible
  }
  ent = bl_block_sum_f64<SS_WAVES>(ent, s_red);
  const int eligible = (int)bl_block_sum_f64<SS_WAVES>(cnt, s_red);  // exact: at most 2^31 ones; also orders the s_key writes
  if (tid == 0) out_entropy[b] = -ent;
  const int kb = K < eligible ? K : eligible;

  double pk = __builtin_huge_val();  // previous winner; (+inf, -1) comes before every entry
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    if (r >= kb) {  // uniform over the workgroup
      if (tid == 0) out_selected[(int64_t)b * K + r] = -1;
      continue;
    }
    double bk = 0.0;
    int bi = -1;
    for (int i = tid; i <= n; i += SS_THREADS) {
      double k;
      if (i < SS_KEY_CACHE) {
        k = s_key[i];
        if (k != k) continue;
      } else {
        const double p = pp[i];
        if (!(p > 0.0)) continue;
        k = ss_key(p, uu[i]);
      }
      if (!ss_before(pk, pi, k, i)) continue;  // already drawn
      if (bl_better(k, i, bk, bi)) {
        bk = k;
        bi = i;
      }
    }
    bl_block_argmax<SS_WAVES>(bk, bi, s_bk, s_bi);
    if (tid == 0) out_selected[(int64_t)b * K + r] = bi;
    pk = bk;
    pi = bi;
  }
}
}  // namespace

extern "C" int bl_score_targets(const float* src, int64_t n_src, const int32_t* tgt_loc, const int32_t* tgt_rw, int32_t B, double* out,
                                void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0, "bl_score_targets: negative size (B %d, n_src %lld)", (int)B, (long long)n_src);
  BL_CHECK_RANGE(bl_fits_int32(n_src), "bl_score_targets: n_src %lld beyond int32 indices", (long long)n_src);
  BL_CHECK_ARG(B == 0 || (src && tgt_loc && tgt_rw && out), "bl_score_targets: null src / tgt_loc / tgt_rw / out");
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(score_targets_kernel, dim3((B + SS_THREADS - 1) / SS_THREADS), dim3(SS_THREADS), 0, (hipStream_t)stream, src, n_src,
                     tgt_loc, tgt_rw, (int)B, out);
  BL_LAUNCH_CHECK("bl_score_targets");
  return BL_OK;
}

extern "C" int bl_selector_sample(const float* src, int64_t n_src, const int32_t* rw_idx, const int32_t* rw_loc_idx, const int32_t* rw_off,
                                  int64_t total_rw, const int32_t* nobug_idx, int32_t B, const double* u_eps, const double* u,
                                  double temperature, double epsilon, int32_t K, double* out_logprob, double* out_p, double* out_entropy,
                                  int32_t* out_selected, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_rw >= 0, "bl_selector_sample: negative size (B %d, n_src %lld, total_rw %lld)", (int)B,
               (long long)n_src, (long long)total_rw);
  BL_CHECK_ARG(K >= 1, "bl_selector_sample: K = %d rewrites per sample, need at least 1", (int)K);
  BL_CHECK_RANGE(K <= BL_SELECTOR_MAX_K, "bl_selector_sample: K = %d rewrites per sample, at most %d supported", (int)K,
                 BL_SELECTOR_MAX_K);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32(total_rw + (int64_t)B),
                 "bl_selector_sample: index space beyond int32 (n_src %lld, total_rw + B %lld)", (long long)n_src,
                 (long long)(total_rw + B));
  BL_CHECK_ARG(temperature == temperature && temperature != 0.0, "bl_selector_sample: temperature %g (the reference divides by it)",
               temperature);
  BL_CHECK_ARG(epsilon == epsilon, "bl_selector_sample: epsilon is NaN");
  BL_CHECK_ARG(B == 0 || (src && rw_off && nobug_idx && u_eps && u), "bl_selector_sample: null src / rw_off / nobug_idx / u_eps / u");
  BL_CHECK_ARG(B == 0 || (out_logprob && out_p && out_entropy && out_selected),
               "bl_selector_sample: null out_logprob / out_p / out_entropy / out_selected");
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && rw_loc_idx), "bl_selector_sample: null rw_idx / rw_loc_idx with %lld rewrite entries",
               (long long)total_rw);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(selector_sample_kernel, dim3(B), dim3(SS_THREADS), 0, (hipStream_t)stream, src, n_src, rw_idx, rw_loc_idx, rw_off,
                     total_rw, nobug_idx, u_eps, u, temperature, epsilon, (int)K, out_logprob, out_p, out_entropy, out_selected);
  BL_LAUNCH_CHECK("bl_selector_sample");
  return BL_OK;
}
