// Confidence calibration: post-hoc scaling of a trained detector's log-probabilities (buglab/models/calibrate.py).  The
// reference has no counterpart: this goes beyond it.  The arithmetic is the one buglab/models/_calibrate.py states in NumPy,
// operation for operation (this file is compiled without fused multiply-adds so that the two differ only in exp / log1p and
// in the order of the sums):
//
//   z_i = beta * l_i (+ bias on a location segment's last entry, NO_BUG);   m = z's first maximum, at entry i_m;
//   w_i = exp(z_i - m);   Z' = sum over i != i_m of w_i;   Z = 1 + Z';   log-softmax_i = (z_i - m) - log1p(Z').
// z - m <= 0, so nothing overflows for any (beta, bias); log1p of the sum WITHOUT the maximum keeps a near-certain segment's
// tiny loss relatively exact.  Entries that are not above -inf (probability 0) are skipped: they enter no maximum and no sum
// and are never multiplied; apply leaves them as they are.
//
// bl_conf_loc_stats / bl_conf_group_stats   one WAVE per segment, lanes stride over its entries (three passes: maximum, the
//   sums, the centred second moment), so a segment may be longer than a wave or a workgroup.  Each segment's six (three)
//   partials are written first; a second kernel sums every column over the segments in an order that depends on nothing but
//   the number of segments (thread t takes segments t, t + 256, ..., then bl_tree_sum_f64), whatever the geometry of the
//   first launch.
// bl_conf_apply   one wave per location segment and per repair group of a minibatch's flat output, in place: fp64 inside,
//   rounded once to fp32.  A wave reads everything it needs of its segment before the pass that writes, and no two segments
//   share an entry.
// Plain vector loads and stores only, no atomics; the reductions and the first-maximum rule are bl_segment_f64.h's.
#include "bl_common.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / BL_WAVE;
constexpr int CF_LOC_COLS = 6;    // F | dF/dbeta | dF/dbias | d2F/dbeta2 | d2F/dbeta dbias | d2F/dbias2
constexpr int CF_GROUP_COLS = 3;  // F | dF/dbeta | d2F/dbeta2

// One segment's terms, by one wave.  v: its n entries; y: the target's place; NOBUG: the last entry takes the bias.
// r = F, dF/dbeta, dF/dbias, d2F/dbeta2, d2F/dbeta dbias, d2F/dbias2 (the same in every lane).
template <bool NOBUG>
__device__ __forceinline__ void cf_segment_stats(const float* __restrict__ v, int n, int y, double beta, double bias, int lane,
                                                 double (&r)[CF_LOC_COLS]) {
#pragma unroll
  for (int c = 0; c < CF_LOC_COLS; ++c) r[c] = 0.0;
  if (n <= 0) return;  // an empty segment contributes nothing
  auto z_of = [&](int i, double l) {
    double z = beta * l;
    if (NOBUG && i == n - 1) z = z + bias;
    return z;
  };
  double m = 0.0;
  int im = -1;
  for (int i = lane; i < n; i += BL_WAVE) {
    const double l = (double)v[i];
    if (!bl_has_prob(l)) continue;
    const double z = z_of(i, l);
    if (bl_better(z, i, m, im)) {
      m = z;
      im = i;
    }
  }
  bl_wave_argmax(m, im);
  if (im < 0 || y < 0 || y >= n) {  // nothing with a probability, or a target outside the segment: the host sends neither
#pragma unroll
    for (int c = 0; c < CF_LOC_COLS; ++c) r[c] = __builtin_nan("");
    return;
  }
  double zp = 0.0, s1 = 0.0;
  for (int i = lane; i < n; i += BL_WAVE) {
    const double l = (double)v[i];
    if (!bl_has_prob(l)) continue;
    const double w = exp(z_of(i, l) - m);
    if (i != im) zp += w;
    s1 += w * l;
  }
  zp = bl_wave_sum_f64(zp);
  s1 = bl_wave_sum_f64(s1);
  const double Z = 1.0 + zp;
  const double E = s1 / Z;  // the mean of l under the calibrated distribution
  double var = 0.0;
  for (int i = lane; i < n; i += BL_WAVE) {
    const double l = (double)v[i];
    if (!bl_has_prob(l)) continue;
    const double w = exp(z_of(i, l) - m);
    const double d = l - E;
    var += w * (d * d);
  }
  var = bl_wave_sum_f64(var);
  const double ly = (double)v[y];
  r[0] = log1p(zp) + (m - z_of(y, ly));  // two terms >= 0
  r[1] = E - ly;
  r[3] = var / Z;
  if (NOBUG) {
    const double ll = (double)v[n - 1];
    const double p = bl_has_prob(ll) ? exp(z_of(n - 1, ll) - m) / Z : 0.0;
    r[2] = p - (y == n - 1 ? 1.0 : 0.0);
    r[4] = bl_has_prob(ll) ? p * (ll - E) : 0.0;
    r[5] = p * (1.0 - p);
  }
}

template <bool NOBUG>
__global__ __launch_bounds__(CF_THREADS) void conf_stats_kernel(const float* __restrict__ vals, int64_t n_vals,
                                                                const int32_t* __restrict__ seg_off, const int32_t* __restrict__ tgt,
                                                                int nseg, double beta, double bias, double* __restrict__ partials) {
  const int s = blockIdx.x * CF_WAVES + threadIdx.x / BL_WAVE, lane = threadIdx.x % BL_WAVE;
  if (s >= nseg) return;  // whole waves leave; nothing below synchronises the workgroup
  int64_t a;
  const int n = (int)bl_csr_row(seg_off, s, n_vals, a);
  double r[CF_LOC_COLS];
  cf_segment_stats<NOBUG>(vals + a, n, tgt[s], beta, bias, lane, r);
  if (lane == 0) {
    if (NOBUG) {
#pragma unroll
      for (int c = 0; c < CF_LOC_COLS; ++c) partials[(int64_t)c * nseg + s] = r[c];
    } else {
      partials[s] = r[0];
      partials[(int64_t)nseg + s] = r[1];
      partials[2 * (int64_t)nseg + s] = r[3];
    }
  }
}

// out[c] = the sum of column c's nseg partials; one workgroup per column
__global__ __launch_bounds__(CF_THREADS) void conf_reduce_kernel(const double* __restrict__ partials, int nseg, double* __restrict__ out) {
  __shared__ double s_acc[CF_THREADS];
  const double* p = partials + (int64_t)blockIdx.x * nseg;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nseg; i += CF_THREADS) acc += p[i];
  bl_tree_sum_f64<CF_THREADS>(acc, s_acc);
  if (threadIdx.x == 0) out[blockIdx.x] = s_acc[0];
}

// One segment rewritten in place by one wave.  at(i): the flat index of entry i, or -1 for an entry to leave out.
template <class At>
__device__ __forceinline__ void cf_segment_apply(float* __restrict__ flat, int n, At at, double beta, double bias, bool nobug, int lane) {
  auto z_of = [&](int i, double l) {
    double z = beta * l;
    if (nobug && i == n - 1) z = z + bias;
    return z;
  };
  double m = 0.0;
  int im = -1;
  for (int i = lane; i < n; i += BL_WAVE) {
    const int64_t j = at(i);
    if (j < 0) continue;
    const double l = (double)flat[j];
    if (!bl_has_prob(l)) continue;
    const double z = z_of(i, l);
    if (bl_better(z, i, m, im)) {
      m = z;
      im = i;
    }
  }
  bl_wave_argmax(m, im);
  if (im < 0) return;  // wave-uniform
  double zp = 0.0;
  for (int i = lane; i < n; i += BL_WAVE) {
    const int64_t j = at(i);
    if (j < 0 || i == im) continue;
    const double l = (double)flat[j];
    if (bl_has_prob(l)) zp += exp(z_of(i, l) - m);
  }
  zp = bl_wave_sum_f64(zp);  // every load above has returned before any lane goes on to store
  const double lz = log1p(zp);
  for (int i = lane; i < n; i += BL_WAVE) {
    const int64_t j = at(i);
    if (j < 0) continue;
    const double l = (double)flat[j];
    if (bl_has_prob(l)) flat[j] = (float)((z_of(i, l) - m) - lz);
  }
}

__global__ __launch_bounds__(CF_THREADS) void conf_apply_kernel(float* __restrict__ flat, const int32_t* __restrict__ candidate_ptr, int B,
                                                                int64_t C, const int32_t* __restrict__ group_ptr,
                                                                const int32_t* __restrict__ group_items, int G, int64_t n_items,
                                                                int64_t item_base, double beta, double bias, double repair_beta) {
  const int s = blockIdx.x * CF_WAVES + threadIdx.x / BL_WAVE, lane = threadIdx.x % BL_WAVE;
  if (s < B) {  // sample s: its candidates flat[candidate_ptr[s] : candidate_ptr[s + 1]], then NO_BUG at flat[C + s]
    int64_t c0;
    const int nc = (int)bl_csr_row(candidate_ptr, s, C, c0);
    cf_segment_apply(flat, nc + 1, [&](int i) { return i < nc ? c0 + i : C + s; }, beta, bias, true, lane);
  } else if (s - B < G) {
    const int g = s - B;
    int64_t g0;
    const int ng = (int)bl_csr_row(group_ptr, g, n_items, g0);
    cf_segment_apply(
        flat, ng,
        [&](int i) {
          const int32_t it = group_items[g0 + i];
          return (it >= 0 && (int64_t)it < n_items) ? item_base + it : (int64_t)-1;
        },
        repair_beta, 0.0, false, lane);
  }
}

bool cf_scale_ok(double beta) { return beta > 0.0 && beta < __builtin_huge_val(); }

int cf_stats(const char* who, bool nobug, const float* vals, int64_t n_vals, const int32_t* seg_off, const int32_t* tgt, int32_t nseg,
             double beta, double bias, double* partials, double* out, void* stream) {
  BL_CHECK_ARG(nseg >= 0 && n_vals >= 0, "%s: negative size (nseg %d, n_vals %lld)", who, (int)nseg, (long long)n_vals);
  BL_CHECK_RANGE(bl_fits_int32(n_vals), "%s: pool beyond int32 offsets (n_vals %lld)", who, (long long)n_vals);
  BL_CHECK_ARG(cf_scale_ok(beta) && bias - bias == 0.0, "%s: beta must be finite and > 0 and the bias finite (beta %g, bias %g)", who, beta,
               bias);
  BL_CHECK_ARG(out, "%s: null out", who);
  BL_CHECK_ARG(nseg == 0 || (seg_off && tgt && partials), "%s: null seg_off / tgt / partials", who);
  BL_CHECK_ARG(n_vals == 0 || vals, "%s: null vals with %lld values", who, (long long)n_vals);
  const int cols = nobug ? CF_LOC_COLS : CF_GROUP_COLS;
  if (nseg > 0) {
    const dim3 grid((nseg + CF_WAVES - 1) / CF_WAVES);
    if (nobug)
      hipLaunchKernelGGL(conf_stats_kernel<true>, grid, dim3(CF_THREADS), 0, (hipStream_t)stream, vals, n_vals, seg_off, tgt, (int)nseg, beta,
                         bias, partials);
    else
      hipLaunchKernelGGL(conf_stats_kernel<false>, grid, dim3(CF_THREADS), 0, (hipStream_t)stream, vals, n_vals, seg_off, tgt, (int)nseg, beta,
                         0.0, partials);
    BL_LAUNCH_CHECK(who);
  }
  hipLaunchKernelGGL(conf_reduce_kernel, dim3(cols), dim3(CF_THREADS), 0, (hipStream_t)stream, partials, (int)nseg, out);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}
}  // namespace

extern "C" int bl_conf_loc_stats(const float* vals, int64_t n_vals, const int32_t* seg_off, const int32_t* tgt, int32_t nseg, double beta,
                                 double bias, double* partials, double* out, void* stream) {
  return cf_stats("bl_conf_loc_stats", true, vals, n_vals, seg_off, tgt, nseg, beta, bias, partials, out, stream);
}

extern "C" int bl_conf_group_stats(const float* vals, int64_t n_vals, const int32_t* seg_off, const int32_t* tgt, int32_t nseg, double beta,
                                   double* partials, double* out, void* stream) {
  return cf_stats("bl_conf_group_stats", false, vals, n_vals, seg_off, tgt, nseg, beta, 0.0, partials, out, stream);
}

extern "C" int bl_conf_apply(float* flat, int64_t n_flat, const int32_t* candidate_ptr, int32_t B, int64_t C, const int32_t* group_ptr,
                             const int32_t* group_items, int32_t G, int64_t n_items, int64_t item_base, double beta, double bias,
                             double repair_beta, void* stream) {
  BL_CHECK_ARG(B >= 0 && G >= 0 && C >= 0 && n_flat >= 0 && n_items >= 0 && item_base >= 0,
               "bl_conf_apply: negative size (B %d, G %d, C %lld, n_flat %lld, n_items %lld, item_base %lld)", (int)B, (int)G, (long long)C,
               (long long)n_flat, (long long)n_items, (long long)item_base);
  BL_CHECK_RANGE(bl_fits_int32(n_flat) && bl_fits_int32((int64_t)B + (int64_t)G + CF_WAVES),
                 "bl_conf_apply: index space beyond int32 (n_flat %lld, B %d, G %d)", (long long)n_flat, (int)B, (int)G);
  BL_CHECK_ARG(cf_scale_ok(beta) && cf_scale_ok(repair_beta) && bias - bias == 0.0,
               "bl_conf_apply: beta and repair_beta must be finite and > 0 and the bias finite (beta %g, repair_beta %g, bias %g)", beta,
               repair_beta, bias);
  BL_CHECK_ARG(B == 0 || C + (int64_t)B <= n_flat, "bl_conf_apply: %lld candidates and %d NO_BUG entries do not fit %lld values", (long long)C,
               (int)B, (long long)n_flat);
  BL_CHECK_ARG(G == 0 || n_items <= n_flat - item_base, "bl_conf_apply: items %lld .. %lld do not fit %lld values", (long long)item_base,
               (long long)item_base + (long long)n_items, (long long)n_flat);
  BL_CHECK_ARG(B == 0 || (flat && candidate_ptr), "bl_conf_apply: null flat / candidate_ptr");
  BL_CHECK_ARG(G == 0 || (flat && group_ptr), "bl_conf_apply: null flat / group_ptr");
  BL_CHECK_ARG(G == 0 || n_items == 0 || group_items, "bl_conf_apply: null group_items with %lld items", (long long)n_items);
  if (B + G == 0) return BL_OK;
  hipLaunchKernelGGL(conf_apply_kernel, dim3((B + G + CF_WAVES - 1) / CF_WAVES), dim3(CF_THREADS), 0, (hipStream_t)stream, flat,
                     candidate_ptr, (int)B, C, group_ptr, group_items, (int)G, n_items, item_base, beta, bias, repair_beta);
  BL_LAUNCH_CHECK("bl_conf_apply");
  return BL_OK;
}
