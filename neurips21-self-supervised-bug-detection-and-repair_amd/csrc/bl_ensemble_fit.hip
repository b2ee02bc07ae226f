// Fitted ensembles: per-member weights and temperatures (buglab/models/ensemble/fit.py, kind `weighted`).  The reference has no
// counterpart: its ensembles (buglab/models/ensemble/wrapper.py:33-89) give every present member the weight 1 / M'.  The
// arithmetic is the one buglab/models/ensemble/_weights.py states in NumPy, operation for operation (this file is compiled
// without fused multiply-adds so that the two differ only in exp / log1p and in the order of the sums).  Per sample, P = the
// present members, l_m = member m's fp32 log-probabilities:
//
//   locations   z_m = beta_m l_m;  s_m = z_m - LSE z_m  (beta_m == 1: s_m = l_m, the member's values as they are);
//               a_m = theta_m - LSE_{k in P} theta_k;   out_i = LSE_{m in P} (a_m + s_m[i])
//   rewrites    b_m = phi_m - LSE_{k in P} phi_k;       out_r = LSE_{m in P} (b_m + l_m[r])
//
// Every LSE of the statistics subtracts the FIRST maximum and takes log1p of the sum without it; entries that are not above
// -inf are skipped: they enter no maximum and no sum and are never multiplied.
//
// bl_ens_loc_stats   F = -sum_s out_s[tgt_s] and its gradient.  One WAVE per segment.  The wave walks the present members; for
//   each, its lanes stride over the entries (two passes: maximum, the sums), so a segment may be longer than a wave or a
//   workgroup.  What is left per member (s_m[tgt], l_m[tgt], E_m[l]) stays in LANE m, and the mixture over the members is a
//   wave reduction over those lanes.  Each segment's 1 + 2M partials are written first; a second kernel sums every column over
//   the segments in an order that depends on nothing but their number.
// bl_ens_rw_stats    the same mixture over the buggy samples' truth entries, one wave per sample, member m in lane m.
// bl_ensemble_combine_weighted   one workgroup per sample: wave 0 turns theta and phi into a and b, wave w the LSE of members
//   w, w + 4, ... at their beta (all kept in LDS), then the threads stride over the entries and fold the present members in
//   member order with numpy's logaddexp, as bl_ensemble_combine does.
// Plain vector loads and stores only, no atomics; the reductions and the first-maximum rule are bl_segment_f64.h's.
#include "bl_common.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int EF_THREADS = 256;
constexpr int EF_WAVES = EF_THREADS / BL_WAVE;
constexpr int EF_MAX = BL_ENSEMBLE_MAX_MEMBERS;
static_assert(EF_MAX <= BL_WAVE, "one member per lane");

struct ef_params {  // one parameter per member, by value: validated on the host, read from scalar registers
  double v[EF_MAX];
};

// entry `lane` of p (0 beyond the members), through constant indices only
__device__ __forceinline__ double ef_lane_param(const ef_params& p, int lane) {
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < EF_MAX; ++k)
    if (lane == k) r = p.v[k];
  return r;
}

// numpy's npy_logaddexp (bl_ensemble.hip's fold)
__device__ __forceinline__ double ef_logaddexp(double x, double y) {
  if (x == y) return x + 0.693147180559945309417232121458176568;
  const double t = x - y;
  if (t > 0) return x + log1p(exp(-t));
  if (t <= 0) return y + log1p(exp(t));
  return t;
}

// Lane m holds member m's weight parameter w: a = w - LSE over the present members, pi = exp(a) as the softmax gives it.
// false: no member is present (a = pi = 0).  Every lane of the wave makes the call.
__device__ __forceinline__ bool ef_log_weights(double w, bool present, int lane, double& a, double& pi) {
  double tm = w;
  int km = present ? lane : -1;
  bl_wave_argmax(tm, km);
  a = pi = 0.0;
  if (km < 0) return false;  // wave-uniform
  const double e = (present && lane != km) ? exp(w - tm) : 0.0;
  const double tz = bl_wave_sum_f64(e);
  if (present) {
    a = (w - tm) - log1p(tz);
    pi = (lane == km ? 1.0 : e) / (1.0 + tz);
  }
  return true;
}

// The mixture, one member per lane: v = the member's log-probability of the target.  -> F = -LSE_{m in P} (a_m + v_m);
// r = the member's responsibility exp(a_m + v_m + F), g = dF/dw_m = -(r_m - pi_m).  No present member: 0, nothing to add.
// No present member gives the target a probability (the host sends no such sample): NaN.
__device__ __forceinline__ double ef_mix(double w, double v, bool present, int lane, double& r, double& g) {
  double a, pi;
  r = g = 0.0;
  if (!ef_log_weights(w, present, lane, a, pi)) return 0.0;
  const double c = a + v;
  const bool counted = present && bl_has_prob(c);
  double cm = c;
  int mm = counted ? lane : -1;
  bl_wave_argmax(cm, mm);
  if (mm < 0) {
    r = g = __builtin_nan("");
    return __builtin_nan("");
  }
  const double cz = bl_wave_sum_f64((counted && lane != mm) ? exp(c - cm) : 0.0);
  const double F = (-cm) - log1p(cz);
  if (counted) r = exp(c + F);
  if (present) g = -(r - pi);
  return F;
}

__global__ __launch_bounds__(EF_THREADS) void ens_loc_stats_kernel(const float* __restrict__ vals, int64_t total,
                                                                   const int32_t* __restrict__ present,
                                                                   const int32_t* __restrict__ seg_off, const int32_t* __restrict__ tgt,
                                                                   int M, int S, ef_params theta, ef_params beta,
                                                                   double* __restrict__ partials) {
  const int s = blockIdx.x * EF_WAVES + threadIdx.x / BL_WAVE, lane = threadIdx.x % BL_WAVE;
  if (s >= S) return;  // whole waves leave; nothing below synchronises the workgroup
  int64_t a0;
  const int n = (int)bl_csr_row(seg_off, s, total, a0);
  const int y = tgt[s];
  const bool here = lane < M && n > 0 && present[(int64_t)lane * S + s] != 0;
  const double my_theta = ef_lane_param(theta, lane), my_beta = ef_lane_param(beta, lane);
  double my_sy = 0.0, my_ly = 0.0, my_E = 0.0;
  bool broken = false;
  for (int m = 0; m < M; ++m) {
    if (!__shfl((int)here, m, BL_WAVE)) continue;  // wave-uniform
    const double b = __shfl(my_beta, m, BL_WAVE);
    const float* __restrict__ v = vals + (int64_t)m * total + a0;
    double mx = 0.0;
    int im = -1;
    for (int i = lane; i < n; i += BL_WAVE) {
      const double l = (double)v[i];
      if (!bl_has_prob(l)) continue;
      const double z = b * l;
      if (bl_better(z, i, mx, im)) {
        mx = z;
        im = i;
      }
    }
    bl_wave_argmax(mx, im);
    if (im < 0 || y < 0 || y >= n) {  // nothing with a probability, or a target outside the segment: the host sends neither
      broken = true;
      break;
    }
    double zp = 0.0, s1 = 0.0;
    for (int i = lane; i < n; i += BL_WAVE) {
      const double l = (double)v[i];
      if (!bl_has_prob(l)) continue;
      const double w = exp(b * l - mx);
      if (i != im) zp += w;
      s1 += w * l;
    }
    zp = bl_wave_sum_f64(zp);
    s1 = bl_wave_sum_f64(s1);
    if (lane == m) {
      my_ly = (double)v[y];
      my_E = s1 / (1.0 + zp);  // the mean of l under the member's distribution at its temperature
      my_sy = b == 1.0 ? my_ly : (b * my_ly - mx) - log1p(zp);
    }
  }
  const int64_t at = s;
  if (broken) {
    if (lane == 0) partials[at] = __builtin_nan("");
    if (lane < M) partials[(int64_t)(1 + lane) * S + at] = partials[(int64_t)(1 + M + lane) * S + at] = __builtin_nan("");
    return;
  }
  double r, g;
  const double F = ef_mix(my_theta, my_sy, here, lane, r, g);
  if (lane == 0) partials[at] = F;
  if (lane < M) {
    partials[(int64_t)(1 + lane) * S + at] = g;
    partials[(int64_t)(1 + M + lane) * S + at] = r > 0.0 ? -(r * (my_ly - my_E)) : (r == r ? 0.0 : r);
  }
}

__global__ __launch_bounds__(EF_THREADS) void ens_rw_stats_kernel(const float* __restrict__ vals, const int32_t* __restrict__ present, int M,
                                                                  int S, ef_params phi, double* __restrict__ partials) {
  const int s = blockIdx.x * EF_WAVES + threadIdx.x / BL_WAVE, lane = threadIdx.x % BL_WAVE;
  if (s >= S) return;
  const bool here = lane < M && present[(int64_t)lane * S + s] != 0;
  const double v = here ? (double)vals[(int64_t)lane * S + s] : 0.0;
  double r, g;
  const double F = ef_mix(ef_lane_param(phi, lane), v, here, lane, r, g);
  if (lane == 0) partials[s] = F;
  if (lane < M) partials[(int64_t)(1 + lane) * S + s] = g;
}

// out[c] = the sum of column c's S partials; one workgroup per column (bl_confidence.hip's order: thread t takes segments
// t, t + 256, ..., then bl_tree_sum_f64)
__global__ __launch_bounds__(EF_THREADS) void ens_reduce_kernel(const double* __restrict__ partials, int S, double* __restrict__ out) {
  __shared__ double s_acc[EF_THREADS];
  const double* p = partials + (int64_t)blockIdx.x * S;
  double acc = 0.0;
  for (int i = threadIdx.x; i < S; i += EF_THREADS) acc += p[i];
  bl_tree_sum_f64<EF_THREADS>(acc, s_acc);
  if (threadIdx.x == 0) out[blockIdx.x] = s_acc[0];
}

// value of entry pos of member m; an index outside src (the host never sends one) reads as NaN instead of out of bounds
__device__ __forceinline__ double ef_load(const float* src, int64_t n_src, const int32_t* idx, int64_t total, int m, int64_t pos) {
  return bl_load_f64(src, n_src, idx[(int64_t)m * total + pos]);
}

__global__ __launch_bounds__(EF_THREADS) void ens_combine_weighted_kernel(const float* __restrict__ src, int64_t n_src,
                                                                          const int32_t* __restrict__ loc_idx,
                                                                          const int32_t* __restrict__ loc_off, int64_t total_loc,
                                                                          const int32_t* __restrict__ rw_idx,
                                                                          const int32_t* __restrict__ rw_off, int64_t total_rw, int M,
                                                                          ef_params theta, ef_params beta, ef_params phi,
                                                                          double* __restrict__ out_loc, double* __restrict__ out_rw) {
  __shared__ int s_active[EF_MAX];
  __shared__ double s_beta[EF_MAX], s_a[EF_MAX], s_b[EF_MAX], s_mx[EF_MAX], s_lz[EF_MAX];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  int64_t l0, r0;
  const int64_t nloc = bl_csr_row(loc_off, b, total_loc, l0), nrw = bl_csr_row(rw_off, b, total_rw, r0);

  if (wave == 0) {
    // a member is absent from a sample when its gather indices there are -1 (the host writes all of them or none)
    const bool here = lane < M && nloc > 0 && loc_idx[(int64_t)lane * total_loc + l0] >= 0;
    double a, bb, pi;
    ef_log_weights(ef_lane_param(theta, lane), here, lane, a, pi);
    ef_log_weights(ef_lane_param(phi, lane), here, lane, bb, pi);
    if (lane < EF_MAX) {
      s_active[lane] = here;
      s_beta[lane] = ef_lane_param(beta, lane);
      s_a[lane] = a;
      s_b[lane] = bb;
      s_mx[lane] = s_lz[lane] = 0.0;
    }
  }
  __syncthreads();

  // the members' LSE at their beta, once per sample and member
  for (int m = wave; m < M; m += EF_WAVES) {
    const double bt = s_beta[m];
    if (!s_active[m] || bt == 1.0) continue;  // wave-uniform; beta == 1: the values as they are
    double mx = 0.0;
    int im = -1;
    for (int64_t i = lane; i < nloc; i += BL_WAVE) {
      const double l = ef_load(src, n_src, loc_idx, total_loc, m, l0 + i);
      if (!bl_has_prob(l)) continue;
      const double z = bt * l;
      if (bl_better(z, (int)i, mx, im)) {
        mx = z;
        im = (int)i;
      }
    }
    bl_wave_argmax(mx, im);
    if (im < 0) continue;  // nothing with a probability: the entries pass through (s_mx = s_lz = 0 is never applied to them)
    double zp = 0.0;
    for (int64_t i = lane; i < nloc; i += BL_WAVE) {
      if ((int)i == im) continue;
      const double l = ef_load(src, n_src, loc_idx, total_loc, m, l0 + i);
      if (bl_has_prob(l)) zp += exp(bt * l - mx);
    }
    zp = bl_wave_sum_f64(zp);
    if (lane == 0) {
      s_mx[m] = mx;
      s_lz[m] = log1p(zp);
    }
  }
  __syncthreads();

  int first_member = -1;
  for (int m = M - 1; m >= 0; --m)
    if (s_active[m]) first_member = m;
  if (first_member < 0) {  // no member predicts this sample (the host skips such samples): NaN, never a made-up value
    const double nan = __builtin_nan("");
    for (int64_t i = tid; i < nloc; i += EF_THREADS) out_loc[l0 + i] = nan;
    for (int64_t i = tid; i < nrw; i += EF_THREADS) out_rw[r0 + i] = nan;
    return;
  }
  auto scaled = [&](int m, int64_t i) {
    const double l = ef_load(src, n_src, loc_idx, total_loc, m, l0 + i);
    const double bt = s_beta[m];
    return (bt == 1.0 || !bl_has_prob(l)) ? l : (bt * l - s_mx[m]) - s_lz[m];
  };
  for (int64_t i = tid; i < nloc; i += EF_THREADS) {
    double r = s_a[first_member] + scaled(first_member, i);
    for (int m = first_member + 1; m < M; ++m)
      if (s_active[m]) r = ef_logaddexp(r, s_a[m] + scaled(m, i));
    out_loc[l0 + i] = r;
  }
  for (int64_t i = tid; i < nrw; i += EF_THREADS) {
    double r = s_b[first_member] + ef_load(src, n_src, rw_idx, total_rw, first_member, r0 + i);
    for (int m = first_member + 1; m < M; ++m)
      if (s_active[m]) r = ef_logaddexp(r, s_b[m] + ef_load(src, n_src, rw_idx, total_rw, m, r0 + i));
    out_rw[r0 + i] = r;
  }
}

// the parameters as the kernels take them; false: null, not finite or outside [lo, hi]
bool ef_take(const double* p, int M, double lo, double hi, ef_params& out) {
  if (!p) return false;
  for (int k = 0; k < EF_MAX; ++k) {
    out.v[k] = k < M ? p[k] : 0.0;
    if (k < M && !(p[k] >= lo && p[k] <= hi)) return false;  // false for NaN too
  }
  return true;
}
}  // namespace

#define EF_CHECK_MEMBERS(who, M)                                                                                                    \
  BL_CHECK_ARG((M) >= 1, "%s: M = %d members, need at least 1", who, (int)(M));                                                     \
  BL_CHECK_RANGE((M) <= BL_ENSEMBLE_MAX_MEMBERS, "%s: M = %d members, at most %d supported", who, (int)(M), BL_ENSEMBLE_MAX_MEMBERS)
#define EF_TAKE(who, name, p, M, lo, hi, out)                                                                                       \
  BL_CHECK_ARG(p, "%s: null %s", who, name);                                                                                        \
  BL_CHECK_ARG(ef_take(p, M, lo, hi, out), "%s: every %s must be finite and inside the box [%g, %g]", who, name, (double)(lo), (double)(hi))

extern "C" int bl_ens_loc_stats(const float* vals, int64_t total, const int32_t* present, const int32_t* seg_off, const int32_t* tgt,
                                int32_t M, int32_t S, const double* theta, const double* beta, double* partials, double* out,
                                void* stream) {
  const char* who = "bl_ens_loc_stats";
  EF_CHECK_MEMBERS(who, M);
  BL_CHECK_ARG(S >= 0 && total >= 0, "%s: negative size (S %d, total %lld)", who, (int)S, (long long)total);
  BL_CHECK_RANGE(bl_fits_int32((int64_t)M * total) && bl_fits_int32((int64_t)(1 + 2 * M) * S + EF_WAVES),
                 "%s: index space beyond int32 (M x total %lld, (1 + 2M) x S %lld)", who, (long long)M * total,
                 (long long)(1 + 2 * M) * S);
  ef_params th, be;
  EF_TAKE(who, "theta", theta, M, -BL_ENS_WEIGHT_BOX, BL_ENS_WEIGHT_BOX, th);
  EF_TAKE(who, "beta", beta, M, BL_ENS_BETA_MIN, BL_ENS_BETA_MAX, be);
  BL_CHECK_ARG(S == 0 || (present && seg_off && tgt && partials && out), "%s: null present / seg_off / tgt / partials / out", who);
  BL_CHECK_ARG(total == 0 || vals, "%s: null vals with %lld values per member", who, (long long)total);
  if (S == 0) return BL_OK;
  hipLaunchKernelGGL(ens_loc_stats_kernel, dim3((S + EF_WAVES - 1) / EF_WAVES), dim3(EF_THREADS), 0, (hipStream_t)stream, vals, total,
                     present, seg_off, tgt, (int)M, (int)S, th, be, partials);
  BL_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(ens_reduce_kernel, dim3(1 + 2 * M), dim3(EF_THREADS), 0, (hipStream_t)stream, partials, (int)S, out);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

extern "C" int bl_ens_rw_stats(const float* vals, const int32_t* present, int32_t M, int32_t S, const double* phi, double* partials,
                               double* out, void* stream) {
  const char* who = "bl_ens_rw_stats";
  EF_CHECK_MEMBERS(who, M);
  BL_CHECK_ARG(S >= 0, "%s: negative size (S %d)", who, (int)S);
  BL_CHECK_RANGE(bl_fits_int32((int64_t)(1 + M) * S + EF_WAVES), "%s: index space beyond int32 ((1 + M) x S %lld)", who,
                 (long long)(1 + M) * S);
  ef_params ph;
  EF_TAKE(who, "phi", phi, M, -BL_ENS_WEIGHT_BOX, BL_ENS_WEIGHT_BOX, ph);
  BL_CHECK_ARG(S == 0 || (vals && present && partials && out), "%s: null vals / present / partials / out", who);
  if (S == 0) return BL_OK;
  hipLaunchKernelGGL(ens_rw_stats_kernel, dim3((S + EF_WAVES - 1) / EF_WAVES), dim3(EF_THREADS), 0, (hipStream_t)stream, vals, present,
                     (int)M, (int)S, ph, partials);
  BL_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(ens_reduce_kernel, dim3(1 + M), dim3(EF_THREADS), 0, (hipStream_t)stream, partials, (int)S, out);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

extern "C" int bl_ensemble_combine_weighted(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off,
                                            int64_t total_loc, const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, int32_t M,
                                            int32_t B, const double* theta, const double* beta, const double* phi, double* out_loc,
                                            double* out_rw, void* stream) {
  const char* who = "bl_ensemble_combine_weighted";
  EF_CHECK_MEMBERS(who, M);
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_loc >= 0 && total_rw >= 0, "%s: negative size (B %d, n_src %lld, total_loc %lld, total_rw %lld)",
               who, (int)B, (long long)n_src, (long long)total_loc, (long long)total_rw);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32((int64_t)M * total_loc) && bl_fits_int32((int64_t)M * total_rw),
                 "%s: index space beyond int32 (n_src %lld, M x total_loc %lld, M x total_rw %lld)", who, (long long)n_src,
                 (long long)M * total_loc, (long long)M * total_rw);
  ef_params th, be, ph;
  EF_TAKE(who, "theta", theta, M, -BL_ENS_WEIGHT_BOX, BL_ENS_WEIGHT_BOX, th);
  EF_TAKE(who, "beta", beta, M, BL_ENS_BETA_MIN, BL_ENS_BETA_MAX, be);
  EF_TAKE(who, "phi", phi, M, -BL_ENS_WEIGHT_BOX, BL_ENS_WEIGHT_BOX, ph);
  BL_CHECK_ARG(loc_off && rw_off, "%s: null offset pointer", who);
  BL_CHECK_ARG(B == 0 || (src && loc_idx && out_loc), "%s: null src / loc_idx / out_loc", who);
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && out_rw), "%s: null rw_idx / out_rw with %lld rewrite entries", who, (long long)total_rw);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(ens_combine_weighted_kernel, dim3(B), dim3(EF_THREADS), 0, (hipStream_t)stream, src, n_src, loc_idx, loc_off, total_loc,
                     rw_idx, rw_off, total_rw, (int)M, th, be, ph, out_loc, out_rw);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}
