// Knowledge distillation: the soft-target term of a student's training loss (buglab/models/distill.py writes the teacher's
// distributions into the records; GnnBugLabModule.set_distillation switches the term on).  The reference has no counterpart:
// this goes beyond it.  The term sits beside the hard-label loss of gnn.py:221-251 / localizationmodule.py:63-124 and reads the
// same logits.  buglab/models/_distill.py states the arithmetic in NumPy, operation for operation (this file is compiled
// without fused multiply-adds so that the two differ only in exp / log and in the order of the sums).  Per segment, in fp64:
//
//   a_i = z_i / tau, ms = a's first maximum, Ss = sum_i exp(a_i - ms):   log q_i = (a_i - ms) - log Ss,  q_i = exp(a_i - ms) / Ss
//   u_i = t_i / tau over the entries with t_i > -inf, mt, St likewise:   log p_i = (u_i - mt) - log St,  p_i = exp(u_i - mt) / St
//   KL = sum over p_i > 0 of p_i (log p_i - log q_i);   delta_i = q_i - p_i  (p_i = 0 where t_i is -inf or NaN).
// a - ms <= 0 and u - mt <= 0, so nothing overflows for any tau.  A segment without a teacher entry above -inf is skipped:
// KL 0, delta 0, counted (an empty repair group -- a location without rewrites -- counts as nothing).
//
// A location segment of graph b: its candidate rows candidate_ptr[b] .. candidate_ptr[b + 1], then NO_BUG, whose student logit is
// the constant 1.0 (no delta) and whose teacher value is teacher_loc[C + b].  A repair segment: a group of the CSR the repair
// log-softmax runs over, its items scattered over the text | var | swap logits.
//
// distill_segment_kernel   one WAVE per segment, lanes stride over its entries (three passes: the maxima, the sums, KL and
//   delta), so a segment may be longer than a wave.  Lane 0 writes the segment's KL and its flags.
// distill_reduce_kernel    out[c], one workgroup each, sums its column over its range of segments in an order that depends on
//   nothing but the number of segments (thread t takes t, t + 256, ..., then bl_tree_sum_f64).
// distill_bwd_kernel       elementwise: g * delta / tau.
// Plain vector loads and stores only, no atomics; the reductions and the first-maximum rule are bl_segment_f64.h's.
#include "bl_common.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int DS_THREADS = 256;
constexpr int DS_WAVES = DS_THREADS / BL_WAVE;
constexpr int DS_OUT = 8;
constexpr double DS_DISTILLED = 1.0, DS_AGREE = 2.0, DS_SKIPPED = 4.0;  // a segment's flags, summed into one double

// One segment by one wave.  at(i, z, t, dst): entry i's student logit, teacher value and where its delta goes (-1: nowhere);
// returns false for an entry to leave out.  -> the segment's KL and flags (the same in every lane).
template <class At>
__device__ __forceinline__ void ds_segment(int n, At at, double tau, float* __restrict__ delta, int lane, double& kl, double& flags) {
  double ms = 0.0, mt = 0.0;
  int is = -1, it = -1;
  for (int i = lane; i < n; i += BL_WAVE) {
    double z, t;
    int64_t dst;
    if (!at(i, z, t, dst)) continue;
    const double a = z / tau;
    // (a NaN logit may enter as a lane's first entry: bl_segment_f64.h leaves NaNs to its callers, and here the segment's sums
    // and with them the loss are NaN whichever entry the maximum falls on; only the agreement counter could differ)
    if (bl_better(a, i, ms, is)) {
      ms = a;
      is = i;
    }
    if (bl_has_prob(t)) {
      const double u = t / tau;
      if (bl_better(u, i, mt, it)) {
        mt = u;
        it = i;
      }
    }
  }
  bl_wave_argmax(ms, is);
  bl_wave_argmax(mt, it);
  kl = 0.0;
  if (it < 0) {  // wave-uniform: no teacher entry with a probability (or no entry at all)
    for (int i = lane; i < n; i += BL_WAVE) {
      double z, t;
      int64_t dst;
      if (at(i, z, t, dst) && dst >= 0) delta[dst] = 0.0f;
    }
    flags = n > 0 ? DS_SKIPPED : 0.0;  // an empty group is neither distilled nor skipped
    return;
  }
  double ss = 0.0, st = 0.0;
  for (int i = lane; i < n; i += BL_WAVE) {
    double z, t;
    int64_t dst;
    if (!at(i, z, t, dst)) continue;
    ss += exp(z / tau - ms);
    if (bl_has_prob(t)) st += exp(t / tau - mt);
  }
  ss = bl_wave_sum_f64(ss);
  st = bl_wave_sum_f64(st);
  const double ls = log(ss), lt = log(st);
  double acc = 0.0;
  for (int i = lane; i < n; i += BL_WAVE) {
    double z, t;
    int64_t dst;
    if (!at(i, z, t, dst)) continue;
    const double da = z / tau - ms;
    const double q = exp(da) / ss;
    double p = 0.0;
    if (bl_has_prob(t)) {
      const double du = t / tau - mt;
      p = exp(du) / st;
      if (p > 0.0) acc += p * ((du - lt) - (da - ls));
    }
    if (dst >= 0) delta[dst] = (float)(q - p);
  }
  kl = bl_wave_sum_f64(acc);
  flags = DS_DISTILLED + (is == it ? DS_AGREE : 0.0);
}

__global__ __launch_bounds__(DS_THREADS) void distill_segment_kernel(
    const float* __restrict__ loc_scores, const float* __restrict__ repair_logits, const float* __restrict__ teacher_loc,
    const float* __restrict__ teacher_repair, const int32_t* __restrict__ candidate_ptr, const int32_t* __restrict__ group_ptr,
    const int32_t* __restrict__ group_items, int B, int G, int64_t C, int64_t R, double tau, double* __restrict__ ws,
    float* __restrict__ delta) {
  const int s = blockIdx.x * DS_WAVES + threadIdx.x / BL_WAVE, lane = threadIdx.x % BL_WAVE;
  const int S = B + G;
  if (s >= S) return;  // whole waves leave; nothing below synchronises the workgroup
  double kl, flags;
  if (s < B) {
    int64_t c0;
    const int nc = (int)bl_csr_row(candidate_ptr, s, C, c0);
    ds_segment(
        nc + 1,
        [&](int i, double& z, double& t, int64_t& dst) {
          if (i < nc) {
            z = (double)loc_scores[c0 + i];
            t = (double)teacher_loc[c0 + i];
            dst = c0 + i;
          } else {  // NO_BUG: a constant logit
            z = 1.0;
            t = (double)teacher_loc[C + s];
            dst = -1;
          }
          return true;
        },
        tau, delta, lane, kl, flags);
  } else {
    const int g = s - B;
    int64_t g0;
    const int ng = (int)bl_csr_row(group_ptr, g, R, g0);
    ds_segment(
        ng,
        [&](int i, double& z, double& t, int64_t& dst) {
          const int32_t item = group_items[g0 + i];
          if (item < 0 || (int64_t)item >= R) return false;  // the host never sends one
          z = (double)repair_logits[item];
          t = (double)teacher_repair[item];
          dst = C + item;
          return true;
        },
        tau, delta, lane, kl, flags);
  }
  if (lane == 0) {
    ws[s] = kl;
    ws[(int64_t)S + s] = flags;
  }
}

// out[0..5] = location KL | repair KL | distilled location segments | distilled repair groups | location segments where the
// student's first maximum is the teacher's | skipped segments; out[6..7] = 0.  One workgroup per entry.
__global__ __launch_bounds__(DS_THREADS) void distill_reduce_kernel(const double* __restrict__ ws, int B, int G, float* __restrict__ out) {
  __shared__ double s_acc[DS_THREADS];
  const int c = blockIdx.x, S = B + G;
  const int lo = (c == 1 || c == 3) ? B : 0, hi = (c == 0 || c == 2 || c == 4) ? B : S;
  double acc = 0.0;
  if (c < 6) {
    for (int i = lo + (int)threadIdx.x; i < hi; i += DS_THREADS) {
      if (c < 2) {
        acc += ws[i];
      } else {
        const int f = (int)ws[(int64_t)S + i];
        acc += (double)((c < 4 ? f : (c == 4 ? f >> 1 : f >> 2)) & 1);
      }
    }
  }
  bl_tree_sum_f64<DS_THREADS>(acc, s_acc);
  if (threadIdx.x == 0) out[c] = (float)s_acc[0];
}

__global__ __launch_bounds__(DS_THREADS) void distill_bwd_kernel(const float* __restrict__ delta, int64_t C, int64_t R,
                                                                 const float* __restrict__ g_loc, const float* __restrict__ g_rep, double tau,
                                                                 float* __restrict__ g_loc_scores, float* __restrict__ g_repair_logits) {
  const int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
  if (i >= C + R) return;
  if (i < C)
    g_loc_scores[i] = (float)((double)g_loc[0] * (double)delta[i] / tau);
  else
    g_repair_logits[i - C] = (float)((double)g_rep[0] * (double)delta[i] / tau);
}

bool ds_tau_ok(double tau) { return tau > 0.0 && tau < __builtin_huge_val(); }

int ds_check_sizes(const char* who, int64_t B, int64_t G, int64_t C, int64_t R) {
  BL_CHECK_ARG(B >= 0 && G >= 0 && C >= 0 && R >= 0, "%s: negative size (B %lld, G %lld, C %lld, R %lld)", who, (long long)B, (long long)G,
               (long long)C, (long long)R);
  BL_CHECK_RANGE(bl_fits_int32(C + R + DS_THREADS) && bl_fits_int32(B + G + DS_WAVES) && bl_fits_int32(C + B),
                 "%s: index space beyond int32 (B %lld, G %lld, C %lld, R %lld)", who, (long long)B, (long long)G, (long long)C, (long long)R);
  return BL_OK;
}
}  // namespace

extern "C" int64_t bl_distill_workspace_bytes(int32_t B, int32_t G) {
  if (B < 0 || G < 0) return -1;
  const int64_t S = (int64_t)B + (int64_t)G;
  return 2 * (S > 0 ? S : 1) * (int64_t)sizeof(double);
}

extern "C" int bl_distill_fwd(const float* loc_scores, const float* repair_logits, const float* teacher_loc, const float* teacher_repair,
                              const int32_t* candidate_ptr, const int32_t* repair_group_ptr, const int32_t* repair_group_items, int32_t B,
                              int32_t G, int64_t C, int64_t R, double tau, void* ws, float* delta, float* out, void* stream) {
  const int rc = ds_check_sizes("bl_distill_fwd", B, G, C, R);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(ds_tau_ok(tau), "bl_distill_fwd: the temperature must be finite and > 0 (tau %g)", tau);
  BL_CHECK_ARG(out && ws, "bl_distill_fwd: null out / ws");
  BL_CHECK_ARG(B > 0 || C == 0, "bl_distill_fwd: %lld candidate rows without a graph", (long long)C);
  BL_CHECK_ARG(G > 0 || R == 0, "bl_distill_fwd: %lld repair logits without a group", (long long)R);
  BL_CHECK_ARG(B == 0 || (candidate_ptr && teacher_loc), "bl_distill_fwd: null candidate_ptr / teacher_loc");
  BL_CHECK_ARG(C == 0 || (loc_scores && delta), "bl_distill_fwd: null loc_scores / delta with %lld candidate rows", (long long)C);
  BL_CHECK_ARG(G == 0 || repair_group_ptr, "bl_distill_fwd: null repair_group_ptr");
  BL_CHECK_ARG(R == 0 || (repair_logits && teacher_repair && repair_group_items && delta),
               "bl_distill_fwd: null repair_logits / teacher_repair / repair_group_items / delta with %lld logits", (long long)R);
  const int S = B + G;
  if (S > 0) {
    hipLaunchKernelGGL(distill_segment_kernel, dim3((S + DS_WAVES - 1) / DS_WAVES), dim3(DS_THREADS), 0, (hipStream_t)stream, loc_scores,
                       repair_logits, teacher_loc, teacher_repair, candidate_ptr, repair_group_ptr, repair_group_items, (int)B, (int)G, C, R, tau,
                       (double*)ws, delta);
    BL_LAUNCH_CHECK("bl_distill_fwd");
  }
  hipLaunchKernelGGL(distill_reduce_kernel, dim3(DS_OUT), dim3(DS_THREADS), 0, (hipStream_t)stream, (const double*)ws, (int)B, (int)G, out);
  BL_LAUNCH_CHECK("bl_distill_fwd");
  return BL_OK;
}

extern "C" int bl_distill_bwd(const float* delta, int64_t C, int64_t R, const float* g_loc, const float* g_rep, double tau,
                              float* g_loc_scores, float* g_repair_logits, void* stream) {
  const int rc = ds_check_sizes("bl_distill_bwd", 0, 0, C, R);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(ds_tau_ok(tau), "bl_distill_bwd: the temperature must be finite and > 0 (tau %g)", tau);
  BL_CHECK_ARG(C + R == 0 || (delta && g_loc && g_rep), "bl_distill_bwd: null delta / g_loc / g_rep");
  BL_CHECK_ARG(C == 0 || g_loc_scores, "bl_distill_bwd: null g_loc_scores with %lld candidate rows", (long long)C);
  BL_CHECK_ARG(R == 0 || g_repair_logits, "bl_distill_bwd: null g_repair_logits with %lld logits", (long long)R);
  if (C + R == 0) return BL_OK;
  hipLaunchKernelGGL(distill_bwd_kernel, dim3((unsigned)((C + R + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, (hipStream_t)stream,
                     delta, C, R, g_loc, g_rep, tau, g_loc_scores, g_repair_logits);
  BL_LAUNCH_CHECK("bl_distill_bwd");
  return BL_OK;
}
