// Evaluation: the device half of buglab/models/evaluate.py -- what one sample contributes to the evaluation report.
//
// Replaces the per-sample Python of reference buglab/models/evaluate.py:60-140 (the predicted location, the best rewrite at the
// predicted and at the true node, and the four verdicts the metrics and threshold curves are counted from), which the reference
// runs on a dict and two lists per sample after copying every log-probability to the host.  Here the model's flat output
// [loc | text | var | swap] (fp32, as it sits on the device after the forward) is read through int32 indices the host derived in
// the collate worker (buglab/models/_evaluate.py::eval_indices), and the verdicts are written at the caller's offset into
// buffers that stay on the device for the whole run: one copy back at the end.
//
// fp64 on purpose (as bl_report.hip): the reference's values are Python floats made from fp32 numbers.  Without assume_buggy
// the confidence is a selected fp32 value, exact; with it, it is that value minus an fp64 log-sum-exp.
//
// bl_eval_judge  one workgroup (4 waves) per sample, threads stride over the sample's entries, so neither the number of
// locations nor of rewrites is bounded by LDS.
//   1  predicted location: first maximum over the location entries in the order the host sends (the key order of the dict
//      `predict` yields), by the rule of Python's max(): a NaN in front wins, a NaN elsewhere never does.  With assume_buggy the
//      last entry (NO_BUG) is left out and the sum of exp(x - max) over the remaining entries is taken: per thread in stride
//      order, then bl_block_sum_f64.
//   2  best rewrite AT A NODE, for the predicted node and for the target's node in one pass over the rewrites: the host's loop
//      that starts from -inf and takes a candidate only if it is strictly greater -- the lowest original index among the maxima;
//      a NaN never wins; nothing but -inf (or no rewrite at that node) is "none".  Nodes are compared by identity (key_node /
//      rw_node: the node's dense id within the sample), never by flat index.
//   3  thread 0 writes confidence and warned | location_correct | repair_given_location | repaired.
// Plain vector loads and stores only, no atomics; bit-identical from run to run.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / BL_WAVE;

__global__ __launch_bounds__(EV_THREADS) void eval_judge_kernel(
    const float* __restrict__ src, int64_t n_src, const int32_t* __restrict__ loc_idx, const int32_t* __restrict__ loc_off,
    const int32_t* __restrict__ key_node, int64_t total_loc, const int32_t* __restrict__ rw_idx, const int32_t* __restrict__ rw_off,
    const int32_t* __restrict__ rw_node, int64_t total_rw, const int32_t* __restrict__ tgt_rw, int assume_buggy,
    double* __restrict__ out_conf, int32_t* __restrict__ out_verdict, int64_t offset, int64_t capacity) {
  __shared__ double s_v[EV_WAVES];
  __shared__ int s_i[EV_WAVES];
  __shared__ double s_sum[EV_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t l0, r0;
  const int n_all = (int)bl_csr_row(loc_off, b, total_loc, l0);
  const int n_loc = assume_buggy ? (n_all > 0 ? n_all - 1 : 0) : n_all;  // the entries the maximum is taken over
  const int n_rw = (int)bl_csr_row(rw_off, b, total_rw, r0);

  // ---- 1: the predicted location
  double bv = 0.0;
  int bi = -1;
  for (int i = tid; i < n_loc; i += EV_THREADS) {
    const double v = bl_load_f64(src, n_src, loc_idx[l0 + i]);
    if (v == v && bl_better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
  bl_block_argmax<EV_WAVES>(bv, bi, s_v, s_i);
  int pred = -1;  // a sample without an entry to choose from (the host raises before it sends one)
  double conf = __builtin_nan("");
  if (n_loc > 0) {
    const double first = bl_load_f64(src, n_src, loc_idx[l0]);
    pred = (first != first || bi < 0) ? 0 : bi;  // a NaN in front, or nothing but NaNs: Python's max() keeps the first
    conf = pred == bi ? bv : first;
  }
  if (assume_buggy && n_loc > 0) {  // uniform over the workgroup
    // log-sum-exp of the remaining entries: shift by their greatest non-NaN value (0 where that is infinite or absent, as
    // torch.logsumexp), every thread's terms in stride order, then the fixed tree
    const double shift = (bi >= 0 && bv - bv == 0.0) ? bv : 0.0;
    double sum = 0.0;
    for (int i = tid; i < n_loc; i += EV_THREADS) sum += exp(bl_load_f64(src, n_src, loc_idx[l0 + i]) - shift);
    conf = conf - (shift + log(bl_block_sum_f64<EV_WAVES>(sum, s_sum)));
  }

  // ---- 2: the best rewrite at the predicted node and at the target's node
  const int32_t tgt = tgt_rw[b];
  const bool has_bug = tgt >= 0 && tgt < n_rw;
  const int32_t pnode = pred >= 0 ? key_node[l0 + pred] : -1;  // -1: NO_BUG
  const int32_t tnode = has_bug ? rw_node[r0 + tgt] : -1;
  double pv = 0.0, tv = 0.0;
  int pi = -1, ti = -1;
  for (int i = tid; i < n_rw; i += EV_THREADS) {
    const int32_t node = rw_node[r0 + i];
    if (node < 0 || (node != pnode && node != tnode)) continue;
    const double v = bl_load_f64(src, n_src, rw_idx[r0 + i]);
    if (!bl_has_prob(v)) continue;  // NaN and -inf never beat the -inf the host's loop starts from
    if (node == pnode && bl_better(v, i, pv, pi)) {
      pv = v;
      pi = i;
    }
    if (node == tnode && bl_better(v, i, tv, ti)) {
      tv = v;
      ti = i;
    }
  }
  bl_block_argmax<EV_WAVES>(pv, pi, s_v, s_i);
  bl_block_argmax<EV_WAVES>(tv, ti, s_v, s_i);

  // ---- 3: the verdicts
  if (tid == 0) {
    const int64_t at = offset + b;  // the host checked 0 <= offset and offset + B <= capacity
    const bool loc_ok = pnode == tnode;
    out_conf[at] = conf;
    out_verdict[at] = pnode >= 0 ? 1 : 0;
    out_verdict[capacity + at] = loc_ok ? 1 : 0;
    out_verdict[2 * capacity + at] = has_bug ? (ti == tgt ? 1 : 0) : -1;
    out_verdict[3 * capacity + at] = (loc_ok && pi == (has_bug ? tgt : -1)) ? 1 : 0;
  }
}
}  // namespace

extern "C" int bl_eval_judge(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, const int32_t* key_node,
                             int64_t total_loc, const int32_t* rw_idx, const int32_t* rw_off, const int32_t* rw_node, int64_t total_rw,
                             const int32_t* tgt_rw, int32_t B, int32_t assume_buggy, double* out_conf, int32_t* out_verdict,
                             int64_t offset, int64_t capacity, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_loc >= 0 && total_rw >= 0,
               "bl_eval_judge: negative size (B %d, n_src %lld, total_loc %lld, total_rw %lld)", (int)B, (long long)n_src,
               (long long)total_loc, (long long)total_rw);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32(total_loc) && bl_fits_int32(total_rw),
                 "bl_eval_judge: index space beyond int32 (n_src %lld, total_loc %lld, total_rw %lld)", (long long)n_src,
                 (long long)total_loc, (long long)total_rw);
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)B <= capacity - offset,
               "bl_eval_judge: samples %lld .. %lld do not fit the outcome buffers of %lld samples", (long long)offset,
               (long long)offset + (long long)B, (long long)capacity);
  BL_CHECK_ARG(B == 0 || (src && loc_off && rw_off && tgt_rw), "bl_eval_judge: null src / loc_off / rw_off / tgt_rw");
  BL_CHECK_ARG(B == 0 || (out_conf && out_verdict), "bl_eval_judge: null out_conf / out_verdict");
  BL_CHECK_ARG(total_loc == 0 || (loc_idx && key_node), "bl_eval_judge: null loc_idx / key_node with %lld location entries",
               (long long)total_loc);
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && rw_node), "bl_eval_judge: null rw_idx / rw_node with %lld rewrites", (long long)total_rw);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(eval_judge_kernel, dim3(B), dim3(EV_THREADS), 0, (hipStream_t)stream, src, n_src, loc_idx, loc_off, key_node,
                     total_loc, rw_idx, rw_off, rw_node, total_rw, tgt_rw, (int)(assume_buggy != 0), out_conf, out_verdict, offset,
                     capacity);
  BL_LAUNCH_CHECK("bl_eval_judge");
  return BL_OK;
}
