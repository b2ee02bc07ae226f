// Explanations: node attributions of a predicted fix (buglab/models/explain.py).
//
// BEYOND THE REFERENCE, which has nothing that says why a location was flagged.  The backward pass (existing kernels) leaves the
// gradient G [N, D] of the explained log-probability with respect to the embedder's output x [N, D]; what follows it is here:
//
// bl_attr_node_scores  a_n = w * sum_d G[n, d] * x[n, d] in fp64, one wave per node, optionally added to what score[n] holds
//                      (the steps of an integrated-gradients path).
// bl_attr_topk         per graph: sum a and sum |a| over its nodes, and its k first nodes by |a| (or by a), one workgroup per graph.
//
// The file sits on bl_segment_f64.h's contract: clamped offsets, fixed trees, no atomics, bl_better as the one ordering, NaNs
// never in a search.  Compiled without fused multiply-adds: score[n] + w * dot is a rounded product and a rounded sum, as NumPy
// forms it.  The NumPy twin (buglab/models/_explain.py::node_scores_host, topk_host) is equal bit for bit.
//
// COLUMN OWNERSHIP of bl_attr_node_scores (bl_lane_dot_f64.h; restated in include/buglab_hip.h and by the twin): columns go in quads, quad q =
// columns 4q .. 4q + 3; lane l of the node's wave owns the quads q with q % 64 == l and adds the products of its columns to its
// own fp64 sum, which starts at +0.0, in ascending column order.  That holds for every D, row stride and alignment: where both
// rows are 16-byte aligned a whole quad is one 16-byte load per operand, elsewhere (and for the last, partial quad) the same
// columns are loaded one by one -- the loads differ, the order of the additions does not.  A product of two fp32 values is exact
// in fp64 (24 + 24 significand bits), so only the additions round.  The 64 lane sums then go through bl_wave_sum_f64.
#include "bl_common.h"
#include "bl_lane_dot_f64.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int AT_THREADS = 256;
constexpr int AT_WAVES = AT_THREADS / BL_WAVE;

__global__ __launch_bounds__(AT_THREADS) void attr_node_scores_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ g,
                                                                      int64_t ldg, int64_t N, int D, double w, int accumulate, int vec,
                                                                      double* __restrict__ score) {
  const int lane = threadIdx.x % BL_WAVE;
  const int64_t n = (int64_t)blockIdx.x * AT_WAVES + threadIdx.x / BL_WAVE;
  if (n >= N) return;  // the whole wave leaves: the shuffles below are among the lanes of one wave
  const float* xr = x + n * ldx;
  const float* gr = g + n * ldg;
  const double dot = bl_wave_sum_f64(vec ? bl_lane_dot_f64<true>(xr, gr, D, lane) : bl_lane_dot_f64<false>(xr, gr, D, lane));
  if (lane == 0) {
    const double t = w * dot;
    score[n] = accumulate ? score[n] + t : t;
  }
}

// b comes strictly after a in bl_better's order (a != b): a's key is greater, or the same at the lower index
__device__ __forceinline__ bool at_after(double ka, int ia, double kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

__global__ __launch_bounds__(AT_THREADS) void attr_topk_kernel(const double* __restrict__ score, const int32_t* __restrict__ node_off,
                                                               int64_t N, int K, int by_abs, int32_t* __restrict__ out_node,
                                                               double* __restrict__ out_score, double* __restrict__ out_sums,
                                                               int64_t offset, int64_t capacity) {
  __shared__ double s_red[AT_WAVES];
  __shared__ double s_v[AT_WAVES];
  __shared__ int s_i[AT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t at = offset + b;  // the host checked 0 <= offset and offset + B <= capacity
  int64_t lo;
  const int n = (int)bl_csr_row(node_off, b, N, lo);  // N fits int32: so does the row
  const double* a = score + lo;

  // ---- the two sums: stride order per thread, then the fixed tree
  double sa = 0.0, sb = 0.0;
  for (int i = tid; i < n; i += AT_THREADS) {
    const double v = a[i];
    sa += v;
    sb += __builtin_fabs(v);
  }
  sa = bl_block_sum_f64<AT_WAVES>(sa, s_red);
  sb = bl_block_sum_f64<AT_WAVES>(sb, s_red);
  if (tid == 0) {
    out_sums[at] = sa;
    out_sums[capacity + at] = sb;
  }

  // ---- K rounds: the best node strictly after the previous pick; nothing is marked
  double pk = 0.0;
  int pi = -1, found = 0;
  for (int r = 0; r < K; ++r) {
    double bk = 0.0;
    int bi = -1;
    for (int i = tid; i < n; i += AT_THREADS) {
      const double v = a[i];
      const double key = by_abs ? __builtin_fabs(v) : v;
      if (key != key) continue;                           // NaN: never in a search
      if (pi >= 0 && !at_after(pk, pi, key, i)) continue;  // not strictly after the previous pick
      if (bl_better(key, i, bk, bi)) {
        bk = key;
        bi = i;
      }
    }
    bl_block_argmax<AT_WAVES>(bk, bi, s_v, s_i);
    if (bi < 0) break;  // the same pair in every thread: nothing is left, in this round and in every later one
    if (tid == 0) {
      out_node[at * K + r] = bi;
      out_score[at * K + r] = a[bi];
    }
    pk = bk;
    pi = bi;
    ++found;
  }
  for (int r = found + tid; r < K; r += AT_THREADS) {
    out_node[at * K + r] = -1;
    out_score[at * K + r] = 0.0;
  }
}
}  // namespace

extern "C" int bl_attr_node_scores(const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t N, int32_t D, double w,
                                   int32_t accumulate, double* score, void* stream) {
  BL_CHECK_ARG(N >= 0 && D >= 1, "bl_attr_node_scores: need N >= 0 and D >= 1 (got N %lld, D %d)", (long long)N, (int)D);
  BL_CHECK_ARG(ldx >= D && ldg >= D, "bl_attr_node_scores: row strides %lld / %lld are below D = %d", (long long)ldx, (long long)ldg, (int)D);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_attr_node_scores: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(N == 0 || (x && g && score), "bl_attr_node_scores: null x / g / score");
  if (N == 0) return BL_OK;
  const auto aligned = [](const float* p, int64_t ld) { return ((uintptr_t)p % 16 == 0) && (ld % 4 == 0); };
  const int vec = aligned(x, ldx) && aligned(g, ldg);
  const int64_t blocks = (N + AT_WAVES - 1) / AT_WAVES;
  hipLaunchKernelGGL(attr_node_scores_kernel, dim3((unsigned)blocks), dim3(AT_THREADS), 0, (hipStream_t)stream, x, ldx, g, ldg, N, (int)D, w,
                     (int)(accumulate != 0), vec, score);
  BL_LAUNCH_CHECK("bl_attr_node_scores");
  return BL_OK;
}

extern "C" int bl_attr_topk(const double* score, const int32_t* node_off, int32_t B, int64_t N, int32_t k, int32_t by_abs,
                            int32_t* out_node, double* out_score, double* out_sums, int64_t offset, int64_t capacity, void* stream) {
  BL_CHECK_ARG(B >= 0 && N >= 0, "bl_attr_topk: negative size (B %d, N %lld)", (int)B, (long long)N);
  BL_CHECK_ARG(k >= 1, "bl_attr_topk: k = %d must be at least 1", (int)k);
  BL_CHECK_RANGE(k <= BL_EXPLAIN_MAX_K, "bl_attr_topk: k = %d is above BL_EXPLAIN_MAX_K = %d", (int)k, BL_EXPLAIN_MAX_K);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_attr_topk: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)B <= capacity - offset,
               "bl_attr_topk: graphs %lld .. %lld do not fit the result buffers of %lld graphs", (long long)offset,
               (long long)offset + (long long)B, (long long)capacity);
  BL_CHECK_ARG(B == 0 || (node_off && out_node && out_score && out_sums), "bl_attr_topk: null node_off / out_node / out_score / out_sums");
  BL_CHECK_ARG(B == 0 || N == 0 || score, "bl_attr_topk: null score with %lld nodes", (long long)N);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(attr_topk_kernel, dim3(B), dim3(AT_THREADS), 0, (hipStream_t)stream, score, node_off, N, (int)k, (int)(by_abs != 0),
                     out_node, out_score, out_sums, offset, capacity);
  BL_LAUNCH_CHECK("bl_attr_topk");
  return BL_OK;
}
