// Ranked suggestions: a sample's k most probable fixes in order, and the rank the model gave the true fix and the true location.
//
// BEYOND THE REFERENCE: its evaluate.py and visualize.py reduce a sample to one answer (the first-maximum location, then the best
// rewrite there).  Here the sample's ENTRIES -- its candidate rewrites by original index, then NO_BUG -- are ranked by their
// joint log-probability, the g_i of bl_selector_sample: src[rw_idx[i]] + src[rw_loc_idx[i]] for a rewrite, src[nobug_idx[b]] for
// NO_BUG.  The model's flat output [loc | text | var | swap] (fp32, as it sits on the device after the forward) is read through
// int32 indices the host derived in the collate worker (buglab/models/_suggest.py::suggest_indices), and the results are written
// at the caller's offset into buffers that stay on the device for the whole run: one copy back at the end.
//
// Everything the kernel does is one fp64 addition per entry (of two fp32 values: the number Python forms from the same floats),
// compares, and integer counts.  No exp, no log: the probabilities are the host's business, so the NumPy twin
// (_suggest.py::rank_host) is equal bit for bit.
//
// bl_rank_suggestions  one workgroup (4 waves) per sample, threads stride over the sample's entries.
//   0  a segment of at most SG_STAGE entries has its fp64 values staged once in LDS (32 KB); a longer one is recomputed from src
//      wherever it is read, so no length is refused.
//   1  K rounds.  The winner of round r is the best entry that comes strictly AFTER the winner of round r - 1 in the total order
//      (greater value first, the lower index among equals): nothing is marked or mutated, each round is one bl_block_argmax.
//      An entry that is NaN or not above -inf takes no part.  The rounds end at the first one without a winner.
//   2  the joint rank of the truth entry and the location rank of the truth location: the number of rankable entries that
//      precede it, counted per thread and added over a fixed tree (integers: any order gives the same bits).
// Plain vector loads and stores only, no atomics; bit-identical from run to run.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / BL_WAVE;
constexpr int SG_STAGE = 4096;  // entries whose fp64 values are kept in LDS: 32 KB
constexpr int SG_NONE = 0x7fffffff;

// a precedes b in the total order (both rankable)
__device__ __forceinline__ bool sg_precedes(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia < ib); }

// sum / minimum of one int per thread over the workgroup, the same value in every thread.  s_red: SG_WAVES entries.  Barriers as
// bl_block_sum_f64: one before the scratch is written, one after.
template <bool MIN>
__device__ __forceinline__ int sg_block_reduce_i32(int v, int* s_red) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const int other = __shfl_xor(v, o, BL_WAVE);
    v = MIN ? (other < v ? other : v) : v + other;
  }
  __syncthreads();
  if (threadIdx.x % BL_WAVE == 0) s_red[threadIdx.x / BL_WAVE] = v;
  __syncthreads();
  int t = s_red[0];
#pragma unroll
  for (int w = 1; w < SG_WAVES; ++w) t = MIN ? (s_red[w] < t ? s_red[w] : t) : t + s_red[w];
  return t;
}

// the number of rankable entries i < n that precede entry t (rankable, value tv); value(i) is the caller's
template <class Value>
__device__ __forceinline__ int sg_rank_of(int t, double tv, int n, const Value& value, int* s_red) {
  int count = 0;
  for (int i = (int)threadIdx.x; i < n; i += SG_THREADS) {
    const double v = value(i);
    if (bl_has_prob(v) && sg_precedes(v, i, tv, t)) ++count;
  }
  return sg_block_reduce_i32<false>(count, s_red);
}

__global__ __launch_bounds__(SG_THREADS) void rank_suggestions_kernel(
    const float* __restrict__ src, int64_t n_src, const int32_t* __restrict__ rw_idx, const int32_t* __restrict__ rw_loc_idx,
    const int32_t* __restrict__ rw_off, int64_t total_rw, const int32_t* __restrict__ nobug_idx, const int32_t* __restrict__ tgt_rw,
    const int32_t* __restrict__ loc_idx, const int32_t* __restrict__ loc_off, const int32_t* __restrict__ key_node, int64_t total_loc,
    const int32_t* __restrict__ rw_node, int K, int skip_nobug, int32_t* __restrict__ out_entry, double* __restrict__ out_logprob,
    int32_t* __restrict__ out_rank, int64_t offset, int64_t capacity) {
  __shared__ double s_val[SG_STAGE];
  __shared__ double s_v[SG_WAVES];
  __shared__ int s_i[SG_WAVES];
  __shared__ int s_n[SG_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t at = offset + b;  // the host checked 0 <= offset and offset + B <= capacity
  int64_t r0, l0;
  const int n_rw = (int)bl_csr_row(rw_off, b, total_rw, r0);
  const int n_ent = n_rw + (skip_nobug ? 0 : 1);  // NO_BUG is entry n_rw
  const int32_t nobug = nobug_idx[b];
  const auto joint = [&](int i) -> double {
    if (i >= n_rw) return bl_load_f64(src, n_src, nobug);
    return bl_load_f64(src, n_src, rw_idx[r0 + i]) + bl_load_f64(src, n_src, rw_loc_idx[r0 + i]);  // -1 (no key): NaN
  };

  // ---- 0: stage the segment's values
  const bool staged = n_ent <= SG_STAGE;  // uniform over the workgroup
  if (staged) {
    for (int i = tid; i < n_ent; i += SG_THREADS) s_val[i] = joint(i);
    __syncthreads();
  }
  const auto value = [&](int i) -> double { return staged ? s_val[i] : joint(i); };

  // ---- 1: the first K entries in the total order
  double pv = 0.0;
  int pi = -1, found = 0;
  for (int r = 0; r < K; ++r) {
    double bv = 0.0;
    int bi = -1;
    for (int i = tid; i < n_ent; i += SG_THREADS) {
      const double v = value(i);
      if (!bl_has_prob(v)) continue;                      // NaN, -inf: not rankable
      if (pi >= 0 && !sg_precedes(pv, pi, v, i)) continue;  // not strictly after the previous winner
      if (bl_better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
    bl_block_argmax<SG_WAVES>(bv, bi, s_v, s_i);
    if (bi < 0) break;  // the same pair in every thread: nothing is left, in this round and in every later one
    if (tid == 0) {
      out_entry[at * K + r] = bi;
      out_logprob[at * K + r] = bv;
    }
    pv = bv;
    pi = bi;
    ++found;
  }
  for (int r = found + tid; r < K; r += SG_THREADS) {
    out_entry[at * K + r] = -1;
    out_logprob[at * K + r] = -__builtin_huge_val();
  }

  // ---- 2a: the joint rank of the truth entry
  const int32_t tgt = tgt_rw[b];
  const bool has_bug = tgt >= 0;
  const int truth = has_bug ? (tgt < n_rw ? tgt : -1) : (skip_nobug ? -1 : n_rw);
  int joint_rank = -1;
  if (truth >= 0) {
    const double tv = value(truth);
    if (bl_has_prob(tv)) joint_rank = sg_rank_of(truth, tv, n_ent, value, s_n);
  }

  // ---- 2b: the location rank: the same order over the location entries (NO_BUG last)
  const int n_all = (int)bl_csr_row(loc_off, b, total_loc, l0);
  const int n_loc = skip_nobug ? (n_all > 0 ? n_all - 1 : 0) : n_all;
  int truth_loc = -1;
  if (!has_bug) {
    truth_loc = (!skip_nobug && n_all > 0) ? n_all - 1 : -1;
  } else if (tgt < n_rw) {
    const int32_t tnode = rw_node[r0 + tgt];  // nodes are compared by identity, as in bl_eval_judge
    int first = SG_NONE;
    if (tnode >= 0)
      for (int i = tid; i < n_loc; i += SG_THREADS)
        if (key_node[l0 + i] == tnode) {
          first = i;
          break;
        }
    first = sg_block_reduce_i32<true>(first, s_n);
    truth_loc = first == SG_NONE ? -1 : first;
  }
  int loc_rank = -1;
  if (truth_loc >= 0) {
    const auto loc_value = [&](int i) -> double { return bl_load_f64(src, n_src, loc_idx[l0 + i]); };
    const double tv = loc_value(truth_loc);
    if (bl_has_prob(tv)) loc_rank = sg_rank_of(truth_loc, tv, n_loc, loc_value, s_n);
  }

  if (tid == 0) {
    out_rank[at] = joint_rank;
    out_rank[capacity + at] = loc_rank;
  }
}
}  // namespace

extern "C" int bl_rank_suggestions(const float* src, int64_t n_src, const int32_t* rw_idx, const int32_t* rw_loc_idx, const int32_t* rw_off,
                                   int64_t total_rw, const int32_t* nobug_idx, const int32_t* tgt_rw, const int32_t* loc_idx,
                                   const int32_t* loc_off, const int32_t* key_node, int64_t total_loc, const int32_t* rw_node, int32_t B,
                                   int32_t K, int32_t skip_nobug, int32_t* out_entry, double* out_logprob, int32_t* out_rank,
                                   int64_t offset, int64_t capacity, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0 && total_loc >= 0 && total_rw >= 0,
               "bl_rank_suggestions: negative size (B %d, n_src %lld, total_loc %lld, total_rw %lld)", (int)B, (long long)n_src,
               (long long)total_loc, (long long)total_rw);
  BL_CHECK_ARG(K >= 1, "bl_rank_suggestions: K = %d must be at least 1", (int)K);
  BL_CHECK_RANGE(K <= BL_SUGGEST_MAX_K, "bl_rank_suggestions: K = %d is above BL_SUGGEST_MAX_K = %d", (int)K, BL_SUGGEST_MAX_K);
  BL_CHECK_RANGE(bl_fits_int32(n_src) && bl_fits_int32(total_loc) && bl_fits_int32(total_rw + 1),
                 "bl_rank_suggestions: index space beyond int32 (n_src %lld, total_loc %lld, total_rw + 1 %lld)", (long long)n_src,
                 (long long)total_loc, (long long)total_rw + 1);
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)B <= capacity - offset,
               "bl_rank_suggestions: samples %lld .. %lld do not fit the result buffers of %lld samples", (long long)offset,
               (long long)offset + (long long)B, (long long)capacity);
  BL_CHECK_ARG(B == 0 || (src && rw_off && loc_off && nobug_idx && tgt_rw),
               "bl_rank_suggestions: null src / rw_off / loc_off / nobug_idx / tgt_rw");
  BL_CHECK_ARG(B == 0 || (out_entry && out_logprob && out_rank), "bl_rank_suggestions: null out_entry / out_logprob / out_rank");
  BL_CHECK_ARG(total_rw == 0 || (rw_idx && rw_loc_idx && rw_node),
               "bl_rank_suggestions: null rw_idx / rw_loc_idx / rw_node with %lld rewrites", (long long)total_rw);
  BL_CHECK_ARG(total_loc == 0 || (loc_idx && key_node), "bl_rank_suggestions: null loc_idx / key_node with %lld location entries",
               (long long)total_loc);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(rank_suggestions_kernel, dim3(B), dim3(SG_THREADS), 0, (hipStream_t)stream, src, n_src, rw_idx, rw_loc_idx, rw_off,
                     total_rw, nobug_idx, tgt_rw, loc_idx, loc_off, key_node, total_loc, rw_node, (int)K, (int)(skip_nobug != 0), out_entry,
                     out_logprob, out_rank, offset, capacity);
  BL_LAUNCH_CHECK("bl_rank_suggestions");
  return BL_OK;
}
