// Warning grouping: the single-linkage clusters of a set of bug-site embeddings at a cosine threshold S (buglab/models/group.py;
// the NumPy twin is buglab/models/_group.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h ("Warning grouping"); in short, on
// bl_sim_quantize's outputs c, q, sumsq, r of the N rows, with l1_i = sum_d |q_id|, s2 = S S and K = 16 16129^2 s2 (1 - 2^-40):
//   filter   idot = sum_d q_id q_jd (int32, exact); A = 4 idot + 2 (l1_i + l1_j) + D (int64);
//            (i, j) is a CANDIDATE iff A > 0 and ((double)A (double)A) (r_i r_j) >= K
//   edge     dot = sum_d c_id c_jd in bl_lane_dot_f64.h's order, then bl_wave_sum_f64 -- bl_sim_rescore's dot;
//            (i, j) is an EDGE iff dot > 0.0 and dot dot >= s2 (sumsq_i sumsq_j)
//   groups   the connected components of the edges; label = the smallest row of the component, degree = edges at the row
// Integer products, fp64 sums in a fixed order, rounded products and compares: no sqrt, no division.  The filter loses no edge
// (DESIGN.md), so labels, degrees and both counters are functions of the input alone: equal to the twin bit for bit whatever the
// slices, the launch geometry and the order in which the pairs are visited.
//
// bl_group_row_l1  one wave per row
// bl_group_link    gr_link_kernel: workgroup (b, s) keeps the 16 rows of tile b in registers as B fragments and walks slice s of
//                  the 16-row tiles b .. T - 1 (the diagonal tile onwards) as A through v_mfma_i32_16x16x64_i8, a tile per
//                  wave and step.  A lane owns ONE row of tile b (its column) and sees 4 rows of the walked tile.  The filter
//                  runs on every accumulator register; where a ballot shows candidates, the whole wave takes them one at a
//                  time: the fp64 dot from c, the edge test, and on an edge lane 0 hooks the two trees.  N x N is never
//                  stored and there is no edge buffer.
// bl_group_labels  one thread per row: the root of its tree
//
// OPERAND and C/D MAPS of the MFMA: bl_similar.hip's.  A = the walked tile, B = tile b: col = l & 15 is row 16 b + col, and
// register `reg` of lane l is the pair with row 16 t + 4 (l >> 4) + reg.
//
// THE FOREST.  parent[x] <= x always: it starts as the identity, and the only writes are (1) a compare-and-swap of a ROOT's
// entry from itself to a smaller row, and (2) an atomic minimum with a row read from the entry of an ancestor, which is below
// the entry's current value or changes nothing.  So entries only decrease, and every entry stays an ancestor of its row: the
// components of the forest are always unions of components of the edges seen so far.
// TERMINATION.  No lock and no wait on another thread's write; every loop is bounded by a quantity that only decreases:
//   gr_find   follows parent from x: each step goes to a strictly smaller row (an entry that is not below its row ends the walk
//             as a root, which also keeps a caller's garbage in bounds), so at most x steps.
//   gr_hook   holds two rows a and b and ends when they are equal.  Each round replaces them by their roots (not above them);
//             with a != b it tries CAS(parent[hi], hi -> lo).  Success: hi's tree hangs below lo, done.  Failure: another
//             thread hooked hi in between and the CAS returns hi's new entry, which is below hi; the round continues from it.
//             So max(a, b) strictly decreases from round to round, at most max(i, j) rounds, and a failed CAS means somebody
//             else's succeeded.
//   the candidate loop clears one bit of a ballot per step; the tile loop and the k-chunks count up to fixed ends.
// A stale read can only show an OLDER entry of a row, which is an ancestor all the same (or the row itself, a former root): a
// hook below a former root keeps parent[x] <= x and joins the same two components, so stale reads cost steps, never an answer.
// After the kernel has completed every path strictly descends to the minimum of its component: bl_group_labels only reads.
#include "bl_common.h"
#include "bl_lane_dot_f64.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int GR_THREADS = 256;
constexpr int GR_WAVES = GR_THREADS / BL_WAVE;
constexpr int GR_TILE = 16;
constexpr int GR_MAX_CHUNKS = BL_SIM_MAX_D / 64;

typedef int gr_v4i __attribute__((ext_vector_type(4)));

// ---- bl_group_row_l1 ----
__global__ __launch_bounds__(GR_THREADS) void gr_row_l1_kernel(const int8_t* __restrict__ q, int64_t N, int Dp, int32_t* __restrict__ l1) {
  const int lane = threadIdx.x % BL_WAVE;
  const int64_t n = (int64_t)blockIdx.x * GR_WAVES + threadIdx.x / BL_WAVE;
  if (n >= N) return;  // the whole wave leaves
  const int32_t* row = reinterpret_cast<const int32_t*>(q + n * (int64_t)Dp);  // 4-byte aligned: the base is 16-byte aligned, Dp a multiple of 64
  int sum = 0;
  for (int w = lane; w < Dp / 4; w += BL_WAVE) {
    const int32_t word = row[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = (int)(int8_t)(word >> (8 * j));
      sum += v < 0 ? -v : v;
    }
  }
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, BL_WAVE);
  if (lane == 0) l1[n] = sum;  // at most 512 * 128
}

// ---- bl_group_link ----
__device__ __forceinline__ int gr_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree; on the way every visited entry is lowered to its grandparent (path halving: an atomic minimum)
__device__ __forceinline__ int gr_find(int32_t* parent, int x) {
  int p = gr_load(parent + x);
  while (p >= 0 && p < x) {  // x strictly decreases
    const int g = gr_load(parent + p);
    if (g >= 0 && g < p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void gr_hook(int32_t* parent, int a, int b) {
  while (true) {  // max(a, b) strictly decreases
    a = gr_find(parent, a);
    b = gr_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return;
    if (!(seen >= 0 && seen < hi)) return;  // an entry that is not below its row is the caller's garbage, not a tree: leave it
    a = seen;  // hi was hooked by another thread: go on from where it hangs now
    b = lo;
  }
}

__global__ __launch_bounds__(GR_THREADS) void gr_link_kernel(const int8_t* __restrict__ q, const double* __restrict__ r,
                                                             const int32_t* __restrict__ l1, const float* __restrict__ c, int64_t ldc,
                                                             const double* __restrict__ sumsq, int64_t N, int D, int Dp, int vec, double s2,
                                                             double K, int S, int32_t* parent, int32_t* degree,
                                                             unsigned long long* counters) {
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int col = lane & 15, group = lane >> 4;
  const int64_t tiles = (N + GR_TILE - 1) / GR_TILE;
  const int64_t b = blockIdx.x;
  const int64_t len = tiles - b;  // tiles b .. tiles - 1, cut into S slices
  const int64_t t_begin = b + len * (int64_t)blockIdx.y / S, t_end = b + len * ((int64_t)blockIdx.y + 1) / S;
  if (t_begin + wave >= t_end) return;  // the whole wave leaves (no barrier below)
  const int chunks = Dp / 64;

  // tile b's rows stay in registers for the whole walk (a row past N loads the last one; its pairs are dropped)
  const int64_t jb = b * GR_TILE + col;
  const int64_t brow = jb < N ? jb : N - 1;
  gr_v4i bfrag[GR_MAX_CHUNKS];
#pragma unroll
  for (int kc = 0; kc < GR_MAX_CHUNKS; ++kc)
    bfrag[kc] = kc < chunks ? *reinterpret_cast<const gr_v4i*>(q + brow * Dp + kc * 64 + group * 16) : gr_v4i{0, 0, 0, 0};
  const double rb = jb < N ? r[brow] : 0.0;  // r <= 0: an invalid row, in no pair
  const int64_t l1b = l1[brow];

  unsigned long long n_cand = 0, n_edge = 0;  // the same in every lane
  int deg_b = 0;                              // lane l < 16: edges at row 16 b + l found by this wave
  for (int64_t t = t_begin + wave; t < t_end; t += GR_WAVES) {
    const int64_t base = t * GR_TILE;
    const int64_t arow = base + col < N ? base + col : N - 1;
    const int8_t* ap = q + arow * Dp + group * 16;
    gr_v4i acc = {0, 0, 0, 0};
#pragma unroll
    for (int kc = 0; kc < GR_MAX_CHUNKS; ++kc)
      if (kc < chunks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const gr_v4i*>(ap + kc * 64), bfrag[kc], acc, 0, 0, 0);
    int deg_a = 0;  // lane l < 16: edges at row base + l found in this tile
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t ia = base + group * 4 + reg;
      bool cand = false;
      if (ia < N && jb < ia && rb > 0.0) {  // jb < ia: the upper triangle, which is every pair off the diagonal tile
        const double ra = r[ia];
        if (ra > 0.0) {
          const int64_t A = 4 * (int64_t)acc[reg] + 2 * (l1b + (int64_t)l1[ia]) + D;
          cand = A > 0 && ((double)A * (double)A) * (rb * ra) >= K;  // A^2 < 2^53: exact; then two rounded products
        }
      }
      unsigned long long mask = __ballot(cand);
      n_cand += __popcll(mask);
      while (mask) {  // one candidate per step, the whole wave on it
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int ra_in_tile = (l >> 4) * 4 + reg, cb = l & 15;
        const int64_t i = b * GR_TILE + cb, j = base + ra_in_tile;  // i < j < N
        const float* xi = c + i * ldc;
        const float* xj = c + j * ldc;
        const double dot = bl_wave_sum_f64(vec ? bl_lane_dot_f64<true>(xi, xj, D, lane) : bl_lane_dot_f64<false>(xi, xj, D, lane));
        if (dot > 0.0 && dot * dot >= s2 * (sumsq[i] * sumsq[j])) {  // three rounded products, one compare
          ++n_edge;
          deg_b += lane == cb;
          deg_a += lane == ra_in_tile;
          if (lane == 0) gr_hook(parent, (int)i, (int)j);
        }
      }
    }
    if (lane < GR_TILE && deg_a) atomicAdd(degree + base + lane, deg_a);  // base + lane < N: it was in an edge
  }
  if (lane < GR_TILE && deg_b) atomicAdd(degree + b * GR_TILE + lane, deg_b);
  if (lane == 0) {
    if (n_cand) atomicAdd(counters, n_cand);
    if (n_edge) atomicAdd(counters + 1, n_edge);
  }
}

// ---- bl_group_labels ----
__global__ __launch_bounds__(GR_THREADS) void gr_labels_kernel(const int32_t* __restrict__ parent, int64_t N, int32_t* __restrict__ label) {
  const int64_t n = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
  if (n >= N) return;
  int x = (int)n;
  int p = parent[x];
  while (p >= 0 && p < x) {  // x strictly decreases
    x = p;
    p = parent[x];
  }
  label[n] = x;
}
}  // namespace

extern "C" int bl_group_row_l1(const int8_t* q, int64_t N, int32_t Dp, int32_t* l1, void* stream) {
  BL_CHECK_ARG(N >= 0, "bl_group_row_l1: negative N (%lld)", (long long)N);
  BL_CHECK_ARG(Dp >= 64 && Dp % 64 == 0, "bl_group_row_l1: Dp = %d must be a positive multiple of 64", (int)Dp);
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, "bl_group_row_l1: Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_group_row_l1: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(N == 0 || (q && l1), "bl_group_row_l1: null q / l1");
  BL_CHECK_ARG(N == 0 || bl_aligned16(q), "bl_group_row_l1: the int8 image must be 16-byte aligned");
  if (N == 0) return BL_OK;
  hipLaunchKernelGGL(gr_row_l1_kernel, dim3((unsigned)((N + GR_WAVES - 1) / GR_WAVES)), dim3(GR_THREADS), 0, (hipStream_t)stream, q, N, (int)Dp,
                     l1);
  BL_LAUNCH_CHECK("bl_group_row_l1");
  return BL_OK;
}

extern "C" int bl_group_link(const int8_t* q, const double* r, const int32_t* l1, const float* c, int64_t ldc, const double* sumsq,
                             int64_t N, int32_t D, int32_t Dp, double s2, double K, int32_t slices, int32_t* parent, int32_t* degree,
                             int64_t* counters, void* stream) {
  BL_CHECK_ARG(N >= 0 && D >= 1, "bl_group_link: need N >= 0 and D >= 1 (got N %lld, D %d)", (long long)N, (int)D);
  BL_CHECK_RANGE(D <= BL_SIM_MAX_D, "bl_group_link: D = %d is above BL_SIM_MAX_D = %d", (int)D, BL_SIM_MAX_D);
  BL_CHECK_ARG(Dp == (D + 63) / 64 * 64, "bl_group_link: Dp = %d must be D = %d rounded up to a multiple of 64", (int)Dp, (int)D);
  BL_CHECK_RANGE(N <= BL_GROUP_MAX_N, "bl_group_link: N = %lld is above BL_GROUP_MAX_N = %d", (long long)N, BL_GROUP_MAX_N);
  BL_CHECK_ARG(ldc >= D, "bl_group_link: the row stride %lld is below D = %d", (long long)ldc, (int)D);
  BL_CHECK_ARG(s2 > 0.0 && s2 <= 1.0, "bl_group_link: s2 = %g must be in (0, 1]: the square of a similarity in (0, 1]", s2);
  BL_CHECK_ARG(K > 0.0 && K <= 16.0 * 16129.0 * 16129.0, "bl_group_link: K = %g must be in (0, 16 * 16129^2]", K);
  BL_CHECK_ARG(slices >= 1 && slices <= BL_GROUP_MAX_SLICES, "bl_group_link: slices = %d must be in [1, %d]", (int)slices, BL_GROUP_MAX_SLICES);
  BL_CHECK_ARG(counters != nullptr, "bl_group_link: null counters");
  BL_CHECK_ARG(((uintptr_t)counters & 7) == 0, "bl_group_link: the counters must be 8-byte aligned");
  BL_CHECK_ARG(N == 0 || (q && r && l1 && c && sumsq && parent && degree), "bl_group_link: null q / r / l1 / c / sumsq / parent / degree");
  BL_CHECK_ARG(N == 0 || bl_aligned16(q), "bl_group_link: the int8 image must be 16-byte aligned");
  if (N == 0) return BL_OK;
  const int vec = ((uintptr_t)c % 16 == 0) && (ldc % 4 == 0);
  const int64_t tiles = (N + GR_TILE - 1) / GR_TILE;
  hipLaunchKernelGGL(gr_link_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(GR_THREADS), 0, (hipStream_t)stream, q, r, l1, c, ldc, sumsq, N,
                     (int)D, (int)Dp, vec, s2, K, (int)slices, parent, degree, reinterpret_cast<unsigned long long*>(counters));
  BL_LAUNCH_CHECK("bl_group_link");
  return BL_OK;
}

extern "C" int bl_group_labels(const int32_t* parent, int64_t N, int32_t* label, void* stream) {
  BL_CHECK_ARG(N >= 0, "bl_group_labels: negative N (%lld)", (long long)N);
  BL_CHECK_RANGE(N <= BL_GROUP_MAX_N, "bl_group_labels: N = %lld is above BL_GROUP_MAX_N = %d", (long long)N, BL_GROUP_MAX_N);
  BL_CHECK_ARG(N == 0 || (parent && label), "bl_group_labels: null parent / label");
  if (N == 0) return BL_OK;
  hipLaunchKernelGGL(gr_labels_kernel, dim3((unsigned)((N + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream, parent, N,
                     label);
  BL_LAUNCH_CHECK("bl_group_labels");
  return BL_OK;
}
