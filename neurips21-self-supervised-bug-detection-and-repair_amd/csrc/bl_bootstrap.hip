// Paired bootstrap of the evaluation counts: the device half of buglab/models/compare.py.
//
// BEYOND THE REFERENCE: it has no counterpart (its buglab/models/evaluate.py prints point estimates).  What is resampled are the
// counts of buglab/models/evaluate.py:139-173 -- every metric and per-scout table is a ratio of them.  A replicate draws n samples
// with replacement and counts them again; the M models being compared share one packed word per sample, so they are counted
// over the SAME draws (that is what makes the bootstrap paired).
//
// The draw contract (include/buglab_hip.h repeats it; buglab/models/_compare.py::draw_indices is the NumPy twin).  Replicate
// r >= 0, draw j in [0, n), all arithmetic uint64 and wrapping:
//   mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
//   base   = mix(seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15)
//   h      = mix(r * n + j + base) >> 32
//   index  = (h * n) >> 32
// splitmix64 as a counter generator: a draw depends on (seed, r, j, n) alone, not on the grid nor on how a run is cut into
// calls.  NOT bl_lowbias32: two cheaper forms built on it failed a chi-square test of the index counts.
//
// bl_bootstrap_counts  one workgroup (4 waves) per replicate, threads stride over j; a workgroup takes replicates blockIdx.x,
// blockIdx.x + gridDim.x, ... so R is not bounded by the grid.  The replicate's output row is built in LDS, in column order.
//   1  the word of draw j is gathered from global memory: n <= 10^5 samples are 400 KB, which stay in the XCD's L2.
//   2  the 4 M scalar counters are per-lane adds in registers, summed over the wave by shuffles after the last draw and added
//      to the LDS row once per wave.
//   3  the per-scout entries (scout_total, and loc_ok / rep_ok per model) are integer LDS adds into the row; a scout id >= K
//      enters none.
//   4  every output element is stored once, from the LDS row.
// Integer adds only: any order gives the same bits.  What was measured and not adopted (wave ballots for the scalar counters, one
// LDS table per wave) is in DESIGN.md.
//
// bl_bootstrap_curve_counts  the same draws, counted per candidate threshold: the device half of
// buglab/models/operatingpoint.py (twin: buglab/models/_operatingpoint.py::curve_counts_host).  Every sample carries, per model,
// the index of the first threshold it passes (bins [M, n], G = none), so a replicate is a histogram over the bins followed by a
// prefix sum -- no ranking.  One workgroup per (replicate, model): blockIdx.y is the model, blockIdx.x strides over the
// replicates.  The models stay paired because a draw depends on (seed, r, j, n) alone.
//   1  the word of draw j is gathered as above; the bin is gathered only when the word sets a counter's flag, and a bin outside
//      [0, G) makes no LDS access.
//   2  the five counters (the order of _curves_of_ranked in buglab/models/evaluate.py) are integer LDS adds into ONE table
//      [5][G] of the workgroup: 20 KB at G = 1024.
//   3  the table is prefix-summed over the bins in place: a serial scan of each thread's ceil(G / 256) bins, a shuffle scan of
//      the threads' totals, the waves' totals through LDS.
//   4  every output element is stored once, from the table; the model-0 workgroup counts num_buggy in registers and stores column 0.
#include "bl_common.h"

namespace {
constexpr int BS_THREADS = 256;
constexpr int BS_MAX_COLS = BL_BOOTSTRAP_MAX_SCOUTS + BL_BOOTSTRAP_MAX_MODELS * (4 + 2 * BL_BOOTSTRAP_MAX_SCOUTS);
constexpr int64_t BS_MAX_GRID = 1 << 20;

__host__ __device__ inline uint64_t bs_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <int M>
__global__ __launch_bounds__(BS_THREADS) void bootstrap_counts_kernel(const uint32_t* __restrict__ packed, uint32_t n, int K,
                                                                      uint64_t base, uint64_t r0, int64_t R,
                                                                      int32_t* __restrict__ out) {
  __shared__ int32_t s_row[BS_MAX_COLS];  // the replicate's output row: scout_total [K] | model m: 4 scalars, loc_ok [K], rep_ok [K]
  const int tid = threadIdx.x;
  const int per_model = 4 + 2 * K, C = K + M * per_model;
  for (int64_t rep = blockIdx.x; rep < R; rep += gridDim.x) {
    for (int c = tid; c < C; c += BS_THREADS) s_row[c] = 0;
    __syncthreads();
    int32_t cnt[4 * M];
#pragma unroll
    for (int i = 0; i < 4 * M; ++i) cnt[i] = 0;
    const uint64_t ctr = (r0 + (uint64_t)rep) * (uint64_t)n + base;
    for (uint32_t j = (uint32_t)tid; j < n; j += BS_THREADS) {  // n < 2^31: no wrap
      const uint32_t h = (uint32_t)(bs_mix(ctr + j) >> 32);
      const uint32_t w = packed[__umulhi(h, n)];  // (h * n) >> 32 < n
      const int scout = (int)(w & 0xFFu);
      const bool buggy = scout != 0;
      const bool tabled = scout < K;
      if (tabled) atomicAdd(&s_row[scout], 1);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const uint32_t f = (w >> (8 + 4 * m)) & 0xFu;
        const bool warned = (f & 1u) != 0, loc = (f & 2u) != 0, rep_ok = (f & 4u) != 0, repaired = (f & 8u) != 0;
        cnt[4 * m + 0] += repaired ? 1 : 0;
        cnt[4 * m + 1] += (repaired && buggy) ? 1 : 0;
        cnt[4 * m + 2] += (warned && buggy) ? 1 : 0;
        cnt[4 * m + 3] += (!warned && !buggy) ? 1 : 0;
        int32_t* mine = s_row + K + per_model * m + 4;
        if (tabled && loc) atomicAdd(&mine[scout], 1);
        if (tabled && rep_ok && buggy) atomicAdd(&mine[K + scout], 1);
      }
    }
    // all lanes are back together here: the wave's sums, then one LDS add per wave and counter
#pragma unroll
    for (int i = 0; i < 4 * M; ++i) {
      int32_t v = cnt[i];
#pragma unroll
      for (int o = BL_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, BL_WAVE);
      if (tid % BL_WAVE == 0) atomicAdd(&s_row[K + per_model * (i / 4) + (i % 4)], v);
    }
    __syncthreads();
    int32_t* row = out + rep * (int64_t)C;
    for (int c = tid; c < C; c += BS_THREADS) row[c] = s_row[c];
    __syncthreads();  // the row is zeroed again at the top
  }
}

template <int M>
void bs_launch(const uint32_t* packed, uint32_t n, int K, uint64_t base, uint64_t r0, int64_t R, int32_t* out, hipStream_t stream) {
  const int64_t grid = R < BS_MAX_GRID ? R : BS_MAX_GRID;
  hipLaunchKernelGGL(bootstrap_counts_kernel<M>, dim3((unsigned)grid), dim3(BS_THREADS), 0, stream, packed, n, K, base, r0, R, out);
}

constexpr int BC_COUNTERS = 5;  // det_true | det_false | full_true | full_false | false_alarm
constexpr int BC_WAVES = BS_THREADS / BL_WAVE;

__global__ __launch_bounds__(BS_THREADS) void bootstrap_curve_counts_kernel(const uint32_t* __restrict__ packed,
                                                                            const int16_t* __restrict__ bins, uint32_t n, int M, int G,
                                                                            uint64_t base, uint64_t r0, int64_t R,
                                                                            int32_t* __restrict__ out) {
  __shared__ int32_t s_tab[BC_COUNTERS * BL_CURVE_MAX_BINS];  // [5][G]: counts per bin, then cumulative over the bins
  __shared__ int32_t s_wave[BC_COUNTERS][BC_WAVES];
  __shared__ int32_t s_buggy;
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int m = (int)blockIdx.y, T = BC_COUNTERS * G;
  const int shift = 8 + 4 * m;
  const int16_t* __restrict__ my_bins = bins + (size_t)m * n;
  const int64_t C = 1 + (int64_t)M * T;
  const int per = (G + BS_THREADS - 1) / BS_THREADS;  // bins a thread scans serially
  const int lo = min(tid * per, G), hi = min(lo + per, G);
  for (int64_t rep = blockIdx.x; rep < R; rep += gridDim.x) {
    for (int c = tid; c < T; c += BS_THREADS) s_tab[c] = 0;
    if (tid == 0) s_buggy = 0;
    __syncthreads();
    int32_t buggy_count = 0;
    const uint64_t ctr = (r0 + (uint64_t)rep) * (uint64_t)n + base;
    for (uint32_t j = (uint32_t)tid; j < n; j += BS_THREADS) {  // n < 2^31: no wrap
      const uint32_t h = (uint32_t)(bs_mix(ctr + j) >> 32);
      const uint32_t at = __umulhi(h, n);  // (h * n) >> 32 < n
      const uint32_t w = packed[at];
      const bool has_bug = (w & 0xFFu) != 0;
      buggy_count += has_bug ? 1 : 0;
      const uint32_t f = w >> shift;
      const bool warned = (f & 1u) != 0, loc = (f & 2u) != 0, rep_ok = (f & 4u) != 0;
      const bool det_true = has_bug && loc;
      if (!(det_true || warned)) continue;  // every counter needs one of the two
      const uint32_t b = (uint32_t)(int32_t)my_bins[at];  // a negative bin becomes a large one
      if (b >= (uint32_t)G) continue;  // passes no threshold
      if (det_true) atomicAdd(&s_tab[0 * G + b], 1);
      if (warned && !loc) atomicAdd(&s_tab[1 * G + b], 1);
      if (det_true && rep_ok) atomicAdd(&s_tab[2 * G + b], 1);
      if (warned && (!loc || !rep_ok)) atomicAdd(&s_tab[3 * G + b], 1);
      if (warned && !has_bug) atomicAdd(&s_tab[4 * G + b], 1);
    }
    if (m == 0) {  // uniform over the workgroup; all lanes are back together here
#pragma unroll
      for (int o = BL_WAVE / 2; o > 0; o >>= 1) buggy_count += __shfl_xor(buggy_count, o, BL_WAVE);
      if (lane == 0) atomicAdd(&s_buggy, buggy_count);
    }
    __syncthreads();
    // inclusive prefix sum over the bins of each counter, in place
    int32_t total[BC_COUNTERS], before[BC_COUNTERS];
#pragma unroll
    for (int c = 0; c < BC_COUNTERS; ++c) {
      int32_t run = 0;
      for (int g = lo; g < hi; ++g) {
        run += s_tab[c * G + g];
        s_tab[c * G + g] = run;
      }
      total[c] = run;
      int32_t v = run;
#pragma unroll
      for (int o = 1; o < BL_WAVE; o <<= 1) {
        const int32_t up = __shfl_up(v, o, BL_WAVE);
        if (lane >= o) v += up;
      }
      if (lane == BL_WAVE - 1) s_wave[c][wave] = v;
      before[c] = v - total[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < BC_COUNTERS; ++c) {
      int32_t add = before[c];
      for (int w2 = 0; w2 < wave; ++w2) add += s_wave[c][w2];
      for (int g = lo; g < hi; ++g) s_tab[c * G + g] += add;
    }
    __syncthreads();
    int32_t* row = out + rep * C;
    if (m == 0 && tid == 0) row[0] = s_buggy;
    int32_t* mine = row + 1 + (int64_t)m * T;
    for (int c = tid; c < T; c += BS_THREADS) mine[c] = s_tab[c];
    __syncthreads();  // the table is zeroed again at the top
  }
}
}  // namespace

extern "C" int bl_bootstrap_counts(const uint32_t* packed, int64_t n, int32_t M, int32_t K, uint64_t seed, int64_t r0, int64_t R,
                                   int32_t* out, void* stream) {
  BL_CHECK_ARG(packed && out, "bl_bootstrap_counts: null packed / out");
  BL_CHECK_ARG(n >= 1, "bl_bootstrap_counts: n must be at least 1 (got %lld)", (long long)n);
  BL_CHECK_ARG(R >= 0 && r0 >= 0, "bl_bootstrap_counts: negative replicate range (r0 %lld, R %lld)", (long long)r0, (long long)R);
  BL_CHECK_ARG(r0 <= INT64_MAX - R, "bl_bootstrap_counts: replicates %lld + %lld are beyond int64", (long long)r0, (long long)R);
  BL_CHECK_ARG(M >= 1 && M <= BL_BOOTSTRAP_MAX_MODELS, "bl_bootstrap_counts: M must be in [1, %d] models (got %d)",
               BL_BOOTSTRAP_MAX_MODELS, (int)M);
  BL_CHECK_ARG(K >= 1 && K <= BL_BOOTSTRAP_MAX_SCOUTS, "bl_bootstrap_counts: K must be in [1, %d] scouts (got %d)",
               BL_BOOTSTRAP_MAX_SCOUTS, (int)K);
  BL_CHECK_RANGE(bl_fits_int32(n), "bl_bootstrap_counts: n %lld is beyond int32 sample positions", (long long)n);
  if (R == 0) return BL_OK;
  const uint64_t base = bs_mix(seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull);
  hipStream_t st = (hipStream_t)stream;
  switch (M) {
    case 1: bs_launch<1>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
    case 2: bs_launch<2>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
    case 3: bs_launch<3>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
    case 4: bs_launch<4>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
    case 5: bs_launch<5>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
    default: bs_launch<6>(packed, (uint32_t)n, K, base, (uint64_t)r0, R, out, st); break;
  }
  BL_LAUNCH_CHECK("bl_bootstrap_counts");
  return BL_OK;
}

extern "C" int bl_bootstrap_curve_counts(const uint32_t* packed, const int16_t* bins, int64_t n, int32_t M, int32_t G, uint64_t seed,
                                         int64_t r0, int64_t R, int32_t* out, void* stream) {
  BL_CHECK_ARG(packed && bins && out, "bl_bootstrap_curve_counts: null packed / bins / out");
  BL_CHECK_ARG(n >= 1, "bl_bootstrap_curve_counts: n must be at least 1 (got %lld)", (long long)n);
  BL_CHECK_ARG(R >= 0 && r0 >= 0, "bl_bootstrap_curve_counts: negative replicate range (r0 %lld, R %lld)", (long long)r0, (long long)R);
  BL_CHECK_ARG(r0 <= INT64_MAX - R, "bl_bootstrap_curve_counts: replicates %lld + %lld are beyond int64", (long long)r0, (long long)R);
  BL_CHECK_ARG(M >= 1 && M <= BL_BOOTSTRAP_MAX_MODELS, "bl_bootstrap_curve_counts: M must be in [1, %d] models (got %d)",
               BL_BOOTSTRAP_MAX_MODELS, (int)M);
  BL_CHECK_ARG(G >= 1 && G <= BL_CURVE_MAX_BINS, "bl_bootstrap_curve_counts: G must be in [1, %d] bins (got %d)", BL_CURVE_MAX_BINS,
               (int)G);
  BL_CHECK_RANGE(bl_fits_int32(n), "bl_bootstrap_curve_counts: n %lld is beyond int32 sample positions", (long long)n);
  if (R == 0) return BL_OK;
  const uint64_t base = bs_mix(seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull);
  const int64_t grid = R < BS_MAX_GRID ? R : BS_MAX_GRID;
  hipLaunchKernelGGL(bootstrap_curve_counts_kernel, dim3((unsigned)grid, (unsigned)M), dim3(BS_THREADS), 0, (hipStream_t)stream, packed,
                     bins, (uint32_t)n, (int)M, (int)G, base, (uint64_t)r0, R, out);
  BL_LAUNCH_CHECK("bl_bootstrap_curve_counts");
  return BL_OK;
}
