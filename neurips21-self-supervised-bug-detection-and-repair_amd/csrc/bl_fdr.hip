// False-discovery-controlled warnings: conformal p-values against a reference of clean scores, and the Benjamini-Hochberg
// step-up over a scan (buglab/models/fdr.py; the NumPy twin is buglab/models/_fdr.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h; in short
//   score   s = src[nobug_idx[b]] (fp32; an index outside src reads as NaN)
//   count   c = #{ j : ref[j] <= s } over the sorted reference ref[0 .. n), n for a NaN s
//   R[c]    the number of scanned samples with count <= c
//   cutoff  c* = max{ c : R[c] > 0 and (double)((c + 1) N) <= q * (double)((n + 1) R[c]) }, -1 if none; flagged iff c <= c*
//   qv(c)   min over c' >= c with R[c'] > 0 of min(1, (double)((c' + 1) N) / (double)((n + 1) R[c']))
// Everything is fp32 compares, integer counts, one fp64 product or one fp64 quotient per bin and fp64 minima: no exp, no sum
// of floats, so the twin is equal bit for bit.  The only atomics are integer adds (any order gives the same bits).
//
// bl_fdr_counts  one thread per sample: the load and a binary search for the upper bound in ref.
// bl_fdr_bh      six launches behind one entry point, over bins = n + 1 histogram bins cut into chunks of FD_CHUNK:
//   0  hipMemsetAsync of the histogram (the caller's workspace may hold anything)
//   1  fd_hist         the histogram of the clamped counts.  The top bin (c = n: every sample that scores above the whole
//                      reference, most of a clean scan) is counted in a register and added once per workgroup; the others go
//                      to an LDS table where bins <= FD_LDS_BINS (flushed with one global add per non-empty bin) and straight
//                      to global memory beyond.  In both, the lanes of a wave that share the first active lane's bin add once
//                      (ballot and population count).
//   2  fd_chunk_sums   one workgroup per chunk: the chunk's total
//   3  fd_scan         one workgroup per chunk: its offset (the totals of the chunks before it, added by the workgroup itself:
//                      at most 257 of them), the inclusive prefix sum R in place, every bin's term of the q-value, the chunk's
//                      greatest qualifying c and its least term
//   4  fd_suffix_min   one workgroup per chunk: the least term of the chunks after it, then the suffix minimum in place
//   5  fd_samples      per sample the flag and the q-value; workgroup 0 reduces the chunks' cutoffs and writes out_cutoff
#include "bl_common.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / BL_WAVE;
constexpr int FD_ITEMS = 16;                       // bins per thread of a scan workgroup
constexpr int FD_CHUNK = FD_THREADS * FD_ITEMS;    // 4096 bins per scan workgroup
constexpr int FD_LDS_BINS = 16000;                 // histograms up to this many bins are privatised in LDS (62.5 KB of the 64 KB a
                                                   // workgroup may declare statically; measured 10 x faster than global adds: DESIGN.md)
constexpr int FD_HIST_PER_THREAD = 16;             // samples a histogram thread takes before the grid is widened
constexpr int FD_HIST_MAX_BLOCKS = 1024;

struct FdWorkspace {  // byte offsets into the caller's workspace
  int64_t hist, chunk_sum, chunk_cut, term, chunk_min, bytes;
  int nchunk;
};

inline FdWorkspace fd_workspace(int64_t n_ref) {
  FdWorkspace w;
  const int64_t bins = n_ref + 1;
  w.nchunk = (int)((bins + FD_CHUNK - 1) / FD_CHUNK);
  w.hist = 0;
  w.chunk_sum = 4 * ((bins + 1) / 2 * 2);
  w.chunk_cut = w.chunk_sum + 4 * (int64_t)w.nchunk;
  w.term = (w.chunk_cut + 4 * (int64_t)w.nchunk + 7) / 8 * 8;
  w.chunk_min = w.term + 8 * bins;
  w.bytes = w.chunk_min + 8 * (int64_t)w.nchunk;
  return w;
}

// ---- workgroup reductions and scans: integers and fp64 minima, exact in any order ----
// sum (MAX = false) or maximum of one int per thread, the same value in every thread.  s_red: FD_WAVES entries.
template <bool MAX>
__device__ __forceinline__ int fd_block_reduce_i32(int v, int* s_red) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const int other = __shfl_xor(v, o, BL_WAVE);
    v = MAX ? (other > v ? other : v) : v + other;
  }
  __syncthreads();  // the previous use of s_red has been read
  if (threadIdx.x % BL_WAVE == 0) s_red[threadIdx.x / BL_WAVE] = v;
  __syncthreads();
  int t = s_red[0];
#pragma unroll
  for (int w = 1; w < FD_WAVES; ++w) t = MAX ? (s_red[w] > t ? s_red[w] : t) : t + s_red[w];
  return t;
}

__device__ __forceinline__ double fd_min(double a, double b) { return b < a ? b : a; }  // no NaN ever enters

__device__ __forceinline__ double fd_block_min_f64(double v, double* s_red) {
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) v = fd_min(v, __shfl_xor(v, o, BL_WAVE));
  __syncthreads();
  if (threadIdx.x % BL_WAVE == 0) s_red[threadIdx.x / BL_WAVE] = v;
  __syncthreads();
  double t = s_red[0];
#pragma unroll
  for (int w = 1; w < FD_WAVES; ++w) t = fd_min(t, s_red[w]);
  return t;
}

// the sum of the values of the threads before this one.  s_scan: FD_THREADS entries.
__device__ __forceinline__ int fd_block_exclusive_sum(int v, int* s_scan) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_scan[tid] = v;
  __syncthreads();
  for (int o = 1; o < FD_THREADS; o <<= 1) {
    const int add = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  return s_scan[tid] - v;
}

// the minimum of the values of the threads after this one (+inf for the last).  s_scan: FD_THREADS entries.
__device__ __forceinline__ double fd_block_exclusive_suffix_min(double v, double* s_scan) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_scan[tid] = v;
  __syncthreads();
  for (int o = 1; o < FD_THREADS; o <<= 1) {
    const double other = tid + o < FD_THREADS ? s_scan[tid + o] : __builtin_huge_val();
    __syncthreads();
    s_scan[tid] = fd_min(s_scan[tid], other);
    __syncthreads();
  }
  const double after = tid + 1 < FD_THREADS ? s_scan[tid + 1] : __builtin_huge_val();
  return after;
}

// ---- bl_fdr_counts ----
__global__ __launch_bounds__(FD_THREADS) void fd_counts_kernel(const float* __restrict__ src, int64_t n_src,
                                                               const int32_t* __restrict__ nobug_idx, int B,
                                                               const float* __restrict__ ref, int n_ref, float* __restrict__ out_score,
                                                               int32_t* __restrict__ out_count, int64_t offset) {
  const int64_t b = (int64_t)blockIdx.x * FD_THREADS + threadIdx.x;
  if (b >= B) return;
  const int32_t j = nobug_idx[b];
  const float s = (j >= 0 && (int64_t)j < n_src) ? src[j] : __builtin_nanf("");
  int lo = 0, hi = n_ref;  // the upper bound: the first place whose entry is above s
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (ref[mid] <= s)
      lo = mid + 1;
    else
      hi = mid;
  }
  out_score[offset + b] = s;  // the host checked 0 <= offset and offset + B <= capacity
  out_count[offset + b] = s != s ? n_ref : lo;
}

// ---- bl_fdr_bh ----
__device__ __forceinline__ int fd_clamped(int32_t c, int n_ref) { return c < 0 ? 0 : (c > n_ref ? n_ref : c); }

template <bool IN_LDS>
__global__ __launch_bounds__(FD_THREADS) void fd_hist_kernel(const int32_t* __restrict__ count, int64_t N, int n_ref,
                                                             int32_t* __restrict__ hist) {
  __shared__ int s_hist[IN_LDS ? FD_LDS_BINS : 1];
  __shared__ int s_red[FD_WAVES];
  const int tid = threadIdx.x;
  if (IN_LDS) {
    for (int c = tid; c < n_ref; c += FD_THREADS) s_hist[c] = 0;
    __syncthreads();
  }
  int top = 0;
  for (int64_t i = (int64_t)blockIdx.x * FD_THREADS + tid; i < N; i += (int64_t)gridDim.x * FD_THREADS) {
    const int c = fd_clamped(count[i], n_ref);
    if (c == n_ref) {
      ++top;
      continue;
    }
    // the lanes that share the first active lane's bin (a scan's other crowd sits at c = 0: below the whole reference) add
    // once, through the lowest of them; the others add for themselves
    int32_t* table = IN_LDS ? s_hist : hist;
    const int lead = __builtin_amdgcn_readfirstlane(c);
    const unsigned long long same = __ballot(c == lead);
    if (c != lead)
      atomicAdd(&table[c], 1);
    else if (__ffsll(same) - 1 == tid % BL_WAVE)
      atomicAdd(&table[lead], __popcll(same));
  }
  top = fd_block_reduce_i32<false>(top, s_red);  // (its barriers also order the LDS adds before the flush)
  if (tid == 0 && top) atomicAdd(&hist[n_ref], top);
  if (IN_LDS)
    for (int c = tid; c < n_ref; c += FD_THREADS) {
      const int v = s_hist[c];
      if (v) atomicAdd(&hist[c], v);
    }
}

__global__ __launch_bounds__(FD_THREADS) void fd_chunk_sums_kernel(const int32_t* __restrict__ hist, int bins,
                                                                   int32_t* __restrict__ chunk_sum) {
  __shared__ int s_red[FD_WAVES];
  const int base = blockIdx.x * FD_CHUNK;
  int v = 0;
  for (int k = threadIdx.x; k < FD_CHUNK; k += FD_THREADS)
    if (base + k < bins) v += hist[base + k];
  v = fd_block_reduce_i32<false>(v, s_red);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = v;
}

__global__ __launch_bounds__(FD_THREADS) void fd_scan_kernel(int32_t* __restrict__ hist, int bins, int64_t N, double q,
                                                             const int32_t* __restrict__ chunk_sum, int32_t* __restrict__ chunk_cut,
                                                             double* __restrict__ term, double* __restrict__ chunk_min) {
  __shared__ int s_scan[FD_THREADS];
  __shared__ int s_red[FD_WAVES];
  __shared__ double s_min[FD_WAVES];
  const int tid = threadIdx.x, chunk = blockIdx.x;
  // the totals of the chunks before this one
  int before = 0;
  for (int j = tid; j < chunk; j += FD_THREADS) before += chunk_sum[j];
  before = fd_block_reduce_i32<false>(before, s_red);
  // this thread's FD_ITEMS consecutive bins
  const int first = chunk * FD_CHUNK + tid * FD_ITEMS;
  int h[FD_ITEMS];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < FD_ITEMS; ++k) {
    h[k] = first + k < bins ? hist[first + k] : 0;
    mine += h[k];
  }
  int run = before + fd_block_exclusive_sum(mine, s_scan);
  int cut = -1;
  double least = __builtin_huge_val();
  const int64_t n1 = (int64_t)bins;  // n + 1
#pragma unroll
  for (int k = 0; k < FD_ITEMS; ++k) {
    const int c = first + k;
    if (c >= bins) break;
    run += h[k];  // R[c]
    hist[c] = run;
    double t = __builtin_huge_val();
    if (run > 0) {
      const double lhs = (double)((int64_t)(c + 1) * N);  // exact: below 2^53
      const double pool = (double)(n1 * (int64_t)run);
      if (lhs <= q * pool) cut = c;  // one rounded product; c ascends, so the last one kept is the greatest
      t = lhs / pool;                // one correctly rounded quotient
      if (t > 1.0) t = 1.0;
    }
    term[c] = t;
    least = fd_min(least, t);
  }
  cut = fd_block_reduce_i32<true>(cut, s_red);
  least = fd_block_min_f64(least, s_min);
  if (tid == 0) {
    chunk_cut[chunk] = cut;
    chunk_min[chunk] = least;
  }
}

__global__ __launch_bounds__(FD_THREADS) void fd_suffix_min_kernel(double* __restrict__ term, int bins,
                                                                   const double* __restrict__ chunk_min, int nchunk) {
  __shared__ double s_scan[FD_THREADS];
  __shared__ double s_min[FD_WAVES];
  const int tid = threadIdx.x, chunk = blockIdx.x;
  double after = __builtin_huge_val();  // the least term of the chunks after this one
  for (int j = chunk + 1 + tid; j < nchunk; j += FD_THREADS) after = fd_min(after, chunk_min[j]);
  after = fd_block_min_f64(after, s_min);
  const int first = chunk * FD_CHUNK + tid * FD_ITEMS;
  double t[FD_ITEMS];
  double mine = __builtin_huge_val();
#pragma unroll
  for (int k = 0; k < FD_ITEMS; ++k) {
    t[k] = first + k < bins ? term[first + k] : __builtin_huge_val();
    mine = fd_min(mine, t[k]);
  }
  double run = fd_min(after, fd_block_exclusive_suffix_min(mine, s_scan));
#pragma unroll
  for (int k = FD_ITEMS - 1; k >= 0; --k) {
    run = fd_min(run, t[k]);
    if (first + k < bins) term[first + k] = run;
  }
}

__global__ __launch_bounds__(FD_THREADS) void fd_samples_kernel(const int32_t* __restrict__ count, int64_t N, int n_ref,
                                                                const int32_t* __restrict__ R, const double* __restrict__ qv,
                                                                const int32_t* __restrict__ chunk_cut, int nchunk,
                                                                int32_t* __restrict__ out_cutoff, int32_t* __restrict__ out_flag,
                                                                double* __restrict__ out_q) {
  __shared__ int s_red[FD_WAVES];
  const int tid = threadIdx.x;
  int cut = -1;
  for (int j = tid; j < nchunk; j += FD_THREADS) cut = chunk_cut[j] > cut ? chunk_cut[j] : cut;
  cut = fd_block_reduce_i32<true>(cut, s_red);
  if (blockIdx.x == 0 && tid == 0) {
    out_cutoff[0] = cut;
    out_cutoff[1] = cut >= 0 ? R[cut] : 0;
  }
  for (int64_t i = (int64_t)blockIdx.x * FD_THREADS + tid; i < N; i += (int64_t)gridDim.x * FD_THREADS) {
    const int c = fd_clamped(count[i], n_ref);
    out_flag[i] = c <= cut ? 1 : 0;
    out_q[i] = qv[c];
  }
}

inline int fd_sample_blocks(int64_t N) {
  const int64_t want = (N + (int64_t)FD_THREADS * FD_HIST_PER_THREAD - 1) / ((int64_t)FD_THREADS * FD_HIST_PER_THREAD);
  return (int)(want < 1 ? 1 : (want > FD_HIST_MAX_BLOCKS ? FD_HIST_MAX_BLOCKS : want));
}
}  // namespace

extern "C" int bl_fdr_counts(const float* src, int64_t n_src, const int32_t* nobug_idx, int32_t B, const float* ref, int64_t n_ref,
                             float* out_score, int32_t* out_count, int64_t offset, int64_t capacity, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_src >= 0, "bl_fdr_counts: negative size (B %d, n_src %lld)", (int)B, (long long)n_src);
  BL_CHECK_ARG(n_ref >= 1, "bl_fdr_counts: the reference holds %lld scores; at least 1 is needed", (long long)n_ref);
  BL_CHECK_RANGE(n_ref <= BL_FDR_MAX_REFERENCE, "bl_fdr_counts: n_ref = %lld is above BL_FDR_MAX_REFERENCE = %d", (long long)n_ref,
                 BL_FDR_MAX_REFERENCE);
  BL_CHECK_RANGE(bl_fits_int32(n_src), "bl_fdr_counts: index space beyond int32 (n_src %lld)", (long long)n_src);
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)B <= capacity - offset,
               "bl_fdr_counts: samples %lld .. %lld do not fit the result buffers of %lld samples", (long long)offset,
               (long long)offset + (long long)B, (long long)capacity);
  BL_CHECK_ARG(ref != nullptr, "bl_fdr_counts: null ref");
  BL_CHECK_ARG(B == 0 || (nobug_idx && out_score && out_count), "bl_fdr_counts: null nobug_idx / out_score / out_count");
  BL_CHECK_ARG(B == 0 || n_src == 0 || src, "bl_fdr_counts: null src with %lld values", (long long)n_src);
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(fd_counts_kernel, dim3((B + FD_THREADS - 1) / FD_THREADS), dim3(FD_THREADS), 0, (hipStream_t)stream, src, n_src,
                     nobug_idx, (int)B, ref, (int)n_ref, out_score, out_count, offset);
  BL_LAUNCH_CHECK("bl_fdr_counts");
  return BL_OK;
}

extern "C" int64_t bl_fdr_bh_workspace_bytes(int64_t n_ref) {
  if (n_ref < 1 || n_ref > BL_FDR_MAX_REFERENCE) return 0;
  return fd_workspace(n_ref).bytes;
}

extern "C" int bl_fdr_bh(const int32_t* count, int64_t N, int64_t n_ref, double q, void* workspace, int32_t* out_cutoff,
                         int32_t* out_flag, double* out_q, void* stream) {
  BL_CHECK_ARG(N >= 1, "bl_fdr_bh: N = %lld samples; at least 1 is needed", (long long)N);
  BL_CHECK_ARG(n_ref >= 1, "bl_fdr_bh: the reference holds %lld scores; at least 1 is needed", (long long)n_ref);
  BL_CHECK_ARG(q > 0.0 && q <= 1.0, "bl_fdr_bh: the level q = %g must be in (0, 1]", q);
  BL_CHECK_RANGE(n_ref <= BL_FDR_MAX_REFERENCE, "bl_fdr_bh: n_ref = %lld is above BL_FDR_MAX_REFERENCE = %d", (long long)n_ref,
                 BL_FDR_MAX_REFERENCE);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_fdr_bh: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(count && workspace && out_cutoff && out_flag && out_q, "bl_fdr_bh: null count / workspace / out_cutoff / out_flag / out_q");
  BL_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "bl_fdr_bh: the workspace must be 8-byte aligned");
  const FdWorkspace w = fd_workspace(n_ref);
  char* base = (char*)workspace;
  int32_t* hist = (int32_t*)(base + w.hist);
  int32_t* chunk_sum = (int32_t*)(base + w.chunk_sum);
  int32_t* chunk_cut = (int32_t*)(base + w.chunk_cut);
  double* term = (double*)(base + w.term);
  double* chunk_min = (double*)(base + w.chunk_min);
  const int bins = (int)n_ref + 1;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)bins, st);
  if (e != hipSuccess) {
    bl_set_error("bl_fdr_bh: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  const int sample_blocks = fd_sample_blocks(N);
  if (bins <= FD_LDS_BINS)
    hipLaunchKernelGGL(fd_hist_kernel<true>, dim3(sample_blocks), dim3(FD_THREADS), 0, st, count, N, (int)n_ref, hist);
  else
    hipLaunchKernelGGL(fd_hist_kernel<false>, dim3(sample_blocks), dim3(FD_THREADS), 0, st, count, N, (int)n_ref, hist);
  BL_LAUNCH_CHECK("bl_fdr_bh (histogram)");
  hipLaunchKernelGGL(fd_chunk_sums_kernel, dim3(w.nchunk), dim3(FD_THREADS), 0, st, hist, bins, chunk_sum);
  BL_LAUNCH_CHECK("bl_fdr_bh (chunk sums)");
  hipLaunchKernelGGL(fd_scan_kernel, dim3(w.nchunk), dim3(FD_THREADS), 0, st, hist, bins, N, q, chunk_sum, chunk_cut, term, chunk_min);
  BL_LAUNCH_CHECK("bl_fdr_bh (prefix sum)");
  hipLaunchKernelGGL(fd_suffix_min_kernel, dim3(w.nchunk), dim3(FD_THREADS), 0, st, term, bins, chunk_min, w.nchunk);
  BL_LAUNCH_CHECK("bl_fdr_bh (suffix minimum)");
  hipLaunchKernelGGL(fd_samples_kernel, dim3(sample_blocks), dim3(FD_THREADS), 0, st, count, N, (int)n_ref, hist, term, chunk_cut, w.nchunk,
                     out_cutoff, out_flag, out_q);
  BL_LAUNCH_CHECK("bl_fdr_bh (samples)");
  return BL_OK;
}
