// Drift detection: the permutation test of the kernel maximum mean discrepancy between two samples of site embeddings
// (buglab/models/drift.py; the NumPy twin is buglab/models/_drift.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h; in short, over the pooled rows
// Z = [X_ref ; X_new] (fp32 [N, D], N = n + m):
//   bandwidth  s = scale * 2 (mean_i |z_i|^2 - |mean_i z_i|^2) in fp64 from column sums; 0 ("no spread") when the difference
//              is at most 2^-40 of mean_i |z_i|^2
//   kernel     k(x, y) = exp(-max(|x|^2 + |y|^2 - 2 x.y, 0) / s)
//   subsets    row r of the mask: row 0 the observed split (i < n), rows 1 .. R the n rows first in (key, i) order with
//              key = mix(base + (r << 32) + i), row R + 1 all ones
//   sums       U = (K - c) mask^T;  A_r = sum_i mask[r, i] U[i, r] + c n n;  B_r = sum_i U[i, r] + c n N;  S = B_{R+1} + c N N
//
// bl_drift_bandwidth         dr_colsum_kernel: a wave per row, lanes stride over the columns; the row's |z|^2 in fp64 (its fp32
//                            rounding is the kernel's row norm) and per-workgroup column sums; dr_bandwidth_kernel: one workgroup
//                            adds the workgroups' partials in their order.  The sums are bl_segment_f64.h's.
// bl_drift_subsets           one workgroup per mask row.  The n-th smallest key by radix selection: 8 passes of 8 bits, each a
//                            256-bin integer histogram in LDS over the keys that share the prefix found so far (a key is
//                            recomputed, never stored); equal keys are taken in index order by an ordered scan.  Integers only.
// bl_drift_permutation_sums  dr_sums_kernel: a workgroup of 4 waves owns 64 rows i (16 per wave) and 16 CT mask rows r (CT = 4, 8, 16).  A wave
//                            keeps its 16 rows of Z in registers.  For every chunk of 32 rows j, staged in LDS:
//                              1  X = Z_j Z_i^T on v_mfma_f32_16x16x4_f32 (exact fp32 products; gfx950 has no xf32), two 16 x 16
//                                 tiles whose COLUMN is i and whose ROWS are j
//                              2  k = exp(-max(n_i + n_j - 2 X, 0) / s) - c in registers, cut into three bf16 planes by
//                                 truncation: hi + mid + lo == k exactly (8 + 8 + 8 significand bits)
//                              3  Y[r, i] += mask[r, j] k[j, i] on v_mfma_f32_16x16x32_bf16, one MFMA per plane: the two X tiles
//                                 are the B operand as they lie (the sum runs over X's row index, so no lane moves and no LDS),
//                                 the 0/1 mask the A operand, exact in bf16 (it enters as 2.0, a power of two, because a byte
//                                 becomes that bf16 with one shift; the factor leaves in the epilogue)
//                            Per 16-row tile and mask row the epilogue adds Y over its 16 rows in fp64 (xor butterfly) and stores
//                            the two partials; dr_finish_kernel adds the tiles in their order in fp64.  No atomics; the order of
//                            every sum is fixed by N alone, so the bits do not depend on CT or the grid.
//
// OPERAND MAPS.  16x16x4 f32: lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; here lane group g = l >> 4
// supplies column d = 16 q + 4 g + e of Z in MFMA (q, e) for both operands, which pairs the same d on either side.  C/D of every
// 16x16 shape: col = l & 15, row = 4 g + reg.  16x16x32 bf16: lane l gives A[row l & 15][k = 8 g + e] and B[k = 8 g + e][col l & 15],
// e = 0 .. 7; the hardware pairs (g, e) of A with (g, e) of B, so with B = [X_0 regs 0..3 | X_1 regs 0..3] element e of group g
// is row j0 + 16 (e >> 2) + 4 g + (e & 3), and the mask's fragment is read from exactly those j.
#include "bl_common.h"
#include "bl_segment_f64.h"

namespace {
constexpr int DR_THREADS = 256;
constexpr int DR_WAVES = DR_THREADS / BL_WAVE;
constexpr int DR_BI = 16 * DR_WAVES;   // rows i of a workgroup
constexpr int DR_BJ = 32;              // rows j of a chunk
constexpr int DR_ROWS_PER_BLOCK = 256; // rows of a column-sum workgroup
constexpr double DR_NO_SPREAD = 0x1p-40;

typedef float dr_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 dr_v8s __attribute__((ext_vector_type(8)));
typedef unsigned int dr_v4u __attribute__((ext_vector_type(4)));

__host__ __device__ inline uint64_t dr_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline int64_t dr_mask_ld(int64_t N) { return (N + DR_BJ - 1) / DR_BJ * DR_BJ; }
inline int64_t dr_tiles16(int64_t N) { return (N + 15) / 16; }
inline int64_t dr_colsum_blocks(int64_t N) { return (N + DR_ROWS_PER_BLOCK - 1) / DR_ROWS_PER_BLOCK; }

// ---- bl_drift_bandwidth ----
__global__ __launch_bounds__(DR_THREADS) void dr_colsum_kernel(const float* __restrict__ z, int64_t ldz, int N, int D,
                                                               float* __restrict__ rown, double* __restrict__ part) {
  __shared__ double s_col[DR_WAVES][BL_DRIFT_MAX_D];
  __shared__ double s_sq[DR_WAVES];
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * DR_ROWS_PER_BLOCK;
  double col[BL_DRIFT_MAX_D / BL_WAVE];
#pragma unroll
  for (int k = 0; k < BL_DRIFT_MAX_D / BL_WAVE; ++k) col[k] = 0.0;
  double total = 0.0;
  for (int rr = wave; rr < DR_ROWS_PER_BLOCK; rr += DR_WAVES) {
    const int64_t row = row0 + rr;
    if (row >= N) break;  // the whole wave leaves
    const float* zr = z + row * ldz;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < BL_DRIFT_MAX_D / BL_WAVE; ++k) {
      const int d = lane + k * BL_WAVE;
      if (d < D) {
        const double v = (double)zr[d];
        col[k] += v;
        sq += v * v;
      }
    }
    sq = bl_wave_sum_f64(sq);
    if (lane == 0) rown[row] = (float)sq;
    total += sq;
  }
#pragma unroll
  for (int k = 0; k < BL_DRIFT_MAX_D / BL_WAVE; ++k) s_col[wave][lane + k * BL_WAVE] = col[k];
  if (lane == 0) s_sq[wave] = total;
  __syncthreads();
  double* mine = part + (int64_t)blockIdx.x * (D + 1);
  for (int d = tid; d < D; d += DR_THREADS) {
    double t = s_col[0][d];
#pragma unroll
    for (int w = 1; w < DR_WAVES; ++w) t += s_col[w][d];
    mine[d] = t;
  }
  if (tid == 0) {
    double t = s_sq[0];
#pragma unroll
    for (int w = 1; w < DR_WAVES; ++w) t += s_sq[w];
    mine[D] = t;
  }
}

__global__ __launch_bounds__(DR_THREADS) void dr_bandwidth_kernel(const double* __restrict__ part, int nb, int N, int D, double scale,
                                                                  double* __restrict__ out) {
  __shared__ double s_acc[DR_THREADS];
  const int tid = threadIdx.x;
  double acc = 0.0;  // sum over this thread's columns of mean_d^2
  for (int d = tid; d < D; d += DR_THREADS) {
    double t = 0.0;
    for (int b = 0; b < nb; ++b) t += part[(int64_t)b * (D + 1) + d];
    const double mean = t / (double)N;
    acc += mean * mean;
  }
  bl_tree_sum_f64<DR_THREADS>(acc, s_acc);
  if (tid == 0) {
    double sq = 0.0;
    for (int b = 0; b < nb; ++b) sq += part[(int64_t)b * (D + 1) + D];
    const double meansq = sq / (double)N;
    const double spread = meansq - s_acc[0];
    out[0] = spread > meansq * DR_NO_SPREAD ? scale * 2.0 * spread : 0.0;
  }
}

// ---- bl_drift_subsets ----
__global__ __launch_bounds__(DR_THREADS) void dr_subsets_kernel(int N, int n, int R, uint64_t base, uint8_t* __restrict__ mask,
                                                                int64_t ldm) {
  __shared__ int s_hist[256];
  __shared__ int s_wave[DR_WAVES];
  __shared__ uint64_t s_prefix;
  __shared__ int s_want, s_ties;
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int r = blockIdx.x;
  uint8_t* row = mask + (int64_t)r * ldm;
  if (r == 0 || r == R + 1) {  // the observed split, and the ones
    const int ones = r == 0 ? n : N;
    for (int64_t i = tid; i < ldm; i += DR_THREADS) row[i] = i < ones ? 1 : 0;
    return;
  }
  const uint64_t ctr = base + ((uint64_t)r << 32);
  // the n-th smallest key: after pass p the top 8 (p + 1) bits of it are known, and how many keys below that prefix there are
  uint64_t prefix = 0;
  int want = n - 1;  // the wanted key's rank among the keys that share the prefix (0-based)
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    s_hist[tid] = 0;  // DR_THREADS == 256 bins
    __syncthreads();
    for (int i = tid; i < N; i += DR_THREADS) {
      const uint64_t key = dr_mix(ctr + (uint64_t)i);
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((key >> shift) & 0xFF)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int before = 0, b = 0;
      for (; b < 255; ++b) {
        if (before + s_hist[b] > want) break;
        before += s_hist[b];
      }
      s_prefix = prefix | ((uint64_t)b << shift);
      s_want = want - before;
      s_ties = s_hist[b];
    }
    __syncthreads();
    prefix = s_prefix;
    want = s_want;
  }
  // `prefix` is the n-th smallest key; of the s_ties rows that carry it the first want + 1 in index order are taken
  const int ties = s_ties, take = want + 1;
  if (ties == take) {  // every row with that key is in: no order to establish
    for (int64_t i = tid; i < ldm; i += DR_THREADS) row[i] = (i < N && dr_mix(ctr + (uint64_t)i) <= prefix) ? 1 : 0;
    return;
  }
  int seen = 0;  // equal keys before this chunk
  for (int64_t i0 = 0; i0 < ldm; i0 += DR_THREADS) {
    const int64_t i = i0 + tid;
    const uint64_t key = i < N ? dr_mix(ctr + (uint64_t)i) : ~0ull;
    const bool tie = i < N && key == prefix;
    const unsigned long long ballot = __ballot(tie);
    const int in_wave = __popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();  // s_wave of the previous chunk has been read
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    int before = seen + in_wave, all = 0;
    for (int w = 0; w < DR_WAVES; ++w) {
      if (w < wave) before += s_wave[w];
      all += s_wave[w];
    }
    if (i < ldm) row[i] = (i < N && (key < prefix || (tie && before < take))) ? 1 : 0;
    seen += all;
  }
}

// ---- bl_drift_permutation_sums ----
__device__ __forceinline__ unsigned int dr_pack(float a, float b) {  // two floats whose low 16 bits are zero -> two bf16
  return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u);
}
// two mask bytes (0 / 1) -> two bf16 (0.0 / 2.0): the byte times 0x40 is the bf16's high byte
__device__ __forceinline__ unsigned int dr_two(unsigned int m) { return ((m & 0xFFu) << 14) | ((m & 0xFF00u) << 22); }

template <int DCH, int CT>
__global__ __launch_bounds__(DR_THREADS) void dr_sums_kernel(const float* __restrict__ z, int64_t ldz, int N, int n, int D, int Dp,
                                                             const float* __restrict__ rown, const uint8_t* __restrict__ mask,
                                                             int64_t ldm, int C, const double* __restrict__ bandwidth, float shift,
                                                             double* __restrict__ part_a, double* __restrict__ part_b,
                                                             double* __restrict__ u0, double* __restrict__ rho) {
  extern __shared__ __attribute__((aligned(16))) float dr_lds[];  // [DR_BJ][Dp + 4] rows j of Z, then their DR_BJ norms
  const int LD = Dp + 4;  // 16 rows x 4 lane groups of 16-byte reads then fall on distinct banks
  float* s_z = dr_lds;
  float* s_n = dr_lds + DR_BJ * LD;
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int col = lane & 15, g = lane >> 4;
  const int i = (int)blockIdx.x * DR_BI + wave * 16 + col;  // this lane's row i (the column of X and of Y)
  const int c0 = (int)blockIdx.y * 16 * CT;
  const int nq = Dp / 16;
  const double s = bandwidth[0];
  const float neg_inv_s = s > 0.0 ? (float)(-1.0 / s) : 0.0f;  // no spread: every kernel value is 1

  dr_v4f zi[4 * DCH];  // columns 16 q + 4 g .. + 3 of row i (zero beyond N and D)
#pragma unroll
  for (int q = 0; q < 4 * DCH; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d = 16 * q + 4 * g + e;
      zi[q][e] = (i < N && d < D) ? z[(int64_t)i * ldz + d] : 0.0f;
    }
  }
  const float ni = i < N ? rown[i] : 0.0f;

  dr_v4f acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) acc[t] = dr_v4f{0.0f, 0.0f, 0.0f, 0.0f};

  // Up to Dp = 256 a chunk travels global -> registers -> LDS, and the loads of chunk j0 + 32 are issued before chunk j0 is
  // computed on, so their latency hides behind the MFMAs; at Dp = 512 the registers are Z_i's and the chunk is staged in place.
  constexpr bool PREFETCH = DCH <= 4;
  constexpr int PF_ROWS = DR_BJ / DR_WAVES;
  float pf[PREFETCH ? PF_ROWS * DCH : 1];
  float pfn = 0.0f;
  auto load_chunk = [&](int j0) {
#pragma unroll
    for (int k = 0; k < PF_ROWS; ++k) {
      const int j = j0 + wave + DR_WAVES * k;
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        const int d = lane + BL_WAVE * c;
        pf[PREFETCH ? k * DCH + c : 0] = (j < N && d < D) ? z[(int64_t)j * ldz + d] : 0.0f;
      }
    }
    pfn = (tid < DR_BJ && j0 + tid < N) ? rown[j0 + tid] : 0.0f;
  };
  if (PREFETCH) load_chunk(0);

  for (int j0 = 0; j0 < N; j0 += DR_BJ) {
    __syncthreads();  // the previous chunk has been read
    if (PREFETCH) {
#pragma unroll
      for (int k = 0; k < PF_ROWS; ++k) {
#pragma unroll
        for (int c = 0; c < DCH; ++c) {
          const int d = lane + BL_WAVE * c;
          if (d < Dp) s_z[(wave + DR_WAVES * k) * LD + d] = pf[PREFETCH ? k * DCH + c : 0];
        }
      }
      if (tid < DR_BJ) s_n[tid] = pfn;
    } else {
      for (int rr = wave; rr < DR_BJ; rr += DR_WAVES) {
        const int j = j0 + rr;
        for (int d = lane; d < Dp; d += BL_WAVE) s_z[rr * LD + d] = (j < N && d < D) ? z[(int64_t)j * ldz + d] : 0.0f;
      }
      if (tid < DR_BJ) s_n[tid] = j0 + tid < N ? rown[j0 + tid] : 0.0f;
    }
    __syncthreads();
    if (PREFETCH && j0 + DR_BJ < N) load_chunk(j0 + DR_BJ);

    dr_v4f x0 = {0.0f, 0.0f, 0.0f, 0.0f}, x1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 4 * DCH; ++q) {
      if (q < nq) {
        const dr_v4f a0 = *reinterpret_cast<const dr_v4f*>(s_z + col * LD + 16 * q + 4 * g);
        const dr_v4f a1 = *reinterpret_cast<const dr_v4f*>(s_z + (16 + col) * LD + 16 * q + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], zi[q][e], x0, 0, 0, 0);
          x1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], zi[q][e], x1, 0, 0, 0);
        }
      }
    }
    // the kernel values of rows j0 + 16 t + 4 g + e against row i, minus the shift, in three exact bf16 planes
    float hi[8], mid[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = e < 4 ? x0[e] : x1[e - 4];
      const float nj = s_n[16 * (e >> 2) + 4 * g + (e & 3)];
      const float d2 = fmaxf((ni + nj) - 2.0f * x, 0.0f);
      const float k = expf(d2 * neg_inv_s) - shift;
      hi[e] = __uint_as_float(__float_as_uint(k) & 0xFFFF0000u);
      const float r1 = k - hi[e];  // exact
      mid[e] = __uint_as_float(__float_as_uint(r1) & 0xFFFF0000u);
      lo[e] = r1 - mid[e];         // exact, and at most 8 significant bits
    }
    dr_v4u phi, pmid, plo;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      phi[w] = dr_pack(hi[2 * w], hi[2 * w + 1]);
      pmid[w] = dr_pack(mid[2 * w], mid[2 * w + 1]);
      plo[w] = dr_pack(lo[2 * w], lo[2 * w + 1]);
    }
    const dr_v8s bhi = __builtin_bit_cast(dr_v8s, phi), bmid = __builtin_bit_cast(dr_v8s, pmid), blo = __builtin_bit_cast(dr_v8s, plo);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int r = c0 + 16 * t + col;
      unsigned int m0 = 0, m1 = 0;
      if (r < C) {  // ldm is a multiple of DR_BJ and 4-byte aligned: both words lie inside row r
        const uint8_t* mr = mask + (int64_t)r * ldm + j0 + 4 * g;
        m0 = *reinterpret_cast<const unsigned int*>(mr);
        m1 = *reinterpret_cast<const unsigned int*>(mr + 16);
      }
      const dr_v4u pa = {dr_two(m0), dr_two(m0 >> 16), dr_two(m1), dr_two(m1 >> 16)};
      const dr_v8s a = __builtin_bit_cast(dr_v8s, pa);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, blo, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bmid, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bhi, acc[t], 0, 0, 0);
    }
  }

  // Y[r = c0 + 16 t + 4 g + e][i]: the sums over this tile's 16 rows i, and the two columns of U the witness takes
  const bool live = i < N;
  const int64_t tile = (int64_t)blockIdx.x * DR_WAVES + wave;
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = c0 + 16 * t + 4 * g + e;
      const bool in = r < C;
      const double y = 0.5 * (double)acc[t][e];  // the mask entered as 2.0
      const bool member = live && in && mask[(int64_t)(in ? r : 0) * ldm + (live ? i : 0)] != 0;
      double pa = member ? y : 0.0, pb = live ? y : 0.0;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        pa += __shfl_xor(pa, o, BL_WAVE);
        pb += __shfl_xor(pb, o, BL_WAVE);
      }
      if (in && col == 0 && tile * 16 < N) {
        part_a[tile * C + r] = pa;
        part_b[tile * C + r] = pb;
      }
      if (live && r == 0) u0[i] = y + (double)shift * (double)n;
      if (live && r == C - 1) rho[i] = y + (double)shift * (double)N;
    }
  }
}

__global__ __launch_bounds__(DR_THREADS) void dr_finish_kernel(const double* __restrict__ part_a, const double* __restrict__ part_b,
                                                               int64_t tiles, int C, int N, int n, double shift,
                                                               double* __restrict__ out) {
  const int r = (int)(blockIdx.x * DR_THREADS + threadIdx.x);
  if (r >= C) return;
  double a = 0.0, b = 0.0;
  for (int64_t t = 0; t < tiles; ++t) {
    a += part_a[t * C + r];
    b += part_b[t * C + r];
  }
  const int R1 = C - 1;  // R + 1 subsets, then the ones
  if (r < R1) {
    out[r] = a + shift * (double)n * (double)n;
    out[R1 + r] = b + shift * (double)n * (double)N;
  } else {
    out[2 * R1] = b + shift * (double)N * (double)N;
  }
}

template <int DCH, int CT>
int dr_launch_sums(dim3 grid, int lds, hipStream_t st, const float* z, int64_t ldz, int N, int n, int D, int Dp, const float* rown,
                   const uint8_t* mask, int64_t ldm, int C, const double* bandwidth, float shift, double* part_a, double* part_b,
                   double* u0, double* rho) {
  static bool raised[BL_MAX_DEVICES] = {};
  if (lds > 64 * 1024 && bl_raise_lds_limit_once((const void*)dr_sums_kernel<DCH, CT>, lds, raised) != BL_OK) {
    bl_set_error("bl_drift_permutation_sums: cannot raise the LDS limit to %d bytes", lds);
    return BL_EINVAL;
  }
  hipLaunchKernelGGL((dr_sums_kernel<DCH, CT>), grid, dim3(DR_THREADS), (size_t)lds, st, z, ldz, N, n, D, Dp, rown, mask, ldm, C, bandwidth,
                     shift, part_a, part_b, u0, rho);
  return BL_OK;
}

template <int CT, class... Args>
int dr_launch_by_dim(int Dp, Args... args) {
  if (Dp <= 64) return dr_launch_sums<1, CT>(args...);
  if (Dp <= 128) return dr_launch_sums<2, CT>(args...);
  if (Dp <= 256) return dr_launch_sums<4, CT>(args...);
  return dr_launch_sums<8, CT>(args...);
}
}  // namespace

extern "C" int32_t bl_drift_ok(int32_t D, int64_t R) { return D >= 1 && D <= BL_DRIFT_MAX_D && R >= 1 && R <= BL_DRIFT_MAX_PERMUTATIONS; }

extern "C" int64_t bl_drift_mask_ld(int64_t N) { return N >= 0 && bl_fits_int32(N) ? dr_mask_ld(N) : 0; }

extern "C" int64_t bl_drift_bandwidth_workspace_bytes(int64_t N, int32_t D) {
  if (N < 0 || D < 1 || D > BL_DRIFT_MAX_D) return 0;
  return dr_colsum_blocks(N) * (int64_t)(D + 1) * 8;
}

extern "C" int bl_drift_bandwidth(const float* z, int64_t ldz, int64_t N, int32_t D, double scale, void* workspace,
                                  int64_t workspace_bytes, float* out_rownorm, double* out_bandwidth, void* stream) {
  BL_CHECK_ARG(z && out_rownorm && out_bandwidth, "bl_drift_bandwidth: null z / out_rownorm / out_bandwidth");
  BL_CHECK_ARG(N >= 4 && D >= 1 && ldz >= D, "bl_drift_bandwidth: need N >= 4, D >= 1 and a row stride of at least D (got N %lld, D %d, ldz %lld)",
               (long long)N, (int)D, (long long)ldz);
  BL_CHECK_ARG(scale > 0.0 && scale < __builtin_huge_val(), "bl_drift_bandwidth: the scale must be positive and finite (got %g)", scale);
  BL_CHECK_RANGE(D <= BL_DRIFT_MAX_D, "bl_drift_bandwidth: D = %d is above BL_DRIFT_MAX_D = %d", (int)D, BL_DRIFT_MAX_D);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_drift_bandwidth: N = %lld is beyond int32", (long long)N);
  const int64_t need = bl_drift_bandwidth_workspace_bytes(N, D);
  BL_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
               "bl_drift_bandwidth: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need,
               (long long)workspace_bytes);
  BL_CHECK_ARG(((uintptr_t)out_bandwidth & 7) == 0, "bl_drift_bandwidth: out_bandwidth must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)dr_colsum_blocks(N);
  hipLaunchKernelGGL(dr_colsum_kernel, dim3((unsigned)nb), dim3(DR_THREADS), 0, st, z, ldz, (int)N, (int)D, out_rownorm, (double*)workspace);
  BL_LAUNCH_CHECK("bl_drift_bandwidth (column sums)");
  hipLaunchKernelGGL(dr_bandwidth_kernel, dim3(1), dim3(DR_THREADS), 0, st, (const double*)workspace, nb, (int)N, (int)D, scale, out_bandwidth);
  BL_LAUNCH_CHECK("bl_drift_bandwidth");
  return BL_OK;
}

extern "C" int bl_drift_subsets(int64_t N, int64_t n, int64_t R, uint64_t seed, uint8_t* out_mask, int64_t ldm, void* stream) {
  BL_CHECK_ARG(out_mask != nullptr, "bl_drift_subsets: null out_mask");
  BL_CHECK_ARG(n >= 2 && N - n >= 2, "bl_drift_subsets: both samples need at least 2 rows (got n %lld of N %lld)", (long long)n, (long long)N);
  BL_CHECK_ARG(R >= 1, "bl_drift_subsets: R must be at least 1 (got %lld)", (long long)R);
  BL_CHECK_RANGE(bl_fits_int32(N) && R <= BL_DRIFT_MAX_PERMUTATIONS, "bl_drift_subsets: N = %lld is beyond int32 or R = %lld above %d",
                 (long long)N, (long long)R, BL_DRIFT_MAX_PERMUTATIONS);
  BL_CHECK_ARG(ldm == dr_mask_ld(N) && ((uintptr_t)out_mask & 3) == 0,
               "bl_drift_subsets: the mask's row stride must be bl_drift_mask_ld(N) = %lld (got %lld) and its base 4-byte aligned",
               (long long)dr_mask_ld(N), (long long)ldm);
  const uint64_t base = dr_mix(seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull);
  hipLaunchKernelGGL(dr_subsets_kernel, dim3((unsigned)(R + 2)), dim3(DR_THREADS), 0, (hipStream_t)stream, (int)N, (int)n, (int)R, base,
                     out_mask, ldm);
  BL_LAUNCH_CHECK("bl_drift_subsets");
  return BL_OK;
}

extern "C" int64_t bl_drift_sums_workspace_bytes(int64_t N, int64_t R) {
  if (N < 0 || R < 1 || R > BL_DRIFT_MAX_PERMUTATIONS) return 0;
  return 2 * dr_tiles16(N) * (R + 2) * 8;
}

extern "C" int bl_drift_permutation_sums(const float* z, int64_t ldz, int64_t N, int64_t n, int32_t D, const float* rownorm,
                                         const uint8_t* mask, int64_t ldm, int64_t R, const double* bandwidth, double shift,
                                         int32_t col_tiles, void* workspace, int64_t workspace_bytes, double* out_sums, double* out_u0,
                                         double* out_rho, void* stream) {
  BL_CHECK_ARG(z && rownorm && mask && bandwidth && out_sums && out_u0 && out_rho,
               "bl_drift_permutation_sums: null z / rownorm / mask / bandwidth / out_sums / out_u0 / out_rho");
  BL_CHECK_ARG(n >= 2 && N - n >= 2, "bl_drift_permutation_sums: both samples need at least 2 rows (got n %lld of N %lld)", (long long)n,
               (long long)N);
  BL_CHECK_ARG(R >= 1 && D >= 1 && ldz >= D, "bl_drift_permutation_sums: need R >= 1, D >= 1 and a row stride of at least D (got R %lld, D %d, ldz %lld)",
               (long long)R, (int)D, (long long)ldz);
  BL_CHECK_RANGE(D <= BL_DRIFT_MAX_D && R <= BL_DRIFT_MAX_PERMUTATIONS, "bl_drift_permutation_sums: D = %d is above %d or R = %lld above %d",
                 (int)D, BL_DRIFT_MAX_D, (long long)R, BL_DRIFT_MAX_PERMUTATIONS);
  BL_CHECK_RANGE(bl_fits_int32(N) && dr_tiles16(N) / DR_WAVES < 0x7fffffff, "bl_drift_permutation_sums: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(ldm == dr_mask_ld(N) && ((uintptr_t)mask & 3) == 0,
               "bl_drift_permutation_sums: the mask's row stride must be bl_drift_mask_ld(N) = %lld (got %lld) and its base 4-byte aligned",
               (long long)dr_mask_ld(N), (long long)ldm);
  BL_CHECK_ARG(col_tiles == 0 || col_tiles == 4 || col_tiles == 8 || col_tiles == 16,
               "bl_drift_permutation_sums: col_tiles must be 0 (default), 4, 8 or 16 (got %d)", (int)col_tiles);
  BL_CHECK_ARG(shift >= 0.0 && shift <= 1.0, "bl_drift_permutation_sums: the shift must be in [0, 1] (got %g)", shift);
  const int64_t need = bl_drift_sums_workspace_bytes(N, R);
  BL_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
               "bl_drift_permutation_sums: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need,
               (long long)workspace_bytes);
  BL_CHECK_ARG((((uintptr_t)out_sums | (uintptr_t)out_u0 | (uintptr_t)out_rho | (uintptr_t)bandwidth) & 7) == 0,
               "bl_drift_permutation_sums: the fp64 buffers must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int C = (int)R + 2, Dp = (D + 63) / 64 * 64;
  // Every workgroup repeats the first product, so the more mask rows it takes the better -- as long as the grid still gives
  // every compute unit a workgroup (256; measured in DESIGN.md).  At Dp = 512 the widest form has no registers to spare.
  const int64_t row_tiles = (N + DR_BI - 1) / DR_BI;
  int CT = 4;
  for (int ct = Dp <= 256 ? 16 : 8; ct > 4; ct /= 2)
    if (C > 8 * ct && row_tiles * ((C + 16 * ct - 1) / (16 * ct)) >= 256) {
      CT = ct;
      break;
    }
  if (col_tiles) CT = col_tiles;
  const int64_t tiles = dr_tiles16(N);
  double* part_a = (double*)workspace;
  double* part_b = part_a + tiles * C;
  const dim3 grid((unsigned)((N + DR_BI - 1) / DR_BI), (unsigned)((C + 16 * CT - 1) / (16 * CT)));
  const int lds = (DR_BJ * (Dp + 4) + DR_BJ) * (int)sizeof(float);
  const float shift_f = (float)shift;  // the kernel subtracts this fp32 value, and the same value comes back in fp64
  int rc;
  if (CT == 16)
    rc = dr_launch_by_dim<16>(Dp, grid, lds, st, z, ldz, (int)N, (int)n, (int)D, Dp, rownorm, mask, ldm, C, bandwidth, shift_f, part_a, part_b,
                              out_u0, out_rho);
  else if (CT == 4)
    rc = dr_launch_by_dim<4>(Dp, grid, lds, st, z, ldz, (int)N, (int)n, (int)D, Dp, rownorm, mask, ldm, C, bandwidth, shift_f, part_a, part_b,
                             out_u0, out_rho);
  else
    rc = dr_launch_by_dim<8>(Dp, grid, lds, st, z, ldz, (int)N, (int)n, (int)D, Dp, rownorm, mask, ldm, C, bandwidth, shift_f, part_a, part_b,
                             out_u0, out_rho);
  if (rc != BL_OK) return rc;
  BL_LAUNCH_CHECK("bl_drift_permutation_sums");
  hipLaunchKernelGGL(dr_finish_kernel, dim3((unsigned)((C + DR_THREADS - 1) / DR_THREADS)), dim3(DR_THREADS), 0, st, part_a, part_b, tiles, C,
                     (int)N, (int)n, (double)shift_f, out_sums);
  BL_LAUNCH_CHECK("bl_drift_permutation_sums (finish)");
  return BL_OK;
}
