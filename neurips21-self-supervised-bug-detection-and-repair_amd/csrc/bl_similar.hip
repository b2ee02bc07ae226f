// Similar-bug search: the embedding of a bug site, its int8 image, an exact top-C search on the integer MFMA and an fp64
// re-score (buglab/models/similar.py; the NumPy twin is buglab/models/_similar.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h; in short, with Dp = D rounded up to a
// multiple of 64:
//   centre    c_d = (float)((double)x_d - (double)mean_d)
//   row       amax = max |c_d|; sumsq = sum c_d c_d in fp64 in bl_lane_dot_f64.h's order; invalid if a c_d is not finite or amax == 0
//   quantise  q_d = (int8)rint((double)c_d * (127.0 / (double)amax)), columns D .. Dp - 1 zero; r = (amax amax) / sumsq;
//             an invalid row: q = 0, sumsq = 0, r = 0
//   key       idot = sum_d qx_d qy_d (int32, exact); key = (double)((int64)idot * |idot|) * r_y
//   search    per valid query the first C valid index rows in bl_better's order on (key, index), -1 padded
//   re-score  dot = sum_d cx_d cy_d as sumsq; key2 = (dot |dot|) / sumsq_y; the first k candidates by (key2, index, place)
// Integer products, fp64 sums in a fixed order, one rounded product or quotient per key: no exp, no sqrt, no atomics, so the
// twin is equal bit for bit whatever the tile sizes, the number of slices and the launch geometry.
//
// bl_sim_embed_sites  one wave per sample: the first maximum of its location entries (or the true one), the row of h behind it
// bl_sim_quantize     one wave per row
// bl_sim_search_i8    sm_search_kernel: a workgroup takes 16 queries and one slice of the index; each of its waves walks 16-row
//                     index tiles through v_mfma_i32_16x16x64_i8 (index rows = A, queries = B, so a lane owns ONE query, its
//                     column, and sees 4 index rows per tile) and keeps a sorted list of its 16 best (key, index) pairs in
//                     registers; the 16 lists per query (4 row groups x 4 waves) are ranked through LDS into the slice's
//                     sorted partial list.  sm_merge_kernel: one workgroup per query ranks the S partial lists into the
//                     exact top C.  The union of top-16 lists holds the top 16 of the union, so neither step loses anything.
// bl_sim_rescore      one workgroup per query: a wave per candidate for the dots, then a ranking of at most 16
//
// OPERAND MAP of the MFMA: lane l loads bytes 16 (l >> 4) .. 16 (l >> 4) + 15 of the 64-byte k-chunk of row (l & 15) -- of an
// index row for A, of a query row for B.  Both images are row-major [rows, Dp] and summed over the same k, and the hardware pairs
// byte j of A's lane group g with byte j of B's lane group g, so any k order inside a chunk gives the same exact sum.  The C/D
// map is the dtype-independent one: col = l & 15 (the query), row = 4 (l >> 4) + reg (the index row).
#include "bl_common.h"
#include "bl_lane_dot_f64.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / BL_WAVE;
constexpr int SM_L = BL_SIM_MAX_CANDIDATES;     // entries of every private and partial list
constexpr int SM_TILE = 16;                     // queries per workgroup, index rows per MFMA tile
constexpr int SM_LISTS = 4 * SM_WAVES;          // private lists per query in a workgroup
constexpr int SM_PER_QUERY = SM_LISTS * SM_L;   // 256 entries: one per thread
constexpr int SM_MAX_CHUNKS = BL_SIM_MAX_D / 64;

typedef int sm_v4i __attribute__((ext_vector_type(4)));

// ---- bl_sim_embed_sites ----
__global__ __launch_bounds__(SM_THREADS) void sm_embed_kernel(const float* __restrict__ flat, int64_t n_flat,
                                                              const int32_t* __restrict__ loc_idx, const int32_t* __restrict__ loc_off,
                                                              int64_t total_loc, int B, const int32_t* __restrict__ cand_rows, int64_t n_cand,
                                                              const float* __restrict__ h, int64_t ldh, int64_t n_rows, int D,
                                                              const int32_t* __restrict__ truth, int skip_nobug, int mode,
                                                              float* __restrict__ out_rows, int32_t* __restrict__ out_place,
                                                              float* __restrict__ out_logprob, int64_t offset) {
  const int lane = threadIdx.x % BL_WAVE;
  const int64_t b = (int64_t)blockIdx.x * SM_WAVES + threadIdx.x / BL_WAVE;
  if (b >= B) return;  // the whole wave leaves
  const int64_t at = offset + b;  // the host checked 0 <= offset and offset + B <= capacity
  int64_t lo;
  const int n = (int)bl_csr_row(loc_off, b, total_loc, lo);  // the sample's location entries: its candidates, then NO_BUG
  int place = -1;
  if (mode == 1) {
    place = truth[b];
  } else {
    const int searched = skip_nobug ? n - 1 : n;
    double bv = 0.0;
    int bi = -1;
    for (int j = lane; j < searched; j += BL_WAVE) {
      const double v = bl_load_f64(flat, n_flat, loc_idx[lo + j]);
      if (v != v) continue;  // NaN (an index outside flat reads as one): never in a search
      if (bl_better(v, j, bv, bi)) {
        bv = v;
        bi = j;
      }
    }
    bl_wave_argmax(bv, bi);
    place = bi;
  }
  // a site is a candidate: NO_BUG (the last entry) is none, and so is anything out of range
  int64_t row = -1;
  float logprob = 0.0f;
  if (place >= 0 && place < n - 1) {
    const int32_t f = loc_idx[lo + place];
    if (f >= 0 && (int64_t)f < n_cand && (int64_t)f < n_flat) {
      row = cand_rows[f];
      logprob = flat[f];
    }
  }
  if (row < 0 || row >= n_rows) {
    row = -1;
    place = -1;
    logprob = 0.0f;
  }
  float* out = out_rows + at * (int64_t)D;
  const float* src = row >= 0 ? h + row * ldh : nullptr;
  for (int d = lane; d < D; d += BL_WAVE) out[d] = src ? src[d] : 0.0f;
  if (lane == 0) {
    out_place[at] = place;
    out_logprob[at] = logprob;
  }
}

// ---- bl_sim_quantize ----
__global__ __launch_bounds__(SM_THREADS) void sm_quantize_kernel(const float* x, int64_t ldx, const float* __restrict__ mean,
                                                                 int64_t N, int D, int Dp, float* c, int64_t ldc,  // c may be x
                                                                
                                                                 int8_t* __restrict__ q, double* __restrict__ sumsq, double* __restrict__ r) {
  const int lane = threadIdx.x % BL_WAVE;
  const int64_t n = (int64_t)blockIdx.x * SM_WAVES + threadIdx.x / BL_WAVE;
  if (n >= N) return;  // the whole wave leaves
  const float* xr = x + n * ldx;
  float* cr = c + n * ldc;
  // this lane's columns: the quads lane and lane + 64 (D <= 512), in ascending order -- bl_lane_dot_f64's ownership, with the
  // partial quad's columns loaded one by one like every other (the loads differ, the order of the additions does not)
  float cv[2][4];
  double acc = 0.0;
  float amax = 0.0f;
  bool finite = true;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = 4 * (lane + p * BL_WAVE) + j;
      float v = 0.0f;
      if (d < D) {
        v = (float)((double)xr[d] - (double)mean[d]);
        cr[d] = v;  // in place is allowed: column d is read and written by this thread alone
        const float a = __builtin_fabsf(v);
        finite = finite && a < __builtin_huge_valf();  // false for an infinity and for NaN
        amax = a > amax ? a : amax;                      // (a NaN never gets in: the row is invalid anyway)
        acc += (double)v * (double)v;
      }
      cv[p][j] = v;
    }
  }
  acc = bl_wave_sum_f64(acc);
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const float other = __shfl_xor(amax, o, BL_WAVE);
    amax = other > amax ? other : amax;
  }
  const bool valid = __all(finite) && amax > 0.0f;
  const double scale = valid ? 127.0 / (double)amax : 0.0;
  int32_t* qr = reinterpret_cast<int32_t*>(q + n * (int64_t)Dp);  // 4-byte aligned: the base is 16-byte aligned, Dp a multiple of 64
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int quad = lane + p * BL_WAVE;
    if (4 * quad >= Dp) continue;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = valid ? (int)__builtin_rint((double)cv[p][j] * scale) : 0;  // half to even; |v| <= 127
      word |= (uint32_t)(v & 0xFF) << (8 * j);
    }
    qr[quad] = (int32_t)word;
  }
  if (lane == 0) {
    sumsq[n] = valid ? acc : 0.0;
    r[n] = valid ? ((double)amax * (double)amax) / acc : 0.0;
  }
}

// ---- bl_sim_search_i8 ----
// rank of entry (k, i) among a list: how many of its entries come strictly before it in bl_better's order (indices are distinct)
__device__ __forceinline__ bool sm_before(double ka, int ia, double kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

__global__ __launch_bounds__(SM_THREADS) void sm_search_kernel(const int8_t* __restrict__ qx, int64_t Q, const int8_t* __restrict__ qy,
                                                               const double* __restrict__ ry, int64_t N, int Dp, int S,
                                                               double* __restrict__ part_key, int32_t* __restrict__ part_idx) {
  __shared__ double s_key[SM_TILE * SM_PER_QUERY];  // 32 KB
  __shared__ int s_idx[SM_TILE * SM_PER_QUERY];     // 16 KB
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int col = lane & 15, group = lane >> 4;
  const int64_t q0 = (int64_t)blockIdx.x * SM_TILE;
  const int s = blockIdx.y;
  const int chunks = Dp / 64;
  const int64_t tiles = (N + SM_TILE - 1) / SM_TILE;
  const int64_t t_begin = tiles * s / S, t_end = tiles * (s + 1) / S;

  // the queries' fragments stay in registers for the whole slice (a query past Q loads the last one; its results are dropped)
  const int64_t qrow = q0 + col < Q ? q0 + col : Q - 1;
  sm_v4i bfrag[SM_MAX_CHUNKS];
#pragma unroll
  for (int kc = 0; kc < SM_MAX_CHUNKS; ++kc)
    bfrag[kc] = kc < chunks ? *reinterpret_cast<const sm_v4i*>(qx + qrow * Dp + kc * 64 + group * 16) : sm_v4i{0, 0, 0, 0};

  double lk[SM_L];
  int li[SM_L];
#pragma unroll
  for (int j = 0; j < SM_L; ++j) {
    lk[j] = 0.0;
    li[j] = -1;
  }
  for (int64_t t = t_begin + wave; t < t_end; t += SM_WAVES) {
    const int64_t base = t * SM_TILE;
    const int64_t arow = base + col < N ? base + col : N - 1;  // a row past N loads the last one; its results are dropped below
    const int8_t* ap = qy + arow * Dp + group * 16;
    sm_v4i acc = {0, 0, 0, 0};
#pragma unroll
    for (int kc = 0; kc < SM_MAX_CHUNKS; ++kc)
      if (kc < chunks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const sm_v4i*>(ap + kc * 64), bfrag[kc], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = base + group * 4 + reg;
      if (row >= N) continue;
      const double ryv = ry[row];
      if (!(ryv > 0.0)) continue;  // an invalid index row is never a candidate
      const int64_t idot = acc[reg];
      const double key = (double)(idot * (idot < 0 ? -idot : idot)) * ryv;  // exact up to 2^53, then one rounded product
      const int idx = (int)row;
      if (!bl_better(key, idx, lk[SM_L - 1], li[SM_L - 1])) continue;
      bool placed = false;
#pragma unroll
      for (int j = SM_L - 1; j > 0; --j) {
        if (placed) continue;
        if (bl_better(key, idx, lk[j - 1], li[j - 1])) {
          lk[j] = lk[j - 1];
          li[j] = li[j - 1];
        } else {
          lk[j] = key;
          li[j] = idx;
          placed = true;
        }
      }
      if (!placed) {
        lk[0] = key;
        li[0] = idx;
      }
    }
  }
  // query `col` of the workgroup: list (wave, group), entry j -> its 256 entries
#pragma unroll
  for (int j = 0; j < SM_L; ++j) {
    const int e = col * SM_PER_QUERY + (wave * 4 + group) * SM_L + j;
    s_key[e] = lk[j];
    s_idx[e] = li[j];
  }
  __syncthreads();
  // thread t ranks entry t of every query in turn; the first SM_L in order are the slice's partial list
  for (int qi = 0; qi < SM_TILE; ++qi) {
    if (q0 + qi >= Q) break;  // the same for every thread
    const double* keys = s_key + qi * SM_PER_QUERY;
    const int* idxs = s_idx + qi * SM_PER_QUERY;
    const double mk = keys[tid];
    const int mi = idxs[tid];
    int rank = 0, present = 0;
    for (int e = 0; e < SM_PER_QUERY; ++e) {
      const int oi = idxs[e];
      if (oi < 0) continue;
      ++present;
      if (mi >= 0 && sm_before(keys[e], oi, mk, mi)) ++rank;
    }
    const int64_t out = ((q0 + qi) * S + s) * SM_L;
    if (mi >= 0 && rank < SM_L) {
      part_key[out + rank] = mk;
      part_idx[out + rank] = mi;
    }
    if (tid < SM_L && tid >= present) {
      part_key[out + tid] = 0.0;
      part_idx[out + tid] = -1;
    }
  }
}

__global__ __launch_bounds__(SM_THREADS) void sm_merge_kernel(const double* __restrict__ part_key, const int32_t* __restrict__ part_idx,
                                                              const double* __restrict__ rx, int S, int C, int32_t* __restrict__ out_idx,
                                                              double* __restrict__ out_key) {
  __shared__ double s_key[BL_SIM_MAX_SLICES * SM_L];
  __shared__ int s_idx[BL_SIM_MAX_SLICES * SM_L];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int total = S * SM_L;
  const bool valid = rx[q] > 0.0;  // an invalid query gets no neighbours
  for (int e = tid; e < total; e += SM_THREADS) {
    s_key[e] = part_key[q * total + e];
    s_idx[e] = valid ? part_idx[q * total + e] : -1;
  }
  __syncthreads();
  int present = 0;
  for (int e = 0; e < total; ++e) present += s_idx[e] >= 0;
  for (int m = tid; m < total; m += SM_THREADS) {
    const double mk = s_key[m];
    const int mi = s_idx[m];
    if (mi < 0) continue;
    int rank = 0;
    for (int e = 0; e < total; ++e) {
      const int oi = s_idx[e];
      if (oi >= 0 && sm_before(s_key[e], oi, mk, mi)) ++rank;
    }
    if (rank < C) {
      out_idx[q * C + rank] = mi;
      out_key[q * C + rank] = mk;
    }
  }
  if (tid < C && tid >= present) {
    out_idx[q * C + tid] = -1;
    out_key[q * C + tid] = 0.0;
  }
}

// ---- bl_sim_rescore ----
__global__ __launch_bounds__(SM_THREADS) void sm_rescore_kernel(const float* __restrict__ cx, int64_t ldx, const float* __restrict__ cy,
                                                                int64_t ldy, const double* __restrict__ sumsq_y, int64_t N, int D, int vec,
                                                                const int32_t* __restrict__ cand, int C, int K, int32_t* __restrict__ out_idx,
                                                                double* __restrict__ out_dot) {
  __shared__ double s_key[SM_L];
  __shared__ double s_dot[SM_L];
  __shared__ int s_idx[SM_L];
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int64_t q = blockIdx.x;
  const float* xr = cx + q * ldx;
  for (int c = wave; c < C; c += SM_WAVES) {  // the same candidate in every lane of the wave
    const int32_t i = cand[q * C + c];
    double dot = 0.0, key = 0.0;
    int idx = -1;
    if (i >= 0 && (int64_t)i < N && sumsq_y[i] > 0.0) {  // an invalid index row (sumsq 0) is never a neighbour
      const float* yr = cy + (int64_t)i * ldy;
      dot = bl_wave_sum_f64(vec ? bl_lane_dot_f64<true>(xr, yr, D, lane) : bl_lane_dot_f64<false>(xr, yr, D, lane));
      key = (dot * __builtin_fabs(dot)) / sumsq_y[i];  // one rounded product, one rounded quotient
      if (key == key) idx = i;                         // NaN (an invalid query): never in a search
    }
    if (lane == 0) {
      s_key[c] = key;
      s_dot[c] = dot;
      s_idx[c] = idx;
    }
  }
  __syncthreads();
  int present = 0;
  for (int e = 0; e < C; ++e) present += s_idx[e] >= 0;
  if (tid < C && s_idx[tid] >= 0) {
    const double mk = s_key[tid];
    const int mi = s_idx[tid];
    int rank = 0;
    for (int e = 0; e < C; ++e) {
      const int oi = s_idx[e];
      if (oi < 0) continue;
      // (key2, index), then the place in the list: a total order even where a caller lists a row twice
      if (sm_before(s_key[e], oi, mk, mi) || (s_key[e] == mk && oi == mi && e < tid)) ++rank;
    }
    if (rank < K) {
      out_idx[q * K + rank] = mi;
      out_dot[q * K + rank] = s_dot[tid];
    }
  }
  if (tid < K && tid >= present) {
    out_idx[q * K + tid] = -1;
    out_dot[q * K + tid] = 0.0;
  }
}

inline bool sm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int bl_sim_embed_sites(const float* flat, int64_t n_flat, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                                  int32_t B, const int32_t* cand_rows, int64_t n_cand, const float* h, int64_t ldh, int64_t n_rows,
                                  int32_t D, const int32_t* truth, int32_t skip_nobug, int32_t mode, float* out_rows, int32_t* out_place,
                                  float* out_logprob, int64_t offset, int64_t capacity, void* stream) {
  BL_CHECK_ARG(B >= 0 && n_flat >= 0 && total_loc >= 0 && n_cand >= 0 && n_rows >= 0,
               "bl_sim_embed_sites: negative size (B %d, n_flat %lld, total_loc %lld, n_cand %lld, n_rows %lld)", (int)B, (long long)n_flat,
               (long long)total_loc, (long long)n_cand, (long long)n_rows);
  BL_CHECK_ARG(D >= 1 && ldh >= D, "bl_sim_embed_sites: need D >= 1 and a row stride of at least D (got D %d, ldh %lld)", (int)D,
               (long long)ldh);
  BL_CHECK_RANGE(D <= BL_SIM_MAX_D, "bl_sim_embed_sites: D = %d is above BL_SIM_MAX_D = %d", (int)D, BL_SIM_MAX_D);
  BL_CHECK_ARG(mode == BL_SIM_SITE_PREDICTED || mode == BL_SIM_SITE_TRUTH, "bl_sim_embed_sites: unknown mode %d", (int)mode);
  BL_CHECK_RANGE(bl_fits_int32(n_flat) && bl_fits_int32(total_loc) && bl_fits_int32(n_rows),
                 "bl_sim_embed_sites: index space beyond int32 (n_flat %lld, total_loc %lld, n_rows %lld)", (long long)n_flat,
                 (long long)total_loc, (long long)n_rows);
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)B <= capacity - offset,
               "bl_sim_embed_sites: samples %lld .. %lld do not fit the result buffers of %lld samples", (long long)offset,
               (long long)offset + (long long)B, (long long)capacity);
  BL_CHECK_ARG(B == 0 || (loc_off && out_rows && out_place && out_logprob), "bl_sim_embed_sites: null loc_off / out_rows / out_place / out_logprob");
  BL_CHECK_ARG(B == 0 || mode != BL_SIM_SITE_TRUTH || truth, "bl_sim_embed_sites: null truth in truth mode");
  BL_CHECK_ARG(B == 0 || ((total_loc == 0 || loc_idx) && (n_flat == 0 || flat) && (n_cand == 0 || cand_rows) && (n_rows == 0 || h)),
               "bl_sim_embed_sites: null loc_idx / flat / cand_rows / h with entries to read");
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(sm_embed_kernel, dim3((B + SM_WAVES - 1) / SM_WAVES), dim3(SM_THREADS), 0, (hipStream_t)stream, flat, n_flat, loc_idx,
                     loc_off, total_loc, (int)B, cand_rows, n_cand, h, ldh, n_rows, (int)D, truth, (int)(skip_nobug != 0), (int)mode, out_rows,
                     out_place, out_logprob, offset);
  BL_LAUNCH_CHECK("bl_sim_embed_sites");
  return BL_OK;
}

extern "C" int bl_sim_quantize(const float* x, int64_t ldx, const float* mean, int64_t N, int32_t D, float* c, int64_t ldc, int8_t* q,
                               double* sumsq, double* r, void* stream) {
  BL_CHECK_ARG(N >= 0 && D >= 1, "bl_sim_quantize: need N >= 0 and D >= 1 (got N %lld, D %d)", (long long)N, (int)D);
  BL_CHECK_RANGE(D <= BL_SIM_MAX_D, "bl_sim_quantize: D = %d is above BL_SIM_MAX_D = %d", (int)D, BL_SIM_MAX_D);
  BL_CHECK_ARG(ldx >= D && ldc >= D, "bl_sim_quantize: row strides %lld / %lld are below D = %d", (long long)ldx, (long long)ldc, (int)D);
  BL_CHECK_RANGE(bl_fits_int32(N), "bl_sim_quantize: N = %lld is beyond int32", (long long)N);
  BL_CHECK_ARG(mean != nullptr, "bl_sim_quantize: null mean");
  BL_CHECK_ARG(N == 0 || (x && c && q && sumsq && r), "bl_sim_quantize: null x / c / q / sumsq / r");
  BL_CHECK_ARG(N == 0 || sm_aligned16(q), "bl_sim_quantize: the int8 image must be 16-byte aligned");
  if (N == 0) return BL_OK;
  const int Dp = (D + 63) / 64 * 64;
  hipLaunchKernelGGL(sm_quantize_kernel, dim3((unsigned)((N + SM_WAVES - 1) / SM_WAVES)), dim3(SM_THREADS), 0, (hipStream_t)stream, x, ldx,
                     mean, N, (int)D, Dp, c, ldc, q, sumsq, r);
  BL_LAUNCH_CHECK("bl_sim_quantize");
  return BL_OK;
}

extern "C" int64_t bl_sim_search_workspace_bytes(int64_t Q, int32_t slices) {
  if (Q < 0 || slices < 1 || slices > BL_SIM_MAX_SLICES) return 0;
  return Q * (int64_t)slices * SM_L * 12;  // the keys (fp64), then the indices (int32)
}

extern "C" int bl_sim_search_i8(const int8_t* qx, const double* rx, int64_t Q, const int8_t* qy, const double* ry, int64_t N, int32_t Dp,
                                int32_t C, int32_t slices, void* workspace, int64_t workspace_bytes, int32_t* out_idx, double* out_key,
                                void* stream) {
  BL_CHECK_ARG(Q >= 0 && N >= 0, "bl_sim_search_i8: negative size (Q %lld, N %lld)", (long long)Q, (long long)N);
  BL_CHECK_ARG(Dp >= 64 && Dp % 64 == 0, "bl_sim_search_i8: Dp = %d must be a positive multiple of 64", (int)Dp);
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, "bl_sim_search_i8: Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);
  BL_CHECK_ARG(C >= 1 && C <= BL_SIM_MAX_CANDIDATES, "bl_sim_search_i8: C = %d must be in [1, %d]", (int)C, BL_SIM_MAX_CANDIDATES);
  BL_CHECK_ARG(slices >= 1 && slices <= BL_SIM_MAX_SLICES, "bl_sim_search_i8: slices = %d must be in [1, %d]", (int)slices, BL_SIM_MAX_SLICES);
  BL_CHECK_RANGE(bl_fits_int32(N) && Q <= (int64_t)65535 * SM_TILE, "bl_sim_search_i8: N = %lld is beyond int32 or Q = %lld beyond %lld",
                 (long long)N, (long long)Q, (long long)65535 * SM_TILE);
  BL_CHECK_ARG(Q == 0 || (qx && rx && out_idx && out_key), "bl_sim_search_i8: null qx / rx / out_idx / out_key");
  BL_CHECK_ARG(Q == 0 || N == 0 || (qy && ry), "bl_sim_search_i8: null qy / ry with %lld index rows", (long long)N);
  BL_CHECK_ARG(Q == 0 || (sm_aligned16(qx) && sm_aligned16(qy)), "bl_sim_search_i8: the int8 images must be 16-byte aligned");
  const int64_t need = bl_sim_search_workspace_bytes(Q, slices);
  BL_CHECK_ARG(Q == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "bl_sim_search_i8: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need,
               (long long)workspace_bytes);
  if (Q == 0) return BL_OK;
  hipStream_t st = (hipStream_t)stream;
  double* part_key = (double*)workspace;
  int32_t* part_idx = (int32_t*)((char*)workspace + Q * (int64_t)slices * SM_L * 8);
  if (N == 0) {  // nothing to search: every partial list is empty
    const hipError_t e = hipMemsetAsync(part_idx, 0xFF, sizeof(int32_t) * (size_t)(Q * slices * SM_L), st);
    if (e != hipSuccess) {
      bl_set_error("bl_sim_search_i8: memset failed: %s", hipGetErrorString(e));
      return (int)e;
    }
  } else {
    hipLaunchKernelGGL(sm_search_kernel, dim3((unsigned)((Q + SM_TILE - 1) / SM_TILE), (unsigned)slices), dim3(SM_THREADS), 0, st, qx, Q, qy, ry,
                       N, (int)Dp, (int)slices, part_key, part_idx);
    BL_LAUNCH_CHECK("bl_sim_search_i8 (search)");
  }
  hipLaunchKernelGGL(sm_merge_kernel, dim3((unsigned)Q), dim3(SM_THREADS), 0, st, part_key, part_idx, rx, (int)slices, (int)C, out_idx, out_key);
  BL_LAUNCH_CHECK("bl_sim_search_i8 (merge)");
  return BL_OK;
}

extern "C" int bl_sim_rescore(const float* cx, int64_t ldx, int64_t Q, const float* cy, int64_t ldy, const double* sumsq_y, int64_t N,
                              int32_t D, const int32_t* cand, int32_t C, int32_t k, int32_t* out_idx, double* out_dot, void* stream) {
  BL_CHECK_ARG(Q >= 0 && N >= 0 && D >= 1, "bl_sim_rescore: need Q >= 0, N >= 0 and D >= 1 (got Q %lld, N %lld, D %d)", (long long)Q,
               (long long)N, (int)D);
  BL_CHECK_RANGE(D <= BL_SIM_MAX_D, "bl_sim_rescore: D = %d is above BL_SIM_MAX_D = %d", (int)D, BL_SIM_MAX_D);
  BL_CHECK_ARG(C >= 1 && C <= BL_SIM_MAX_CANDIDATES, "bl_sim_rescore: C = %d must be in [1, %d]", (int)C, BL_SIM_MAX_CANDIDATES);
  BL_CHECK_ARG(k >= 1 && k <= C, "bl_sim_rescore: k = %d must be in [1, C = %d]", (int)k, (int)C);
  BL_CHECK_ARG(ldx >= D && ldy >= D, "bl_sim_rescore: row strides %lld / %lld are below D = %d", (long long)ldx, (long long)ldy, (int)D);
  BL_CHECK_RANGE(bl_fits_int32(N) && bl_fits_int32(Q), "bl_sim_rescore: N = %lld or Q = %lld is beyond int32", (long long)N, (long long)Q);
  BL_CHECK_ARG(Q == 0 || (cx && cand && out_idx && out_dot), "bl_sim_rescore: null cx / cand / out_idx / out_dot");
  BL_CHECK_ARG(Q == 0 || N == 0 || (cy && sumsq_y), "bl_sim_rescore: null cy / sumsq_y with %lld index rows", (long long)N);
  if (Q == 0) return BL_OK;
  const auto aligned = [](const float* p, int64_t ld) { return ((uintptr_t)p % 16 == 0) && (ld % 4 == 0); };
  const int vec = aligned(cx, ldx) && (N == 0 || aligned(cy, ldy));
  hipLaunchKernelGGL(sm_rescore_kernel, dim3((unsigned)Q), dim3(SM_THREADS), 0, (hipStream_t)stream, cx, ldx, cy, ldy, sumsq_y, N, (int)D, vec,
                     cand, (int)C, (int)k, out_idx, out_dot);
  BL_LAUNCH_CHECK("bl_sim_rescore");
  return BL_OK;
}
