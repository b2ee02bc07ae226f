// Warning triage: the Newton statistics and the scores of a ridge-regularised logistic re-ranker on the bug-site embeddings
// (buglab/models/triage.py; the NumPy twin and the Newton driver are buglab/models/_triage.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h ("Warning triage"); in short, with
// P = D + 2 and, for row n, phi_nc = ((double)x_nc - shift_c) * scale_c for c < D, phi_nD = ((double)logprob_n - shift_D) * scale_D,
// phi_n,D+1 = 1:
//   margin   z_n = sum_c w_c phi_nc: lane l owns the column quads q with q % 64 == l (bl_lane_dot_f64.h's ownership), adds the
//            rounded products in ascending column order to a sum that starts at +0.0; then bl_wave_sum_f64.  The twin restates it:
//            margins are equal bit for bit.
//   row      e = exp(-|z|); (p, 1 - p) = (1, e) / (1 + e) for z >= 0, (e, 1) / (1 + e) otherwise; s = c (p (1 - p));
//            r = y ? -(c (1 - p)) : c p; loss = c (softplus(z) - y z) = c (max(u, 0) + log1p(e)), u = y ? -z : z.  No overflow
//            and no cancellation at any z.
//   H, g, L  H = sum_n (s_n phi_n) phi_n^T + lambda I~, g = sum_n r_n phi_n + lambda w~, L = sum_n loss_n + (lambda / 2) |w~|^2; the
//            tilde leaves the intercept (column D + 1) out.  A row with a non-finite x or logprob is in no sum and is counted.
// fp64 throughout, compiled without fused multiply-adds, fixed summation trees, no atomics: the same bits on every run.
//
// bl_triage_newton_stats is four launches on the caller's stream:
//   tr_rows_kernel    one wave per row, 64 rows per workgroup: z, then s (-1 marks a skipped row) and r to the workspace; the
//                     workgroup's partial (loss, c, used, skipped) through bl_block_sum_f64.
//   tr_gram_kernel    workgroup (g, slice): g is a 4 x 4 block of 16 x 16 tiles on or below the diagonal; each of its 4 waves
//                     owns a 2 x 2 sub-block in registers (tiles above the diagonal are left out) and walks the slice's rows four
//                     at a time through v_mfma_f64_16x16x4_f64: A = s phi of the tile's rows, B = phi of its columns.  The
//                     operands come straight from global memory, widened and standardised in registers: one 4-byte load
//                     and two or three fp64 VALU operations per MFMA, and the fp64 MFMA is the slowest matrix instruction, so
//                     there is nothing for LDS to save; with no LDS and 86 VGPRs five waves share a SIMD, which is what hides
//                     the load latency (DESIGN.md has the measurements).
//   tr_grad_kernel    workgroup (64 columns, slice): thread (column, k) adds r_n phi_nc over the rows n = begin + k, + 4, ...; the
//                     four k are added in order.
//   tr_finish_kernel  adds the slices' partials in slice order, mirrors the lower triangle (the diagonal tiles' own upper halves
//                     included, so H == H^T bit for bit), adds the ridge, and reduces the workgroups' scalars with
//                     bl_tree_sum_f64.
// OPERAND and C/D MAPS of v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one fp64
// each; accumulator register `reg` of lane l is C[row = (l >> 4) + 4 reg][col = l & 15] -- NOT the fp32 forms' row rule.
//
// SLICES: S = min(64, max(1, ceil(N / 128))), rows per slice = ceil(N / S) rounded up to a multiple of 4 (a k-step never
// straddles two slices); a function of N alone.  No slice is empty, and an empty one would write zeros.
#include "bl_common.h"
#include "bl_segment_f64.h"

#pragma clang fp contract(off)

namespace {
constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / BL_WAVE;
constexpr int TR_ROWS_PER_BLOCK = 64;  // tr_rows_kernel / tr_score_kernel: 16 rows per wave
constexpr int TR_TILE = 16;
constexpr int TR_BLOCK_TILES = 4;  // a workgroup's block of tiles is 4 x 4, a wave's 2 x 2
constexpr int TR_SLICE_ROWS = 128;
constexpr int TR_GRAD_COLS = 64;

typedef double tr_v4d __attribute__((ext_vector_type(4)));

struct TrLayout {  // the workspace, in doubles
  int64_t s, r, part, gpart, hpart, total;
  int64_t row_blocks, tiles, ntiles, slice_rows;
  int slices, P, Pp;
};

inline TrLayout tr_layout(int64_t N, int D) {
  TrLayout L;
  L.P = D + 2;
  L.tiles = (L.P + TR_TILE - 1) / TR_TILE;
  L.Pp = (int)L.tiles * TR_TILE;
  L.ntiles = L.tiles * (L.tiles + 1) / 2;
  int64_t S = (N + TR_SLICE_ROWS - 1) / TR_SLICE_ROWS;
  S = S < 1 ? 1 : (S > BL_TRIAGE_MAX_SLICES ? BL_TRIAGE_MAX_SLICES : S);
  L.slices = (int)S;
  L.slice_rows = ((N + S - 1) / S + 3) / 4 * 4;
  L.row_blocks = (N + TR_ROWS_PER_BLOCK - 1) / TR_ROWS_PER_BLOCK;
  L.s = 0;
  L.r = L.s + N;
  L.part = L.r + N;
  L.gpart = L.part + 4 * L.row_blocks;
  L.hpart = L.gpart + S * L.Pp;
  L.total = L.hpart + S * L.ntiles * (TR_TILE * TR_TILE);
  return L;
}

struct TrRows {  // the operands that describe the rows
  const float* x;
  int64_t ldx;
  const float* logprob;
  const double* shift;
  const double* scale;
  int D;
};

// ---- the margin of one row, one wave: every lane returns z; `finite` is false where an entry of x or logprob is not ----
template <bool VEC>
__device__ __forceinline__ double tr_margin(const TrRows& R, const double* __restrict__ w, int64_t n, int lane, bool& finite) {
  const float* xr = R.x + n * R.ldx;
  const int D = R.D, P = D + 2;
  const float lp = R.logprob[n];
  bool ok = true;
  double acc = 0.0;
  const int full = P / 4;
  for (int q = lane; q <= full; q += BL_WAVE) {  // q == full: the last, partial quad (empty when P % 4 == 0)
    const int c0 = 4 * q;
    float v[4];
    if (VEC && c0 + 4 <= D) {
      const float4 a = *reinterpret_cast<const float4*>(xr + c0);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < D ? xr[c0 + j] : (c0 + j == D ? lp : 1.0f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      if (c < P) {
        ok = ok && __builtin_isfinite(v[j]);
        const double phi = c <= D ? ((double)v[j] - R.shift[c]) * R.scale[c] : 1.0;
        acc += w[c] * phi;
      }
    }
  }
  finite = __all(ok);
  return bl_wave_sum_f64(acc);
}

// p and 1 - p of a margin, and log1p(exp(-|z|)); exact 0 / 1 far out, never NaN for a finite z
__device__ __forceinline__ void tr_logistic(double z, double& p, double& q, double& tail) {
  const double e = exp(-fabs(z));
  const double d = 1.0 + e;
  const double big = 1.0 / d, small = e / d;
  p = z >= 0.0 ? big : small;
  q = z >= 0.0 ? small : big;
  tail = log1p(e);  // softplus(u) = max(u, 0) + tail for u = z and for u = -z
}

template <bool VEC>
__global__ __launch_bounds__(TR_THREADS) void tr_rows_kernel(TrRows R, const double* __restrict__ w, const uint8_t* __restrict__ y,
                                                             const double* __restrict__ c, int64_t N, double* __restrict__ ws_s,
                                                             double* __restrict__ ws_r, double* __restrict__ part) {
  __shared__ double s_red[TR_WAVES];
  const int lane = threadIdx.x % BL_WAVE, wave = threadIdx.x / BL_WAVE;
  const int64_t base = (int64_t)blockIdx.x * TR_ROWS_PER_BLOCK;
  double loss = 0.0, csum = 0.0, used = 0.0, skipped = 0.0;  // lane 0's are the wave's, the other lanes' stay 0
  for (int k = wave; k < TR_ROWS_PER_BLOCK; k += TR_WAVES) {
    const int64_t n = base + k;
    if (n >= N) break;  // the whole wave
    bool finite;
    const double z = tr_margin<VEC>(R, w, n, lane, finite);
    if (lane != 0) continue;
    if (!finite) {
      ws_s[n] = -1.0;
      ws_r[n] = 0.0;
      skipped += 1.0;
      continue;
    }
    double p, q, sp;
    tr_logistic(z, p, q, sp);
    const double cn = c ? c[n] : 1.0;
    const bool yn = y[n] != 0;
    ws_s[n] = cn * (p * q);
    ws_r[n] = yn ? -(cn * q) : cn * p;
    const double u = yn ? -z : z;  // softplus(z) - y z = softplus(u): no difference of two large numbers
    loss += cn * ((u > 0.0 ? u : 0.0) + sp);
    csum += cn;
    used += 1.0;
  }
  loss = bl_block_sum_f64<TR_WAVES>(loss, s_red);
  csum = bl_block_sum_f64<TR_WAVES>(csum, s_red);
  used = bl_block_sum_f64<TR_WAVES>(used, s_red);
  skipped = bl_block_sum_f64<TR_WAVES>(skipped, s_red);
  if (threadIdx.x == 0) {
    double* o = part + 4 * (int64_t)blockIdx.x;
    o[0] = loss, o[1] = csum, o[2] = used, o[3] = skipped;
  }
}

template <bool VEC>
__global__ __launch_bounds__(TR_THREADS) void tr_score_kernel(TrRows R, const double* __restrict__ w, int64_t N,
                                                              double* __restrict__ margin, double* __restrict__ prob) {
  const int lane = threadIdx.x % BL_WAVE, wave = threadIdx.x / BL_WAVE;
  const int64_t base = (int64_t)blockIdx.x * TR_ROWS_PER_BLOCK;
  for (int k = wave; k < TR_ROWS_PER_BLOCK; k += TR_WAVES) {
    const int64_t n = base + k;
    if (n >= N) break;
    bool finite;
    const double z = tr_margin<VEC>(R, w, n, lane, finite);
    if (lane != 0) continue;
    double p = __builtin_nan(""), q, sp;
    if (finite) tr_logistic(z, p, q, sp);
    margin[n] = finite ? z : __builtin_nan("");
    prob[n] = p;
  }
}

// ---- one column of phi as a lane sees it: where its value comes from, and its shift and scale ----
struct TrColumn {
  int kind;  // 0: x[c], 1: logprob, 2: the constant 1, 3: padding (0)
  int c;
  double shift, scale;
};
__device__ __forceinline__ TrColumn tr_column(const TrRows& R, int c) {
  TrColumn col;
  col.c = c;
  col.kind = c < R.D ? 0 : (c == R.D ? 1 : (c == R.D + 1 ? 2 : 3));
  col.shift = c <= R.D ? R.shift[c] : 0.0;
  col.scale = c <= R.D ? R.scale[c] : (c == R.D + 1 ? 1.0 : 0.0);
  return col;
}
// `live`: the row exists and was not skipped (its x may hold NaN otherwise, which a product with 0 would keep)
__device__ __forceinline__ double tr_phi(const TrColumn& col, const float* __restrict__ xr, float lp, bool live) {
  float v = 0.0f;
  if (live) v = col.kind == 0 ? xr[col.c] : (col.kind == 1 ? lp : (col.kind == 2 ? 1.0f : 0.0f));
  return ((double)v - col.shift) * col.scale;  // padding: (0 - 0) * 0; a dead row: finite, and its s is 0
}

__global__ __launch_bounds__(TR_THREADS) void tr_gram_kernel(TrRows R, int64_t N, int64_t slice_rows, int tiles, int64_t ntiles,
                                                             const double* __restrict__ ws_s, double* __restrict__ hpart) {
  const int lane = threadIdx.x % BL_WAVE, wave = threadIdx.x / BL_WAVE;
  const int col = lane & 15, krow = lane >> 4;
  // block (bi, bj), bj <= bi, from the linear index g = bi (bi + 1) / 2 + bj
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  const int ti0 = bi * TR_BLOCK_TILES + 2 * (wave >> 1), tj0 = bj * TR_BLOCK_TILES + 2 * (wave & 1);
  bool want[2][2];
  bool any = false;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      want[a][b] = ti0 + a < tiles && tj0 + b <= ti0 + a;  // on or below the diagonal (tj < tiles follows)
      any = any || want[a][b];
    }
  if (!any) return;  // the whole wave; no barrier below

  TrColumn ci[2], cj[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    ci[a] = tr_column(R, (ti0 + a) * TR_TILE + col);
    cj[a] = tr_column(R, (tj0 + a) * TR_TILE + col);
  }
  tr_v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = tr_v4d{0.0, 0.0, 0.0, 0.0};

  const int64_t begin = (int64_t)blockIdx.y * slice_rows;
  const int64_t end = begin + slice_rows < N ? begin + slice_rows : N;
  for (int64_t n0 = begin; n0 < end; n0 += 4) {
    const int64_t n = n0 + krow;
    double s = 0.0;
    bool live = false;
    if (n < end) {
      s = ws_s[n];
      live = s >= 0.0;
      if (!live) s = 0.0;
    }
    const float* xr = R.x + (live ? n : 0) * R.ldx;
    const float lp = live ? R.logprob[n] : 0.0f;
    double fa[2], fb[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      fa[a] = s * tr_phi(ci[a], xr, lp, live);
      fb[a] = tr_phi(cj[a], xr, lp, live);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if (want[a][b]) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (want[a][b]) {
        const int64_t ti = ti0 + a, tj = tj0 + b;
        double* o = hpart + ((int64_t)blockIdx.y * ntiles + ti * (ti + 1) / 2 + tj) * (TR_TILE * TR_TILE);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o[(krow + 4 * reg) * TR_TILE + col] = acc[a][b][reg];
      }
}

__global__ __launch_bounds__(TR_THREADS) void tr_grad_kernel(TrRows R, int64_t N, int64_t slice_rows, int Pp,
                                                             const double* __restrict__ ws_s, const double* __restrict__ ws_r,
                                                             double* __restrict__ gpart) {
  __shared__ double s_g[TR_WAVES][TR_GRAD_COLS];
  const int cl = threadIdx.x % TR_GRAD_COLS, k = threadIdx.x / TR_GRAD_COLS;
  const int c = (int)blockIdx.x * TR_GRAD_COLS + cl;  // < Pp: the grid covers Pp rounded up, the padding columns give 0
  const TrColumn colm = tr_column(R, c);
  const int64_t begin = (int64_t)blockIdx.y * slice_rows;
  const int64_t end = begin + slice_rows < N ? begin + slice_rows : N;
  double acc = 0.0;
  for (int64_t n = begin + k; n < end; n += TR_WAVES) {
    const bool live = ws_s[n] >= 0.0;
    if (!live) continue;  // the same for the whole wave
    acc += ws_r[n] * tr_phi(colm, R.x + n * R.ldx, R.logprob[n], true);
  }
  s_g[k][cl] = acc;
  __syncthreads();
  if (k == 0 && c < Pp) {
    double t = s_g[0][cl];
#pragma unroll
    for (int j = 1; j < TR_WAVES; ++j) t += s_g[j][cl];
    gpart[(int64_t)blockIdx.y * Pp + c] = t;
  }
}

// blocks 0 .. ntiles - 1: one tile of H each; then ceil(P / 256) blocks of g; the last block: the four scalars
__global__ __launch_bounds__(TR_THREADS) void tr_finish_kernel(int P, int Pp, int tiles, int64_t ntiles, int slices, int64_t row_blocks,
                                                               double lambda, const double* __restrict__ w,
                                                               const double* __restrict__ hpart, const double* __restrict__ gpart,
                                                               const double* __restrict__ part, double* __restrict__ H,
                                                               double* __restrict__ g, double* __restrict__ scalars) {
  __shared__ double s_acc[TR_THREADS];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int gblocks = (P + TR_THREADS - 1) / TR_THREADS;
  if (b < ntiles) {
    int ti = 0;
    while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
    const int tj = (int)(b - (int64_t)ti * (ti + 1) / 2);
    double acc = 0.0;
    for (int s = 0; s < slices; ++s) acc += hpart[((int64_t)s * ntiles + b) * (TR_TILE * TR_TILE) + tid];
    const int row = ti * TR_TILE + tid / TR_TILE, col = tj * TR_TILE + tid % TR_TILE;
    if (row < P && col <= row) {
      if (row == col && row != P - 1) acc += lambda;
      H[(int64_t)row * P + col] = acc;
      H[(int64_t)col * P + row] = acc;
    }
  } else if (b < ntiles + gblocks) {
    const int c = (int)(b - ntiles) * TR_THREADS + tid;
    if (c < P) {
      double acc = 0.0;
      for (int s = 0; s < slices; ++s) acc += gpart[(int64_t)s * Pp + c];
      if (c != P - 1) acc += lambda * w[c];
      g[c] = acc;
    }
  } else {
    double out[4];
    for (int f = 0; f < 4; ++f) {
      double acc = 0.0;
      for (int64_t i = tid; i < row_blocks; i += TR_THREADS) acc += part[4 * i + f];
      bl_tree_sum_f64<TR_THREADS>(acc, s_acc);
      out[f] = s_acc[0];
      __syncthreads();  // s_acc[0] has been read before the next round writes it
    }
    double ww = 0.0;
    for (int c = tid; c < P - 1; c += TR_THREADS) ww += w[c] * w[c];
    bl_tree_sum_f64<TR_THREADS>(ww, s_acc);
    if (tid == 0) {
      scalars[0] = out[0] + (0.5 * lambda) * s_acc[0];
      scalars[1] = out[1], scalars[2] = out[2], scalars[3] = out[3];
    }
  }
}

inline bool tr_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the checks the two entry points share; 0 or an error code with the text set
int tr_check_rows(const char* what, const float* x, int64_t ldx, const float* logprob, const double* shift, const double* scale,
                  const double* w, int64_t N, int32_t D) {
  BL_CHECK_ARG(N >= 0 && D >= 1, "%s: need N >= 0 and D >= 1 (got N %lld, D %d)", what, (long long)N, (int)D);
  BL_CHECK_RANGE(D <= BL_TRIAGE_MAX_D, "%s: D = %d is above BL_TRIAGE_MAX_D = %d", what, (int)D, BL_TRIAGE_MAX_D);
  BL_CHECK_RANGE(N <= ((int64_t)1 << 36), "%s: N = %lld is above 2^36 rows", what, (long long)N);
  BL_CHECK_ARG(ldx >= D, "%s: the row stride %lld is below D = %d", what, (long long)ldx, (int)D);
  BL_CHECK_ARG(shift && scale && w, "%s: null shift / scale / w", what);
  BL_CHECK_ARG(tr_aligned(shift, 8) && tr_aligned(scale, 8) && tr_aligned(w, 8), "%s: shift, scale and w must be 8-byte aligned", what);
  BL_CHECK_ARG(N == 0 || (x && logprob), "%s: null x / logprob", what);
  BL_CHECK_ARG(tr_aligned(x, 4) && tr_aligned(logprob, 4), "%s: x and logprob must be 4-byte aligned", what);
  return BL_OK;
}
}  // namespace

extern "C" int64_t bl_triage_workspace_bytes(int64_t N, int32_t D) {
  if (N < 0 || D < 1 || D > BL_TRIAGE_MAX_D || N > ((int64_t)1 << 36)) return -1;
  return tr_layout(N, (int)D).total * (int64_t)sizeof(double);
}

extern "C" int bl_triage_newton_stats(const float* x, int64_t ldx, const float* logprob, const double* shift, const double* scale,
                                      const double* w, const uint8_t* y, const double* c, int64_t N, int32_t D, double lambda,
                                      void* workspace, int64_t workspace_bytes, double* H, double* g, double* scalars, void* stream) {
  const char* what = "bl_triage_newton_stats";
  const int rc = tr_check_rows(what, x, ldx, logprob, shift, scale, w, N, D);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(lambda > 0.0 && lambda < __builtin_huge_val(), "%s: lambda = %g must be positive and finite", what, lambda);
  BL_CHECK_ARG(N == 0 || (H && g && scalars), "%s: null H / g / scalars", what);
  BL_CHECK_ARG(tr_aligned(H, 8) && tr_aligned(g, 8) && tr_aligned(scalars, 8) && tr_aligned(c, 8),
               "%s: H, g, scalars and c must be 8-byte aligned", what);
  BL_CHECK_ARG(N == 0 || y, "%s: null y", what);
  const TrLayout L = tr_layout(N, (int)D);
  const int64_t need = L.total * (int64_t)sizeof(double);
  BL_CHECK_ARG(N == 0 || (workspace && tr_aligned(workspace, 8)), "%s: the workspace is null or not 8-byte aligned", what);
  BL_CHECK_ARG(N == 0 || workspace_bytes >= need, "%s: the workspace has %lld bytes, N = %lld and D = %d need %lld", what,
               (long long)workspace_bytes, (long long)N, (int)D, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int P = L.P;
  if (N == 0) {  // zeros where there is an output, nothing launched
    if ((H && hipMemsetAsync(H, 0, sizeof(double) * (size_t)P * P, st) != hipSuccess) ||
        (g && hipMemsetAsync(g, 0, sizeof(double) * P, st) != hipSuccess) ||
        (scalars && hipMemsetAsync(scalars, 0, sizeof(double) * 4, st) != hipSuccess)) {
      bl_set_error("%s: clearing the outputs failed", what);
      return BL_EINVAL;
    }
    return BL_OK;
  }
  double* ws = static_cast<double*>(workspace);
  const TrRows R{x, ldx, logprob, shift, scale, (int)D};
  const bool vec = bl_aligned16(x) && ldx % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(tr_rows_kernel<true>, dim3((unsigned)L.row_blocks), dim3(TR_THREADS), 0, st, R, w, y, c, N, ws + L.s, ws + L.r,
                       ws + L.part);
  else
    hipLaunchKernelGGL(tr_rows_kernel<false>, dim3((unsigned)L.row_blocks), dim3(TR_THREADS), 0, st, R, w, y, c, N, ws + L.s, ws + L.r,
                       ws + L.part);
  BL_LAUNCH_CHECK(what);
  const int nb = ((int)L.tiles + TR_BLOCK_TILES - 1) / TR_BLOCK_TILES;
  hipLaunchKernelGGL(tr_gram_kernel, dim3((unsigned)(nb * (nb + 1) / 2), (unsigned)L.slices), dim3(TR_THREADS), 0, st, R, N, L.slice_rows,
                     (int)L.tiles, L.ntiles, ws + L.s, ws + L.hpart);
  BL_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(tr_grad_kernel, dim3((unsigned)((L.Pp + TR_GRAD_COLS - 1) / TR_GRAD_COLS), (unsigned)L.slices), dim3(TR_THREADS), 0, st, R,
                     N, L.slice_rows, L.Pp, ws + L.s, ws + L.r, ws + L.gpart);
  BL_LAUNCH_CHECK(what);
  const unsigned fin = (unsigned)(L.ntiles + (P + TR_THREADS - 1) / TR_THREADS + 1);
  hipLaunchKernelGGL(tr_finish_kernel, dim3(fin), dim3(TR_THREADS), 0, st, P, L.Pp, (int)L.tiles, L.ntiles, L.slices, L.row_blocks, lambda, w,
                     ws + L.hpart, ws + L.gpart, ws + L.part, H, g, scalars);
  BL_LAUNCH_CHECK(what);
  return BL_OK;
}

extern "C" int bl_triage_score(const float* x, int64_t ldx, const float* logprob, const double* shift, const double* scale,
                               const double* w, int64_t N, int32_t D, double* margin, double* prob, void* stream) {
  const char* what = "bl_triage_score";
  const int rc = tr_check_rows(what, x, ldx, logprob, shift, scale, w, N, D);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(N == 0 || (margin && prob), "%s: null margin / prob", what);
  BL_CHECK_ARG(tr_aligned(margin, 8) && tr_aligned(prob, 8), "%s: margin and prob must be 8-byte aligned", what);
  if (N == 0) return BL_OK;
  const TrRows R{x, ldx, logprob, shift, scale, (int)D};
  const unsigned blocks = (unsigned)((N + TR_ROWS_PER_BLOCK - 1) / TR_ROWS_PER_BLOCK);
  if (bl_aligned16(x) && ldx % 4 == 0)
    hipLaunchKernelGGL(tr_score_kernel<true>, dim3(blocks), dim3(TR_THREADS), 0, (hipStream_t)stream, R, w, N, margin, prob);
  else
    hipLaunchKernelGGL(tr_score_kernel<false>, dim3(blocks), dim3(TR_THREADS), 0, (hipStream_t)stream, R, w, N, margin, prob);
  BL_LAUNCH_CHECK(what);
  return BL_OK;
}
