// fp32-accurate GEMMs on the fp16 matrix cores ("f16x3"): the message-passing GEMMs' second operand split.
//
// csrc/bl_gemm_x6.hip splits an fp32 operand into THREE bf16 planes and evaluates a product as six bf16 MFMA terms.  fp16 has
// 11 significant bits where bf16 has 8: TWO planes
//      x s = hi + lo (+ r, |r| <= 2^-24 |x s|),    hi = fp16(x s),  lo = fp16(x s - hi)          (s: a power of two, below)
// carry the same 22+ bits, and a product needs three terms
//      a b = (a_h b_h + a_h b_l + a_l b_h) / (s_a s_b)                                   (fp32 accumulate; a_l b_l < 2^-22 |ab| dropped)
// -- half the matrix-pipe work of bf16x6 and 4 instead of 6 bytes per packed element (the row GEMMs are co-limited by the
// delivery of the gathered operand).  Timing proxy before it was built (two planes / three terms of the
// bf16 kernels, results wrong; profiles/r06e_planes2_proxy.log): message GEMM 0.257 -> 0.167 ms, routed input-gradient GEMM
// 0.336 -> 0.242, weight gradient (128 x 128 tile) 0.234 -> 0.160 at the c2 layer shape.
//
// What fp16 does not have is bf16's exponent range (5 bits: 6e-8 ... 65504), so every packed tensor carries a power-of-two
// scale s that puts it into the upper part of the range, where BOTH planes are normal numbers:
//   * values with |x s| >= 2^-3 keep 22 bits (relative error 2^-24: fp32's own rounding unit);
//   * below that, lo becomes subnormal and the error is ABSOLUTE: <= 2^-25 / s.  With |x s| <= 2^15 that floor is 2^-40 of the
//     tensor's largest representable magnitude -- eight decades below fp32's relative precision at the top of the range.
//   * |x s| > 65504 saturates (finite values never become inf; +-inf and NaN propagate as NaN like in the bf16 split).
// Scales: layer inputs (tanh x dropout outputs, |h| <= 1.25; embedding rows) 2^8, weights 2^6 (|w| < 512) -- fixed, host-known
// constants of the call; gradient tensors have no bound known in advance: their packer takes the tensor's amax from DEVICE
// memory (written by the producing kernel with one atomic max per workgroup) and derives s = 2^(14 - ceil(log2 amax)); the
// consuming GEMM reads the same number and multiplies its result by 1 / (s_a s_b).  Power-of-two scaling commutes with every
// rounding involved, so results do not depend on s as long as nothing saturates or falls below the absolute floor.
// Error against fp64 on c2-like operands (emulation, tools/experiments/README.md "f16x3"): rms 2.4e-8 where a plain fp32
// matmul has 1.0e-7 and bf16x6 2.2e-9 -- below fp32 accumulation noise; parity tests keep their 1e-4 bound.
//
// Kernel shapes are bl_gemm_x6.hip's: 128 x 128 tile, 4 waves 2 x 2, 32 k's per LDS stage with a register prefetch, swapped MFMA
// operands (transposed accumulators), LDS-staged epilogue, XCD-aware work order (bl_x6_locate.h).  LDS stage row:
// [plane (2)][k-group slot (4)] x 16 B + 16 B of padding = 144 B (36 r mod 64 walks all sixteen 4-bank groups over 16 rows:
// fragment reads conflict-free).
#include <stdio.h>
#include <stdlib.h>

#include "bl_common.h"
#include "bl_gemm_host.h"
#include "bl_gemm_split.h"
#include "bl_x6_locate.h"
#include "bl_h3_image.h"

// ---- packing ------------------------------------------------------------------------------------
// rows: out[r][plane][kg][j] = plane(x[r, 8 kg + j] * scale), planes back to back (row = 2 D halves)
// (kg_total, kg_off) as in pack_rows_kernel: a ConcatResidual pair is packed without a concatenated copy
// LIST (bl_pack_f16x2_rows): the R rows rows[0..R-1] of x, each written at its own row of the whole-layout `out`; no other row of
// either is touched (the live forward of a layer: the rows outside the list were never computed)
template <bool LIST>
__global__ __launch_bounds__(256) void pack_rows_h_kernel(const float* __restrict__ x, int ld, long long R, int D, uint4* __restrict__ out,
                                                          int kg_total, int kg_off, float scale, const float* __restrict__ amax_dev,
                                                          unsigned* __restrict__ sat_counter, const int* __restrict__ rows) {
  const int kgs = D >> 3;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R * kgs) return;
  if (amax_dev) scale *= h3_scale_from_amax(*amax_dev);
  const long long r = LIST ? (long long)rows[t / kgs] : t / kgs;
  const int kgn = kg_total;
  const int kg = (int)(t % kgs) + kg_off;
  x -= 8 * kg_off;
  const float4 a = *reinterpret_cast<const float4*>(x + r * ld + 8 * kg);
  const float4 b = *reinterpret_cast<const float4*>(x + r * ld + 8 * kg + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint16_t h[8], l[8];
  bool sat = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) split2h(v[j] * scale, h[j], l[j], sat);
  if (sat && sat_counter) atomicAdd(sat_counter, 1u);  // (rare by construction: the scales leave 2^6 - 2^8 of headroom)
  uint4* o = out + r * 2 * kgn + kg;
  o[0] = make_uint4(PK(h[0], h[1]), PK(h[2], h[3]), PK(h[4], h[5]), PK(h[6], h[7]));
  o[kgn] = make_uint4(PK(l[0], l[1]), PK(l[2], l[3]), PK(l[4], l[5]), PK(l[6], l[7]));
}

__global__ __launch_bounds__(256) void pack_weights_h_kernel(const float* __restrict__ w, int G, int K, int N, int w_is_kn,
                                                             uint4* __restrict__ out, float scale, unsigned* __restrict__ sat_counter) {
  pack_weights_h_thread(w, G, K, N, w_is_kn, out, (long long)blockIdx.x * blockDim.x + threadIdx.x, scale, sat_counter);
}

// ---- row GEMM --------------------------------------------------------------------------------------
// gemm_rows_body (bl_gemm_split.h) on the two-plane fp16 split, epilogue-free: C[rows of g] = out_scale * rows(a) . B_g with
// out_scale = 1 / (s_a s_b) (host part) x the reciprocal of h3_scale_from_amax(*a_amax_dev) when the left operand's scale lives in
// device memory.  ONE (bl_set_msg_gemm_mode(2), `train.py --amp`): one fp16 MFMA term with fp32 accumulation, what
// torch.cuda.amp.autocast makes of a Linear.
template <bool MASKED, bool ONE>
__global__ __launch_bounds__(256, MASKED ? 2 : 3) void gemm_rows_h3_kernel(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint32_t* __restrict__ win_bits, int ld_bits, const uint4* __restrict__ bp,
    long long strideB, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G, int M, int N, int K,
    float* __restrict__ c, int ldc, int xcd_remap, float out_scale, const float* __restrict__ a_amax_dev) {
  gemm_rows_body<SplitF16x2, MASKED, -1, ONE>(xp0, xp1, xp2, idx0, idx1, idx2, w0, w1, w2, koff1, koff2, nsrc, win_bits, ld_bits, bp,
                                              strideB, group_ptr, group_w, G, M, N, K, c, ldc, xcd_remap, X6Epi{}, out_scale, a_amax_dev);
}

// ---- weight-gradient GEMM (128 x 128 tile) ---------------------------------------------------------
// gemm_wgrad_body (bl_gemm_split.h) on the two-plane fp16 split: gW_g[i, n] += out_scale * sum_{e in group g} A[e, i] * Gr[e, n]
template <bool ROUTED, bool ONE>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_h3_kernel(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint4* __restrict__ gp, const int* __restrict__ g_idx,
    const uint32_t* __restrict__ win_bits, int ld_bits, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G,
    int M, int N, int K, int kchunk, float* __restrict__ gw_base, long long strideW, int ldw, int ntiles_n, int xcd_remap,
    unsigned* __restrict__ order_ctr, float out_scale, const float* __restrict__ g_amax_dev) {
  gemm_wgrad_body<SplitF16x2, ROUTED, ONE>(xp0, xp1, xp2, idx0, idx1, idx2, w0, w1, w2, koff1, koff2, nsrc, gp, g_idx, win_bits, ld_bits,
                                           group_ptr, group_w, G, M, N, K, kchunk, gw_base, strideW, ldw, ntiles_n, xcd_remap, order_ctr,
                                           out_scale, g_amax_dev);
}

// ---- amax of a tensor into device memory (gradient operands) ----------------------------------------
// *amax = max(*amax, max |x|): non-negative floats order like their bit patterns; the caller zeroes *amax first
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long n4, float* __restrict__ amax) {
  __shared__ float part[4];
  float m = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  m = bl_wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  // ONE atomic per workgroup, few workgroups: same-address atomics serialise at the L2 (~40 ns each)
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned int*>(amax), __float_as_uint(m));
  }
}

// ---- saturation events ----------------------------------------------------------------------------------
// One unsigned per device, allocated on first use and never freed (like the ordered-flush ring of bl_core.hip): a packing thread
// that had to clamp a finite value to +-65504 adds 1.  The fixed scales leave 2^6 - 2^8 of headroom over every bounded tensor, so a
// non-zero count means a layer input beyond +-255.9 or a weight beyond +-1023 -- a diverging run, or a model this split does not fit.
unsigned* bl_h3_sat_counter() {
  static unsigned* ctr[BL_MAX_DEVICES] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= BL_MAX_DEVICES) return nullptr;
  if (ctr[dev] == nullptr) {
    if (hipMalloc((void**)&ctr[dev], sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(ctr[dev], 0, sizeof(unsigned)) != hipSuccess) return nullptr;
  }
  return ctr[dev];
}

// number of saturation events on the current device since the last reset (synchronises the device); -1 if unavailable
extern "C" int64_t bl_h3_saturation_events(int32_t reset) {
  unsigned* c = bl_h3_sat_counter();
  unsigned v = 0;
  if (c == nullptr || hipMemcpy(&v, c, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (reset && hipMemset(c, 0, sizeof(unsigned)) != hipSuccess) return -1;
  return (int64_t)v;
}

// ================================================================================================
extern "C" int bl_pack_f16x2(const float* x, int32_t ld, int64_t R, int32_t D, int32_t D_total, int32_t col_off, float scale,
                             const float* amax_dev, uint16_t* out, void* stream) {
  if (R == 0) return BL_OK;
  BL_CHECK_ARG(x && out && bl_aligned16(x) && bl_aligned16(out), "bl_pack_f16x2: null or misaligned pointer");
  BL_CHECK_ARG(D > 0 && D % 8 == 0 && ld % 4 == 0 && D_total % 8 == 0 && col_off % 8 == 0 && col_off >= 0 && col_off + D <= D_total,
               "bl_pack_f16x2: widths / offset must be multiples of 8 with col_off + D <= D_total");
  BL_CHECK_ARG(scale > 0.f, "bl_pack_f16x2: scale must be positive (a power of two)");
  const long long total = (long long)R * (D / 8);
  hipLaunchKernelGGL(pack_rows_h_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld, (long long)R, D,
                     reinterpret_cast<uint4*>(out), D_total / 8, col_off / 8, scale, amax_dev, bl_h3_sat_counter(), nullptr);
  BL_LAUNCH_CHECK("bl_pack_f16x2");
  return BL_OK;
}

// bl_pack_f16x2 for the rows rows[0..R-1] (ids below nrows) of x [nrows, ld] and of out [nrows, 2 D_total]: every other row of
// both stays untouched and unread
extern "C" int bl_pack_f16x2_rows(const float* x, int32_t ld, const int32_t* rows, int32_t R, int32_t D, int32_t D_total, int32_t col_off,
                                  float scale, uint16_t* out, void* stream) {
  if (R == 0) return BL_OK;
  BL_CHECK_ARG(x && out && rows && R > 0 && bl_aligned16(x) && bl_aligned16(out), "bl_pack_f16x2_rows: null or misaligned pointer");
  BL_CHECK_ARG(D > 0 && D % 8 == 0 && ld % 4 == 0 && D_total % 8 == 0 && col_off % 8 == 0 && col_off >= 0 && col_off + D <= D_total,
               "bl_pack_f16x2_rows: widths / offset must be multiples of 8 with col_off + D <= D_total");
  BL_CHECK_ARG(scale > 0.f, "bl_pack_f16x2_rows: scale must be positive (a power of two)");
  const long long total = (long long)R * (D / 8);
  hipLaunchKernelGGL(pack_rows_h_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld, (long long)R, D,
                     reinterpret_cast<uint4*>(out), D_total / 8, col_off / 8, scale, nullptr, bl_h3_sat_counter(), rows);
  BL_LAUNCH_CHECK("bl_pack_f16x2_rows");
  return BL_OK;
}

extern "C" int bl_amax(const float* x, int64_t n, float* amax_dev, void* stream) {
  if (n == 0) return BL_OK;
  BL_CHECK_ARG(x && amax_dev && bl_aligned16(x) && n % 4 == 0, "bl_amax: aligned pointer and a multiple of 4 elements required");
  const long long n4 = n / 4;
  const int grid = (int)((n4 + 255) / 256 < (long long)bl_num_cus() * 2 ? (n4 + 255) / 256 : (long long)bl_num_cus() * 2);
  hipLaunchKernelGGL(amax_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n4, amax_dev);
  BL_LAUNCH_CHECK("bl_amax");
  return BL_OK;
}

extern "C" int64_t bl_packed_weight_elems_h3(int32_t G, int32_t K, int32_t N) { return (int64_t)G * ((N + 127) / 128) * (K / 32) * 8192; }

extern "C" int bl_pack_weights_h3(const float* w, int32_t G, int32_t K, int32_t N, int32_t w_is_kn, float scale, uint16_t* out,
                                  void* stream) {
  if (G == 0) return BL_OK;
  BL_CHECK_ARG(w && out && bl_aligned16(out), "bl_pack_weights_h3: null or misaligned pointer");
  BL_CHECK_ARG(K > 0 && K % 32 == 0 && N > 0 && scale > 0.f, "bl_pack_weights_h3: K must be a multiple of 32 (got %d), scale positive", K);
  const long long total = (long long)G * ((N + 127) / 128) * (K / 32) * 512;
  hipLaunchKernelGGL(pack_weights_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, G, K, N, w_is_kn,
                     reinterpret_cast<uint4*>(out), scale, bl_h3_sat_counter());
  BL_LAUNCH_CHECK("bl_pack_weights_h3");
  return BL_OK;
}

// 1: the f16x3 GEMMs of this file evaluate the high-plane term only (bl_set_msg_gemm_mode(2), `train.py --amp`); see the ONE forms
bool g_h3_one_term = false;

extern "C" int bl_gemm_rows_h3(const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp,
                               int64_t b_group_stride, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N,
                               int32_t K, float out_scale, const float* a_amax_dev, float* c, int32_t ldc, void* stream) {
  const char* who = "bl_gemm_rows_h3";
  if (M == 0) return BL_OK;
  BlPackedRows r;
  dim3 grid;
  if (int rc = bl_rows_gemm_plan(who, a, win_bits, ld_bits, bp, group_ptr, G, M, N, K, c, ldc, XBM, r, grid)) return rc;
  BL_CHECK_ARG(b_group_stride % 8 == 0 && (G <= 1 || b_group_stride >= bl_packed_weight_elems_h3(1, K, N)),
               "%s: packed group stride must cover one group's tiled weights (bl_pack_weights_h3)", who);
  BL_CHECK_ARG(out_scale > 0.f, "%s: out_scale must be positive", who);
#define H3_ARGS                                                                                                               \
  BL_PACKED_ROWS_ARGS(r), win_bits, ld_bits, reinterpret_cast<const uint4*>(bp), (long long)(b_group_stride / 8), group_ptr, \
      group_w, G, M, N, K, c, ldc, 1, out_scale, a_amax_dev
  if (g_h3_one_term) {
    if (win_bits)
      hipLaunchKernelGGL((gemm_rows_h3_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, H3_ARGS);
    else
      hipLaunchKernelGGL((gemm_rows_h3_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, H3_ARGS);
  } else if (win_bits)
    hipLaunchKernelGGL((gemm_rows_h3_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, H3_ARGS);
  else
    hipLaunchKernelGGL((gemm_rows_h3_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, H3_ARGS);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

// (a template, so that naming the kernel here does not instantiate it ahead of the dispatch chain: the chain orders the code object)
template <bool ROUTED>
static int wgrad_h3_resident() {
  return bl_resident_workgroups<gemm_wgrad_h3_kernel<ROUTED, false>>(256, 2);
}

extern "C" int bl_gemm_wgrad_h3(const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx, const uint32_t* win_bits,
                                int32_t ld_bits, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N,
                                int32_t K, float out_scale, const float* g_amax_dev, float* gw, int64_t gw_group_stride, int32_t ld_gw,
                                void* stream) {
  return bl_gemm_wgrad_h3_impl(a, g_packed, g_idx, win_bits, ld_bits, group_ptr, group_w, G, M, N, K, out_scale, g_amax_dev, gw,
                               gw_group_stride, ld_gw, false, stream);
}

int bl_gemm_wgrad_h3_impl(const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx, const uint32_t* win_bits,
                          int32_t ld_bits, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K,
                          float out_scale, const float* g_amax_dev, float* gw, int64_t gw_group_stride, int32_t ld_gw,
                          bool group_w_one_to_one, void* stream) {
  const char* who = "bl_gemm_wgrad_h3";
  if (M == 0) return BL_OK;
  BlPackedRows r;
  if (int rc = bl_packed_rows(who, a, K, r)) return rc;
  BL_CHECK_ARG(M > 0 && N > 0 && N % 32 == 0 && g_packed && gw && bl_aligned16(g_packed) && out_scale > 0.f,
               "%s: N a multiple of 32, aligned pointers and a positive out_scale required", who);
  const bool routed = win_bits != nullptr;
  BL_CHECK_ARG(!routed || (g_idx && ld_bits * 32 >= N), "%s: the routed form needs g_idx and ld_bits >= N / 32", who);
  const BlWgradPlan p = bl_wgrad_plan(group_ptr, group_w, G, M, N, K, XBM, XBN, routed ? wgrad_h3_resident<true>() : wgrad_h3_resident<false>(),
                                      stream, group_w_one_to_one);
  const dim3 grid = p.grid;
#define HW_ARGS                                                                                                                  \
  BL_PACKED_ROWS_ARGS(r), reinterpret_cast<const uint4*>(g_packed), g_idx, win_bits, ld_bits, group_ptr, group_w, G, M, N, K, p.kchunk, \
      gw, (long long)gw_group_stride, ld_gw, p.ntiles_n, p.xcd, p.order_ctr, out_scale, g_amax_dev
  if (g_h3_one_term) {
    if (routed)
      hipLaunchKernelGGL((gemm_wgrad_h3_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, HW_ARGS);
    else
      hipLaunchKernelGGL((gemm_wgrad_h3_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, HW_ARGS);
  } else if (routed)
    hipLaunchKernelGGL((gemm_wgrad_h3_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, HW_ARGS);
  else
    hipLaunchKernelGGL((gemm_wgrad_h3_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, HW_ARGS);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}
