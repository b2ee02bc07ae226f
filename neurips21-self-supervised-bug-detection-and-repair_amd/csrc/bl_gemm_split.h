// The packed-row GEMM kernels, written once for both operand splits.
//
// bl_gemm_x6.hip splits an fp32 operand into three bf16 planes (six MFMA terms per product), bl_gemm_h3.hip into two scaled fp16
// planes (three terms).  Everything else -- loader mapping, LDS staging, k loop, wave tiling, the result tile's way out -- is one
// kernel shape: the two bodies below, which the __global__ kernels of those files instantiate with a split trait.  A trait carries
// what the split decides (planes, fragment type, MFMA and term list, LDS row layout of the row GEMM, result scaling); the bodies
// never branch on it at run time.
#pragma once
#include <float.h>

#include "bl_common.h"
#include "bl_x6_locate.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#define XBM 128
#define XBN 128
#define PK(a_, b_) ((uint32_t)(a_) | ((uint32_t)(b_) << 16))

// scale from a device-resident amax (gradient tensors): s = 2^(14 - e) with 2^(e-1) < amax <= 2^e; amax == 0 (or non-finite) -> 1
__device__ __forceinline__ float h3_scale_from_amax(float amax) {
  if (!(amax > 0.f) || amax > FLT_MAX) return 1.f;
  int e;
  (void)frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
  int k = 14 - e;
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  return ldexpf(1.f, k);
}

// ---- operand splits --------------------------------------------------------------------------------
// term(t, x, y, acc): acc + x[plane] . y[plane] for pair t of the split's NT plane pairs, small terms first, the high planes'
// pair last -- the only one of the ONE forms (reduced precision: bl_set_seq_gemm_mode(1) / bl_set_msg_gemm_mode(2)).  x is the
// MFMA's first operand.
//
// LDS row of a row-GEMM stage image (row() uint4): [plane][k-group slot (4)] x 16 B, in one of two layouts:
//   padded    rows of one more uint4: fragment reads conflict-free, the staging stores' 16-lane groups overlap in 4 of 64 banks
//             (bf16: SQ_LDS_BANK_CONFLICT a third of SQ_LDS_IDX_ACTIVE, profiles/r04z_fwd_gemm_pmc.json);
//   swizzled  unpadded rows, k-group kg of a row in slot kg ^ ((row >> 2) & 3): four consecutive rows' 64-byte plane segments tile
//             the 64 banks and the reads of 16 consecutive rows hit 16 different (segment, slot) pairs -- conflict-free both ways.
struct SplitBf16x3 {
  static constexpr int NP = 3;  // hi, mid, lo
  typedef bf16x8 frag;
  static constexpr bool SCALED = false;     // no operand scales: the result is the accumulator
  static constexpr bool STREAM_OUT = false;  // (the streaming result store was measured on the fp16 split only)
  // Measured (profiles/r04y_swizzle.log): the routed form gains 2 % (H = 128 layer) / 4.3 % (concat layer) from the swizzle, the
  // plain form loses 2 % at the H = 128 layer (equal at the concat layer).  So: swizzled for the routed form, padded for the plain
  // one.  ONE: rows of 64 B, padded to 80 B in the plain form (16 rows' b128 reads on 64 different banks).
  static constexpr bool swizzled(bool masked) { return masked; }
  static constexpr int row(bool masked, bool one) { return one ? (masked ? 4 : 5) : (masked ? 12 : 13); }
  static constexpr int NT = 6;  // (m,m) (l,h) (h,l) (m,h) (h,m) (h,h)
  static __device__ __forceinline__ f32x16 term(int t, const frag* x, const frag* y, f32x16 a) {
    constexpr int X[NT] = {1, 2, 0, 1, 0, 0}, Y[NT] = {1, 0, 2, 0, 1, 0};
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[X[t]], y[Y[t]], a, 0, 0, 0);
  }
};

struct SplitF16x2 {
  static constexpr int NP = 2;  // hi, lo
  typedef f16x8 frag;
  static constexpr bool SCALED = true;     // operands carry power-of-two scales: the result is out_scale x the accumulator
  static constexpr bool STREAM_OUT = true;  // result rows leave with non-temporal stores
  // 144-byte rows in every form (36 r mod 64 walks all sixteen 4-bank groups over 16 rows: fragment reads conflict-free)
  static constexpr bool swizzled(bool) { return false; }
  static constexpr int row(bool, bool) { return 9; }
  static constexpr int NT = 3;  // (l,h) (h,l) (h,h)
  static __device__ __forceinline__ f32x16 term(int t, const frag* x, const frag* y, f32x16 a) {
    constexpr int X[NT] = {1, 0, 0}, Y[NT] = {0, 1, 0};
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(x[X[t]], y[Y[t]], a, 0, 0, 0);
  }
};

// ---- row GEMM ----------------------------------------------------------------------------------------
// optional epilogue of the row GEMM: C = drop(act(A . B + bias)) -- the dense node update of the message-passing layer
// (ptgnn MlpMessagePassingLayer's Linear -> tanh -> Dropout tail; call site buglab/models/gnnlayerdefs.py:6-23)
struct X6Epi {
  const float* bias;  // [N] or nullptr
  int act;            // BL_ACT_*
  uint32_t drop_key, drop_thresh;
  float drop_scale;
  // the extended forms (bl_gemm_rows_x6_epi2: the Linear layers of the relational transformer block, csrc/bl_great_layer.hip)
  int form;                // BL_X6_EPI_*
  const float* res;        // RES: c = A . B + res[row, n]
  int ld_res;
  const uint2* himask;     // MASK: the packed forward output y [M][3 N] -- c = (y's hi plane != 0) ? A . B x mask_scale : 0
  float mask_scale;
  float* colsum;           // MASK: [N] += column sums of c (the bias gradient)
  uint2* c_packed;         // PACK / MASK: the result in bl_pack_bf16x3's form [M][3 N] instead of fp32
  const int* out_rows;     // ROWS: result row i is stored at row out_rows[i] of c, and its dropout counter is that row's
};

// C[rows of g] = rows(a) . B_g, rows gathered from <= 3 packed sources; MASKED: the routed (winner-masked) left operand, one
// source, of the input-gradient GEMM.  128 x 128 tile, 4 waves 2 x 2, 32 k's per LDS stage with a register prefetch.
// EPI: -1 = no epilogue, else the epilogue family of the unscaled split: 0..15 = activation code (bias / activation / dropout,
// fp32 result); 16 + code = the same, result PACKED only; 32 = + residual (fp32 result); 64 = masked by the packed forward output,
// column sums, result packed only; 128 + code = ROWS, the 0..15 form whose result row i goes to row epi.out_rows[i] of c with that
// row's dropout counter (the dense update of a layer's live nodes: a kept row is bit-identical to the full launch's).
// (The activation is a template parameter: with a run-time switch the compiler evaluates every
// activation's libm call for every element -- measured 0.12 vs 0.05 ms on the c2 dense shape.)
// A SCALED split multiplies the result by out_scale = 1 / (s_a s_b) (host part), divided by h3_scale_from_amax(*a_amax_dev) when
// the left operand's scale lives in device memory.
// ONE: the same packed images, high planes only -- the other planes are neither loaded nor staged, one MFMA term per 16 k's, fp32
// accumulation; every epilogue as in the full form.
// (ablation builds of this kernel -- rows not gathered, no MFMAs, no result stores, term-major MFMA order, direct stores -- are made
// from tools/experiments/bl_gemm_x6_switches.hip; their numbers are in tools/experiments/README.md)
template <class S, bool MASKED, int EPI, bool ONE>
__device__ __forceinline__ void gemm_rows_body(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint32_t* __restrict__ win_bits, int ld_bits, const uint4* __restrict__ bp,
    long long strideB, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G, int M, int N, int K,
    float* __restrict__ c, int ldc, int xcd_remap, X6Epi epi, float out_scale, const float* __restrict__ a_amax_dev) {
  static_assert(EPI == -1 || !S::SCALED, "the epilogues are built for the unscaled split only");
  constexpr bool E_ROWS = EPI >= 128 && EPI < 144;
  constexpr bool E_ACT = (EPI >= 0 && EPI < 32) || E_ROWS, E_PACK = EPI >= 16 && (EPI < 32 || EPI == 64), E_RES = EPI == 32, E_MASK = EPI == 64;
  constexpr int ACT = EPI >= 0 ? (EPI & 15) : 0;
  constexpr bool SWZ = S::swizzled(MASKED);
  constexpr int NP = ONE ? 1 : S::NP;    // planes loaded, staged and multiplied
  constexpr int T0 = ONE ? S::NT - 1 : 0;  // first term evaluated
  constexpr int XROW = S::row(MASKED, ONE);
  constexpr int XEPI = 4 * 32 * 68 / 4;  // uint4 the four waves' result tiles take on their way out
  constexpr int XLDS = (XBM + XBN) * XROW > XEPI ? (XBM + XBN) * XROW : XEPI;
#define XSLOT(row_, kg_) (SWZ ? ((kg_) ^ (((row_) >> 2) & 3)) : (kg_))
  // one array: after the last stage the four waves' result tiles are staged in it on their way out (see the epilogue)
  __shared__ uint4 ABs[XLDS];
  uint4* As = ABs;
  uint4* Bs = ABs + XBM * XROW;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int g, row0, nrows, tile_y;
  if (!x6_locate(group_ptr, G, M, XBM, xcd_remap, tile_y, g, row0, nrows)) return;
  const int n0 = tile_y * XBN;
  const int wsel = group_w ? group_w[g] : g;
  // tiled packed weights: this workgroup's stage blocks (S::NP x 512 uint4), thread t reads uint4s t + 256 q
  const uint4* __restrict__ Bt = bp + (long long)wsel * strideB + (size_t)tile_y * (K >> 5) * (S::NP * 512) + tid;

  // loader mapping: (row, k-group) pairs, 2 per thread; 4 consecutive lanes cover one row's 64-byte
  // plane segment.  Gathered row ids live in registers (one per piece and source).
  const int p_kg = tid & 3, p_row0 = tid >> 2;  // rows p_row0 and p_row0 + 64
  int gr0[2], gr1[2], gr2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = row0 + min(p_row0 + 64 * i, nrows - 1);
    gr0[i] = idx0 ? idx0[r] : r;
    gr1[i] = nsrc > 1 ? (idx1 ? idx1[r] : r) : 0;
    gr2[i] = nsrc > 2 ? (idx2 ? idx2[r] : r) : 0;
  }
  uint4 ra[2][NP], rb[2][NP];
  uint32_t ma[2];
  const int nk = (K + 31) / 32;

#define ROWS_LOAD_STAGE(k0_)                                                                                  \
  {                                                                                                           \
    const int k_ = (k0_) + 8 * p_kg;                                                                          \
    const int kc_ = k_ < K ? k_ : 0;                                                                          \
    int j_ = 0;                                                                                               \
    if (nsrc > 1 && kc_ >= koff1) j_ = 1;                                                                     \
    if (nsrc > 2 && kc_ >= koff2) j_ = 2;                                                                     \
    const int kl_ = kc_ - (j_ == 0 ? 0 : (j_ == 1 ? koff1 : koff2));                                          \
    const uint4* base_ = j_ == 0 ? xp0 : (j_ == 1 ? xp1 : xp2);                                               \
    const int wj_ = j_ == 0 ? w0 : (j_ == 1 ? w1 : w2);                                                       \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                           \
      const int row_ = p_row0 + 64 * i;                                                                       \
      const int gr_ = j_ == 0 ? gr0[i] : (j_ == 1 ? gr1[i] : gr2[i]);                                         \
      const uint4* src_ = base_ + (size_t)gr_ * S::NP * (wj_ >> 3) + (kl_ >> 3);                              \
      ra[i][0] = src_[0];                                                                                     \
      if constexpr (NP > 1) ra[i][1] = src_[wj_ >> 3];                                                        \
      if constexpr (NP > 2) ra[i][2] = src_[2 * (wj_ >> 3)];                                                  \
      if (MASKED) ma[i] = win_bits[(size_t)(row0 + min(row_, nrows - 1)) * ld_bits + (kc_ >> 5)];              \
      const uint4* bsrc_ = Bt + (size_t)((k0_) >> 5) * (S::NP * 512) + i * (S::NP * 256);                     \
      rb[i][0] = bsrc_[0];                                                                                    \
      if constexpr (NP > 1) rb[i][1] = bsrc_[256];                                                            \
      if constexpr (NP > 2) rb[i][2] = bsrc_[512];                                                            \
    }                                                                                                         \
  }
#define ROWS_STORE_STAGE(k0_)                                                                                 \
  {                                                                                                           \
    const bool kok_ = (k0_) + 8 * p_kg < K;                                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                           \
      const int row_ = p_row0 + 64 * i;                                                                       \
      uint4 keep_ = make_uint4(~0u, ~0u, ~0u, ~0u);                                                           \
      if (MASKED) keep_ = keep_from_bits(ma[i] >> (8 * p_kg)); /* k0 is a multiple of 32 */                  \
      if (!kok_) keep_ = make_uint4(0u, 0u, 0u, 0u);                                                          \
      const bool nok_ = kok_ && (n0 + row_ < N);                                                              \
      _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                                        \
        uint4 a_ = ra[i][p];                                                                                  \
        a_.x &= keep_.x; a_.y &= keep_.y; a_.z &= keep_.z; a_.w &= keep_.w;                                   \
        As[row_ * XROW + p * 4 + XSLOT(row_, p_kg)] = a_;                                                     \
        Bs[row_ * XROW + p * 4 + XSLOT(row_, p_kg)] = nok_ ? rb[i][p] : make_uint4(0u, 0u, 0u, 0u);           \
      }                                                                                                       \
    }                                                                                                         \
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;

  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, half = lane >> 5;

  ROWS_LOAD_STAGE(0)
  ROWS_STORE_STAGE(0)
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) ROWS_LOAD_STAGE((kt + 1) * 32)
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two 16-k MFMA steps per stage; this lane's 8 k's = group 2s + half
      const int kg = 2 * s + half;
      typename S::frag af[2][NP], bf[2][NP];  // a fragment (8 k's of one row): one ds_read_b128 per plane, 64 B apart
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4* pa = &As[(wm * 64 + t * 32 + li) * XROW + XSLOT(li, kg)];
        const uint4* pb = &Bs[(wn * 64 + t * 32 + li) * XROW + XSLOT(li, kg)];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          af[t][p] = __builtin_bit_cast(typename S::frag, pa[4 * p]);
          bf[t][p] = __builtin_bit_cast(typename S::frag, pb[4 * p]);
        }
      }
      // swapped operands (B fragment in the A slot): the accumulator holds the transposed tile, so
      // a lane owns 4 consecutive columns of one row.  The terms of one accumulator are written back to
      // back (hipcc alternates between two accumulators); letting the four accumulators take turns instead measured equal
      // (profiles/r04y_term_major.log): a dependent MFMA two issue slots later does not stall
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          f32x16 a = acc[ti][tj];
#pragma unroll
          for (int t = T0; t < S::NT; ++t) a = S::term(t, bf[tj], af[ti], a);
          acc[ti][tj] = a;
        }
    }
    __syncthreads();
    if (kt + 1 < nk) {
      ROWS_STORE_STAGE((kt + 1) * 32)
      __syncthreads();
    }
  }
#undef ROWS_LOAD_STAGE
#undef ROWS_STORE_STAGE
#undef XSLOT

  if constexpr (S::SCALED)
    if (a_amax_dev) out_scale /= h3_scale_from_amax(*a_amax_dev);
  // The accumulator layout gives a lane 4 consecutive columns of one row, a wave-wide store 64 pieces of 16 B on 32 different
  // rows: 32-byte segments.  The tile goes through LDS instead (per wave [32 rows][64 + 4] fp32, the operand images are dead
  // after the last stage's barrier) and leaves as whole 256-byte row pieces, 16 lanes per piece: measured on the node
  // update's backward kernel (same layout, csrc/bl_node_bwd.hip), the direct form cost 2-3x the time of its bytes.
  float* stage = reinterpret_cast<float*>(ABs) + wave * (32 * 68);
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int m = wm * 64 + ti * 32 + li;
    // (ROWS: the row whose dropout counter this result row takes; rows past the tile's last are computed and dropped as ever)
    const uint32_t drow = E_ROWS ? (uint32_t)epi.out_rows[row0 + min(m, nrows - 1)] : (uint32_t)(row0 + m);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int n = n0 + wn * 64 + tj * 32 + 8 * gq + 4 * half;
        float v[4] = {acc[ti][tj][4 * gq + 0], acc[ti][tj][4 * gq + 1], acc[ti][tj][4 * gq + 2], acc[ti][tj][4 * gq + 3]};
        if constexpr (S::SCALED) {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] *= out_scale;
        }
        if (E_ACT) {
          float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (epi.bias && n < N) bv = *reinterpret_cast<const float4*>(epi.bias + n);
          v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v[u] = bl_act(ACT, v[u]);
            if (epi.drop_thresh) {  // same counter as the fp32 row GEMM: element index row * N + column
              const uint32_t idx = drow * (uint32_t)N + (uint32_t)(n + u);
              v[u] = ((bl_lowbias32(idx + epi.drop_key) >> 8) >= epi.drop_thresh) ? v[u] * epi.drop_scale : 0.f;
            }
          }
        }
        *reinterpret_cast<float4*>(stage + li * 68 + tj * 32 + 8 * gq + 4 * half) = make_float4(v[0], v[1], v[2], v[3]);
      }
    // (a wave reads back only what it wrote itself; its LDS operations execute in order)
    const int c4 = lane & 15, n = n0 + wn * 64 + 4 * c4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = (lane >> 4) + 4 * j;
      const int mm = wm * 64 + ti * 32 + r;
      float4 v = *reinterpret_cast<const float4*>(stage + r * 68 + 4 * c4);
      if (mm < nrows && n < N) {
        const size_t grow = E_ROWS ? (size_t)epi.out_rows[row0 + mm] : (size_t)(row0 + mm);
        if (E_RES) {
          const float4 rv = *reinterpret_cast<const float4*>(epi.res + grow * epi.ld_res + n);
          v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
        }
        if (E_MASK) {  // y = drop(relu(z)) != 0  <=>  kept and z > 0: the hi plane of a non-zero fp32 is non-zero
          const uint2 hm = epi.himask[(grow * 3 * N + n) >> 2];
          v.x = (hm.x & 0x7fffu) ? v.x * epi.mask_scale : 0.f;
          v.y = (hm.x & 0x7fff0000u) ? v.y * epi.mask_scale : 0.f;
          v.z = (hm.y & 0x7fffu) ? v.z * epi.mask_scale : 0.f;
          v.w = (hm.y & 0x7fff0000u) ? v.w * epi.mask_scale : 0.f;
          csum.x += v.x; csum.y += v.y; csum.z += v.z; csum.w += v.w;
        }
        if (E_PACK) {
          uint16_t h[4], m[4], l[4];
          split3(v.x, h[0], m[0], l[0]);
          split3(v.y, h[1], m[1], l[1]);
          split3(v.z, h[2], m[2], l[2]);
          split3(v.w, h[3], m[3], l[3]);
          uint2* o = epi.c_packed + ((grow * 3 * N + n) >> 2);
          o[0] = make_uint2(PK(h[0], h[1]), PK(h[2], h[3]));
          o[N >> 2] = make_uint2(PK(m[0], m[1]), PK(m[2], m[3]));
          o[N >> 1] = make_uint2(PK(l[0], l[1]), PK(l[2], l[3]));
        } else if constexpr (S::STREAM_OUT) {
          bl_store_streaming(c + grow * ldc + n, v);
        } else {
          *reinterpret_cast<float4*>(c + grow * ldc + n) = v;
        }
      }
    }
  }
  if (E_MASK) {  // column sums of this wave's 64 x 64 block: over the four row groups of the lanes, then one atomic per column
    csum.x += __shfl_xor(csum.x, 16, 64); csum.y += __shfl_xor(csum.y, 16, 64); csum.z += __shfl_xor(csum.z, 16, 64); csum.w += __shfl_xor(csum.w, 16, 64);
    csum.x += __shfl_xor(csum.x, 32, 64); csum.y += __shfl_xor(csum.y, 32, 64); csum.z += __shfl_xor(csum.z, 32, 64); csum.w += __shfl_xor(csum.w, 32, 64);
    const int n = n0 + wn * 64 + 4 * (lane & 15);
    if (lane < 16 && n < N && epi.colsum) {
      unsafeAtomicAdd(epi.colsum + n, csum.x);
      unsafeAtomicAdd(epi.colsum + n + 1, csum.y);
      unsafeAtomicAdd(epi.colsum + n + 2, csum.z);
      unsafeAtomicAdd(epi.colsum + n + 3, csum.w);
    }
  }
}

// ---- weight-gradient GEMM (128 x 128 tile) -----------------------------------------------------------
// gW_g[i, n] += sum_{e in group g} A[e, i] * Gr[e, n]     A = gathered packed rows (h[src] | h[tgt]),
//                                                          Gr[e, :] = g_node[g_idx[e], :] where winner == e
// (x out_scale, as in the row GEMM, for a SCALED split).
// The contraction runs over MESSAGES, but the 16-bit MFMA wants 8 consecutive k's of one row in a
// lane: the operands have to be transposed on the way.  Both tiles are stored in LDS exactly as
// they arrive -- [plane][message][feature], feature-contiguous rows of 320 B -- and the fragments are
// read with ds_read_b64_tr_b16, gfx950's transposing LDS read: a 16-lane group reads a
// [4 messages][16 features] block (lane 4j+q supplies the address of message j, features 4q..4q+3)
// and lane i receives the 4 messages of feature i.  Two reads = the 8 k's of one MFMA operand.
// Row stride 320 B puts the 4 message rows of a block 16 banks apart: conflict-free.
// Global loads are full 256-byte plane rows (16 lanes x 16 B per message and plane).
#define WRS 160                 // shorts per LDS message row (128 features + 32 pad)
#define WPLANE (32 * WRS)       // shorts per plane (32 messages)

template <class F>
__device__ __forceinline__ F tr_frag(const short* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p + 4 * WRS));
  return __builtin_bit_cast(F, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ONE: the high planes only, as in gemm_rows_body
template <class S, bool ROUTED, bool ONE>
__device__ __forceinline__ void gemm_wgrad_body(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint4* __restrict__ gp, const int* __restrict__ g_idx,
    const uint32_t* __restrict__ win_bits, int ld_bits, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G,
    int M, int N, int K, int kchunk, float* __restrict__ gw_base, long long strideW, int ldw, int ntiles_n, int xcd_remap,
    unsigned* __restrict__ order_ctr, float out_scale, const float* __restrict__ g_amax_dev) {
  constexpr int NP = ONE ? 1 : S::NP, T0 = ONE ? S::NT - 1 : 0;
  __shared__ __attribute__((aligned(16))) short As[NP * WPLANE];
  __shared__ __attribute__((aligned(16))) short Bs[NP * WPLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int g, e0, ne, tile_y;
  if (!x6_locate(group_ptr, G, M, kchunk, xcd_remap, tile_y, g, e0, ne)) return;
  const int e1 = e0 + ne;
  const int i0 = (tile_y / ntiles_n) * XBM;
  const int n0 = (tile_y % ntiles_n) * XBN;
  const int wsel = group_w ? group_w[g] : g;

  // loader: units (message, 8-feature group); unit u = tid + 256 i -> message u >> 4, group u & 15
  const int fg = tid & 15, msg0 = tid >> 4;  // messages msg0 and msg0 + 16
  const int fi = i0 + 8 * fg, nn = n0 + 8 * fg;
  const bool a_ok = fi < K, b_ok = nn < N;
  const int fic = a_ok ? fi : 0, nnc = b_ok ? nn : 0;
  int aj = 0;
  if (nsrc > 1 && fic >= koff1) aj = 1;
  if (nsrc > 2 && fic >= koff2) aj = 2;
  const uint4* __restrict__ abase = (aj == 0 ? xp0 : (aj == 1 ? xp1 : xp2)) + ((fic - (aj == 0 ? 0 : (aj == 1 ? koff1 : koff2))) >> 3);
  const int* __restrict__ aidx = aj == 0 ? idx0 : (aj == 1 ? idx1 : idx2);
  const int awg = (aj == 0 ? w0 : (aj == 1 ? w1 : w2)) >> 3;  // uint4 per plane of an A row
  const int gwg = N >> 3;                                      // uint4 per plane of a G row
  const uint4* __restrict__ gbase = gp + (nnc >> 3);
  const uint32_t* __restrict__ mbase = ROUTED ? win_bits + (nnc >> 5) : nullptr;
  const int mshift = nnc & 31;

  uint4 ra[2][NP], rb[2][NP];
  uint32_t mk[2];
  int arow[2], grow[2], mrow[2];  // gathered rows / message ids of the NEXT stage to load

#define WGRAD_LOAD_IDX(k0_)                                        \
  {                                                                \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                \
      const int e_ = (k0_) + msg0 + 16 * i;                        \
      const int ec_ = e_ < e1 ? e_ : e0;                           \
      arow[i] = aidx ? aidx[ec_] : ec_;                            \
      grow[i] = g_idx ? g_idx[ec_] : ec_;                          \
      mrow[i] = ec_;                                               \
    }                                                              \
  }
#define WGRAD_LOAD_STAGE()                                                                       \
  {                                                                                              \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                              \
      const uint4* a_ = abase + (size_t)arow[i] * S::NP * awg;                                   \
      ra[i][0] = a_[0];                                                                          \
      if constexpr (NP > 1) ra[i][1] = a_[awg];                                                  \
      if constexpr (NP > 2) ra[i][2] = a_[2 * awg];                                              \
      const uint4* g_ = gbase + (size_t)grow[i] * S::NP * gwg;                                   \
      rb[i][0] = g_[0];                                                                          \
      if constexpr (NP > 1) rb[i][1] = g_[gwg];                                                  \
      if constexpr (NP > 2) rb[i][2] = g_[2 * gwg];                                              \
      mk[i] = ROUTED ? mbase[(size_t)mrow[i] * ld_bits] : 0u;                                    \
    }                                                                                            \
  }
#define WGRAD_STORE_STAGE(k0_)                                                                   \
  {                                                                                              \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                              \
      const int eid_ = (k0_) + msg0 + 16 * i;                                                    \
      const bool eok_ = eid_ < e1;                                                               \
      uint4 keep_ = ROUTED ? keep_from_bits(mk[i] >> mshift) : make_uint4(~0u, ~0u, ~0u, ~0u);   \
      if (!(eok_ && b_ok)) keep_ = make_uint4(0u, 0u, 0u, 0u);                                   \
      const int slot_ = (msg0 + 16 * i) * WRS + 8 * fg;                                          \
      _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                           \
        *reinterpret_cast<uint4*>(&As[p * WPLANE + slot_]) = (eok_ && a_ok) ? ra[i][p] : make_uint4(0u, 0u, 0u, 0u); \
        uint4 b_ = rb[i][p];                                                                     \
        b_.x &= keep_.x; b_.y &= keep_.y; b_.z &= keep_.z; b_.w &= keep_.w;                      \
        *reinterpret_cast<uint4*>(&Bs[p * WPLANE + slot_]) = b_;                                 \
      }                                                                                          \
    }                                                                                            \
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;

  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, half = lane >> 5;
  // transposing-read address of this lane inside a [32 messages][WRS] plane, tile feature base 0
  const int l16 = lane & 15, grp = lane >> 4;
  const int tr_off = ((grp >> 1) * 8 + (l16 >> 2)) * WRS + (grp & 1) * 16 + 4 * (l16 & 3);
  const short* a_tr = As + tr_off + wm * 64;
  const short* b_tr = Bs + tr_off + wn * 64;
  const int nk = (ne + 31) / 32;

  WGRAD_LOAD_IDX(e0)
  WGRAD_LOAD_STAGE()
  WGRAD_LOAD_IDX(e0 + 32)
  WGRAD_STORE_STAGE(e0)
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      WGRAD_LOAD_STAGE()
      WGRAD_LOAD_IDX(e0 + (kt + 2) * 32)
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two 16-message MFMA steps per stage
      typename S::frag af[2][NP], bf[2][NP];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          af[t][p] = tr_frag<typename S::frag>(a_tr + p * WPLANE + s * 16 * WRS + t * 32);
          bf[t][p] = tr_frag<typename S::frag>(b_tr + p * WPLANE + s * 16 * WRS + t * 32);
        }
#pragma unroll
      for (int t = T0; t < S::NT; ++t)  // term-major: the four accumulators take turns
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = S::term(t, af[ti], bf[tj], acc[ti][tj]);
    }
    __syncthreads();
    if (kt + 1 < nk) {
      WGRAD_STORE_STAGE(e0 + (kt + 1) * 32)
      __syncthreads();
    }
  }
#undef WGRAD_LOAD_IDX
#undef WGRAD_LOAD_STAGE
#undef WGRAD_STORE_STAGE

  if constexpr (S::SCALED)
    if (g_amax_dev) out_scale /= h3_scale_from_amax(*g_amax_dev);
  float* __restrict__ gw = gw_base + (long long)wsel * strideW;
  // deterministic mode (launched without the XCD remap): the message chunks of one (group, tile) add in chunk order
  unsigned* ctr = order_ctr ? order_ctr + (size_t)g * gridDim.y + tile_y : nullptr;
  const unsigned turn = (unsigned)((e0 - (group_ptr ? group_ptr[g] : 0)) / kchunk);
  bl_ordered_enter(ctr, turn);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int n = n0 + wn * 64 + tj * 32 + li;
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = i0 + wm * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (f < K) unsafeAtomicAdd(&gw[(size_t)f * ldw + n], S::SCALED ? acc[ti][tj][r] * out_scale : acc[ti][tj][r]);
      }
    }
  bl_ordered_leave(ctr, turn);
}
