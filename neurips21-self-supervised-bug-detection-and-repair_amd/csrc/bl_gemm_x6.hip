// fp32-accurate GEMMs on the bf16 matrix cores ("bf16x6").
//
// The exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 MFMA rate, and at the
// ~1.9 GHz the chip sustains under this load the message / input-gradient GEMMs are pinned at
// 85-110 TF/s.  Here every fp32 operand x is split ONCE into three bf16 terms
//      x = hi + mid + lo  (+ r, |r| <= 2^-27 |x|),   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)
// and a product a*b is evaluated as the six bf16 x bf16 MFMA terms
//      a_h b_h + a_h b_m + a_m b_h + a_h b_l + a_l b_h + a_m b_m          (fp32 accumulate),
// dropping only terms below 2^-26 |ab| -- smaller than fp32's own rounding unit (2^-24): results
// are fp32-equivalent (the parity tests keep the same 1e-4 bound and pass with ~1e-6).  Six
// v_mfma_f32_32x32x16_bf16 (32 cycles each) replace eight v_mfma_f32_32x32x2_f32 (64 cycles each)
// per 16 k's: 2.67x fewer matrix-pipe cycles.
//
// Packed operand layout ("bf16x3 packed", produced by bl_pack_bf16x3*): every row is three bf16
// planes back to back, [hi x D | mid x D | lo x D] (6 D bytes): a row's plane is contiguous, which
// is what both the k-contiguous loads of this file's row GEMM (64 B per row, plane and 32-k stage)
// and the feature-contiguous loads of the weight-gradient GEMM want.  In LDS a stage row of the row
// GEMM is [plane][k-group][8] (row stride 208 B: b128 reads conflict-free, the 8-lane write groups
// overlap in one of four slots), an MFMA fragment (8 k's of one row) is three ds_read_b128 64 B apart.
//
// Kernel shape is the fp32 one's (csrc/bl_gemm.hip): 128 x 128 tile, 4 waves 2 x 2, transposed
// accumulators -> float4 epilogue stores, wave-cooperative group lookup, optional routed
// (winner-masked) left operand for the input-gradient GEMM.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bl_common.h"
#include "bl_gemm_host.h"
#include "bl_gemm_split.h"
#include "bl_x6_locate.h"
#include "bl_x6w_image.h"
#include "bl_h3_image.h"

// ---- packing ------------------------------------------------------------------------------------
// rows: out[r][kg][plane][j] = plane(x[r, 8 kg + j])
// (kg_total, kg_off): the packed row is kg_total k-groups wide per plane and this source fills the groups
// kg_off .. kg_off + D/8 -- how [stash ; current] of a ConcatResidual layer is packed without a concatenated copy
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ x, int ld, long long R, int D,
                                                        uint4* __restrict__ out, int kg_total, int kg_off) {
  const int kgs = D >> 3;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R * kgs) return;
  const long long r = t / kgs;
  const int kgn = kg_total;
  const int kg = (int)(t % kgs) + kg_off;
  x -= 8 * kg_off;  // column index below is relative to the packed row
  const float4 a = *reinterpret_cast<const float4*>(x + r * ld + 8 * kg);
  const float4 b = *reinterpret_cast<const float4*>(x + r * ld + 8 * kg + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint16_t h[8], m[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) split3(v[j], h[j], m[j], l[j]);
  uint4* o = out + r * 3 * kgn + kg;
  o[0] = make_uint4(PK(h[0], h[1]), PK(h[2], h[3]), PK(h[4], h[5]), PK(h[6], h[7]));
  o[kgn] = make_uint4(PK(m[0], m[1]), PK(m[2], m[3]), PK(m[4], m[5]), PK(m[6], m[7]));
  o[2 * kgn] = make_uint4(PK(l[0], l[1]), PK(l[2], l[3]), PK(l[4], l[5]), PK(l[6], l[7]));
}

// The B operand (weights) is packed TILED: for every group, 128-column tile and 32-k stage one
// contiguous 24 KB block, ordered [i (2)][plane (3)][row_lo (64)][k-group (4)] x 8 bf16, column
// n = 64 i + row_lo of the tile.  Thread t of the GEMM reads uint4s t, t + 256, ... of the block: every
// wave-load is 1 KB contiguous, and the block's 24 KB spread over all L2 channels.  With the row-major
// packed form ([n][plane][K], 16 x 64-byte pieces per wave-load, the same few lines requested by every
// workgroup of an edge type at once) the B loads cost 1.8x more (load-only microbenchmark, c2 shapes:
// 0.082 -> 0.045 ms per GEMM).  Columns past N are zero.
// w is [G][K][N] (w_is_kn = 1: the forward weights, transposed on the fly) or [G][N][K] (w_is_kn = 0).
__device__ __forceinline__ void pack_weights_thread(const float* __restrict__ w, int G, int K, int N, int w_is_kn,
                                                    uint4* __restrict__ out, long long t) {
  const int nst = K >> 5, ntn = (N + 127) >> 7;  // t = one (g, tile, stage, i, row_lo, kg)
  if (t >= (long long)G * ntn * nst * 512) return;
  int r = (int)(t & 511);
  const long long blk = t >> 9;
  const int st = (int)(blk % nst), tile = (int)((blk / nst) % ntn), g = (int)(blk / ((long long)nst * ntn));
  // consecutive threads -> consecutive n when the source is [K][N] (coalesced), consecutive k-groups otherwise
  int i, row_lo, kg;
  if (w_is_kn) { row_lo = r & 63; i = (r >> 6) & 1; kg = r >> 7; }
  else { kg = r & 3; row_lo = (r >> 2) & 63; i = r >> 8; }
  const int n = tile * 128 + 64 * i + row_lo, k0 = st * 32 + 8 * kg;
  uint16_t h[8], m[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = 0.f;
    if (n < N) v = w_is_kn ? w[((size_t)g * K + k0 + j) * N + n] : w[((size_t)g * N + n) * K + k0 + j];
    split3(v, h[j], m[j], l[j]);
  }
  uint4* o = out + (size_t)blk * 1536 + i * 768 + row_lo * 4 + kg;
  o[0] = make_uint4(PK(h[0], h[1]), PK(h[2], h[3]), PK(h[4], h[5]), PK(h[6], h[7]));
  o[256] = make_uint4(PK(m[0], m[1]), PK(m[2], m[3]), PK(m[4], m[5]), PK(m[6], m[7]));
  o[512] = make_uint4(PK(l[0], l[1]), PK(l[2], l[3]), PK(l[4], l[5]), PK(l[6], l[7]));
}

__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, int G, int K, int N, int w_is_kn,
                                                           uint4* __restrict__ out) {
  pack_weights_thread(w, G, K, N, w_is_kn, out, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}

// Every operand copy a training step needs of the (just updated) weights in ONE launch: a table of jobs in device memory
// (built once per model by the caller), job j owning the workgroups first_block[j] .. first_block[j+1].
//   kind 0 / 1: bl_pack_weights_x6 with w_is_kn = kind;  kind 2: out[g][n][k] = w[g][k][n] in fp32 (W transposed, the
//   operand of bl_routed_dgrad_nodes);  kind 3 / 4: bl_pack_weights_x6w (the wide row GEMM's image) with w_is_kn = kind - 3;
//   kind 5 / 6: bl_pack_weights_h3 (the f16x3 image) with w_is_kn = kind - 5.
__global__ __launch_bounds__(256) void pack_weights_multi_kernel(const bl_pack_job_t* __restrict__ jobs, int njobs,
                                                                 unsigned* __restrict__ h3_sat_counter) {
  int j = 0;
  while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].first_block) ++j;  // (a few dozen jobs: a linear walk of a cached table)
  const bl_pack_job_t job = jobs[j];
  const long long t = (long long)((int)blockIdx.x - job.first_block) * 256 + threadIdx.x;
  if (job.kind <= 1) {
    pack_weights_thread(job.w, job.G, job.K, job.N, job.kind, reinterpret_cast<uint4*>(job.out), t);
  } else if (job.kind >= 5) {  // 5 / 6: bl_pack_weights_h3 (the f16x3 image, scale BL_H3_W_SCALE) with w_is_kn = kind - 5
    pack_weights_h_thread(job.w, job.G, job.K, job.N, job.kind - 5, reinterpret_cast<uint4*>(job.out), t, BL_H3_W_SCALE, h3_sat_counter);
  } else if (job.kind >= 3) {
    pack_weights_wide_thread(job.w, job.G, job.K, job.N, job.kind - 3, reinterpret_cast<uint4*>(job.out), t);
  } else {
    const long long per = (long long)job.K * job.N;
    if (t >= per * job.G) return;
    const int g = (int)(t / per);
    const long long r = t - (long long)g * per;
    const int n = (int)(r / job.K), k = (int)(r - (long long)n * job.K);  // consecutive threads -> consecutive k of the output row
    reinterpret_cast<float*>(job.out)[t] = job.w[((size_t)g * job.K + k) * job.N + n];
  }
}

// ---- GEMM -----------------------------------------------------------------------------------------
// (work-item lookup x6_find_piece / x6_locate, XCD-contiguous tile order, routing masks: bl_x6_locate.h)
// gemm_rows_body (bl_gemm_split.h) on the three-plane bf16 split, with its epilogue family (X6Epi).
// The plain form fits three workgroups per CU (3 x 52 KB of LDS, <= 168 registers); the routed form
// keeps its routing bytes and masks in registers and runs two.
#define X6_MASKED_WGS 2  // workgroups per CU the routed form is compiled for (3: 168 registers with 11 of them in scratch)
#define X6_PLAIN_WGS 3
template <bool MASKED, int EPI, bool ONE>
__global__ __launch_bounds__(256, MASKED ? X6_MASKED_WGS : X6_PLAIN_WGS) void gemm_rows_x6_kernel(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint32_t* __restrict__ win_bits, int ld_bits, const uint4* __restrict__ bp,
    long long strideB, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G, int M, int N, int K,
    float* __restrict__ c, int ldc, int xcd_remap, X6Epi epi) {
  gemm_rows_body<SplitBf16x3, MASKED, EPI, ONE>(xp0, xp1, xp2, idx0, idx1, idx2, w0, w1, w2, koff1, koff2, nsrc, win_bits, ld_bits, bp,
                                                strideB, group_ptr, group_w, G, M, N, K, c, ldc, xcd_remap, epi, 1.f, nullptr);
}

// ---- weight-gradient GEMM -------------------------------------------------------------------------
// gemm_wgrad_body (bl_gemm_split.h) on the three-plane bf16 split
template <bool ROUTED, bool ONE>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_x6_kernel(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint4* __restrict__ gp, const int* __restrict__ g_idx,
    const uint32_t* __restrict__ win_bits, int ld_bits, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G,
    int M, int N, int K, int kchunk, float* __restrict__ gw_base, long long strideW, int ldw, int ntiles_n, int xcd_remap,
    unsigned* __restrict__ order_ctr) {
  gemm_wgrad_body<SplitBf16x3, ROUTED, ONE>(xp0, xp1, xp2, idx0, idx1, idx2, w0, w1, w2, koff1, koff2, nsrc, gp, g_idx, win_bits, ld_bits,
                                            group_ptr, group_w, G, M, N, K, kchunk, gw_base, strideW, ldw, ntiles_n, xcd_remap, order_ctr,
                                            1.f, nullptr);
}

// ---- weight-gradient GEMM, wide tile ---------------------------------------------------------------
// Same contraction, 256 (features of A) x 128 (channels) per workgroup: 8 waves, each the 64 x 64 block of the kernel above.
// What the PMC counters of the 128 x 128 kernel say (profiles/r04b_wgrad_pmc.json): its matrix pipe is 39 % busy with every
// operand L2-resident or not (0.254 vs 0.269 ms), its waves spend a quarter of their cycles issuing ~6 non-MFMA instructions
// per MFMA (staging: address arithmetic, routing masks, zero-selects, LDS stores) and half of them stalled -- the two waves
// of a SIMD run their staging phases and their MFMA phases at the same time more often than not.  So this kernel
//  * stages the routed operand -- the packed node gradient of the messages' targets -- ONCE per message instead of once
//    per 128-feature half (a quarter less staging work per MFMA),
//  * owns the CU (one 512-thread workgroup, 2 x 72 KB of LDS: double-buffered stages, ONE barrier per 32-message stage),
//  * and runs its two wave groups in opposite phases: waves 0-3 do the stage's 48 MFMAs first and their share of the
//    staging (LDS stores of stage k+1, global loads of stage k+2) after them, waves 4-7 -- the SIMDs' second waves -- do
//    their staging first and the MFMAs after it, so that a SIMD's matrix pipe sees one wave's MFMA stream while the other
//    wave stages.
// LDS image of a stage: [operand: A half 0, A half 1, B][plane][message (32)][128 features], rows of 256 B without padding;
// the four 64-byte granules of a row are XOR-swizzled with (message & 3), which puts the four message rows of a
// transposing read's [4 messages][32 features] block on four different bank groups (conflict-free, SQ_LDS_BANK_CONFLICT 0)
// and keeps the 16-byte stores of 8 consecutive lanes on 32 different banks.
// Used when K is a multiple of 256, every source's width a multiple of 128 and the operands are either all gathered or
// all direct (the message weight gradients of every shipped configuration); everything else runs on the kernel above.
// A rows past the end of the chunk are NOT zeroed: their B rows are (the keep mask), and the clamped row they load is a
// real message of the chunk, so a non-finite value there is in the exact result as well.
#define WW_ROW 128                      // shorts per LDS message row
#define WW_PLANE (32 * WW_ROW)          // shorts per plane (32 messages)
#define WW_OPER (3 * WW_PLANE)          // shorts per operand image
#define WW_STAGE (3 * WW_OPER)          // shorts per stage (A half 0, A half 1, B): 36 864 shorts = 72 KB

__device__ __forceinline__ bf16x8 tr_frag_w(const short* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p + 4 * WW_ROW));  // messages +4: same (message & 3)
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// routing byte -> AND-masks, three VALU per dword (two sign-extending bit-field extracts + one bit-field insert)
__device__ __forceinline__ uint4 keep_from_bits_bfi(uint32_t b) {
  uint4 k;
#define KB_(i_) (uint32_t)__builtin_amdgcn_sbfe(b, i_, 1)
  k.x = (KB_(0) & 0x0000FFFFu) | (KB_(1) & 0xFFFF0000u);
  k.y = (KB_(2) & 0x0000FFFFu) | (KB_(3) & 0xFFFF0000u);
  k.z = (KB_(4) & 0x0000FFFFu) | (KB_(5) & 0xFFFF0000u);
  k.w = (KB_(6) & 0x0000FFFFu) | (KB_(7) & 0xFFFF0000u);
#undef KB_
  return k;
}

// GATHER: every operand row is addressed through an index array (idx0/1/2, g_idx all non-null); otherwise none is
template <bool ROUTED, bool GATHER>
__global__ __launch_bounds__(512) void gemm_wgrad_x6_wide_kernel(
    const uint4* __restrict__ xp0, const uint4* __restrict__ xp1, const uint4* __restrict__ xp2,
    const int* __restrict__ idx0, const int* __restrict__ idx1, const int* __restrict__ idx2, int w0, int w1, int w2,
    int koff1, int koff2, int nsrc, const uint4* __restrict__ gp, const int* __restrict__ g_idx,
    const uint32_t* __restrict__ win_bits, int ld_bits, const int* __restrict__ group_ptr, const int* __restrict__ group_w, int G,
    int M, int N, int K, int kchunk, float* __restrict__ gw_base, long long strideW, int ldw, int ntiles_n, int xcd_remap,
    unsigned* __restrict__ order_ctr) {
  __shared__ __attribute__((aligned(16))) short Ls[2 * WW_STAGE];  // the ONE LDS object of this kernel (144 KB)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int g, e0, ne, tile_y;
  if (!x6_locate(group_ptr, G, M, kchunk, xcd_remap, tile_y, g, e0, ne)) return;
  const int e1 = e0 + ne;
  const int i0 = (tile_y / ntiles_n) * 256;
  const int n0 = (tile_y % ntiles_n) * XBN;
  const int wsel = group_w ? group_w[g] : g;

  // loader: thread -> (message tid >> 4 of the stage, 16-byte chunk tid & 15 = 8 features) of each of the three operand rows
  const int fg = tid & 15, msg = tid >> 4;
  const int nn = n0 + 8 * fg;
  const bool b_ok = nn < N;
  const int nnc = b_ok ? nn : 0;
  // per 128-feature half of the A tile: source (wave-uniform: a half lies inside one source), row length, this thread's chunk.
  // Row offsets are 32-bit in units of 16 bytes (a packed operand below 64 GB).
#define WW_HALF(h_, src_, idx_, rowq_, planeq_, colq_)                                                                 \
  const int fi##h_ = i0 + 128 * h_;                                                                                    \
  const int aj##h_ = (nsrc > 2 && fi##h_ >= koff2) ? 2 : ((nsrc > 1 && fi##h_ >= koff1) ? 1 : 0);                      \
  const uint4* __restrict__ src_ = aj##h_ == 0 ? xp0 : (aj##h_ == 1 ? xp1 : xp2);                                      \
  const int* __restrict__ idx_ = aj##h_ == 0 ? idx0 : (aj##h_ == 1 ? idx1 : idx2);                                     \
  const uint32_t planeq_ = (uint32_t)((aj##h_ == 0 ? w0 : (aj##h_ == 1 ? w1 : w2)) >> 3); /* uint4 per plane */        \
  const uint32_t rowq_ = 3u * planeq_;                                                                                 \
  const uint32_t colq_ = (uint32_t)((fi##h_ - (aj##h_ == 0 ? 0 : (aj##h_ == 1 ? koff1 : koff2))) >> 3) + (uint32_t)fg;
  WW_HALF(0, asrc0, aidx0, arowq0, aplq0, acolq0)
  WW_HALF(1, asrc1, aidx1, arowq1, aplq1, acolq1)
  const uint32_t gplq = (uint32_t)(N >> 3), growq = 3u * gplq, gcolq = (uint32_t)(nnc >> 3);
  const uint32_t* __restrict__ mbase = ROUTED ? win_bits + (nnc >> 5) : nullptr;
  const int mshift = nnc & 31;
  // this thread's slot in an operand plane (shorts): row `msg`, granule (fg >> 2) ^ (msg & 3), chunk fg & 3
  const int slot = msg * WW_ROW + ((((fg >> 2) ^ (msg & 3)) << 2) | (fg & 3)) * 8;

  // Two register sets (A, B) of staged operands, alternating per stage: set X receives stage k+2 while set Y, loaded one
  // iteration earlier, is masked and stored to LDS as stage k+1.  (scalars, not arrays: hipcc sends small arrays that are
  // written under control flow to scratch)
  uint4 ra00A, ra01A, ra02A, ra10A, ra11A, ra12A, rb0A, rb1A, rb2A, ra00B, ra01B, ra02B, ra10B, ra11B, ra12B, rb0B, rb1B, rb2B;
  uint32_t mkA = 0u, mkB = 0u;
  uint32_t ar0A, ar1A, grA, mrA, ar0B, ar1B, grB, mrB;  // gathered rows / message id of a stage still to be loaded

  // rows of the stage that starts at message k0_ -> index set S_   (past the end of the chunk: the chunk's first message --
  // a valid row whose B row gets a zero keep mask)
#define WW_IDX(k0_, S_)                                      \
  {                                                          \
    const int e_ = (k0_) + msg;                              \
    const uint32_t ec_ = (uint32_t)(e_ < e1 ? e_ : e0);      \
    ar0##S_ = GATHER ? (uint32_t)aidx0[ec_] : ec_;           \
    ar1##S_ = GATHER ? (uint32_t)aidx1[ec_] : ec_;           \
    gr##S_ = GATHER ? (uint32_t)g_idx[ec_] : ec_;            \
    mr##S_ = ec_;                                            \
  }
#define WW_LOAD_A0(S_)                                       \
  {                                                          \
    const uint32_t o_ = ar0##S_ * arowq0 + acolq0;           \
    ra00##S_ = asrc0[o_];                                    \
    ra01##S_ = asrc0[o_ + aplq0];                            \
    ra02##S_ = asrc0[o_ + 2u * aplq0];                       \
  }
#define WW_LOAD_A1(S_)                                       \
  {                                                          \
    const uint32_t o_ = ar1##S_ * arowq1 + acolq1;           \
    ra10##S_ = asrc1[o_];                                    \
    ra11##S_ = asrc1[o_ + aplq1];                            \
    ra12##S_ = asrc1[o_ + 2u * aplq1];                       \
  }
#define WW_LOAD_B(S_)                                                    \
  {                                                                      \
    const uint32_t o_ = gr##S_ * growq + gcolq;                          \
    rb0##S_ = gp[o_];                                                    \
    rb1##S_ = gp[o_ + gplq];                                             \
    rb2##S_ = gp[o_ + 2u * gplq];                                        \
    if (ROUTED) mk##S_ = mbase[(size_t)mr##S_ * (uint32_t)ld_bits];      \
  }
#define WW_ST1(off_, v_) *reinterpret_cast<uint4*>(wr_ + (off_)) = (v_);
#define WW_STB(off_, v_)                                                 \
  {                                                                      \
    uint4 b_ = (v_);                                                     \
    b_.x &= keep_.x; b_.y &= keep_.y; b_.z &= keep_.z; b_.w &= keep_.w;  \
    *reinterpret_cast<uint4*>(wr_ + 2 * WW_OPER + (off_)) = b_;          \
  }
#define WW_KEEP(S_, k0_)                                                                             \
  uint4 keep_ = ROUTED ? keep_from_bits_bfi(mk##S_ >> mshift) : make_uint4(~0u, ~0u, ~0u, ~0u);      \
  if (!((k0_) + msg < e1 && b_ok)) keep_ = make_uint4(0u, 0u, 0u, 0u);
#define WW_STORE_A0(S_) WW_ST1(0, ra00##S_) WW_ST1(WW_PLANE, ra01##S_) WW_ST1(2 * WW_PLANE, ra02##S_)
#define WW_STORE_A1(S_) WW_ST1(WW_OPER, ra10##S_) WW_ST1(WW_OPER + WW_PLANE, ra11##S_) WW_ST1(WW_OPER + 2 * WW_PLANE, ra12##S_)
#define WW_STORE_B(S_) WW_STB(0, rb0##S_) WW_STB(WW_PLANE, rb1##S_) WW_STB(2 * WW_PLANE, rb2##S_)

  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;

  // wave -> (A half, 64-feature block of the half, 64-channel block of B)
  const int wq = wave & 3, wn = wave >> 2, li = lane & 31, half = lane >> 5;
  const int ahalf = wq >> 1, afb = (wq & 1) * 64, bfb = wn * 64;
  // transposing read of this lane: message (grp >> 1) * 8 + (l16 >> 2) (+ 4, + 16 s), features base + 32 t + 16 (grp & 1) + 4 (l16 & 3)
  const int l16 = lane & 15, grp = lane >> 4;
  const int tr_row = ((grp >> 1) * 8 + (l16 >> 2)) * WW_ROW;
  const int tr_in = (grp & 1) * 16 + 4 * (l16 & 3);  // inside the 32-feature granule
  const int sw = (l16 >> 2) & 3;                      // (message & 3) of every row this lane reads
  int a_off[2], b_off[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    a_off[t] = ahalf * WW_OPER + tr_row + ((((afb >> 5) + t) ^ sw) << 5) + tr_in;
    b_off[t] = 2 * WW_OPER + tr_row + ((((bfb >> 5) + t) ^ sw) << 5) + tr_in;
  }
  const int nk = (ne + 31) / 32;
  const int nk2 = (nk + 1) & ~1;  // the loop runs stage pairs; a phantom last stage has an all-zero B image

#define WW_FRAGS(rd_, s_)                                                                              \
  _Pragma("unroll") for (int t = 0; t < 2; ++t) _Pragma("unroll") for (int p = 0; p < 3; ++p) {        \
    af[t][p] = tr_frag_w((rd_) + (s_) * 16 * WW_ROW + a_off[t] + p * WW_PLANE);                        \
    bf[t][p] = tr_frag_w((rd_) + (s_) * 16 * WW_ROW + b_off[t] + p * WW_PLANE);                        \
  }
  // One loop iteration = one 32-message stage, straight-line (no branch: loads past the chunk's end are clamped to valid
  // rows, stores past it fill a buffer nobody reads), the staging of the NEXT stages cut in pieces and placed between the
  // six-MFMA-term groups of this stage, so that a wave never leaves the matrix pipe for a whole staging phase: in the
  // phase-structured form (profiles/r04c_trace2.log) a stage took ~7 000 cycles of which each wave spent ~3 400 staging
  // (500-1 000 waiting for its loads, 1 100 on masks + LDS stores, 1 500-1 800 on address arithmetic + issuing 13 loads into
  // a busy texture path) with the matrix pipe idle for half of the stage.
  //   X: the register set that receives stage KT + 2 (rows from index set X, loaded one iteration ago)
  //   Y: the set that holds stage KT + 1 (loaded one iteration ago), masked and stored to the other LDS buffer now;
  //      index set Y receives the rows of stage KT + 3
// scheduling fence: VALU, SALU and LDS reads may move across it; MFMAs, global loads and LDS stores may not -- the staging pieces
// stay where they are written (left alone, hipcc sinks the loads to the end of the iteration and hoists the stores)
#define WW_PIN() __builtin_amdgcn_sched_barrier(0x106);
// (WW_S staging piece, WW_T six-term MFMA group, WW_F fragment reads: the ablation / trace builds that blank them out one at a
// time are made from tools/experiments/bl_gemm_x6_switches.hip, profiles/r04d_wgrad_ablation.log)
#define WW_S(x_) x_
#define WW_T(pa_, pb_)                                                                                \
  _Pragma("unroll") for (int ti = 0; ti < 2; ++ti) _Pragma("unroll") for (int tj = 0; tj < 2; ++tj)   \
      acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][pa_], bf[tj][pb_], acc[ti][tj], 0, 0, 0);
#define WW_F(rd_, s_) WW_FRAGS(rd_, s_)
#define WW_ITER(X, Y, KT)                                                                              \
  {                                                                                                    \
    const int kt_ = (KT);                                                                              \
    const short* rd_ = Ls + (kt_ & 1) * WW_STAGE;                                                      \
    short* wr_ = Ls + ((kt_ + 1) & 1) * WW_STAGE + slot;                                               \
    WW_F(rd_, 0)                                                                                       \
    WW_S(WW_IDX(e0 + (kt_ + 3) * 32, Y))                                                               \
    WW_PIN()                                                                                           \
    WW_T(1, 1)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_LOAD_A0(X))                                                                                \
    WW_PIN()                                                                                           \
    WW_T(2, 0)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_LOAD_A1(X))                                                                                \
    WW_PIN()                                                                                           \
    WW_T(0, 2)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_LOAD_B(X))                                                                                 \
    WW_PIN()                                                                                           \
    WW_T(1, 0)                                                                                         \
    WW_S(WW_KEEP(Y, e0 + (kt_ + 1) * 32))                                                              \
    WW_T(0, 1)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_STORE_A0(Y))                                                                               \
    WW_PIN()                                                                                           \
    WW_T(0, 0)                                                                                         \
    WW_F(rd_, 1)                                                                                       \
    WW_T(1, 1)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_STORE_A1(Y))                                                                               \
    WW_PIN()                                                                                           \
    WW_T(2, 0)                                                                                         \
    WW_PIN()                                                                                           \
    WW_S(WW_STORE_B(Y))                                                                                \
    WW_PIN()                                                                                           \
    WW_T(0, 2) WW_T(1, 0) WW_T(0, 1) WW_T(0, 0)                                                        \
    __syncthreads();                                                                                   \
  }

  // prologue: stage 0 through set A into buffer 0, stage 1 into set B, rows of stage 2 into index set A
  WW_IDX(e0, A)
  WW_LOAD_A0(A) WW_LOAD_A1(A) WW_LOAD_B(A)
  WW_IDX(e0 + 32, B)
  {
    short* wr_ = Ls + slot;
    WW_KEEP(A, e0)
    WW_STORE_A0(A) WW_STORE_A1(A) WW_STORE_B(A)
  }
  WW_LOAD_A0(B) WW_LOAD_A1(B) WW_LOAD_B(B)
  WW_IDX(e0 + 64, A)
  __syncthreads();
  bf16x8 af[2][3], bf[2][3];
  for (int kt = 0; kt < nk2; kt += 2) {
    WW_ITER(A, B, kt)
    WW_ITER(B, A, kt + 1)
  }

  float* __restrict__ gw = gw_base + (long long)wsel * strideW;
  unsigned* ctr = order_ctr ? order_ctr + (size_t)g * gridDim.y + tile_y : nullptr;
  const unsigned turn = (unsigned)((e0 - (group_ptr ? group_ptr[g] : 0)) / kchunk);
  bl_ordered_enter(ctr, turn);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int n = n0 + bfb + tj * 32 + li;
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = i0 + 128 * ahalf + afb + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        unsafeAtomicAdd(&gw[(size_t)f * ldw + n], acc[ti][tj][r]);  // (K is a multiple of 256: every row of the tile exists)
      }
    }
  bl_ordered_leave(ctr, turn);
}

// ================================================================================================
// rows [R, D] of x into columns [col_off, col_off + D) of a packed [R, D_total] matrix; cols: which entry point's width rule to report
static int pack_bf16x3_impl(const char* who, bool cols, const float* x, int32_t ld, int64_t R, int32_t D, int32_t D_total, int32_t col_off,
                            uint16_t* out, void* stream) {
  if (R == 0) return BL_OK;
  BL_CHECK_ARG(x && out && bl_aligned16(x) && bl_aligned16(out), "%s: null or misaligned pointer", who);
  const bool ok = D > 0 && D % 8 == 0 && ld % 4 == 0 && D_total % 8 == 0 && col_off % 8 == 0 && col_off >= 0 && col_off + D <= D_total;
  if (cols) BL_CHECK_ARG(ok, "%s: widths / offset must be multiples of 8 with col_off + D <= D_total", who);
  BL_CHECK_ARG(ok, "%s: D must be a multiple of 8 (got %d)", who, D);
  const long long total = (long long)R * (D / 8);
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld,
                     (long long)R, D, reinterpret_cast<uint4*>(out), D_total / 8, col_off / 8);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

extern "C" int bl_pack_bf16x3(const float* x, int32_t ld, int64_t R, int32_t D, uint16_t* out, void* stream) {
  return pack_bf16x3_impl("bl_pack_bf16x3", false, x, ld, R, D, D, 0, out, stream);
}

extern "C" int bl_pack_bf16x3_cols(const float* x, int32_t ld, int64_t R, int32_t D, int32_t D_total, int32_t col_off,
                                   uint16_t* out, void* stream) {
  return pack_bf16x3_impl("bl_pack_bf16x3_cols", true, x, ld, R, D, D_total, col_off, out, stream);
}

extern "C" int bl_pack_weights_x6(const float* w, int32_t G, int32_t K, int32_t N, int32_t w_is_kn, uint16_t* out,
                                  void* stream) {
  if (G == 0) return BL_OK;
  BL_CHECK_ARG(w && out && bl_aligned16(out), "bl_pack_weights_x6: null or misaligned pointer");
  BL_CHECK_ARG(K > 0 && K % 32 == 0 && N > 0, "bl_pack_weights_x6: K must be a multiple of 32 (got %d)", K);
  const long long total = (long long)G * ((N + 127) / 128) * (K / 32) * 512;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, G, K,
                     N, w_is_kn, reinterpret_cast<uint4*>(out));
  BL_LAUNCH_CHECK("bl_pack_weights_x6");
  return BL_OK;
}

extern "C" int64_t bl_pack_job_blocks(int32_t kind, int32_t G, int32_t K, int32_t N) {
  if (kind <= 1 || kind >= 5) return ((int64_t)G * ((N + 127) / 128) * (K / 32) * 512 + 255) / 256;
  if (kind >= 3) return ((int64_t)G * ((N + WBN - 1) / WBN) * (K / 32) * (WBN * 4) + 255) / 256;
  return ((int64_t)G * K * N + 255) / 256;
}

extern "C" int bl_pack_weights_multi(const bl_pack_job_t* jobs_device, int32_t njobs, int32_t total_blocks, void* stream) {
  if (njobs == 0 || total_blocks == 0) return BL_OK;
  BL_CHECK_ARG(jobs_device && njobs > 0 && total_blocks > 0, "bl_pack_weights_multi: bad arguments");
  hipLaunchKernelGGL(pack_weights_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device, njobs,
                     bl_h3_sat_counter());
  BL_LAUNCH_CHECK("bl_pack_weights_multi");
  return BL_OK;
}

// Operand split of the packed-row GEMMs the sequence models' projections run on (bl_gemm_rows_x6 / _epi / _epi2 / x6w,
// bl_gemm_wgrad_x6): 0 = bf16x6 (six MFMA terms, fp32-equivalent; the default), 1 = bf16x1 (the ONE forms: high planes only --
// bf16 operands, fp32 accumulation and results; `train.py --amp`).  BL_SEQ_GEMM=x1 / bf16x1 / amp in the environment sets
// the initial value.
static int g_seq_gemm_mode = -1;
extern "C" int32_t bl_seq_gemm_mode(void) {
  if (g_seq_gemm_mode < 0) {
    const char* e = getenv("BL_SEQ_GEMM");
    g_seq_gemm_mode = (e && (strcmp(e, "x1") == 0 || strcmp(e, "bf16x1") == 0 || strcmp(e, "amp") == 0)) ? 1 : 0;
  }
  return g_seq_gemm_mode;
}
extern "C" int32_t bl_set_seq_gemm_mode(int32_t mode) {
  const int32_t prev = bl_seq_gemm_mode();
  BL_CHECK_ARG(mode == 0 || mode == 1, "bl_set_seq_gemm_mode: mode must be 0 (bf16x6) or 1 (bf16x1), got %d", mode);
  g_seq_gemm_mode = mode;
  return prev;
}

namespace {
int gemm_rows_x6_impl(const char* who, const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp,
                      int64_t b_group_stride, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N,
                      int32_t K, const X6Epi* epi, float* c, int32_t ldc, void* stream) {
  const bool one = bl_seq_gemm_mode() == 1;
  if (M == 0) return BL_OK;
  BlPackedRows r;
  dim3 grid;
  if (int rc = bl_rows_gemm_plan(who, a, win_bits, ld_bits, bp, group_ptr, G, M, N, K, c, ldc, XBM, r, grid)) return rc;
  BL_CHECK_ARG(b_group_stride % 8 == 0 && (G <= 1 || b_group_stride >= (int64_t)((N + 127) / 128) * (K / 32) * 12288),
               "%s: packed group stride must cover one group's tiled weights (bl_pack_weights_x6)", who);
  BL_CHECK_ARG(!(win_bits && epi), "%s: the routed form has no epilogue", who);
  const int xcd = 1;  // XCD-contiguous tile order (x6_locate)
  X6Epi e = {nullptr, BL_ACT_NONE, 0u, 0u, 1.f, 0, nullptr, 0, nullptr, 1.f, nullptr, nullptr};
  if (epi) e = *epi;
#define X6_ARGS                                                                                                               \
  BL_PACKED_ROWS_ARGS(r), win_bits, ld_bits, reinterpret_cast<const uint4*>(bp), (long long)(b_group_stride / 8), group_ptr, \
      group_w, G, M, N, K, c, ldc, xcd, e
#define X6_LAUNCH(masked_, epi_)                                                                                        \
  {                                                                                                                    \
    if (one)                                                                                                           \
      hipLaunchKernelGGL((gemm_rows_x6_kernel<masked_, epi_, true>), grid, dim3(256), 0, (hipStream_t)stream, X6_ARGS);  \
    else                                                                                                               \
      hipLaunchKernelGGL((gemm_rows_x6_kernel<masked_, epi_, false>), grid, dim3(256), 0, (hipStream_t)stream, X6_ARGS); \
  }
  if (win_bits)
    X6_LAUNCH(true, -1)
  else if (epi && e.form == BL_X6_EPI_ACT_PACK && e.act == BL_ACT_RELU)
    X6_LAUNCH(false, 16 + BL_ACT_RELU)
  else if (epi && e.form == BL_X6_EPI_RES)
    X6_LAUNCH(false, 32)
  else if (epi && e.form == BL_X6_EPI_MASK_PACK)
    X6_LAUNCH(false, 64)
  else if (epi && e.out_rows) {  // (bl_gemm_rows_x6_epi_rows: the node update's tanh only)
    if (e.form != BL_X6_EPI_ACT || e.act != BL_ACT_TANH) {
      bl_set_error("%s: the row-list epilogue is built for bias / tanh / dropout only (got form %d, activation %d)", who, e.form, e.act);
      return BL_EINVAL;
    }
    X6_LAUNCH(false, 128 + BL_ACT_TANH)
  } else if (epi && e.form != BL_X6_EPI_ACT) {
    bl_set_error("%s: epilogue form %d with activation %d is not built (packed result: relu only)", who, e.form, e.act);
    return BL_EINVAL;
  } else if (epi == nullptr)
    X6_LAUNCH(false, -1)
  else if (e.act == BL_ACT_TANH)
    X6_LAUNCH(false, BL_ACT_TANH)
  else if (e.act == BL_ACT_RELU)
    X6_LAUNCH(false, BL_ACT_RELU)
  else if (e.act == BL_ACT_SIGMOID)
    X6_LAUNCH(false, BL_ACT_SIGMOID)
  else if (e.act == BL_ACT_NONE)
    X6_LAUNCH(false, BL_ACT_NONE)
  else {
    bl_set_error("%s: activation %d has no bf16x6 epilogue (none / relu / sigmoid / tanh)", who, e.act);
    return BL_EINVAL;
  }
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

bool g_wgrad_wide = true;  // bl_set_wgrad_tile: A/B switch between the 256 x 128 and the 128 x 128 weight-gradient tile

// (a template, so that naming the kernel here does not instantiate it ahead of the dispatch chain: the chain orders the code object)
template <bool ROUTED, bool ONE>
int wgrad_x6_resident() {
  return bl_resident_workgroups<gemm_wgrad_x6_kernel<ROUTED, ONE>>(256, 2);
}

int gemm_wgrad_x6_impl(const char* who, const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx,
                       const uint32_t* win_bits, int32_t ld_bits, const int32_t* group_ptr, const int32_t* group_w, int32_t G,
                       int32_t M, int32_t N, int32_t K, float* gw, int64_t gw_group_stride, int32_t ld_gw, bool one, void* stream) {
  if (M == 0) return BL_OK;
  BlPackedRows r;
  if (int rc = bl_packed_rows(who, a, K, r)) return rc;
  BL_CHECK_ARG(M > 0 && N > 0 && N % 32 == 0 && g_packed && gw && bl_aligned16(g_packed),
               "%s: N a multiple of 32 and aligned pointers required", who);
  const bool routed = win_bits != nullptr;
  BL_CHECK_ARG(!routed || (g_idx && ld_bits * 32 >= N), "%s: the routed form needs g_idx and ld_bits >= N / 32", who);
  // the 256 x 128 tile (8 waves, routed operand staged once per message) when every 128-feature half lies in one source
  bool wide = g_wgrad_wide && K % 256 == 0;
  int nidx = g_idx ? 1 : 0;
  for (int j = 0; j < a->nsrc; ++j) {
    wide = wide && a->width[j] % 128 == 0;
    nidx += a->idx[j] ? 1 : 0;
  }
  const bool gather = nidx == a->nsrc + 1;
  wide = wide && (gather || nidx == 0) && (gather || !routed);
  // plain (direct-row) weight gradients with few rows -- the sequence models' Linears, 16 384 token rows -- are faster on the
  // 128 x 128 tile (two workgroups per CU): 58 vs 64 us per launch at seq-great's shapes (profiles/r03q / r04m seq kernel stats)
  if (!gather && M < 65536) wide = false;
  if (one) wide = false;  // bf16x1 has the 128 x 128 tile only
  // rows reduced by one workgroup: an integer number of rounds of resident workgroups (bl_wgrad_kchunk)
  const int resident = wide ? bl_num_cus() : (one ? (routed ? wgrad_x6_resident<true, true>() : wgrad_x6_resident<false, true>())
                                                        : (routed ? wgrad_x6_resident<true, false>() : wgrad_x6_resident<false, false>()));
  const BlWgradPlan p = bl_wgrad_plan(group_ptr, group_w, G, M, N, K, wide ? 256 : XBM, XBN, resident, stream);
  const dim3 grid = p.grid;
#define WX6_ARGS                                                                                                              \
  BL_PACKED_ROWS_ARGS(r), reinterpret_cast<const uint4*>(g_packed), g_idx, win_bits, ld_bits, group_ptr, group_w, G, M, N, K, \
      p.kchunk, gw, (long long)gw_group_stride, ld_gw, p.ntiles_n, p.xcd, p.order_ctr
  if (wide && routed)
    hipLaunchKernelGGL((gemm_wgrad_x6_wide_kernel<true, true>), grid, dim3(512), 0, (hipStream_t)stream, WX6_ARGS);
  else if (wide && gather)
    hipLaunchKernelGGL((gemm_wgrad_x6_wide_kernel<false, true>), grid, dim3(512), 0, (hipStream_t)stream, WX6_ARGS);
  else if (wide)
    hipLaunchKernelGGL((gemm_wgrad_x6_wide_kernel<false, false>), grid, dim3(512), 0, (hipStream_t)stream, WX6_ARGS);
  else if (routed && one)
    hipLaunchKernelGGL((gemm_wgrad_x6_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, WX6_ARGS);
  else if (one)
    hipLaunchKernelGGL((gemm_wgrad_x6_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, WX6_ARGS);
  else if (routed)
    hipLaunchKernelGGL((gemm_wgrad_x6_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, WX6_ARGS);
  else
    hipLaunchKernelGGL((gemm_wgrad_x6_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, WX6_ARGS);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}
}  // namespace

// 256: the wide (256 x 128, 8-wave) weight-gradient tile where it applies (default); 128: the 128 x 128 tile everywhere.
// A measurement switch (tools/gemm_bench.py); returns the previous setting.
extern "C" int32_t bl_set_wgrad_tile(int32_t rows) {
  const int32_t prev = g_wgrad_wide ? 256 : 128;
  g_wgrad_wide = rows != 128;
  return prev;
}

// Rows per workgroup of the weight-gradient GEMMs (both operand splits): the chunk is the smallest one that fills an integer number of rounds
// of resident workgroups and is <= cap rows.  Returns the previous cap.
extern "C" int32_t bl_set_wgrad_kchunk_cap(int32_t rows) {
  const int32_t prev = g_wgrad_kchunk_cap;
  if (rows >= 256) g_wgrad_kchunk_cap = rows;
  return prev;
}

extern "C" int bl_gemm_rows_x6(const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp,
                               int64_t b_group_stride, const int32_t* group_ptr, const int32_t* group_w, int32_t G,
                               int32_t M, int32_t N, int32_t K, float* c, int32_t ldc, void* stream) {
  return gemm_rows_x6_impl("bl_gemm_rows_x6", a, win_bits, ld_bits, bp, b_group_stride, group_ptr, group_w, G, M, N, K, nullptr, c, ldc,
                           stream);
}

extern "C" int bl_gemm_rows_x6_epi(const bl_rows_packed_t* a, const uint16_t* bp, int64_t b_group_stride, const int32_t* group_ptr,
                                   const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, const float* bias,
                                   int32_t act, bl_dropout_t drop, float* c, int32_t ldc, void* stream) {
  BL_CHECK_ARG((uint64_t)M * (uint64_t)N < (1ull << 32) || drop.p <= 0.f, "bl_gemm_rows_x6_epi: dropout index space is 32 bit");
  BL_CHECK_ARG(bias == nullptr || bl_aligned16(bias), "bl_gemm_rows_x6_epi: misaligned bias");
  const bl_drop_dev d = bl_make_drop(drop);
  X6Epi e = {bias, act, d.key, d.thresh, d.scale, 0, nullptr, 0, nullptr, 1.f, nullptr, nullptr};
  return gemm_rows_x6_impl("bl_gemm_rows_x6_epi", a, nullptr, 0, bp, b_group_stride, group_ptr, group_w, G, M, N, K, &e, c, ldc, stream);
}

// bl_gemm_rows_x6_epi (one group, tanh) whose result row i is stored at row out_rows[i] (< nrows_out) of c, with the dropout counter
// of THAT row (row * N + column): what it stores is bit-identical to the same rows of the launch over all nrows_out rows.
extern "C" int bl_gemm_rows_x6_epi_rows(const bl_rows_packed_t* a, const uint16_t* bp, int32_t M, int32_t N, int32_t K, const float* bias,
                                        int32_t act, bl_dropout_t drop, const int32_t* out_rows, int32_t nrows_out, float* c, int32_t ldc,
                                        void* stream) {
  BL_CHECK_ARG(out_rows && nrows_out >= M, "bl_gemm_rows_x6_epi_rows: out_rows missing or fewer output rows than result rows");
  BL_CHECK_ARG((uint64_t)nrows_out * (uint64_t)N < (1ull << 32) || drop.p <= 0.f, "bl_gemm_rows_x6_epi_rows: dropout index space is 32 bit");
  BL_CHECK_ARG(bias == nullptr || bl_aligned16(bias), "bl_gemm_rows_x6_epi_rows: misaligned bias");
  const bl_drop_dev d = bl_make_drop(drop);
  X6Epi e = {bias, act, d.key, d.thresh, d.scale, 0, nullptr, 0, nullptr, 1.f, nullptr, nullptr, out_rows};
  return gemm_rows_x6_impl("bl_gemm_rows_x6_epi_rows", a, nullptr, 0, bp, 0, nullptr, nullptr, 1, M, N, K, &e, c, ldc, stream);
}

extern "C" int bl_gemm_rows_x6_epi2(const bl_rows_packed_t* a, const uint16_t* bp, int32_t M, int32_t N, int32_t K, const bl_x6_epi_t* epi,
                                    float* c, int32_t ldc, void* stream) {
  BL_CHECK_ARG(epi, "bl_gemm_rows_x6_epi2: null epilogue");
  BL_CHECK_ARG((uint64_t)M * (uint64_t)N < (1ull << 32) || epi->drop.p <= 0.f, "bl_gemm_rows_x6_epi2: dropout index space is 32 bit");
  BL_CHECK_ARG(epi->bias == nullptr || bl_aligned16(epi->bias), "bl_gemm_rows_x6_epi2: misaligned bias");
  const bool packs = epi->form == BL_X6_EPI_ACT_PACK || epi->form == BL_X6_EPI_MASK_PACK;
  BL_CHECK_ARG(!packs || (epi->c_packed && bl_aligned16(epi->c_packed) && N % 8 == 0),
               "bl_gemm_rows_x6_epi2: the packed result needs a 16-byte aligned buffer and N %% 8 == 0");
  BL_CHECK_ARG(epi->form != BL_X6_EPI_RES || (epi->res && bl_aligned16(epi->res) && epi->ld_res % 4 == 0 && epi->ld_res >= N),
               "bl_gemm_rows_x6_epi2: the residual needs an aligned [M, ld_res >= N] matrix");
  BL_CHECK_ARG(epi->form != BL_X6_EPI_MASK_PACK || (epi->y_packed && bl_aligned16(epi->y_packed)),
               "bl_gemm_rows_x6_epi2: the masked form needs the packed forward output");
  BL_CHECK_ARG(epi->form != BL_X6_EPI_MASK_PACK || epi->colsum == nullptr || !bl_get_deterministic(),
               "bl_gemm_rows_x6_epi2: the column sums are flushed by unordered atomics (deterministic mode is on)");
  const bl_drop_dev d = bl_make_drop(epi->drop);
  X6Epi e = {epi->bias, epi->act, d.key, d.thresh, d.scale, epi->form, epi->res, epi->ld_res,
             reinterpret_cast<const uint2*>(epi->y_packed), epi->mask_scale, epi->colsum, reinterpret_cast<uint2*>(epi->c_packed)};
  // (the packed forms never touch c: any non-null aligned pointer passes the common checks)
  float* cc = packs ? reinterpret_cast<float*>(epi->c_packed) : c;
  return gemm_rows_x6_impl("bl_gemm_rows_x6_epi2", a, nullptr, 0, bp, 0, nullptr, nullptr, 1, M, N, K, &e, cc, packs ? N : ldc, stream);
}

extern "C" int bl_gemm_wgrad_routed_x6(const bl_rows_packed_t* a, const uint16_t* g_node_packed, const int32_t* g_idx,
                                       const uint32_t* win_bits, int32_t ld_bits, const int32_t* group_ptr,
                                       const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, float* gw,
                                       int64_t gw_group_stride, int32_t ld_gw, void* stream) {
  BL_CHECK_ARG(M == 0 || (g_idx && win_bits), "bl_gemm_wgrad_routed_x6: needs g_idx and the winner bitmask");
  return gemm_wgrad_x6_impl("bl_gemm_wgrad_routed_x6", a, g_node_packed, g_idx, win_bits, ld_bits, group_ptr, group_w, G, M, N, K, gw,
                            gw_group_stride, ld_gw, false, stream);  // (a message GEMM: bl_set_msg_gemm_mode's, not the sequence switch's)
}

extern "C" int bl_gemm_wgrad_x6(const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx, const int32_t* group_ptr,
                                const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, float* gw,
                                int64_t gw_group_stride, int32_t ld_gw, void* stream) {
  return gemm_wgrad_x6_impl("bl_gemm_wgrad_x6", a, g_packed, g_idx, nullptr, 0, group_ptr, group_w, G, M, N, K, gw, gw_group_stride, ld_gw,
                            bl_seq_gemm_mode() == 1, stream);
}
