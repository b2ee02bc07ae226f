// What the GREAT var-misuse head's training forward (bl_varmisuse_head.hip) and its forward-only prediction
// (bl_varmisuse_predict.hip) share: the row pass LayerNorm -> Linear(D, 2) -> masked logits of one wave, the workgroup first-index
// arg-max, and the descriptor checks.  One copy of the row arithmetic, so the two entry points write the same bits.
#pragma once
#include "bl_common.h"

namespace {
constexpr int VM_ROW_THREADS = 256;     // forward rows: 4 waves, one row each
constexpr int VM_SAMPLE_THREADS = 256;  // one workgroup per sample
constexpr int VM_SAMPLE_WAVES = VM_SAMPLE_THREADS / 64;
constexpr int VM_MAX_D = 1024;
#define VM_NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float hsum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// (value, index) arg-max across a wave: larger value wins, a tie goes to the smaller index (torch.argmax's first index)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// the same over the workgroup, combined in wave order; every thread gets the result
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sv, int* si) {
  wave_argmax(v, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wave] = v;
    si[wave] = i;
  }
  __syncthreads();
  v = sv[0];
  i = si[0];
  for (int w = 1; w < VM_SAMPLE_WAVES; ++w)
    if (sv[w] > v || (sv[w] == v && si[w] < i)) {
      v = sv[w];
      i = si[w];
    }
  __syncthreads();
}

// One wave, one row of x [B * L, D]: LayerNorm statistics (mu, rs) and the two logits before bias and masking (a0, a1), in every
// lane.  NK = float4 chunks per lane, ceil(D / 256).
template <int NK>
__device__ __forceinline__ void vm_row_logits(const bl_varmisuse_head_t& d, int64_t row, int lane, float& mu, float& rs, float& a0,
                                              float& a1) {
  const int D = d.D, D4 = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(d.x + row * D);
  float4 v[NK];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int j = lane + 64 * k;
    v[k] = j < D4 ? xr[j] : f4(0.f);
    s += hsum(v[k]);
  }
  mu = bl_wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (lane + 64 * k < D4) {
      const float4 c = make_float4(v[k].x - mu, v[k].y - mu, v[k].z - mu, v[k].w - mu);
      q += (c.x * c.x + c.y * c.y) + (c.z * c.z + c.w * c.w);
    }
  }
  rs = 1.0f / sqrtf(bl_wave_sum(q) / (float)D + d.ln_eps);
  const float4* g4 = reinterpret_cast<const float4*>(d.ln_g);
  const float4* b4 = reinterpret_cast<const float4*>(d.ln_b);
  const float4* w4 = reinterpret_cast<const float4*>(d.W);  // W [D, 2]: float4 2j = rows 4j, 4j+1; 2j+1 = rows 4j+2, 4j+3
  a0 = 0.f;
  a1 = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int j = lane + 64 * k;
    if (j < D4) {
      const float4 g = g4[j], bb = b4[j], wa = w4[2 * j], wb = w4[2 * j + 1];
      const float y0 = (v[k].x - mu) * rs * g.x + bb.x, y1 = (v[k].y - mu) * rs * g.y + bb.y;
      const float y2 = (v[k].z - mu) * rs * g.z + bb.z, y3 = (v[k].w - mu) * rs * g.w + bb.w;
      a0 += (y0 * wa.x + y1 * wa.z) + (y2 * wb.x + y3 * wb.z);
      a1 += (y0 * wa.y + y1 * wa.w) + (y2 * wb.y + y3 * wb.w);
    }
  }
  a0 = bl_wave_sum(a0);
  a1 = bl_wave_sum(a1);
}

// the row's stored logits: bias added, -inf at a masked position, the pointer column -inf at a non-candidate too
__device__ __forceinline__ float2 vm_masked_logits(const bl_varmisuse_head_t& d, int64_t row, float a0, float a1) {
  const int b = (int)(row / d.L), i = (int)(row - (int64_t)b * d.L);
  // token mask `arange(L) > length` (greatreimplementation.py:198, :203): the caller passes lens_att = min(length + 1, L)
  const bool valid = i < d.lens_att[b];
  const float l0 = valid ? a0 + d.bias[0] : VM_NEG_INF;
  const float l1 = (valid && d.candidate_mask[row]) ? a1 + d.bias[1] : VM_NEG_INF;  // :211
  return make_float2(l0, l1);
}

int vm_check(const bl_varmisuse_head_t* d, const char* who) {
  BL_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  BL_CHECK_ARG(d->B >= 1 && d->L >= 1, "%s: B (%d) and L (%d) must be >= 1", who, d->B, d->L);
  BL_CHECK_ARG((int64_t)d->B * d->L <= 0x7fffffff, "%s: B * L (%lld) exceeds int32", who, (long long)d->B * d->L);
  BL_CHECK_ARG(d->D >= 4 && d->D <= VM_MAX_D && d->D % 4 == 0, "%s: D (%d) must be a multiple of 4 in [4, %d]", who, d->D, VM_MAX_D);
  BL_CHECK_ARG(d->ln_eps > 0.f, "%s: ln_eps must be positive", who);
  BL_CHECK_ARG(d->x && d->ln_g && d->ln_b && d->W && d->bias && d->lens_att && d->error_location && d->candidate_mask && d->target_mask,
               "%s: null input pointer", who);
  BL_CHECK_ARG(bl_aligned16(d->x) && bl_aligned16(d->ln_g) && bl_aligned16(d->ln_b) && bl_aligned16(d->W),
               "%s: x, ln_g, ln_b and W must be 16-byte aligned", who);
  return BL_OK;
}
}  // namespace
