// The fp64 dot product of two fp32 rows as one wave forms it, shared by bl_explain.hip (bl_attr_node_scores) and bl_similar.hip
// (bl_sim_quantize, bl_sim_rescore): the COLUMN OWNERSHIP that include/buglab_hip.h states for bl_attr_node_scores.  Columns go in
// quads, quad q = columns 4q .. 4q + 3; lane l owns the quads q with q % 64 == l and adds the products of its columns to its own
// fp64 sum, which starts at +0.0, in ascending column order.  That holds for every D, row stride and alignment: where both rows
// are 16-byte aligned (VEC) a whole quad is one 16-byte load per operand, elsewhere (and for the last, partial quad) the same
// columns are loaded one by one -- the loads differ, the order of the additions does not.  A product of two fp32 values is exact
// in fp64 (24 + 24 significand bits), so only the additions round.  The caller sends the 64 lane sums through bl_wave_sum_f64.
//
// Inline, so the including file's `#pragma clang fp contract(off)` governs the copy compiled into it.
#pragma once
#include "bl_common.h"

namespace {
template <bool VEC>
__device__ __forceinline__ double bl_lane_dot_f64(const float* __restrict__ xr, const float* __restrict__ gr, int D, int lane) {
  double acc = 0.0;
  const int full = D / 4;  // whole quads
  for (int q = lane; q < full; q += BL_WAVE) {
    float xv[4], gv[4];
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4*>(xr + 4 * q);
      const float4 b = *reinterpret_cast<const float4*>(gr + 4 * q);
      xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w;
      gv[0] = b.x, gv[1] = b.y, gv[2] = b.z, gv[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[j] = xr[4 * q + j];
        gv[j] = gr[4 * q + j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)xv[j] * (double)gv[j];
  }
  if (full % BL_WAVE == lane)  // the last, partial quad belongs to the lane that would own it whole (it comes after all of its others)
    for (int c = 4 * full; c < D; ++c) acc += (double)xr[c] * (double)gr[c];
  return acc;
}
}  // namespace
