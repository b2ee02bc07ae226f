// Host side shared by the GEMM entry points (bl_gemm*.hip): the rules of the packed rows descriptor, the order in which
// its twelve kernel arguments are passed, the weight gradients' chunk solver and the cached resident-workgroup count.
// Host-only: no device code and nothing exported.
#pragma once
#include "bl_common.h"

// bl_rows_packed_t as the kernels take it; slots >= nsrc are null / 0
struct BlPackedRows {
  const uint4* x[3];
  const int32_t* idx[3];
  int width[3];
  int koff[3];  // first k of each source
  int nsrc;
};

// 1..3 sources, each non-null, 16-byte aligned and a multiple of 32 wide, widths summing to K
static inline int bl_packed_rows(const char* who, const bl_rows_packed_t* a, int K, BlPackedRows& r) {
  BL_CHECK_ARG(a && a->nsrc >= 1 && a->nsrc <= 3, "%s: rows descriptor needs 1..3 sources", who);
  r = BlPackedRows{};
  int off = 0;
  for (int j = 0; j < a->nsrc; ++j) {
    BL_CHECK_ARG(a->xp[j] && bl_aligned16(a->xp[j]) && a->width[j] > 0 && a->width[j] % 32 == 0,
                 "%s: source %d: packed pointer 16-byte aligned and width a multiple of 32 required", who, j);
    r.x[j] = reinterpret_cast<const uint4*>(a->xp[j]);
    r.idx[j] = a->idx[j];
    r.width[j] = a->width[j];
    r.koff[j] = off;
    off += a->width[j];
  }
  BL_CHECK_ARG(off == K, "%s: K (%d) != sum of source widths (%d)", who, K, off);
  r.nsrc = a->nsrc;
  return BL_OK;
}

// the first twelve arguments of every packed-row GEMM kernel
#define BL_PACKED_ROWS_ARGS(r)                                                                                            \
  (r).x[0], (r).x[1], (r).x[2], (r).idx[0], (r).idx[1], (r).idx[2], (r).width[0], (r).width[1], (r).width[2], (r).koff[1], \
      (r).koff[2], (r).nsrc

// Rows one workgroup of a weight-gradient GEMM reduces before it flushes its output tile: the chunk of the smallest integer
// number of rounds of `resident` workgroups that is <= cap rows (a partial last round is tail: 1.24 rounds at a fixed chunk
// cost 38 % of the kernel), a multiple of 32 and >= 256 so that the tile-sized atomic flush is amortised.
// ntiles_all: output tiles; extra: workgroups beyond M / kchunk per tile (the partial last pieces of the groups).
static inline int bl_wgrad_kchunk(long long M, int ntiles_all, int extra, int resident, int cap) {
  int kchunk = 256;
  for (int rounds = 1; rounds <= 64; ++rounds) {
    const long long slots = (long long)resident * rounds - extra;
    if (slots <= 0) continue;
    const long long kc = (M * ntiles_all + slots - 1) / slots;
    if (kc <= cap || rounds == 64) {
      kchunk = (int)((kc + 31) / 32 * 32);
      break;
    }
  }
  return kchunk < 256 ? 256 : kchunk;
}

// workgroups of `threads` threads (no dynamic LDS) of Kernel that the device holds at once; asked once per process and kernel
template <auto Kernel>
int bl_resident_workgroups(int threads, int fallback_per_cu) {
  static int resident = 0;
  if (resident == 0) {
    int per_cu = 0;
    hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads, 0);
    if (oe != hipSuccess || per_cu <= 0) per_cu = fallback_per_cu;
    resident = per_cu * bl_num_cus();
  }
  return resident;
}
