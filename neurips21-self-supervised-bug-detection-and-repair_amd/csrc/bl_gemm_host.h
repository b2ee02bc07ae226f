// Host side shared by the GEMM entry points (bl_gemm*.hip): the rules of the packed rows descriptor, the order in which
// its twelve kernel arguments are passed, the argument rules and grid of the 128 x 128 row GEMMs, the weight gradients'
// launch plan (chunk solver, grid, flush order) and the cached resident-workgroup count.
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

// What the row GEMMs of both operand splits (bl_gemm_rows_x6*, bl_gemm_rows_h3) ask of their arguments besides the weight
// image's size, which each checks itself, and their grid: row pieces of `tile` rows (one partial piece more per group) x column tiles.
static inline int bl_rows_gemm_plan(const char* who, const bl_rows_packed_t* a, const uint32_t* win_bits, int ld_bits, const void* bp,
                                    const int32_t* group_ptr, int G, int M, int N, int K, const float* c, int ldc, int tile,
                                    BlPackedRows& r, dim3& grid) {
  if (int rc = bl_packed_rows(who, a, K, r)) return rc;
  BL_CHECK_ARG(M > 0 && N > 0 && N % 4 == 0 && ldc % 4 == 0 && bp && c && bl_aligned16(bp) && bl_aligned16(c),
               "%s: N/ldc multiples of 4, aligned pointers required", who);
  BL_CHECK_ARG(win_bits == nullptr || (a->nsrc == 1 && a->idx[0] && ld_bits * 32 >= K),
               "%s: the routed form needs exactly one gathered source and ld_bits >= K / 32", who);
  grid = dim3((M + tile - 1) / tile + (group_ptr ? G : 0), (N + tile - 1) / tile);
  return BL_OK;
}

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

// Largest number of rows one workgroup of a weight-gradient GEMM (either operand split) reduces before it flushes its output
// tile (bl_set_wgrad_kchunk_cap).  Every flush is tile-size fp32 atomics, and the chip retires ~312 G of those per second whatever
// the addresses (tools/atomic_bench.py): at c2's layer shape (E = 640 000, K = 256, N = 128) the 864-row chunks of the old cap
// (1024) were 97 MB = 24 M atomics per launch, ~0.08 ms of a 0.25-ms kernel; the cap trades that against the balance of the last
// round of workgroups.  Measured on bf16x6 (profiles/r04e_kcap_*.log, same box): H = 128 layer 0.254 / 0.232 / 0.210 / 0.220 /
// 0.217 ms at 1024 / 2048 / 3072 / 4096 / 8192, concat layer 0.921 / 0.863 / 0.824 / 0.829 / 0.908 ms at 1024 / 2048 / 4096 /
// 8192 / 16384.
inline int g_wgrad_kchunk_cap = 4096;

// Launch plan of a weight-gradient GEMM with tile_rows x tile_cols output tiles: rows per workgroup (bl_wgrad_kchunk: an integer
// number of rounds of `resident` workgroups), the grid, and the flush order -- without group_w every (group, tile) owns its output
// and its chunks can add in order (the counters are null unless the deterministic mode is on).
struct BlWgradPlan {
  int ntiles_n, kchunk, xcd;
  dim3 grid;
  unsigned* order_ctr;
};
static inline BlWgradPlan bl_wgrad_plan(const int32_t* group_ptr, const int32_t* group_w, int G, int M, int N, int K, int tile_rows,
                                        int tile_cols, int resident, void* stream, bool group_w_one_to_one = false) {
  BlWgradPlan p;
  p.ntiles_n = (N + tile_cols - 1) / tile_cols;
  const int ntiles_all = ((K + tile_rows - 1) / tile_rows) * p.ntiles_n;
  p.kchunk = bl_wgrad_kchunk(M, ntiles_all, (group_ptr ? G : 0) * ntiles_all, resident, g_wgrad_kchunk_cap);
  p.grid = dim3((M + p.kchunk - 1) / p.kchunk + (group_ptr ? G : 0), ntiles_all);
  // (a group_w the caller vouches for as one-to-one leaves every (group, tile) its own output: ordered like no group_w at all)
  p.order_ctr = (group_w && !group_w_one_to_one) ? nullptr : bl_order_counters((group_ptr ? G : 1) * ntiles_all, stream);
  p.xcd = p.order_ctr ? 0 : 1;  // ordered flushes want "lower chunk = lower workgroup id"
  return p;
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
