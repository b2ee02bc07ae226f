// Review queues: k-center greedy (farthest-point) selection of the warnings a reviewer should label next
// (buglab/models/review.py; the NumPy twin is buglab/models/_review.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h ("Review queue"); in short, on the int8
// images q [M, Dp] of bl_sim_quantize, all M rows in one row space:
//   norm      n_i = sum_d q_id^2 (int32, exact); 0 marks an invalid row
//   affinity  a(i, j) = (double)(idot |idot|) / (double)(n_i n_j), idot = sum_d q_id q_jd: both products in int64 and below
//             2^53, one IEEE quotient; a(i, i) == 1.0
//   cover     per valid row (best, near): the greatest affinity to a centre, the lower centre index among equals; -2.0 / -1: none
//   pick      among rows with eligible != 0, n > 0 and best < stop the lowest best, the lowest index among equals; none: the
//             queue has ended.  Otherwise centre s is applied to every valid row: a(i, s) > best_i replaces (best_i, near_i).
// Integer dots, one rounded quotient per pair, compares: no sqrt, no exp, no atomics, nothing that depends on a launch geometry,
// so the twin is equal bit for bit for every number of slices and of workgroups.
//
// bl_review_norms     one wave per row, the packed int8 dot of a row with itself
// bl_review_cover_i8  rv_cover_kernel: workgroup (b, s) keeps rows 16 b .. 16 b + 15 in registers as B fragments and walks slice s
//                     of the centres' 16-row tiles as A through v_mfma_i32_16x16x64_i8, a tile per wave and step.  A lane owns
//                     ONE row (its column) and sees 4 centres per tile: the epilogue turns each accumulator into an affinity
//                     and keeps the lane's running (best, near).  The 16 running pairs per row (4 lane groups x 4 waves) are
//                     combined through shuffles and LDS into the slice's partial; rv_cover_merge_kernel, one thread per row,
//                     combines the S partials and the caller's state.  Every combine is the total order "greater affinity,
//                     then lower centre index", so neither the cut nor the order of the visits shows.  M x L is never stored.
// bl_review_greedy    B + 1 launches of rv_step_kernel on the caller's stream.  NO COMMUNICATION BETWEEN WORKGROUPS INSIDE A
//                     LAUNCH: every hand-off is a kernel boundary.  Launch k (a) reduces, in EVERY workgroup, the G partials
//                     (best, index) that launch k - 1 wrote -- all arrive at the same winner, workgroup 0 records it as pick
//                     k - 1, and every workgroup applies the end rule itself; (b) loads the winner's image and norm once;
//                     (c) updates its rows with the packed int8 dot (v_dot4c_i32_i8) on 16-byte loads, four lanes per row;
//                     (d) writes its own partial of the updated state.  The partials are ping-pong buffered: launch k reads
//                     set (k - 1) & 1 and writes set k & 1, so a workgroup that is still reading never sees a set being
//                     written.  The word that says the queue has ended is handed on the same way: launch k reads the word
//                     launch k - 1 wrote and writes the other one, so no launch reads a word that is written during it.
//                     Launch 0 only scans (and resets its ended word and the pick lists); once the queue has ended the
//                     remaining launches read one word, pass it on and return.
//
// OPERAND and C/D MAPS of the MFMA: bl_similar.hip's.  A = the centres' tile, B = the rows: col = l & 15 is row 16 b + col, and
// register `reg` of lane l is the pair with centre 16 t + 4 (l >> 4) + reg.
#include "bl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int RV_THREADS = 256;
constexpr int RV_WAVES = RV_THREADS / BL_WAVE;
constexpr int RV_TILE = 16;
constexpr int RV_MAX_CHUNKS = BL_SIM_MAX_D / 64;
constexpr int RV_LANES_PER_ROW = 4;                          // of the greedy step: 16 bytes per lane and load
constexpr int RV_ROWS_PER_PASS = RV_THREADS / RV_LANES_PER_ROW;  // == BL_REVIEW_ROWS_PER_BLOCK
constexpr int RV_MAX_PIECES = BL_SIM_MAX_D / 16 / RV_LANES_PER_ROW;  // 16-byte pieces of a row per lane
constexpr int RV_CTRL_BYTES = 16;                            // int32 [4]: the ended word of even launches | of odd ones | unused

typedef int rv_v4i __attribute__((ext_vector_type(4)));

// one IEEE quotient of two exact conversions: |idot| <= 512 * 127^2 < 2^23, so both int64 products stay below 2^53
__device__ __forceinline__ double rv_affinity(int idot, int ni, int nj) {
  const int64_t d = idot;
  return (double)(d * (d < 0 ? -d : d)) / (double)((int64_t)ni * (int64_t)nj);
}

// the order of a cover: greater affinity, then the lower centre index (near < 0: no centre yet)
__device__ __forceinline__ bool rv_covers_better(double a, int id, double best, int near) {
  return near < 0 || a > best || (a == best && id < near);
}

// the order of a pick: lower best, then the lower row index (index < 0: no row)
__device__ __forceinline__ bool rv_picks_before(double a, int i, double b, int j) { return i >= 0 && (j < 0 || a < b || (a == b && i < j)); }

// ---- bl_review_norms ----
__global__ __launch_bounds__(RV_THREADS) void rv_norms_kernel(const int8_t* __restrict__ q, int64_t ldq, int64_t M, int Dp,
                                                              int32_t* __restrict__ n) {
  const int lane = threadIdx.x % BL_WAVE;
  const int64_t i = (int64_t)blockIdx.x * RV_WAVES + threadIdx.x / BL_WAVE;
  if (i >= M) return;  // the whole wave leaves
  const int32_t* row = reinterpret_cast<const int32_t*>(q + i * ldq);  // 4-byte aligned: base and stride are multiples of 16
  int sum = 0;
  for (int w = lane; w < Dp / 4; w += BL_WAVE) {
    const int32_t word = row[w];
    sum = __builtin_amdgcn_sdot4(word, word, sum, false);
  }
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, BL_WAVE);
  if (lane == 0) n[i] = sum;  // at most 512 * 127^2
}

// ---- bl_review_cover_i8 ----
__global__ __launch_bounds__(RV_THREADS) void rv_cover_kernel(const int8_t* __restrict__ q, int64_t ldq, const int32_t* __restrict__ n,
                                                              int64_t M, const int8_t* __restrict__ qc, int64_t ldc,
                                                              const int32_t* __restrict__ nc, int64_t L, int first_id, int Dp, int S,
                                                              double* __restrict__ part_best, int32_t* __restrict__ part_near) {
  __shared__ double s_best[RV_WAVES][RV_TILE];
  __shared__ int s_near[RV_WAVES][RV_TILE];
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int col = lane & 15, group = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * RV_TILE;
  const int s = blockIdx.y;
  const int chunks = Dp / 64;
  const int64_t tiles = (L + RV_TILE - 1) / RV_TILE;
  const int64_t t_begin = tiles * s / S, t_end = tiles * (s + 1) / S;

  // the rows' fragments stay in registers for the whole slice (a row past M loads the last one; its results are dropped)
  const int64_t mine = r0 + col < M ? r0 + col : M - 1;
  rv_v4i bfrag[RV_MAX_CHUNKS];
#pragma unroll
  for (int kc = 0; kc < RV_MAX_CHUNKS; ++kc)
    bfrag[kc] = kc < chunks ? *reinterpret_cast<const rv_v4i*>(q + mine * ldq + kc * 64 + group * 16) : rv_v4i{0, 0, 0, 0};
  const int n_mine = r0 + col < M ? n[mine] : 0;  // 0: an invalid row, covered by nothing

  double best = -2.0;
  int near = -1;
  for (int64_t t = t_begin + wave; t < t_end; t += RV_WAVES) {
    const int64_t base = t * RV_TILE;
    const int64_t arow = base + col < L ? base + col : L - 1;  // a centre past L loads the last one; its results are dropped below
    const int8_t* ap = qc + arow * ldc + group * 16;
    rv_v4i acc = {0, 0, 0, 0};
#pragma unroll
    for (int kc = 0; kc < RV_MAX_CHUNKS; ++kc)
      if (kc < chunks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const rv_v4i*>(ap + kc * 64), bfrag[kc], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t j = base + group * 4 + reg;
      if (j >= L || n_mine <= 0) continue;
      const int nj = nc[j];
      if (nj <= 0) continue;  // an invalid centre covers nothing
      const double a = rv_affinity(acc[reg], n_mine, nj);
      const int id = first_id + (int)j;
      if (rv_covers_better(a, id, best, near)) {
        best = a;
        near = id;
      }
    }
  }
  // the four lane groups of a row, then the four waves
#pragma unroll
  for (int o = 16; o < BL_WAVE; o <<= 1) {
    const double ob = __shfl_xor(best, o, BL_WAVE);
    const int on = __shfl_xor(near, o, BL_WAVE);
    if (on >= 0 && rv_covers_better(ob, on, best, near)) {
      best = ob;
      near = on;
    }
  }
  if (group == 0) {
    s_best[wave][col] = best;
    s_near[wave][col] = near;
  }
  __syncthreads();
  if (tid < RV_TILE && r0 + tid < M) {
    best = s_best[0][tid];
    near = s_near[0][tid];
#pragma unroll
    for (int w = 1; w < RV_WAVES; ++w) {
      const double ob = s_best[w][tid];
      const int on = s_near[w][tid];
      if (on >= 0 && rv_covers_better(ob, on, best, near)) {
        best = ob;
        near = on;
      }
    }
    part_best[(int64_t)s * M + r0 + tid] = best;
    part_near[(int64_t)s * M + r0 + tid] = near;
  }
}

__global__ __launch_bounds__(RV_THREADS) void rv_cover_merge_kernel(const double* __restrict__ part_best,
                                                                    const int32_t* __restrict__ part_near, int64_t M, int S,
                                                                    double* __restrict__ best, int32_t* __restrict__ near) {
  const int64_t i = (int64_t)blockIdx.x * RV_THREADS + threadIdx.x;
  if (i >= M) return;
  double b = best[i];
  int c = near[i];
  bool changed = false;
  for (int s = 0; s < S; ++s) {
    const double ob = part_best[(int64_t)s * M + i];
    const int on = part_near[(int64_t)s * M + i];
    if (on >= 0 && rv_covers_better(ob, on, b, c)) {
      b = ob;
      c = on;
      changed = true;
    }
  }
  if (changed) {
    best[i] = b;
    near[i] = c;
  }
}

// ---- bl_review_greedy ----
// the first of the workgroup's (value, index) pairs in the order of a pick, in every thread; two barriers
__device__ __forceinline__ void rv_block_first(double& v, int& i, double* s_v, int* s_i) {
  const int lane = threadIdx.x % BL_WAVE, wave = threadIdx.x / BL_WAVE;
#pragma unroll
  for (int o = BL_WAVE / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, BL_WAVE);
    const int oi = __shfl_xor(i, o, BL_WAVE);
    if (rv_picks_before(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();  // the arrays may still be read from the call before
  if (lane == 0) {
    s_v[wave] = v;
    s_i[wave] = i;
  }
  __syncthreads();
  v = s_v[0];
  i = s_i[0];
#pragma unroll
  for (int w = 1; w < RV_WAVES; ++w)
    if (rv_picks_before(s_v[w], s_i[w], v, i)) {
      v = s_v[w];
      i = s_i[w];
    }
}

__global__ __launch_bounds__(RV_THREADS) void rv_step_kernel(const int8_t* __restrict__ q, int64_t ldq, const int32_t* __restrict__ n,
                                                             const uint8_t* __restrict__ eligible, int64_t M, int Dp, int B, int k,
                                                             double stop, int32_t* ctrl, double* part_best, int32_t* part_idx,
                                                             double* __restrict__ best, int32_t* __restrict__ near,
                                                             int32_t* __restrict__ picks, double* __restrict__ pick_aff,
                                                             int32_t* __restrict__ pick_near) {
  __shared__ double s_v[RV_WAVES];
  __shared__ int s_i[RV_WAVES];
  const int tid = threadIdx.x, G = gridDim.x;
  const int sub = tid % RV_LANES_PER_ROW;
  const int pieces = Dp / 16;  // 16-byte pieces of a row: 4 .. 32, a multiple of 4

  int winner = -1;
  int n_w = 0;
  rv_v4i wfrag[RV_MAX_PIECES];
  const bool scribe = blockIdx.x == 0 && tid == 0;  // the one thread that records picks and the ended word
  if (k == 0) {  // reset what the chain owns: the ended word and the pick lists
    if (blockIdx.x == 0) {
      if (tid == 0) ctrl[0] = 0;
      for (int p = tid; p < B; p += RV_THREADS) {
        picks[p] = -1;
        pick_aff[p] = 0.0;
        pick_near[p] = -1;
      }
    }
  } else {
    // The ended word is ping-pong buffered like the partials: launch k reads word (k - 1) & 1, which launch k - 1 wrote and
    // nobody writes now, and ALWAYS writes word k & 1.  So every wave of every workgroup of a launch reads the same value.
    if (ctrl[(k - 1) & 1] != 0) {  // the queue ended in an earlier launch
      if (scribe) ctrl[k & 1] = 1;
      return;
    }
    // (a) the winner of the partials of launch k - 1: every workgroup reduces all of them and arrives at the same row
    const double* pb = part_best + (int64_t)((k - 1) & 1) * G;
    const int32_t* pi = part_idx + (int64_t)((k - 1) & 1) * G;
    double wv = 0.0;
    for (int g = tid; g < G; g += RV_THREADS) {
      const double v = pb[g];
      const int i = pi[g];
      if (rv_picks_before(v, i, wv, winner)) {
        wv = v;
        winner = i;
      }
    }
    rv_block_first(wv, winner, s_v, s_i);
    if (winner < 0 || (int64_t)winner >= M) {  // no row left (or garbage, which is never an address): the end, the state stays
      if (scribe) ctrl[k & 1] = 1;
      return;
    }
    if (scribe) {
      ctrl[k & 1] = 0;
      picks[k - 1] = winner;
      pick_aff[k - 1] = wv;
    }
    // (b) the winner's image and norm, once: this lane's pieces sub, sub + 4, ...
    n_w = n[winner];
    const int8_t* wrow = q + (int64_t)winner * ldq;
#pragma unroll
    for (int p = 0; p < RV_MAX_PIECES; ++p) {
      const int piece = sub + p * RV_LANES_PER_ROW;
      wfrag[p] = piece < pieces ? *reinterpret_cast<const rv_v4i*>(wrow + piece * 16) : rv_v4i{0, 0, 0, 0};
    }
  }

  // (c) + (d) this workgroup's rows: four lanes per row, 64 rows per pass
  const int64_t per = (M + G - 1) / G;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < M ? lo + per : M;
  double mv = 0.0;
  int mi = -1;
  for (int64_t r = lo + tid / RV_LANES_PER_ROW; r < hi; r += RV_ROWS_PER_PASS) {  // the four lanes of a row stay together
    const int nr = n[r];
    double b = best[r];
    if (winner >= 0 && nr > 0) {
      const int8_t* row = q + r * ldq;
      int idot = 0;
#pragma unroll
      for (int p = 0; p < RV_MAX_PIECES; ++p) {
        const int piece = sub + p * RV_LANES_PER_ROW;
        if (piece < pieces) {
          const rv_v4i v = *reinterpret_cast<const rv_v4i*>(row + piece * 16);
#pragma unroll
          for (int j = 0; j < 4; ++j) idot = __builtin_amdgcn_sdot4(v[j], wfrag[p][j], idot, false);
        }
      }
      idot += __shfl_xor(idot, 1, BL_WAVE);
      idot += __shfl_xor(idot, 2, BL_WAVE);
      const double a = rv_affinity(idot, nr, n_w);
      if (sub == 0 && r == winner) pick_near[k - 1] = near[r];  // what covered the pick so far: the one thread that owns the row
      if (a > b) {  // strict: a queued pick never displaces an equal earlier centre
        b = a;
        if (sub == 0) {
          best[r] = a;
          near[r] = winner;
        }
      }
    }
    if (nr > 0 && b < stop && (eligible == nullptr || eligible[r] != 0) && rv_picks_before(b, (int)r, mv, mi)) {
      mv = b;
      mi = (int)r;
    }
  }
  rv_block_first(mv, mi, s_v, s_i);
  if (tid == 0) {
    part_best[(int64_t)(k & 1) * G + blockIdx.x] = mv;
    part_idx[(int64_t)(k & 1) * G + blockIdx.x] = mi;
  }
}

inline bool rv_dp_ok(int32_t Dp) { return Dp >= 64 && Dp % 64 == 0; }
inline bool rv_ld_ok(int64_t ld, int32_t Dp) { return ld >= Dp && ld % 16 == 0; }
}  // namespace

extern "C" int bl_review_norms(const int8_t* q, int64_t ldq, int64_t M, int32_t Dp, int32_t* n, void* stream) {
  BL_CHECK_ARG(M >= 0, "bl_review_norms: negative M (%lld)", (long long)M);
  BL_CHECK_ARG(rv_dp_ok(Dp), "bl_review_norms: Dp = %d must be a positive multiple of 64", (int)Dp);
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, "bl_review_norms: Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);
  BL_CHECK_RANGE(M <= BL_REVIEW_MAX_ROWS, "bl_review_norms: M = %lld is above BL_REVIEW_MAX_ROWS = %d", (long long)M, BL_REVIEW_MAX_ROWS);
  BL_CHECK_ARG(rv_ld_ok(ldq, Dp), "bl_review_norms: the row stride %lld must be a multiple of 16 and at least Dp = %d", (long long)ldq, (int)Dp);
  BL_CHECK_ARG(M == 0 || (q && n), "bl_review_norms: null q / n");
  BL_CHECK_ARG(M == 0 || bl_aligned16(q), "bl_review_norms: the int8 image must be 16-byte aligned");
  if (M == 0) return BL_OK;
  hipLaunchKernelGGL(rv_norms_kernel, dim3((unsigned)((M + RV_WAVES - 1) / RV_WAVES)), dim3(RV_THREADS), 0, (hipStream_t)stream, q, ldq, M,
                     (int)Dp, n);
  BL_LAUNCH_CHECK("bl_review_norms");
  return BL_OK;
}

extern "C" int64_t bl_review_cover_workspace_bytes(int64_t M, int32_t slices) {
  if (M < 0 || M > BL_REVIEW_MAX_ROWS || slices < 1 || slices > BL_REVIEW_MAX_SLICES) return -1;
  return M * (int64_t)slices * 12;  // the affinities (fp64), then the centres (int32)
}

extern "C" int bl_review_cover_i8(const int8_t* q, int64_t ldq, const int32_t* n, int64_t M, const int8_t* qc, int64_t ldc,
                                  const int32_t* nc, int64_t L, int32_t first_id, int32_t Dp, int32_t slices, void* workspace,
                                  int64_t workspace_bytes, double* best, int32_t* near, void* stream) {
  BL_CHECK_ARG(M >= 0 && L >= 0, "bl_review_cover_i8: negative size (M %lld, L %lld)", (long long)M, (long long)L);
  BL_CHECK_ARG(rv_dp_ok(Dp), "bl_review_cover_i8: Dp = %d must be a positive multiple of 64", (int)Dp);
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, "bl_review_cover_i8: Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);
  BL_CHECK_RANGE(M <= BL_REVIEW_MAX_ROWS && L <= BL_REVIEW_MAX_ROWS, "bl_review_cover_i8: M = %lld or L = %lld is above BL_REVIEW_MAX_ROWS = %d",
                 (long long)M, (long long)L, BL_REVIEW_MAX_ROWS);
  BL_CHECK_ARG(first_id >= 0 && (int64_t)first_id + L <= (int64_t)0x7fffffff, "bl_review_cover_i8: the centre indices %d .. %lld leave int32",
               (int)first_id, (long long)first_id + (long long)L);
  BL_CHECK_ARG(slices >= 1 && slices <= BL_REVIEW_MAX_SLICES, "bl_review_cover_i8: slices = %d must be in [1, %d]", (int)slices,
               BL_REVIEW_MAX_SLICES);
  BL_CHECK_ARG(rv_ld_ok(ldq, Dp) && rv_ld_ok(ldc, Dp), "bl_review_cover_i8: the row strides %lld / %lld must be multiples of 16 and at least Dp = %d",
               (long long)ldq, (long long)ldc, (int)Dp);
  BL_CHECK_ARG(M == 0 || (q && n && best && near), "bl_review_cover_i8: null q / n / best / near");
  BL_CHECK_ARG(M == 0 || L == 0 || (qc && nc), "bl_review_cover_i8: null qc / nc with %lld centres", (long long)L);
  BL_CHECK_ARG(M == 0 || (bl_aligned16(q) && (L == 0 || bl_aligned16(qc))), "bl_review_cover_i8: the int8 images must be 16-byte aligned");
  BL_CHECK_ARG(M == 0 || ((uintptr_t)best & 7) == 0, "bl_review_cover_i8: best must be 8-byte aligned");
  const int64_t need = bl_review_cover_workspace_bytes(M, slices);
  BL_CHECK_ARG(M == 0 || L == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "bl_review_cover_i8: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need,
               (long long)workspace_bytes);
  if (M == 0 || L == 0) return BL_OK;
  hipStream_t st = (hipStream_t)stream;
  double* part_best = (double*)workspace;
  int32_t* part_near = (int32_t*)((char*)workspace + M * (int64_t)slices * 8);
  hipLaunchKernelGGL(rv_cover_kernel, dim3((unsigned)((M + RV_TILE - 1) / RV_TILE), (unsigned)slices), dim3(RV_THREADS), 0, st, q, ldq, n, M, qc,
                     ldc, nc, L, (int)first_id, (int)Dp, (int)slices, part_best, part_near);
  BL_LAUNCH_CHECK("bl_review_cover_i8 (cover)");
  hipLaunchKernelGGL(rv_cover_merge_kernel, dim3((unsigned)((M + RV_THREADS - 1) / RV_THREADS)), dim3(RV_THREADS), 0, st, part_best, part_near, M,
                     (int)slices, best, near);
  BL_LAUNCH_CHECK("bl_review_cover_i8 (merge)");
  return BL_OK;
}

extern "C" int32_t bl_review_blocks(int64_t M) {
  if (M < 1) return 1;
  const int64_t g = (M + BL_REVIEW_ROWS_PER_BLOCK - 1) / BL_REVIEW_ROWS_PER_BLOCK;
  return (int32_t)(g < BL_REVIEW_MAX_BLOCKS ? g : BL_REVIEW_MAX_BLOCKS);
}

extern "C" int64_t bl_review_workspace_bytes(int64_t M) {
  if (M < 0 || M > BL_REVIEW_MAX_ROWS) return -1;
  return RV_CTRL_BYTES + 2 * (int64_t)BL_REVIEW_MAX_BLOCKS * 12;  // control | two sets of partials: the affinities, then the rows
}

extern "C" int bl_review_greedy(const int8_t* q, int64_t ldq, const int32_t* n, const uint8_t* eligible, int64_t M, int32_t Dp,
                                int32_t B, double stop, int32_t blocks, void* workspace, int64_t workspace_bytes, double* best,
                                int32_t* near, int32_t* picks, double* pick_aff, int32_t* pick_near, void* stream) {
  static_assert(RV_ROWS_PER_PASS == BL_REVIEW_ROWS_PER_BLOCK, "a pass of the step kernel is BL_REVIEW_ROWS_PER_BLOCK rows");
  BL_CHECK_ARG(M >= 0 && B >= 0, "bl_review_greedy: negative size (M %lld, B %d)", (long long)M, (int)B);
  BL_CHECK_ARG(rv_dp_ok(Dp), "bl_review_greedy: Dp = %d must be a positive multiple of 64", (int)Dp);
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, "bl_review_greedy: Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);
  BL_CHECK_RANGE(M <= BL_REVIEW_MAX_ROWS, "bl_review_greedy: M = %lld is above BL_REVIEW_MAX_ROWS = %d", (long long)M, BL_REVIEW_MAX_ROWS);
  BL_CHECK_RANGE(B <= BL_REVIEW_MAX_BUDGET, "bl_review_greedy: B = %d is above BL_REVIEW_MAX_BUDGET = %d", (int)B, BL_REVIEW_MAX_BUDGET);
  BL_CHECK_ARG(stop > 0.0 && stop <= 1.0, "bl_review_greedy: stop = %g must be in (0, 1]: the square of a similarity in (0, 1]", stop);
  BL_CHECK_ARG(blocks >= 0 && blocks <= BL_REVIEW_MAX_BLOCKS, "bl_review_greedy: blocks = %d must be in [0, %d] (0: bl_review_blocks(M))",
               (int)blocks, BL_REVIEW_MAX_BLOCKS);
  BL_CHECK_ARG(rv_ld_ok(ldq, Dp), "bl_review_greedy: the row stride %lld must be a multiple of 16 and at least Dp = %d", (long long)ldq, (int)Dp);
  BL_CHECK_ARG(B == 0 || (picks && pick_aff && pick_near), "bl_review_greedy: null picks / pick_aff / pick_near");
  BL_CHECK_ARG(B == 0 || ((uintptr_t)pick_aff & 7) == 0, "bl_review_greedy: pick_aff must be 8-byte aligned");
  BL_CHECK_ARG(B == 0 || M == 0 || (q && n && best && near), "bl_review_greedy: null q / n / best / near");
  BL_CHECK_ARG(B == 0 || M == 0 || bl_aligned16(q), "bl_review_greedy: the int8 image must be 16-byte aligned");
  BL_CHECK_ARG(B == 0 || M == 0 || ((uintptr_t)best & 7) == 0, "bl_review_greedy: best must be 8-byte aligned");
  const int64_t need = bl_review_workspace_bytes(M);
  BL_CHECK_ARG(B == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "bl_review_greedy: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need,
               (long long)workspace_bytes);
  if (B == 0) return BL_OK;
  const int G = blocks > 0 ? (int)blocks : (int)bl_review_blocks(M);
  int32_t* ctrl = (int32_t*)workspace;
  double* part_best = (double*)((char*)workspace + RV_CTRL_BYTES);
  int32_t* part_idx = (int32_t*)((char*)workspace + RV_CTRL_BYTES + 2 * (int64_t)BL_REVIEW_MAX_BLOCKS * 8);
  for (int k = 0; k <= B; ++k) {  // M == 0: every workgroup scans nothing, the first reduction ends the queue
    hipLaunchKernelGGL(rv_step_kernel, dim3((unsigned)G), dim3(RV_THREADS), 0, (hipStream_t)stream, q, ldq, n, eligible, M, (int)Dp, (int)B, k,
                       stop, ctrl, part_best, part_idx, best, near, picks, pick_aff, pick_near);
    BL_LAUNCH_CHECK("bl_review_greedy");
  }
  return BL_OK;
}
