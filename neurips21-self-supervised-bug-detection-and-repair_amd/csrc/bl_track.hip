// Warning tracking: a one-to-one matching of the warnings of two scans (buglab/models/track.py; the NumPy twin is
// buglab/models/_track.py).
//
// BEYOND THE REFERENCE: it has no counterpart.  The contract is in include/buglab_hip.h ("Warning tracking"); in short, on the
// int8 images of bl_sim_quantize, L old rows and N new rows in one row space, with bl_review_norms' norms:
//   affinity    a(i, j) = (double)(idot |idot|) / (double)(n_i n_j): review's, both products in int64, one IEEE quotient
//   admissible  n_i > 0, n_j > 0, a(i, j) >= floor, and key_old[i] == key_new[j] where keys are given
//   matching    repeatedly the first admissible pair of two unmatched rows in the order (greater affinity, lower old index,
//               lower new index)
// and the device computes it in ROUNDS of mutual best: every open row of either side finds its best admissible open row of the
// other (the lower index among equals), every pair that chose each other is matched, a round that matches nothing ends it.
// Integer dots, one rounded quotient per pair, compares: no sqrt, no exp, no atomics, nothing that depends on a launch geometry.
//
// tk_compact_kernel   one workgroup per side: the open rows of a side as an ASCENDING list of indices, by a prefix sum over
//                     contiguous parts of the list before (or of 0 .. rows - 1).  It also keeps the books: the counts, the rounds
//                     and pairs so far, the word that says the matching has ended.  The control words and the lists are ping-pong
//                     buffered: launch r reads set r & 1 and writes the other, each workgroup its own side's words, so no
//                     workgroup reads a word that another writes during the same launch.
// tk_best_kernel      rv_cover_kernel's scheme on two lists: workgroup (b, s) keeps the open X rows at places 16 b .. 16 b + 15 in
//                     registers as B fragments and walks slice s of the open Y rows' 16-row tiles as A through
//                     v_mfma_i32_16x16x64_i8, a tile per wave and step.  Each lane loads its own row of a tile, so the gather
//                     through the list costs the GEMM nothing.  The epilogue applies the key gate and the floor and keeps the
//                     lane's running (best, arg); shuffles and LDS combine the 16 running pairs of a row into the slice's
//                     partial.  Round r works on open x open, not on L x N; workgroups past the open rows leave at once.
// tk_merge_kernel     one thread per open X row: the S partials in the same total order -> best / arg at the row's OWN index.
// tk_mutual_kernel    one thread per open new row j: i = arg_new[j] and arg_old[i] == j is a match.
// Every hand-off is a kernel boundary; once the matching has ended the remaining launches read one word and return.
//
// OPERAND and C/D MAPS of the MFMA: bl_similar.hip's.  A = the Y tile, B = the X rows: col = l & 15 is place 16 b + col of the X
// list, and register `reg` of lane l is the pair with place 16 t + 4 (l >> 4) + reg of the Y list.
#include "bl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / BL_WAVE;
constexpr int TK_TILE = 16;
constexpr int TK_MAX_CHUNKS = BL_SIM_MAX_D / 64;
constexpr int TK_SCAN_THREADS = 1024;
constexpr int TK_SCAN_WAVES = TK_SCAN_THREADS / BL_WAVE;
constexpr int TK_CTRL_WORDS = 8;                  // one set of control words
constexpr int TK_CTRL_BYTES = 2 * TK_CTRL_WORDS * 4;  // two sets
// the control words of a set: the open rows of side 0 (X / old) and 1 (Y / new), then what the new side's workgroup keeps
enum { TK_COUNT = 0, TK_ENDED = 2, TK_ROUNDS = 3, TK_PAIRS = 4 };

typedef int tk_v4i __attribute__((ext_vector_type(4)));

// review's affinity: |idot| <= 512 * 127^2 < 2^23, so both int64 products stay below 2^53
__device__ __forceinline__ double tk_affinity(int idot, int ni, int nj) {
  const int64_t d = idot;
  return (double)(d * (d < 0 ? -d : d)) / (double)((int64_t)ni * (int64_t)nj);
}

// the order of a row's choice: greater affinity, then the lower index of the other side (arg < 0: nothing yet)
__device__ __forceinline__ bool tk_better(double a, int id, double best, int arg) { return arg < 0 || a > best || (a == best && id < arg); }

// ---- the open rows of a side as an ascending list ----
// side s = blockIdx.x.  Source: places 0 .. count - 1 of list_in (or the rows 0 .. rows - 1 themselves when `fresh`); a row stays
// when mask[row] != 0 (or there is no mask) and match[row] < 0 (or there is no match array).
struct tk_side {
  const int32_t* list_in;
  int32_t* list_out;
  const uint8_t* mask;
  const int32_t* match;
  int32_t rows;
};

__device__ __forceinline__ bool tk_open(const tk_side& sd, int row) {
  return (sd.mask == nullptr || sd.mask[row] != 0) && (sd.match == nullptr || sd.match[row] < 0);
}

__global__ __launch_bounds__(TK_SCAN_THREADS) void tk_compact_kernel(tk_side old_side, tk_side new_side, int fresh,
                                                                     const int32_t* __restrict__ ctrl_in, int32_t* __restrict__ ctrl_out,
                                                                     int32_t* __restrict__ status) {
  __shared__ int s_wave[TK_SCAN_WAVES];
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int side = blockIdx.x;
  const tk_side sd = side == 0 ? old_side : new_side;
  if (!fresh && ctrl_in[TK_ENDED] != 0) {  // ended in an earlier launch: hand the words on, the lists are not read again
    if (tid == 0) {
      ctrl_out[TK_COUNT + side] = ctrl_in[TK_COUNT + side];
      if (side == 1) {
        ctrl_out[TK_ENDED] = 1;
        ctrl_out[TK_ROUNDS] = ctrl_in[TK_ROUNDS];
        ctrl_out[TK_PAIRS] = ctrl_in[TK_PAIRS];
      }
    }
    return;
  }
  int count = fresh ? sd.rows : ctrl_in[TK_COUNT + side];
  count = count < 0 ? 0 : (count > sd.rows ? sd.rows : count);  // a list never holds more than the side's rows
  const int per = (count + TK_SCAN_THREADS - 1) / TK_SCAN_THREADS;
  const int lo = tid * per < count ? tid * per : count;
  const int hi = lo + per < count ? lo + per : count;
  int kept = 0;
  for (int p = lo; p < hi; ++p) kept += tk_open(sd, fresh ? p : sd.list_in[p]) ? 1 : 0;
  // the exclusive prefix sum of `kept` over the workgroup: inside a wave by shuffles, then the waves' totals through LDS
  int incl = kept;
#pragma unroll
  for (int o = 1; o < BL_WAVE; o <<= 1) {
    const int up = __shfl_up(incl, o, BL_WAVE);
    if (lane >= o) incl += up;
  }
  if (lane == BL_WAVE - 1) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < TK_SCAN_WAVES; ++w) {
    const int t = s_wave[w];
    if (w < wave) before += t;
    total += t;
  }
  int at = before + incl - kept;
  for (int p = lo; p < hi; ++p) {
    const int row = fresh ? p : sd.list_in[p];
    if (tk_open(sd, row)) sd.list_out[at++] = row;  // at < total <= count <= rows
  }
  if (tid == 0) {
    ctrl_out[TK_COUNT + side] = total;
    if (side == 1) {  // the books: the new side's workgroup alone keeps them, from its own side's numbers
      const int matched = fresh ? 0 : count - total;
      const int ended = fresh ? 0 : (matched == 0 ? 1 : 0);
      const int rounds = fresh ? 0 : ctrl_in[TK_ROUNDS] + (matched > 0 ? 1 : 0);
      const int pairs = fresh ? 0 : ctrl_in[TK_PAIRS] + matched;
      ctrl_out[TK_ENDED] = ended;
      ctrl_out[TK_ROUNDS] = rounds;
      ctrl_out[TK_PAIRS] = pairs;
      if (status != nullptr) {
        status[0] = rounds;
        status[1] = pairs;
        status[2] = ended;
        status[3] = total;
      }
    }
  }
}

// ---- the directional best ----
__global__ __launch_bounds__(TK_THREADS) void tk_best_kernel(const int8_t* __restrict__ qx, int64_t ldx, const int32_t* __restrict__ nx,
                                                             const int32_t* __restrict__ keyx, const int32_t* __restrict__ listx,
                                                             const int8_t* __restrict__ qy, int64_t ldy, const int32_t* __restrict__ ny,
                                                             const int32_t* __restrict__ keyy, const int32_t* __restrict__ listy,
                                                             const int32_t* __restrict__ ctrl, int side_x, int Dp, int S, double floor,
                                                             int64_t cap, double* __restrict__ part_best, int32_t* __restrict__ part_arg) {
  __shared__ double s_best[TK_WAVES][TK_TILE];
  __shared__ int s_arg[TK_WAVES][TK_TILE];
  if (ctrl[TK_ENDED] != 0) return;
  const int cx = ctrl[TK_COUNT + side_x], cy = ctrl[TK_COUNT + 1 - side_x];  // the open rows of either side
  const int r0 = blockIdx.x * TK_TILE;
  if (r0 >= cx) return;  // the whole workgroup leaves: the open rows have shrunk below this tile
  const int tid = threadIdx.x, lane = tid % BL_WAVE, wave = tid / BL_WAVE;
  const int col = lane & 15, group = lane >> 4;
  const int s = blockIdx.y;
  const int chunks = Dp / 64;
  const int tiles = (cy + TK_TILE - 1) / TK_TILE;
  const int t_begin = (int)((int64_t)tiles * s / S), t_end = (int)((int64_t)tiles * (s + 1) / S);

  // the X rows' fragments stay in registers for the whole slice (a place past cx loads the last row; its results are dropped)
  const bool live = r0 + col < cx;
  const int64_t mine = listx[live ? r0 + col : cx - 1];
  tk_v4i bfrag[TK_MAX_CHUNKS];
#pragma unroll
  for (int kc = 0; kc < TK_MAX_CHUNKS; ++kc)
    bfrag[kc] = kc < chunks ? *reinterpret_cast<const tk_v4i*>(qx + mine * ldx + kc * 64 + group * 16) : tk_v4i{0, 0, 0, 0};
  const int n_mine = live ? nx[mine] : 0;  // 0: an invalid row, which chooses nothing
  const int k_mine = keyx != nullptr ? keyx[mine] : 0;

  double best = -2.0;
  int arg = -1;
  for (int t = t_begin + wave; t < t_end; t += TK_WAVES) {  // cy > 0 here: there is a tile
    const int base = t * TK_TILE;
    const int64_t arow = listy[base + col < cy ? base + col : cy - 1];  // a place past cy loads the last row; dropped below
    const int8_t* ap = qy + arow * ldy + group * 16;
    tk_v4i acc = {0, 0, 0, 0};
#pragma unroll
    for (int kc = 0; kc < TK_MAX_CHUNKS; ++kc)
      if (kc < chunks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const tk_v4i*>(ap + kc * 64), bfrag[kc], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int place = base + group * 4 + reg;
      if (place >= cy || n_mine <= 0) continue;
      const int j = listy[place];
      const int nj = ny[j];
      if (nj <= 0) continue;                                  // an invalid row is chosen by nothing
      if (keyx != nullptr && keyy[j] != k_mine) continue;     // the key gate
      const double a = tk_affinity(acc[reg], n_mine, nj);
      if (!(a >= floor)) continue;                            // the floor
      if (tk_better(a, j, best, arg)) {
        best = a;
        arg = j;
      }
    }
  }
  // the four lane groups of a row, then the four waves
#pragma unroll
  for (int o = 16; o < BL_WAVE; o <<= 1) {
    const double ob = __shfl_xor(best, o, BL_WAVE);
    const int oa = __shfl_xor(arg, o, BL_WAVE);
    if (oa >= 0 && tk_better(ob, oa, best, arg)) {
      best = ob;
      arg = oa;
    }
  }
  if (group == 0) {
    s_best[wave][col] = best;
    s_arg[wave][col] = arg;
  }
  __syncthreads();
  if (tid < TK_TILE && r0 + tid < cx) {
    best = s_best[0][tid];
    arg = s_arg[0][tid];
#pragma unroll
    for (int w = 1; w < TK_WAVES; ++w) {
      const double ob = s_best[w][tid];
      const int oa = s_arg[w][tid];
      if (oa >= 0 && tk_better(ob, oa, best, arg)) {
        best = ob;
        arg = oa;
      }
    }
    part_best[(int64_t)s * cap + r0 + tid] = best;  // by PLACE in the list: r0 + tid < cx <= cap
    part_arg[(int64_t)s * cap + r0 + tid] = arg;
  }
}

__global__ __launch_bounds__(TK_THREADS) void tk_merge_kernel(const double* __restrict__ part_best, const int32_t* __restrict__ part_arg,
                                                              const int32_t* __restrict__ listx, const int32_t* __restrict__ ctrl, int side_x,
                                                              int S, int64_t cap, double* __restrict__ best, int32_t* __restrict__ arg) {
  if (ctrl[TK_ENDED] != 0) return;
  const int64_t p = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (p >= ctrl[TK_COUNT + side_x]) return;
  double b = -2.0;
  int c = -1;
  for (int s = 0; s < S; ++s) {
    const double ob = part_best[(int64_t)s * cap + p];
    const int oa = part_arg[(int64_t)s * cap + p];
    if (oa >= 0 && tk_better(ob, oa, b, c)) {
      b = ob;
      c = oa;
    }
  }
  const int row = listx[p];  // the result goes to the row's own index
  best[row] = c >= 0 ? b : -2.0;
  arg[row] = c;
}

__global__ __launch_bounds__(TK_THREADS) void tk_fill_kernel(int64_t X, double* __restrict__ best, int32_t* __restrict__ arg) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= X) return;
  best[i] = -2.0;
  arg[i] = -1;
}

// ---- the pairs that chose each other ----
__global__ __launch_bounds__(TK_THREADS) void tk_mutual_kernel(const int32_t* __restrict__ list_new, const int32_t* __restrict__ ctrl,
                                                               const double* __restrict__ best_new, const int32_t* __restrict__ arg_new,
                                                               const int32_t* __restrict__ arg_old, int64_t L, int32_t* __restrict__ match_old,
                                                               int32_t* __restrict__ match_new, double* __restrict__ match_aff) {
  if (ctrl[TK_ENDED] != 0) return;
  const int64_t p = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (p >= ctrl[TK_COUNT + 1]) return;
  const int j = list_new[p];
  const int i = arg_new[j];
  if (i < 0 || (int64_t)i >= L) return;  // nothing admissible (or garbage, which is never an address)
  if (arg_old[i] != j) return;           // i is open, so this round wrote its choice
  match_old[i] = j;                      // one thread per pair: j is this thread's alone, and i chose only j
  match_new[j] = i;
  match_aff[j] = best_new[j];
}

inline bool tk_dp_ok(int32_t Dp) { return Dp >= 64 && Dp % 64 == 0; }
inline bool tk_ld_ok(int64_t ld, int32_t Dp) { return ld >= Dp && ld % 16 == 0; }
inline bool tk_floor_ok(double f) { return f > 0.0 && f <= 1.0; }  // false for NaN
inline int64_t tk_up8(int64_t v) { return (v + 7) / 8 * 8; }

// one direction: best + merge.  X is side `side_x` of the control words
inline int tk_direction(const char* what, const int8_t* qx, int64_t ldx, const int32_t* nx, const int32_t* keyx, const int32_t* listx,
                        int64_t X, const int8_t* qy, int64_t ldy, const int32_t* ny, const int32_t* keyy, const int32_t* listy,
                        const int32_t* ctrl, int side_x, int Dp, int S, double floor, double* part_best, int32_t* part_arg, double* best,
                        int32_t* arg, hipStream_t st) {
  hipLaunchKernelGGL(tk_best_kernel, dim3((unsigned)((X + TK_TILE - 1) / TK_TILE), (unsigned)S), dim3(TK_THREADS), 0, st, qx, ldx, nx, keyx, listx,
                     qy, ldy, ny, keyy, listy, ctrl, side_x, Dp, S, floor, X, part_best, part_arg);
  BL_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(tk_merge_kernel, dim3((unsigned)((X + TK_THREADS - 1) / TK_THREADS)), dim3(TK_THREADS), 0, st, part_best, part_arg, listx, ctrl,
                     side_x, S, X, best, arg);
  BL_LAUNCH_CHECK(what);
  return BL_OK;
}
}  // namespace

// the checks both entry points share; `what` names the caller
#define TK_CHECK_IMAGES(what)                                                                                                              \
  BL_CHECK_ARG(L >= 0 && N >= 0, what ": negative size (%lld, %lld)", (long long)L, (long long)N);                                         \
  BL_CHECK_ARG(tk_dp_ok(Dp), what ": Dp = %d must be a positive multiple of 64", (int)Dp);                                                 \
  BL_CHECK_RANGE(Dp <= BL_SIM_MAX_D, what ": Dp = %d is above BL_SIM_MAX_D = %d", (int)Dp, BL_SIM_MAX_D);                                  \
  BL_CHECK_RANGE(L <= BL_REVIEW_MAX_ROWS && N <= BL_REVIEW_MAX_ROWS, what ": %lld or %lld rows are above BL_REVIEW_MAX_ROWS = %d",         \
                 (long long)L, (long long)N, BL_REVIEW_MAX_ROWS);                                                                          \
  BL_CHECK_ARG(tk_floor_ok(floor), what ": floor = %g must be in (0, 1]: the square of a similarity in (0, 1]", floor);                    \
  BL_CHECK_ARG(slices >= 1 && slices <= BL_TRACK_MAX_SLICES, what ": slices = %d must be in [1, %d]", (int)slices, BL_TRACK_MAX_SLICES);   \
  BL_CHECK_ARG(tk_ld_ok(ld_old, Dp) && tk_ld_ok(ld_new, Dp), what ": the row strides %lld / %lld must be multiples of 16 and at least Dp = %d", \
               (long long)ld_old, (long long)ld_new, (int)Dp);                                                                             \
  BL_CHECK_ARG((key_old == nullptr) == (key_new == nullptr), what ": the keys of both sides come together");                               \
  BL_CHECK_ARG(L == 0 || (q_old && n_old), what ": null image / norms of the first side");                                                 \
  BL_CHECK_ARG(N == 0 || (q_new && n_new), what ": null image / norms of the second side");                                                \
  BL_CHECK_ARG((L == 0 || bl_aligned16(q_old)) && (N == 0 || bl_aligned16(q_new)), what ": the int8 images must be 16-byte aligned")

extern "C" int64_t bl_track_best_workspace_bytes(int64_t X, int64_t Y, int32_t slices) {
  if (X < 0 || Y < 0 || X > BL_REVIEW_MAX_ROWS || Y > BL_REVIEW_MAX_ROWS || slices < 1 || slices > BL_TRACK_MAX_SLICES) return -1;
  // control | the partial affinities (fp64) | the partial choices, the two lists (int32)
  return TK_CTRL_BYTES + X * (int64_t)slices * 8 + tk_up8(4 * (X * (int64_t)slices + X + Y));
}

extern "C" int bl_track_best_i8(const int8_t* q_old, int64_t ld_old, const int32_t* n_old, const int32_t* key_old, const uint8_t* open_old,
                                int64_t L, const int8_t* q_new, int64_t ld_new, const int32_t* n_new, const int32_t* key_new,
                                const uint8_t* open_new, int64_t N, int32_t Dp, double floor, int32_t slices, void* workspace,
                                int64_t workspace_bytes, double* best, int32_t* arg, void* stream) {
  TK_CHECK_IMAGES("bl_track_best_i8");
  BL_CHECK_ARG(L == 0 || (best && arg), "bl_track_best_i8: null best / arg");
  BL_CHECK_ARG(L == 0 || ((uintptr_t)best & 7) == 0, "bl_track_best_i8: best must be 8-byte aligned");
  const int64_t need = bl_track_best_workspace_bytes(L, N, slices);
  BL_CHECK_ARG(L == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "bl_track_best_i8: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need, (long long)workspace_bytes);
  if (L == 0) return BL_OK;
  hipStream_t st = (hipStream_t)stream;
  int32_t* ctrl = (int32_t*)workspace;
  double* part_best = (double*)((char*)workspace + TK_CTRL_BYTES);
  int32_t* part_arg = (int32_t*)(part_best + L * (int64_t)slices);
  int32_t* list_x = part_arg + L * (int64_t)slices;
  int32_t* list_y = list_x + L;
  const tk_side sx = {nullptr, list_x, open_old, nullptr, (int32_t)L}, sy = {nullptr, list_y, open_new, nullptr, (int32_t)N};
  hipLaunchKernelGGL(tk_compact_kernel, dim3(2), dim3(TK_SCAN_THREADS), 0, st, sx, sy, 1, (const int32_t*)nullptr, ctrl, (int32_t*)nullptr);
  BL_LAUNCH_CHECK("bl_track_best_i8 (lists)");
  hipLaunchKernelGGL(tk_fill_kernel, dim3((unsigned)((L + TK_THREADS - 1) / TK_THREADS)), dim3(TK_THREADS), 0, st, L, best, arg);
  BL_LAUNCH_CHECK("bl_track_best_i8 (fill)");
  return tk_direction("bl_track_best_i8", q_old, ld_old, n_old, key_old, list_x, L, q_new, ld_new, n_new, key_new, list_y, ctrl, 0, (int)Dp,
                      (int)slices, floor, part_best, part_arg, best, arg, st);
}

extern "C" int64_t bl_track_match_workspace_bytes(int64_t L, int64_t N, int32_t slices) {
  if (L < 0 || N < 0 || L > BL_REVIEW_MAX_ROWS || N > BL_REVIEW_MAX_ROWS || slices < 1 || slices > BL_TRACK_MAX_SLICES) return -1;
  // control | per row: best and the partial affinities (fp64) | per row: arg, the partial choices, two lists (int32)
  return TK_CTRL_BYTES + (L + N) * (int64_t)(8 + 8 * slices) + tk_up8((L + N) * (int64_t)(4 + 4 * slices + 8));
}

extern "C" int bl_track_match(const int8_t* q_old, int64_t ld_old, const int32_t* n_old, const int32_t* key_old, int64_t L,
                              const int8_t* q_new, int64_t ld_new, const int32_t* n_new, const int32_t* key_new, int64_t N, int32_t Dp,
                              double floor, int32_t max_rounds, int32_t slices, void* workspace, int64_t workspace_bytes, int32_t* match_old,
                              int32_t* match_new, double* match_aff, int32_t* status, void* stream) {
  TK_CHECK_IMAGES("bl_track_match");
  BL_CHECK_ARG(max_rounds >= 1, "bl_track_match: max_rounds = %d must be at least 1", (int)max_rounds);
  BL_CHECK_RANGE(max_rounds <= BL_TRACK_MAX_ROUNDS, "bl_track_match: max_rounds = %d is above BL_TRACK_MAX_ROUNDS = %d", (int)max_rounds,
                 BL_TRACK_MAX_ROUNDS);
  BL_CHECK_ARG(status != nullptr, "bl_track_match: null status");
  BL_CHECK_ARG((L == 0 || match_old) && (N == 0 || (match_new && match_aff)), "bl_track_match: null match_old / match_new / match_aff");
  BL_CHECK_ARG(N == 0 || ((uintptr_t)match_aff & 7) == 0, "bl_track_match: match_aff must be 8-byte aligned");
  const int64_t need = bl_track_match_workspace_bytes(L, N, slices);
  BL_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
               "bl_track_match: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", (long long)need, (long long)workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = slices;
  int32_t* ctrl = (int32_t*)workspace;
  double* best_old = (double*)((char*)workspace + TK_CTRL_BYTES);
  double* best_new = best_old + L;
  double* pb_old = best_new + N;
  double* pb_new = pb_old + S * L;
  int32_t* arg_old = (int32_t*)(pb_new + S * N);
  int32_t* arg_new = arg_old + L;
  int32_t* pa_old = arg_new + N;
  int32_t* pa_new = pa_old + S * L;
  int32_t* list_old = pa_new + S * N;  // two lists of L
  int32_t* list_new = list_old + 2 * L;  // two lists of N

  // the open rows of the state that came in: control set 0, lists 0
  {
    const tk_side so = {nullptr, list_old, nullptr, match_old, (int32_t)L}, sn = {nullptr, list_new, nullptr, match_new, (int32_t)N};
    hipLaunchKernelGGL(tk_compact_kernel, dim3(2), dim3(TK_SCAN_THREADS), 0, st, so, sn, 1, (const int32_t*)nullptr, ctrl, status);
    BL_LAUNCH_CHECK("bl_track_match (lists)");
  }
  if (L == 0 || N == 0) {  // nothing can match: one empty round ends it, on the device as everywhere else
    const tk_side so = {list_old, list_old + L, nullptr, match_old, (int32_t)L}, sn = {list_new, list_new + N, nullptr, match_new, (int32_t)N};
    hipLaunchKernelGGL(tk_compact_kernel, dim3(2), dim3(TK_SCAN_THREADS), 0, st, so, sn, 0, (const int32_t*)ctrl, ctrl + TK_CTRL_WORDS, status);
    BL_LAUNCH_CHECK("bl_track_match (lists)");
    return BL_OK;
  }
  for (int r = 0; r < max_rounds; ++r) {
    const int in = r & 1, out = in ^ 1;
    const int32_t* c = ctrl + in * TK_CTRL_WORDS;
    const int32_t* lo = list_old + in * L;
    const int32_t* ln = list_new + in * N;
    int rc = tk_direction("bl_track_match (old)", q_old, ld_old, n_old, key_old, lo, L, q_new, ld_new, n_new, key_new, ln, c, 0, (int)Dp,
                          (int)slices, floor, pb_old, pa_old, best_old, arg_old, st);
    if (rc != BL_OK) return rc;
    rc = tk_direction("bl_track_match (new)", q_new, ld_new, n_new, key_new, ln, N, q_old, ld_old, n_old, key_old, lo, c, 1, (int)Dp, (int)slices,
                      floor, pb_new, pa_new, best_new, arg_new, st);
    if (rc != BL_OK) return rc;
    hipLaunchKernelGGL(tk_mutual_kernel, dim3((unsigned)((N + TK_THREADS - 1) / TK_THREADS)), dim3(TK_THREADS), 0, st, ln, c,
                       (const double*)best_new, (const int32_t*)arg_new, (const int32_t*)arg_old, L, match_old, match_new, match_aff);
    BL_LAUNCH_CHECK("bl_track_match (mutual)");
    const tk_side so = {lo, list_old + out * L, nullptr, match_old, (int32_t)L}, sn = {ln, list_new + out * N, nullptr, match_new, (int32_t)N};
    hipLaunchKernelGGL(tk_compact_kernel, dim3(2), dim3(TK_SCAN_THREADS), 0, st, so, sn, 0, c, ctrl + out * TK_CTRL_WORDS, status);
    BL_LAUNCH_CHECK("bl_track_match (lists)");
  }
  return BL_OK;
}
