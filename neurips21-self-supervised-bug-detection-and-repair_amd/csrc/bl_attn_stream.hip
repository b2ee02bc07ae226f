// Streaming (online-softmax) relational self-attention: `seq-great` / `seq-transformer` without any [L, L] array in memory
// (reference multihead_attention.py:46-80 with the edge terms of relational_multihead_attention.py:72-152, mode 0, no value
// biases).  Same arithmetic as the stored-P path of bl_seq_ops.hip: q pre-scaled by dk^-1/2, score = q_i.k_j + sum over the row's
// CSR entries at key j of <q_i, bias[code]>, keys >= lens[b] masked, softmax, nn.Dropout on the probabilities (counter hash at
// row * L + key), ctx = Pd.V -- but the probabilities live one 64-key tile at a time in registers:
//   forward    one workgroup per (sample, head, 32 query rows); a wave owns 8 rows, a lane one key of the tile.  Running row
//              maximum m, running sum l and the rescaled accumulator (lane = channel, the two half-waves split the tile's keys);
//              writes ctx and lse = m + log l per row.
//   backward   the probability tile is recomputed from q, k, the entries and lse.  dS = P (mask dPd / (1 - p) - delta),
//              delta_i = sum_j P_ij mask dPd_ij / (1 - p), summed from the recomputed tiles in a sweep of its own -- NOT the identity
//              delta_i = dO_i . ctx_i: where a row's probability is one-hot, dPd_j - delta cancels exactly with the sum (P_j = 1.0)
//              and only to the rounding of the stored fp32 ctx with the identity, an absolute error in dS that a large key or bias
//              row multiplies into dQ (measured 9 x the stored-P path's error on such a row).
//                dq kernel    same decomposition as the forward, two sweeps over the key tiles: delta (written out for the dkv
//                             kernel), then dQ = (dS.K + sum dS_ij bias[code]) scale and the bias tables' gradients sum dS_ij q_i
//                             (registers per wave -> LDS per workgroup -> one atomic per element);
//                dkv kernel   one workgroup per (sample, head, 64 keys): a lane holds its key's k and v rows and its dK / dV rows
//                             in registers, the waves split the query rows and are summed in wave order through LDS.
//              No float atomics on dQ / dK / dV / ctx: every output row has one owner and a fixed order of additions.
// All products are fp32 FMAs on the vector unit, every sum over dk runs d = 0 .. 31 in the three kernels alike, so the three
// recompute the same score bits.  Nothing in LDS or registers scales with L.  The CSR entries of a row are in edge-list order:
// each kernel picks the entries of the current key tile itself (ballot over 64 entries at a time), in list order, so repeated
// (row, key) entries add up exactly as in the row-wise kernels.
#include "bl_common.h"

#define ST_NEG_INF (-__builtin_huge_valf())
#define ST_LOG2E 1.44269504088896340736f
#define ST_DK 32          // head dimension
#define ST_BN 64          // keys per tile = lanes of a wave
#define ST_R 8            // query rows per wave
#define ST_WAVES 4
#define ST_BM (ST_R * ST_WAVES)  // query rows per workgroup
#define ST_LD (ST_DK + 1)        // row stride of the LDS tiles: lane j reads row j, lane d reads column d, both conflict-free
#define ST_MAX_CODES 32          // 2 T <= 32 (2 T dk <= 1024: the dq kernel keeps the bias-gradient table in 16 registers per lane)
#define ST_TAB_REGS 16

struct StView {  // bl_head_view_t on the device
  float* p;
  long long sb;
  int sh, sl;
};
__device__ __forceinline__ float* st_mat(const StView& v, int b, int h) { return v.p + (size_t)b * v.sb + (size_t)h * v.sh; }
__device__ __forceinline__ float st_rl(float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); }

// f(key - j0, code) for the entries of one query row whose key lies in [j0, j0 + 64), in list order.  (key0, code0): the row's
// first 64 entries, one per lane (-1 beyond the row's count).  Everything about an entry is wave-uniform.
template <class F>
__device__ __forceinline__ void st_tile_entries(const int* __restrict__ ekey, const int* __restrict__ ecode, int ebeg, int cnt, int key0,
                                                int code0, int j0, int lane, F f) {
  for (int base = 0; base < cnt; base += 64) {
    int key = key0, code = code0;
    if (base > 0) {
      const int p = base + lane;
      key = p < cnt ? ekey[ebeg + p] : -1;
      code = p < cnt ? ecode[ebeg + p] : 0;
    }
    unsigned long long mask = __ballot(key >= j0 && key < j0 + ST_BN);
    while (mask) {
      const int pl = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
      mask &= mask - 1;
      f(__builtin_amdgcn_readlane(key, pl) - j0, __builtin_amdgcn_readlane(code, pl) & 63);
    }
  }
}

// K / V rows j0 .. j0 + 63 of one head into [64][ST_LD] (zeros beyond L)
__device__ __forceinline__ void st_stage_tile(float* __restrict__ dst, const float* __restrict__ src, int sl, int j0, int L, int tid) {
  for (int x = tid; x < ST_BN * (ST_DK / 4); x += 64 * ST_WAVES) {
    const int j = x >> 3, d = 4 * (x & 7);
    const float4 t = j0 + j < L ? *reinterpret_cast<const float4*>(src + (size_t)(j0 + j) * sl + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    float* o = dst + j * ST_LD + d;
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  }
}
__device__ __forceinline__ void st_stage_bias(float* __restrict__ bl, const float* __restrict__ bias_f, const float* __restrict__ bias_r, int T,
                                              int H, int h, int tid) {
  for (int x = tid; x < 2 * T * ST_DK; x += 64 * ST_WAVES) {
    const int c = x >> 5, d = x & 31;
    bl[c * ST_LD + d] = ((c & 1) ? bias_r : bias_f)[(size_t)(c >> 1) * H * ST_DK + h * ST_DK + d];
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * ST_WAVES) void attn_stream_fwd_kernel(const StView q, const float q_scale, const StView k, const StView v,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ ekey,
                                                                        const int* __restrict__ ecode, int L, int H, int T,
                                                                        const float* __restrict__ bias_f, const float* __restrict__ bias_r,
                                                                        const int* __restrict__ lens, bl_drop_dev drop, int has_drop,
                                                                        const StView out, float* __restrict__ lse) {
  __shared__ float Ks[ST_BN * ST_LD], Vs[ST_BN * ST_LD], bl[ST_MAX_CODES * ST_LD];
  __shared__ __attribute__((aligned(16))) float ps[ST_WAVES][ST_R][ST_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, b = g / H, h = g - b * H;
  const int i0 = blockIdx.y * ST_BM + wave * ST_R;
  const int n = min(lens[b], L);
  const float* __restrict__ qg = st_mat(q, b, h);
  const float* __restrict__ kg = st_mat(k, b, h);
  const float* __restrict__ vg = st_mat(v, b, h);
  if (row_ptr) st_stage_bias(bl, bias_f, bias_r, T, H, h, tid);
  float qv[ST_R], tv[ST_R], m[ST_R], l[ST_R], acc[ST_R];
  int ebeg[ST_R], ecnt[ST_R], ek[ST_R], ec[ST_R];
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    const int i = i0 + r;
    qv[r] = qg[(size_t)min(i, L - 1) * q.sl + (lane & 31)] * q_scale;
    ebeg[r] = (row_ptr && i < L) ? row_ptr[b * L + i] : 0;
    ecnt[r] = (row_ptr && i < L) ? row_ptr[b * L + i + 1] - ebeg[r] : 0;
    ek[r] = lane < ecnt[r] ? ekey[ebeg[r] + lane] : -1;
    ec[r] = lane < ecnt[r] ? ecode[ebeg[r] + lane] : 0;
    m[r] = ST_NEG_INF;
    l[r] = 0.f;
    acc[r] = 0.f;
    tv[r] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    if (ecnt[r] > 0 && lane < 2 * T) {  // lane c: <bias[c][h, :], q_i>
      float t = 0.f;
#pragma unroll
      for (int d = 0; d < ST_DK; ++d) t = fmaf(bl[lane * ST_LD + d], st_rl(qv[r], d), t);
      tv[r] = t;
    }
  }
  const int hf = lane >> 5, dch = lane & 31;
  for (int j0 = 0; j0 < n; j0 += ST_BN) {  // (tiles of padding keys only are never visited)
    __syncthreads();
    st_stage_tile(Ks, kg, k.sl, j0, L, tid);
    st_stage_tile(Vs, vg, v.sl, j0, L, tid);
    __syncthreads();
    float s[ST_R];
#pragma unroll
    for (int r = 0; r < ST_R; ++r) s[r] = 0.f;
#pragma unroll 8
    for (int d = 0; d < ST_DK; ++d) {
      const float kd = Ks[lane * ST_LD + d];
#pragma unroll
      for (int r = 0; r < ST_R; ++r) s[r] = fmaf(st_rl(qv[r], d), kd, s[r]);
    }
    const bool valid = j0 + lane < n;
#pragma unroll
    for (int r = 0; r < ST_R; ++r) {
      if (ecnt[r] > 0) {
        float sr = s[r];
        const float tr = tv[r];
        st_tile_entries(ekey, ecode, ebeg[r], ecnt[r], ek[r], ec[r], j0, lane, [&](int kk, int cc) { sr += lane == kk ? st_rl(tr, cc) : 0.f; });
        s[r] = sr;
      }
      const float sm = valid ? s[r] : ST_NEG_INF;
      const float mn = fmaxf(m[r], bl_wave_max(sm));  // finite: key j0 of the tile is valid
      const float alpha = __builtin_amdgcn_exp2f((m[r] - mn) * ST_LOG2E);  // first tile: 2^-inf = 0
      float p = valid ? __builtin_amdgcn_exp2f((sm - mn) * ST_LOG2E) : 0.f;
      l[r] = l[r] * alpha + bl_wave_sum(p);
      acc[r] *= alpha;
      m[r] = mn;
      if (has_drop) {
        const uint32_t e = ((uint32_t)g * (uint32_t)L + (uint32_t)min(i0 + r, L - 1)) * (uint32_t)L + (uint32_t)(j0 + lane);
        p = bl_keep(drop, e) ? p * drop.scale : 0.f;
      }
      ps[wave][r][lane] = p;
    }
    __syncthreads();
#pragma unroll 2
    for (int jj = 0; jj < 32; jj += 4) {  // half-wave hf takes the keys 32 hf .. 32 hf + 31 of the tile
      const int j = 32 * hf + jj;
      const float v0 = Vs[j * ST_LD + dch], v1 = Vs[(j + 1) * ST_LD + dch], v2 = Vs[(j + 2) * ST_LD + dch], v3 = Vs[(j + 3) * ST_LD + dch];
#pragma unroll
      for (int r = 0; r < ST_R; ++r) {
        const float4 p4 = *reinterpret_cast<const float4*>(&ps[wave][r][j]);
        acc[r] = fmaf(p4.x, v0, acc[r]);
        acc[r] = fmaf(p4.y, v1, acc[r]);
        acc[r] = fmaf(p4.z, v2, acc[r]);
        acc[r] = fmaf(p4.w, v3, acc[r]);
      }
    }
  }
  float* __restrict__ og = st_mat(out, b, h);
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    const int i = i0 + r;
    const float a = acc[r] + __shfl_xor(acc[r], 32, 64);
    if (i < L) {  // (wave-uniform)
      const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;  // (a sample of length 0 has no keys: zeros)
      if (lane < ST_DK) og[(size_t)i * out.sl + lane] = a * inv;
      if (lane == 0) lse[(size_t)g * L + i] = l[r] > 0.f ? m[r] + logf(l[r]) : 0.f;
    }
  }
}

// ---- backward: dQ, the edge terms' part of it and the bias tables' gradients ---------------------------------------------------------
__global__ __launch_bounds__(64 * ST_WAVES) void attn_stream_dq_kernel(const StView g_ctx, const StView q, const float q_scale,
                                                                       const StView k, const StView v, const float* __restrict__ lse,
                                                                       const int* __restrict__ row_ptr, const int* __restrict__ ekey,
                                                                       const int* __restrict__ ecode, int L, int H, int T,
                                                                       const float* __restrict__ bias_f, const float* __restrict__ bias_r,
                                                                       const int* __restrict__ lens, bl_drop_dev drop, int has_drop,
                                                                       float* __restrict__ delta, const StView g_q,
                                                                       float* __restrict__ g_bias_f, float* __restrict__ g_bias_r) {
  __shared__ float Ks[ST_BN * ST_LD], Vs[ST_BN * ST_LD], bl[ST_MAX_CODES * ST_LD], tab[ST_MAX_CODES * ST_DK];
  __shared__ __attribute__((aligned(16))) float ps[ST_WAVES][ST_R][ST_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, b = g / H, h = g - b * H;
  const int i0 = blockIdx.y * ST_BM + wave * ST_R;
  const int n = min(lens[b], L);
  const int ntab = 2 * T * ST_DK;
  const float* __restrict__ qg = st_mat(q, b, h);
  const float* __restrict__ kg = st_mat(k, b, h);
  const float* __restrict__ vg = st_mat(v, b, h);
  const float* __restrict__ gog = st_mat(g_ctx, b, h);
  if (row_ptr) {
    st_stage_bias(bl, bias_f, bias_r, T, H, h, tid);
    for (int x = tid; x < ntab; x += 64 * ST_WAVES) tab[x] = 0.f;
  }
  float qv[ST_R], gv[ST_R], tv[ST_R], dlt[ST_R], ls[ST_R], acc[ST_R], coef[ST_R];
  int ebeg[ST_R], ecnt[ST_R], ek[ST_R], ec[ST_R];
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    const int i = i0 + r, ic = min(i, L - 1);
    qv[r] = qg[(size_t)ic * q.sl + (lane & 31)] * q_scale;
    gv[r] = (i < L && lane < ST_DK) ? gog[(size_t)ic * g_ctx.sl + lane] : 0.f;  // (rows beyond L: dS = 0)
    dlt[r] = 0.f;
    ls[r] = lse[(size_t)g * L + ic];
    ebeg[r] = (row_ptr && i < L) ? row_ptr[b * L + i] : 0;
    ecnt[r] = (row_ptr && i < L) ? row_ptr[b * L + i + 1] - ebeg[r] : 0;
    ek[r] = lane < ecnt[r] ? ekey[ebeg[r] + lane] : -1;
    ec[r] = lane < ecnt[r] ? ecode[ebeg[r] + lane] : 0;
    acc[r] = 0.f;
    coef[r] = 0.f;
    tv[r] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    if (ecnt[r] > 0 && lane < 2 * T) {
      float t = 0.f;
#pragma unroll
      for (int d = 0; d < ST_DK; ++d) t = fmaf(bl[lane * ST_LD + d], st_rl(qv[r], d), t);
      tv[r] = t;
    }
  }
  const int hf = lane >> 5, dch = lane & 31;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {  // 0: delta;  1: dS and what is made of it
  for (int j0 = 0; j0 < n; j0 += ST_BN) {
    __syncthreads();
    st_stage_tile(Ks, kg, k.sl, j0, L, tid);
    st_stage_tile(Vs, vg, v.sl, j0, L, tid);
    __syncthreads();
    float s[ST_R], dp[ST_R];
#pragma unroll
    for (int r = 0; r < ST_R; ++r) s[r] = dp[r] = 0.f;
#pragma unroll 8
    for (int d = 0; d < ST_DK; ++d) {
      const float kd = Ks[lane * ST_LD + d], vd = Vs[lane * ST_LD + d];
#pragma unroll
      for (int r = 0; r < ST_R; ++r) {
        s[r] = fmaf(st_rl(qv[r], d), kd, s[r]);
        dp[r] = fmaf(st_rl(gv[r], d), vd, dp[r]);
      }
    }
    const bool valid = j0 + lane < n;
#pragma unroll
    for (int r = 0; r < ST_R; ++r) {
      if (ecnt[r] > 0) {
        float sr = s[r];
        const float tr = tv[r];
        st_tile_entries(ekey, ecode, ebeg[r], ecnt[r], ek[r], ec[r], j0, lane, [&](int kk, int cc) { sr += lane == kk ? st_rl(tr, cc) : 0.f; });
        s[r] = sr;
      }
      const float p = valid ? __builtin_amdgcn_exp2f((s[r] - ls[r]) * ST_LOG2E) : 0.f;
      float dpd = dp[r];
      if (has_drop) {
        const uint32_t e = ((uint32_t)g * (uint32_t)L + (uint32_t)min(i0 + r, L - 1)) * (uint32_t)L + (uint32_t)(j0 + lane);
        dpd = bl_keep(drop, e) ? dpd * drop.scale : 0.f;
      }
      if (pass == 0) {
        dlt[r] += bl_wave_sum(p * dpd);  // (tiles in order, lanes in the order of the wave sum: the same bits every run)
        continue;
      }
      const float ds = p * (dpd - dlt[r]);
      ps[wave][r][lane] = ds;
      if (ecnt[r] > 0) {
        float cf = coef[r];
        st_tile_entries(ekey, ecode, ebeg[r], ecnt[r], ek[r], ec[r], j0, lane, [&](int kk, int cc) {
          const float gval = st_rl(ds, kk);
          cf += lane == cc ? gval : 0.f;
        });
        coef[r] = cf;
      }
    }
    if (pass == 0) continue;  // (uniform)
    __syncthreads();
#pragma unroll 2
    for (int jj = 0; jj < 32; jj += 4) {
      const int j = 32 * hf + jj;
      const float k0 = Ks[j * ST_LD + dch], k1 = Ks[(j + 1) * ST_LD + dch], k2 = Ks[(j + 2) * ST_LD + dch], k3 = Ks[(j + 3) * ST_LD + dch];
#pragma unroll
      for (int r = 0; r < ST_R; ++r) {
        const float4 p4 = *reinterpret_cast<const float4*>(&ps[wave][r][j]);
        acc[r] = fmaf(p4.x, k0, acc[r]);
        acc[r] = fmaf(p4.y, k1, acc[r]);
        acc[r] = fmaf(p4.z, k2, acc[r]);
        acc[r] = fmaf(p4.w, k3, acc[r]);
      }
    }
  }
    if (pass == 0 && lane == 0) {
#pragma unroll
      for (int r = 0; r < ST_R; ++r)
        if (i0 + r < L) delta[(size_t)g * L + i0 + r] = dlt[r];
    }
  }
  float* __restrict__ gqg = st_mat(g_q, b, h);
  float tabacc[ST_TAB_REGS];
#pragma unroll
  for (int kk = 0; kk < ST_TAB_REGS; ++kk) tabacc[kk] = 0.f;
  bool any_edges = false;
#pragma unroll
  for (int r = 0; r < ST_R; ++r) {
    const int i = i0 + r;
    float a = acc[r] + __shfl_xor(acc[r], 32, 64);
    if (ecnt[r] > 0) {  // (wave-uniform)
      any_edges = true;
      float gq = 0.f;
      for (int c = 0; c < 2 * T; ++c) gq = fmaf(st_rl(coef[r], c), bl[c * ST_LD + dch], gq);
      a += gq;
#pragma unroll
      for (int kk = 0; kk < ST_TAB_REGS; ++kk) {
        if (64 * kk < ntab) {  // element (code, d) = (e / 32, e % 32) of the table, e = lane + 64 kk: e % 32 == lane % 32
          const int e = lane + 64 * kk;
          const float cv = __shfl(coef[r], min(e >> 5, 63), 64);
          if (e < ntab) tabacc[kk] = fmaf(cv, qv[r], tabacc[kk]);
        }
      }
    }
    if (i < L && lane < ST_DK) gqg[(size_t)i * g_q.sl + lane] = a * q_scale;
  }
  if (row_ptr) {
    if (any_edges) {
#pragma unroll
      for (int kk = 0; kk < ST_TAB_REGS; ++kk) {
        const int e = lane + 64 * kk;
        if (e < ntab && tabacc[kk] != 0.f) atomicAdd(&tab[e], tabacc[kk]);
      }
    }
    __syncthreads();
    for (int x = tid; x < ntab; x += 64 * ST_WAVES) {
      const float val = tab[x];
      if (val != 0.f) {
        const int c = x >> 5, d = x & 31;
        unsafeAtomicAdd(((c & 1) ? g_bias_r : g_bias_f) + (size_t)(c >> 1) * H * ST_DK + h * ST_DK + d, val);
      }
    }
  }
}

// ---- backward: dK = dS^T.Q and dV = Pd^T.dO -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * ST_WAVES) void attn_stream_dkv_kernel(const StView g_ctx, const StView q, const float q_scale, const StView k,
                                                                        const StView v, const float* __restrict__ lse,
                                                                        const float* __restrict__ delta,
                                                                        const int* __restrict__ row_ptr, const int* __restrict__ ekey,
                                                                        const int* __restrict__ ecode, int L, int H, int T,
                                                                        const float* __restrict__ bias_f, const float* __restrict__ bias_r,
                                                                        const int* __restrict__ lens, bl_drop_dev drop, int has_drop,
                                                                        const StView g_k, const StView g_v) {
  __shared__ __attribute__((aligned(16))) float Qs[ST_BM * ST_DK], Gs[ST_BM * ST_DK];
  __shared__ float lss[ST_BM], dls[ST_BM], bl[ST_MAX_CODES * ST_LD], red[ST_WAVES * ST_BN * ST_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, b = g / H, h = g - b * H;
  const int j0 = blockIdx.y * ST_BN, jkey = j0 + lane;
  const int n = min(lens[b], L);
  float* __restrict__ gkg = st_mat(g_k, b, h);
  float* __restrict__ gvg = st_mat(g_v, b, h);
  if (j0 >= n) {  // a tile of padding keys: P = 0 there
    for (int x = tid; x < ST_BN * ST_DK; x += 64 * ST_WAVES) {
      const int j = j0 + (x >> 5), d = x & 31;
      if (j < L) {
        gkg[(size_t)j * g_k.sl + d] = 0.f;
        gvg[(size_t)j * g_v.sl + d] = 0.f;
      }
    }
    return;
  }
  const float* __restrict__ qg = st_mat(q, b, h);
  const float* __restrict__ gog = st_mat(g_ctx, b, h);
  if (row_ptr) st_stage_bias(bl, bias_f, bias_r, T, H, h, tid);
  float kr[ST_DK], vr[ST_DK], dk_acc[ST_DK], dv_acc[ST_DK];
  {
    const float* __restrict__ kp = st_mat(k, b, h) + (size_t)min(jkey, L - 1) * k.sl;
    const float* __restrict__ vp = st_mat(v, b, h) + (size_t)min(jkey, L - 1) * v.sl;
#pragma unroll
    for (int d = 0; d < ST_DK; d += 4) {
      const float4 a = *reinterpret_cast<const float4*>(kp + d), c = *reinterpret_cast<const float4*>(vp + d);
      kr[d] = a.x; kr[d + 1] = a.y; kr[d + 2] = a.z; kr[d + 3] = a.w;
      vr[d] = c.x; vr[d + 1] = c.y; vr[d + 2] = c.z; vr[d + 3] = c.w;
    }
#pragma unroll
    for (int d = 0; d < ST_DK; ++d) dk_acc[d] = dv_acc[d] = 0.f;
  }
  const bool valid = jkey < n;
  for (int it0 = 0; it0 < L; it0 += ST_BM) {
    __syncthreads();
    {  // stage 32 query rows: q * scale, dO, lse, delta (thread = (row, 4 channels))
      const int r = tid >> 3, d = 4 * (tid & 7), i = it0 + r;
      float4 qq = make_float4(0.f, 0.f, 0.f, 0.f), gg = qq;
      if (i < L) {
        qq = *reinterpret_cast<const float4*>(qg + (size_t)i * q.sl + d);
        gg = *reinterpret_cast<const float4*>(gog + (size_t)i * g_ctx.sl + d);
      }
      qq.x *= q_scale; qq.y *= q_scale; qq.z *= q_scale; qq.w *= q_scale;
      *reinterpret_cast<float4*>(Qs + r * ST_DK + d) = qq;
      *reinterpret_cast<float4*>(Gs + r * ST_DK + d) = gg;
      if ((tid & 7) == 0) {
        dls[r] = i < L ? delta[(size_t)g * L + i] : 0.f;
        lss[r] = i < L ? lse[(size_t)g * L + i] : 0.f;
      }
    }
    __syncthreads();
    for (int rr = 0; rr < ST_R; ++rr) {
      const int r = wave + ST_WAVES * rr, i = it0 + r;
      if (i >= L) break;  // (wave-uniform)
      const float* __restrict__ qr = Qs + r * ST_DK;
      const float* __restrict__ gr = Gs + r * ST_DK;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < ST_DK; ++d) {
        s = fmaf(qr[d], kr[d], s);
        dp = fmaf(gr[d], vr[d], dp);
      }
      if (row_ptr) {
        const int ebeg = row_ptr[b * L + i], cnt = row_ptr[b * L + i + 1] - ebeg;
        if (cnt > 0) {
          const int key0 = lane < cnt ? ekey[ebeg + lane] : -1, code0 = lane < cnt ? ecode[ebeg + lane] : 0;
          float tr = 0.f;
          bool have = false;
          st_tile_entries(ekey, ecode, ebeg, cnt, key0, code0, j0, lane, [&](int kk, int cc) {
            if (!have) {  // (uniform) lane c: <bias[c][h, :], q_i>, same order of the 32 products as the other kernels
              have = true;
              if (lane < 2 * T) {
#pragma unroll
                for (int d = 0; d < ST_DK; ++d) tr = fmaf(bl[lane * ST_LD + d], qr[d], tr);
              }
            }
            s += lane == kk ? st_rl(tr, cc) : 0.f;
          });
        }
      }
      const float p = valid ? __builtin_amdgcn_exp2f((s - lss[r]) * ST_LOG2E) : 0.f;
      float dpd = dp, pd = p;
      if (has_drop) {
        const uint32_t e = ((uint32_t)g * (uint32_t)L + (uint32_t)i) * (uint32_t)L + (uint32_t)jkey;
        const bool keep = bl_keep(drop, e);
        dpd = keep ? dp * drop.scale : 0.f;
        pd = keep ? p * drop.scale : 0.f;
      }
      const float ds = p * (dpd - dls[r]);
#pragma unroll
      for (int d = 0; d < ST_DK; ++d) {
        dk_acc[d] = fmaf(ds, qr[d], dk_acc[d]);
        dv_acc[d] = fmaf(pd, gr[d], dv_acc[d]);
      }
    }
  }
  // the four waves' partial rows, added in wave order
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
#pragma unroll
    for (int d = 0; d < ST_DK; ++d) red[(wave * ST_BN + lane) * ST_LD + d] = which == 0 ? dk_acc[d] : dv_acc[d];
    __syncthreads();
    float* __restrict__ og = which == 0 ? gkg : gvg;
    const int osl = which == 0 ? g_k.sl : g_v.sl;
    for (int x = tid; x < ST_BN * ST_DK; x += 64 * ST_WAVES) {
      const int jl = x >> 5, d = x & 31;
      float t = red[jl * ST_LD + d];
#pragma unroll
      for (int w = 1; w < ST_WAVES; ++w) t += red[(w * ST_BN + jl) * ST_LD + d];
      if (j0 + jl < L) og[(size_t)(j0 + jl) * osl + d] = t;
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
extern "C" int32_t bl_rel_attn_stream_ok(int32_t L, int32_t dk, int32_t T) {
  return (L > 0 && L % 4 == 0 && dk == ST_DK && T > 0 && 2 * T * dk <= 64 * ST_TAB_REGS) ? 1 : 0;
}

static int st_check_view(const char* who, const char* what, const bl_head_view_t* v) {
  BL_CHECK_ARG(v && v->p, "%s: null pointer (%s)", who, what);
  BL_CHECK_ARG(bl_aligned16(v->p) && v->sb % 4 == 0 && v->sh % 4 == 0 && v->sl % 4 == 0,
               "%s: head view %s needs a 16-byte aligned base and strides that are multiples of 4", who, what);
  return BL_OK;
}
static inline StView st_from(const bl_head_view_t* a) {
  StView v = {a->p, (long long)a->sb, a->sh, a->sl};
  return v;
}
static int st_check_common(const char* who, const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                           int32_t dk, int32_t T, const float* bias_f, const float* bias_r, const int32_t* lens, bl_dropout_t drop) {
  BL_CHECK_ARG(bias_f && bias_r && lens, "%s: null pointer (bias_f, bias_r or lens)", who);
  BL_CHECK_ARG((row_ptr == nullptr) == (ekey == nullptr) && (ekey == nullptr) == (ecode == nullptr), "%s: partial edge CSR", who);
  BL_CHECK_ARG(B >= 0 && H > 0, "%s: bad shape B=%d H=%d", who, B, H);
  BL_CHECK_ARG(bl_rel_attn_stream_ok(L, dk, T), "%s: unsupported shape L=%d dk=%d T=%d (L %% 4 == 0, dk == 32, 2 T dk <= 1024)", who, L, dk, T);
  BL_CHECK_ARG((long long)B * H <= 0x7fffffffll && (long long)B * L < 0x7fffffffll, "%s: too many rows (B=%d H=%d L=%d)", who, B, H, L);
  BL_CHECK_ARG(drop.p >= 0.f && drop.p < 1.f, "%s: dropout probability outside [0, 1)", who);
  BL_CHECK_ARG(drop.p <= 0.f || (long long)B * H * L * L < (1ll << 32), "%s: dropout needs fewer than 2^32 scores (B H L^2)", who);
  return BL_OK;
}

extern "C" int bl_rel_attn_stream_fwd(const bl_head_view_t* q, float q_scale, const bl_head_view_t* k, const bl_head_view_t* v,
                                      const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                                      int32_t dk, int32_t T, const float* bias_f, const float* bias_r, const int32_t* lens, bl_dropout_t drop,
                                      const bl_head_view_t* ctx, float* lse, void* stream) {
  const char* who = "bl_rel_attn_stream_fwd";
  int rc = st_check_view(who, "q", q);
  if (rc == BL_OK) rc = st_check_view(who, "k", k);
  if (rc == BL_OK) rc = st_check_view(who, "v", v);
  if (rc == BL_OK) rc = st_check_view(who, "ctx", ctx);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(lse, "%s: null pointer (lse)", who);
  rc = st_check_common(who, row_ptr, ekey, ecode, B, L, H, dk, T, bias_f, bias_r, lens, drop);
  if (rc != BL_OK) return rc;
  if (B == 0) return BL_OK;
  hipLaunchKernelGGL(attn_stream_fwd_kernel, dim3(B * H, (L + ST_BM - 1) / ST_BM), dim3(64 * ST_WAVES), 0, (hipStream_t)stream, st_from(q), q_scale,
                     st_from(k), st_from(v), row_ptr, ekey, ecode, L, H, T, bias_f, bias_r, lens, bl_make_drop(drop), drop.p > 0.f ? 1 : 0,
                     st_from(ctx), lse);
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}

extern "C" int bl_rel_attn_stream_bwd(const bl_head_view_t* g_ctx, const float* lse, const bl_head_view_t* q, float q_scale,
                                      const bl_head_view_t* k, const bl_head_view_t* v, const int32_t* row_ptr, const int32_t* ekey,
                                      const int32_t* ecode, int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T, const float* bias_f,
                                      const float* bias_r, const int32_t* lens, bl_dropout_t drop, float* delta, const bl_head_view_t* g_q,
                                      const bl_head_view_t* g_k, const bl_head_view_t* g_v, float* g_bias_f, float* g_bias_r,
                                      void* stream) {
  const char* who = "bl_rel_attn_stream_bwd";
  const bl_head_view_t* views[7] = {g_ctx, q, k, v, g_q, g_k, g_v};
  const char* names[7] = {"g_ctx", "q", "k", "v", "g_q", "g_k", "g_v"};
  for (int x = 0; x < 7; ++x) {
    const int rc = st_check_view(who, names[x], views[x]);
    if (rc != BL_OK) return rc;
  }
  BL_CHECK_ARG(lse && delta, "%s: null pointer (lse or delta)", who);
  int rc = st_check_common(who, row_ptr, ekey, ecode, B, L, H, dk, T, bias_f, bias_r, lens, drop);
  if (rc != BL_OK) return rc;
  BL_CHECK_ARG(row_ptr == nullptr || (g_bias_f && g_bias_r), "%s: edge entries need g_bias_f and g_bias_r", who);
  if (B == 0) return BL_OK;
  hipStream_t st = (hipStream_t)stream;
  const bl_drop_dev dd = bl_make_drop(drop);
  const int hd = drop.p > 0.f ? 1 : 0;
  hipLaunchKernelGGL(attn_stream_dq_kernel, dim3(B * H, (L + ST_BM - 1) / ST_BM), dim3(64 * ST_WAVES), 0, st, st_from(g_ctx), st_from(q), q_scale,
                     st_from(k), st_from(v), lse, row_ptr, ekey, ecode, L, H, T, bias_f, bias_r, lens, dd, hd, delta, st_from(g_q), g_bias_f,
                     g_bias_r);
  BL_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(attn_stream_dkv_kernel, dim3(B * H, (L + ST_BN - 1) / ST_BN), dim3(64 * ST_WAVES), 0, st, st_from(g_ctx), st_from(q),
                     q_scale, st_from(k), st_from(v), lse, delta, row_ptr, ekey, ecode, L, H, T, bias_f, bias_r, lens, dd, hd, st_from(g_k),
                     st_from(g_v));
  BL_LAUNCH_CHECK(who);
  return BL_OK;
}
