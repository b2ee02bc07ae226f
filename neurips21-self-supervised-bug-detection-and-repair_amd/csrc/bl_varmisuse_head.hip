// GREAT var-misuse head: LayerNorm -> Linear(D, 2) -> localization / repair-pointer losses, metrics kept on the device.
//
// Replaces the tail of reference buglab/models/greatreimplementation.py: `__predictions(__ln_out(state))`, the token and
// candidate masking and the pointer log-softmax (:202-214), the localization cross-entropy, the repair logsumexp over the targets
// and the metric counters (:138-174).  The reference's chain synchronises with the host on every step (int(...) / float(...) on the
// counters, `if num_buggy > 0`, boolean-mask indexing); here nothing is read back until the caller reads `stats`.
//
// Forward, two launches:
//   vm_fwd_rows     one wave per row of x [B * L, D]: LayerNorm statistics and the two logits; writes the masked logits
//                   (-inf at positions >= lens_att, and in the pointer column at non-candidates), mean and rstd;
//   vm_fwd_samples  one workgroup per sample: max / logsumexp / first-index argmax of the localization column over the
//                   unmasked positions, of the pointer column over the candidates, logsumexp over candidates that are targets;
//                   per-sample losses and hits go to the workspace, and the LAST workgroup to arrive (ticket counter) sums
//                   them in sample order into the loss, the device count of buggy samples and the running `stats`.
// Backward, two launches:
//   vm_bwd_rows     a few hundred workgroups, one wave per row at a time: the row's logit gradients from the saved per-sample
//                   logsumexps and the device g_loss, the LayerNorm backward (every row of g_x written, zeros where masked), and
//                   per-workgroup partials of g_W, g_bias, g_ln_g, g_ln_b (fixed wave order through LDS);
//   vm_bwd_reduce   the partials summed in workgroup order.
// Every sum runs in a fixed order, so results are bit-identical from run to run whatever bl_get_deterministic() says.
#include "bl_common.h"
#include "bl_varmisuse_rows.h"  // vm_row_logits, vm_masked_logits, block_argmax, vm_check (shared with bl_varmisuse_predict.hip)

namespace {
constexpr int VM_BWD_THREADS = 512;     // backward rows: 8 waves
constexpr int VM_BWD_WAVES = VM_BWD_THREADS / 64;
constexpr int VM_BWD_MAX_BLOCKS = 512;
constexpr int VM_RED_THREADS = 1024;    // partial reduction: 16 waves x 64 columns
constexpr int VM_RED_WAVES = VM_RED_THREADS / 64;
constexpr int VM_PS = 8;                // per-sample slots in the workspace
constexpr int VM_COUNTER_BYTES = 16;    // ticket counter at the front of the workspace
enum { PS_LOC_LOSS = 0, PS_REP_LOSS, PS_LOC_HIT, PS_REP_HIT, PS_BUGGY };

inline int vm_bwd_blocks(int64_t nrows) {
  const int64_t w = (nrows + VM_BWD_WAVES - 1) / VM_BWD_WAVES;
  return (int)(w < VM_BWD_MAX_BLOCKS ? w : VM_BWD_MAX_BLOCKS);
}
// partial row of one backward workgroup: [g_W (2 D, interleaved as W) | g_ln_g (D) | g_ln_b (D) | g_bias (2) | pad (2)]
__host__ __device__ inline int vm_partial_cols(int D) { return 4 * D + 4; }

__device__ __forceinline__ float block_sum(float s, float* sv) {
  s = bl_wave_sum(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sv[wave] = s;
  __syncthreads();
  float t = sv[0];
  for (int w = 1; w < VM_SAMPLE_WAVES; ++w) t += sv[w];
  __syncthreads();
  return t;
}

// ---- forward, row pass -------------------------------------------------------------------------------------------------
template <int NK>
__global__ __launch_bounds__(VM_ROW_THREADS) void vm_fwd_rows(bl_varmisuse_head_t d, float* __restrict__ logits,
                                                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                              unsigned* __restrict__ counter) {
  if (blockIdx.x == 0 && threadIdx.x == 0)  // the ticket counter of vm_fwd_samples (next launch on this stream)
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (VM_ROW_THREADS / 64) + (threadIdx.x >> 6);
  const int64_t nrows = (int64_t)d.B * d.L;
  if (row >= nrows) return;  // (whole wave)
  float mu, rs, a0, a1;
  vm_row_logits<NK>(d, row, lane, mu, rs, a0, a1);
  if (lane == 0) {
    reinterpret_cast<float2*>(logits)[row] = vm_masked_logits(d, row, a0, a1);
    mean_out[row] = mu;
    rstd_out[row] = rs;
  }
}

// ---- forward, per-sample pass + the last workgroup's fixed-order reduction ------------------------------------------
__global__ __launch_bounds__(VM_SAMPLE_THREADS) void vm_fwd_samples(bl_varmisuse_head_t d, const float* __restrict__ logits,
                                                                    float* __restrict__ lse, float* __restrict__ ps,
                                                                    unsigned* __restrict__ counter, float* __restrict__ loss,
                                                                    double* __restrict__ stats) {
  __shared__ float sv[VM_SAMPLE_WAVES];
  __shared__ int si[VM_SAMPLE_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, L = d.L;
  int la = d.lens_att[b];
  la = la < 0 ? 0 : (la > L ? L : la);
  const int err = d.error_location[b];
  const bool buggy = err != 0;  // `is_buggy = error_locations != 0` (:209)
  const float2* lg = reinterpret_cast<const float2*>(logits) + (int64_t)b * L;
  const uint8_t* tgt = d.target_mask + (int64_t)b * L;
  // pass 1: maxima (and first-index arg-maxima) of the localization column over the unmasked positions, of the pointer column
  // over the candidates (the other entries are -inf), of the pointer column over candidates that are targets
  float m0 = VM_NEG_INF, m1 = VM_NEG_INF, m2 = VM_NEG_INF;
  int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
  for (int i = tid; i < la; i += VM_SAMPLE_THREADS) {  // a thread's positions increase: strict > keeps its first maximum
    const float2 v = lg[i];
    if (v.x > m0) m0 = v.x, i0 = i;
    if (v.y > m1) m1 = v.y, i1 = i;
    if (tgt[i] && v.y > m2) m2 = v.y;
  }
  block_argmax(m0, i0, sv, si);
  block_argmax(m1, i1, sv, si);
  block_argmax(m2, i2, sv, si);
  // pass 2: sums of exp(. - max)
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < la; i += VM_SAMPLE_THREADS) {
    const float2 v = lg[i];
    s0 += expf(v.x - m0);
    if (v.y != VM_NEG_INF) {
      s1 += expf(v.y - m1);
      if (tgt[i]) s2 += expf(v.y - m2);
    }
  }
  s0 = block_sum(s0, sv);
  s1 = block_sum(s1, sv);
  s2 = block_sum(s2, sv);
  if (tid != 0) return;
  const float lse0 = m0 + logf(s0);
  const float lse1 = m1 == VM_NEG_INF ? VM_NEG_INF : m1 + logf(s1);
  const float lse2 = m2 == VM_NEG_INF ? VM_NEG_INF : m2 + logf(s2);
  lse[3 * b + 0] = lse0;
  lse[3 * b + 1] = lse1;
  lse[3 * b + 2] = lse2;
  const float l_err = (err >= 0 && err < la) ? lg[err].x : VM_NEG_INF;
  // cross_entropy over the unmasked positions (:143); repair: -logsumexp over the targets of the pointer log-softmax (:161-163)
  const float loc_loss = lse0 - l_err;
  const float rep_loss = buggy ? lse1 - lse2 : 0.f;
  const float loc_hit = i0 == err ? 1.f : 0.f;                         // :146
  const float rep_hit = (buggy && i1 < la && tgt[i1]) ? 1.f : 0.f;     // :165-168
  float* mine = ps + (int64_t)VM_PS * b;
  __hip_atomic_store(mine + PS_LOC_LOSS, loc_loss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(mine + PS_REP_LOSS, rep_loss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(mine + PS_LOC_HIT, loc_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(mine + PS_REP_HIT, rep_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(mine + PS_BUGGY, buggy ? 1.f : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // release our slots, acquire everybody else's if we are last
  const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != (unsigned)(d.B - 1)) return;
  float sl = 0.f, sr = 0.f, nb = 0.f, lh = 0.f, blh = 0.f, rh = 0.f;
  for (int s = 0; s < d.B; ++s) {
    const float* p = ps + (int64_t)VM_PS * s;
    const float ll = __hip_atomic_load(p + PS_LOC_LOSS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float rl = __hip_atomic_load(p + PS_REP_LOSS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float hl = __hip_atomic_load(p + PS_LOC_HIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float hr = __hip_atomic_load(p + PS_REP_HIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float bg = __hip_atomic_load(p + PS_BUGGY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sl += ll;
    lh += hl;
    if (bg != 0.f) {
      sr += rl;
      nb += 1.f;
      blh += hl;
      rh += hr;
    }
  }
  // loss = mean localization loss + (mean repair loss over the buggy samples, or 0 without any) (:143, :156-174)
  loss[0] = sl / (float)d.B + (nb > 0.f ? sr / nb : 0.f);
  loss[1] = nb;
  const double add[BL_VARMISUSE_STATS] = {(double)d.B, lh, blh, nb, rh, sl, sr, 1.0};
  for (int k = 0; k < BL_VARMISUSE_STATS; ++k) {
    const double old = __hip_atomic_load(stats + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(stats + k, old + add[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- backward, row pass ------------------------------------------------------------------------------------------------
template <int NK>
__global__ __launch_bounds__(VM_BWD_THREADS) void vm_bwd_rows(bl_varmisuse_head_t d, const float* __restrict__ logits,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ lse, const float* __restrict__ lossv,
                                                              const float* __restrict__ g_loss, float* __restrict__ part,
                                                              float* __restrict__ g_x) {
  __shared__ float4 red[VM_BWD_WAVES][VM_MAX_D / 4];
  __shared__ float rb[VM_BWD_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = d.D, D4 = D >> 2, L = d.L;
  const int64_t nrows = (int64_t)d.B * L;
  const float gs = g_loss[0], nb = lossv[1];
  const float inv_b = 1.0f / (float)d.B, inv_nb = nb > 0.f ? 1.0f / nb : 0.f, inv_d = 1.0f / (float)D;
  const float4* g4 = reinterpret_cast<const float4*>(d.ln_g);
  const float4* b4 = reinterpret_cast<const float4*>(d.ln_b);
  const float4* w4 = reinterpret_cast<const float4*>(d.W);
  float4 G[NK], Be[NK], Wa[NK], Wb[NK];
  float4 aw0[NK], aw1[NK], ag[NK], ab[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int j = lane + 64 * k;
    const bool in = j < D4;
    G[k] = in ? g4[j] : f4(0.f);
    Be[k] = in ? b4[j] : f4(0.f);
    Wa[k] = in ? w4[2 * j] : f4(0.f);
    Wb[k] = in ? w4[2 * j + 1] : f4(0.f);
    aw0[k] = aw1[k] = ag[k] = ab[k] = f4(0.f);
  }
  float sdl = 0.f, sdp = 0.f;
  const int64_t stride = (int64_t)gridDim.x * VM_BWD_WAVES;
  for (int64_t row = (int64_t)blockIdx.x * VM_BWD_WAVES + wave; row < nrows; row += stride) {
    const int b = (int)(row / L), i = (int)(row - (int64_t)b * L);
    float4* gxr = reinterpret_cast<float4*>(g_x + row * D);
    if (i >= d.lens_att[b]) {  // masked position: -inf logits, no gradient (wave-uniform branch)
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (lane + 64 * k < D4) gxr[lane + 64 * k] = f4(0.f);
      continue;
    }
    const int err = d.error_location[b];
    const float2 lg = reinterpret_cast<const float2*>(logits)[row];
    // d loss / d logit: localization softmax minus one-hot, over B; pointer softmax over the candidates minus the softmax over
    // candidates that are targets, over the number of buggy samples (0 for NO_BUG samples: the reference drops their rows)
    const float dl = gs * (expf(lg.x - lse[3 * b]) - (i == err ? 1.f : 0.f)) * inv_b;
    float dp = 0.f;
    if (err != 0 && lg.y != VM_NEG_INF) {
      const float pc = expf(lg.y - lse[3 * b + 1]);
      const float pt = d.target_mask[row] ? expf(lg.y - lse[3 * b + 2]) : 0.f;
      dp = gs * (pc - pt) * inv_nb;
    }
    sdl += dl;
    sdp += dp;
    const float mu = mean[row], rs = rstd[row];
    const float4* xr = reinterpret_cast<const float4*>(d.x + row * D);
    float4 xh[NK], dxh[NK];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int j = lane + 64 * k;
      const float4 x = j < D4 ? xr[j] : f4(0.f);
      xh[k] = make_float4((x.x - mu) * rs, (x.y - mu) * rs, (x.z - mu) * rs, (x.w - mu) * rs);
      const float4 y = make_float4(xh[k].x * G[k].x + Be[k].x, xh[k].y * G[k].y + Be[k].y, xh[k].z * G[k].z + Be[k].z,
                                   xh[k].w * G[k].w + Be[k].w);
      // g_W[r, c] += y_r * dlogit_c   (W [D, 2]: float4 2j = (r 4j: c0 c1, r 4j+1: c0 c1))
      aw0[k].x += y.x * dl; aw0[k].y += y.x * dp; aw0[k].z += y.y * dl; aw0[k].w += y.y * dp;
      aw1[k].x += y.z * dl; aw1[k].y += y.z * dp; aw1[k].z += y.w * dl; aw1[k].w += y.w * dp;
      const float4 dy = make_float4(dl * Wa[k].x + dp * Wa[k].y, dl * Wa[k].z + dp * Wa[k].w, dl * Wb[k].x + dp * Wb[k].y,
                                    dl * Wb[k].z + dp * Wb[k].w);
      ag[k].x += dy.x * xh[k].x; ag[k].y += dy.y * xh[k].y; ag[k].z += dy.z * xh[k].z; ag[k].w += dy.w * xh[k].w;
      ab[k].x += dy.x; ab[k].y += dy.y; ab[k].z += dy.z; ab[k].w += dy.w;
      dxh[k] = make_float4(dy.x * G[k].x, dy.y * G[k].y, dy.z * G[k].z, dy.w * G[k].w);
      s1 += hsum(dxh[k]);
      s2 += (dxh[k].x * xh[k].x + dxh[k].y * xh[k].y) + (dxh[k].z * xh[k].z + dxh[k].w * xh[k].w);
    }
    s1 = bl_wave_sum(s1) * inv_d;
    s2 = bl_wave_sum(s2) * inv_d;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int j = lane + 64 * k;
      if (j < D4)
        gxr[j] = make_float4(rs * (dxh[k].x - s1 - xh[k].x * s2), rs * (dxh[k].y - s1 - xh[k].y * s2),
                             rs * (dxh[k].z - s1 - xh[k].z * s2), rs * (dxh[k].w - s1 - xh[k].w * s2));
    }
  }
  // this workgroup's partials: the waves' accumulators summed in wave order, one quantity at a time through LDS
  const int nc = vm_partial_cols(D);
  float* out = part + (int64_t)blockIdx.x * nc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int j = lane + 64 * k;
      if (j < D4) red[wave][j] = r == 0 ? aw0[k] : r == 1 ? aw1[k] : r == 2 ? ag[k] : ab[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < D4; j += VM_BWD_THREADS) {
      float4 t = red[0][j];
      for (int w = 1; w < VM_BWD_WAVES; ++w) {
        const float4 u = red[w][j];
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      const int col = r == 0 ? 8 * j : r == 1 ? 8 * j + 4 : r == 2 ? 2 * D + 4 * j : 3 * D + 4 * j;
      *reinterpret_cast<float4*>(out + col) = t;
    }
    __syncthreads();
  }
  if (lane == 0) {
    rb[wave][0] = sdl;
    rb[wave][1] = sdp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t0 = rb[0][0], t1 = rb[0][1];
    for (int w = 1; w < VM_BWD_WAVES; ++w) t0 += rb[w][0], t1 += rb[w][1];
    *reinterpret_cast<float4*>(out + 4 * D) = make_float4(t0, t1, 0.f, 0.f);
  }
}

// ---- backward, partial reduction: 64 columns per workgroup, 16 waves over slices of the partial rows, combined in order ----
__global__ __launch_bounds__(VM_RED_THREADS) void vm_bwd_reduce(const float* __restrict__ part, int nblocks, int D,
                                                                float* __restrict__ g_W, float* __restrict__ g_bias,
                                                                float* __restrict__ g_ln_g, float* __restrict__ g_ln_b) {
  __shared__ float red[VM_RED_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = vm_partial_cols(D), used = 4 * D + 2;
  const int col = blockIdx.x * 64 + lane;
  const int per = (nblocks + VM_RED_WAVES - 1) / VM_RED_WAVES;
  const int r0 = wave * per, r1 = min(nblocks, r0 + per);
  float s = 0.f;
  if (col < used)
    for (int r = r0; r < r1; ++r) s += part[(int64_t)r * nc + col];
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || col >= used) return;
  float t = red[0][lane];
  for (int w = 1; w < VM_RED_WAVES; ++w) t += red[w][lane];
  if (col < 2 * D) g_W[col] = t;
  else if (col < 3 * D) g_ln_g[col - 2 * D] = t;
  else if (col < 4 * D) g_ln_b[col - 3 * D] = t;
  else g_bias[col - 4 * D] = t;
}

}  // namespace

extern "C" int64_t bl_varmisuse_head_workspace_bytes(int32_t B, int32_t L, int32_t D) {
  if (B < 1 || L < 1 || D < 4 || D > VM_MAX_D || D % 4 != 0) return -1;
  const int64_t fwd = VM_COUNTER_BYTES + (int64_t)VM_PS * B * (int64_t)sizeof(float);
  const int64_t bwd = (int64_t)vm_bwd_blocks((int64_t)B * L) * vm_partial_cols(D) * (int64_t)sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

extern "C" int bl_varmisuse_head_fwd(const bl_varmisuse_head_t* d, float* logits, float* mean, float* rstd, float* lse, void* workspace,
                                     float* loss, double* stats, void* stream) {
  if (int rc = vm_check(d, "bl_varmisuse_head_fwd")) return rc;
  BL_CHECK_ARG(logits && mean && rstd && lse && workspace && loss && stats, "bl_varmisuse_head_fwd: null output pointer");
  BL_CHECK_ARG((((uintptr_t)logits) & 7u) == 0 && bl_aligned16(workspace) && (((uintptr_t)stats) & 7u) == 0,
               "bl_varmisuse_head_fwd: logits / stats must be 8-byte and workspace 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nrows = (int64_t)d->B * d->L;
  unsigned* counter = reinterpret_cast<unsigned*>(workspace);
  float* ps = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + VM_COUNTER_BYTES);
  const dim3 grid((unsigned)((nrows + VM_ROW_THREADS / 64 - 1) / (VM_ROW_THREADS / 64)));
  const int nk = (d->D / 4 + 63) / 64;
  switch (nk) {
    case 1: vm_fwd_rows<1><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits, mean, rstd, counter); break;
    case 2: vm_fwd_rows<2><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits, mean, rstd, counter); break;
    case 3: vm_fwd_rows<3><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits, mean, rstd, counter); break;
    default: vm_fwd_rows<4><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits, mean, rstd, counter); break;
  }
  BL_LAUNCH_CHECK("vm_fwd_rows");
  vm_fwd_samples<<<d->B, VM_SAMPLE_THREADS, 0, st>>>(*d, logits, lse, ps, counter, loss, stats);
  BL_LAUNCH_CHECK("vm_fwd_samples");
  return BL_OK;
}

extern "C" int bl_varmisuse_head_bwd(const bl_varmisuse_head_t* d, const float* logits, const float* mean, const float* rstd,
                                     const float* lse, const float* loss, const float* g_loss, void* workspace, float* g_x,
                                     float* g_W, float* g_bias, float* g_ln_g, float* g_ln_b, void* stream) {
  if (int rc = vm_check(d, "bl_varmisuse_head_bwd")) return rc;
  BL_CHECK_ARG(logits && mean && rstd && lse && loss && g_loss && workspace, "bl_varmisuse_head_bwd: null saved-tensor pointer");
  BL_CHECK_ARG(g_x && g_W && g_bias && g_ln_g && g_ln_b, "bl_varmisuse_head_bwd: null gradient pointer");
  BL_CHECK_ARG((((uintptr_t)logits) & 7u) == 0 && bl_aligned16(workspace) && bl_aligned16(g_x),
               "bl_varmisuse_head_bwd: logits must be 8-byte, workspace and g_x 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nrows = (int64_t)d->B * d->L;
  const int nblocks = vm_bwd_blocks(nrows);
  float* part = reinterpret_cast<float*>(workspace);
  const int nk = (d->D / 4 + 63) / 64;
  switch (nk) {
    case 1: vm_bwd_rows<1><<<nblocks, VM_BWD_THREADS, 0, st>>>(*d, logits, mean, rstd, lse, loss, g_loss, part, g_x); break;
    case 2: vm_bwd_rows<2><<<nblocks, VM_BWD_THREADS, 0, st>>>(*d, logits, mean, rstd, lse, loss, g_loss, part, g_x); break;
    case 3: vm_bwd_rows<3><<<nblocks, VM_BWD_THREADS, 0, st>>>(*d, logits, mean, rstd, lse, loss, g_loss, part, g_x); break;
    default: vm_bwd_rows<4><<<nblocks, VM_BWD_THREADS, 0, st>>>(*d, logits, mean, rstd, lse, loss, g_loss, part, g_x); break;
  }
  BL_LAUNCH_CHECK("vm_bwd_rows");
  const int used = 4 * d->D + 2;
  vm_bwd_reduce<<<(used + 63) / 64, VM_RED_THREADS, 0, st>>>(part, nblocks, d->D, g_W, g_bias, g_ln_g, g_ln_b);
  BL_LAUNCH_CHECK("vm_bwd_reduce");
  return BL_OK;
}
