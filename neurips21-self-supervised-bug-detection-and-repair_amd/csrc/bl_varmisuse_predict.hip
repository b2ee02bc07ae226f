// GREAT var-misuse prediction: the head forward-only, every sample judged on the device.
//
// The reference has no predict (greatreimplementation.py ends at finalize_minibatch); this is the inference counterpart of its
// head (:176-214) in this repository's style: the masked logits of the training forward, and per sample the predicted location
// and repair, their log-probabilities and the two verdicts an evaluation counts, written at the caller's offset into buffers
// that stay on the device for the whole run (the convention of bl_eval_judge).  No mean / rstd, workspace, loss or stats; no
// synchronisation; nothing is read on the host.
//
// Two launches:
//   vm_predict_rows     one wave per row of x [B * L, D]: the row arithmetic of vm_fwd_rows (bl_varmisuse_rows.h, one copy), so
//                       the logits are the training forward's, bit for bit.  B * L / 4 workgroups: with B around 30 this is
//                       the part that reads x, and it fills the device where B workgroups would not;
//   vm_predict_samples  one workgroup (4 waves) per sample, threads stride over its positions:
//     1  first-index maxima on the fp32 logits (exact): the localization column over positions < lens_att, the pointer column
//        over the candidates among them (the others hold -inf), and the pointer maximum over candidates that are targets.  A NaN
//        never wins (strict >);
//     2  the three sums of exp(double(v) - double(max)) in fp64: per thread in stride order, then bl_block_sum_f64
//        (bl_segment_f64.h) -- a fixed order, so a rerun is bit-identical;
//     3  thread 0 writes the record.
// fp64 on purpose (as bl_evaluate.hip): the record's log-probabilities are what a host would compute from the fp32 logits in
// Python floats, and they are compared and ranked across minibatches.
// Plain vector loads and stores only, no atomics.
#include "bl_common.h"
#include "bl_segment_f64.h"
#include "bl_varmisuse_rows.h"

namespace {
template <int NK>
__global__ __launch_bounds__(VM_ROW_THREADS) void vm_predict_rows(bl_varmisuse_head_t d, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (VM_ROW_THREADS / 64) + (threadIdx.x >> 6);
  const int64_t nrows = (int64_t)d.B * d.L;
  if (row >= nrows) return;  // (whole wave)
  float mu, rs, a0, a1;
  vm_row_logits<NK>(d, row, lane, mu, rs, a0, a1);
  if (lane == 0) reinterpret_cast<float2*>(logits)[row] = vm_masked_logits(d, row, a0, a1);
}

__global__ __launch_bounds__(VM_SAMPLE_THREADS) void vm_predict_samples(bl_varmisuse_head_t d, const float* __restrict__ logits,
                                                                        double* __restrict__ out_d, int32_t* __restrict__ out_i,
                                                                        int64_t offset, int64_t capacity) {
  __shared__ float sv[VM_SAMPLE_WAVES];
  __shared__ int si[VM_SAMPLE_WAVES];
  __shared__ double sd[VM_SAMPLE_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, L = d.L;
  int la = d.lens_att[b];
  la = la < 0 ? 0 : (la > L ? L : la);
  const float2* lg = reinterpret_cast<const float2*>(logits) + (int64_t)b * L;
  const uint8_t* tgt = d.target_mask + (int64_t)b * L;
  // ---- 1: maxima and first-index arg-maxima, as vm_fwd_samples takes them
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
  // ---- 2: sums of exp(. - max) in fp64
  const double dm0 = (double)m0, dm1 = (double)m1, dm2 = (double)m2;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < la; i += VM_SAMPLE_THREADS) {
    const float2 v = lg[i];
    s0 += exp((double)v.x - dm0);
    if (v.y != VM_NEG_INF) {
      s1 += exp((double)v.y - dm1);
      if (tgt[i]) s2 += exp((double)v.y - dm2);
    }
  }
  // three reductions through one sd: each call's leading barrier comes after every thread has read the previous call's sums
  s0 = bl_block_sum_f64<VM_SAMPLE_WAVES>(s0, sd);
  s1 = bl_block_sum_f64<VM_SAMPLE_WAVES>(s1, sd);
  s2 = bl_block_sum_f64<VM_SAMPLE_WAVES>(s2, sd);
  if (tid != 0) return;
  // ---- 3: the record
  const double ninf = -__builtin_huge_val();
  const double lse0 = m0 == VM_NEG_INF ? ninf : dm0 + log(s0);
  const double lse1 = m1 == VM_NEG_INF ? ninf : dm1 + log(s1);
  const double lse2 = m2 == VM_NEG_INF ? ninf : dm2 + log(s2);
  const int pred = i0 < la ? i0 : 0;       // nothing above -inf (the host never sends such a sample): torch.argmax's 0
  const int rep = i1 < la ? i1 : -1;       // no candidate
  const int err = d.error_location[b];
  const int64_t at = offset + b;           // the host checked 0 <= offset and offset + B <= capacity
  out_d[at] = lse0;
  out_d[capacity + at] = lse1;
  out_d[2 * capacity + at] = (double)lg[pred].x - lse0;
  out_d[3 * capacity + at] = (double)lg[0].x - lse0;
  out_d[4 * capacity + at] = (err >= 0 && err < la) ? (double)lg[err].x - lse0 : ninf;
  out_d[5 * capacity + at] = rep >= 0 ? (double)lg[rep].y - lse1 : __builtin_nan("");
  // logsumexp over the targets of the pointer log-softmax (:161): lse(targets) - lse(candidates)
  out_d[6 * capacity + at] = m2 == VM_NEG_INF ? ninf : lse2 - lse1;
  out_i[at] = pred;
  out_i[capacity + at] = rep;
  out_i[2 * capacity + at] = pred == err ? 1 : 0;
  out_i[3 * capacity + at] = (rep >= 0 && tgt[rep]) ? 1 : 0;
}
}  // namespace

extern "C" int bl_varmisuse_predict(const bl_varmisuse_head_t* d, float* logits, double* out_d, int32_t* out_i, int64_t offset,
                                    int64_t capacity, void* stream) {
  if (int rc = vm_check(d, "bl_varmisuse_predict")) return rc;
  BL_CHECK_ARG(logits && out_d && out_i, "bl_varmisuse_predict: null output pointer");
  BL_CHECK_ARG(offset >= 0 && capacity >= 0 && offset <= capacity && (int64_t)d->B <= capacity - offset,
               "bl_varmisuse_predict: samples %lld .. %lld do not fit the record buffers of %lld samples", (long long)offset,
               (long long)offset + (long long)d->B, (long long)capacity);
  BL_CHECK_ARG((((uintptr_t)logits) & 7u) == 0 && (((uintptr_t)out_d) & 7u) == 0 && (((uintptr_t)out_i) & 3u) == 0,
               "bl_varmisuse_predict: logits / out_d must be 8-byte and out_i 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nrows = (int64_t)d->B * d->L;
  const dim3 grid((unsigned)((nrows + VM_ROW_THREADS / 64 - 1) / (VM_ROW_THREADS / 64)));
  const int nk = (d->D / 4 + 63) / 64;
  switch (nk) {
    case 1: vm_predict_rows<1><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits); break;
    case 2: vm_predict_rows<2><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits); break;
    case 3: vm_predict_rows<3><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits); break;
    default: vm_predict_rows<4><<<grid, VM_ROW_THREADS, 0, st>>>(*d, logits); break;
  }
  BL_LAUNCH_CHECK("vm_predict_rows");
  vm_predict_samples<<<d->B, VM_SAMPLE_THREADS, 0, st>>>(*d, logits, out_d, out_i, offset, capacity);
  BL_LAUNCH_CHECK("vm_predict_samples");
  return BL_OK;
}
