/*
 * buglab_hip.h -- C ABI of libbuglab_hip.so, the MI355X (gfx950) kernels behind BugLab's
 * `gnn-mlp` message-passing + scoring-head hot path.
 *
 * Conventions:
 *   - every function is extern "C", returns 0 on success, a positive hipError_t or a negative
 *     BL_E* argument error otherwise; bl_last_error() gives the text for the calling thread;
 *   - the CALLER owns every buffer (PyTorch-ROCm tensors -> data_ptr()); nothing here allocates;
 *   - all index arrays are int32, all values float32, matrices row-major with an explicit
 *     leading dimension where one is given; pointers must be 16-byte aligned and every leading
 *     dimension / width a multiple of 4 floats -- except where an entry point says "any width": bl_segment_max_fwd,
 *     bl_mp_scatter_grad / _split and bl_gru_cell_fwd / _bwd address their rows element by element and take any width
 *     and any leading dimension >= the width, with pointers that need only be 4-byte aligned (the heads run the segmented
 *     max over [*, 1] columns); bl_segment_max_bwd is NOT one of them, see there;
 *   - no entry point writes outside [rows, width] of an output or outside the bytes its *_bytes / *_elems function reports,
 *     and nothing outside an input's [rows, width] (the columns width .. ld, the rows around it) influences a result
 *     (tests/test_abi_strides_gpu.py);
 *   - the last argument is the hipStream_t to launch on
 *     (torch.cuda.current_stream().cuda_stream); entry points never synchronise.
 *
 * The reference has no native code at all: each entry point below names the reference Python
 * (or the third-party op called from it) that it replaces.  Paths are relative to
 * /root/reference.
 */
#ifndef BUGLAB_HIP_H
#define BUGLAB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BL_OK 0
#define BL_EINVAL (-1) /* bad argument (null pointer, misaligned, unsupported size) */
#define BL_ERANGE (-2) /* dimension outside what the kernels were built for */

/* activation codes shared by every entry point.  BL_ACT_GELU_AGG is accepted only where a segmented max is involved
 * (bl_segment_max_fwd / _bwd, bl_mp_layer_t.msg_act): GELU applied to the AGGREGATE, out = gelu(max_i x_i), instead of to every
 * item before the max, out = max_i gelu(x_i) (BL_ACT_GELU) -- the two placements of ptgnn's `message_activation`. */
enum { BL_ACT_NONE = 0, BL_ACT_RELU = 1, BL_ACT_SIGMOID = 2, BL_ACT_TANH = 3, BL_ACT_GELU = 4, BL_ACT_GELU_AGG = 5 };

const char* bl_last_error(void);
int bl_version(void);
/* Deterministic-gradient mode (also switched on by BL_DETERMINISTIC=1 in the environment at first use).  The kernels that
 * add into one address from several workgroups -- the split-K weight gradients (bl_gemm_wgrad*, bl_gemm_wgrad_routed_x6),
 * the column sums of bl_layernorm_bwd / bl_act_bwd / bl_rowdot_bwd -- then flush in a fixed workgroup order (a turn
 * counter per output tile), bl_scatter_add_rows and bl_embed_subtoken_max_bwd walk their rows serially per column: every
 * gradient is bit-identical from run to run, at a cost (the flushes serialise).  bl_embed_subtoken_max_bwd_sorted is
 * reproducible when every token is ONE chunk (the collator does that in this mode).  Not covered: the relational-attention
 * bias gradients (bl_rel_attn_bias_bwd, bl_rel_value_bias_bwd).  The reference has no counterpart (torch's index_add /
 * scatter backward are atomic too); this exists so that a parity failure can be reproduced. */
void bl_set_deterministic(int32_t on);
int32_t bl_get_deterministic(void);

/* Rows of a (virtually) concatenated, gathered operand:
 *   row r = [ x[0][idx[0][r], 0:width[0]] ; x[1][idx[1][r], 0:width[1]] ; ... ]   (nsrc <= 3)
 * idx[j] == NULL means the identity (row r of x[j]).  This is how `torch.cat((h[src], h[tgt]), -1)`
 * and the heads' `torch.cat((a[i], b[j]), -1)` are consumed without ever being materialised. */
typedef struct {
  const float* x[3];
  const int32_t* idx[3];
  int32_t ld[3];
  int32_t width[3];
  int32_t nsrc;
} bl_rows_t;

/* counter-based dropout (oracle: oracle/buglab_oracle.py::dropout_keep_mask).  p == 0 disables. */
typedef struct {
  float p;
  uint32_t seed;
  uint32_t stream;
} bl_dropout_t;

/* ---------------------------------------------------------------------------------------------
 * M0  node embedder: out[n,:] = Dropout(max_{s < lens[n]} table[ids[n,s], :]), argsub = winning s.
 * Replaces ptgnn StrElementRepresentationModel (configured at buglab/models/modelregistry.py:59-82:
 * subtoken splitting, <= 6 subtokens, "max" combination).
 * bwd: g_table[ids[n, argsub[n,h]], h] += g_out[n,h] (masked by the same dropout), fp32 atomics.
 * drop_before_pool: 0 (default spec) = dropout on the pooled rows, out = drop(max_s emb); 1 = dropout on the embedded subtokens
 * before the pooling, out = max_s drop(emb)[n, s, :] with mask index (n S + s) H + h (the other placement ptgnn's
 * SubtokenUnitEmbedder may have: DESIGN.md section 2); backward scales by the winner's mask bit. */
int bl_embed_subtoken_max_fwd(const float* table, int32_t V, int32_t H, const int32_t* ids, const int32_t* lens,
                              int32_t N, int32_t S, bl_dropout_t drop, int32_t drop_before_pool, float* out, int32_t ld_out,
                              int8_t* argsub, void* stream);
int bl_embed_subtoken_max_bwd(const float* g_out, int32_t ld_g, const int32_t* ids, const int8_t* argsub, int32_t N,
                              int32_t S, int32_t H, int32_t V, bl_dropout_t drop, int32_t drop_before_pool, float* g_table,
                              void* stream);
/* The same gradient from a token-sorted occurrence list: occ[i] = n * S + s (every valid subtoken slot),
 * sorted by ids[n, s] and cut in chunks of one token each (chunk_ptr [nchunks + 1], chunk_tok [nchunks];
 * the collator uses <= 256 occurrences per chunk).  One atomic per (chunk, channel) instead of one per
 * (node, channel): subtoken frequencies are Zipfian and same-address atomics serialise. */
int bl_embed_subtoken_max_bwd_sorted(const float* g_out, int32_t ld_g, const int32_t* occ, const int32_t* chunk_ptr,
                                     const int32_t* chunk_tok, int32_t nchunks, const int8_t* argsub, int32_t S,
                                     int32_t H, bl_dropout_t drop, int32_t drop_before_pool, float* g_table, void* stream);

/* The embedder with the node model's other `subtoken_combination` values (reference buglab/models/modelregistry.py:65-66 sets "max"
 * unless the caller's node_representations says otherwise; ptgnn's StrElementRepresentationModel also takes "sum" and "mean"):
 * combination BL_POOL_MAX = the three entry points above; BL_POOL_SUM: out[n] = drop(sum_{s < lens[n]} emb[n, s]);
 * BL_POOL_MEAN: the sum / lens[n].  argsub is used by BL_POOL_MAX only (NULL otherwise); bwd needs lens for sum / mean (every
 * slot s < lens[n] receives g_out[n] (/ lens[n]), under its own mask bit with drop_before_pool); the sorted form needs lens for
 * BL_POOL_MEAN. */
#define BL_POOL_MAX 0
#define BL_POOL_SUM 1
#define BL_POOL_MEAN 2
int bl_embed_subtoken_pool_fwd(const float* table, int32_t V, int32_t H, const int32_t* ids, const int32_t* lens, int32_t N, int32_t S,
                               int32_t combination, bl_dropout_t drop, int32_t drop_before_pool, float* out, int32_t ld_out,
                               int8_t* argsub, void* stream);
int bl_embed_subtoken_pool_bwd(const float* g_out, int32_t ld_g, const int32_t* ids, const int32_t* lens, const int8_t* argsub, int32_t N,
                               int32_t S, int32_t H, int32_t V, int32_t combination, bl_dropout_t drop, int32_t drop_before_pool,
                               float* g_table, void* stream);
int bl_embed_subtoken_pool_bwd_sorted(const float* g_out, int32_t ld_g, const int32_t* occ, const int32_t* chunk_ptr,
                                      const int32_t* chunk_tok, int32_t nchunks, const int32_t* lens, const int8_t* argsub, int32_t S,
                                      int32_t H, int32_t combination, bl_dropout_t drop, int32_t drop_before_pool, float* g_table,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped, gathered fp32 GEMM on MFMA (v_mfma_f32_32x32x2_f32, exact fp32).
 *   for group g (rows group_ptr[g] .. group_ptr[g+1]):  C[r, 0:N] = drop(act(rows(a)[r, 0:K] . B_g + bias))
 *   B_g = b + group_w[g] * b_group_stride ; if b_is_nk == 0, B_g is [K, N] row-major (ldb),
 *   else B_g is [N, K] row-major and is used transposed (C = A . B_g^T).
 * group_ptr == NULL: one group covering rows 0..M.  group_w == NULL: identity.
 * Replaces, per edge type, ptgnn MlpMessagePassingLayer's gather + cat + Linear
 * (call site buglab/models/gnnlayerdefs.py:6-23), ptgnn's dense node update, and the heads'
 * nn.Linear / MLP layers (buglab/models/layers/mlp.py:6-20, localizationmodule.py:22-24, 56-60,
 * fixermodules.py:36-39, 71-73, 116-124).  With b_is_nk = 1 it is the input-gradient GEMM. */
int bl_gemm_rows(const bl_rows_t* a, const float* b, int64_t b_group_stride, int32_t ldb, int32_t b_is_nk,
                 const float* bias, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N,
                 int32_t K, int32_t act, bl_dropout_t drop, float* c, int32_t ldc, void* stream);

/* Input-gradient GEMM with the max-aggregation ROUTING folded into the operand load:
 *   row r of the left operand is  G[r, k] = (winner[idx[r], k] == r) ? a.x[0][idx[r], k] : 0
 * (a has exactly one gathered source: a.x[0] = d loss / d aggregate per node [N, K], idx = target node
 * of message r; `winner` = the arg-max table of bl_segment_max_fwd), then C = G . B_g^T as in
 * bl_gemm_rows with b_is_nk = 1.  Replaces torch_scatter's scatter_max backward (a gather of the
 * gradient at arg) + the autograd of the per-type Linear, without materialising the [E, Dm] gradient. */
int bl_gemm_rows_routed(const bl_rows_t* a, const int32_t* winner, int32_t ld_winner, const float* b,
                        int64_t b_group_stride, int32_t ldb, const int32_t* group_ptr, const int32_t* group_w, int32_t G,
                        int32_t M, int32_t N, int32_t K, float* c, int32_t ldc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32-accurate GEMM on the bf16 matrix cores ("bf16x6"): every fp32 operand is split once into
 * three bf16 terms hi + mid + lo (bl_pack_bf16x3*: every row is three bf16 planes back to
 * back, [hi x D | mid x D | lo x D]) and a product is evaluated as the six MFMA terms hh + hm + mh + hl + lh + mm
 * with fp32 accumulation; dropped terms are < 2^-26 of the product, below fp32's own rounding.
 * Same contract as bl_gemm_rows (C[rows of g] = A . B_g), B given by bl_pack_weights_x6, no
 * bias/activation epilogue.  win_bits != NULL selects the routed left operand of bl_gemm_rows_routed,
 * with the routing given as bl_segment_max_fwd's per-message bitmask (row r keeps channel k iff bit k
 * of win_bits[r * ld_bits ...] is set; ld_bits in 32-bit words).  Source widths: multiples of 32. */
typedef struct {
  const uint16_t* xp[3];  /* packed matrices (bl_pack_bf16x3) */
  const int32_t* idx[3];  /* row gather index or NULL */
  int32_t width[3];       /* k's taken from each source (the packed matrix's D) */
  int32_t nsrc;
} bl_rows_packed_t;
int bl_pack_bf16x3(const float* x, int32_t ld, int64_t R, int32_t D, uint16_t* out, void* stream);
/* the same into the columns col_off .. col_off + D of a packed matrix whose rows are D_total wide: how the
 * [stash ; current] input of a ConcatResidual layer (gnnlayerdefs.py:24-38) is packed without a concatenated copy */
int bl_pack_bf16x3_cols(const float* x, int32_t ld, int64_t R, int32_t D, int32_t D_total, int32_t col_off, uint16_t* out,
                        void* stream);
/* Weights of the bf16x6 row GEMM, packed and TILED: per group ceil(N/128) * (K/32) blocks of 24 KB
 * (12288 uint16), block (tile, stage) = [i (2)][plane (3)][row_lo (64)][k-group (4)][8] for column
 * n = 128 tile + 64 i + row_lo and k = 32 stage + 8 k-group + 0..7; columns past N are zero.
 * w is [G][K][N] if w_is_kn (forward weights W[t]: C = A . W) or [G][N][K] (C = A . w^T). */
int bl_pack_weights_x6(const float* w, int32_t G, int32_t K, int32_t N, int32_t w_is_kn, uint16_t* out, void* stream);
/* All the operand copies of the weights a training step needs, in ONE launch (they are re-made after every optimiser
 * step): a table of jobs in DEVICE memory, built once per model.  kind 0 / 1 = bl_pack_weights_x6 with w_is_kn = kind
 * (w [G][N][K] / [G][K][N]); kind 2 = the fp32 transpose out[g][n][k] = w[g][k][n] (the W^T of bl_routed_dgrad_nodes);
 * kind 3 / 4 = bl_pack_weights_x6w (the wide row GEMM's image) with w_is_kn = kind - 3.
 * first_block = sum of bl_pack_job_blocks(...) of the jobs before; total_blocks = that sum over all jobs. */
typedef struct {
  const float* w;
  void* out;
  int32_t kind, G, K, N;
  int32_t first_block, pad_;
} bl_pack_job_t;
int64_t bl_pack_job_blocks(int32_t kind, int32_t G, int32_t K, int32_t N);
int bl_pack_weights_multi(const bl_pack_job_t* jobs_device, int32_t njobs, int32_t total_blocks, void* stream);
int bl_gemm_rows_x6(const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp,
                    int64_t b_group_stride, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M,
                    int32_t N, int32_t K, float* c, int32_t ldc, void* stream);
/* Wide form of bl_gemm_rows_x6 (csrc/bl_gemm_x6w.hip): 128 x 256 output tile, 8 waves, operands DMA'd into a double-buffered
 * LDS image (global_load_lds), ping-pong schedule.  Same contract, same summation order per element -- results are bit-identical
 * to bl_gemm_rows_x6 -- for the message GEMMs with >= 256 output columns and long K (ptgnn MlpMessagePassingLayer's per-type
 * Linear and its input gradient, call site buglab/models/gnnlayerdefs.py:6-23: the ConcatResidual layers of the hidden-128
 * model, every layer at hidden 256).  Shapes the layer calls send here: bl_gemm_rows_x6w_ok(N, K) -- N a multiple of 256, K a
 * multiple of 64 and >= 256 (the entry point itself takes any K >= 64 that is a multiple of 64).  The
 * weights come in their own image, bl_pack_weights_x6w (a 48 KB block per group, 256-column tile and 32-k stage in the exact
 * LDS layout; bl_packed_weight_elems_x6w uint16 elements; kinds 3 / 4 of bl_pack_weights_multi).  bl_set_rows_tile(128) makes bl_gemm_rows_x6w_ok return 0 (measurement switch; returns the previous tile). */
int32_t bl_gemm_rows_x6w_ok(int32_t N, int32_t K);
int32_t bl_set_rows_tile(int32_t cols);
int64_t bl_packed_weight_elems_x6w(int32_t G, int32_t K, int32_t N);
int bl_pack_weights_x6w(const float* w, int32_t G, int32_t K, int32_t N, int32_t w_is_kn, uint16_t* out, void* stream);
int bl_gemm_rows_x6w(const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp,
                     int64_t b_group_stride, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M,
                     int32_t N, int32_t K, float* c, int32_t ldc, void* stream);
/* the same with bl_gemm_rows' epilogue, C = drop(act(A . B_g + bias)): ptgnn MlpMessagePassingLayer's dense node update
 * Linear -> tanh -> Dropout (call site buglab/models/gnnlayerdefs.py:6-23) on the bf16 matrix cores */
int bl_gemm_rows_x6_epi(const bl_rows_packed_t* a, const uint16_t* bp, int64_t b_group_stride, const int32_t* group_ptr,
                        const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, const float* bias, int32_t act,
                        bl_dropout_t drop, float* c, int32_t ldc, void* stream);
/* Extended epilogues of the plain (one group) bf16x6 row GEMM: what the Linear layers of the relational transformer block
 * (reference buglab/models/layers/relational_transformer.py:104-124, multihead_attention.py:27-35) hand to the next kernel
 * without an elementwise pass in between (csrc/bl_great_layer.hip).
 *   BL_X6_EPI_ACT        c = drop(act(A . B + bias)), fp32                                     (= bl_gemm_rows_x6_epi)
 *   BL_X6_EPI_ACT_PACK   the same, written ONLY in bl_pack_bf16x3's form to c_packed [M, 3 N]  (act = relu: linear1 -> linear2)
 *   BL_X6_EPI_RES        c = A . B + res[row, 0:N], fp32                    (input gradient + the residual branch's gradient)
 *   BL_X6_EPI_MASK_PACK  c = (y != 0) ? A . B x mask_scale : 0 with y = drop(relu(z)) given by its packed form y_packed [M, 3 N]
 *                        (only the hi plane is read: y != 0 <=> kept and z > 0), written only packed to c_packed;
 *                        colsum[0:N] (optional) += the column sums of c (unordered atomics: not in deterministic mode)
 *                        -- the gradient through dropout(relu(.)) of linear1, its bias gradient and the operand of its
 *                        weight / input gradient GEMMs in the epilogue of linear2's input gradient. */
#define BL_X6_EPI_ACT 0
#define BL_X6_EPI_ACT_PACK 1
#define BL_X6_EPI_RES 2
#define BL_X6_EPI_MASK_PACK 3
typedef struct {
  int32_t form;
  const float* bias; /* ACT forms: [N] or NULL */
  int32_t act;
  bl_dropout_t drop;
  const float* res; /* RES */
  int32_t ld_res;
  const uint16_t* y_packed; /* MASK_PACK */
  float mask_scale;
  float* colsum;
  uint16_t* c_packed; /* ACT_PACK, MASK_PACK */
} bl_x6_epi_t;
int bl_gemm_rows_x6_epi2(const bl_rows_packed_t* a, const uint16_t* bp, int32_t M, int32_t N, int32_t K, const bl_x6_epi_t* epi,
                         float* c, int32_t ldc, void* stream);
/* bf16x6 form of bl_gemm_wgrad_routed (below): `a` packed rows, g_node_packed = bl_pack_bf16x3 of the
 * node gradient [*, N]; the message-major operands are transposed on the fly by gfx950's transposing
 * LDS read (ds_read_b64_tr_b16).  N and the source widths must be multiples of 32. */
int bl_gemm_wgrad_routed_x6(const bl_rows_packed_t* a, const uint16_t* g_node_packed, const int32_t* g_idx,
                            const uint32_t* win_bits, int32_t ld_bits, const int32_t* group_ptr, const int32_t* group_w,
                            int32_t G, int32_t M, int32_t N, int32_t K, float* gw, int64_t gw_group_stride, int32_t ld_gw,
                            void* stream);

/* Tile of the two bf16x6 weight-gradient GEMMs above.  256 (default): a 256 x 128 output tile per 8-wave workgroup with
 * double-buffered stages wherever K is a multiple of 256 and every source width a multiple of 128 -- the routed operand is
 * staged once per message instead of once per 128-feature half; 128: the 128 x 128 tile everywhere.  Same results either
 * way (same products, same per-tile accumulation order); a measurement switch (tools/gemm_bench.py).  Returns the
 * previous setting. */
int32_t bl_set_wgrad_tile(int32_t rows);

/* Most rows one workgroup of the two bf16x6 weight-gradient GEMMs above reduces before it adds its output tile into gw
 * (fp32 atomics: one flush = one tile of them).  The chunk is the smallest one that fills an integer number of rounds of
 * resident workgroups and stays <= the cap; rows < 256 are ignored.  Returns the previous cap. */
int32_t bl_set_wgrad_kchunk_cap(int32_t rows);

/* bf16x6 form of bl_gemm_wgrad (below), no routing: gw[g] += rows(a)^T . g_packed[g_idx[r] or r, 0:N] -- the weight
 * gradient of a plain Linear (the dense node update) from packed operands */
int bl_gemm_wgrad_x6(const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx, const int32_t* group_ptr,
                     const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, float* gw, int64_t gw_group_stride,
                     int32_t ld_gw, void* stream);

/* Weight-gradient GEMM (reduction over rows, split across row chunks, fp32 atomics):
 *   gw[group_w[g]][0:K, 0:N] += rows(a)[rows of g, 0:K]^T . g_c[rows of g, 0:N]
 * gw must be zeroed (or hold the running gradient) by the caller.  autograd equivalent:
 * the weight gradient of every Linear named above. */
int bl_gemm_wgrad(const bl_rows_t* a, const float* g_c, int32_t ld_g, const int32_t* group_ptr,
                  const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, float* gw,
                  int64_t gw_group_stride, int32_t ld_gw, void* stream);
/* the same with the routed right operand  g_c[r, n] = (winner[g_idx[r], n] == r) ? g_node[g_idx[r], n] : 0 */
int bl_gemm_wgrad_routed(const bl_rows_t* a, const float* g_node, int32_t ld_g, const int32_t* g_idx,
                         const int32_t* winner, int32_t ld_winner, const int32_t* group_ptr, const int32_t* group_w,
                         int32_t G, int32_t M, int32_t N, int32_t K, float* gw, int64_t gw_group_stride, int32_t ld_gw,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * M2(+M3a)  segmented max with argmax, optional fused LayerNorm.
 *   out[v, d] = max_{i in seg_ptr[v]..seg_ptr[v+1]} act(x[item(i), d]),  item(i) = seg_items ? seg_items[i] : i
 *   (act = BL_ACT_GELU_AGG: out[v, d] = gelu(max_i x[item(i), d]) -- the winner is the largest RAW item)
 *   arg[v, d] = that item (ties: first in segment order), -1 and out = 0 for an empty segment;
 *   if ln_g != NULL also  ln_out[v,:] = LayerNorm(out[v,:]; ln_g, ln_b, eps), mean[v], rstd[v];
 *   if dact != NULL also  dact[v, d] = act'(x[arg[v, d], d]) (0 for an empty segment): with it the
 *   backward pass needs only [nseg, D] arrays, never the [items, D] pre-activations again;
 *   if winbits != NULL also  winbits[item, w] bit b = (arg[seg(item), 32 w + b] == item), ceil(D/32)
 *   words per item: the routing table in the form the bf16x6 routed GEMMs read;
 *   seg_order (optional): a permutation of 0..nseg-1 = the order segments are processed in (the collator puts
 *   high-degree nodes first: one wave works through a 512-item hub for about as long as the whole launch takes).
 * Any width: D in 1..512 and ldx >= D need not be multiples of 4 (out, arg, dact are [nseg, D] without padding).
 * Replaces torch_scatter.scatter_max at ptgnn's "max" aggregation (gnnlayerdefs.py:11,21) and at
 * buglab/models/layers/localizationmodule.py:56-58, plus ptgnn's nn.LayerNorm. */
int bl_segment_max_fwd(const float* x, int32_t ldx, const int32_t* seg_ptr, const int32_t* seg_items, int32_t nseg,
                       int32_t D, int32_t act, float* out, int32_t* arg, const float* ln_g, const float* ln_b,
                       float eps, float* ln_out, float* mean, float* rstd, float* dact, uint32_t* winbits,
                       const int32_t* seg_order, void* stream);

/* backward of the segmented max, gather form (deterministic, no atomics):
 *   g_x[i, d] = (arg[seg_of[i], d] == i) ? g_out[seg_of[i], d] * act'(x[i, d]) : 0      (g_x may alias x)
 * Unlike bl_segment_max_fwd this one moves float4s: D and ldx (shared by x and g_x) must be multiples of 4 and g_out, x and
 * g_x 16-byte aligned -- a forward call at an odd width has no backward call here. */
int bl_segment_max_bwd(const float* g_out, const int32_t* arg, const float* x, int32_t ldx, const int32_t* seg_of,
                       int32_t nitems, int32_t D, int32_t act, float* g_x, void* stream);

/* LayerNorm backward (rows of even D <= 512):  g_x (times post_scale elementwise if not NULL -- used to
 * fold the message activation's derivative `dact` in), and g_gamma/g_beta ACCUMULATED with fp32 atomics.
 * g_x_packed (if not NULL; D % 8 == 0) also receives the result in bl_pack_bf16x3's packed form, the
 * operand of the bf16x6 routed GEMMs; g_x may then be NULL. */
int bl_layernorm_bwd(const float* g_y, const float* x, const float* mean, const float* rstd, const float* gamma,
                     int32_t nrows, int32_t D, float* g_x, float* g_gamma, float* g_beta, const float* post_scale,
                     uint16_t* g_x_packed, void* stream);

/* LayerNorm backward where the normalised tensor was  x + dropout(branch)  (the two sublayers of the relational transformer
 * block, reference relational_transformer.py:104-124): g_x (fp32, unmasked) is the residual's gradient, and the BRANCH's
 * gradient -- g_x through the dropout mask of the branch, element index row * D + d -- leaves in bl_pack_bf16x3's form
 * (g_branch_packed [nrows, 3 D], the operand of the branch Linear's two gradient GEMMs) with its column sums added to
 * g_bias (the Linear's bias gradient; may be NULL).  D a multiple of 8 up to 512.  branch_drop.p == 0: no mask. */
int bl_layernorm_bwd_branch(const float* g_y, const float* x, const float* mean, const float* rstd, const float* gamma,
                            int32_t nrows, int32_t D, float* g_x, float* g_gamma, float* g_beta, bl_dropout_t branch_drop,
                            float* g_bias, uint16_t* g_branch_packed, void* stream);

/* activation(+dropout) backward from the OUTPUT y of y = drop(act(z + bias)); g_bias (if not NULL)
 * accumulates column sums of g_z with fp32 atomics.  g_z may alias g_y.  (GELU is not supported
 * here: it needs the pre-activation, see bl_segment_max_bwd.) */
int bl_act_bwd(const float* g_y, const float* y, int32_t nrows, int32_t N, int32_t ld, int32_t act, bl_dropout_t drop,
               float* g_z, float* g_bias, void* stream);
/* the same with the result also (or only: g_z may then be NULL) in bl_pack_bf16x3's packed form [nrows, 3 N] (N % 8 == 0):
 * the operand of the bf16x6 input- and weight-gradient GEMMs of a Linear */
int bl_act_bwd_packed(const float* g_y, const float* y, int32_t nrows, int32_t N, int32_t ld, int32_t act, bl_dropout_t drop,
                      float* g_z, float* g_bias, uint16_t* g_z_packed, void* stream);

/* M1 backward, last step: gradient w.r.t. node states from the per-message input gradients
 *   g_h[n, 0:Din] (+)= sum_{e in src CSR of n} g_a[e, 0:Din] + sum_{e in tgt CSR of n} g_a[e, Din:2Din]
 * (deterministic segmented sums; replaces autograd's index_add of the two h[...] gathers).
 * tgt_ptr == tgt_msgs == NULL: source half only (messages built from h[src] alone, `ggnn`).
 * Any width: Din in 1..512; ld_ga >= 2 Din (Din without the target half) and ld_gh >= Din need not be multiples of 4. */
int bl_mp_scatter_grad(const float* g_a, int32_t ld_ga, const int32_t* src_ptr, const int32_t* src_msgs,
                       const int32_t* tgt_ptr, const int32_t* tgt_msgs, int32_t N, int32_t Din, int32_t accumulate,
                       float* g_h, int32_t ld_gh, const int32_t* node_order,
                       void* stream);

/* the same with the columns 0..split-1 written to g_h_lo and split..Din-1 to g_h_hi: the gradients of the two
 * inputs of a folded ConcatResidual ([stash ; current]), each in its own contiguous matrix */
int bl_mp_scatter_grad_split(const float* g_a, int32_t ld_ga, const int32_t* src_ptr, const int32_t* src_msgs,
                             const int32_t* tgt_ptr, const int32_t* tgt_msgs, int32_t N, int32_t Din, int32_t split,
                             float* g_h_lo, int32_t ld_lo, float* g_h_hi, int32_t ld_hi, const int32_t* node_order,
                             void* stream);

/* Routed input gradient of the message layer from the NON-ZEROS of the message gradient alone (vector units, exact
 * fp32): the max aggregation gives every (node, channel) gradient to ONE message, so only N * Dm of the E * Dm entries
 * the routed GEMM multiplies are non-zero.  gq [*, Dm] fp32 = d loss / d (winning pre-activation) per node, wt =
 * W transposed [T, Dm, 2 Din], win_bits / type_ptr as in bl_gemm_rows_x6 (messages type-major, target-sorted inside a type).
 *   bl_routed_dgrad_vec    writes the per-message rows g_a[e, :] = sum_{d won by e} gq[tgt(e), d] * W[type(e)][:, d]
 *                          (the result of the routed bl_gemm_rows_x6 up to fp32 summation order);
 *   bl_routed_dgrad_nodes  adds them straight into the node gradient: g_h[src(e), 0:Din] += g_a[e, 0:Din] per message,
 *                          g_h[tgt, 0:Din] += sum over a run of messages sharing the target of g_a[e, Din:2Din] (fp32 atomics;
 *                          the caller zeroes g_h).  Columns < split go to g_h_lo, the rest to g_h_hi (split == Din: one output).
 *                          = bl_routed_dgrad_vec + bl_mp_scatter_grad without the [E, 2 Din] round trip through memory.
 * Both replace the autograd of ptgnn's gather + per-type Linear + torch_scatter.scatter_max (call site
 * buglab/models/gnnlayerdefs.py:6-23).  bl_routed_dgrad_vec_ok: whether (Dm, K2 = 2 Din) is supported (W[t]^T must fit
 * one 128 KB LDS block: Dm in {64, 128}, K2 in {128, 256}, Dm * K2 <= 32768). */
int32_t bl_routed_dgrad_vec_ok(int32_t Dm, int32_t K2);
int bl_routed_dgrad_vec(const float* gq, int32_t ld_gq, const int32_t* msg_tgt, const uint32_t* win_bits, int32_t ld_bits,
                        const int32_t* type_ptr, int32_t T, const float* wt, int32_t E, int32_t Dm, int32_t K2, float* g_a,
                        int32_t ld_ga, void* stream);
int bl_routed_dgrad_nodes(const float* gq, int32_t ld_gq, const int32_t* msg_src, const int32_t* msg_tgt,
                          const uint32_t* win_bits, int32_t ld_bits, const int32_t* type_ptr, int32_t T, const float* wt,
                          int32_t E, int32_t Dm, int32_t Din, int32_t split, float* g_h_lo, int32_t ld_lo, float* g_h_hi,
                          int32_t ld_hi, void* stream);
/* bl_routed_dgrad_nodes with the SOURCE half kept per message: g_src[e, 0:Din] = g_a[e, 0:Din] as plain rows (g_src != NULL;
 * summed per node afterwards by bl_mp_scatter_grad over the source CSR with accumulate = 1), the target half by atomics as
 * above.  Halves the fp32 atomics, which bound the all-atomic form (one 4-byte atomic per L2 channel per clock). */
int bl_routed_dgrad_nodes_rows(const float* gq, int32_t ld_gq, const int32_t* msg_src, const int32_t* msg_tgt,
                               const uint32_t* win_bits, int32_t ld_bits, const int32_t* type_ptr, int32_t T, const float* wt,
                               int32_t E, int32_t Dm, int32_t Din, int32_t split, float* g_h_lo, int32_t ld_lo, float* g_h_hi,
                               int32_t ld_hi, float* g_src, int32_t ld_src, void* stream);

/* GRU cell of the gated (`ggnn`) node update -- the elementwise part of torch.nn.GRUCell (gate order
 * r | z | n) after gi = x W_i + b_i and gh = h W_h + b_h [N, 3D] were produced by bl_gemm_rows:
 *   h' = drop((1 - z) * tanh(gi_n + r * gh_n) + z * h).  Replaces ptgnn GatedMessagePassingLayer's
 * nn.GRUCell state update (reference call site buglab/models/gnnlayerdefs.py:42-68).
 * bwd writes g_gi, g_gh [N, 3D] and the direct part of g_h (z * g_out) [N, D].  Any width: D and ld_h >= D need not be
 * multiples of 4; gi, gh, out and the gradients are contiguous. */
int bl_gru_cell_fwd(const float* gi, const float* gh, const float* h, int32_t ld_h, int32_t N, int32_t D,
                    bl_dropout_t drop, float* out, void* stream);
int bl_gru_cell_bwd(const float* g_out, const float* gi, const float* gh, const float* h, int32_t ld_h, int32_t N,
                    int32_t D, bl_dropout_t drop, float* g_gi, float* g_gh, float* g_h, void* stream);

/* Time recurrence of one BIDIRECTIONAL GRU layer over a padded [B, L] minibatch (`seq-gru`): replaces torch.nn.GRU(bidirectional,
 * batch_first) applied to a PackedSequence (reference buglab/models/seqmodel.py:119-126, called at :385-392 between
 * pack_padded_sequence(lengths, enforce_sorted=False) and pad_packed_sequence): every sequence runs over its own length, the
 * reverse direction starts at its last real token, positions >= lens[b] come back as zeros.  Row b * L + t everywhere.
 *   gi   [B L, >= 6 Hh]  x W_ih + b_ih of both directions, columns [direction][r | z | n][Hh]  (one row GEMM outside)
 *   w_hh [2][Hh][3 Hh]   gh = h . w_hh[direction] + b_hh[direction]   (torch's weight_hh_l{k}{_reverse}, transposed); b_hh [2][3 Hh]
 *   out  [B L, >= 2 Hh]  forward direction in columns 0 .. Hh - 1, reverse in Hh .. 2 Hh - 1
 *   saved  bl_gru_scan_saved_elems floats kept for bl_gru_scan_bwd (NULL: forward only), gates [2][B L][r | z | n | gh_n] then h_prev [2][B L][Hh]
 * Hh in {32, 64, 128}.  One workgroup per (sequence, direction); exact fp32 arithmetic.
 * bwd: g_out [B L, >= 2 Hh] -> g_gi [B L, >= 6 Hh] (gradient of gi; zeros at padded rows) and g_gh [2][B L][3 Hh] (gradient of
 * the recurrent pre-activations: the caller forms g_w_hh[d] = h_prev[d]^T g_gh[d] (bl_gemm_wgrad on saved's h_prev block) and
 * g_b_hh[d] = column sums of g_gh[d]). */
int64_t bl_gru_scan_saved_elems(int32_t B, int32_t L, int32_t Hh);
int bl_gru_scan_fwd(const float* gi, int32_t ld_gi, const float* w_hh, const float* b_hh, const int32_t* lens, int32_t B, int32_t L,
                    int32_t Hh, float* out, int32_t ld_out, float* saved, void* stream);
int bl_gru_scan_bwd(const float* g_out, int32_t ld_g, const float* w_hh, const float* saved, const int32_t* lens, int32_t B, int32_t L,
                    int32_t Hh, float* g_gi, int32_t ld_ggi, float* g_gh, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ONE MlpMessagePassingLayer per call (SURVEY.md section 8b's minimum set).  Replaces ptgnn's
 * MlpMessagePassingLayer.forward and its autograd; kwargs of the reference call site
 * buglab/models/gnnlayerdefs.py:6-23 map to Din = input_state_dimension, Dm = message_dimension,
 * Dout = output_state_dimension, T = num_edge_types, aggregation "max", drop.p = dropout_rate.
 *   msg_act BL_ACT_GELU_AGG (ptgnn's order as recollected, the product's default):
 *     m_e = [h_src ; h_tgt] . W[type(e)];  a_v = gelu(max_{e -> v} m_e) (0 if none);
 *   msg_act BL_ACT_GELU: m_e = gelu([h_src ; h_tgt] . W[type(e)]);  a_v = max_{e -> v} m_e (0 if none);  BL_ACT_NONE: no gelu;
 *   h'_v = Dropout(tanh(LayerNorm(a_v; ln_g, ln_b, ln_eps) . Wd + bd))
 * Widths: Din, Dm multiples of 32 (the message GEMMs run as bf16x6), Dm <= 512.  Messages are type-major
 * (type_ptr [T+1]) and target-sorted inside a type; tgt_ptr/tgt_msgs and src_ptr/src_msgs are the CSRs node ->
 * incoming / outgoing message ids; node_order (optional) = processing order of the per-node kernels. */
typedef struct {
  int32_t N, E, T, Din, Dm, Dout;
  const int32_t *msg_src, *msg_tgt, *type_ptr, *tgt_ptr, *tgt_msgs, *src_ptr, *src_msgs, *node_order;
  const float* W;                 /* [T, 2 Din, Dm] */
  const float *ln_g, *ln_b;       /* [Dm] */
  const float* Wd;                /* [Dm, Dout] */
  const float* bd;                /* [Dout] */
  int32_t msg_act;                /* BL_ACT_GELU_AGG, BL_ACT_GELU or BL_ACT_NONE */
  float ln_eps;
  bl_dropout_t drop;
  const float* Wt;                /* optional (backward only): W transposed, [T, Dm, 2 Din].  When given and
                                   * bl_routed_dgrad_vec_ok(Dm, 2 Din), the input gradient is computed from the non-zeros of
                                   * the routed message gradient (bl_routed_dgrad_nodes; bl_routed_dgrad_vec + bl_mp_scatter_grad
                                   * in the deterministic mode) instead of the routed matrix-core GEMM; NULL: matrix cores */
  const uint16_t* Wd_packed;      /* optional: bl_pack_weights_x6(Wd, 1, Dm, Dout, w_is_kn = 1).  When given (and Dm, Dout are
                                   * multiples of 32) the dense node update runs as bf16x6 GEMMs: forward, input gradient and
                                   * weight gradient; the same layer's backward call must then also carry ... */
  const uint16_t* Wd_packed_bwd;  /* ... bl_pack_weights_x6(Wd, 1, Dout, Dm, w_is_kn = 0), the form of g_ln = g_z . Wd^T.
                                   * NULL / NULL: exact-fp32 MFMA GEMMs (bl_gemm_rows / bl_gemm_wgrad) */
  int32_t num_hub_slots;          /* how many leading entries of node_order may be hubs (nodes with very long target segments get
                                   * a whole workgroup in the segmented max); < 0: unknown -- the first 4096 are looked at;
                                   * 0: no hubs -- node_order is then not read at all (the collators list the hubs first and every
                                   * other node in natural order, i.e. the identity; any order gives the same results) */
  int32_t aggregation;            /* BL_AGG_MAX (0: the reference's recipe, gnnlayerdefs.py:11,21), BL_AGG_SUM or BL_AGG_MEAN -- ptgnn's other
                                   * message_aggregation_function values: a_v = act(sum_{e -> v} m_e (/ in-degree)), 0 for a node without
                                   * messages; msg_act must then be BL_ACT_GELU_AGG or BL_ACT_NONE; no winner table (winner_out untouched), every
                                   * message receives its target's gradient in backward (unrouted GEMMs on the matrix cores) */
  /* Optional: the RUNS of the minibatch (maximal consecutive messages of one type with one target; the collators make these
   * arrays, buglab/data/collate.py::message_run_arrays).  The routing masks of a run's members are disjoint and the target
   * halves of their input and weight gradients are summed anyway, so backward computes a run's target half as ONE GEMM row with
   * the OR of the masks: the routed f16x3 GEMMs then run over E + R rows of Din columns (rows 0..E-1 the messages' source
   * halves, rows E..E+R-1 the runs' target halves) instead of E rows of 2 Din.  num_runs == 0 or run_ptr == NULL: none.
   * With run arrays the routing bitmask inside `saved` has E + num_runs rows: size it with bl_mp_layer_saved_bytes(N, E +
   * num_runs, ...) and hand the SAME arrays to forward and backward.  Taken (bl_set_run_rows) by the f16x3 mode with max
   * aggregation, matrix-core input gradient and Din a multiple of 128; every other configuration ignores the arrays. */
  int32_t num_runs;               /* R <= E */
  const int32_t* run_ptr;         /* [R + 1] message range of every run */
  const int32_t* bwd_group_ptr;   /* [2 T + 1] groups 0..T-1: the types over message rows; T..2T-1: the types over run rows (+ E) */
  const int32_t* bwd_group_w;     /* [2 T] weight slice of a group, W viewed as [2 T, Din, Dm]: g -> 2 g, T + g -> 2 g + 1 */
  const int32_t* bwd_rows_tgt;    /* [E + R] = [msg_tgt ; run target] */
  const int32_t* bwd_rows_src;    /* [E + R] = [msg_src ; run target] */
  const int32_t* tgt_run_ptr;     /* [N + 1] CSR node -> the rows of its runs ... */
  const int32_t* tgt_run_rows;    /* [R]     ... E + run id, ascending */
  /* Optional: the LIVE ROWS of this layer (the collators make these arrays per minibatch and layer,
   * buglab/data/collate.py::live_set_arrays).  By handing them in the caller states that g_out is zero outside the rows
   * live_nodes: the heads read the encoder's output through one gather of a few rows, and a layer's input can receive a
   * gradient only at the layer's live nodes and at the sources of the messages into them (live_recv = the layer below's
   * live_nodes).  Backward then runs over the live rows only -- N' nodes, the E' messages and R' runs into them -- and writes
   * the rows live_recv of g_h_lo / g_h_hi, every other row zero.  Taken where the run-row path and bl_node_update_bwd apply
   * (bl_set_live_backward); every other configuration ignores the arrays.  live_nodes == NULL: none.
   * FORWARD reads them only with live_fwd set (below); without it they may be filled or not, bl_mp_layer_fwd ignores them. */
  int32_t live_num_nodes;           /* N' */
  int32_t live_num_recv;            /* N'' */
  int32_t live_num_msgs;            /* E' (messages keep their order: type-major, target-sorted inside a type) */
  int32_t live_num_runs;            /* R' */
  const int32_t* live_nodes;        /* [N']  node ids, ascending */
  const int32_t* live_recv;         /* [N''] node ids, ascending: live_nodes and the sources of the live messages */
  const int32_t* live_msgs;         /* [E']  message ids, ascending (rows of the routing bitmask) */
  const int32_t* live_run_ptr;      /* [R' + 1] range of every live run in 0..E' */
  const int32_t* live_group_ptr;    /* [2 T + 1] bwd_group_ptr of the E' + R' rows (weight slices: bwd_group_w) */
  const int32_t* live_rows_tgt;     /* [E' + R'] target of a message / run as a position in live_nodes */
  const int32_t* live_rows_src;     /* [E' + R'] [source node id of a message ; target node id of a run] */
  const int32_t* live_src_ptr;      /* [N'' + 1] CSR position in live_recv -> live messages it is the source of ... */
  const int32_t* live_src_msgs;     /* [E']      ... as rows 0..E'-1, ascending */
  const int32_t* live_run_csr_ptr;  /* [N'' + 1] CSR position in live_recv -> rows of the live runs into it ... */
  const int32_t* live_run_csr_rows; /* [R']      ... E' + run, ascending */
  /* Live rows in FORWARD too.  The same reachability run upwards: with the heads' gather as the only reader, the output of this layer
   * is needed only at the rows live_nodes, and its input only at live_recv.  Non-zero: the caller states (a) that nothing reads h_out
   * outside the rows live_nodes -- the layer above runs live as well, so it reads its live_recv = this layer's live_nodes -- and
   * (b) that the input is valid at least on the rows live_recv.  bl_mp_layer_fwd then computes those rows only (each bit-identical to
   * the full forward's) and leaves the saved state valid on the live rows / live messages only; bl_mp_layer_bwd, handed the same
   * value, takes the live path or returns BL_EINVAL -- never the full backward over half-valid state.  Set it only after
   * bl_mp_layer_live_ok(L, ..., forward = 1) said yes.  BL_LIVE_FWD_LAST additionally zero-fills h_out first (the layer whose output
   * is handed out as the encoder's), BL_LIVE_FWD_INNER leaves the other rows untouched (uninitialised). */
  int32_t live_fwd;
} bl_mp_layer_t;
#define BL_LIVE_FWD_INNER 1
#define BL_LIVE_FWD_LAST 2
#define BL_AGG_MAX 0
#define BL_AGG_SUM 1
#define BL_AGG_MEAN 2

/* buffer sizes (bytes): `saved` is written by forward and read by backward; the workspace is scratch of one call.
 * backward: 0 = forward call, 1 = backward call, 2 = backward call that will take the bl_routed_dgrad_nodes_rows path (Wt
 * given, shape supported, deterministic mode off): [E, Din] source-half rows instead of the [E, 2 Din] per-message gradient,
 * 3 = forward-only call (bl_mp_layer_fwd with saved == NULL: the workspace then also holds the packed input and the
 * LayerNorm output).  E sizes the routing bitmask of `saved` and nothing else: a descriptor with run arrays passes E + num_runs. */
int64_t bl_mp_layer_saved_bytes(int32_t N, int32_t E, int32_t Din, int32_t Dm, int32_t msg_act);
int64_t bl_mp_layer_workspace_bytes(int32_t N, int32_t E, int32_t Din, int32_t Dm, int32_t Dout, int32_t backward);
/* uint16 elements of the packed weights a layer call takes: bl_pack_weights_x6(W, T, 2 Din, Dm, w_is_kn = 1) for
 * forward, bl_pack_weights_x6(W, T, Dm, 2 Din, w_is_kn = 0) for backward (pack once per optimiser step) -- or, where
 * bl_mp_layer_weight_image(Din, Dm, for_backward) returns 1 (the layer's GEMM of that direction has a multiple of 256
 * output columns: the wide row GEMM runs it), bl_pack_weights_x6w with the same arguments.  The answer depends on the shape
 * and on bl_set_rows_tile only: choose the tile before packing. */
int32_t bl_mp_layer_weight_image(int32_t Din, int32_t Dm, int32_t for_backward);
int64_t bl_mp_layer_packed_weight_elems(int32_t T, int32_t Din, int32_t Dm, int32_t for_backward);

/* forward.  The layer input is h_lo [N, width_lo] alone (h_hi NULL, width_lo == Din) or the virtual concatenation
 * [h_lo ; h_hi] of a ConcatResidual layer (gnnlayerdefs.py:24-38), never materialised.  winner_out (optional,
 * int32 [N, Dm]): the arg-max message per (node, channel), -1 = none.  saved == NULL: forward-only call (the reference's
 * predict / evaluate path, buglab/models/gnn.py:606-645) -- nothing is stored for a backward pass (no routing bitmask,
 * activation derivative, aggregate, LayerNorm statistics), ws is sized by bl_mp_layer_workspace_bytes(..., 3). */
int bl_mp_layer_fwd(const bl_mp_layer_t* L, const float* h_lo, int32_t ld_lo, int32_t width_lo, const float* h_hi,
                    int32_t ld_hi, const uint16_t* w_packed, float* h_out, int32_t* winner_out, void* saved, void* ws,
                    void* stream);
/* backward.  g_h_lo / g_h_hi are written; g_W, g_ln_g, g_ln_b, g_Wd, g_bd are ACCUMULATED into (fp32 atomics):
 * hand in zeroed buffers or the running gradients.  side_stream (optional): the two weight-gradient GEMMs run
 * there next to the input-gradient chain; with join_side == 0 they are left running (the caller joins the
 * streams before it reads the weight gradients, and keeps `saved` / `ws` alive until then). */
int bl_mp_layer_bwd(const bl_mp_layer_t* L, const float* h_out, const float* g_out, const uint16_t* w_packed_bwd,
                    const void* saved, void* ws, float* g_h_lo, int32_t ld_lo, int32_t width_lo, float* g_h_hi,
                    int32_t ld_hi, float* g_W, float* g_ln_g, float* g_ln_b, float* g_Wd, float* g_bd, void* stream,
                    void* side_stream, int32_t join_side);

/* Backward of the layer's node update  h_out = drop(tanh(LayerNorm(agg) . Wd + bd))  from g_out, in one kernel per 64-node
 * tile (ptgnn MlpMessagePassingLayer's LayerNorm -> Linear -> tanh -> Dropout tail; call site
 * buglab/models/gnnlayerdefs.py:6-23):
 *   g_z = g_out . dropout mask . (1 - tanh^2)      -> g_z_packed [nrows, 3 Dout] (bl_pack_bf16x3 form; the operand of the dense
 *                                                     weight-gradient GEMM), g_bias [Dout] += its column sums (may be NULL)
 *   g_ln = g_z . Wd^T                              (bf16x6; wd_packed_bwd = bl_pack_weights_x6(Wd, 1, Dm, Dout, w_is_kn = 0))
 *   gq = LayerNorm backward(g_ln; agg, mean, rstd, ln_g) x dact   -> gq [nrows, Dm] fp32 and / or gq_packed [nrows, 3 Dm]
 *   g_ln_g, g_ln_b [Dm] += the gamma / beta gradients
 * = bl_act_bwd_packed + bl_gemm_rows_x6_epi + bl_layernorm_bwd without the g_z / g_ln round trips.  dact (the message
 * activation's derivative at the winners) may be NULL (= 1).  Shapes: bl_node_update_bwd_ok(Dm, Dout) -- Dm 128 or 256,
 * Dout a multiple of 32 up to 256, deterministic mode off (the column sums are flushed by unordered atomics). */
int32_t bl_node_update_bwd_ok(int32_t Dm, int32_t Dout);
int bl_node_update_bwd(const float* g_out, const float* h_out, int32_t nrows, int32_t Dout, bl_dropout_t drop,
                       const uint16_t* wd_packed_bwd, const float* agg, const float* mean, const float* rstd, const float* ln_g,
                       const float* dact, int32_t Dm, uint16_t* g_z_packed, float* g_bias, float* gq, uint16_t* gq_packed,
                       float* g_ln_g, float* g_ln_b, void* stream);
/* A/B switch: 1 (default) = bl_mp_layer_bwd uses bl_node_update_bwd where it applies, 0 = the three kernels it replaces.
 * Returns the previous value. */
int32_t bl_set_fused_node_bwd(int32_t on);

/* The pieces of bl_mp_layer_bwd's run-row path (bl_mp_layer_t.num_runs; backward of the per-type Linear + scatter-max of
 * ptgnn's MlpMessagePassingLayer, buglab/models/gnnlayerdefs.py:6-23).
 *   bl_winbits_or_runs: bits[E + r, 0:words] = OR over e in run_ptr[r] .. run_ptr[r + 1] of bits[e, 0:words], behind the E
 *     message rows of the same buffer (rows ld_bits words apart).
 *   bl_mp_scatter_grad_runs: bl_mp_scatter_grad / _split (g_h_hi != NULL: columns >= split go there) with both halves at
 *     column 0 of g_a: g_h[n] = sum_{e in src CSR of n} g_a[e, 0:Din] + sum_{row in run CSR of n} g_a[row, 0:Din];
 *     num_hub_slots as in bl_mp_layer_t.
 *   bl_set_run_rows: A/B switch, 1 (default; BL_RUN_ROWS=0 in the environment starts with 0) = bl_mp_layer_bwd takes the
 *     run-row path where it applies, 0 = the per-message launches on the same arrays.  Returns the previous value. */
int bl_winbits_or_runs(uint32_t* bits, int32_t ld_bits, const int32_t* run_ptr, int32_t E, int32_t R, int32_t words, void* stream);
int bl_mp_scatter_grad_runs(const float* g_a, int32_t ld_ga, const int32_t* src_ptr, const int32_t* src_msgs,
                            const int32_t* tgt_run_ptr, const int32_t* tgt_run_rows, int32_t N, int32_t Din, int32_t split,
                            float* g_h_lo, int32_t ld_lo, float* g_h_hi, int32_t ld_hi, const int32_t* node_order,
                            int32_t num_hub_slots, void* stream);
int32_t bl_set_run_rows(int32_t on);
/* The pieces of bl_mp_layer_bwd's live-row path (bl_mp_layer_t.live_nodes):
 *   bl_winbits_gather: out[i, 0:words] = bits[rows[i], 0:words] for i < n (rows ld_bits / ld_out words apart; bits has nrows_in
 *     rows) -- the compact copy of the live messages' routing masks.
 *   bl_node_update_bwd_rows: bl_node_update_bwd over the nodes rows[0..nrows-1]: every per-node input (g_out, h_out, agg, mean,
 *     rstd, dact) is read at row rows[i], the dropout mask is that row's, g_z_packed / gq / gq_packed are written at row i.
 *   bl_mp_scatter_grad_rows: bl_mp_scatter_grad_runs over CSRs of `n` segments whose sums go to row out_rows[i] of g_h_lo /
 *     g_h_hi (other rows untouched).
 *   bl_set_live_backward: A/B switch, 1 (default; BL_LIVE_BWD=0 in the environment starts with 0) = bl_mp_layer_bwd takes the
 *     live-row path where it applies, 0 = the full backward on the same descriptor.  Returns the previous value;
 *     bl_get_live_backward the current one. */
int bl_winbits_gather(const uint32_t* bits, int32_t ld_bits, int32_t nrows_in, const int32_t* rows, int32_t n, int32_t words,
                      uint32_t* out, int32_t ld_out, void* stream);
int bl_node_update_bwd_rows(const float* g_out, const float* h_out, const int32_t* rows, int32_t nrows, int32_t Dout, bl_dropout_t drop,
                            const uint16_t* wd_packed_bwd, const float* agg, const float* mean, const float* rstd, const float* ln_g,
                            const float* dact, int32_t Dm, uint16_t* g_z_packed, float* g_bias, float* gq, uint16_t* gq_packed,
                            float* g_ln_g, float* g_ln_b, void* stream);
int bl_mp_scatter_grad_rows(const float* g_a, int32_t ld_ga, const int32_t* src_ptr, const int32_t* src_msgs,
                            const int32_t* run_csr_ptr, const int32_t* run_csr_rows, const int32_t* out_rows, int32_t n, int32_t Din,
                            int32_t split, float* g_h_lo, int32_t ld_lo, float* g_h_hi, int32_t ld_hi, void* stream);
int32_t bl_set_live_backward(int32_t on);
int32_t bl_get_live_backward(void);
/* The live rows in forward (bl_mp_layer_t.live_fwd):
 *   bl_mp_layer_live_ok: THE decision whether a layer call runs over its live rows, one host function for both directions (no GPU
 *     work).  1 when the descriptor carries the live arrays and: live backward on, run rows on and present, f16x3 three-term
 *     message GEMMs, max aggregation, matrix-core input gradient (have_w_packed_bwd: backward gets / got the packed W^T image, and
 *     L->Wt does not select the vector path), Din a multiple of 128, dense update on bf16x6 (L->Wd_packed), the one-kernel node
 *     update backward applies (which excludes the deterministic mode), the dropout counter of a node's own row fits 32 bits, the
 *     compact gradient + masks fit the backward workspace.  forward != 0 adds: live forward on (bl_set_live_forward), no winner
 *     table (want_winners == 0), compact pre [E', Dm] + message-position map [E] + target ids [E'] fit the forward workspace
 *     bl_mp_layer_workspace_bytes(.., 0).  0 otherwise, the reason then in bl_last_error().  The caller asks from the LAST layer
 *     downwards and sets live_fwd on the longest run of layers from the top that all pass.
 *   bl_set_live_forward: A/B switch, 1 (default; BL_LIVE_FWD=0 in the environment starts with 0); it applies only where the live
 *     backward is on.  0: every kernel and launch as without it.  Returns the previous value; bl_get_live_forward the current one.
 *   bl_pack_f16x2_rows: bl_pack_f16x2 (fixed scale) for the rows rows[0..R-1] of x, each written at its own row of `out`; no other
 *     row of x is read, none of out written.
 *   bl_gemm_rows_x6_epi_rows: bl_gemm_rows_x6_epi (one group, bias / tanh / dropout) whose result row i goes to row out_rows[i]
 *     (< nrows_out) of c with that row's dropout counter (row * N + column): bit-identical to the same rows of the full launch. */
int32_t bl_mp_layer_live_ok(const bl_mp_layer_t* L, int32_t have_w_packed_bwd, int32_t forward, int32_t want_winners);
int32_t bl_set_live_forward(int32_t on);
int32_t bl_get_live_forward(void);
int bl_pack_f16x2_rows(const float* x, int32_t ld, const int32_t* rows, int32_t R, int32_t D, int32_t D_total, int32_t col_off,
                       float scale, uint16_t* out, void* stream);
int bl_gemm_rows_x6_epi_rows(const bl_rows_packed_t* a, const uint16_t* bp, int32_t M, int32_t N, int32_t K, const float* bias,
                             int32_t act, bl_dropout_t drop, const int32_t* out_rows, int32_t nrows_out, float* c, int32_t ldc,
                             void* stream);

/* optional per-kernel timing of the launches made inside bl_mp_layer_fwd / _bwd (HIP events on the stream each
 * kernel is launched on); read after a device synchronisation.  bench.py's roofline numbers come from here. */
int bl_prof_enable(int32_t on);
int bl_prof_reset(void);
int bl_prof_num_kinds(void);
const char* bl_prof_kind_name(int32_t kind);
int bl_prof_read(int32_t kind, double* ms, double* flop, int64_t* launches, int32_t* overlapped);
double bl_prof_read_bytes(int32_t kind); /* algorithmic bytes recorded with a memory-bound kind's launches (0: none) */

/* ---------------------------------------------------------------------------------------------
 * fp32-accurate GEMMs on the fp16 matrix cores ("f16x3", csrc/bl_gemm_h3.hip): the second operand split of the message-passing
 * GEMMs.  An fp32 operand x, multiplied by a power-of-two scale s of its tensor, is split into TWO fp16 planes hi + lo
 * (22+ significant bits where |x s| >= 2^-3; an absolute error of 2^-25 / s below; finite values saturate at 65504 / s); a
 * product is three fp16 MFMA terms hh + hl + lh with fp32 accumulation, times 1 / (s_a s_b): half the matrix-pipe work and
 * two thirds of the operand bytes of bf16x6 at fp32-class accuracy (error vs fp64 below a plain fp32 matmul's) -- for tensors
 * whose range is bounded or measured.  Same contracts as the bf16x6 entry points they mirror (ptgnn MlpMessagePassingLayer's
 * per-type Linear forward / backward, buglab/models/gnnlayerdefs.py:6-23).
 *   packed rows: two planes back to back per row, [hi x D | lo x D] halves (4 D bytes);
 *   bl_pack_f16x2: rows of x[:, 0:D] into columns col_off .. col_off + D of D_total-wide packed rows (a ConcatResidual pair is
 *     packed in two calls); effective scale = scale x (amax_dev ? 2^(14 - ceil(log2 *amax_dev)) : 1) -- amax_dev: device float
 *     holding max |x| of the tensor (gradient tensors, whose magnitude is not known in advance; bl_amax or a producing kernel);
 *   bl_amax: *amax_dev = max(*amax_dev, max |x[0:n]|) (zero it first);
 *   bl_pack_weights_h3 / bl_packed_weight_elems_h3: tiled weight image (16 KB block per group, 128-column tile, 32-k stage);
 *   bl_gemm_rows_h3: C[rows of g] = out_scale x rows(a) . B_g (+ routed left operand with win_bits); out_scale = 1 / (s_a s_b),
 *     divided by 2^(14 - ceil(log2 *a_amax_dev)) when a_amax_dev is given (left operand packed with a device amax);
 *   bl_gemm_wgrad_h3: gW_g += out_scale x rows(a)^T . G rows (g_idx gather, win_bits routing as bl_gemm_wgrad_routed_x6);
 *     g_amax_dev: the device amax G was packed with. */
#define BL_H3_ROW_SCALE 256.0f /* layer inputs: |h| <= 1.25 after tanh x dropout, embedding rows O(1); saturation at 255.9 */
#define BL_H3_W_SCALE 64.0f    /* weights: saturation at 1023 */
/* which split the message GEMMs of bl_mp_layer_fwd / _bwd use: 1 = f16x3 (default), 0 = bf16x6, 2 = f16x1 -- the f16x3 images
 * and kernels with the high-plane term only (fp16 operands, fp32 accumulation and results, gradient operand scaled by its
 * device-side amax): the reduced-precision mode behind the reference's `train.py --amp` (/root/reference/buglab/models/train.py:8,106),
 * never the default and never the benchmarked headline.  BL_MSG_GEMM=x6 / h3 / amp in the environment sets the initial value.
 * Returns the previous mode.  bl_mp_layer_weight_image returns 2 (f16x3 image) in modes 1 and 2. */
int32_t bl_set_msg_gemm_mode(int32_t mode);
int32_t bl_get_msg_gemm_mode(void);
/* Operand split of the packed-row GEMMs behind the sequence models' Linear layers -- bl_gemm_rows_x6, bl_gemm_rows_x6_epi,
 * bl_gemm_rows_x6_epi2, bl_gemm_rows_x6w and bl_gemm_wgrad_x6, op by op and inside bl_great_layer_fwd / _bwd:
 *   0  bf16x6 (default): three bf16 planes per operand, six MFMA terms, fp32-equivalent;
 *   1  bf16x1: the same packed images, HIGH PLANES ONLY -- the other two are neither loaded nor staged -- one bf16 MFMA term per
 *      16 k's, fp32 accumulation, every epilogue unchanged (a packed result stays a full three-plane image).  The reduced-precision
 *      mode behind the reference's `train.py --amp` (reference buglab/models/train.py:8,106: autocast) for seq-great, seq-rat,
 *      seq-transformer and seq-gru's input projections; attention products, LayerNorm, heads, losses, the GRU recurrence and the
 *      optimiser stay fp32.  Never the default and never the benchmarked headline.
 * BL_SEQ_GEMM=x1 / bf16x1 / amp in the environment sets the initial value.  bl_set_seq_gemm_mode returns the previous mode, or
 * BL_EINVAL for any other value (the mode is then unchanged).  bl_great_layer_fwd records the mode its `saved` was written in (a host-side
 * table keyed by the pointer: nothing is read back from the device); bl_great_layer_bwd returns BL_EINVAL when the current mode differs.  bl_gemm_wgrad_routed_x6 (a message GEMM) does not follow this switch. */
int32_t bl_set_seq_gemm_mode(int32_t mode);
int32_t bl_seq_gemm_mode(void);
/* packing threads that had to saturate a finite value at +-65504 since the last reset, on the current device (synchronises; -1 if
 * the counter is unavailable): 0 in a healthy run -- the trainer checks it once per epoch (runtime/trainer.py). */
int64_t bl_h3_saturation_events(int32_t reset);
int bl_pack_f16x2(const float* x, int32_t ld, int64_t R, int32_t D, int32_t D_total, int32_t col_off, float scale,
                  const float* amax_dev, uint16_t* out, void* stream);
int bl_amax(const float* x, int64_t n, float* amax_dev, void* stream);
int64_t bl_packed_weight_elems_h3(int32_t G, int32_t K, int32_t N);
int bl_pack_weights_h3(const float* w, int32_t G, int32_t K, int32_t N, int32_t w_is_kn, float scale, uint16_t* out, void* stream);
int bl_gemm_rows_h3(const bl_rows_packed_t* a, const uint32_t* win_bits, int32_t ld_bits, const uint16_t* bp, int64_t b_group_stride,
                    const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K, float out_scale,
                    const float* a_amax_dev, float* c, int32_t ldc, void* stream);
int bl_gemm_wgrad_h3(const bl_rows_packed_t* a, const uint16_t* g_packed, const int32_t* g_idx, const uint32_t* win_bits,
                     int32_t ld_bits, const int32_t* group_ptr, const int32_t* group_w, int32_t G, int32_t M, int32_t N, int32_t K,
                     float out_scale, const float* g_amax_dev, float* gw, int64_t gw_group_stride, int32_t ld_gw, void* stream);

/* Box calibration (measurement support for bench.py; nothing on the training path calls these): boxes
 * of the pool differ by several per cent in the shader clock they sustain at the package power limit, so the bench line
 * carries what THIS chip delivers on two fixed kernels next to the paper peaks.  The caller times the launch with HIP events.
 *   bl_calib_mfma_bf16: `workgroups` x 4 waves, each `iters` x 4 independent chains of v_mfma_f32_32x32x16_bf16 from registers;
 *     *flop = the launch's floating-point operations (dense bf16 MFMA: paper peak 2 500 TF/s).
 *   bl_calib_stream_copy: 16 B / lane grid-stride copy of nbytes (multiple of 16, aligned): 2 x nbytes of HBM traffic. */
int bl_calib_mfma_bf16(int32_t iters, int32_t workgroups, float* sink, double* flop, void* stream);
int bl_calib_stream_copy(const void* src, void* dst, int64_t nbytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Heads.
 * H7  scatter_log_softmax (buglab/models/utils.py:15-28) over CSR segments:
 *     y[i] = x[i] - max_seg - log(sum_seg exp(x - max_seg) + eps)
 * bwd: g_x[i] = g_y[i] - exp(y[i]) * sum_seg g_y */
int bl_segment_log_softmax_fwd(const float* x, const int32_t* seg_ptr, const int32_t* seg_items, int32_t nseg,
                               float eps, float* y, void* stream);
int bl_segment_log_softmax_bwd(const float* g_y, const float* y, const int32_t* seg_ptr, const int32_t* seg_items,
                               int32_t nseg, float* g_x, void* stream);

/* final score layer Linear(H -> 1): y[r] = x[r, :] . w + b   (mlp.py:17, localizationmodule.py:24, 60) */
int bl_rowdot_fwd(const float* x, int32_t ldx, const float* w, const float* b, int32_t R, int32_t H, float* y,
                  void* stream);
/* g_x[r,:] = g_y[r] * w ;  g_w += sum_r g_y[r] x[r,:] ;  g_b += sum_r g_y[r]   (atomics) */
int bl_rowdot_bwd(const float* g_y, const float* x, int32_t ldx, const float* w, int32_t R, int32_t H, float* g_x,
                  int32_t ld_gx, float* g_w, float* g_b, void* stream);

/* out[idx[r], 0:width] += src[r, col_off : col_off + width]  (fp32 atomics).  Backward of every
 * `reprs[node_idx]` gather in buglab/models/gnn.py:170-172, 261-289 and of the rewrite-embedding
 * lookup in fixermodules.py:36. */
int bl_scatter_add_rows(const float* src, int32_t ld_src, int32_t col_off, int32_t width, const int32_t* idx,
                        int32_t R, float* out, int32_t ld_out, void* stream);
/* out[r, 0:width] = x[idx[r], 0:width]: ONE gather of every node row the heads reference
 * (buglab/models/gnn.py:170-172, 261-289 gather `reprs[node_idx]` once per scorer); the scorers then work on
 * the compact [R, H] copy, so backward has one [N, H] scatter instead of one per gather. */
int bl_gather_rows(const float* x, int32_t ld_x, const int32_t* idx, int32_t R, int32_t width, float* out,
                   int32_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole scoring heads per call (the kernels are the ones above; these entry points sequence them).
 * H3/H4/H5  score[r] = w2 . relu(concat_j(x_j[idx_j[r]]) . W1 + b1) + b2 -- the MLP(k H -> H -> 1) of
 * buglab/models/layers/mlp.py:6-20 behind TextRepairModule / SingleCandidateNodeSelectorModule /
 * CandidatePairSelectorModule (fixermodules.py:36-39, 71-73, 116-124).  `hidden` [R, H] is kept for backward.
 * bwd ACCUMULATES into g_W1 [K, H], g_b1, g_w2, g_b2 and into every non-NULL g_x[j] (the gradient matrix of source j,
 * rows addressed through a->idx[j]; several sources may name the same matrix). */
int bl_gather_concat_mlp_score_fwd(const bl_rows_t* a, const float* W1, const float* b1, const float* w2, const float* b2,
                                   int32_t R, int32_t H, float* hidden, float* score, void* stream);
int64_t bl_gather_concat_mlp_score_workspace_bytes(int32_t R, int32_t H, int32_t K);
int bl_gather_concat_mlp_score_bwd(const bl_rows_t* a, const float* W1, const float* w2, const float* hidden,
                                   const float* g_score, int32_t R, int32_t H, void* ws, float* g_W1, float* g_b1,
                                   float* g_w2, float* g_b2, float* const* g_x, const int32_t* ld_gx, void* stream);
/* H1  candidate localization scores (localizationmodule.py:54-60), before the NO_BUG logit and the log-softmax:
 *   s = x[cand] . Ws + bs;  pool[g] = max over graph g's candidates (contiguous rows cand_ptr[g]..cand_ptr[g+1]);
 *   score[c] = w . sigmoid([x[cand[c]] ; pool[cand_graph[c]]] . W1 + b1)
 * bwd ACCUMULATES into g_x (rows addressed through cand) and the parameter gradients. */
int64_t bl_localization_scores_saved_bytes(int32_t C, int32_t B, int32_t H);
int64_t bl_localization_scores_workspace_bytes(int32_t C, int32_t B, int32_t H, int32_t backward);
int bl_localization_scores_fwd(const float* x, int32_t ld_x, const int32_t* cand, const int32_t* cand_graph,
                               const int32_t* cand_ptr, int32_t C, int32_t B, int32_t H, const float* Ws, const float* bs,
                               const float* W1, const float* b1, const float* w, void* saved, void* ws, float* score,
                               void* stream);
int bl_localization_scores_bwd(const float* x, int32_t ld_x, const int32_t* cand, const int32_t* cand_graph,
                               const int32_t* cand_ptr, int32_t C, int32_t B, int32_t H, const float* Ws, const float* W1,
                               const float* w, const void* saved, void* ws, const float* g_score, float* g_x,
                               int32_t ld_gx, float* g_Ws, float* g_bs, float* g_W1, float* g_b1, float* g_w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H2 + H6 + H7 + H8 on the training path: everything between the scorers' logits and the scalar loss in one kernel per
 * direction.  Replaces LocalizationModule.forward's NO_BUG logit / log-softmax / torch.where pick / clamp at log 0.995 /
 * abstain term / (weighted) mean and accuracy counters (buglab/models/layers/localizationmodule.py:63-124), the joint
 * log-softmax of the three repair scorers' logits over the location groups and the arg-max flags
 * (buglab/models/gnn.py:295-311, utils.py:15-28), the fixers' -logprob[target] and counters (fixermodules.py:41-53, 86-98,
 * 134-147) and the loss assembly loc + w_buggy * (text + var + swap) / B (gnn.py:221-251).
 * Items of the localization log-softmax are the C candidate rows followed by one NO_BUG slot per graph (value 1.0). */
typedef struct {
  int32_t B, C, Rt, Rv, Rs, G;                 /* graphs, candidate rows, text / var / swap logits, repair location groups */
  const float* loc_scores;                     /* [C] candidate scores (bl_localization_scores_fwd) */
  const float* repair_logits;                  /* [Rt + Rv + Rs]: text | var | swap */
  const int32_t *loc_group_ptr, *loc_group_items;        /* CSR graph -> its items among 0 .. C + B - 1 */
  const int32_t* candidate_ptr;                /* [B + 1]: the candidate rows of graph b are candidate_ptr[b] .. candidate_ptr[b+1] */
  const uint8_t* has_bug;                      /* [B] */
  const int32_t* correct_candidate_idxs;       /* [B] row of the buggy location (read where has_bug) */
  const int32_t *repair_group_ptr, *repair_group_items;  /* CSR location group -> its logits */
  const int32_t* logit_group[3];               /* location group of every text / var / swap logit */
  const int32_t* target[3];                    /* indices (into their slice) of the correct text / var / swap rewrites */
  int32_t ntarget[3];
  float w_buggy, abstain_weight;
} bl_bug_loss_t;
/* stats[16]: B, graphs localized correctly, NO_BUG graphs, NO_BUG graphs predicted so, -sum of the location logprobs, then
 * (arg-max hits, count) for text / var / swap rewrites, loss, repair loss (times w_buggy), buggy graphs, 1, 0. */
int bl_bug_loss_fwd(const bl_bug_loss_t* d, float* loc_logprobs, float* repair_logprobs, float* group_max, float* loss,
                    float* stats, void* stream);
/* Both calls walk the values through the two CSRs: loc_group_items names every item 0 .. C + B - 1 exactly once and
 * repair_group_items every logit 0 .. Rt + Rv + Rs - 1 exactly once (the collator's CSR of cat(logit_group): every logit has
 * a location group).  An item no group names would get no log-probability and no gradient.  An empty location group is fine:
 * its group_max is -inf.  For the same inputs the outputs of both calls are the same bits on every run.
 * g_loss: device scalar; scratch: C + B + Rt + Rv + Rs floats; under the condition above bwd writes every entry of
 * g_loc_scores [C] and g_repair_logits [Rt + Rv + Rs]: the caller need not clear them */
int bl_bug_loss_bwd(const bl_bug_loss_t* d, const float* loc_logprobs, const float* repair_logprobs, const float* g_loss,
                    float* scratch, float* g_loc_scores, float* g_repair_logits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GREAT var-misuse head (buglab/models/greatreimplementation.py): LayerNorm -> Linear(D, 2) -> masked logits (:202-214),
 * localization cross-entropy, repair logsumexp over the targets of the candidate log-softmax, the loss loc + repair and the
 * metric counters (:118-174, :103-116), in csrc/bl_varmisuse_head.hip.  Position i of sample b is unmasked iff
 * i < lens_att[b]; the caller passes lens_att = min(length + 1, L) (the reference's mask is `arange(L) > length`, :198).
 * A sample is buggy iff error_location != 0 (:209).  Every reduction runs in a fixed order: results are bit-identical
 * from run to run. */
#define BL_VARMISUSE_STATS 8
typedef struct {
  int32_t B, L, D;                             /* samples, padded length, width (multiple of 4, <= 1024) */
  float ln_eps;
  const float* x;                              /* [B * L, D] last layer's output */
  const float *ln_g, *ln_b;                    /* [D] */
  const float* W;                              /* [D, 2] (stored [in, out]) */
  const float* bias;                           /* [2] */
  const int32_t* lens_att;                     /* [B] unmasked positions per sample */
  const int32_t* error_location;               /* [B] */
  const uint8_t *candidate_mask, *target_mask; /* [B * L] */
} bl_varmisuse_head_t;
/* workspace bytes of both directions (-1 for an unsupported shape) */
int64_t bl_varmisuse_head_workspace_bytes(int32_t B, int32_t L, int32_t D);
/* greatreimplementation.py:118-214.  logits [B * L, 2] (-inf where masked; column 1 also at non-candidates), mean / rstd [B * L],
 * lse [B, 3] (localization, candidates, candidates that are targets), loss [2] = (loss, number of buggy samples), both on the device.
 * stats [BL_VARMISUSE_STATS] (double) is ADDED to: samples, localization hits, buggy localization hits, buggy samples, repair
 * hits, localization loss sum, repair loss sum, steps (the counters of :93-101). */
int bl_varmisuse_head_fwd(const bl_varmisuse_head_t* d, float* logits, float* mean, float* rstd, float* lse, void* workspace,
                          float* loss, double* stats, void* stream);
/* greatreimplementation.py:143, :161-174 differentiated.  g_loss: device scalar.  Writes every row of g_x [B * L, D] (zeros at
 * masked rows) and g_W [D, 2], g_bias [2], g_ln_g [D], g_ln_b [D]. */
int bl_varmisuse_head_bwd(const bl_varmisuse_head_t* d, const float* logits, const float* mean, const float* rstd, const float* lse,
                          const float* loss, const float* g_loss, void* workspace, float* g_x, float* g_W, float* g_bias,
                          float* g_ln_g, float* g_ln_b, void* stream);
/* The head forward-only, every sample judged on the device: the inference counterpart of greatreimplementation.py:176-214 (the
 * reference has no predict), in csrc/bl_varmisuse_predict.hip.  Same descriptor; error_location and target_mask are always given
 * (zeros for unlabelled data).  Reads or writes no mean / rstd, workspace, loss or stats; no synchronisation.
 * logits [B * L, 2]: the masked logits of bl_varmisuse_head_fwd for the same inputs, bit for bit.  Sample b's record goes to
 * sample offset + b of buffers the caller keeps for the whole run (capacity samples; offset + B <= capacity), with
 * la = lens_att[b] clamped to [0, L], "candidates" = positions i < la with candidate_mask set, and log-probability =
 * double(logit) - lse:
 *   out_d [7, capacity] (double)  0 localization log-sum-exp over i < la | 1 pointer log-sum-exp over the candidates (-inf without
 *       one) | 2 log-probability of the predicted location | 3 of position 0 ("no bug") | 4 of error_location[b] (-inf outside
 *       [0, la)) | 5 pointer log-probability of the predicted repair (NaN without a candidate) | 6 log-sum-exp of the pointer
 *       log-probabilities over candidates that are targets, the repair log-probability of :161 (-inf without one);
 *   out_i [4, capacity] (int32)   0 predicted location | 1 predicted repair position (-1 without a candidate) | 2 predicted
 *       location == error_location[b] | 3 target_mask at the predicted repair (0 without one).
 * Predictions are first maxima of the fp32 logits (lower index on a tie, as torch.argmax; a NaN never wins).  Each log-sum-exp is
 * max + log(sum exp(double(v) - double(max))) in fp64, summed in a fixed order: results are bit-identical from run to run.
 * BL_EINVAL: null pointers, negative sizes, offset + B > capacity, D not a multiple of 4 or above 1024. */
int bl_varmisuse_predict(const bl_varmisuse_head_t* d, float* logits, double* out_d, int32_t* out_i, int64_t offset, int64_t capacity,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble combine (buglab/models/ensemble/wrapper.py:33-89: `EnsembleWrapper.predict`'s avg / consensus and
 * `_avg_ensembling`), in csrc/bl_ensemble.hip.  src: the M members' flat fp32 outputs [loc | text | var | swap], concatenated
 * (n_src floats).  loc_idx [M, total_loc] / rw_idx [M, total_rw]: per member, the index into src of every entry of the canonical
 * layout -- sample b owns entries loc_off[b] .. loc_off[b + 1] (np.unique(reference_nodes) ascending, then NO_BUG) and
 * rw_off[b] .. rw_off[b + 1] (by original candidate-rewrite index); -1 on all of a sample's entries = the member has no
 * prediction for it.  Per sample, with the M' present members in member order:
 *   BL_ENSEMBLE_AVG        r = a_0 + w, r = logaddexp(r, a_m + w), w = -log(M') (numpy's logaddexp);
 *   BL_ENSEMBLE_CONSENSUS  the avg result if every present member's first-maximum location (canonical order; Python's max
 *                          semantics for NaN) is the same entry, else every location -inf, NO_BUG 0 and the first present
 *                          member's rewrite values unchanged.
 * A sample no member predicts gets NaN.  out_loc [total_loc] and out_rw [total_rw] are DOUBLE: an explicit exception to the
 * float32 convention above, because the reference combines Python floats (doubles) made from the members' fp32 outputs, and an
 * ensemble of one member must then equal that member's own prediction bit for bit (v + -log(1) = v).  One launch, one
 * workgroup per sample, no atomics: bit-identical from run to run.  BL_ERANGE: M > BL_ENSEMBLE_MAX_MEMBERS, or n_src,
 * M * total_loc or M * total_rw beyond int32. */
#define BL_ENSEMBLE_AVG 0
#define BL_ENSEMBLE_CONSENSUS 1
#define BL_ENSEMBLE_MAX_MEMBERS 16
int bl_ensemble_combine(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                        const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, int32_t M, int32_t B, int32_t kind,
                        double* out_loc, double* out_rw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fitted ensembles (buglab/models/ensemble/fit.py, the `weighted` kind), in csrc/bl_ensemble_fit.hip.  BEYOND THE REFERENCE: it
 * has no counterpart -- its ensembles weigh every present member 1 / M' (buglab/models/ensemble/wrapper.py:33-89, whose
 * canonical per-sample layout is the one used here: np.unique(reference_nodes) ascending then NO_BUG, rewrites by original
 * index).  One weight per member for each head and one inverse temperature per member for the location distribution; per
 * sample, with P the present members and l_m member m's fp32 log-probabilities:
 *   locations  z_m = beta_m l_m;  s_m = z_m - LSE z_m (beta_m == 1 exactly: s_m = l_m, the member's values as they are);
 *              a_m = theta_m - LSE_{k in P} theta_k;  out_i = LSE_{m in P} (a_m + s_m[i]);
 *   rewrites   b_m = phi_m - LSE_{k in P} phi_k;      out_r = LSE_{m in P} (b_m + l_m[r]).
 * fp64 throughout, compiled without fused multiply-adds; buglab/models/ensemble/_weights.py is the same arithmetic in NumPy.  In
 * the statistics every LSE subtracts its first maximum and takes log1p of the sum without it, and entries that are not above
 * -inf are skipped (they enter no maximum and no sum).  theta, beta, phi: M doubles each ON THE HOST, read before the launch.
 *
 * bl_ens_loc_stats: a POOL of S location segments; member m's values of segment s are vals[m * total + seg_off[s] .. seg_off[s + 1]]
 *   (offsets clamped to [0, total]), present[m * S + s] != 0 where member m predicts the sample, the target at place tgt[s].
 *   With F = -sum_s out_s[tgt[s]], r_m = exp(a_m + s_m[tgt] + F_s) and pi = softmax of theta over P:
 *   out[0] = F, out[1 + m] = dF/dtheta_m = -sum_s (r_m - pi_m), out[1 + M + m] = dF/dbeta_m = -sum_s r_m (l_m[tgt] - E_m[l]),
 *   E_m[l] = sum_i exp(s_m[i]) l_m[i].  A segment without a present member contributes 0; one where a present member has
 *   nothing above -inf, the target lies outside, or no present member gives the target a probability contributes NaN.
 *   One wave per segment (any length); the segments' terms go to partials ([1 + 2M, S] doubles, the caller's) and a second
 *   kernel sums each column in an order fixed by S alone: no atomics, bit-identical from launch to launch.
 * bl_ens_rw_stats: the same mixture over S buggy samples' truth entries vals[m * S + s]:  out[0] = F_rw,
 *   out[1 + m] = dF_rw/dphi_m; partials [1 + M, S].
 * bl_ensemble_combine_weighted: bl_ensemble_combine's arguments without the kind; out_loc / out_rw as there (DOUBLE), the present
 *   members folded in member order with numpy's logaddexp; an entry without a probability keeps its value under any beta.  A
 *   sample no member predicts gets NaN.  At theta = phi = 0, beta = 1 this is BL_ENSEMBLE_AVG up to the rounding of log(M').
 * S == 0 / B == 0: nothing is launched and nothing written.  No synchronisation.
 * BL_EINVAL: null pointers, M < 1, negative sizes, a theta / phi that is not finite or outside [-BL_ENS_WEIGHT_BOX,
 * BL_ENS_WEIGHT_BOX], a beta outside [BL_ENS_BETA_MIN, BL_ENS_BETA_MAX].  BL_ERANGE: M > BL_ENSEMBLE_MAX_MEMBERS, an index space
 * beyond int32. */
#define BL_ENS_WEIGHT_BOX 20.0
#define BL_ENS_BETA_MIN 0.015625
#define BL_ENS_BETA_MAX 64.0
int bl_ens_loc_stats(const float* vals, int64_t total, const int32_t* present, const int32_t* seg_off, const int32_t* tgt, int32_t M,
                     int32_t S, const double* theta, const double* beta, double* partials, double* out, void* stream);
int bl_ens_rw_stats(const float* vals, const int32_t* present, int32_t M, int32_t S, const double* phi, double* partials, double* out,
                    void* stream);
int bl_ensemble_combine_weighted(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                                 const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, int32_t M, int32_t B,
                                 const double* theta, const double* beta, const double* phi, double* out_loc, double* out_rw,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-supervision services (buglab/controllers/bugselectorserver.py:22-28, 120-150 and
 * buglab/controllers/detectordatascoringworker.py:118-130), in csrc/bl_selfsup.hip.  Both read a model's flat fp32 output
 * src = [loc | text | var | swap] (n_src floats) through int32 indices derived from `prediction_layout`, and work in DOUBLE
 * from the fp32 inputs -- the same exception to the fp32 convention as bl_ensemble_combine, for the same reason: the
 * reference does this arithmetic on Python floats made from fp32 values.  One launch each per minibatch, no atomics,
 * bit-identical from run to run.  An index outside [0, n_src) reads as NaN.
 *
 * bl_score_targets: out[b] = src[tgt_loc[b]] + (tgt_rw[b] >= 0 ? src[tgt_rw[b]] : 0), b < B.  tgt_loc: the location entry of
 * the ground node (or NO_BUG's for a sample without a bug); tgt_rw: the target rewrite's entry, -1 for a sample without a bug.
 *
 * bl_selector_sample: sample b has n_b = rw_off[b + 1] - rw_off[b] candidate rewrites (by original rewrite index; total_rw in
 * all) and n_b + 1 ENTRIES, NO_BUG last, at e_b = rw_off[b] + b .. e_b + n_b of u, out_logprob and out_p (total_rw + B each).
 *   out_logprob  g_i = src[rw_idx[i]] + src[rw_loc_idx[i]] (rw_loc_idx: the location entry of the rewrite's reference node);
 *                g_{n_b} = src[nobug_idx[b]];
 *   out_p        1 / (n_b + 1) if u_eps[b] < epsilon, else exp(g_i / T) / sum_j exp(g_j / T) computed literally (no max
 *                subtraction: where the reference overflows to inf / nan, so does this);
 *   out_entropy  [B] -sum_i p_i log p_i (0 * log 0 = nan, as NumPy);
 *   out_selected [B, K] int32: k_b = min(K, #{i : p_i > 0}) entries drawn without replacement by Gumbel top-k,
 *                key_i = log p_i - log(-log u_i), u in (0, 1) from the caller; the k_b largest keys in descending order, ties to
 *                the lower index; -1 padded.  Entry index n_b means NO_BUG.
 * BL_EINVAL: K < 1, temperature 0 or NaN, null pointers, negative sizes.  BL_ERANGE: K > BL_SELECTOR_MAX_K, or n_src or
 * total_rw + B beyond int32. */
#define BL_SELECTOR_MAX_K 32
int bl_score_targets(const float* src, int64_t n_src, const int32_t* tgt_loc, const int32_t* tgt_rw, int32_t B, double* out, void* stream);
int bl_selector_sample(const float* src, int64_t n_src, const int32_t* rw_idx, const int32_t* rw_loc_idx, const int32_t* rw_off,
                       int64_t total_rw, const int32_t* nobug_idx, int32_t B, const double* u_eps, const double* u, double temperature,
                       double epsilon, int32_t K, double* out_logprob, double* out_p, double* out_entropy, int32_t* out_selected,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bug reports (buglab/models/visualize.py:75-170: what decides whether and where a sample appears), in csrc/bl_report.hip.
 * Same conventions as the self-supervision services: src = a model's flat fp32 output (n_src floats), int32 indices, DOUBLE
 * results, no atomics, bit-identical from run to run, an index outside [0, n_src) reads as NaN.  "First maximum" is Python's
 * max(): the first value stays unless a later one is greater (a NaN in front wins, a NaN elsewhere never does).
 *
 * bl_report_summarize, one launch per predict minibatch of B samples.  Sample b owns
 *   loc_idx[loc_off[b] : loc_off[b + 1]]   its location entries in the key order of the dict `predict` yields, NO_BUG last;
 *   rw_idx [rw_off[b]  : rw_off[b + 1]]    its rewrites by original index (as PredictionLayout), rw_eq_target alongside: 1 where
 *                                          the rewrite's value equals the target rewrite's value;
 *   groups grp_off[b] : grp_off[b + 1]     its range groups (rewrites with equal candidate_rewrite_ranges), by first occurrence.
 * Group g owns grp_rw[grp_rw_off[g] : grp_rw_off[g + 1]]: its rewrites as positions in rw_idx, ascending (grp_rw_off has
 * total_grp + 1 entries and covers [0, total_rw]); grp_loc[g]: the POSITION among the sample's location entries of the node the
 * group's last rewrite refers to; grp_shown[g]: 1 if the range survives text_to_range_segments.  tgt_grp[b]: the target
 * rewrite's group within the sample (-1: NO_BUG); ground_loc[b]: the position of the ground node's location entry (NO_BUG's
 * without a target); nobug_idx[b]: NO_BUG's entry in src.
 *   out_best_rw    [total_grp] the group's first-maximum rewrite, as an index within the sample's rewrites;
 *   out_best_range [total_grp] src[location of grp_loc[g]] + that rewrite's log-probability (one fp64 addition);
 *   out_sample_i   [3, B]      pred_loc (position of the first-maximum location entry) | pred_is_nobug | is_wrong: ground_loc !=
 *                              pred_loc, replaced, when the target's group is shown, by (grp_loc != pred_loc, or
 *                              rw_eq_target[best rewrite of the group] == 0);
 *   out_sample_d   [2, B]      prediction_logprob = the greatest non-NaN out_best_range over the shown groups, -inf if none |
 *                              no_bug_logprob = src[nobug_idx[b]].
 *
 * bl_report_order, once per report: out[0 : *out_count] = the indices i < n with keep[i] != 0, ordered as Python's stable
 * sorted(key=-keys[i]) orders them when by_confidence != 0 (greater key first, input order on ties, -inf last, NaN after that)
 * and in input order otherwise; cut to the first k when k > 0.  out has room for n entries; those beyond *out_count are not
 * written.  BL_ERANGE: n > BL_REPORT_MAX_SAMPLES (the ranks are counted pair by pair). */
#define BL_REPORT_MAX_SAMPLES (1 << 20)
int bl_report_summarize(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc,
                        const int32_t* rw_idx, const int32_t* rw_off, int64_t total_rw, const int32_t* rw_eq_target,
                        const int32_t* grp_rw, const int32_t* grp_rw_off, const int32_t* grp_loc, const int32_t* grp_shown,
                        const int32_t* grp_off, int64_t total_grp, const int32_t* tgt_grp, const int32_t* ground_loc,
                        const int32_t* nobug_idx, int32_t B, int32_t* out_best_rw, double* out_best_range, int32_t* out_sample_i,
                        double* out_sample_d, void* stream);
int bl_report_order(const double* keys, const int32_t* keep, int64_t n, int64_t k, int32_t by_confidence, int32_t* out,
                    int32_t* out_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation (buglab/models/evaluate.py:60-140: `judge_sample`, what one sample contributes to the metrics and the threshold
 * curves), in csrc/bl_evaluate.hip.  Same conventions as the bug reports: src = a model's flat fp32 output (n_src floats), int32
 * indices, DOUBLE confidence, no atomics, bit-identical from run to run, an index outside [0, n_src) reads as NaN, "first
 * maximum" is Python's max().
 *
 * bl_eval_judge, one launch per predict minibatch of B samples, no synchronisation.  Sample b owns
 *   loc_idx[loc_off[b] : loc_off[b + 1]]   its location entries in the key order of the dict `predict` yields, NO_BUG last, and
 *                                          key_node alongside: the dense id of the entry's node within the sample (its index in
 *                                          np.unique(reference_nodes)), -1 for NO_BUG;
 *   rw_idx [rw_off[b]  : rw_off[b + 1]]    its rewrites by original index (as PredictionLayout), rw_node alongside: the dense id
 *                                          of the rewrite's reference node;
 *   tgt_rw[b]                              target_fix_action_idx (an index within the sample's rewrites), -1 without a bug.
 * Everything is decided by node identity, as the host compares node ids: two entries that share a flat index stay two keys, and
 * a target whose node has no entry can never be "location correct".
 *   predicted entry  the first maximum over the location entries; with assume_buggy != 0 over all but the last (NO_BUG);
 *   best rewrite at a node (the predicted one, the target's one): the greatest log-probability STRICTLY above -inf among the
 *                    rewrites at that node, lowest index among equals, NaN never; "none" if there is no such rewrite or the
 *                    node is NO_BUG.
 * Results go to sample offset + b of buffers the caller keeps for the whole run (capacity samples; offset + B <= capacity):
 *   out_conf    [capacity]     src[predicted entry], exact; with assume_buggy minus the log-sum-exp of the entries the maximum
 *                              was taken over, in fp64: shifted by their maximum, exp summed over a fixed tree;
 *   out_verdict [4, capacity]  warned (the predicted entry is not NO_BUG) | location_correct (predicted node == the target's
 *                              node; NO_BUG predicted without a bug) | repair_given_location (best rewrite at the target's node ==
 *                              tgt_rw; -1 without a bug) | repaired (location_correct and best rewrite at the predicted node ==
 *                              tgt_rw, "none" == the -1 of a sample without a bug).
 * A sample with no entry to choose from gets confidence NaN and "NO_BUG predicted"; the host refuses such a sample first.
 * BL_EINVAL: null pointers, negative sizes, offset + B > capacity.  BL_ERANGE: n_src, total_loc or total_rw beyond int32. */
int bl_eval_judge(const float* src, int64_t n_src, const int32_t* loc_idx, const int32_t* loc_off, const int32_t* key_node,
                  int64_t total_loc, const int32_t* rw_idx, const int32_t* rw_off, const int32_t* rw_node, int64_t total_rw,
                  const int32_t* tgt_rw, int32_t B, int32_t assume_buggy, double* out_conf, int32_t* out_verdict, int64_t offset,
                  int64_t capacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ranked suggestions (buglab/models/suggest.py, buglab/models/evaluate.py --top-k), in csrc/bl_suggest.hip.  BEYOND THE
 * REFERENCE: its evaluate.py:60-140 and visualize.py:75-144 reduce a sample to one answer (the first-maximum location, then the
 * best rewrite there); nothing there ranks a sample's fixes.  Same conventions as the evaluation: src = a model's flat fp32
 * output (n_src floats), int32 indices, DOUBLE log-probabilities, no atomics, bit-identical from run to run, an index outside
 * [0, n_src) reads as NaN.
 *
 * bl_rank_suggestions, one launch per predict minibatch of B samples, no synchronisation.  Sample b has
 * n_b = rw_off[b + 1] - rw_off[b] candidate rewrites and n_b + 1 ENTRIES: entry i < n_b is rewrite i (original index), entry n_b
 * is NO_BUG.  It owns
 *   rw_idx [rw_off[b] : rw_off[b + 1]]     its rewrites by original index (as PredictionLayout); alongside rw_loc_idx: the flat
 *                                          index of the location entry of the rewrite's reference node, -1 where that node has no
 *                                          location key; and rw_node: the dense id of that node (as bl_eval_judge);
 *   nobug_idx[b]                           NO_BUG's location entry in src;
 *   tgt_rw[b]                              target_fix_action_idx (an index within the sample's rewrites), negative without a bug;
 *   loc_idx[loc_off[b] : loc_off[b + 1]]   its location entries in the key order of the dict `predict` yields, NO_BUG last, and
 *                                          key_node alongside (as bl_eval_judge: -1 for NO_BUG).
 * The VALUE of entry i < n_b is (double)src[rw_idx[i]] + (double)src[rw_loc_idx[i]], one fp64 addition (the g_i of
 * bl_selector_sample; NaN where rw_loc_idx is -1); of NO_BUG, (double)src[nobug_idx[b]].  With skip_nobug != 0 the NO_BUG entry
 * does not take part; values are not renormalised (a common shift changes no rank).  An entry whose value is NaN or not strictly
 * above -inf is NOT RANKABLE: it precedes nothing and is never listed.  TOTAL ORDER: a precedes b iff v_a > v_b, or v_a == v_b
 * and a < b.  The RANK of an entry is the number of rankable entries that precede it.
 * Results go to sample offset + b of buffers the caller keeps for the whole run (capacity samples; offset + B <= capacity):
 *   out_entry   [capacity, K] int32   the first min(K, #rankable) entries in that order, then -1;
 *   out_logprob [capacity, K] double  their values, then -inf;
 *   out_rank    [2, capacity] int32   row 0, the joint rank of the TRUTH entry: tgt_rw[b], or NO_BUG's entry without a bug;
 *                                     -1 if that entry is not rankable, if tgt_rw[b] >= n_b, or if it is NO_BUG under skip_nobug.
 *                                     Row 1, the location rank: the same order and rule over the values src[loc_idx[.]] of the
 *                                     sample's location entries (all but the last under skip_nobug); the truth is the first entry
 *                                     whose key_node equals rw_node[tgt_rw[b]], or the last entry (NO_BUG) without a bug; -1 if
 *                                     there is no such entry or it is not rankable.
 * No exp or log is taken: one addition, compares and integer counts, so buglab/models/_suggest.py::rank_host gives the same bits.
 * Joint rank 0 is NOT bl_eval_judge's `repaired`: that takes the best rewrite at the first-maximum location, this ranks the sums.
 * A segment of at most 4096 entries is staged in LDS; a longer one is recomputed from src in every round (no length is refused).
 * BL_EINVAL: K < 1, null pointers, negative sizes, offset + B > capacity.  BL_ERANGE: K > BL_SUGGEST_MAX_K, or n_src, total_loc
 * or total_rw + 1 beyond int32. */
#define BL_SUGGEST_MAX_K 32
int bl_rank_suggestions(const float* src, int64_t n_src, const int32_t* rw_idx, const int32_t* rw_loc_idx, const int32_t* rw_off,
                        int64_t total_rw, const int32_t* nobug_idx, const int32_t* tgt_rw, const int32_t* loc_idx,
                        const int32_t* loc_off, const int32_t* key_node, int64_t total_loc, const int32_t* rw_node, int32_t B, int32_t K,
                        int32_t skip_nobug, int32_t* out_entry, double* out_logprob, int32_t* out_rank, int64_t offset,
                        int64_t capacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Explanations: node attributions of a predicted fix (buglab/models/explain.py), in csrc/bl_explain.hip.  BEYOND THE REFERENCE:
 * it has no counterpart -- its visualize.py shows what was flagged, nothing says why.  The backward pass (existing kernels)
 * gives G [N, D], the gradient of the explained log-probability with respect to the node embedder's output x [N, D]; these two
 * reduce it.  fp64, fixed trees, no atomics, compiled without fused multiply-adds, bit-identical from run to run and equal bit
 * for bit to buglab/models/_explain.py::node_scores_host / topk_host.  No synchronisation, no allocation.
 *
 * bl_attr_node_scores: score[n] = t or score[n] + t (accumulate != 0: the steps of an integrated-gradients path), with
 *   t = w * dot_n (one rounded product, then one rounded addition) and dot_n = sum_d x[n, d] * g[n, d].  x, g: fp32, row strides
 *   ldx, ldg in ELEMENTS (>= D); score: double [N].  One wave per node.  COLUMN OWNERSHIP: columns go in quads, quad q = columns
 *   4q .. 4q + 3 (the last one may be partial); lane l owns the quads with q % 64 == l and adds the products of its columns, each
 *   exact in fp64 (24 + 24 significand bits), to its own fp64 sum (initially +0.0) in ascending column order.  The 64 lane sums
 *   are then added by the xor butterfly, strides 32 .. 1, and lane 0's value is dot_n.  The ownership is the same for every D,
 *   stride and alignment: with x, g 16-byte aligned and both strides multiples of 4 a quad is one 16-byte load per operand,
 *   otherwise the same columns are loaded one by one.  Any D >= 1; N == 0 is a no-op.  Bandwidth bound: 2 N D 4 bytes.
 *   BL_EINVAL: D < 1, N < 0, a stride below D, null pointers.  BL_ERANGE: N beyond int32.
 *
 * bl_attr_topk: one workgroup per graph b of B over the nodes [node_off[b], node_off[b + 1]) of score (int32 offsets, clamped
 *   to [0, N]); results go to row offset + b of buffers the caller keeps for the whole run (capacity graphs):
 *   out_sums  [2, capacity] double   sum a | sum |a| over the graph's nodes: thread t of 256 adds nodes t, t + 256, .. in that
 *                                    order, then the xor butterfly in each wave and the four waves' sums in wave order.  A NaN
 *                                    score makes both NaN.
 *   out_node  [capacity, k] int32    the first min(k, #non-NaN) nodes, as indices WITHIN the graph, in the order "greater key
 *                                    first, the lower index among equals", key = |a| (by_abs != 0) or a; then -1.  k rounds, each
 *                                    the first maximum among the nodes strictly after the previous pick in that order (nothing is
 *                                    marked).  A node whose score is NaN is never listed.
 *   out_score [capacity, k] double   a of the listed nodes (signed, whatever the key); then 0.0.
 *   Nothing outside rows offset .. offset + B - 1 is written.  BL_EINVAL: k < 1, negative sizes, null pointers, offset + B >
 *   capacity.  BL_ERANGE: k > BL_EXPLAIN_MAX_K, N beyond int32. */
#define BL_EXPLAIN_MAX_K 32
int bl_attr_node_scores(const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t N, int32_t D, double w, int32_t accumulate,
                        double* score, void* stream);
int bl_attr_topk(const double* score, const int32_t* node_off, int32_t B, int64_t N, int32_t k, int32_t by_abs, int32_t* out_node,
                 double* out_score, double* out_sums, int64_t offset, int64_t capacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Paired bootstrap of the evaluation counts (buglab/models/compare.py), in csrc/bl_bootstrap.hip.  BEYOND THE REFERENCE: it
 * has no counterpart -- its evaluate.py prints point estimates only.  What is resampled are the counts of
 * buglab/models/evaluate.py:139-173 (the numerators and denominators of every metric and of the per-scout tables): each
 * replicate draws n samples with replacement and counts them again, for M models over the SAME draws.
 *
 * The draw contract (buglab/models/_compare.py::draw_indices is the same arithmetic in NumPy).  Replicate r >= 0 draws n
 * sample positions; for j in [0, n), all arithmetic uint64, wrapping:
 *   mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   base   = mix(seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15)
 *   h      = mix(r * n + j + base) >> 32
 *   index  = (h * n) >> 32
 * (splitmix64 as a counter generator).  A draw depends on (seed, r, j, n) alone: not on the grid, not on how a run is cut
 * into calls.  The multiply-shift maps h to an index with a relative bias below n / 2^32.  Seed 0, n = 10: replicate 0 draws
 * 2 9 6 4 2 1 5 5 5 3, replicate 1 draws 3 6 3 2 2 0 3 0 2 2.
 *
 * packed [n]: one uint32 per sample, shared by the M models.  Bits 0-7: the sample's scout id (0 = "NoBug": the sample has no
 * bug; 1 .. K - 1: the bug kinds, as ColumnarEvaluationReport.scout_names numbers them).  Model m owns bits 8 + 4m .. 11 + 4m:
 * warned | location_correct << 1 | (repair_given_location == 1) << 2 | repaired << 3.
 *
 * out [R, C] int32, C = K + M (4 + 2K); row i holds replicate r0 + i:
 *   columns 0 .. K - 1               scout_total[k]: draws whose sample has scout k;
 *   model m, from column K + m (4 + 2K):  repaired | repaired_and_buggy | warned_and_buggy | silent_and_not_buggy |
 *                                    loc_ok[k] (K entries: location_correct and scout k) |
 *                                    rep_ok[k] (K entries: bit 2 set and scout k; the entry for k = 0 is always 0).
 * "buggy" is scout != 0.  A scout id >= K (the caller's mistake) counts as buggy and enters no [k] column.  The rest derives:
 * n_buggy = n - scout_total[0], located = sum loc_ok, repair_ok = sum rep_ok.  Integer counts: any summation order gives the
 * same bits, so the result equals the twin's exactly and every call gives the same result.
 *
 * One launch, one workgroup per replicate, the words gathered from global memory (L2); integer LDS adds, no float atomics,
 * one plain store per output element; no synchronisation, no allocation.  R == 0 is a no-op.
 * BL_EINVAL: null packed / out, n < 1, R < 0, r0 < 0 (or r0 + R beyond int64), M outside [1, BL_BOOTSTRAP_MAX_MODELS], K outside
 * [1, BL_BOOTSTRAP_MAX_SCOUTS].  BL_ERANGE: n >= 2^31. */
#define BL_BOOTSTRAP_MAX_MODELS 6
#define BL_BOOTSTRAP_MAX_SCOUTS 64
int bl_bootstrap_counts(const uint32_t* packed, int64_t n, int32_t M, int32_t K, uint64_t seed, int64_t r0, int64_t R,
                        int32_t* out /* [R, C] */, void* stream);

/* bl_bootstrap_curve_counts: the same replicates counted per candidate threshold (buglab/models/operatingpoint.py; the NumPy
 * twin is buglab/models/_operatingpoint.py::curve_counts_host).  BEYOND THE REFERENCE, which prints the six threshold curves
 * as point estimates.  The thresholds are fixed once, per model, and every sample carries the index of the first threshold it
 * passes, so a replicate is a histogram over those indices and a prefix sum -- no ranking inside a replicate.
 *
 * packed [n]: the words above, unchanged; has_bug = (word & 0xFF) != 0, and of model m's bits at 8 + 4m: warned = bit 0,
 * loc_ok = bit 1, rep_ok = bit 2.  bins [M, n] int16: bins[m, i] in [0, G] is the number of model m's thresholds that sample i
 * does NOT pass (thresholds descend, so "bin <= g" is "passes threshold g"); G passes none, and so does any value outside
 * [0, G).  The draws are those of the contract above, word for word: for the same (seed, r, n), replicate r of this function
 * and of bl_bootstrap_counts count the same samples.
 *
 * out [R, 1 + M * 5 * G] int32; row i holds replicate r0 + i:
 *   column 0                      num_buggy: draws with has_bug;
 *   then [M][5][G]                for model m, counter c and threshold g the count over the draws with bin <= g (inclusive
 *                                 cumulative over the bins) of, in the order of _curves_of_ranked in buglab/models/evaluate.py:
 *                                   det_true = has_bug & loc_ok | det_false = warned & ~loc_ok |
 *                                   full_true = has_bug & loc_ok & rep_ok | full_false = warned & (~loc_ok | ~rep_ok) |
 *                                   false_alarm = warned & ~has_bug
 * applied to the bits as written (a word may hold combinations no model produces).  Integer counts: any order gives the same
 * bits, so the result equals the twin's exactly and every call gives the same result.
 *
 * One launch, one workgroup per (replicate, model) striding over the replicates; integer LDS adds into one [5][G] table (20 KB
 * at G = BL_CURVE_MAX_BINS), the prefix sum in LDS, one plain store per output element; no synchronisation, no allocation.
 * R == 0 is a no-op.  BL_EINVAL: null packed / bins / out, n < 1, R < 0, r0 < 0 (or r0 + R beyond int64), M outside
 * [1, BL_BOOTSTRAP_MAX_MODELS], G outside [1, BL_CURVE_MAX_BINS].  BL_ERANGE: n >= 2^31. */
#define BL_CURVE_MAX_BINS 1024
int bl_bootstrap_curve_counts(const uint32_t* packed, const int16_t* bins /* [M, n] */, int64_t n, int32_t M, int32_t G,
                              uint64_t seed, int64_t r0, int64_t R, int32_t* out /* [R, 1 + M * 5 * G] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * False-discovery-controlled warnings (buglab/models/fdr.py), in csrc/bl_fdr.hip.  BEYOND THE REFERENCE: it has no counterpart.
 * Conformal p-values against a reference set of clean samples, then the Benjamini-Hochberg (BH) step-up over a scan: if the
 * reference is exchangeable with the clean part of the scan, the expected share of false alarms among the flagged samples is
 * at most q, whatever the share of buggy samples.  buglab/models/_fdr.py is the same arithmetic in NumPy, equal bit for bit on
 * every output.  Definitions:
 *   SCORE of sample b   s = src[nobug_idx[b]]: the fp32 NO_BUG location log-probability of the model's flat output (calibrated
 *                       where the checkpoint carries a calibration).  Lower is more suspicious.  An index outside [0, n_src)
 *                       reads as NaN.
 *   REFERENCE           ref[0 .. n): the scores of n >= 1 clean samples, fp32, sorted ascending, no NaN (the host drops and
 *                       counts them at fit time), n <= BL_FDR_MAX_REFERENCE.
 *   COUNT               c = #{ j : ref[j] <= s }, fp32 compares as IEEE makes them (-0.0 == 0.0); c = n for a NaN s.
 *   P-VALUE             p = (c + 1) / (n + 1), formed on the host; no decision uses the float.
 *   BH over N samples at level q:  R[c] = the number of samples with count <= c;
 *                       c* = max{ c in [0, n] : R[c] > 0 and (double)((int64)(c + 1) * N) <= q * (double)((int64)(n + 1) * R[c]) },
 *                       an exact integer on the left, ONE rounded fp64 product on the right (both integers are below 2^53);
 *                       c* = -1 if there is no such c.  A sample is FLAGGED iff c <= c*.  (The textbook step-up: the largest k
 *                       with p_(k) <= q k / N.)
 *   Q-VALUE             qv(c) = min over c' >= c with R[c'] > 0 of min(1, (double)((int64)(c' + 1) * N) / (double)((int64)(n + 1) * R[c'])),
 *                       each term ONE correctly rounded fp64 quotient; an fp64 minimum is exact, so any order gives the same bits.
 * Benjamini-Yekutieli (arbitrary dependence) divides q by sum_{i <= N} 1 / i on the host; the kernels know nothing of it.
 *
 * bl_fdr_counts: one launch per predict minibatch of B samples, no synchronisation; one thread per sample, a binary search for
 *   the upper bound in ref.  Writes out_score[offset + b] = s (the NaN's bits as loaded; 0x7FC00000 for an index outside src)
 *   and out_count[offset + b] = c into buffers the caller keeps for the whole run (capacity samples); nothing else is written.
 *   The same entry serves a bulk call over N scores with nobug_idx the identity.
 *   BL_EINVAL: null pointers, negative sizes, n_ref < 1, offset + B > capacity.  BL_ERANGE: n_ref > BL_FDR_MAX_REFERENCE, n_src
 *   beyond int32.
 *
 * bl_fdr_bh: count [N] int32 (a value outside [0, n_ref] is clamped into it) -> out_cutoff int32 [2] = { c*, R[c*] or 0 },
 *   out_flag int32 [N] (1 = flagged), out_q double [N] = qv(count).  workspace: bl_fdr_bh_workspace_bytes(n_ref) bytes, 8-byte
 *   aligned, may hold anything on entry; on return its first n_ref + 1 int32 hold R.  Several launches on `stream`, no
 *   synchronisation, no allocation: the histogram of the counts is zeroed and filled (integer adds, the only atomics: to an LDS
 *   table of the workgroup where n_ref + 1 <= 16000, to global memory beyond; the top bin c = n_ref is counted in registers and
 *   added once per workgroup), an inclusive prefix sum in chunks of 4096 bins gives R, every bin's term and the chunk's greatest
 *   qualifying c are formed in the same pass, a suffix minimum over the terms gives qv, and one pass over the samples writes
 *   out_flag and out_q.  The same bytes on every call.
 *   BL_EINVAL: null pointers, a workspace that is not 8-byte aligned, N < 1, n_ref < 1, q outside (0, 1] (NaN included).
 *   BL_ERANGE: n_ref > BL_FDR_MAX_REFERENCE, N beyond int32.  bl_fdr_bh_workspace_bytes returns 0 for an n_ref out of range. */
#define BL_FDR_MAX_REFERENCE (1 << 20)
int bl_fdr_counts(const float* src, int64_t n_src, const int32_t* nobug_idx, int32_t B, const float* ref, int64_t n_ref,
                  float* out_score, int32_t* out_count, int64_t offset, int64_t capacity, void* stream);
int64_t bl_fdr_bh_workspace_bytes(int64_t n_ref);
int bl_fdr_bh(const int32_t* count, int64_t N, int64_t n_ref, double q, void* workspace, int32_t* out_cutoff, int32_t* out_flag,
              double* out_q, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Similar-bug search (buglab/models/similar.py), in csrc/bl_similar.hip.  BEYOND THE REFERENCE: it has no counterpart.
 *
 * A SITE is one candidate location of one sample; its embedding is the row of the head input h behind that candidate.  An index
 * of such rows is searched in two stages: an exact top-C search on the int8 images with v_mfma_i32_16x16x64_i8, and an fp64
 * re-score of those C.  buglab/models/_similar.py is the same arithmetic in NumPy, equal bit for bit on every output.  The
 * kernels sit on bl_segment_f64.h's contract and are compiled without fused multiply-adds; no exp, no sqrt, no atomics.
 * Dp = D rounded up to a multiple of 64.
 *
 *   centre     c_d = (float)((double)x_d - (double)mean_d)
 *   row        amax = max_d |c_d|; sumsq = sum_d c_d c_d in fp64 with bl_attr_node_scores' column ownership and butterfly.
 *              A row is INVALID if a c_d is not finite or amax == 0: q = 0, sumsq = 0, r = 0; never a candidate, and as a query
 *              it has no neighbours.
 *   quantise   q_d = (int8)rint((double)c_d * (127.0 / (double)amax)), half to even; columns D .. Dp - 1 zero;
 *              r = ((double)amax * (double)amax) / sumsq
 *   key        idot = sum_d qx_d qy_d, exact in int32; key = (double)((int64)idot * |idot|) * r_y: apart from quantisation
 *              error monotone in the cosine
 *   search     per valid query the C valid index rows that come first in "greater key, or the same key at the lower index",
 *              -1 (key 0.0) padded: the exact top C under a total order, whatever the tiles, the slices and the geometry
 *   re-score   dot = sum_d cx_d cy_d in fp64 in the order of sumsq; key2 = (dot * |dot|) / sumsq_y; the k <= C first candidates
 *              by (greater key2, lower index, earlier place in the list), -1 (dot 0.0) padded.  A candidate outside [0, N), with
 *              sumsq_y <= 0 or with a NaN key2 is absent.  The host forms the cosine dot / sqrt(sumsq_x sumsq_y).
 *
 * bl_sim_embed_sites: one launch per predict minibatch of B samples, one wave per sample.  flat [n_flat]: the model's flat
 *   output, whose first n_cand entries are the candidates' location log-probabilities; loc_idx / loc_off: the PredictionLayout's
 *   location entries (a sample's candidates in canonical order, NO_BUG last; offsets clamped into [0, total_loc]); cand_rows
 *   [n_cand]: the row of h behind each candidate; h [n_rows, D], row stride ldh.  mode BL_SIM_SITE_PREDICTED: the site is the
 *   first maximum of the sample's entries (NaN and indices outside flat never enter; skip_nobug leaves NO_BUG out); a NO_BUG
 *   that wins means no site.  BL_SIM_SITE_TRUTH: truth [B] is the site's place within the segment, -1 for none.  Written at
 *   offset + b of the run-long buffers: out_rows [capacity, D] (zeros without a site), out_place (-1 without), out_logprob (the
 *   fp32 entry as it is; 0 without).  Any index out of range means "no site", never an out-of-bounds read.
 *   BL_EINVAL: null pointers, negative sizes, ldh < D, unknown mode, offset + B > capacity.  BL_ERANGE: D > BL_SIM_MAX_D, index
 *   spaces beyond int32.
 * bl_sim_quantize: x [N, D] (row stride ldx, any alignment), mean [D] -> c [N, D] (row stride ldc; c == x with ldc == ldx is
 *   allowed), q int8 [N, Dp] (contiguous, 16-byte aligned), sumsq and r double [N].  One wave per row.
 * bl_sim_search_i8: qx [Q, Dp] / rx [Q] the queries, qy [N, Dp] / ry [N] the index (r <= 0 marks an invalid row) -> out_idx
 *   int32 [Q, C], out_key double [Q, C].  slices in [1, BL_SIM_MAX_SLICES]: the index is cut into that many parts, searched by
 *   separate workgroups and merged; the result does not depend on it.  workspace: bl_sim_search_workspace_bytes(Q, slices)
 *   bytes, 8-byte aligned, contents irrelevant.  BL_EINVAL: Dp not a multiple of 64, C outside [1, BL_SIM_MAX_CANDIDATES], slices
 *   out of range, a workspace too small, images not 16-byte aligned.  BL_ERANGE: Dp > BL_SIM_MAX_D, N beyond int32.
 * bl_sim_rescore: cx [Q, D], cy [N, D] (row strides, any alignment), sumsq_y [N], cand int32 [Q, C] -> out_idx int32 [Q, k],
 *   out_dot double [Q, k].  BL_EINVAL: k outside [1, C], C outside [1, BL_SIM_MAX_CANDIDATES].
 * No call synchronises. */
#define BL_SIM_MAX_D 512
#define BL_SIM_MAX_CANDIDATES 16
#define BL_SIM_MAX_SLICES 64
#define BL_SIM_SITE_PREDICTED 0
#define BL_SIM_SITE_TRUTH 1
int bl_sim_embed_sites(const float* flat, int64_t n_flat, const int32_t* loc_idx, const int32_t* loc_off, int64_t total_loc, int32_t B,
                       const int32_t* cand_rows, int64_t n_cand, const float* h, int64_t ldh, int64_t n_rows, int32_t D,
                       const int32_t* truth, int32_t skip_nobug, int32_t mode, float* out_rows, int32_t* out_place,
                       float* out_logprob, int64_t offset, int64_t capacity, void* stream);
int bl_sim_quantize(const float* x, int64_t ldx, const float* mean, int64_t N, int32_t D, float* c, int64_t ldc, int8_t* q,
                    double* sumsq, double* r, void* stream);
int64_t bl_sim_search_workspace_bytes(int64_t Q, int32_t slices);
int bl_sim_search_i8(const int8_t* qx, const double* rx, int64_t Q, const int8_t* qy, const double* ry, int64_t N, int32_t Dp,
                     int32_t C, int32_t slices, void* workspace, int64_t workspace_bytes, int32_t* out_idx, double* out_key,
                     void* stream);
int bl_sim_rescore(const float* cx, int64_t ldx, int64_t Q, const float* cy, int64_t ldy, const double* sumsq_y, int64_t N, int32_t D,
                   const int32_t* cand, int32_t C, int32_t k, int32_t* out_idx, double* out_dot, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Warning grouping (buglab/models/group.py), in csrc/bl_group.hip.  BEYOND THE REFERENCE: it has no counterpart.  The warnings of
 * a scan are mostly the same few patterns many times; this groups the N site embeddings into the connected components of "cosine
 * of the centred embeddings >= S" (single linkage at S), so that a reviewer looks at a pattern once.  It is the all-pairs join of
 * ONE set of rows with itself, an N x N / 2 integer GEMM whose result is never stored: the epilogue decides, re-scores and links
 * in place.  buglab/models/_group.py is the same arithmetic in NumPy, equal bit for bit on every output.
 *
 * Inputs: bl_sim_quantize's outputs for the N rows (centred with their own column mean, or not centred): c float [N, D], q int8
 * [N, Dp], sumsq and r double [N]; l1_i = sum_d |q_id|, int32 and exact (bl_group_row_l1); S in (0, 1].  The host forms
 * s2 = S * S and K = ((16 * 16129^2) * s2) * (1 - 2^-40) once, in double, and passes both.
 *
 *   edge     for i < j with both rows valid (r > 0): dot = sum_d c_id c_jd in bl_attr_node_scores' column ownership and butterfly
 *            -- exactly the dot of bl_sim_rescore.  (i, j) is an EDGE iff dot > 0.0 and dot * dot >= s2 * (sumsq_i * sumsq_j):
 *            three rounded products and one compare, no sqrt and no division.  Two identical rows have dot == sumsq bit for bit,
 *            so duplicates link at S = 1.
 *   filter   idot = sum_d q_id q_jd, exact in int32; A = 4 idot + 2 (l1_i + l1_j) + D in int64.  (i, j) is a CANDIDATE iff
 *            A > 0 and ((double)A * (double)A) * (r_i * r_j) >= K.  A^2 < 2^53, so the square is exact; then two rounded
 *            products and a compare.  Only candidates are re-scored.  The filter loses no edge: with u = c * 127 / amax and
 *            q = u + e, |e_d| <= 1/2, u_i . u_j <= idot + (l1_i + l1_j) / 2 + D / 4 = A / 4 and |u_i|^2 = 16129 / r_i, so
 *            cos >= S implies A / 4 >= S * 16129 / sqrt(r_i r_j); the factor 1 - 2^-40 absorbs every rounding.
 *   groups   the connected components of the edge graph.  label_i = the smallest row index of i's component; an invalid row is
 *            its own group.  degree_i = the number of edges at i.  counters = { number of candidates, number of edges }.
 *            All of them are functions of the input alone: the same whatever the order in which the pairs are visited.
 *
 * bl_group_row_l1: q [N, Dp] (contiguous, 16-byte aligned) -> l1 int32 [N].  One wave per row.
 * bl_group_link: covers the upper triangle of 16 x 16 tiles with v_mfma_i32_16x16x64_i8.  UPDATES parent int32 [N] (the caller
 *   sets it to the identity first), degree int32 [N] (zeroed first) and counters int64 [2] (zeroed first, 8-byte aligned) with
 *   vector global atomics; c has row stride ldc and any alignment.  A lock-free union-find: parent[x] <= x always, a root is
 *   hooked below a smaller root by compare-and-swap, no thread waits for another.  parent is NOT unique (it depends on the order
 *   of the hooks); the partition it encodes is.  slices in [1, BL_GROUP_MAX_SLICES]: every tile row's range of the triangle is cut
 *   into that many parts for separate workgroups; the result does not depend on it.
 * bl_group_labels: parent [N] -> label int32 [N], each row's root; to be called after bl_group_link on the same stream.  An entry
 *   of parent outside [0, row) ends the walk there, so garbage stays in bounds.
 * A member's cosine to its group's representative: bl_sim_rescore with cand [N, 1] and k = 1.
 * BL_EINVAL: null pointers, negative sizes, Dp not D rounded up to a multiple of 64, ldc < D, s2 outside (0, 1] or K outside
 *   (0, 16 * 16129^2] (NaN included), slices out of range, q not 16-byte aligned, counters not 8-byte aligned.  BL_ERANGE:
 *   D or Dp > BL_SIM_MAX_D, N > BL_GROUP_MAX_N (the work is N^2 / 2 tile products: DESIGN.md has the time at the cap).
 * No call synchronises. */
#define BL_GROUP_MAX_N (1 << 19)
#define BL_GROUP_MAX_SLICES 64
int bl_group_row_l1(const int8_t* q, int64_t N, int32_t Dp, int32_t* l1, void* stream);
int bl_group_link(const int8_t* q, const double* r, const int32_t* l1, const float* c, int64_t ldc, const double* sumsq, int64_t N,
                  int32_t D, int32_t Dp, double s2, double K, int32_t slices, int32_t* parent, int32_t* degree, int64_t* counters,
                  void* stream);
int bl_group_labels(const int32_t* parent, int64_t N, int32_t* label, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Drift detection (buglab/models/drift.py), in csrc/bl_drift.hip.  BEYOND THE REFERENCE: it has no counterpart.  A two-sample
 * permutation test of the kernel maximum mean discrepancy (MMD) between the site embeddings of a reference (a SiteIndex) and
 * those of the data about to be scanned.  buglab/models/_drift.py is the twin: the subsets bit for bit, the sums in fp64.
 *
 *   pooled rows  Z = [X_ref ; X_new], fp32 [N, D], N = n + m, n, m >= 2: the index's centred embeddings, then the scanned
 *                sites' embeddings centred with the index's mean.
 *   bandwidth    s = scale * (1 / N^2) sum_ij |z_i - z_j|^2 = scale * 2 (mean_i |z_i|^2 - |mean_i z_i|^2), in fp64 from column
 *                sums.  NO SPREAD: when the bracket is at most 2^-40 of mean_i |z_i|^2 (all rows equal up to fp64 rounding of
 *                the sums), s = 0; the sums then take every kernel value as 1 and the report says statistic 0, p-value 1.
 *   kernel       k(x, y) = exp(-max(|x|^2 + |y|^2 - 2 x.y, 0) / s); the row norms are the fp32 roundings of fp64 sums.
 *   subsets      a_0[i] = 1 iff i < n.  For r = 1 .. R, row i has the key mix(base + (r << 32) + i), uint64 and wrapping, with
 *                bl_bootstrap_counts' mix and base = mix(seed * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15): it depends on
 *                (seed, r, i) alone.  a_r[i] = 1 iff fewer than n rows precede (key_i, i) in lexicographic order, so equal keys
 *                go to the lower row.  Integer work: device and twin agree bit for bit.
 *   the mask     uint8 [R + 2, ldm], ldm = bl_drift_mask_ld(N) = N rounded up to a multiple of 32: row r <= R is a_r, row
 *                R + 1 is all ones (it yields rho = K 1 and S); bytes N .. ldm - 1 of every row are 0.
 *   sums         with U = K A (A the [N, R + 2] matrix whose columns are the mask's rows):
 *                A_r = sum_i a_r[i] U[i, r];  B_r = sum_i U[i, r] = a_r^T K 1;  S = 1^T K 1;
 *                MMD2_r = A_r / n^2 + (S - 2 B_r + A_r) / m^2 - 2 (B_r - A_r) / (n m)   (the biased V-statistic)
 *                The MMD weights sum to zero, so the device works on K - c for a caller-chosen constant c in [0, 1] (`shift`;
 *                drift.py passes exp(-1 / scale), the kernel value at the mean squared distance) and adds c n^2, c n N, c N^2,
 *                c n and c N back in fp64: every output is of K itself.
 *   p-value      (1 + #{r >= 1 : MMD2_r >= MMD2_0}) / (R + 1), on the host in fp64.
 *   witness      for a scanned row i >= n: f_i = U[i, 0] / n - (rho_i - U[i, 0]) / m, rho = K 1; the most negative are the
 *                samples least like the reference.
 *
 * Arithmetic of bl_drift_permutation_sums.  Z_j Z_i^T on v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation (gfx950
 * has no xf32; embeddings are unbounded, which rules the clamped f16x3 images out).  The kernel tile in registers: n_i + n_j - 2 G,
 * clamp at 0, expf, minus c.  Then K ALONE is cut into three bf16 planes by truncation, hi + mid + lo == the fp32 value exactly,
 * and each plane is one v_mfma_f32_16x16x32_bf16 against the mask, which is exact in bf16: an fp32-class second product in three
 * terms.  The first product's accumulator tiles are the second's B operand as they lie.  Nothing of size N x N or N x R reaches
 * memory beyond the byte mask and, per 16 rows, one fp64 partial of A_r and B_r; a second kernel adds those in row order in fp64.
 * No atomics: equal bits on every run and for every col_tiles.  Rows beyond N, mask rows beyond R + 1 and the padding of D (to a
 * multiple of 64, as the similar-bug search pads) contribute exactly nothing.
 *
 * bl_drift_ok: 1 <= D <= BL_DRIFT_MAX_D and 1 <= R <= BL_DRIFT_MAX_PERMUTATIONS.
 * bl_drift_bandwidth: z [N, D] (row stride ldz, any alignment) -> out_rownorm float [N], out_bandwidth double [1] = s.
 *   workspace: bl_drift_bandwidth_workspace_bytes(N, D) bytes, 8-byte aligned.
 * bl_drift_subsets: -> out_mask uint8 [R + 2, ldm], ldm == bl_drift_mask_ld(N), 4-byte aligned.  One workgroup per row; the n-th
 *   smallest key by 8-bit radix selection over recomputed keys, no sort and no key in memory.
 * bl_drift_permutation_sums: -> out_sums double [2 (R + 1) + 1] = A_0 .. A_R | B_0 .. B_R | S; out_u0 double [N] = U[:, 0];
 *   out_rho double [N] = K 1.  bandwidth: the DEVICE double bl_drift_bandwidth wrote (no synchronisation in between).
 *   col_tiles: 16-row groups of the mask per workgroup, 4, 8 or 16, 0 = the default; for tests and tuning, the result does not
 *   depend on it.  workspace: bl_drift_sums_workspace_bytes(N, R) bytes, 8-byte aligned.
 * BL_EINVAL: null pointers, n < 2 or N - n < 2, R < 1, ldz < D, a wrong ldm, misaligned buffers, a workspace too small, shift
 *   outside [0, 1], col_tiles not in {0, 4, 8, 16}.  BL_ERANGE: D > BL_DRIFT_MAX_D, R > BL_DRIFT_MAX_PERMUTATIONS, N beyond int32.
 * No call synchronises. */
#define BL_DRIFT_MAX_D 512
#define BL_DRIFT_MAX_PERMUTATIONS 65533
int32_t bl_drift_ok(int32_t D, int64_t R);
int64_t bl_drift_mask_ld(int64_t N);
int64_t bl_drift_bandwidth_workspace_bytes(int64_t N, int32_t D);
int bl_drift_bandwidth(const float* z, int64_t ldz, int64_t N, int32_t D, double scale, void* workspace, int64_t workspace_bytes,
                       float* out_rownorm, double* out_bandwidth, void* stream);
int bl_drift_subsets(int64_t N, int64_t n, int64_t R, uint64_t seed, uint8_t* out_mask, int64_t ldm, void* stream);
int64_t bl_drift_sums_workspace_bytes(int64_t N, int64_t R);
int bl_drift_permutation_sums(const float* z, int64_t ldz, int64_t N, int64_t n, int32_t D, const float* rownorm, const uint8_t* mask,
                              int64_t ldm, int64_t R, const double* bandwidth, double shift, int32_t col_tiles, void* workspace,
                              int64_t workspace_bytes, double* out_sums, double* out_u0, double* out_rho, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Warning triage (buglab/models/triage.py), in csrc/bl_triage.hip.  BEYOND THE REFERENCE: it has no counterpart.  A ridge-
 * regularised logistic re-ranker fitted on a reviewer's verdicts (1 = accepted, 0 = dismissed), over the site embedding and the
 * site's location log-probability that bl_sim_embed_sites writes.  The fit is Newton's method on the host (buglab/models/
 * _triage.py::fit_logistic); the device forms the statistics of one iteration over all N labelled rows and, once fitted, scores
 * the rows of a scan.  buglab/models/_triage.py is the twin: the margins bit for bit, the sums in fp64.
 *
 *   features   P = D + 2.  phi_c = ((double)x_c - shift_c) * scale_c for c < D; phi_D = ((double)logprob - shift_D) * scale_D;
 *              phi_{D+1} = 1, the intercept.  shift, scale double [D + 1]: the host's, computed once (a constant column has
 *              scale 0).  w double [P].
 *   margin     z = sum_c w_c phi_c by ONE wave: columns in quads, lane l owns the quads q with q % 64 == l (the ownership of
 *              bl_attr_node_scores) and adds the ROUNDED products w_c * phi_c in ascending column order to its own sum, which
 *              starts at +0.0; the 64 sums go through the xor butterfly, strides 32 .. 1.
 *   row        e = exp(-|z|), d = 1 + e; (p, 1 - p) = (1 / d, e / d) for z >= 0 and (e / d, 1 / d) otherwise;
 *              s = c (p (1 - p)); r = -(c (1 - p)) for y != 0 and c p otherwise; loss = c (softplus(z) - y z), formed as
 *              c (max(u, 0) + log1p(e)) with u = -z for y != 0 and z otherwise: the same number without the difference of two
 *              large ones.  Nothing overflows: at |z| = 800 the loss is finite and s is exactly 0.
 *   sums       L = sum loss + (lambda / 2) sum_{c <= D} w_c^2;  g = sum_n r_n phi_n + lambda w~;
 *              H = sum_n (s_n phi_n) phi_n^T + lambda I~  (w~, I~: the intercept left out).
 *   skipped    a row with a non-finite entry in x or logprob is in no sum; it is counted.
 *
 * bl_triage_newton_stats: x float [N, D] (row stride ldx; 16-byte alignment with ldx % 4 == 0 only buys wider loads), logprob
 *   float [N], y uint8 [N], c double [N] >= 0 or NULL for all ones, lambda > 0 -> H double [P, P], both triangles and H == H^T bit
 *   for bit; g double [P]; scalars double [4] = L, sum of c over the rows used, rows used, rows skipped.  The Gram matrix runs on
 *   v_mfma_f64_16x16x4_f64 over the 16 x 16 tiles of the lower triangle, the embeddings widened in registers.  The rows are cut
 *   into S = min(BL_TRIAGE_MAX_SLICES, max(1, ceil(N / 128))) slices of ceil(N / S) rows rounded up to a multiple of 4; every
 *   slice's partial H and g go to the workspace and a last kernel adds them in slice order.  No atomics: the same bits on every
 *   run.  workspace: bl_triage_workspace_bytes(N, D) bytes (-1 for sizes the kernels do not take), 8-byte aligned, contents
 *   irrelevant.  Four launches, no synchronisation.  N == 0: BL_OK, zeros in the outputs that are not NULL, nothing launched.
 * bl_triage_score: the same rows and w -> margin double [N], prob double [N] = p; NaN in both for a skipped row.  One wave per
 *   row, the dot product above.
 * BL_EINVAL: null pointers, negative sizes, ldx < D, doubles not 8-byte or floats not 4-byte aligned, lambda <= 0, NaN or
 *   infinite, a workspace too small (the text names the size needed).  BL_ERANGE: D > BL_TRIAGE_MAX_D, N > 2^36.  All of it is
 *   checked before the first HIP call. */
#define BL_TRIAGE_MAX_D 512
#define BL_TRIAGE_MAX_SLICES 64
int64_t bl_triage_workspace_bytes(int64_t N, int32_t D);
int bl_triage_newton_stats(const float* x, int64_t ldx, const float* logprob, const double* shift, const double* scale, const double* w,
                           const uint8_t* y, const double* c, int64_t N, int32_t D, double lambda, void* workspace,
                           int64_t workspace_bytes, double* H, double* g, double* scalars, void* stream);
int bl_triage_score(const float* x, int64_t ldx, const float* logprob, const double* shift, const double* scale, const double* w,
                    int64_t N, int32_t D, double* margin, double* prob, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Review queue (buglab/models/review.py), in csrc/bl_review.hip.  BEYOND THE REFERENCE: it has no counterpart.  Given a budget
 * of B reviews and what was reviewed already, pick the B warnings that cover the scan best: each pick is the warning least like
 * everything reviewed or queued so far.  This is k-center greedy, or farthest-point selection (Gonzalez 1985; the core-set
 * selection of Sener & Savarese 2018).  buglab/models/_review.py is the same arithmetic in NumPy, equal bit for bit on every
 * output: picks, pick affinities, final best and near.
 *
 * All M rows live in ONE row space: first the L reviewed rows, then the N candidate rows.  The rows are bl_sim_quantize's int8
 * images q [M, Dp] (Dp = D rounded up to a multiple of 64, padding columns zero) with their r; r_i > 0 means the row is valid.
 * Selection runs on the images, where dot products are exact integers.
 *
 *   norm       n_i = sum_d q_id^2, int32 and exact, at most 512 * 127^2 = 8 258 048.  0 for an invalid row (its image is zero); a
 *              valid row has an entry +-127, so n_i >= 16129.
 *   affinity   a(i, j) = (double)(idot * |idot|) / (double)(n_i * n_j), idot = sum_d q_id q_jd.  Both products are formed in
 *              int64 and stay below 2^53, so both conversions are exact; the result is ONE IEEE quotient.  It is the signed
 *              squared cosine of the images, and a(i, i) == 1.0.  The affinity is monotone in the angle, and min, max and argmin
 *              commute with monotone maps: the picks are those of farthest-point selection on the angular metric.  No sqrt and
 *              no exp runs on the device.
 *   cover      per row: best_i double, -2.0 meaning "no centre yet"; near_i int32, -1 meaning none.  Applying a centre j to a
 *              valid row i: if a(i, j) > best_i, then best_i = a(i, j) and near_i = j.  For a SET of centres the result is
 *              (greater affinity, then lower centre index), and bl_review_cover_i8 combines with the caller's state in that same
 *              total order; an invalid centre covers nothing, an invalid row is left as it is.  A queued pick never displaces
 *              an equal earlier centre, because the comparison is strict.
 *   pick       among the rows with eligible_i != 0, n_i > 0 and best_i < stop, the one with the lowest best_i; ties go to the
 *              lowest index.  stop = S * S for a greatest similarity S in (0, 1].  If there is no such row the queue has ENDED:
 *              this pick and all later ones are -1 (affinity 0.0) and the state is left as it is.  Otherwise (s, best_s) is
 *              recorded and centre s applied to every valid row; row s itself gets best = 1.0, near = s by that same rule
 *              (best_s < stop <= 1 == a(s, s)), so it cannot be picked again.
 * Nothing in the arithmetic depends on a launch geometry.
 *
 * Image operands have a row stride (ldq, ldc): a multiple of 16, at least Dp, the base 16-byte aligned.
 * bl_review_norms: q -> n int32 [M].  One wave per row, the packed int8 dot.
 * bl_review_cover_i8: applies the L centres qc / nc (centre j has the index first_id + j) to the M rows q / n and UPDATES best
 *   double [M] and near int32 [M].  An M x L int8 GEMM on v_mfma_i32_16x16x64_i8 that is never stored: the epilogue turns each
 *   accumulator into an affinity in registers and keeps a running (best, near) per row.  slices in [1, BL_REVIEW_MAX_SLICES]:
 *   the centres are cut into that many parts for separate workgroups; the result does not depend on it.  Calling it twice over
 *   two parts of the centres equals calling it once with all of them.  No atomics.  workspace:
 *   bl_review_cover_workspace_bytes(M, slices) bytes (-1 for sizes the kernels do not take), 8-byte aligned, contents irrelevant.
 *   Two launches.
 * bl_review_greedy: B picks from the state (best, near), which it UPDATES -> picks int32 [B], pick_aff double [B] and pick_near
 *   int32 [B]: (best_s, near_s) at the time of the pick, the nearest earlier item (0.0 and -1 for no pick; -2.0 and -1 for a pick
 *   that no centre covered).  eligible uint8 [M] or NULL for all.  ONE call enqueues the whole chain, B + 1 launches of one step kernel,
 *   with no host synchronisation and no communication between workgroups inside a launch: every workgroup reduces the per-
 *   workgroup partials (best, index) of the launch before, all arrive at the same winner, each updates its own rows and writes its
 *   own partial into the other of two buffers.  blocks: the number of workgroups, 0 for bl_review_blocks(M) =
 *   min(BL_REVIEW_MAX_BLOCKS, ceil(M / BL_REVIEW_ROWS_PER_BLOCK)), a function of M alone; the results are the same for every
 *   value.  workspace: bl_review_workspace_bytes(M) bytes (-1 for M out of range), 8-byte aligned, contents irrelevant.
 * BL_EINVAL: null pointers, negative sizes, Dp not a multiple of 64, a row stride below Dp or not a multiple of 16, images not
 *   16-byte aligned, doubles not 8-byte aligned, stop outside (0, 1] (NaN included), slices or blocks out of range, a workspace too
 *   small.  BL_ERANGE: Dp > BL_SIM_MAX_D, M or L > BL_REVIEW_MAX_ROWS, B > BL_REVIEW_MAX_BUDGET.  All of it is checked before the
 *   first launch.  No call synchronises. */
#define BL_REVIEW_MAX_ROWS (1 << 20)
#define BL_REVIEW_MAX_BUDGET 16384
#define BL_REVIEW_MAX_SLICES 64
#define BL_REVIEW_MAX_BLOCKS 1024
#define BL_REVIEW_ROWS_PER_BLOCK 64
int bl_review_norms(const int8_t* q, int64_t ldq, int64_t M, int32_t Dp, int32_t* n, void* stream);
int64_t bl_review_cover_workspace_bytes(int64_t M, int32_t slices);
int bl_review_cover_i8(const int8_t* q, int64_t ldq, const int32_t* n, int64_t M, const int8_t* qc, int64_t ldc, const int32_t* nc,
                       int64_t L, int32_t first_id, int32_t Dp, int32_t slices, void* workspace, int64_t workspace_bytes, double* best,
                       int32_t* near, void* stream);
int32_t bl_review_blocks(int64_t M);
int64_t bl_review_workspace_bytes(int64_t M);
int bl_review_greedy(const int8_t* q, int64_t ldq, const int32_t* n, const uint8_t* eligible, int64_t M, int32_t Dp, int32_t B,
                     double stop, int32_t blocks, void* workspace, int64_t workspace_bytes, double* best, int32_t* near,
                     int32_t* picks, double* pick_aff, int32_t* pick_near, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Warning tracking (buglab/models/track.py), in csrc/bl_track.hip.  BEYOND THE REFERENCE: it has no counterpart.  Given the
 * warnings of an earlier scan and those of this one, find the ONE-TO-ONE assignment between them: which warnings persist (and
 * what the reviewer said about them), which are new, which are gone.  buglab/models/_track.py is the same arithmetic in NumPy,
 * equal bit for bit on every output, by ANOTHER algorithm (it orders the pairs; the device runs rounds).
 *
 *   rows        L old rows and N new rows: bl_sim_quantize's int8 images [rows, Dp] in ONE row space -- the old rows are a
 *               SiteIndex's embeddings, already centred, the new rows are centred with the index's mean -- with bl_review_norms'
 *               norms n (int32, 0 for an invalid row).
 *   affinity    the review queue's: a(i, j) = (double)(idot * |idot|) / (double)(n_i * n_j), idot = sum_d q_id q_jd, both
 *               products in int64 and below 2^53, ONE IEEE quotient.
 *   admissible  a pair (old i, new j) with n_i > 0, n_j > 0, a(i, j) >= floor (floor = S * S for a least similarity S in
 *               (0, 1]) and, when keys are given, key_old[i] == key_new[j].  A key is an int32 per row (the file or package,
 *               numbered on the host over the union of both sides).
 *   matching    repeatedly take, among the admissible pairs whose two rows are both unmatched, the FIRST in the order
 *               (greater affinity, then lower old index, then lower new index), and match it; stop when none is left.  A
 *               function of the input alone, and the unique stable matching under that order: no admissible pair in which each
 *               side would come before its partner.
 *   rounds      how the device computes it, without sorting L x N pairs.  A row is OPEN while it is unmatched.  In a round every
 *               open old row finds its best admissible open new row (the lower new index among equals) and every open new row
 *               its best admissible open old row (the lower old index among equals); EVERY pair that chose each other is
 *               matched.  A round that matches nothing ends the matching.  This equals the sequential definition: the first pair
 *               of the order is always mutual, and no pair that is mutual among the open rows can be pre-empted by an earlier
 *               pair of the order.  `rounds`, the number of rounds that matched something, is a function of the input too.
 * Nothing in the arithmetic depends on a launch geometry: no float atomics, no exp, no sqrt, compiled without contraction.
 *
 * Image operands have a row stride (a multiple of 16, at least Dp) and a 16-byte aligned base: bl_review_*'s rules.  Keys come
 * for both sides or for neither (NULL).
 * bl_track_best_i8: the directional best.  For each OPEN row i of the first side (open_old[i] != 0; NULL: all) the best
 *   admissible OPEN row of the second side -> best double [L], arg int32 [L]: (affinity, index), the lower index among equals;
 *   (-2.0, -1) for none and for a row that is not open.  The other direction is the same call with the sides exchanged.  An
 *   L x N int8 GEMM on v_mfma_i32_16x16x64_i8 that is never stored; the open rows of either side are compacted into ascending
 *   index lists first (a prefix sum), and each lane gathers its own row of a tile through the list.  slices in
 *   [1, BL_TRACK_MAX_SLICES]: into how many parts the second side is cut; the result does not depend on it.  workspace:
 *   bl_track_best_workspace_bytes(L, N, slices) bytes (-1 out of range), 8-byte aligned, contents irrelevant.  Four launches.
 * bl_track_match: up to max_rounds rounds from a state that it UPDATES: match_old int32 [L] and match_new int32 [N] (the partner,
 *   -1: unmatched; a fresh state is all -1) and match_aff double [N] (the affinity of a matched new row).  ONE call enqueues
 *   1 + 6 max_rounds launches on the caller's stream with no host synchronisation and no communication between workgroups
 *   inside a launch: the open lists of the state, then per round both directions of the best kernel with their merges, a mutual
 *   kernel with one thread per open new row, and the compaction, which also keeps the counts and the word that says the
 *   matching has ended.  Control words and lists are ping-pong buffered from launch to launch; once the matching has ended the
 *   remaining launches read the word and return.  status int32 [4]: rounds run by THIS call that matched something | pairs
 *   matched by this call | whether the matching has ended (a round of this call matched nothing) | open new rows left.  A call
 *   from the state an earlier call left continues the matching: two calls of max_rounds = r equal one call of 2 r in the state,
 *   and their rounds and pairs add up.  workspace: bl_track_match_workspace_bytes(L, N, slices) bytes.
 * BL_EINVAL: null pointers, negative sizes, Dp not a multiple of 64, a row stride below Dp or not a multiple of 16, images not
 *   16-byte aligned, doubles not 8-byte aligned, floor outside (0, 1] (NaN included), max_rounds < 1, slices out of range, keys
 *   for one side only, a workspace too small.  BL_ERANGE: Dp > BL_SIM_MAX_D, L or N > BL_REVIEW_MAX_ROWS, max_rounds >
 *   BL_TRACK_MAX_ROUNDS.  All of it is checked before the first launch.  No call synchronises. */
#define BL_TRACK_MAX_SLICES 64
#define BL_TRACK_MAX_ROUNDS 4096
int64_t bl_track_best_workspace_bytes(int64_t L, int64_t N, int32_t slices);
int bl_track_best_i8(const int8_t* q_old, int64_t ld_old, const int32_t* n_old, const int32_t* key_old, const uint8_t* open_old,
                     int64_t L, const int8_t* q_new, int64_t ld_new, const int32_t* n_new, const int32_t* key_new,
                     const uint8_t* open_new, int64_t N, int32_t Dp, double floor, int32_t slices, void* workspace,
                     int64_t workspace_bytes, double* best, int32_t* arg, void* stream);
int64_t bl_track_match_workspace_bytes(int64_t L, int64_t N, int32_t slices);
int bl_track_match(const int8_t* q_old, int64_t ld_old, const int32_t* n_old, const int32_t* key_old, int64_t L, const int8_t* q_new,
                   int64_t ld_new, const int32_t* n_new, const int32_t* key_new, int64_t N, int32_t Dp, double floor,
                   int32_t max_rounds, int32_t slices, void* workspace, int64_t workspace_bytes, int32_t* match_old,
                   int32_t* match_new, double* match_aff, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Confidence calibration (buglab/models/calibrate.py), in csrc/bl_confidence.hip.  BEYOND THE REFERENCE: it has no
 * counterpart; what is calibrated is the confidence its evaluate.py:60-140 thresholds and its visualize.py ranks by.  One
 * inverse temperature beta and a NO_BUG bias rescale the localization distribution, one repair_beta the repair groups:
 *   z_i = beta * l_i (+ bias on NO_BUG);  l'_i = log_softmax(z)_i = (z_i - m) - log1p(sum over i != i_m of exp(z_i - m)),
 * m = z's first maximum, at i_m.  fp64 throughout, compiled without fused multiply-adds; buglab/models/_calibrate.py is the
 * same arithmetic in NumPy.  Entries that are not above -inf have probability 0: they enter no maximum and no sum.
 *
 * bl_conf_loc_stats: a POOL of nseg location segments, segment s = vals[seg_off[s] : seg_off[s + 1]] (fp32 log-probabilities,
 *   offsets clamped to [0, n_vals]), NO_BUG at its last place, the target at place tgt[s] of the segment.  With
 *   F(beta, bias) = - sum_s l'_s[tgt[s]]:  out[0..5] = F, dF/dbeta, dF/dbias, d2F/dbeta2, d2F/dbeta dbias, d2F/dbias2.
 *   Per segment (E = sum_i p_i l_i, p = exp(l'), p_nb = NO_BUG's):  log1p(Z') + (m - z_tgt) | E - l_tgt | p_nb - [tgt is NO_BUG] |
 *   sum_i p_i (l_i - E)^2 | p_nb (l_nb - E) | p_nb (1 - p_nb).  An empty segment contributes 0; a segment with nothing above
 *   -inf or a target outside it contributes NaN.
 * bl_conf_group_stats: the same over nseg repair groups with one scale and no bias: out[0..2] = F_r, F_r', F_r''.
 *   Both: one wave per segment, lanes stride over it (any length); the segments' terms are written to partials
 *   ([6, nseg] / [3, nseg] doubles, the caller's) and a second kernel sums each column in an order fixed by nseg alone: no
 *   atomics, bit-identical from launch to launch.  nseg == 0 writes zeros.  No synchronisation.
 *
 * bl_conf_apply: a predict minibatch's flat output [loc | text | var | swap] (n_flat floats) IN PLACE.  Sample b < B owns
 *   flat[candidate_ptr[b] : candidate_ptr[b + 1]] (clamped to [0, C]) and its NO_BUG entry flat[C + b]: they become l'.
 *   Repair group g < G owns flat[item_base + group_items[k]] for k in group_ptr[g] : group_ptr[g + 1] (the CSR the model's own
 *   log-softmax runs over; items outside [0, n_items) are left out): they become log_softmax(repair_beta * r).  Every entry
 *   belongs to at most one segment.  Rounded once to fp32; -inf stays -inf.  B == 0 / G == 0 leave that part untouched.
 * BL_EINVAL: null pointers, negative sizes, a scale that is not finite and > 0, a bias that is not finite, C + B > n_flat,
 * item_base + n_items > n_flat.  BL_ERANGE: n_vals / n_flat beyond int32. */
int bl_conf_loc_stats(const float* vals, int64_t n_vals, const int32_t* seg_off, const int32_t* tgt, int32_t nseg, double beta,
                      double bias, double* partials, double* out, void* stream);
int bl_conf_group_stats(const float* vals, int64_t n_vals, const int32_t* seg_off, const int32_t* tgt, int32_t nseg, double beta,
                        double* partials, double* out, void* stream);
int bl_conf_apply(float* flat, int64_t n_flat, const int32_t* candidate_ptr, int32_t B, int64_t C, const int32_t* group_ptr,
                  const int32_t* group_items, int32_t G, int64_t n_items, int64_t item_base, double beta, double bias,
                  double repair_beta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Knowledge distillation (buglab/models/distill.py annotates records with a teacher's distributions; GnnBugLabModule
 * .set_distillation switches the term on), in csrc/bl_distill.hip.  BEYOND THE REFERENCE: it has no soft-target loss; the term
 * sits beside the hard-label loss assembly of buglab/models/gnn.py:221-251 and
 * buglab/models/layers/localizationmodule.py:63-124 (bl_bug_loss_fwd above) and reads the same logits.  Per segment, in fp64,
 * compiled without fused multiply-adds (buglab/models/_distill.py is the same arithmetic in NumPy):
 *   a_i = z_i / tau, ms = max a, Ss = sum exp(a_i - ms):  log q_i = (a_i - ms) - log Ss,  q_i = exp(a_i - ms) / Ss;
 *   u_i = t_i / tau over the teacher entries t_i > -inf, mt, St likewise:  log p_i = (u_i - mt) - log St,  p_i = exp(u_i - mt) / St;
 *   KL = sum over p_i > 0 of p_i (log p_i - log q_i);  delta_i = q_i - p_i, p_i = 0 where t_i is -inf or NaN.
 * Location segment b < B: the candidate rows candidate_ptr[b] .. candidate_ptr[b + 1] (clamped to [0, C]) and then NO_BUG,
 * whose student logit is the constant 1.0 and whose teacher value is teacher_loc[C + b] (teacher_loc has C + B entries, in the
 * item order of the localization log-softmax).  Repair segment g < G: the logits repair_group_items[k], k in
 * repair_group_ptr[g] : repair_group_ptr[g + 1] (the CSR of the model's own repair log-softmax: every logit belongs to exactly one
 * group; items outside [0, R) are left out), teacher_repair in the order of repair_logits = text | var | swap.  A segment with
 * no teacher entry above -inf is skipped: KL 0, delta 0, counted; an empty group counts as nothing.
 *
 * bl_distill_fwd: one wave per segment, lanes stride over it (any length).  delta [C + R] = candidates | logits, rounded once to
 *   fp32; NO_BUG has none.  out[8] = location KL sum | repair KL sum | distilled location segments | distilled repair groups |
 *   location segments where the student's first maximum is the teacher's | skipped segments | 0 | 0.  The sums: per-segment
 *   values in ws (bl_distill_workspace_bytes(B, G) bytes, the caller's), then a second kernel in an order fixed by B and G
 *   alone; fp64, rounded once to fp32; no atomics, bit-identical from launch to launch.  B, G, C, R may each be 0.
 * bl_distill_bwd: g_loc_scores[i] = g_loc * delta[i] / tau (i < C), g_repair_logits[j] = g_rep * delta[C + j] / tau (j < R);
 *   g_loc, g_rep: device scalars.  Elementwise, multi-workgroup, writes every entry.
 * BL_EINVAL: null pointers, negative sizes, a temperature that is not finite and > 0, C > 0 with B == 0, R > 0 with G == 0.
 * BL_ERANGE: sizes beyond int32. */
int64_t bl_distill_workspace_bytes(int32_t B, int32_t G);
int bl_distill_fwd(const float* loc_scores, const float* repair_logits, const float* teacher_loc, const float* teacher_repair,
                   const int32_t* candidate_ptr, const int32_t* repair_group_ptr, const int32_t* repair_group_items, int32_t B,
                   int32_t G, int64_t C, int64_t R, double tau, void* ws, float* delta, float* out, void* stream);
int bl_distill_bwd(const float* delta, int64_t C, int64_t R, const float* g_loc, const float* g_rep, double tau,
                   float* g_loc_scores, float* g_repair_logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Near-duplicate detection (buglab/data/deduplication/index.py:15-70: `DuplicationIndex.check_if_duplicate_and_add`, which
 * updates a 256-permutation MinHash one token at a time and keeps one Python dict per LSH band), in csrc/bl_dedup.hip.  The
 * arithmetic is the written specification of DESIGN.md "Near-duplicate detection"; all of it is integer work and every result is
 * exact.  Buffers are the caller's, on the device; nothing is read back.
 *
 * bl_dedup_sha1_u32 (index.py:36-37, `min_hash.update(token.encode())`: the token's hash value): token t is
 *   bytes[tok_off[t] : tok_off[t + 1]] (tok_off has ntokens + 1 entries, clamped to [0, nbytes]; any length, the empty token
 *   included); out[t] = the first four bytes of its SHA-1 digest read as a little-endian uint32.  One thread per token.
 *
 * bl_dedup_minhash (index.py:35-37): document d owns hashes[doc_off[d] : doc_off[d + 1]] (ndocs + 1 offsets, clamped to
 *   [0, nhashes]); sigs[d, k] = min(2^32 - 1, min over its hashes hv of (((perm_a[k] * hv + perm_b[k]) mod 2^64) mod (2^61 - 1))
 *   & 0xFFFFFFFF), k < num_perm; sigs is [ndocs, num_perm].  One workgroup per document, one permutation per lane:
 *   BL_EINVAL unless 1 <= num_perm <= BL_DEDUP_MAX_PERM.  A repeated hash changes nothing (a minimum).
 *
 * bl_dedup_lsh_insert_query (index.py:39-46, the query and the insert): sigs [total, num_perm] holds the signatures of the
 *   documents numbered 0 .. total - 1 in insertion order; band j of a document is its values [j rows, (j + 1) rows).  table
 *   [bands, slots] uint32, 0xFFFFFFFF = empty, slots a power of two: per band an open-addressing table in which each band key
 *   owns one slot holding the smallest document number inserted with that key; keys are told apart by comparing all `rows`
 *   values with the stored signature.  The call files documents insert_from .. total - 1, and then (a second launch) writes
 *   flags[i - query_from] = 1 if some document numbered below i shares a whole band with i, else 0, for i = query_from ..
 *   total - 1.  The answers do not depend on the order in which the device runs the threads, nor on how the documents were
 *   split into calls.  insert_from = 0 on an empty table rebuilds the index (growth, or a loaded checkpoint); query_from =
 *   total asks nothing (flags may be NULL).  BL_EINVAL: bands * rows > num_perm, slots not a power of two, 2 * total > slots
 *   (the load bound: rebuild at a larger capacity first), ranges out of order, null pointers.  *status (device, zeroed by the
 *   caller once) has bit 0 / bit 1 set if an insert found no slot / a queried document was not in the table: both mean the
 *   caller broke the contract, and the flags of that call are then not to be trusted. */
#define BL_DEDUP_MAX_PERM 256
int bl_dedup_sha1_u32(const uint8_t* bytes, int64_t nbytes, const int64_t* tok_off, int64_t ntokens, uint32_t* out, void* stream);
int bl_dedup_minhash(const uint32_t* hashes, int64_t nhashes, const int64_t* doc_off, int64_t ndocs, const uint64_t* perm_a,
                     const uint64_t* perm_b, int32_t num_perm, uint32_t* sigs, void* stream);
int bl_dedup_lsh_insert_query(const uint32_t* sigs, int32_t num_perm, int32_t bands, int32_t rows, uint32_t* table, int64_t slots,
                              int64_t insert_from, int64_t query_from, int64_t total, int32_t* flags, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * `seq-great` / `seq-rat` relational-transformer block (reference buglab/models/layers/relational_transformer.py,
 * relational_multihead_attention.py, multihead_attention.py): the row-wise kernels around the MFMA GEMMs.
 * q (pre-scaled by dk^-0.5), k, v, the attention context and their gradients are [B, H, L, dk] (one [L, dk] matrix per
 * (sample, head) = one GEMM group); scores / probabilities are [B * H * L, L].  The minibatch's edges come as a CSR over
 * query rows (b * L + i): ekey = key position, ecode = 2 * edge_type + direction (0: the query is the edge's source). */
/* y = LayerNorm(x + r) (r may be NULL); z_out (optional) receives x + r; the backward is bl_layernorm_bwd.
 * nn.LayerNorm of relational_transformer.py:84-85 + the residual adds of :113,122 */
int bl_add_layernorm_fwd(const float* x, const float* r, const float* gamma, const float* beta, float eps, int32_t nrows,
                         int32_t D, float* z_out, float* y, float* mean, float* rstd, void* stream);
/* S[(b, h, i), key] += edge term, relational_multihead_attention.py:90-152 (index_put_ with accumulate=True):
 * mode 0: <bias[code][h, :], q[b, h, i, :]> (what seq-great runs, :135-152); mode 1: bias[code][h] * sum_d k[b, h, key, d] */
int bl_rel_attn_bias_fwd(const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                         int32_t dk, int32_t mode, const float* qk, const float* bias_f, const float* bias_r, float* S,
                         void* stream);
/* gradients of the edge terms from dS: g_q += (mode 0, row-owned), g_k += (mode 1, atomics), g_bias_* += (atomics) */
int bl_rel_attn_bias_bwd(const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                         int32_t dk, int32_t mode, int32_t T, const float* qk, const float* bias_f, const float* bias_r,
                         const float* dS, float* g_q, float* g_k, float* g_bias_f, float* g_bias_r, void* stream);
/* softmax over keys with the padding keys (key >= lens[row / rows_per_sample]) masked, in place (multihead_attention.py:65-71) */
int bl_masked_softmax_fwd(float* S, int32_t R, int32_t L, int32_t rows_per_sample, const int32_t* lens, void* stream);
/* ... and nn.Dropout on the probabilities in the same pass (multihead_attention.py:72): S <- P, Pd <- dropout(P) with mask
 * element row * L + k (= bl_dropout_inplace on a copy of P); drop.p == 0: Pd is not written */
int bl_masked_softmax_dropout_fwd(float* S, int32_t R, int32_t L, int32_t rows_per_sample, const int32_t* lens, bl_dropout_t drop,
                                  float* Pd, void* stream);
/* dP <- P * (dP - sum_k P dP) */
int bl_softmax_bwd(const float* P, float* dP, int32_t R, int32_t L, void* stream);
/* the same with dP arriving as the gradient of dropout(P): it passes the mask first (bl_dropout_inplace + bl_softmax_bwd) */
int bl_softmax_dropout_bwd(const float* P, float* dP, int32_t R, int32_t L, bl_dropout_t drop, void* stream);
/* The attention probabilities of `seq-great` in one kernel (multihead_attention.py:54-72 with the edge terms of
 * relational_multihead_attention.py:135-152, mode 0): P[(b, h, i), :] = softmax_keys(q[b, h, i, :] . k[b, h, :, :]^T + edge terms,
 * keys >= lens[b] masked), Pd = dropout(P) (mask element row * L + key; drop.p == 0: Pd not written).  q (pre-scaled), k:
 * [B, H, L, dk]; the edge CSR may be NULL (no entries); T edge types, bias_f / bias_r [T, H * dk].  Replaces the grouped
 * Q.K^T GEMM + bl_rel_attn_bias_fwd + bl_masked_softmax_dropout_fwd (three passes over the [B H L, L] scores).
 * bl_rel_attn_probs_ok: whether the shape is handled (L % 4 == 0, L <= 1024, dk in {16, 32, 64}, K^T of one head in 64 KB,
 * 2 T dk <= 1024). */
int32_t bl_rel_attn_probs_ok(int32_t L, int32_t dk, int32_t T);
int bl_rel_attn_probs_fwd(const float* q, const float* k, const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode,
                          int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T, const float* bias_f, const float* bias_r,
                          const int32_t* lens, bl_dropout_t drop, float* P, float* Pd, void* stream);
/* ... and their backward: g_ctx [B, H, L, dk] = gradient of the context, v, q [B, H, L, dk], P from the forward call ->
 * dS [B H L, L] = d loss / d scores (the grouped GEMMs dQ = dS.K and dK = dS^T.Q read it);  with an edge CSR also
 * gq_edge [B, H, L, dk] = the edge terms' part of d loss / d q (every row is written: zeros where a row has no entries) and
 * g_bias_f / g_bias_r [T, H dk] += (atomics).  Replaces dO.V^T GEMM + bl_softmax_dropout_bwd + bl_rel_attn_bias_bwd. */
int bl_rel_attn_probs_bwd(const float* g_ctx, const float* v, const float* P, const float* q, const int32_t* row_ptr,
                          const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T,
                          const float* bias_f, const float* bias_r, bl_dropout_t drop, float* dS, float* gq_edge, float* g_bias_f,
                          float* g_bias_r, void* stream);
/* The attention's four tall-and-skinny products for head dimension 32 (bl_attn_mm32_ok: dk == 32, L % 4 == 0, L <= 1164),
 * exact-fp32 matrix cores, the head's [L, 32] matrix whole in LDS and the [G L, L] operand streamed once:
 *   bl_attn_rows_times        out[(g, i), :] = (sum_k A[(g, i), k] M[g, k, :] (+ add[(g, i), :])) * scale   -- P.V, dS.K
 *   bl_attn_transposed_times  out[g, k, :]   = sum_i A[(g, i), k] Bm[g, i, :]                              -- P^T.dO, dS^T.Q
 * (the grouped bl_gemm_rows / bl_gemm_wgrad calls of multihead_attention.py:73-77 and their autograd). */
int32_t bl_attn_mm32_ok(int32_t L, int32_t dk);
int bl_attn_rows_times(const float* A, const float* M, int32_t G, int32_t L, int32_t dk, const float* add, float scale, float* out,
                       void* stream);
int bl_attn_transposed_times(const float* A, const float* Bm, int32_t G, int32_t L, int32_t dk, float* out, void* stream);
/* The same four kernels on HEAD VIEWS: a [B, H, L, dk] operand given by a base pointer and three strides (element (b, h, l, d) at
 * p[b sb + h sh + l sl + d]; 16-byte aligned base, strides multiples of 4), so that q / k / v are read straight from the QKV
 * projection's [B L, H 3 dk] output (per head [q | k | v], multihead_attention.py:46-50: p = qkv + which dk, sb = L 3 H dk,
 * sh = 3 dk, sl = 3 H dk), the context is written as [B L, H dk] and the gradients land in the layout the projection's
 * gradient GEMMs read -- no permuted copies.  q_scale / bm_scale multiply q where it is loaded (the reference's pre-scaled
 * queries, multihead_attention.py:54: same rounding as a scaled copy).  P, Pd, dS, gq_edge, add stay [B H L, *] contiguous. */
typedef struct {
  float* p;
  int64_t sb;
  int32_t sh, sl;
} bl_head_view_t;
int bl_rel_attn_probs_fwd_v(const bl_head_view_t* q, float q_scale, const bl_head_view_t* k, const int32_t* row_ptr, const int32_t* ekey,
                            const int32_t* ecode, int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T, const float* bias_f,
                            const float* bias_r, const int32_t* lens, bl_dropout_t drop, float* P, float* Pd, void* stream);
int bl_rel_attn_probs_bwd_v(const bl_head_view_t* g_ctx, const bl_head_view_t* v, const float* P, const bl_head_view_t* q, float q_scale,
                            const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H, int32_t dk,
                            int32_t T, const float* bias_f, const float* bias_r, bl_dropout_t drop, float* dS, float* gq_edge,
                            float* g_bias_f, float* g_bias_r, void* stream);
/* a_drop (p > 0): A is read through the counter-hash dropout mask, element index (g L + i) L + k -- A = the probabilities P of
 * bl_rel_attn_probs_fwd_v called with Pd == NULL: nn.Dropout on the attention probabilities (multihead_attention.py:72) without
 * a stored copy of the dropped matrix */
/* out_packed (optional; out may then be NULL): the result in bl_pack_bf16x3's form as columns of a packed [B L, 3 W] matrix --
 * element (b, h, l, d), plane pl at p[((b L + l) 3 + pl) W + col0 + h hs + d] (16-byte aligned base, W a multiple of 8, col0 and hs
 * multiples of 4): the context as the output projection's operand (W = H dk, col0 = 0, hs = dk), the gradients of q / k / v as the
 * operand of the QKV projection's gradient GEMMs (W = 3 H dk, col0 = which dk, hs = 3 dk) */
typedef struct {
  uint16_t* p;
  int32_t W, col0, hs;
} bl_packed_head_view_t;
int bl_attn_rows_times_v(const float* A, const bl_head_view_t* M, int32_t B, int32_t H, int32_t L, int32_t dk, const float* add, float scale,
                         const bl_head_view_t* out, bl_dropout_t a_drop, const bl_packed_head_view_t* out_packed, void* stream);
int bl_attn_transposed_times_v(const float* A, const bl_head_view_t* Bm, float bm_scale, int32_t B, int32_t H, int32_t L, int32_t dk,
                               const bl_head_view_t* out, bl_dropout_t a_drop, const bl_packed_head_view_t* out_packed, void* stream);
/* Streaming (online-softmax) form of the same attention, any L % 4 == 0: multihead_attention.py:46-80 with the edge terms of
 * relational_multihead_attention.py:72-178 (mode 0, no value biases) without a [B H L, L] array in either direction.
 *   fwd  ctx[b, h, i, :] = sum_j Pd[i, j] v[b, h, j, :] and lse[(b H + h) L + i] = max_j s_ij + log sum_j e^(s_ij - max), where
 *        s_ij = q_scale q_i . k_j + sum over the CSR entries (row b L + i, key j, code) of <q_scale q_i, bias[code][h, :]>, keys
 *        >= lens[b] masked, P = softmax_j s, Pd = dropout(P) with mask element ((b H + h) L + i) L + j (bl_rel_attn_probs_fwd's).
 *   bwd  recomputes P tile by tile from q, k, the entries and lse; dS = P (mask g_Pd / (1 - p) - delta) with delta_i = sum_j P_ij mask
 *        g_Pd_ij / (1 - p) summed from the recomputed tiles first (delta: fp32 [B H L] scratch of the caller, written and read here);
 *        g_q = (dS.K + sum dS_ij bias[code]) q_scale, g_k = dS^T.(q_scale q), g_v = Pd^T.g_ctx: every row written by one owner in a
 *        fixed order (bitwise reproducible, no float atomics); g_bias_f / g_bias_r [T, H dk] += sum dS_ij q_scale q_i (per
 *        workgroup table, then atomics, as bl_rel_attn_probs_bwd).
 * q, k, v, ctx, g_ctx, g_q, g_k, g_v are head views (16-byte aligned base, strides multiples of 4); lse fp32 [B H L]; the edge
 * CSR may be NULL (all three); bias_f / bias_r [T, H dk] are read only when there is a CSR but must not be NULL.  With dropout
 * B H L^2 < 2^32.  bl_rel_attn_stream_ok: L % 4 == 0, dk == 32, 2 T dk <= 1024; no upper bound on L. */
int32_t bl_rel_attn_stream_ok(int32_t L, int32_t dk, int32_t T);
int bl_rel_attn_stream_fwd(const bl_head_view_t* q, float q_scale, const bl_head_view_t* k, const bl_head_view_t* v, const int32_t* row_ptr,
                           const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T,
                           const float* bias_f, const float* bias_r, const int32_t* lens, bl_dropout_t drop, const bl_head_view_t* ctx,
                           float* lse, void* stream);
int bl_rel_attn_stream_bwd(const bl_head_view_t* g_ctx, const float* lse, const bl_head_view_t* q, float q_scale, const bl_head_view_t* k,
                           const bl_head_view_t* v, const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L,
                           int32_t H, int32_t dk, int32_t T, const float* bias_f, const float* bias_r, const int32_t* lens,
                           bl_dropout_t drop, float* delta, const bl_head_view_t* g_q, const bl_head_view_t* g_k,
                           const bl_head_view_t* g_v, float* g_bias_f, float* g_bias_r, void* stream);
/* `rat` edge value biases (relational_multihead_attention.py:155-178): ctx[b, h, i, :] += P[(b, h, i), key] * vb[code][h, :] */
int bl_rel_value_bias_fwd(const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                          int32_t dk, const float* P, const float* vb_f, const float* vb_r, float* ctx, void* stream);
int bl_rel_value_bias_bwd(const int32_t* row_ptr, const int32_t* ekey, const int32_t* ecode, int32_t B, int32_t L, int32_t H,
                          int32_t dk, int32_t T, const float* P, const float* g_ctx, const float* vb_f, const float* vb_r,
                          float* dP, float* g_vb_f, float* g_vb_r, void* stream);
/* in-place counter-hash dropout (forward and backward are the same call) */
int bl_dropout_inplace(float* x, int64_t n, bl_dropout_t drop, void* stream);

/* bl_add_layernorm_fwd with a lane owning four consecutive channels (D a multiple of 4, 16-byte aligned pointers) and,
 * if y_packed != NULL, the result also in bl_pack_bf16x3's form [nrows, 3 D]: the next Linear's operand without a packing pass */
int bl_add_layernorm_fwd_packed(const float* x, const float* r, const float* gamma, const float* beta, float eps, int32_t nrows,
                                int32_t D, float* z_out, float* y, float* mean, float* rstd, uint16_t* y_packed, void* stream);

/* One relational transformer encoder layer per call (csrc/bl_great_layer.hip): reference
 * buglab/models/layers/relational_transformer.py:104-124 in the configuration `seq-great` runs -- normalisation "postnorm"
 * (both sublayers normalised by norm1, :123-124), rezero off, relu feed-forward, vector query edge bias
 * (relational_multihead_attention.py:135-152), no edge value biases; head dimension 32.
 *   x1  = norm1(x + dropout(out_proj(attention(qkv_proj(x)))))       out = norm1(x1 + dropout(linear2(dropout(relu(linear1(x1))))))
 * Weights come packed (bl_pack_weights_x6 of the [in, out] matrices: w_is_kn = 1 for forward, the *_bwd images w_is_kn = 0 for the
 * input-gradient GEMMs; NULL in a forward-only description).  Activations are [B L, *] row-major fp32; x_packed (optional) is
 * bl_pack_bf16x3 of x -- the previous layer's out_packed -- and must stay alive until the backward call; out_packed (optional)
 * receives the packed output.  Dropout counters as the op-by-op path (bl_gemm_rows_x6_epi / bl_rel_attn_probs_fwd): element
 * index row * width + column of the tensor the mask applies to.
 * bl_great_layer_ok: dk == 32, bl_rel_attn_probs_ok(L, dk, T), H dk and FF multiples of 32, H dk <= 512, fewer than 2^32 elements
 * in any dropout index space, deterministic mode off. */
typedef struct {
  int32_t B, L, H, dk, T, FF;
  const int32_t* row_ptr; /* edge CSR over query rows (bl_rel_attn_probs_fwd); all three NULL: no entries */
  const int32_t* ekey;
  const int32_t* ecode;
  const int32_t* lens;  /* [B] */
  const float* bias_f;  /* [T, H dk] */
  const float* bias_r;
  const float* norm_g;  /* [H dk] norm1 */
  const float* norm_b;
  const float* lin1_b;  /* [FF] */
  const float* lin2_b;  /* [H dk] */
  const uint16_t *qkv_w, *out_w, *lin1_w, *lin2_w;                 /* forward images */
  const uint16_t *qkv_w_bwd, *out_w_bwd, *lin1_w_bwd, *lin2_w_bwd; /* input-gradient images */
  float ln_eps;
  bl_dropout_t drop_attn;      /* on the attention probabilities */
  bl_dropout_t drop_att_out;   /* dropout1: on the attention branch */
  bl_dropout_t drop_ff_hidden; /* inside the feed-forward block */
  bl_dropout_t drop_ff_out;    /* dropout2: on the feed-forward branch */
} bl_great_layer_t;
/* gradient buffers, all ACCUMULATED into (fp32 atomics): zeroed buffers or the running gradients */
typedef struct {
  float *qkv_w, *out_w, *lin1_w, *lin1_b, *lin2_w, *lin2_b; /* [D, 3 D], [D, D], [D, FF], [FF], [FF, D], [D] */
  float *norm_g, *norm_b;                                   /* [D] */
  float *bias_f, *bias_r;                                   /* [T, D] (may be NULL without edge entries) */
} bl_great_layer_grads_t;
int32_t bl_great_layer_ok(int32_t B, int32_t L, int32_t H, int32_t dk, int32_t T, int32_t FF);
/* `saved` (forward -> backward; own_xp: the call packs x itself because no x_packed is handed in) and workspace bytes
 * (backward: 0 = forward, 1 = backward, 3 = forward-only call with saved == NULL) */
int64_t bl_great_layer_saved_bytes(int32_t B, int32_t L, int32_t H, int32_t dk, int32_t FF, int32_t own_xp);
int64_t bl_great_layer_workspace_bytes(int32_t B, int32_t L, int32_t H, int32_t dk, int32_t FF, int32_t backward);
int bl_great_layer_fwd(const bl_great_layer_t* d, const float* x, const uint16_t* x_packed, float* out, uint16_t* out_packed, void* saved,
                       void* ws, void* stream);
/* side_stream (optional): the four weight-gradient GEMMs run there next to the input-gradient chain; joined before the call returns */
int bl_great_layer_bwd(const bl_great_layer_t* d, const uint16_t* x_packed, const float* g_out, const void* saved, void* ws, float* g_x,
                       const bl_great_layer_grads_t* g, void* stream, void* side_stream);

/* ---------------------------------------------------------------------------------------------
 * T1  optimiser on flat fp32 buffers: global-norm clip (buglab/models/train.py:104, clip 0.5) fused
 * with Adam (buglab/models/utils.py:51-52).  bl_sqnorm writes sum(g^2) to *out (device scalar);
 * bl_adam_clip_step reads it on the device -- no host sync.  The sum is taken in one fixed order (per-block partials in
 * `scratch`, bl_sqnorm_scratch_bytes() bytes, then one block): equal gradients give a bit-equal norm on every replica. */
int64_t bl_sqnorm_scratch_bytes(void);
int bl_sqnorm(const float* g, int64_t n, float* out, float* scratch, void* stream);
int bl_adam_clip_step(float* param, const float* grad, float* m, float* v, int64_t n, const float* grad_sqnorm,
                      float grad_prescale, float clip_norm, float lr, float beta1, float beta2, float eps,
                      int32_t step, void* stream);
/* data-parallel form: `grad` is the all-reduced SUM over ranks of (graphs on the rank) x (the rank's gradient) and
 * *batch_total (device) the all-reduced number of graphs: the update uses grad / *batch_total; *batch_total <= 0 (no
 * rank had a minibatch) leaves parameters and moments untouched.  No value returns to the host. */
int bl_adam_clip_step_dp(float* param, const float* grad, float* m, float* v, int64_t n, const float* grad_sqnorm,
                         const float* batch_total, float clip_norm, float lr, float beta1, float beta2, float eps,
                         int32_t step, void* stream);
/* Weight averaging (beyond the reference): the two calls above, keeping an exponential moving average of the parameters in the
 * SAME pass -- after the new value p_new of an element is written, ema = fma(ema_one_minus_decay, p_new - ema, ema).
 * `param`, `m`, `v` come out bit-identical to the calls without the average.  ema_one_minus_decay = 1 - decay of THIS update,
 * 0 < it <= 1 (the host owns the warm-up of the decay); `ema` must not overlap `param`.  In the data-parallel form
 * *batch_total <= 0 leaves `ema` untouched as well. */
int bl_adam_clip_step_ema(float* param, const float* grad, float* m, float* v, float* ema, int64_t n, const float* grad_sqnorm,
                          float grad_prescale, float clip_norm, float lr, float beta1, float beta2, float eps, int32_t step,
                          float ema_one_minus_decay, void* stream);
int bl_adam_clip_step_dp_ema(float* param, const float* grad, float* m, float* v, float* ema, int64_t n, const float* grad_sqnorm,
                             const float* batch_total, float clip_norm, float lr, float beta1, float beta2, float eps, int32_t step,
                             float ema_one_minus_decay, void* stream);
/* exchanges the contents of two fp32 buffers of n elements in one pass (evaluating / saving the averaged weights: the
 * parameters' views stay where they are, the CONTENTS trade places).  Any 4-byte aligned pointers; n == 0 is a no-op;
 * overlapping ranges are refused. */
int bl_swap_f32(float* a, float* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BUGLAB_HIP_H */
