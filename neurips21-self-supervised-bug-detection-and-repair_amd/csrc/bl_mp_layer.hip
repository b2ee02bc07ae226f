// One MlpMessagePassingLayer per C call: bl_mp_layer_fwd / bl_mp_layer_bwd (SURVEY.md section 8b's minimum
// set; kwargs of the reference call site buglab/models/gnnlayerdefs.py:6-23) + the optional per-kernel
// HIP-event timing bench.py reads (bl_prof_*).
//
//   forward   pack h (one or two sources: a ConcatResidual input [stash ; current] is packed in place, no
//             concatenated copy) -> bf16x6 message GEMM -> segmented max + GELU + LayerNorm (+ routing bitmask,
//             activation derivative at the winners) -> dense + tanh + dropout
//   backward  node update's backward in one kernel (bl_node_update_bwd: act/dropout backward + bias gradient, dense input
//             gradient, LayerNorm backward, packed results; three kernels where its shapes do not apply) -> dense weight
//             gradient (side stream) || routed bf16x6 weight gradient (side stream) || routed input gradient (vector
//             units from the non-zeros, or bf16x6 GEMM) -> segmented sums over the src / tgt CSRs (two outputs for a
//             folded concat).  With the run arrays of the minibatch (bl_mp_layer_t.num_runs; f16x3, max aggregation, matrix cores):
//             OR of the routing masks per run -> both routed GEMMs over E + R rows of Din columns (source halves per message,
//             target halves per run) -> segmented sums over the source CSR and the run CSR.  With the live arrays of the minibatch
//             (bl_mp_layer_t.live_nodes: the rows of g_out that can be non-zero at all) the same chain over the live rows only:
//             N' nodes, E' + R' GEMM rows, a compact copy of their routing masks, sums into a zero-filled [N, Din]
//   forward, live form (bl_mp_layer_t.live_fwd; the decision is live_ok() below, made once per layer before forward and enforced
//             again at backward): the same chain over the rows the heads can reach -- pack the rows live_recv -> message GEMM over the
//             E' live messages into a compact `pre` -> segmented max + LayerNorm of the N' live nodes -> dense update of those rows.
//             Saved state and h_out are valid on the live rows only; backward of such a layer must take the live path
//   forward-only (saved == NULL): the same forward without any store that only a backward pass reads
// The caller owns every buffer: `saved` lives from forward to backward, `ws` only during the call
// (sizes from bl_mp_layer_saved_bytes / bl_mp_layer_workspace_bytes); nothing is allocated here except three
// HIP events per device (created once) used to fork / join the side stream.
#include <vector>

#include <string.h>

#include "bl_common.h"

// ---- per-kernel timing ----------------------------------------------------------------------------
namespace {
struct ProfRec {
  int kind;
  double flop;
  hipEvent_t e0, e1;
  bool overlapped;
  double bytes;
};
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_prof_pool;
const char* kProfNames[] = {"pack_rows",      "msg_gemm_x6",  "segment_max_ln", "dense_fwd",    "act_bwd",       "dense_wgrad",
                            "dense_dgrad",    "layernorm_bwd", "msg_wgrad_x6",   "msg_dgrad_x6", "node_grad_sums", "msg_dgrad_nodes",
                            "node_update_bwd", "msg_gemm_h3", "msg_wgrad_h3", "msg_dgrad_h3", "pack_gq_h3",
                            // the relational transformer block (csrc/bl_great_layer.hip; BL_PROF_GREAT_* in bl_common.h)
                            "linear_x6_epi", "linear_dgrad_x6", "gemm_wgrad_x6", "attn_probs_fwd", "attn_probs_bwd", "attn_rows_times",
                            "attn_transposed_times", "add_layernorm", "layernorm_bwd_branch",
                            // the run rows of bl_mp_layer_bwd: OR of the routing masks per run (bl_winbits_or_runs)
                            "winbits_or_runs",
                            // the live rows of bl_mp_layer_bwd: compact copy of the live messages' routing masks (bl_winbits_gather)
                            "winbits_gather_live",
                            // the live rows of bl_mp_layer_fwd: message -> row of the compact pre-activations, target ids of the live messages
                            "live_index_fwd"};
constexpr int kProfWinbitsOrRuns = 26;
constexpr int kProfWinbitsGatherLive = 27;
constexpr int kProfLiveIndexFwd = 28;
constexpr int kProfKinds = sizeof(kProfNames) / sizeof(kProfNames[0]);
static_assert(kProfLiveIndexFwd == kProfKinds - 1 && kProfWinbitsGatherLive == kProfKinds - 2 && kProfWinbitsOrRuns == kProfKinds - 3,
              "the kProf constants must index their names");

hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) {
    hipEvent_t e = g_prof_pool.back();
    g_prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

struct ProfScope {  // brackets the launches made while it is alive with two events on `st`
  hipStream_t st;
  bool on;
  ProfScope(int kind, double flop, hipStream_t s, bool overlapped) : st(s), on(g_prof_on) {
    if (!on) return;
    ProfRec r{kind, flop, prof_event(), prof_event(), overlapped, 0.0};
    (void)hipEventRecord(r.e0, st);
    g_prof.push_back(r);
  }
  ~ProfScope() {
    if (on) (void)hipEventRecord(g_prof.back().e1, st);
  }
};
}  // namespace

// the same for the other per-layer entry points of the library (declared in bl_common.h)
BlProfScope::BlProfScope(int kind, double flop, void* stream, double bytes, bool overlapped) : st(stream), on(g_prof_on) {
  if (!on) return;
  ProfRec r{kind, flop, prof_event(), prof_event(), overlapped, bytes};
  (void)hipEventRecord(r.e0, (hipStream_t)st);
  g_prof.push_back(r);
}
BlProfScope::~BlProfScope() {
  if (on) (void)hipEventRecord(g_prof.back().e1, (hipStream_t)st);
}

extern "C" int bl_prof_enable(int32_t on) {
  g_prof_on = on != 0;
  return BL_OK;
}
extern "C" int bl_prof_reset(void) {
  for (auto& r : g_prof) {
    g_prof_pool.push_back(r.e0);
    g_prof_pool.push_back(r.e1);
  }
  g_prof.clear();
  return BL_OK;
}
extern "C" int bl_prof_num_kinds(void) { return kProfKinds; }
extern "C" const char* bl_prof_kind_name(int32_t kind) { return kind >= 0 && kind < kProfKinds ? kProfNames[kind] : ""; }
// totals of one kind since the last reset; the caller must have synchronised the device
extern "C" int bl_prof_read(int32_t kind, double* ms, double* flop, int64_t* launches, int32_t* overlapped) {
  double t = 0, f = 0;
  int64_t n = 0;
  int ov = 0;
  for (auto& r : g_prof) {
    if (r.kind != kind) continue;
    float dt = 0.f;
    hipError_t e = hipEventElapsedTime(&dt, r.e0, r.e1);
    if (e != hipSuccess) {
      bl_set_error("bl_prof_read: %s (synchronise the device first)", hipGetErrorString(e));
      return (int)e;
    }
    t += dt;
    f += r.flop;
    ov |= r.overlapped ? 1 : 0;
    ++n;
  }
  if (ms) *ms = t;
  if (flop) *flop = f;
  if (launches) *launches = n;
  if (overlapped) *overlapped = ov;
  return BL_OK;
}
// algorithmic bytes the launches of a (memory-bound) kind were recorded with since the last reset (0 for the GEMM kinds)
extern "C" double bl_prof_read_bytes(int32_t kind) {
  double b = 0;
  for (auto& r : g_prof)
    if (r.kind == kind) b += r.bytes;
  return b;
}

// ---- buffer carving ---------------------------------------------------------------------------------
extern bool g_h3_one_term;  // csrc/bl_gemm_h3.hip: the f16x3 GEMMs evaluate the high-plane term only (mode 2)
namespace {
inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t packed_w_elems(int G, int K, int N) { return (size_t)G * ((N + 127) / 128) * (K / 32) * 12288; }

struct Saved {  // forward -> backward
  uint16_t* hp;      // [N, 3 Din]  packed layer input
  float* dact;       // [N, Dm]     message activation derivative at each winner (GELU only)
  uint32_t* bits;    // [E + R, Dm/32]  routing bitmask of the messages, then (backward fills them) of the R runs of the layer descriptor
  float* agg;        // [N, Dm]
  float* mean;       // [N]
  float* rstd;       // [N]
  float* ln_out;     // [N, Dm] fp32, or (dense node update as bf16x6) the bf16x3-packed form [N, 3 Dm] in the same region
  size_t bytes;
};
// (E counts the rows of the routing bitmask and nothing else: callers with run arrays pass E + R)
Saved carve_saved(void* base, int N, int E, int Din, int Dm, int msg_act) {
  Saved s;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += al(b); return q; };
  s.hp = (uint16_t*)take((size_t)N * 3 * Din * 2);
  s.dact = (float*)(msg_act == BL_ACT_NONE ? nullptr : take((size_t)N * Dm * 4));
  s.bits = (uint32_t*)take((size_t)E * (Dm / 32) * 4);
  s.agg = (float*)take((size_t)N * Dm * 4);
  s.mean = (float*)take((size_t)N * 4);
  s.rstd = (float*)take((size_t)N * 4);
  s.ln_out = (float*)take((size_t)N * Dm * 6);
  s.bytes = o;
  return s;
}
struct WsInfer {  // forward-only call (saved == NULL): the three buffers a forward pass cannot do without
  float* pre;      // [E, Dm]     pre-activations of the messages
  uint16_t* hp;    // [N, 3 Din]  packed layer input
  float* ln_out;   // [N, Dm] fp32 or its packed form [N, 3 Dm]
  size_t bytes;
};
WsInfer carve_infer(void* base, int N, int E, int Din, int Dm) {
  WsInfer w;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += al(b); return q; };
  w.pre = (float*)take((size_t)E * Dm * 4);
  w.hp = (uint16_t*)take((size_t)N * 3 * Din * 2);
  w.ln_out = (float*)take((size_t)N * Dm * 6);
  w.bytes = o;
  return w;
}
struct WsBwd {
  float* g_z;      // [N, Dout] fp32, or its bf16x3-packed form [N, 3 Dout] (same region)
  float* g_ln;     // [N, Dm]
  uint16_t* gqp;   // [N, 3 Dm] (bf16x3) or [N, 2 Dm] (f16x2)
  float* g_a;      // [E, 2 Din]; [E, Din] (source halves only) when the node sums are fused into the input gradient
  float* amax;     // f16x3 message GEMMs: max |gq| of this layer, on the device
  size_t bytes;
};
WsBwd carve_bwd(void* base, int N, int E, int Din, int Dm, int Dout, bool full_ga = true) {
  WsBwd w;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += al(b); return q; };
  w.g_z = (float*)take((size_t)N * Dout * 6);
  w.g_ln = (float*)take((size_t)N * Dm * 4);
  w.gqp = (uint16_t*)take((size_t)N * 3 * Dm * 2);
  w.g_a = (float*)take((size_t)E * (full_ga ? 2 : 1) * Din * 4);
  w.amax = (float*)take(256);
  w.bytes = o;
  return w;
}

// Message GEMMs (forward, weight gradient, routed input gradient) as f16x3 (csrc/bl_gemm_h3.hip: two fp16 planes per operand,
// three MFMA terms) instead of bf16x6.  The operands of the forward GEMM and the weight gradient's left operand are layer inputs
// and weights -- bounded tensors, fixed power-of-two scales BL_H3_ROW_SCALE / BL_H3_W_SCALE; the routed gradient operand gq has
// no bound known in advance: its amax is taken on the device and the scale derived from it there (no host round trip).  The
// dense node update stays on bf16x6 (its operands g_z / LayerNorm outputs are produced packed by fused kernels).
// Mode 2 ("f16x1", `train.py --amp`): the same packed images and kernels, high-plane term only (g_h3_one_term in bl_gemm_h3.hip) --
// fp16 operands, fp32 accumulation and fp32 results, the gradient operand scaled by its device-side amax (what a GradScaler is for).
int g_msg_h3 = -1;
bool msg_h3() {
  if (g_msg_h3 < 0) {
    const char* e = getenv("BL_MSG_GEMM");
    g_msg_h3 = (e && (e[0] == 'x' || e[0] == 'b')) ? 0 : ((e && (strcmp(e, "amp") == 0 || strcmp(e, "f16x1") == 0)) ? 2 : 1);  // "x6" / "bf16x6" -> 0; "amp" / "f16x1" -> 2; default f16x3
    g_h3_one_term = g_msg_h3 == 2;
  }
  return g_msg_h3 >= 1;
}

bool g_fused_node_bwd = true;  // bl_set_fused_node_bwd: act backward -> dense input gradient -> LayerNorm backward in one kernel

// bl_set_run_rows / BL_RUN_ROWS: the target halves of the routed f16x3 gradients once per run instead of once per message
int g_run_rows = -1;
bool run_rows_on() {
  if (g_run_rows < 0) {
    const char* e = getenv("BL_RUN_ROWS");
    g_run_rows = (e && e[0] == '0') ? 0 : 1;
  }
  return g_run_rows != 0;
}
// bl_set_live_backward / BL_LIVE_BWD: backward over the live rows of a descriptor that carries them (bl_mp_layer_t.live_nodes)
int g_live_bwd = -1;
bool live_bwd_on() {
  if (g_live_bwd < 0) {
    const char* e = getenv("BL_LIVE_BWD");
    g_live_bwd = (e && e[0] == '0') ? 0 : 1;
  }
  return g_live_bwd != 0;
}
// a descriptor carries the live arrays when all of them are there (the per-message ones may be NULL when no message is live)
inline bool layer_has_live(const bl_mp_layer_t* L) {
  if (!(L->live_nodes && L->live_num_nodes > 0 && L->live_num_nodes <= L->N && L->live_recv && L->live_num_recv > 0 && L->live_num_recv <= L->N &&
        L->live_num_msgs >= 0 && L->live_num_msgs <= L->E && L->live_num_runs >= 0 && L->live_num_runs <= L->live_num_msgs && L->live_group_ptr))
    return false;
  return L->live_num_msgs == 0 || (L->live_msgs && L->live_run_ptr && L->live_rows_tgt && L->live_rows_src && L->live_src_ptr &&
                                   L->live_src_msgs && L->live_run_csr_ptr && L->live_run_csr_rows);
}
// R of a descriptor that carries the run arrays (all of them), else 0; decides the rows of the routing bitmask in `saved`
inline int layer_runs(const bl_mp_layer_t* L) {
  return (L->num_runs > 0 && L->run_ptr && L->bwd_group_ptr && L->bwd_group_w && L->bwd_rows_tgt && L->bwd_rows_src && L->tgt_run_ptr &&
          L->tgt_run_rows) ? L->num_runs : 0;
}

// bl_set_live_forward / BL_LIVE_FWD: forward of the last layers over their live rows too (only where the live backward is on)
int g_live_fwd = -1;
bool live_fwd_on() {
  if (g_live_fwd < 0) {
    const char* e = getenv("BL_LIVE_FWD");
    g_live_fwd = (e && e[0] == '0') ? 0 : 1;
  }
  return g_live_fwd != 0;
}

// bytes of the live forward's scratch: compact pre [E', Dm] | msg_pos [E] (only the E' live entries are written and read) | tgt_id [E']
struct WsLiveFwd {
  float* pre;
  int32_t* msg_pos;
  int32_t* tgt_id;
  size_t bytes;
};
WsLiveFwd carve_live_fwd(void* base, int E, int Ex, int Dm) {
  WsLiveFwd w;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += al(b); return q; };
  w.pre = (float*)take((size_t)Ex * Dm * 4);
  w.msg_pos = (int32_t*)take((size_t)E * 4);
  w.tgt_id = (int32_t*)take((size_t)Ex * 4);
  w.bytes = o;
  return w;
}

// THE decision whether a layer runs over its live rows (bl_mp_layer_live_ok): asked before forward for the live forward, evaluated
// again by bl_mp_layer_bwd.  A layer whose forward ran live has valid saved state on its live rows only, so whatever is false here
// at backward after a live forward is an error there, never a fall-back.
//   have_w_bwd: the packed C = G . W^T image of the message weights will be / is handed to backward (not the Wt path)
//   forward:    also what the live FORWARD needs: its switch, no winner table, its scratch inside the forward workspace
bool live_ok(const bl_mp_layer_t* L, bool have_w_bwd, bool forward, bool want_winners, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  const int N = L->N, E = L->E, Din = L->Din, Dm = L->Dm, Dout = L->Dout;
#define LIVE_NEEDS(cond_, text_) \
  if (!(cond_)) { *why = text_; return false; }
  LIVE_NEEDS(live_bwd_on(), "the live backward is switched off (bl_set_live_backward / BL_LIVE_BWD)");
  LIVE_NEEDS(layer_has_live(L), "the descriptor carries no (complete) live arrays");
  LIVE_NEEDS(layer_runs(L) > 0 && E > 0 && run_rows_on(), "the run rows are off or the minibatch carries no run arrays");
  LIVE_NEEDS(msg_h3() && g_msg_h3 == 1, "the message GEMMs are not in the f16x3 three-term mode");
  LIVE_NEEDS(L->aggregation == BL_AGG_MAX, "the aggregation is not max");
  LIVE_NEEDS(have_w_bwd && !(L->Wt != nullptr && bl_routed_dgrad_vec_ok(Dm, 2 * Din)), "the input gradient takes the vector-unit (Wt) path");
  LIVE_NEEDS(Din % 128 == 0, "Din is not a multiple of 128");
  LIVE_NEEDS(L->Wd_packed != nullptr && Dm % 32 == 0 && Dout % 32 == 0, "the dense node update is not on the bf16x6 path");
  LIVE_NEEDS(g_fused_node_bwd && bl_node_update_bwd_ok(Dm, Dout), "the one-kernel node update backward does not apply (shape, switch or deterministic mode)");
  LIVE_NEEDS((uint64_t)N * (uint64_t)Dout < (1ull << 32) || L->drop.p <= 0.f, "the dropout counter of a node's own row leaves 32 bits");
  const size_t Ex = (size_t)L->live_num_msgs, Rx = (size_t)L->live_num_runs;
  LIVE_NEEDS(al((Ex + Rx) * Din * 4) + (Ex + Rx) * (Dm / 32) * 4 <= (size_t)E * 2 * Din * 4, "the compact gradient and masks do not fit the backward workspace");
  if (forward) {
    LIVE_NEEDS(live_fwd_on(), "the live forward is switched off (bl_set_live_forward / BL_LIVE_FWD)");
    LIVE_NEEDS(!want_winners, "a winner table is wanted");
    LIVE_NEEDS(carve_live_fwd(nullptr, E, (int)Ex, Dm).bytes <= al((size_t)E * Dm * 4), "the compact pre-activations and index arrays do not fit the forward workspace");
  }
#undef LIVE_NEEDS
  return true;
}

// msg_pos[live_msgs[i]] = i (row of message live_msgs[i] in the compact pre-activations), tgt_id[i] = msg_tgt[live_msgs[i]]
__global__ __launch_bounds__(256) void live_index_kernel(const int* __restrict__ live_msgs, const int* __restrict__ msg_tgt, int Ex, int E,
                                                         int* __restrict__ msg_pos, int* __restrict__ tgt_id) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= Ex) return;
  const int e = live_msgs[i];
  if ((unsigned)e >= (unsigned)E) return;  // (a malformed list must not write outside the region)
  msg_pos[e] = i;
  tgt_id[i] = msg_tgt[e];
}

// fork / join events of the side stream, one set per device (a process that drives several GPUs -- tests, tools -- must not
// record an event created on another device)
constexpr int kMaxDevices = 16;
struct SideEvents { hipEvent_t fork1 = nullptr, fork2 = nullptr, join = nullptr; };
SideEvents g_side_events[kMaxDevices];
SideEvents* ensure_events() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  SideEvents& e = g_side_events[dev];
  if (e.join) return &e;
  if (hipEventCreateWithFlags(&e.fork1, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e.fork2, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess)
    return nullptr;
  return &e;
}

inline int saved_act_code(const bl_mp_layer_t* L) {
  return (L->aggregation == BL_AGG_MEAN && L->msg_act == BL_ACT_NONE) ? BL_ACT_GELU_AGG : L->msg_act;
}

int check_layer(const bl_mp_layer_t* L, const char* who) {
  BL_CHECK_ARG(L && L->N > 0 && L->E >= 0 && L->T > 0, "%s: bad sizes", who);
  BL_CHECK_ARG(L->Din % 32 == 0 && L->Dm % 32 == 0 && L->Dout % 4 == 0 && L->Din > 0 && L->Dm > 0 && L->Dm <= 512 && L->Dout > 0,
               "%s: the fused layer needs Din, Dm multiples of 32 (bf16x6 GEMMs), Dm <= 512", who);
  // (a minibatch without messages has empty per-message arrays: PyTorch hands out NULL for those)
  BL_CHECK_ARG(L->type_ptr && L->tgt_ptr && L->src_ptr && (L->E == 0 || (L->msg_src && L->msg_tgt && L->tgt_msgs && L->src_msgs)),
               "%s: null graph index array", who);
  BL_CHECK_ARG(L->W && L->ln_g && L->ln_b && L->Wd && L->bd, "%s: null parameter", who);
  BL_CHECK_ARG(L->msg_act == BL_ACT_NONE || L->msg_act == BL_ACT_GELU || L->msg_act == BL_ACT_GELU_AGG,
               "%s: message activation must be none, gelu (per message) or gelu_agg (on the aggregate)", who);
  BL_CHECK_ARG(L->aggregation >= BL_AGG_MAX && L->aggregation <= BL_AGG_MEAN, "%s: aggregation must be BL_AGG_MAX, BL_AGG_SUM or BL_AGG_MEAN", who);
  BL_CHECK_ARG(L->num_runs >= 0 && L->num_runs <= L->E && (long long)L->E + L->num_runs <= 0x7fffffffLL, "%s: num_runs outside 0..E", who);
  BL_CHECK_ARG(L->aggregation == BL_AGG_MAX || L->msg_act != BL_ACT_GELU,
               "%s: sum / mean aggregation takes the activation on the aggregate (BL_ACT_GELU_AGG) or none: a per-message activation would need "
               "the [E, Dm] messages again in backward", who);
  return BL_OK;
}
}  // namespace

// A/B switch (tests, bench): 1 (default) = the node update's backward chain runs as bl_node_update_bwd where the shapes allow
// (Dm 128 / 256, dense node update on the bf16x6 path, deterministic mode off); 0 = three kernels.  Returns the previous value.
extern "C" int32_t bl_set_fused_node_bwd(int32_t on) {
  const int32_t prev = g_fused_node_bwd ? 1 : 0;
  g_fused_node_bwd = on != 0;
  return prev;
}

extern "C" int32_t bl_set_run_rows(int32_t on) {
  const int32_t prev = run_rows_on() ? 1 : 0;
  g_run_rows = on != 0 ? 1 : 0;
  return prev;
}

extern "C" int32_t bl_set_live_backward(int32_t on) {
  const int32_t prev = live_bwd_on() ? 1 : 0;
  g_live_bwd = on != 0 ? 1 : 0;
  return prev;
}

extern "C" int32_t bl_get_live_backward(void) { return live_bwd_on() ? 1 : 0; }

extern "C" int32_t bl_set_live_forward(int32_t on) {
  const int32_t prev = live_fwd_on() ? 1 : 0;
  g_live_fwd = on != 0 ? 1 : 0;
  return prev;
}

extern "C" int32_t bl_get_live_forward(void) { return live_fwd_on() ? 1 : 0; }

extern "C" int32_t bl_mp_layer_live_ok(const bl_mp_layer_t* L, int32_t have_w_packed_bwd, int32_t forward, int32_t want_winners) {
  if (L == nullptr || check_layer(L, "bl_mp_layer_live_ok") != BL_OK) return 0;
  const char* why = nullptr;
  const bool ok = live_ok(L, have_w_packed_bwd != 0, forward != 0, want_winners != 0, &why);
  if (!ok) bl_set_error("bl_mp_layer_live_ok: %s", why);  // (a reason to read, not a failure: the caller runs the full form)
  return ok ? 1 : 0;
}

extern "C" int64_t bl_mp_layer_saved_bytes(int32_t N, int32_t E, int32_t Din, int32_t Dm, int32_t msg_act) {
  return (int64_t)carve_saved(nullptr, N, E, Din, Dm, msg_act).bytes;
}
// forward scratch: the [E, Dm] pre-activations; backward scratch: g_z, g_ln, packed node gradient, [E, 2 Din] input gradients
extern "C" int64_t bl_mp_layer_workspace_bytes(int32_t N, int32_t E, int32_t Din, int32_t Dm, int32_t Dout, int32_t backward) {
  if (backward == 3) return (int64_t)carve_infer(nullptr, N, E, Din, Dm).bytes;
  if (backward) return (int64_t)carve_bwd(nullptr, N, E, Din, Dm, Dout, backward != 2).bytes;
  return (int64_t)al((size_t)E * Dm * 4);
}
// Which image of the per-type weights a layer call expects: 1 = bl_pack_weights_x6w (the wide row GEMM takes this shape:
// message GEMM N = Dm, K = 2 Din; input-gradient GEMM N = 2 Din, K = Dm), 0 = bl_pack_weights_x6.
extern "C" int32_t bl_mp_layer_weight_image(int32_t Din, int32_t Dm, int32_t for_backward) {
  if (msg_h3()) return 2;  // bl_pack_weights_h3 (kinds 5 / 6 of bl_pack_weights_multi)
  return for_backward ? bl_gemm_rows_x6w_ok(2 * Din, Dm) : bl_gemm_rows_x6w_ok(Dm, 2 * Din);
}
extern "C" int32_t bl_set_msg_gemm_mode(int32_t mode) {
  (void)msg_h3();
  const int32_t prev = g_msg_h3;
  g_msg_h3 = mode == 2 ? 2 : (mode ? 1 : 0);
  g_h3_one_term = g_msg_h3 == 2;
  return prev;
}
extern "C" int32_t bl_get_msg_gemm_mode(void) {
  (void)msg_h3();
  return g_msg_h3;
}

extern "C" int64_t bl_mp_layer_packed_weight_elems(int32_t T, int32_t Din, int32_t Dm, int32_t for_backward) {
  if (msg_h3()) return for_backward ? bl_packed_weight_elems_h3(T, Dm, 2 * Din) : bl_packed_weight_elems_h3(T, 2 * Din, Dm);
  if (bl_mp_layer_weight_image(Din, Dm, for_backward))
    return for_backward ? bl_packed_weight_elems_x6w(T, Dm, 2 * Din) : bl_packed_weight_elems_x6w(T, 2 * Din, Dm);
  return (int64_t)(for_backward ? packed_w_elems(T, Dm, 2 * Din) : packed_w_elems(T, 2 * Din, Dm));
}

#define BL_TRY(call_)        \
  do {                       \
    int rc_ = (call_);       \
    if (rc_ != BL_OK) return rc_; \
  } while (0)

extern "C" int bl_mp_layer_fwd(const bl_mp_layer_t* L, const float* h_lo, int32_t ld_lo, int32_t width_lo, const float* h_hi,
                               int32_t ld_hi, const uint16_t* w_packed, float* h_out, int32_t* winner_out, void* saved,
                               void* ws, void* stream) {
  BL_TRY(check_layer(L, "bl_mp_layer_fwd"));
  const int N = L->N, E = L->E, T = L->T, Din = L->Din, Dm = L->Dm, Dout = L->Dout;
  // saved == NULL: forward-only call (model.predict, evaluate.py) -- nothing is kept for a backward pass: no routing bitmask, no
  // activation derivative, no aggregate / mean / rstd stores; the packed input and the LayerNorm output live in `ws`
  const bool infer = saved == nullptr;
  BL_CHECK_ARG(h_lo && w_packed && h_out && (ws || (E == 0 && !infer)), "bl_mp_layer_fwd: null buffer");
  BL_CHECK_ARG((h_hi == nullptr && width_lo == Din) || (h_hi != nullptr && width_lo > 0 && width_lo < Din && width_lo % 32 == 0),
               "bl_mp_layer_fwd: width_lo must be Din (one source) or a multiple of 32 below Din (two sources)");
  hipStream_t st = (hipStream_t)stream;
  // node_order lists the hubs first and the other nodes in natural order: without hubs it is the identity, and the per-node
  // kernels skip the load (one dependent round trip less per wave)
  const int32_t* node_order = L->num_hub_slots == 0 ? nullptr : L->node_order;
  // ("mean" without an activation still needs the [N, Dm] derivative array: it carries the 1 / in-degree)
  Saved S = carve_saved(saved, N, E + layer_runs(L), Din, Dm, saved_act_code(L));
  float* pre = (float*)ws;
  if (infer) {
    const WsInfer I = carve_infer(ws, N, E, Din, Dm);
    pre = I.pre;
    S.hp = I.hp;
    S.ln_out = I.ln_out;
    S.dact = nullptr; S.bits = nullptr; S.agg = nullptr; S.mean = nullptr; S.rstd = nullptr;
  }
  const bool h3 = msg_h3();
  if (L->live_fwd) {
    // Live rows, forward: the caller (GraphNeuralNetwork.forward, after bl_mp_layer_live_ok) states that nothing reads h_out outside
    // the rows live_nodes -- the layer above, live as well, reads its live_recv = these live_nodes, the heads gather a subset of the
    // last layer's -- and that the input is valid at least on the rows live_recv.  Every buffer keeps its whole-problem layout
    // (saved state by node / message id, h_out by node id), so bl_mp_layer_bwd's live path reads it unchanged; only `pre` is compact.
    const char* why = nullptr;
    if (infer || !live_ok(L, true, true, winner_out != nullptr, &why)) {
      bl_set_error("bl_mp_layer_fwd: live_fwd is set but the layer cannot run over its live rows: %s", infer ? "forward-only call (saved == NULL)" : why);
      return BL_EINVAL;
    }
    const int Nx = L->live_num_nodes, Nr = L->live_num_recv, Ex = L->live_num_msgs;
    const WsLiveFwd V = carve_live_fwd(ws, E, Ex, Dm);
    if (L->live_fwd == BL_LIVE_FWD_LAST &&  // the output handed out as the encoder's: no caller ever sees a row nobody computed
        hipMemsetAsync(h_out, 0, (size_t)N * Dout * 4, st) != hipSuccess) {
      bl_set_error("bl_mp_layer_fwd: memset failed");
      return BL_EINVAL;
    }
    if (Ex > 0) {
      ProfScope ps(kProfLiveIndexFwd, 0.0, st, false);
      hipLaunchKernelGGL(live_index_kernel, dim3((unsigned)((Ex + 255) / 256)), dim3(256), 0, st, L->live_msgs, L->msg_tgt, Ex, E, V.msg_pos, V.tgt_id);
      BL_LAUNCH_CHECK("bl_mp_layer_fwd (live index)");
    }
    {  // rows outside the previous layer's live set were never computed: only the rows live_recv are read and packed
      ProfScope ps(0, 0.0, st, false);
      BL_TRY(bl_pack_f16x2_rows(h_lo, ld_lo, L->live_recv, Nr, h_hi ? width_lo : Din, Din, 0, BL_H3_ROW_SCALE, S.hp, st));
      if (h_hi) BL_TRY(bl_pack_f16x2_rows(h_hi, ld_hi, L->live_recv, Nr, Din - width_lo, Din, width_lo, BL_H3_ROW_SCALE, S.hp, st));
    }
    if (Ex > 0) {  // the live messages keep their order (type-major): the first T + 1 entries of live_group_ptr are their type ranges
      bl_rows_packed_t a;
      a.xp[0] = S.hp; a.xp[1] = S.hp; a.xp[2] = nullptr;
      a.idx[0] = L->live_rows_src; a.idx[1] = V.tgt_id; a.idx[2] = nullptr;
      a.width[0] = Din; a.width[1] = Din; a.width[2] = 0;
      a.nsrc = 2;
      ProfScope ps(13, 2.0 * Ex * (2.0 * Din) * Dm, st, false);
      BL_TRY(bl_gemm_rows_h3(&a, nullptr, 0, w_packed, bl_packed_weight_elems_h3(1, 2 * Din, Dm), L->live_group_ptr, nullptr, T, Ex, Dm, 2 * Din,
                             1.0f / (BL_H3_ROW_SCALE * BL_H3_W_SCALE), nullptr, V.pre, Dm, st));
    }
    {  // every message into a live node is live: the full target CSR, the segments live_nodes, the items' rows through msg_pos
      ProfScope ps(2, 0.0, st, false);
      BL_TRY(bl_segment_max_fwd_impl(V.pre, Dm, L->tgt_ptr, L->tgt_msgs, Nx, Dm, L->msg_act, S.agg, nullptr, L->ln_g, L->ln_b, L->ln_eps, nullptr,
                                     S.mean, S.rstd, S.dact, S.bits, L->live_nodes, (uint16_t*)S.ln_out, 0, st, V.msg_pos, Ex));
    }
    {
      ProfScope ps(3, 2.0 * Nx * (double)Dm * Dout, st, false);
      bl_rows_packed_t d;
      d.xp[0] = (const uint16_t*)S.ln_out; d.xp[1] = d.xp[2] = nullptr; d.idx[0] = L->live_nodes; d.idx[1] = d.idx[2] = nullptr;
      d.width[0] = Dm; d.width[1] = d.width[2] = 0; d.nsrc = 1;
      BL_TRY(bl_gemm_rows_x6_epi_rows(&d, L->Wd_packed, Nx, Dout, Dm, L->bd, BL_ACT_TANH, L->drop, L->live_nodes, N, h_out, Dout, st));
    }
    return BL_OK;
  }
  if (h3) {
    ProfScope ps(0, 0.0, st, false);
    BL_TRY(bl_pack_f16x2(h_lo, ld_lo, N, h_hi ? width_lo : Din, Din, 0, BL_H3_ROW_SCALE, nullptr, S.hp, st));
    if (h_hi) BL_TRY(bl_pack_f16x2(h_hi, ld_hi, N, Din - width_lo, Din, width_lo, BL_H3_ROW_SCALE, nullptr, S.hp, st));
  } else {
    ProfScope ps(0, 0.0, st, false);
    if (h_hi == nullptr) {
      BL_TRY(bl_pack_bf16x3(h_lo, ld_lo, N, Din, S.hp, st));
    } else {
      BL_TRY(bl_pack_bf16x3_cols(h_lo, ld_lo, N, width_lo, Din, 0, S.hp, st));
      BL_TRY(bl_pack_bf16x3_cols(h_hi, ld_hi, N, Din - width_lo, Din, width_lo, S.hp, st));
    }
  }
  bl_rows_packed_t a;
  a.xp[0] = S.hp; a.xp[1] = S.hp; a.xp[2] = nullptr;
  a.idx[0] = L->msg_src; a.idx[1] = L->msg_tgt; a.idx[2] = nullptr;
  a.width[0] = Din; a.width[1] = Din; a.width[2] = 0;
  a.nsrc = 2;
  if (h3) {
    ProfScope ps(13, 2.0 * E * (2.0 * Din) * Dm, st, false);
    BL_TRY(bl_gemm_rows_h3(&a, nullptr, 0, w_packed, bl_packed_weight_elems_h3(1, 2 * Din, Dm), L->type_ptr, nullptr, T, E, Dm, 2 * Din,
                           1.0f / (BL_H3_ROW_SCALE * BL_H3_W_SCALE), nullptr, pre, Dm, st));
  } else {
    ProfScope ps(1, 2.0 * E * (2.0 * Din) * Dm, st, false);
    if (bl_mp_layer_weight_image(Din, Dm, 0))  // >= 256 output columns: the wide (128 x 256 tile, LDS-DMA) form, bit-identical
      BL_TRY(bl_gemm_rows_x6w(&a, nullptr, 0, w_packed, bl_packed_weight_elems_x6w(1, 2 * Din, Dm), L->type_ptr, nullptr, T, E, Dm,
                              2 * Din, pre, Dm, st));
    else
      BL_TRY(bl_gemm_rows_x6(&a, nullptr, 0, w_packed, (int64_t)packed_w_elems(1, 2 * Din, Dm), L->type_ptr, nullptr, T, E, Dm,
                             2 * Din, pre, Dm, st));
  }
  // dense node update on the bf16x6 path when the caller packed Wd (bl_pack_weights_x6(Wd, 1, Dm, Dout, w_is_kn = 1)): the
  // LayerNorm epilogue of the segmented max then emits its result in packed form and no fp32 copy is kept
  const bool dense_x6 = L->Wd_packed != nullptr && Dm % 32 == 0 && Dout % 32 == 0;
  {
    ProfScope ps(2, 0.0, st, false);
    // (E == 0: every segment is empty and the kernel never dereferences `pre`)
    if (L->aggregation != BL_AGG_MAX)  // ptgnn's "sum" / "mean" (no winners: winner_out is left untouched)
      BL_TRY(bl_segment_sum_fwd_impl(pre, Dm, L->tgt_ptr, L->tgt_msgs, N, Dm, L->msg_act, L->aggregation == BL_AGG_MEAN, S.agg, L->ln_g, L->ln_b,
                                     L->ln_eps, dense_x6 ? nullptr : S.ln_out, S.mean, S.rstd, S.dact, node_order,
                                     dense_x6 ? (uint16_t*)S.ln_out : nullptr, st));
    else
    BL_TRY(bl_segment_max_fwd_impl(pre, Dm, L->tgt_ptr, L->tgt_msgs, N, Dm, L->msg_act, S.agg, winner_out, L->ln_g, L->ln_b,
                                   L->ln_eps, dense_x6 ? nullptr : S.ln_out, S.mean, S.rstd, S.dact, S.bits, node_order,
                                   dense_x6 ? (uint16_t*)S.ln_out : nullptr, L->num_hub_slots, st));
  }
  {
    ProfScope ps(3, 2.0 * N * (double)Dm * Dout, st, false);
    if (dense_x6) {
      bl_rows_packed_t d;
      d.xp[0] = (const uint16_t*)S.ln_out; d.xp[1] = d.xp[2] = nullptr; d.idx[0] = d.idx[1] = d.idx[2] = nullptr;
      d.width[0] = Dm; d.width[1] = d.width[2] = 0; d.nsrc = 1;
      BL_TRY(bl_gemm_rows_x6_epi(&d, L->Wd_packed, 0, nullptr, nullptr, 1, N, Dout, Dm, L->bd, BL_ACT_TANH, L->drop, h_out, Dout, st));
    } else {
      bl_rows_t d;
      d.x[0] = S.ln_out; d.idx[0] = nullptr; d.ld[0] = Dm; d.width[0] = Dm; d.nsrc = 1;
      d.x[1] = d.x[2] = nullptr; d.idx[1] = d.idx[2] = nullptr; d.ld[1] = d.ld[2] = 0; d.width[1] = d.width[2] = 0;
      BL_TRY(bl_gemm_rows(&d, L->Wd, 0, Dout, 0, L->bd, nullptr, nullptr, 1, N, Dout, Dm, BL_ACT_TANH, L->drop, h_out, Dout, st));
    }
  }
  return BL_OK;
}

extern "C" int bl_mp_layer_bwd(const bl_mp_layer_t* L, const float* h_out, const float* g_out, const uint16_t* w_packed_bwd,
                               const void* saved, void* ws, float* g_h_lo, int32_t ld_lo, int32_t width_lo, float* g_h_hi,
                               int32_t ld_hi, float* g_W, float* g_ln_g, float* g_ln_b, float* g_Wd, float* g_bd,
                               void* stream, void* side_stream, int32_t join_side) {
  BL_TRY(check_layer(L, "bl_mp_layer_bwd"));
  const int N = L->N, E = L->E, T = L->T, Din = L->Din, Dm = L->Dm, Dout = L->Dout;
  BL_CHECK_ARG(h_out && g_out && saved && ws && g_h_lo && g_W && g_ln_g && g_ln_b && g_Wd && g_bd, "bl_mp_layer_bwd: null buffer");
  BL_CHECK_ARG(w_packed_bwd || (L->Wt && L->E > 0 && bl_routed_dgrad_vec_ok(L->Dm, 2 * L->Din)) || L->E == 0,
               "bl_mp_layer_bwd: w_packed_bwd may only be NULL when the input gradient takes the Wt path");
  BL_CHECK_ARG((g_h_hi == nullptr && width_lo == Din) || (g_h_hi != nullptr && width_lo > 0 && width_lo < Din),
               "bl_mp_layer_bwd: width_lo must be Din (one output) or below Din (two outputs)");
  hipStream_t st = (hipStream_t)stream, side = side_stream ? (hipStream_t)side_stream : st;
  const int32_t* node_order = L->num_hub_slots == 0 ? nullptr : L->node_order;  // (identity without hubs: see bl_mp_layer_fwd)
  const bool two = side != st;
  SideEvents* ev = two ? ensure_events() : nullptr;
  if (two) BL_CHECK_ARG(ev != nullptr, "bl_mp_layer_bwd: cannot create HIP events");
  const int R = layer_runs(L);
  Saved S = carve_saved(const_cast<void*>(saved), N, E + R, Din, Dm, saved_act_code(L));
  const uint32_t* bits = L->aggregation == BL_AGG_MAX ? S.bits : nullptr;  // sum / mean: every message receives its target's gradient
  // the input gradient from the non-zeros of the routed message gradient (vector units) when the caller supplied W^T and
  // W[t]^T fits one LDS block; node sums fused in (atomics) unless the deterministic mode asks for a fixed summation order
  const bool vec_dgrad = L->Wt != nullptr && E > 0 && bl_routed_dgrad_vec_ok(Dm, 2 * Din) && L->aggregation == BL_AGG_MAX;
  const bool fused_sums = vec_dgrad && !bl_get_deterministic();
  // Run rows: the target halves of the routed input and weight gradients as one GEMM row per run (the masks of a run's members are
  // disjoint, their target halves are summed anyway) -- E + R rows of Din columns instead of E rows of 2 Din.  f16x3 with max
  // aggregation on the matrix cores; Din a multiple of 128 because the backward weight image of [T] groups x 2 Din columns, read
  // with half the group stride, then IS the image of [2 T] groups x Din columns (blocks are ordered [column tile][stage] in a group)
  const bool run_rows = R > 0 && E > 0 && run_rows_on() && msg_h3() && g_msg_h3 == 1 && !vec_dgrad && L->aggregation == BL_AGG_MAX &&
                        Din % 128 == 0 && w_packed_bwd != nullptr;
  WsBwd B = carve_bwd(ws, N, E, Din, Dm, Dout, !fused_sums);

  // dense node update on the bf16x6 path: forward must have run with Wd_packed too (it decides the form of `saved`)
  const bool dense_x6 = L->Wd_packed != nullptr && L->Wd_packed_bwd != nullptr && Dm % 32 == 0 && Dout % 32 == 0;
  BL_CHECK_ARG(dense_x6 || L->Wd_packed == nullptr, "bl_mp_layer_bwd: Wd_packed given without Wd_packed_bwd");
  // act backward -> dense input gradient -> LayerNorm backward x activation derivative in ONE kernel (csrc/bl_node_bwd.hip)
  const bool fused_node = dense_x6 && g_fused_node_bwd && bl_node_update_bwd_ok(Dm, Dout);
  // Live rows: the caller states that g_out is zero outside the rows live_nodes (the heads read the encoder's output through one
  // gather of a few rows, and a layer's input can receive a gradient only at its live rows and at the sources of the messages
  // into them).  Rows with a zero gradient contribute additions of zero to every result, so the whole chain runs over the N' live
  // nodes and the E' messages / R' runs into them: the node update's backward reads its rows through live_nodes and writes g_z and
  // gq compact, the GEMMs see an ordinary smaller problem (operand rows gathered by global node id, gq rows by position in
  // live_nodes, a compact copy of the routing masks), the segmented sums write the rows live_recv of a zero-filled [N, Din].
  // THE place where a layer's backward takes this form: whatever the run rows and the one-kernel node update exclude (bf16x6 and
  // f16x1, sum / mean, the deterministic mode, Din not a multiple of 128, the vector-unit input gradient) keeps the full backward.
  const int Ex = L->live_num_msgs, Rx = L->live_num_runs;
  const size_t live_ga_bytes = al(((size_t)Ex + Rx) * Din * 4);
  // (the conditions are live_ok()'s, the same function the caller asked before a live FORWARD)
  const char* why_not = "the run-row path or the one-kernel node update does not apply";
  const bool live = run_rows && fused_node && live_ok(L, w_packed_bwd != nullptr, false, false, &why_not);
  if (L->live_fwd && !live) {  // forward left the saved state valid on the live rows only: the full backward would read garbage
    bl_set_error("bl_mp_layer_bwd: this layer's forward ran over its live rows, but backward cannot take the live path: %s (a switch "
                 "was changed between forward and backward?)", why_not);
    return BL_EINVAL;
  }
  const int Nn = live ? L->live_num_nodes : N;  // rows of the node update's backward and of everything it writes
  uint32_t* live_bits = live ? (uint32_t*)((char*)B.g_a + live_ga_bytes) : nullptr;
  // f16x3 message GEMMs: gq leaves its producer in fp32 (B.g_ln); its packed form is made below, once its amax is known
  const bool h3 = msg_h3();
  if (h3 && E > 0 && hipMemsetAsync(B.amax, 0, 4, st) != hipSuccess) { bl_set_error("bl_mp_layer_bwd: memset failed"); return BL_EINVAL; }
  if (fused_node) {
    ProfScope ps(12, 2.0 * Nn * (double)Dm * Dout, st, false);
    BL_TRY(bl_node_update_bwd_impl(g_out, h_out, Nn, Dout, L->drop, L->Wd_packed_bwd, S.agg, S.mean, S.rstd, L->ln_g, S.dact, Dm,
                                   (uint16_t*)B.g_z, g_bd, (vec_dgrad || h3) ? B.g_ln : nullptr, h3 ? nullptr : B.gqp, g_ln_g, g_ln_b,
                                   (h3 && E > 0) ? B.amax : nullptr, live ? L->live_nodes : nullptr, st));
  } else {  // y = drop(tanh(z)): g_z (packed for the bf16x6 GEMMs), bias gradient
    ProfScope ps(4, 0.0, st, false);
    BL_TRY(bl_act_bwd_impl(g_out, h_out, N, Dout, Dout, BL_ACT_TANH, L->drop, dense_x6 ? nullptr : B.g_z, g_bd,
                           dense_x6 ? (uint16_t*)B.g_z : nullptr, st));
  }
  bl_rows_t r1;
  r1.x[1] = r1.x[2] = nullptr; r1.idx[0] = r1.idx[1] = r1.idx[2] = nullptr; r1.ld[1] = r1.ld[2] = 0; r1.width[1] = r1.width[2] = 0; r1.nsrc = 1;
  bl_rows_packed_t p1;
  p1.xp[1] = p1.xp[2] = nullptr; p1.idx[0] = p1.idx[1] = p1.idx[2] = nullptr; p1.width[1] = p1.width[2] = 0; p1.nsrc = 1;
  if (two) {
    (void)hipEventRecord(ev->fork1, st);
    (void)hipStreamWaitEvent(side, ev->fork1, 0);
  }
  {  // dense weight gradient, next to the input-gradient chain
    ProfScope ps(5, 2.0 * Nn * (double)Dm * Dout, side, two);
    if (dense_x6) {  // (live: the compact g_z against the LayerNorm outputs of the live nodes)
      p1.xp[0] = (const uint16_t*)S.ln_out; p1.width[0] = Dm; p1.idx[0] = live ? L->live_nodes : nullptr;
      BL_TRY(bl_gemm_wgrad_x6(&p1, (const uint16_t*)B.g_z, nullptr, nullptr, nullptr, 1, Nn, Dout, Dm, g_Wd, 0, Dout, side));
      p1.idx[0] = nullptr;
    } else {
      r1.x[0] = S.ln_out; r1.ld[0] = Dm; r1.width[0] = Dm;
      BL_TRY(bl_gemm_wgrad(&r1, B.g_z, Dout, nullptr, nullptr, 1, N, Dout, Dm, g_Wd, 0, Dout, side));
    }
  }
  if (!fused_node) {
    ProfScope ps(6, 2.0 * N * (double)Dm * Dout, st, two);
    if (dense_x6) {
      p1.xp[0] = (const uint16_t*)B.g_z; p1.width[0] = Dout;
      // (the epilogue form with nothing in it: a kernel instantiation of its own, so that per-kernel profiles do not mix
      // this small GEMM with the message GEMM's launches)
      bl_dropout_t nodrop = {0.f, 0u, 0u};
      BL_TRY(bl_gemm_rows_x6_epi(&p1, L->Wd_packed_bwd, 0, nullptr, nullptr, 1, N, Dm, Dout, nullptr, BL_ACT_NONE, nodrop, B.g_ln, Dm, st));
    } else {
      r1.x[0] = B.g_z; r1.ld[0] = Dout; r1.width[0] = Dout;
      bl_dropout_t nodrop = {0.f, 0u, 0u};
      BL_TRY(bl_gemm_rows(&r1, L->Wd, 0, Dout, 1, nullptr, nullptr, nullptr, 1, N, Dm, Dout, BL_ACT_NONE, nodrop, B.g_ln, Dm, st));
    }
  }
  if (!fused_node) {  // LayerNorm backward x activation derivative at the winners -> packed d loss / d (winning pre-activation)
    ProfScope ps(7, 0.0, st, two);
    // (the fp32 form of the result, for the vector input gradient, overwrites g_ln in place: the kernel is row-local)
    BL_TRY(bl_layernorm_bwd(B.g_ln, S.agg, S.mean, S.rstd, L->ln_g, N, Dm, (vec_dgrad || h3) ? B.g_ln : nullptr, g_ln_g, g_ln_b, S.dact,
                            h3 ? nullptr : B.gqp, st));
  }
  if (h3 && E > 0) {  // amax of gq on the device -> its power-of-two scale -> two fp16 planes
    ProfScope ps(16, 0.0, st, two);
    if (!fused_node) BL_TRY(bl_amax(B.g_ln, (int64_t)N * Dm, B.amax, st));  // (the fused node-update backward took it on the way)
    BL_TRY(bl_pack_f16x2(B.g_ln, Dm, Nn, Dm, Dm, 0, 1.0f, B.amax, B.gqp, st));  // (rows of zeros left out do not change the amax)
  }
  if (live && Ex > 0) {
    ProfScope ps(kProfWinbitsGatherLive, 0.0, st, two);
    BL_TRY(bl_winbits_gather(S.bits, Dm / 32, E, L->live_msgs, Ex, Dm / 32, live_bits, Dm / 32, st));
  }
  if (live) {
    if (Ex > 0) {
      ProfScope ps(kProfWinbitsOrRuns, 0.0, st, two);
      BL_TRY(bl_winbits_or_runs(live_bits, Dm / 32, L->live_run_ptr, Ex, Rx, Dm / 32, st));
    }
  } else if (run_rows) {  // (before the weight-gradient fork: both GEMMs read the runs' masks)
    ProfScope ps(kProfWinbitsOrRuns, 0.0, st, two);
    BL_TRY(bl_winbits_or_runs(S.bits, Dm / 32, L->run_ptr, E, R, Dm / 32, st));
  }
  // the row space of the two routed GEMMs on the run-row path: the minibatch's E + R rows, or the E' + R' live ones
  const int rr_rows = live ? Ex + Rx : E + R;
  const int32_t* rr_group_ptr = live ? L->live_group_ptr : L->bwd_group_ptr;
  const int32_t* rr_rows_tgt = live ? L->live_rows_tgt : L->bwd_rows_tgt;  // live: positions in live_nodes (gq is compact)
  const int32_t* rr_rows_src = live ? L->live_rows_src : L->bwd_rows_src;  // node ids either way (the packed layer input is whole)
  const uint32_t* rr_bits = live ? live_bits : bits;
  // The routed weight gradient (side stream) reads what is ready at this point: the packed layer input, the packed gradient operand, the
  // routing bits.  WHEN it is forked decides what it runs next to.  Layers up to 128 wide: here, side by side with the routed input
  // gradient.  Wider layers (the hidden-256 configurations): behind the segmented sums, i.e. next to the bandwidth-bound tail of this layer
  // and the head of the next one -- measured on one box, two interleaved pairs (tools/experiments/fork_probe.sh,
  // profiles/r06zzn_fork_probe.log): c3 shard 1 664 / 1 660 -> 1 684 / 1 692 graphs/s with the late fork, c2 4 917 / 4 942 -> 4 904 / 4 911
  // (and 4 768 / 4 774 when forked between the input gradient and the sums).
  const bool late_fork = two && Dout >= 256;
  auto launch_wgrad = [&]() -> int {
    bl_rows_packed_t a;
    a.xp[0] = S.hp; a.xp[1] = S.hp; a.xp[2] = nullptr;
    a.idx[0] = L->msg_src; a.idx[1] = L->msg_tgt; a.idx[2] = nullptr;
    a.width[0] = Din; a.width[1] = Din; a.width[2] = 0;
    a.nsrc = 2;
    if (two) {
      (void)hipEventRecord(ev->fork2, st);
      (void)hipStreamWaitEvent(side, ev->fork2, 0);
    }
    if (run_rows) {  // one source: the message rows gather h[src], the run rows h[tgt]; gW viewed as [2 T, Din, Dm]
      ProfScope ps(14, 2.0 * (double)rr_rows * Din * Dm, side, two);
      a.idx[0] = rr_rows_src; a.xp[1] = nullptr; a.idx[1] = nullptr; a.width[1] = 0;
      a.nsrc = 1;
      BL_TRY(bl_gemm_wgrad_h3_impl(&a, B.gqp, rr_rows_tgt, rr_bits, Dm / 32, rr_group_ptr, L->bwd_group_w, 2 * T, rr_rows, Dm, Din,
                                   1.0f / BL_H3_ROW_SCALE, B.amax, g_W, (int64_t)Din * Dm, Dm, true, side));
    } else if (h3) {
      ProfScope ps(14, 2.0 * E * (2.0 * Din) * Dm, side, two);
      BL_TRY(bl_gemm_wgrad_h3(&a, B.gqp, L->msg_tgt, bits, Dm / 32, L->type_ptr, nullptr, T, E, Dm, 2 * Din, 1.0f / BL_H3_ROW_SCALE, B.amax,
                              g_W, (int64_t)2 * Din * Dm, Dm, side));
    } else {
      ProfScope ps(8, 2.0 * E * (2.0 * Din) * Dm, side, two);
      if (bits)
        BL_TRY(bl_gemm_wgrad_routed_x6(&a, B.gqp, L->msg_tgt, bits, Dm / 32, L->type_ptr, nullptr, T, E, Dm, 2 * Din, g_W,
                                       (int64_t)2 * Din * Dm, Dm, side));
      else
        BL_TRY(bl_gemm_wgrad_x6(&a, B.gqp, L->msg_tgt, L->type_ptr, nullptr, T, E, Dm, 2 * Din, g_W, (int64_t)2 * Din * Dm, Dm, side));
    }
    return BL_OK;
  };
  const bool msgs = E > 0 && !(live && Ex == 0);  // (no live message: nothing reaches W or the layer input)
  if (msgs) {
    if (!late_fork) BL_TRY(launch_wgrad());
    bl_rows_packed_t g;
    g.xp[0] = B.gqp; g.xp[1] = g.xp[2] = nullptr; g.idx[0] = L->msg_tgt; g.idx[1] = g.idx[2] = nullptr;
    g.width[0] = Dm; g.width[1] = g.width[2] = 0; g.nsrc = 1;
    if (fused_sums) {
      ProfScope ps(11, 2.0 * N * (2.0 * Din) * Dm, st, two);  // FLOPs of the non-zeros: one winner per (node, channel)
      const int split = g_h_hi ? width_lo : Din;
      if (ld_lo == split) {
        if (hipMemsetAsync(g_h_lo, 0, (size_t)N * split * 4, st) != hipSuccess) { bl_set_error("bl_mp_layer_bwd: memset failed"); return BL_EINVAL; }
      } else if (hipMemset2DAsync(g_h_lo, (size_t)ld_lo * 4, 0, (size_t)split * 4, N, st) != hipSuccess) { bl_set_error("bl_mp_layer_bwd: memset failed"); return BL_EINVAL; }
      if (g_h_hi) {
        if (ld_hi == Din - split) {
          if (hipMemsetAsync(g_h_hi, 0, (size_t)N * (Din - split) * 4, st) != hipSuccess) { bl_set_error("bl_mp_layer_bwd: memset failed"); return BL_EINVAL; }
        } else if (hipMemset2DAsync(g_h_hi, (size_t)ld_hi * 4, 0, (size_t)(Din - split) * 4, N, st) != hipSuccess) { bl_set_error("bl_mp_layer_bwd: memset failed"); return BL_EINVAL; }
      }
      // target halves by atomics (one per run of equal targets), source halves as rows + a segmented sum over the source CSR:
      // all-atomic, the kernel is bound by the L2's one fp32 atomic per channel per clock (0.475 vs 0.404 ms at c2's layer shape;
      // tools/dgrad_bench.py times both forms through bl_routed_dgrad_nodes / bl_routed_dgrad_nodes_rows)
      BL_TRY(bl_routed_dgrad_nodes_rows(B.g_ln, Dm, L->msg_src, L->msg_tgt, S.bits, Dm / 32, L->type_ptr, T, L->Wt, E, Dm, Din, split,
                                        g_h_lo, ld_lo, g_h_hi, ld_hi, B.g_a, Din, st));
      BL_TRY(bl_mp_scatter_src_accum_impl(B.g_a, Din, L->src_ptr, L->src_msgs, N, Din, split, g_h_lo, ld_lo, g_h_hi, ld_hi,
                                          node_order, L->num_hub_slots, st));
    } else if (vec_dgrad) {
      ProfScope ps(9, 2.0 * N * (2.0 * Din) * Dm, st, two);
      BL_TRY(bl_routed_dgrad_vec(B.g_ln, Dm, L->msg_tgt, S.bits, Dm / 32, L->type_ptr, T, L->Wt, E, Dm, 2 * Din, B.g_a, 2 * Din, st));
    } else if (run_rows) {  // g_a [E + R, Din]: rows 0..E-1 the messages' source halves, E..E+R-1 the runs' target halves
      ProfScope ps(15, 2.0 * (double)rr_rows * Din * Dm, st, two);
      g.idx[0] = rr_rows_tgt;
      BL_TRY(bl_gemm_rows_h3(&g, rr_bits, Dm / 32, w_packed_bwd, bl_packed_weight_elems_h3(1, Dm, Din), rr_group_ptr, L->bwd_group_w, 2 * T,
                             rr_rows, Din, Dm, 1.0f / BL_H3_W_SCALE, B.amax, B.g_a, Din, st));
    } else if (h3) {
      ProfScope ps(15, 2.0 * E * (2.0 * Din) * Dm, st, two);
      BL_TRY(bl_gemm_rows_h3(&g, bits, Dm / 32, w_packed_bwd, bl_packed_weight_elems_h3(1, Dm, 2 * Din), L->type_ptr, nullptr, T, E, 2 * Din,
                             Dm, 1.0f / BL_H3_W_SCALE, B.amax, B.g_a, 2 * Din, st));
    } else {
      ProfScope ps(9, 2.0 * E * (2.0 * Din) * Dm, st, two);
      if (bl_mp_layer_weight_image(Din, Dm, 1))
        BL_TRY(bl_gemm_rows_x6w(&g, bits, Dm / 32, w_packed_bwd, bl_packed_weight_elems_x6w(1, Dm, 2 * Din), L->type_ptr, nullptr, T,
                                E, 2 * Din, Dm, B.g_a, 2 * Din, st));
      else
        BL_TRY(bl_gemm_rows_x6(&g, bits, Dm / 32, w_packed_bwd, (int64_t)packed_w_elems(1, Dm, 2 * Din), L->type_ptr, nullptr, T, E,
                               2 * Din, Dm, B.g_a, 2 * Din, st));
    }
  }
  if (!fused_sums) {
    ProfScope ps(10, 0.0, st, two);
    // E == 0: both CSRs are empty and g_a is never read
    if (live) {  // sums over the reduced CSRs into the rows live_recv of a zero-filled result
      const int split = g_h_hi ? width_lo : Din;
      auto zero = [&](float* p, int ld, int w) {
        return ld == w ? hipMemsetAsync(p, 0, (size_t)N * w * 4, st) : hipMemset2DAsync(p, (size_t)ld * 4, 0, (size_t)w * 4, N, st);
      };
      if (zero(g_h_lo, ld_lo, split) != hipSuccess || (g_h_hi && zero(g_h_hi, ld_hi, Din - split) != hipSuccess)) {
        bl_set_error("bl_mp_layer_bwd: memset failed");
        return BL_EINVAL;
      }
      if (Ex > 0)
        BL_TRY(bl_mp_scatter_grad_hubs_impl(B.g_a, Din, L->live_src_ptr, L->live_src_msgs, L->live_run_csr_ptr, L->live_run_csr_rows,
                                            L->live_num_recv, Din, width_lo, g_h_lo, ld_lo, g_h_hi, ld_hi, nullptr, 0, 0, st, L->live_recv));
    } else if (run_rows)
      BL_TRY(bl_mp_scatter_grad_hubs_impl(B.g_a, Din, L->src_ptr, L->src_msgs, L->tgt_run_ptr, L->tgt_run_rows, N, Din, width_lo, g_h_lo, ld_lo,
                                          g_h_hi, ld_hi, node_order, L->num_hub_slots, 0, st));
    else
    BL_TRY(bl_mp_scatter_grad_hubs_impl(B.g_a, 2 * Din, L->src_ptr, L->src_msgs, L->tgt_ptr, L->tgt_msgs, N, Din, width_lo, g_h_lo, ld_lo,
                                        g_h_hi, ld_hi, node_order, L->num_hub_slots, Din, st));
  }
  if (msgs && late_fork) BL_TRY(launch_wgrad());
  if (two && join_side) {
    (void)hipEventRecord(ev->join, side);
    (void)hipStreamWaitEvent(st, ev->join, 0);
  }
  return BL_OK;
}
