// qtx_host.h — what the C-ABI's host sources (qtx_model.hip, qtx_api.hip, qtx_fault.hip,
// qtx_trials.hip, qtx_enctrials.hip, qtx_search.hip, qtx_ops.hip) share, internal to libqtx: the model handle, the
// error and status helpers, the frame and the argument rules of a model-level entry, and the
// stack and decode-step helpers that cross files.  Host code only: no kernel in any of them.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/qtx.h"
#include "qtx_kernels.h"
#include "qtx_knobs.h"
#include "qtx_carve.h"       // Arena, Scratch, CrossKV and the workspaces with their carving
#include "qtx_stepgraph.h"   // StepGraphs: the decode graphs' capture, cache and replay

namespace qtx {

// One quantized linear: int8 q [N,K] (or packed int4 [N,K/2]), per-channel scale, bias.
struct QLin {
  int8_t* q = nullptr;
  float* s = nullptr;
  float* b = nullptr;
  int N = 0, K = 0;
  int8_t* qkp = nullptr;   // encoder, 8-bit: q in the row GEMM's KP layout (pack_w_kp)
  int8_t* qws = nullptr;   // encoder, 8-bit, K == 512: q in the weight-stationary order
  int8_t* qws32 = nullptr; // encoder Q/K/V, FFN1 in the WS32 order (diagnostic build: QTX_WS32)
  // 4-bit models: the int4 values (in [-7, 7]) unpacked to int8 [N, K] once at load, so the
  // int8 kernels run them — exact (integer products), and the decode is latency-bound, so
  // the packed form's half bytes bought nothing while its unpack lengthened every kernel
  // (cfg4 15.97 vs cfg2 14.45 ms per decode at r03d).  q stays packed (qtx_model_linear).
  int8_t* q8 = nullptr;
  const int8_t* w8() const { return q8 ? q8 : q; }   // the int8 form (8-bit models: q)
};

struct EncLayer {
  QLin qkv, o, w1, w2;
  const float* ln[2][2];
  int8_t* ffn = nullptr;   // W1 + W2 as k_ffn_fused's weight stream (launch_pack_ffn)
};
struct DecLayer {
  QLin qkv, o, cq, ckv, co, w1, w2;
  const float* ln[3][2];
};

}  // namespace qtx

struct qtx_model {
  qtx_config cfg;
  std::vector<qtx::EncLayer> enc;
  std::vector<qtx::DecLayer> dec;
  const float* enc_norm[2];
  const float* dec_norm[2];
  const float *src_lut, *tgt_lut, *pe, *gen_w, *gen_b;
  float* gen_wt = nullptr;   // generator weight in k_generator_mfma's MFMA order (pack_gen)
  // the decoder layers' cross K/V linears as ONE [n_layers * 2 * d_model, d_model] linear
  // (each dec[l].ckv is a view of rows 2 d_model l ..): the once-per-decode cross K/V of all
  // layers in one launch instead of n_layers (cross_kv)
  qtx::QLin ckv_all;
  void* mem = nullptr;
  size_t bytes = 0;
  // guards sg, dfault and the encoder's second stream
  std::mutex mu;
  qtx::StepGraphs sg;   // the decode-step graphs with their streams and events (qtx_stepgraph.h)
  // validity headers of the decoder-fault decode's workspaces, by workspace pointer (guarded
  // by mu; include/qtx.h qtx_greedy_dfault_resume)
  struct DfaultHdr {
    int B, S, L;         // the shapes the workspace was filled for
    int n;               // cache rows and ids of steps 0 .. n are golden
    bool gold_full;      // the golden copies hold a whole golden decode
    size_t bytes;
    long long nonce;     // also stamped into the workspace: memory reused or overwritten by
                         // someone else no longer matches
  };
  std::map<const void*, DfaultHdr> dfault;
  // encoder sub-batch pipelining: second stream + fork/lag/join events (lazily created)
  hipStream_t estream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_lag = nullptr, ev_join = nullptr;
  int device = 0;            // the device the model's memory lives on
  unsigned long long serial = 0;   // unique per created model (call status records)
  unsigned* status = nullptr;      // kStatusSlots 16-byte status words (model memory)
  std::mutex slot_mu;              // guards slot_used
  std::vector<bool> slot_used;     // a live thread holds the slot (qtx_model.hip CallStatus)
  std::vector<bool> slot_had_owner;  // a thread held the slot before (its kernels may still
                                     // be in flight on that thread's streams)
};

namespace qtx {

// ---- errors (qtx_model.hip) -------------------------------------------------------------
// Records the calling thread's last error text (qtx_last_error) and returns code.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return ::qtx::fail(QTX_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                         __FILE__, __LINE__);                                           \
  } while (0)

#define RC(expr)                       \
  do {                                 \
    int rc_ = (expr);                  \
    if (rc_ != QTX_OK) return rc_;     \
  } while (0)

// a base the kernels' 16-byte vector loads / stores can take (null: not passed)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Makes the model's device current for the lifetime of the guard (streams and events are
// created on the current device), restoring the caller's device afterwards.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---- the frame of a model-level entry (qtx_model.hip) -----------------------------------
// A model-level entry runs, in this order: its null and pair checks; the shape and limit
// rules below; the workspace size (check_workspace); the validation of its fault; then
// frame_begin; then the staging of src_mask, the launches, and the copy-out.  Nothing before
// frame_begin touches the model or the workspace, so a refused call changes nothing.
struct CallFrame {
  Arena ar;                     // over the caller's workspace
  unsigned* status = nullptr;   // the calling thread's status word (claim_status)
};
inline Arena ws_arena(void* ws, size_t ws_bytes) {
  Arena ar;
  ar.base = static_cast<uint8_t*>(ws); ar.cap = ws_bytes;
  return ar;
}
// Drops the decoder-fault decode's header of ws (the call rewrites the workspace: a later
// qtx_greedy_dfault_resume on that memory is refused), lays the Arena over ws and, with
// claim_status, claims the thread's status word (call_status_begin).  Three entries differ on
// purpose: qtx_decoder_forward_fault claims no word (no decoder kernel sets one, so an error
// an earlier encode left stays until qtx_model_check reports it); qtx_greedy_decode_kvfault
// carves (ws_arena) and validates its upset against the carved caches first, so only a call
// that will run forgets the header; qtx_greedy_dfault_resume has no frame: it reads the
// header and forgets it only when its stamp check fails or it overwrites the golden state.
int frame_begin(const qtx_model* m, void* ws, size_t ws_bytes, hipStream_t st, bool claim_status,
                CallFrame* f);
void dfault_forget(const qtx_model* m, const void* ws);
int call_status_begin(const qtx_model* m, unsigned** word, hipStream_t st);
// ids [B, max_len] and, with top_ids and max_len > 1, the steps' two best [B, max_len - 1, 2],
// from the workspace's (or the golden) copies to the caller's; the record [B, 2, 2] likewise
int copy_out(const int64_t* ws_ids, const int64_t* ws_top_ids, const float* ws_top_logp, int B,
             int max_len, int64_t* ids, int64_t* top_ids, float* top_logp, hipStream_t st);
int copy_out_record(const int64_t* ws_rec_ids, const float* ws_rec_logp, int B, int64_t* rec_ids,
                    float* rec_logp, hipStream_t st);

// The argument rules several entries share, one function each; QTX_OK or the refusal.
// bad_decode_shape: B sentences of S source tokens and up to T target positions, as every
// decode and the target scoring take them
bool bad_decode_shape(const qtx_config& c, int B, int S, int T);
int check_decode_shape(const qtx_config& c, int B, int S, int max_len);
inline int check_below_2_30(const qtx_config& c, int B, int max_len) {
  if ((long)B * c.tgt_vocab >= (1L << 30) || (long)B * max_len * c.d_model >= (1L << 30))
    return fail(QTX_E_INVALID, "B * tgt_vocab and B * max_len * d_model must be below 2^30");
  return QTX_OK;
}
inline int check_top2_vocab(const qtx_config& c) {
  return c.tgt_vocab < 2 ? fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", c.tgt_vocab) : QTX_OK;
}
inline int check_pairs(const void* top_ids, const void* top_logp, const void* rec_ids, const void* rec_logp) {
  if (!top_ids != !top_logp || !rec_ids != !rec_logp)
    return fail(QTX_E_INVALID, "top_ids / top_logp and rec_ids / rec_logp come in pairs");
  return QTX_OK;
}
inline int check_top_pair(const void* top_ids, const void* top_logp) {
  return !top_ids != !top_logp ? fail(QTX_E_INVALID, "top_ids and top_logp come as a pair") : QTX_OK;
}
inline int refuse_dbg_tail(const char* entry) {
  return knobs().dbg_tail ? fail(QTX_E_UNSUPPORTED, "%s: not with QTX_DBG_TAIL", entry) : QTX_OK;
}
inline int check_fault_bits(const qtx_config& c) {
  return c.weight_bits != 8 ? fail(QTX_E_UNSUPPORTED, "fault injection needs 8-bit weights") : QTX_OK;
}
inline int check_workspace(size_t ws_bytes, size_t need) {
  return ws_bytes < need ? fail(QTX_E_WORKSPACE, "workspace too small") : QTX_OK;
}

// qtx_row_gemm as the kernels' RowGemmArgs with qtx_linear_rows' argument rules (qtx_ops.hip;
// qtx_linear_rows_faults, qtx_enctrials.hip, applies the same)
int row_gemm_args(const qtx_row_gemm* a, RowGemmArgs* g);
int launched(hipError_t e, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- stack building blocks (qtx_api.hip) --------------------------------------------------
RowArgs rows_quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s);
int ln_quant(const float* x, int rows, const float* const* ln, int D, int8_t* q, float* s,
             hipStream_t st, bool kp = false);
int ln_out(const float* x, int rows, const float* const* ln, int D, float* y, hipStream_t st);
int quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s, hipStream_t st,
          bool kp = false);
int linear(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
           int flags, const float* res, float* out, long ldo, hipStream_t st,
           const FaultArgs& fa = FaultArgs{});
int cross_attn_block(const qtx_model* m, const DecLayer& L, int l, Scratch& s, const CrossKV& x,
                     int B, int T, int S, const uint8_t* src_mask, hipStream_t st,
                     const FaultArgs& fcq = FaultArgs{}, const FaultArgs& fco = FaultArgs{},
                     const AttnFault* af = nullptr);
int ffn_block(const qtx_config& c, const QLin& w1, const QLin& w2, const float* const* ln,
              Scratch& s, int M, hipStream_t st, const FaultArgs& f1 = FaultArgs{},
              const FaultArgs& f2 = FaultArgs{});

// fault injection (qtx_fault, include/qtx.h): the GEMM that computes a given reference MatMul
enum GemmId { G_QKV, G_O, G_FFN1, G_FFN2, G_CQ, G_CKV, G_CO };
FaultArgs fault_for(const qtx_fault* f, int module, int layer, GemmId gid, int M,
                    const qtx_config& c);
bool attn_fault_for(const qtx_fault* f, int module, int layer, bool cross, int Sq, int Sk,
                    AttnFault& af);
// self_keys / w_window (0: Sq): a cached step's self-attention has Sq = 1 query over self_keys
// keys, and takes a WEIGHT16 window anywhere (one past query row 0 has no effect)
int check_fault(const qtx_model* m, const qtx_fault* f, int module, long B, long Sq, long Ss,
                long self_keys = 0, long w_window = 0);
// whether f sits in a memory K / V projection (the fault then needs its own cross K/V)
bool ckv_fault(const qtx_model* m, const qtx_fault* f, int Ms);

// the row-complete chain's pieces the encoder trials decode shares (qtx_api.hip)
bool row_path(const qtx_config& c);
RowGemmArgs rowgemm(const QLin& L, const int8_t* a8, const float* sa, int M, int epi, bool kp);
int attention_quant(const AttnArgs& a, const AttnFault* af, int M, int D, Scratch& s, bool kp,
                    hipStream_t st);
// linear() at any M on the row-fault GEMM, every row with its own table entry (qtx_trials.hip)
int rf_linear(const QLin& L, const int8_t* a8, const float* sa, int M, int flags, const float* res,
              float* out, long ldo, const RowFault* tab, int t, int l, GemmId gid, hipStream_t st);
// The refusal of row b, with the row in its text (qtx_trials.hip)
int named(int rc, int b);
// the steps of a greedy decode after greedy_prologue (greedy_run's path selection)
int greedy_steps(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, hipStream_t st);

// ---- the stacks and the decode steps (qtx_api.hip) ----------------------------------------
int encoder_run(const qtx_model* m, const float* x, const uint8_t* mask, int B, int S,
                float* out, Scratch& s, hipStream_t st, const qtx_fault* f = nullptr,
                hipEvent_t after_first = nullptr);
int cross_kv(const qtx_model* m, const float* memory, int Ms, CrossKV& x, hipStream_t st,
             const qtx_fault* f = nullptr);
int decoder_body(const qtx_model* m, Scratch& s, const CrossKV& x, const uint8_t* src_mask,
                 const uint8_t* tgt_mask, long tm_bs, int B, int T, int S, float* out,
                 const qtx_fault* f, hipStream_t st);
Groups decode_groups(int B);
bool greedy_fused(const qtx_config& c, int S, int max_len);   // the fused step, else the unfused
// k_dec_attn's arguments for layer l's cached self / cross attention on g's step scratch
DecAttnArgs dec_attn_self(const GreedyWS& g, int l, int B, int max_len, int host_step1);
DecAttnArgs dec_attn_cross(const GreedyWS& g, int l, int B, int S, const uint8_t* src_mask);
// The unfused step's cached self-attention of layer l: q, and the K and V rows into the cache
// at the step's position, quantized from the Q/K/V GEMM's output in s.y; attention over
// position + 1 keys (af: its faulty row recomputed).  t >= 0: the position from the host,
// else the device counter g.step.
int cached_self_attn_unfused(GreedyWS& g, int l, int B, int max_len, int t, const AttnFault* af,
                             hipStream_t st);
int greedy_step_unfused(const qtx_model* m, GreedyWS& g, int B, int S, int max_len,
                        int64_t* ids, const uint8_t* src_mask, hipStream_t st);
// x's values of every layer in k_dec_attn's 4-key groups (cvg: all layers, GreedyWS::cvg[0])
int regroup_cross_values(const qtx_config& c, const CrossKV& x, int B, int S, int8_t* cvg,
                         hipStream_t st);
int encode_src(const qtx_model* m, GreedyWS& g, const int64_t* src, const uint8_t* mask, int B,
               int S, CrossKV& x, int8_t* cvg, const qtx_fault* f, hipStream_t st);
int greedy_prologue(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S,
                    int max_len, int64_t start, const qtx_fault* f, bool fused, hipStream_t st);
// the sub-batches' workspaces (group_view) of g
inline std::vector<GreedyWS> group_views(const GreedyWS& g, const qtx_config& c, const Groups& gr,
                                         int S, int max_len) {
  std::vector<GreedyWS> gv;
  for (int i = 0; i < gr.G; ++i) gv.push_back(group_view(g, c, i, gr.b0(i), S, max_len));
  return gv;
}
// The request of fused steps on B rows in the groups gr, gv[i] the workspace of group i (it
// must outlive the request): the key, and the per-group step with its ids / mask offsets.
// The caller adds the plan (and, for the beam form, the select's constants).
StepRequest step_request(const qtx_model* m, std::vector<GreedyWS>& gv, const Groups& gr, int B,
                         int S, int max_len, StepForm form);
// steps per graph of the decodes that run in chunks (QTX_GRAPH_STEPS, default 8)
inline int graph_chunk() { return knobs().graph_steps > 0 ? knobs().graph_steps : 8; }
int run_steps(const qtx_model* m, const StepRequest& rq, hipStream_t st);
// a stack's attention arguments on the scratch s (kbs_rows: the K/V rows per sentence)
AttnArgs attn_args(const Scratch& s, int B, int Sq, int Sk, long kbs_rows);

// ---- the fault decodes' parts the trials decode is built from (qtx_fault.hip) -------------
int dfault_steps(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t0, int t1,
                 hipStream_t st);
int record_top2(const float* logits, int B, int V, int64_t* rec_ids, float* rec_logp, int which,
                hipStream_t st);
int kvfault_check_fault(const qtx_model* m, const qtx_fault* f, int B, int S, int step);
struct UpsetAt { int8_t* c0; int8_t* c1; float* s; };
int kvfault_upset_at(const qtx_config& c, GreedyWS& g, const qtx_cache_upset* u, int B, int S,
                     int max_len, int step, bool fused, UpsetAt* at);

}  // namespace qtx
