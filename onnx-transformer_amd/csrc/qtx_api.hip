// qtx_api.hip — the C-ABI (include/qtx.h): model handle, per-op entry points and the
// encoder / decoder / greedy-decode drivers built from the kernels of qtx_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <string>
#include <vector>

#include "../../include/qtx.h"
#include "qtx_kernels.h"
#include "qtx_knobs.h"
#include "qtx_carve.h"   // Arena, Scratch, CrossKV, GreedyWS, BeamWS and their carving
#include "qtx_stepgraph.h"   // StepGraphs: the decode graphs' capture, cache and replay

using namespace qtx;

#ifdef QTX_DIAG
namespace qtx {   // csrc/diag/qtx_wsgemm_diag.hip
hipError_t launch_pack_w_ws32(const int8_t* W, int N, int K, int8_t* out, hipStream_t st);
}
#endif

namespace {

thread_local std::string g_err;

// the WS32 copies exist only in the diagnostic build (qws32 stays null in the product)
hipError_t pack_w_ws32(const int8_t* W, int N, int K, int8_t* out, hipStream_t st) {
#ifdef QTX_DIAG
  return launch_pack_w_ws32(W, N, K, out, st);
#else
  (void)W; (void)N; (void)K; (void)out; (void)st;
  return hipErrorInvalidValue;
#endif
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(QTX_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                            \
  } while (0)

// a base the kernels' 16-byte vector loads / stores can take (null: not passed)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int qtx::stepgraph_hip_error(const char* what, hipError_t e) {
  return fail(QTX_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

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

struct qtx_model {
  qtx_config cfg;
  std::vector<EncLayer> enc;
  std::vector<DecLayer> dec;
  const float* enc_norm[2];
  const float* dec_norm[2];
  const float *src_lut, *tgt_lut, *pe, *gen_w, *gen_b;
  float* gen_wt = nullptr;   // generator weight in k_generator_mfma's MFMA order (pack_gen)
  // the decoder layers' cross K/V linears as ONE [n_layers * 2 * d_model, d_model] linear
  // (each dec[l].ckv is a view of rows 2 d_model l ..): the once-per-decode cross K/V of all
  // layers in one launch instead of n_layers (cross_kv)
  QLin ckv_all;
  void* mem = nullptr;
  size_t bytes = 0;
  // guards sg, dfault and the encoder's second stream
  std::mutex mu;
  StepGraphs sg;   // the decode-step graphs with their streams and events (qtx_stepgraph.h)
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
  std::vector<bool> slot_used;     // a live thread holds the slot (qtx_api.hip CallStatus)
  std::vector<bool> slot_had_owner;  // a thread held the slot before (its kernels may still
                                     // be in flight on that thread's streams)
};

namespace {
// A call that rewrites a workspace drops the decoder-fault decode's header for it: a later
// qtx_greedy_dfault_resume on that memory is refused.
void dfault_forget(const qtx_model* mc, const void* ws) {
  qtx_model* m = const_cast<qtx_model*>(mc);
  std::lock_guard<std::mutex> lk(m->mu);
  m->dfault.erase(ws);
}
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
}  // namespace

namespace {

// ---- the device status word ------------------------------------------------------------
const char* status_text(unsigned v) {
  return (v & DEV_E_EXCHANGE_TIMEOUT)
             ? "k_gemm_wsx: the in-launch exchange of FFN1 row maxima timed out (the encoder's "
               "FFN hidden was quantized from a partial row maximum): outputs invalid"
             : "device status word set";
}
// Status words live in the model's own memory: kStatusSlots 16-byte words, one per live
// calling thread.  A thread's first model-level call that can raise a device error (the
// encoder and greedy-decode entry points) claims a free slot and zeroes it (call_status_begin);
// the slot returns to the model when the thread exits.  A thread should check (or at least
// synchronise) before it exits: an error its kernels raise after it is gone is dropped when
// the next owner claims the slot.  A kernel that detects an error it
// cannot repair (k_gemm_wsy's exchange timeout) ORs a DEV_E_* bit into the word, and the bit
// stays until qtx_model_check reports it (later calls never clear it: ADVICE r04).
// qtx_model_check(m, stream) synchronises the stream and reads the calling thread's word,
// so an error is reported to the thread whose call raised it and no other thread's call can
// clear it, and no later use of a caller's workspace can overwrite it.
// No slot is ever shared: a thread that finds every slot held by a live thread gets
// QTX_E_UNSUPPORTED (VERDICT r04 hygiene; QTX_STATUS_SLOTS lowers the cap for the test).
constexpr int kStatusSlots = 256;
struct CallStatus {
  const qtx_model* m = nullptr;
  unsigned long long serial = 0;    // the model's creation serial (a new model at a freed
  int slot = -1;                    // address is a different model)
};
// live models by serial: a thread's exit returns its slots only to models still alive
std::mutex g_live_mu;
std::map<unsigned long long, qtx_model*> g_live;
void release_slot(const CallStatus& c);
struct ThreadCalls {
  std::vector<CallStatus> v;
  ~ThreadCalls() {
    for (const CallStatus& c : v) release_slot(c);
  }
};
thread_local ThreadCalls t_calls;

int status_slot_cap() {
  const int n = knobs().status_slots;
  return n > 0 && n < kStatusSlots ? n : kStatusSlots;
}

// the calling thread's word for m if it holds one (nullptr otherwise)
unsigned* held_status_word(const qtx_model* m) {
  for (const CallStatus& c : t_calls.v)
    if (c.m == m && c.serial == m->serial) return m->status + 4 * c.slot;
  return nullptr;
}

// the calling thread's word for m (nullptr: every slot is held by a live thread); *fresh is
// set when the slot was claimed by this call (its word must be zeroed), *reused when a
// thread held that slot before
unsigned* thread_status_word(qtx_model* m, bool* fresh, bool* reused) {
  *fresh = false;
  *reused = false;
  if (unsigned* w = held_status_word(m)) return w;
  int slot = -1;
  {
    std::lock_guard<std::mutex> lk(m->slot_mu);
    const int cap = status_slot_cap();
    for (int i = 0; i < cap; ++i)
      if (!m->slot_used[i]) {
        m->slot_used[i] = true;
        *reused = m->slot_had_owner[i];
        m->slot_had_owner[i] = true;
        slot = i;
        break;
      }
  }
  if (slot < 0) return nullptr;
  // drop the records of models destroyed since (their serials are gone from g_live)
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    auto& v = t_calls.v;
    v.erase(std::remove_if(v.begin(), v.end(),
                           [](const CallStatus& c) {
                             auto it = g_live.find(c.serial);
                             return it == g_live.end() || it->second != c.m;
                           }),
            v.end());
  }
  t_calls.v.push_back(CallStatus{m, m->serial, slot});
  *fresh = true;
  return m->status + 4 * slot;
}

void release_slot(const CallStatus& c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  auto it = g_live.find(c.serial);
  if (it == g_live.end() || it->second != c.m) return;   // the model is gone
  qtx_model* m = it->second;
  std::lock_guard<std::mutex> lk2(m->slot_mu);
  m->slot_used[c.slot] = false;
}

// the calling thread's word, claimed and zeroed by its first status-carrying call on the
// model: zeroed eagerly (a synchronous hipMemset, so a claim cannot be
// captured into a graph and never run), and — when a thread held the slot before and may
// have exited with kernels still in flight that can set a bit — after the device has
// drained them, so no stale bit of the previous owner survives the zero
int call_status_begin(const qtx_model* mc, unsigned** word, hipStream_t st) {
  qtx_model* m = const_cast<qtx_model*>(mc);
  if ((*word = held_status_word(m)) != nullptr) return QTX_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIPCHK(hipStreamIsCapturing(st, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return fail(QTX_E_INVALID,
                "a thread's first encoder / greedy call on a model claims its device status "
                "word and cannot be stream-captured: make one uncaptured call first");
  bool fresh = false, reused = false;
  *word = thread_status_word(m, &fresh, &reused);
  if (!*word)
    return fail(QTX_E_UNSUPPORTED,
                "every device status word of this model is held by a live thread (%d): "
                "at most that many threads may call one model at a time",
                status_slot_cap());
  if (fresh) {
    if (reused) HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(*word, 0, 16));
  }
  return QTX_OK;
}

// ---- model layout ---------------------------------------------------------------------
// Linear order per layer follows qtx/weights.py:linear_names():
//   enc: self_attn.linears.0..3, w_1, w_2        (6 linears, 12 tensors)
//   dec: self_attn.linears.0..3, src_attn.linears.0..3, w_1, w_2   (10 linears)
int enc_tensor_base(const qtx_config& c, int L) { return 12 * L; }
int dec_tensor_base(const qtx_config& c, int L) { return 12 * c.n_layers + 20 * L; }
int norm_tensor_base(const qtx_config& c) { return 32 * c.n_layers; }

// The shapes every decode and the target scoring refuse: B sentences of S source tokens and
// up to T target positions.
bool bad_decode_shape(const qtx_config& c, int B, int S, int T) {
  return B <= 0 || S <= 0 || S > 512 || T < 1 || T > 512 || T > c.max_len || S > c.max_len;
}
int check_decode_shape(const qtx_config& c, int B, int S, int max_len) {
  if (bad_decode_shape(c, B, S, max_len))
    return fail(QTX_E_INVALID, "bad shape B=%d S=%d max_len=%d", B, S, max_len);
  return QTX_OK;
}

int check_cfg(const qtx_config* c) {
  if (!c) return fail(QTX_E_INVALID, "null config");
  if (c->d_model != 512 || c->n_heads * 64 != c->d_model)
    return fail(QTX_E_UNSUPPORTED, "d_model must be 512 with 64-wide heads");
  if (c->d_ff % 256 || c->d_ff > 2048 || c->d_ff < 256)
    return fail(QTX_E_UNSUPPORTED, "d_ff must be a multiple of 256 <= 2048");
  if (c->weight_bits != 8 && c->weight_bits != 4)
    return fail(QTX_E_UNSUPPORTED, "weight_bits must be 8 or 4");
  if (c->n_layers <= 0 || c->src_vocab <= 0 || c->tgt_vocab <= 0 || c->max_len <= 0)
    return fail(QTX_E_INVALID, "bad config");
  return QTX_OK;
}

size_t wbytes(const qtx_config& c, int N, int K) {
  return c.weight_bits == 8 ? (size_t)N * K : (size_t)N * K / 2;
}

// quantize rows [row0, row0+N) of lin from fp32 W [N,K] on device
int quantize_into(const qtx_config& c, QLin& L, int row0, const float* W, const float* b,
                  int N, int K, int8_t* tmp, hipStream_t st) {
  RowArgs a{};
  a.x = W; a.ldx = K; a.rows = N; a.D = K;
  a.qmax = c.weight_bits == 8 ? 127.0f : 7.0f;
  a.rpb = N; a.dst_bstride = 0; a.dst_off = 0;
  a.s = L.s + row0;
  if (c.weight_bits == 8) {
    a.q = L.q + (size_t)row0 * K; a.ldq = K;
    HIPCHK(launch_rows(a, st));
  } else {
    a.q = tmp; a.ldq = K;
    HIPCHK(launch_rows(a, st));
    HIPCHK(launch_pack_int4(tmp, N, K, reinterpret_cast<uint8_t*>(L.q) + (size_t)row0 * K / 2,
                            st));
    if (L.q8)
      HIPCHK(hipMemcpyAsync(L.q8 + (size_t)row0 * K, tmp, (size_t)N * K, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(L.b + row0, b, N * sizeof(float), hipMemcpyDeviceToDevice, st));
  return QTX_OK;
}

}  // namespace

// =======================================================================================
extern "C" {

const char* qtx_last_error(void) { return g_err.c_str(); }
const char* qtx_version(void) { return "qtx 0.1 gfx950"; }

int32_t qtx_model_tensor_count(const qtx_config* cfg) {
  if (check_cfg(cfg)) return -1;
  const int L = cfg->n_layers;
  return 12 * L + 20 * L + 2 * (2 * L + 1 + 3 * L + 1) + 4;
}

int32_t qtx_model_create(const qtx_config* cfg, const float* const* t, int32_t n,
                         const float* pe, void* stream, qtx_model** out) {
  if (int e = check_cfg(cfg)) return e;
  if (!t || !pe || !out) return fail(QTX_E_INVALID, "null argument");
  if (n != qtx_model_tensor_count(cfg))
    return fail(QTX_E_INVALID, "expected %d tensors, got %d", qtx_model_tensor_count(cfg), n);
  for (int i = 0; i < n; ++i)
    if (!t[i]) return fail(QTX_E_INVALID, "tensor %d is null", i);
  hipStream_t st = (hipStream_t)stream;
  const qtx_config c = *cfg;
  const int D = c.d_model, F = c.d_ff, NL = c.n_layers;

  // ---- size the arena (two passes of the same carve) ----
  auto carve = [&](qtx_model* m, Arena& ar) {
    auto lin = [&](QLin& L, int N, int K) {
      L.N = N; L.K = K;
      L.q = ar.take<int8_t>(wbytes(c, N, K));
      if (c.weight_bits == 4) L.q8 = ar.take<int8_t>((size_t)N * K);
      L.s = ar.take<float>(N);
      L.b = ar.take<float>(N);
    };
    m->enc.resize(NL);
    m->dec.resize(NL);
    for (auto& e : m->enc) { lin(e.qkv, 3 * D, D); lin(e.o, D, D); lin(e.w1, F, D); lin(e.w2, D, F); }
    // the row GEMM's KP copies and the weight-stationary ones serve the row-GEMM chain only
    // (row_path: d_ff % 512 == 0; launch_pack_w_kp takes whole 512-column tiles)
    if (c.d_ff % 512 == 0)
      for (auto& e : m->enc)
        for (QLin* L : {&e.qkv, &e.o, &e.w1, &e.w2}) L->qkp = ar.take<int8_t>((size_t)L->N * L->K);
    if (c.d_ff % 512 == 0)   // weight-stationary copies (K = 512 GEMMs)
      for (auto& e : m->enc) {
        for (QLin* L : {&e.qkv, &e.o, &e.w1}) L->qws = ar.take<int8_t>((size_t)L->N * L->K);
#ifdef QTX_DIAG
        for (QLin* L : {&e.qkv, &e.w1}) L->qws32 = ar.take<int8_t>((size_t)L->N * L->K);
#endif
      }
#ifdef QTX_DIAG
    // the fused FFN's weight stream (F KB per layer): only where QTX_FFN_FUSED_MIN_M can turn
    // that launch on (the diagnostic build; measured slower than the split launches, DESIGN
    // §4), not 12 MB of every product model
    if (c.d_ff % 64 == 0)
      for (auto& e : m->enc) e.ffn = ar.take<int8_t>((size_t)F * 1024);
#endif
    lin(m->ckv_all, NL * 2 * D, D);
    for (int l = 0; l < NL; ++l) {   // dec[l].ckv: rows 2Dl .. 2D(l+1) of ckv_all
      QLin& v = m->dec[l].ckv;
      const QLin& a = m->ckv_all;
      v.N = 2 * D; v.K = D;
      if (a.q) {
        v.q = a.q + wbytes(c, 2 * D, D) * l;
        v.q8 = a.q8 ? a.q8 + (size_t)2 * D * D * l : nullptr;
        v.s = a.s + 2 * D * l;
        v.b = a.b + 2 * D * l;
      }
    }
    for (auto& d : m->dec) {
      lin(d.qkv, 3 * D, D); lin(d.o, D, D); lin(d.cq, D, D);
      lin(d.co, D, D); lin(d.w1, F, D); lin(d.w2, D, F);
    }
    float* norms = ar.take<float>((size_t)2 * D * (5 * NL + 2));
    float* src_lut = ar.take<float>((size_t)c.src_vocab * D);
    float* tgt_lut = ar.take<float>((size_t)c.tgt_vocab * D);
    float* pe_d = ar.take<float>((size_t)c.max_len * D);
    float* gw = ar.take<float>((size_t)c.tgt_vocab * D);
    float* gb = ar.take<float>(c.tgt_vocab);
    // int4 staging of quantize_into: the largest N * K it is called with (D x D where F < D)
    int8_t* tmp = ar.take<int8_t>((size_t)std::max(F, D) * D);
    m->gen_wt = ar.take<float>((size_t)((c.tgt_vocab + 15) / 16) * 16 * D);
    m->status = ar.take<unsigned>(4 * kStatusSlots);
    return std::make_tuple(norms, src_lut, tgt_lut, pe_d, gw, gb, tmp);
  };
  qtx_model* m = new qtx_model();
  static std::atomic<unsigned long long> next_serial{1};
  m->serial = next_serial.fetch_add(1);
  m->slot_used.assign(kStatusSlots, false);
  m->slot_had_owner.assign(kStatusSlots, false);
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live[m->serial] = m;
  }
  m->cfg = c;
  (void)hipGetDevice(&m->device);
  Arena sizing;
  carve(m, sizing);
  const size_t bytes = align_up(sizing.used);
  void* mem = nullptr;
  hipError_t he = hipMalloc(&mem, bytes);
  if (he != hipSuccess) {
    delete m;
    return fail(QTX_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(he));
  }
  m->mem = mem;
  m->bytes = bytes;
  Arena ar;
  ar.base = (uint8_t*)mem;
  ar.cap = bytes;
  float *norms, *src_lut, *tgt_lut, *pe_d, *gw, *gb;
  int8_t* tmp;
  std::tie(norms, src_lut, tgt_lut, pe_d, gw, gb, tmp) = carve(m, ar);
  if (hipMemset(m->status, 0, 16 * kStatusSlots) != hipSuccess) {
    qtx_model_destroy(m);
    return fail(QTX_E_HIP, "hipMemset(status words)");
  }

  int rc = QTX_OK;
  auto Q = [&](QLin& L, int row0, int ti, int N, int K) {
    if (rc == QTX_OK) rc = quantize_into(c, L, row0, t[ti], t[ti + 1], N, K, tmp, st);
  };
  for (int l = 0; l < NL; ++l) {
    const int b = enc_tensor_base(c, l);
    EncLayer& e = m->enc[l];
    for (int i = 0; i < 3; ++i) Q(e.qkv, i * D, b + 2 * i, D, D);
    Q(e.o, 0, b + 6, D, D);
    Q(e.w1, 0, b + 8, F, D);
    Q(e.w2, 0, b + 10, D, F);
  }
  for (int l = 0; l < NL; ++l) {
    const int b = dec_tensor_base(c, l);
    DecLayer& d = m->dec[l];
    for (int i = 0; i < 3; ++i) Q(d.qkv, i * D, b + 2 * i, D, D);
    Q(d.o, 0, b + 6, D, D);
    Q(d.cq, 0, b + 8, D, D);
    Q(d.ckv, 0, b + 10, D, D);
    Q(d.ckv, D, b + 12, D, D);
    Q(d.co, 0, b + 14, D, D);
    Q(d.w1, 0, b + 16, F, D);
    Q(d.w2, 0, b + 18, D, F);
  }
  if (rc) { qtx_model_destroy(m); return rc; }
  for (auto& e : m->enc)
    for (QLin* L : {&e.qkv, &e.o, &e.w1, &e.w2})
      if ((L->qkp && launch_pack_w_kp(L->w8(), L->N, L->K, L->qkp, st) != hipSuccess) ||
          (L->qws && launch_pack_w_ws(L->w8(), L->N, L->K, L->qws, st) != hipSuccess) ||
          (L->qws32 && pack_w_ws32(L->w8(), L->N, L->K, L->qws32, st) != hipSuccess)) {
        qtx_model_destroy(m);
        return fail(QTX_E_HIP, "KP / WS weight pack");
      }
  for (auto& e : m->enc)
    if (e.ffn && launch_pack_ffn(e.w1.w8(), e.w2.w8(), F, e.ffn, st) != hipSuccess) {
      qtx_model_destroy(m);
      return fail(QTX_E_HIP, "fused FFN weight pack");
    }
  // norms: order of weights.py:norm_names — enc L x 2, enc final, dec L x 3, dec final
  const int nb = norm_tensor_base(c);
  const int n_norms = 5 * NL + 2;
  for (int i = 0; i < n_norms; ++i)
    for (int j = 0; j < 2; ++j) {
      he = hipMemcpyAsync(norms + (size_t)(2 * i + j) * D, t[nb + 2 * i + j], D * sizeof(float),
                          hipMemcpyDeviceToDevice, st);
      if (he != hipSuccess) { qtx_model_destroy(m); return fail(QTX_E_HIP, "copy norms"); }
    }
  auto nrm = [&](int i, int j) -> const float* { return norms + (size_t)(2 * i + j) * D; };
  int ni = 0;
  for (int l = 0; l < NL; ++l)
    for (int s = 0; s < 2; ++s, ++ni) { m->enc[l].ln[s][0] = nrm(ni, 0); m->enc[l].ln[s][1] = nrm(ni, 1); }
  m->enc_norm[0] = nrm(ni, 0); m->enc_norm[1] = nrm(ni, 1); ++ni;
  for (int l = 0; l < NL; ++l)
    for (int s = 0; s < 3; ++s, ++ni) { m->dec[l].ln[s][0] = nrm(ni, 0); m->dec[l].ln[s][1] = nrm(ni, 1); }
  m->dec_norm[0] = nrm(ni, 0); m->dec_norm[1] = nrm(ni, 1); ++ni;
  const int eb = nb + 2 * n_norms;
  struct Cp { float* dst; const float* src; size_t n; } cps[] = {
      {src_lut, t[eb], (size_t)c.src_vocab * D}, {tgt_lut, t[eb + 1], (size_t)c.tgt_vocab * D},
      {gw, t[eb + 2], (size_t)c.tgt_vocab * D}, {gb, t[eb + 3], (size_t)c.tgt_vocab},
      {pe_d, pe, (size_t)c.max_len * D}};
  for (auto& cp : cps) {
    he = hipMemcpyAsync(cp.dst, cp.src, cp.n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (he != hipSuccess) { qtx_model_destroy(m); return fail(QTX_E_HIP, "copy tables"); }
  }
  m->src_lut = src_lut; m->tgt_lut = tgt_lut; m->pe = pe_d; m->gen_w = gw; m->gen_b = gb;
  he = launch_pack_gen(gw, c.tgt_vocab, m->gen_wt, st);
  if (he != hipSuccess) { qtx_model_destroy(m); return fail(QTX_E_HIP, "pack generator"); }
  he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    qtx_model_destroy(m);
    return fail(QTX_E_HIP, "model create: %s", hipGetErrorString(he));
  }
  *out = m;
  return QTX_OK;
}

int32_t qtx_model_destroy(qtx_model* m) {
  if (!m) return QTX_OK;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);   // no thread exit returns a slot to it now
    g_live.erase(m->serial);
  }
  m->sg.destroy();
  for (hipEvent_t e : {m->ev_fork, m->ev_lag, m->ev_join})
    if (e) (void)hipEventDestroy(e);
  if (m->estream) (void)hipStreamDestroy(m->estream);
  if (m->mem) (void)hipFree(m->mem);
  delete m;
  return QTX_OK;
}

size_t qtx_model_device_bytes(const qtx_model* m) { return m ? m->bytes : 0; }

int32_t qtx_model_linear(const qtx_model* m, int32_t module, int32_t layer, int32_t index,
                         const void** q, const float** s, const float** b, int32_t* N,
                         int32_t* K) {
  if (!m || !q || !s || !b || !N || !K) return fail(QTX_E_INVALID, "qtx_model_linear: null argument");
  if (layer < 0 || layer >= m->cfg.n_layers) return fail(QTX_E_INVALID, "layer %d out of range", layer);
  // a slice of `rows` output channels starting at `r0` of a stored (possibly concatenated) linear
  auto view = [&](const QLin& l, int r0, int rows) {
    const long rb = m->cfg.weight_bits == 4 ? l.K / 2 : l.K;   // bytes per weight row
    *q = l.q + (long)r0 * rb;
    *s = l.s + r0;
    *b = l.b + r0;
    *N = rows;
    *K = l.K;
    return (int32_t)QTX_OK;
  };
  const int D = m->cfg.d_model;
  if (module == 0) {
    const EncLayer& e = m->enc[layer];
    switch (index) {
      case 0: case 1: case 2: return view(e.qkv, index * D, D);
      case 3: return view(e.o, 0, e.o.N);
      case 4: return view(e.w1, 0, e.w1.N);
      case 5: return view(e.w2, 0, e.w2.N);
    }
  } else if (module == 1) {
    const DecLayer& d = m->dec[layer];
    switch (index) {
      case 0: case 1: case 2: return view(d.qkv, index * D, D);
      case 3: return view(d.o, 0, d.o.N);
      case 4: return view(d.cq, 0, d.cq.N);
      case 5: case 6: return view(d.ckv, (index - 5) * D, D);
      case 7: return view(d.co, 0, d.co.N);
      case 8: return view(d.w1, 0, d.w1.N);
      case 9: return view(d.w2, 0, d.w2.N);
    }
  }
  return fail(QTX_E_INVALID, "qtx_model_linear: no linear %d of module %d", index, module);
}

int32_t qtx_model_norm(const qtx_model* m, int32_t module, int32_t layer, int32_t sub,
                       const float** a, const float** b) {
  if (!m || !a || !b) return fail(QTX_E_INVALID, "qtx_model_norm: null argument");
  if (layer == -1 && (module == 0 || module == 1)) {
    const float* const* n = module == 0 ? m->enc_norm : m->dec_norm;
    *a = n[0];
    *b = n[1];
    return QTX_OK;
  }
  if (layer < 0 || layer >= m->cfg.n_layers) return fail(QTX_E_INVALID, "layer %d out of range", layer);
  if (module == 0 && sub >= 0 && sub < 2) {
    *a = m->enc[layer].ln[sub][0];
    *b = m->enc[layer].ln[sub][1];
    return QTX_OK;
  }
  if (module == 1 && sub >= 0 && sub < 3) {
    *a = m->dec[layer].ln[sub][0];
    *b = m->dec[layer].ln[sub][1];
    return QTX_OK;
  }
  return fail(QTX_E_INVALID, "qtx_model_norm: no norm %d of module %d layer %d", sub, module, layer);
}

}  // extern "C"

// =======================================================================================
// drivers
// =======================================================================================
namespace {

// (Scratch / carve_scratch, the scratch for one stack pass over M rows: qtx_carve.h)

// ---- building blocks ------------------------------------------------------------------
RowArgs rows_quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s) {
  RowArgs a{};
  a.x = x; a.ldx = ldx; a.rows = rows; a.D = D;
  a.q = q; a.ldq = D; a.s = s; a.qmax = 127.0f;
  a.rpb = rows > 0 ? rows : 1; a.dst_bstride = 0; a.dst_off = 0;
  return a;
}

int ln_quant(const float* x, int rows, const float* const* ln, int D, int8_t* q, float* s,
             hipStream_t st, bool kp = false) {
  RowArgs a = rows_quant(x, D, rows, D, q, s);
  a.ln_a = ln[0]; a.ln_b = ln[1]; a.kp = kp;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int ln_out(const float* x, int rows, const float* const* ln, int D, float* y, hipStream_t st) {
  RowArgs a{};
  a.x = x; a.ldx = D; a.rows = rows; a.D = D; a.ln_a = ln[0]; a.ln_b = ln[1];
  a.yout = y; a.ldy = D; a.rpb = rows > 0 ? rows : 1;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int quant(const float* x, long ldx, int rows, int D, int8_t* q, float* s, hipStream_t st,
          bool kp = false) {
  RowArgs a = rows_quant(x, ldx, rows, D, q, s);
  a.kp = kp;
  HIPCHK(launch_rows(a, st));
  return QTX_OK;
}

int linear(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
           int flags, const float* res, float* out, long ldo, hipStream_t st,
           const FaultArgs& fa = FaultArgs{}) {
  GemmArgs g{};
  g.fault = fa;
  g.A = a8; g.lda = L.K; g.sa = sa;
  const int wb = L.q8 ? 8 : c.weight_bits;
  g.W = L.w8(); g.ldw = wb == 8 ? L.K : L.K / 2; g.sw = L.s; g.bias = L.b;
  g.out = out; g.ldo = ldo; g.res = res; g.ldr = ldo;
  g.M = M; g.N = L.N; g.K = L.K; g.flags = flags;
  HIPCHK(launch_gemm(g, wb, st));
  return QTX_OK;
}

// Row-complete GEMM (k_gemm_row) for 8-bit weights: epilogues of whole 512-wide rows.
bool row_path(const qtx_config& c) {   // (4-bit models: on the unpacked int8 weights)
  return c.d_ff % 512 == 0 && !knobs().no_rowgemm;
}
// kp: A (a8) in the KP layout and W from L.qkp; the int8 lnq / FFN-hidden outputs are
// then written KP as well (RE_QUANT's q8 stays row-major: attention reads it).
// With kp, a K = 512 GEMM over many rows runs weight-stationary (kp = 2, W from L.qws):
// each workgroup keeps a 512-column slice of W on chip (qtx_wsgemm.hip); below ws_min_m
// rows the per-workgroup W load is not amortized and the row GEMM is faster.
// Measured (tools/enc_small.py, the greedy decode's encoder): at M = 2304 (B = 32, S = 72)
// the Q/K/V and FFN1 launches on the weight-stationary kernel took the encoder 0.83 ->
// 0.73 ms (the row GEMM's 128-row tiles give 18 workgroups).  The O-projection's residual +
// LayerNorm epilogue runs weight-stationary only between ws_res_min_m and ws_res_max_m
// (above it the KP row GEMM is faster).  QTX_WS_MIN_M / QTX_WS_RES_MIN_M / _MAX_M: A/B.
long ws_min_m() { return knobs().ws_min_m; }
bool ws_res_ok(long M) { return M >= knobs().ws_res_min_m && M < knobs().ws_res_max_m; }
RowGemmArgs rowgemm(const QLin& L, const int8_t* a8, const float* sa, int M, int epi,
                    bool kp = false) {
  RowGemmArgs g{};
  const bool ws = kp && L.qws && L.K == 512 &&
                  (epi == RE_RES_LN ? ws_res_ok(M) : M >= ws_min_m());
  // Q/K/V on the 32x32x32 MFMA kernel (diagnostic build, QTX_WS32)
  const bool ws32 = ws && epi == RE_QUANT && L.qws32 && knobs().ws32;
  g.A = a8; g.lda = L.K; g.sa = sa; g.W = ws32 ? L.qws32 : ws ? L.qws : kp ? L.qkp : L.w8();
  g.ldw = L.K;
  g.sw = L.s; g.bias = L.b;
  g.M = M; g.N = L.N; g.K = L.K; g.epi = epi; g.kp = ws32 ? 4 : ws ? 2 : kp;
  return g;
}
hipError_t launch_row_gemm_any(const RowGemmArgs& g, hipStream_t st) {
  return g.kp == 2 || g.kp == 4 ? launch_gemm_ws(g, st) : launch_gemm_row(g, st);
}
// out = per-token quantized (a8 . W^T) per 512-wide tile into out8 + t*M*512, os + t*M
int row_quant(const QLin& L, const int8_t* a8, const float* sa, int M, int8_t* out8,
              float* os, hipStream_t st, const FaultArgs& fa = FaultArgs{}, bool kp = false,
              void* zero = nullptr, long zero16 = 0) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_QUANT, kp);
  g.fault = fa;
  g.zero = zero; g.zero16 = zero16;   // a side job (launch_gemm_ws), else a zeroing kernel
  g.out8 = out8; g.ldo8 = 512; g.o8_ts = (long)M * 512; g.os = os; g.os_ts = M;
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}
// x += a8 . W^T, then LayerNorm(x) (ln) quantized into (lnq, lns) or fp32 into lnout
// part: scratch for split-K partials (>= 4 * M * 2 KB; the FFN2 call sites pass the fp32
// GEMM scratch, free by then).  A KP row GEMM over at most 64 row tiles (FFN2 at the decode
// encoder's M = 2304: 18 workgroups, 43.9 us) runs K split 4 ways + a row-wise epilogue.
int row_res_ln(const QLin& L, const int8_t* a8, const float* sa, int M, float* x,
               const float* const* ln, int8_t* lnq, float* lns, float* lnout, hipStream_t st,
               const FaultArgs& fa = FaultArgs{}, bool kp = false, float* part = nullptr) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RES_LN, kp);
  g.fault = fa;
  g.res = x; g.xout = x; g.ln_a = ln[0]; g.ln_b = ln[1];
  g.lnq = lnq; g.lns = lns; g.lnout = lnout;
  if (part && g.kp == 1 && fa.kind == FK_NONE && (M + 127) / 128 <= 64 && L.K % 2048 == 0 &&
      !knobs().no_splitk) {
    g.part = reinterpret_cast<int32_t*>(part);
    g.ksplit = 4;
  }
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}
// FFN1: relu(a8 . W1^T) quantized per token over all d_ff columns, two passes (row
// maxima, then recompute + quantize: cheaper than the fp32 hidden's round trip)
// FFN1 in one weight-stationary pass with the row maxima exchanged between the column
// slices' workgroups inside the launch (k_gemm_wsx); QTX_NO_WSX=1: the two passes
bool wsx_on() { return !knobs().no_wsx; }
// Whether row_ffn1 takes the one-pass FFN1 (k_gemm_wsx / wsy) with its exchange scratch in
// s.y: then the layer's Q/K/V launch can zero that scratch as a side job (encoder_run).
bool ffn1_onepass(const QLin& L, int M, bool kp, const FaultArgs& fa) {
  return rowgemm(L, nullptr, nullptr, M, RE_RELU_PMAX, kp).kp == 2 && L.N == 2048 &&
         fa.kind == FK_NONE && wsx_on();
}
long ffn1_scratch16(int M) { return (4L * 32 * ((M + 31) / 32) + 2) / 2; }   // 16-B chunks
int row_ffn1(const qtx_config& c, const QLin& L, const int8_t* a8, const float* sa, int M,
             Scratch& s, hipStream_t st,
             const FaultArgs& fa = FaultArgs{}, bool kp = false, unsigned* status = nullptr,
             bool prezeroed = false) {
  RowGemmArgs g = rowgemm(L, a8, sa, M, RE_RELU_PMAX, kp);
  if (g.kp == 2 && L.N == 2048 && fa.kind == FK_NONE && wsx_on()) {
    g.epi = RE_RELU_QUANT_PMAX;
    g.prezeroed = prezeroed;
    if (L.qws32 && knobs().ws32) { g.W = L.qws32; g.kp = 5; }   // k_gemm_wsy32
    g.pmax_out = s.y;                // granules + ticket: <= 32 * M + 2048 bytes of the (unused) fp32 GEMM scratch
    g.out8 = s.h8; g.ldo8 = c.d_ff; g.os = s.sh;
    g.status = status;               // the model's status word: a timeout becomes an error
    HIPCHK(launch_gemm_wsx(g, st));
    return QTX_OK;
  }
  g.fault = fa;
  g.pmax_out = s.pmax;
  HIPCHK(launch_row_gemm_any(g, st));
  g.epi = RE_RELU_QUANT_PMAX;
  g.pmax_in = s.pmax; g.pmax_n = c.d_ff / 512;
  g.out8 = s.h8; g.ldo8 = c.d_ff; g.os = s.sh;
  HIPCHK(launch_row_gemm_any(g, st));
  return QTX_OK;
}

AttnArgs attn_args(const Scratch& s, int B, int Sq, int Sk, long kbs_rows) {
  AttnArgs a{};
  const int D = 512;
  a.q = s.q8; a.q_bs = (long)Sq * D; a.q_ld = D; a.sq = s.sq; a.sq_bs = Sq;
  a.k = s.k8; a.k_bs = kbs_rows * D; a.k_ld = D; a.sk = s.sk; a.sk_bs = kbs_rows;
  a.v = s.v8; a.v_bs = kbs_rows * D; a.v_ld = D; a.sv = s.sv; a.sv_bs = kbs_rows;
  a.ctx = s.ctx; a.c_bs = (long)Sq * D; a.c_ld = D;
  a.B = B; a.H = 8; a.Sq = Sq; a.Sk = Sk;
  return a;
}

#define RC(expr)                       \
  do {                                 \
    int rc_ = (expr);                  \
    if (rc_ != QTX_OK) return rc_;     \
  } while (0)

// Self-attention sublayer: x += O(attn(LN(x)))   (sublayer_connection.py:15-17,
// attention.py:39-67).  Q/K/V come out of ONE N=3D GEMM and are quantized per token.
// fqkv / fo / af: a fault of a fault-injection run in the Q/K/V GEMM, the O projection or
// the attention MatMuls (fault_for, attn_fault_for), as on the row-GEMM chain.
int self_attn_block(const qtx_config& c, const QLin& qkv, const QLin& o,
                    const float* const* ln, Scratch& s, int B, int S, const uint8_t* mask,
                    long m_bs, long m_is, bool dec, hipStream_t st,
                    const FaultArgs& fqkv = FaultArgs{}, const FaultArgs& fo = FaultArgs{},
                    const AttnFault* af = nullptr) {
  const int D = c.d_model, M = B * S;
  RC(ln_quant(s.x, M, ln, D, s.a8, s.sa, st));
  RC(linear(c, qkv, s.a8, s.sa, M, 0, nullptr, s.y, 3 * D, st, fqkv));
  RC(quant(s.y, 3 * D, M, D, s.q8, s.sq, st));
  RC(quant(s.y + D, 3 * D, M, D, s.k8, s.sk, st));
  RC(quant(s.y + 2 * D, 3 * D, M, D, s.v8, s.sv, st));
  AttnArgs a = attn_args(s, B, S, S, S);
  a.mask = mask; a.m_bs = m_bs; a.m_is = m_is;
  a.dec = dec;
  HIPCHK(launch_attention(a, st));
  if (af) HIPCHK(launch_attn_fault_rows(a, *af, st));   // the faulty rows recomputed
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  RC(linear(c, o, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, fo));
  return QTX_OK;
}

// FFN sublayer: x += w_2(relu(w_1(LN(x))))   (position_feed_forward.py:11-12)
int ffn_block(const qtx_config& c, const QLin& w1, const QLin& w2, const float* const* ln,
              Scratch& s, int M, hipStream_t st, const FaultArgs& f1 = FaultArgs{},
              const FaultArgs& f2 = FaultArgs{}) {
  const int D = c.d_model, F = c.d_ff;
  RC(ln_quant(s.x, M, ln, D, s.a8, s.sa, st));
  RC(linear(c, w1, s.a8, s.sa, M, EPI_RELU, nullptr, s.y, F, st, f1));
  RC(quant(s.y, F, M, F, s.a8, s.sa, st));
  RC(linear(c, w2, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, f2));
  return QTX_OK;
}


// ---- fault injection (qtx_fault, include/qtx.h) -------------------------------------
// The GEMM that computes a given reference MatMul, and that linear's column offset in it.
enum GemmId { G_QKV, G_O, G_FFN1, G_FFN2, G_CQ, G_CKV, G_CO };
FaultArgs fault_for(const qtx_fault* f, int module, int layer, GemmId gid, int M,
                    const qtx_config& c) {
  FaultArgs fa{};
  if (!f || f->kind == QTX_FAULT_NONE || f->module != module || f->layer != layer) return fa;
  const int lin = f->linear;
  long off = 0, nlin = c.d_model;
  switch (gid) {
    case G_QKV: if (lin < QTX_LIN_Q || lin > QTX_LIN_V) return fa; off = (long)lin * c.d_model; break;
    case G_CKV: if (lin != QTX_LIN_CK && lin != QTX_LIN_CV) return fa;
                off = (long)(lin - QTX_LIN_CK) * c.d_model; break;
    case G_O: if (lin != QTX_LIN_O) return fa; break;
    case G_FFN1: if (lin != QTX_LIN_FFN1) return fa; nlin = c.d_ff; break;
    case G_FFN2: if (lin != QTX_LIN_FFN2) return fa; break;
    case G_CQ: if (lin != QTX_LIN_CQ) return fa; break;
    case G_CO: if (lin != QTX_LIN_CO) return fa; break;
  }
  fa.bit = f->bit;
  switch (f->kind) {
    case QTX_FAULT_INPUT: case QTX_FAULT_INPUT16:
      fa.kind = FK_INPUT; fa.row = f->row; fa.col = f->col;
      fa.lo = off + (f->kind == QTX_FAULT_INPUT16 ? f->win_start : 0);
      fa.hi = f->kind == QTX_FAULT_INPUT16 ? fa.lo + f->win_len : off + nlin;
      break;
    case QTX_FAULT_WEIGHT: case QTX_FAULT_WEIGHT16:
      fa.kind = FK_WEIGHT; fa.row = off + f->row; fa.col = f->col;
      fa.lo = f->kind == QTX_FAULT_WEIGHT16 ? f->win_start : 0;
      fa.hi = f->kind == QTX_FAULT_WEIGHT16 ? fa.lo + f->win_len : M;
      break;
    case QTX_FAULT_OUTPUT:
      fa.kind = FK_OUTPUT; fa.row = f->row; fa.col = off + f->col; fa.value = f->value;
      break;
  }
  return fa;
}

// The fault as an AttnFault if it targets this layer's self (cross = false) or cross
// attention MatMuls (see qtx.h for the index conventions).
bool attn_fault_for(const qtx_fault* f, int module, int layer, bool cross, int Sq, int Sk,
                    AttnFault& af) {
  if (!f || f->kind == QTX_FAULT_NONE || f->module != module || f->layer != layer) return false;
  const int lin = f->linear;
  bool qk;
  if (!cross && (lin == QTX_LIN_QK || lin == QTX_LIN_PV)) qk = lin == QTX_LIN_QK;
  else if (cross && (lin == QTX_LIN_CQK || lin == QTX_LIN_CPV)) qk = lin == QTX_LIN_CQK;
  else return false;
  const bool in = f->kind == QTX_FAULT_INPUT || f->kind == QTX_FAULT_INPUT16;
  const bool win = f->kind == QTX_FAULT_INPUT16 || f->kind == QTX_FAULT_WEIGHT16;
  af = AttnFault{};
  af.bit = f->bit;
  af.value = f->value;
  const long row = f->row, col = f->col;
  if (f->kind == QTX_FAULT_OUTPUT) {
    af.kind = qk ? AF_QK_OUTPUT : AF_PV_OUTPUT;
    af.b = row / Sq; af.i = row % Sq;
    if (qk) { af.h = col / Sk; af.j = col % Sk; } else { af.h = col / 64; af.d = col % 64; }
    af.row0 = af.i; af.nrows = 1;
    return true;
  }
  if (in) {
    af.kind = qk ? AF_QK_INPUT : AF_PV_INPUT;
    af.b = row / Sq; af.i = row % Sq;
    if (qk) { af.h = col / 64; af.d = col % 64; } else { af.h = col / Sk; af.j = col % Sk; }
    af.lo = win ? (int)f->win_start : 0;
    af.hi = win ? (int)(f->win_start + f->win_len) : (qk ? Sk : 64);
    af.row0 = af.i; af.nrows = 1;
  } else {
    af.kind = qk ? AF_QK_WEIGHT : AF_PV_WEIGHT;
    af.b = row / Sk; af.j = row % Sk; af.h = col / 64; af.d = col % 64;
    af.lo = win ? (int)f->win_start : 0;
    af.hi = win ? (int)(f->win_start + f->win_len) : Sq;
    af.row0 = af.lo; af.nrows = af.hi - af.lo;
  }
  return true;
}

// attention with an optional fault: fp32 context (+ the faulty rows recomputed), then the
// per-token quantization of the O-projection input
int attention_fault(const AttnArgs& a, const AttnFault& af, int M, int D, Scratch& s,
                    hipStream_t st) {
  HIPCHK(launch_attention(a, st));
  HIPCHK(launch_attn_fault_rows(a, af, st));
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  return QTX_OK;
}

// Validates a fault against the shapes of its target MatMul (M token rows of the module,
// Ms memory rows for the decoder's cross K/V); returns QTX_OK or an error code.
int check_fault(const qtx_model* m, const qtx_fault* f, int module, long B, long Sq, long Ss) {
  if (!f || f->kind == QTX_FAULT_NONE) return QTX_OK;
  const qtx_config& c = m->cfg;
  const long M = B * Sq, Ms = B * Ss;
  if (c.weight_bits != 8)
    return fail(QTX_E_UNSUPPORTED, "fault injection needs 8-bit weights");
  if (f->kind < 0 || f->kind > QTX_FAULT_OUTPUT) return fail(QTX_E_INVALID, "fault kind %d", f->kind);
  if (f->module != module) return fail(QTX_E_INVALID, "fault module %d", f->module);
  if (f->layer < 0 || f->layer >= c.n_layers) return fail(QTX_E_INVALID, "fault layer %d", f->layer);
  const int lin = f->linear;
  const bool in_kind = f->kind == QTX_FAULT_INPUT || f->kind == QTX_FAULT_INPUT16;
  const bool w_kind = f->kind == QTX_FAULT_WEIGHT || f->kind == QTX_FAULT_WEIGHT16;
  const bool win = f->kind == QTX_FAULT_INPUT16 || f->kind == QTX_FAULT_WEIGHT16;
  if ((in_kind || w_kind) && (f->bit < 0 || f->bit > 7)) return fail(QTX_E_INVALID, "fault bit %d", f->bit);
  auto bad_idx = [&](long r, long nr, long cc, long nc) {
    return fail(QTX_E_INVALID, "fault index (%ld, %ld) outside [%ld, %ld]", r, cc, nr, nc);
  };
  const long row = f->row, col = f->col;
  const bool attn_self = lin == QTX_LIN_QK || lin == QTX_LIN_PV;
  const bool attn_cross = lin == QTX_LIN_CQK || lin == QTX_LIN_CPV;
  if (attn_self || attn_cross) {
    if (attn_cross && module != 1) return fail(QTX_E_INVALID, "fault linear %d", lin);
    const long sq = Sq, sk = attn_cross ? Ss : Sq, H = c.n_heads;
    if (sk > 512) return fail(QTX_E_UNSUPPORTED, "attention fault with %ld keys", sk);
    const bool qk = lin == QTX_LIN_QK || lin == QTX_LIN_CQK;
    long nr, nc, wmax;
    if (f->kind == QTX_FAULT_OUTPUT) { nr = B * sq; nc = qk ? H * sk : H * 64; wmax = 0; }
    else if (in_kind) { nr = B * sq; nc = qk ? H * 64 : H * sk; wmax = qk ? sk : 64; }
    else { nr = B * sk; nc = H * 64; wmax = sq; }
    if (row < 0 || row >= nr || col < 0 || col >= nc) return bad_idx(row, nr, col, nc);
    if (win && (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > wmax))
      return fail(QTX_E_INVALID, "fault window [%ld, +%d) outside %ld", (long)f->win_start, f->win_len, wmax);
    return QTX_OK;
  }
  const bool enc_ok = lin == QTX_LIN_Q || lin == QTX_LIN_K || lin == QTX_LIN_V || lin == QTX_LIN_O ||
                      lin == QTX_LIN_FFN1 || lin == QTX_LIN_FFN2;
  const bool dec_ok = enc_ok || (lin >= QTX_LIN_CQ && lin <= QTX_LIN_CO);
  if (!(module == 0 ? enc_ok : dec_ok)) return fail(QTX_E_INVALID, "fault linear %d", lin);
  const long rows = (lin == QTX_LIN_CK || lin == QTX_LIN_CV) ? Ms : M;
  const long K = lin == QTX_LIN_FFN2 ? c.d_ff : c.d_model;
  const long N = lin == QTX_LIN_FFN1 ? c.d_ff : c.d_model;
  if (in_kind && (row < 0 || row >= rows || col < 0 || col >= K)) return bad_idx(row, rows, col, K);
  if (w_kind && (row < 0 || row >= N || col < 0 || col >= K)) return bad_idx(row, N, col, K);
  if (f->kind == QTX_FAULT_OUTPUT && (row < 0 || row >= rows || col < 0 || col >= N))
    return bad_idx(row, rows, col, N);
  if (f->kind == QTX_FAULT_INPUT16 &&
      (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > N))
    return fail(QTX_E_INVALID, "INPUT16 window");
  if (f->kind == QTX_FAULT_WEIGHT16 &&
      (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > rows))
    return fail(QTX_E_INVALID, "WEIGHT16 window");
  return QTX_OK;
}

// The fused FFN launch (qtx_ffn.hip) replaces the one-pass FFN1 + the FFN2 row GEMM on the
// KP path from ffn_fused_min_m rows (QTX_FFN_FUSED_MIN_M; QTX_NO_FFN_FUSED: never): one
// workgroup per 128 rows, so below ~1 block per CU the split launches use the chip better.
bool ffn_fused_ok(const EncLayer& L, long M, bool kp) {
  return kp && L.ffn && !knobs().no_ffn_fused && M >= knobs().ffn_fused_min_m;
}

int encoder_run(const qtx_model* m, const float* x, const uint8_t* mask, int B, int S,
                float* out, Scratch& s, hipStream_t st, const qtx_fault* f = nullptr,
                hipEvent_t after_first = nullptr) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * S;
  if (x != s.x) HIPCHK(hipMemcpyAsync(s.x, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
  if (!row_path(c)) {
    for (int l = 0; l < c.n_layers; ++l) {
      const EncLayer& L = m->enc[l];
      auto fa = [&](GemmId gid) { return fault_for(f, 0, l, gid, M, c); };
      AttnFault af;
      const bool attn_f = attn_fault_for(f, 0, l, false, S, S, af);
      RC(self_attn_block(c, L.qkv, L.o, L.ln[0], s, B, S, mask, S, 0, false, st, fa(G_QKV),
                         fa(G_O), attn_f ? &af : nullptr));
      RC(ffn_block(c, L.w1, L.w2, L.ln[1], s, M, st, fa(G_FFN1), fa(G_FFN2)));
    }
    RC(ln_out(s.x, M, m->enc_norm, D, out, st));
    return QTX_OK;
  }
  // Every LayerNorm + per-token quantization after the first is fused into the epilogue of
  // the GEMM that produces the residual it normalizes (O-proj, FFN2); Q/K/V and the FFN
  // hidden are quantized in their GEMM's epilogue; the last FFN2 applies the final norm.
  // KP: the int8 activations between the kernels (LN output, attention context, FFN
  // hidden) live in the KP layout the row GEMM's 64-byte-step DMA reads as full lines
  // (qtx_common.h kp_off); the fault variants keep the row-major layout.
  const int NL = c.n_layers;
  const bool kp = (f == nullptr || f->kind == QTX_FAULT_NONE) && m->enc[0].qkv.qkp &&
                  !knobs().no_kp;
  RC(ln_quant(s.x, M, m->enc[0].ln[0], D, s.a8, s.sa, st, kp));
  for (int l = 0; l < NL; ++l) {
    const EncLayer& L = m->enc[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 0, l, gid, M, c); };
    // the FFN1 below in one pass: its exchange scratch (in s.y, which nothing between here
    // and it writes) zeroed by the Q/K/V launch instead of a kernel of its own
    const bool zero_ffn1 = kp && !ffn_fused_ok(L, M, kp) && ffn1_onepass(L.w1, M, kp, fa(G_FFN1));
    RC(row_quant(L.qkv, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_QKV), kp,
                 zero_ffn1 ? s.y : nullptr, zero_ffn1 ? ffn1_scratch16(M) : 0));
    if (l == 0 && after_first) HIPCHK(hipEventRecord(after_first, st));
    AttnArgs a = attn_args(s, B, S, S, S);
    a.mask = mask; a.m_bs = S; a.m_is = 0;
    a.c_ld = D;
    AttnFault af;
    const hipError_t ea = attn_fault_for(f, 0, l, false, S, S, af)
                              ? hipErrorNotSupported
                              : (knobs().no_attn_encq ? hipErrorNotSupported
                                                            : launch_attention_encq(a, s.a8, s.sa, st,
                                                                                    false, kp));
    if (attn_fault_for(f, 0, l, false, S, S, af)) {
      RC(attention_fault(a, af, M, D, s, st));
    } else if (ea == hipErrorNotSupported) {  // other shapes: fp32 context + quantization
      HIPCHK(launch_attention(a, st));
      RC(quant(s.ctx, D, M, D, s.a8, s.sa, st, kp));
    } else {
      HIPCHK(ea);
    }
    RC(row_res_ln(L.o, s.a8, s.sa, M, s.x, L.ln[1], s.a8, s.sa, nullptr, st, fa(G_O), kp));
    if (ffn_fused_ok(L, M, kp)) {
      // the FFN sublayer in one launch (k_ffn_fused): the hidden stays on chip; each
      // workgroup reads its rows of a8 / sa before it writes them (the next LN's codes)
      FfnArgs g{};
      g.A = s.a8; g.sa = s.sa; g.wf = L.ffn;
      g.sw1 = L.w1.s; g.b1 = L.w1.b; g.sw2 = L.w2.s; g.b2 = L.w2.b;
      g.x = s.x; g.M = M; g.F = c.d_ff;
      if (l + 1 < NL) {
        g.ln_a = m->enc[l + 1].ln[0][0]; g.ln_b = m->enc[l + 1].ln[0][1];
        g.lnq = s.a8; g.lns = s.sa;
      } else {
        g.ln_a = m->enc_norm[0]; g.ln_b = m->enc_norm[1]; g.lnout = out;
      }
      HIPCHK(launch_ffn_fused(g, st));
      continue;
    }
    RC(row_ffn1(c, L.w1, s.a8, s.sa, M, s, st, fa(G_FFN1), kp, s.status, zero_ffn1));
    if (l + 1 < NL)
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc[l + 1].ln[0], s.a8, s.sa, nullptr, st,
                    fa(G_FFN2), kp, s.y));
    else
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->enc_norm, nullptr, nullptr, out, st,
                    fa(G_FFN2), kp, s.y));
  }
  return QTX_OK;
}

// Encoder sub-batch pipelining: a batch of >= 256 sentences runs as two halves on two
// streams, the second half one kernel behind, so the HBM-bound epilogues (residual +
// LayerNorm) of one half overlap the MFMA / VALU-bound kernels (attention, FFN) of the
// other on different CUs.  Results are identical (rows are independent).
// (not with the one-pass FFN1, which makes the layer's kernels MFMA / exchange-bound rather
// than HBM-bound: the split measured no gain before it, 2.07 vs 2.05 ms)
bool wsx_on();
bool enc_split(int B) { return B >= 256 && !knobs().enc_nosplit && !wsx_on(); }

size_t enc_ws(const qtx_config& c, int B, int S) {
  Arena ar;
  carve_scratch(ar, c, (long)B * S);
  if (enc_split(B)) {
    Arena a2;
    carve_scratch(a2, c, (long)(B / 2) * S);
    carve_scratch(a2, c, (long)(B - B / 2) * S);
    ar.used = std::max(ar.used, a2.used);
  }
  return align_up(ar.used);
}

// (CrossKV / carve_cross, quantized memory + cross K/V for all layers: qtx_carve.h)

// memory -> per-layer cross K/V (get_quantized_model.py:160-168: K/V outputs quantized)
int cross_kv(const qtx_model* m, const float* memory, int Ms, CrossKV& x, hipStream_t st,
             const qtx_fault* f = nullptr) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  RC(quant(memory, D, Ms, D, x.am8, x.sam, st));
  bool ckv_fault = false;
  for (int l = 0; l < c.n_layers; ++l) ckv_fault |= fault_for(f, 1, l, G_CKV, Ms, c).kind != FK_NONE;
  if (row_path(c) && D == 512 && !ckv_fault) {
    // every layer's K and V in ONE row GEMM (N = n_layers * 2 * 512): its 512-column tiles
    // are the layers' K / V, each quantized per token in the epilogue exactly as the
    // per-layer launches below (decode prologue: 6 launches of 36 workgroups -> one of 216)
    RC(row_quant(m->ckv_all, x.am8, x.sam, Ms, x.k8[0], x.sk[0], st));
    return QTX_OK;
  }
  for (int l = 0; l < c.n_layers; ++l) {
    if (row_path(c)) {     // K and V tiles quantized in the GEMM epilogue
      RC(row_quant(m->dec[l].ckv, x.am8, x.sam, Ms, x.k8[l], x.sk[l], st,
                   fault_for(f, 1, l, G_CKV, Ms, c)));
      continue;
    }
    RC(linear(c, m->dec[l].ckv, x.am8, x.sam, Ms, 0, nullptr, x.y, 2 * D, st,
              fault_for(f, 1, l, G_CKV, Ms, c)));
    RC(quant(x.y, 2 * D, Ms, D, x.k8[l], x.sk[l], st));
    RC(quant(x.y + D, 2 * D, Ms, D, x.v8[l], x.sv[l], st));
  }
  return QTX_OK;
}

// Cross-attention sublayer: x += O(attn(LN(x) -> Q, memory -> K/V)), decoder.py:32
int cross_attn_block(const qtx_model* m, const DecLayer& L, int l, Scratch& s,
                     const CrossKV& x, int B, int T, int S, const uint8_t* src_mask,
                     hipStream_t st, const FaultArgs& fcq = FaultArgs{},
                     const FaultArgs& fco = FaultArgs{}, const AttnFault* af = nullptr) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  RC(ln_quant(s.x, M, L.ln[1], D, s.a8, s.sa, st));
  RC(linear(c, L.cq, s.a8, s.sa, M, 0, nullptr, s.y, D, st, fcq));
  RC(quant(s.y, D, M, D, s.q8, s.sq, st));
  AttnArgs a = attn_args(s, B, T, S, S);
  a.k = x.k8[l]; a.sk = x.sk[l]; a.v = x.v8[l]; a.sv = x.sv[l];
  a.mask = src_mask; a.m_bs = S; a.m_is = 0;
  a.dec = 1;
  HIPCHK(launch_attention(a, st));
  if (af) HIPCHK(launch_attn_fault_rows(a, *af, st));
  RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
  RC(linear(c, L.co, s.a8, s.sa, M, EPI_RESIDUAL, s.x, s.x, D, st, fco));
  return QTX_OK;
}

size_t dec_ws(const qtx_config& c, int B, int T, int S) {
  Arena ar;
  carve_scratch(ar, c, (long)B * T);
  carve_cross(ar, c, (long)B * S);
  return align_up(ar.used);
}

// (GreedyWS, the greedy decode workspace, and BeamTail, the beam step's tail: qtx_carve.h)

// Sub-batch split of the fused decode.  Sentences are independent (per-token quantization:
// no value depends on another sentence), and one sub-batch's step is a chain of ~50
// latency-bound kernels that each occupy a fraction of the 256 CUs.  G sub-batch graphs
// on G streams (ms per decode, profiles/r03_concurrency.md): B = 32: 14.5 / 21.0 for
// G = 1 / 2; B = 256: 34.9 / 35.8; B = 512: 59.0 / 51.9 — two chains of 256 rows overlap
// as well as two processes of 256 sentences each (50.6), two of 128 or 16 do not gain.
// Default G = 2 from B = 512, else 1; QTX_DECODE_GROUPS overrides it (experiments).
struct Groups {
  int G, Bg;   // G groups of Bg rows (the last one may be shorter)
  int b0(int i) const { return i * Bg; }
  int rows(int i, int B) const { return std::min(B, (i + 1) * Bg) - i * Bg; }
};
Groups decode_groups(int B) {
  int G = B >= 512 ? 2 : 1;
  if (knobs().decode_groups > 0) G = knobs().decode_groups;
  G = std::max(1, std::min(std::min(G, QTX_MAX_GROUPS), B));
  const int Bg = (B + G - 1) / G;
  return Groups{(B + Bg - 1) / Bg, Bg};   // no empty group
}

// scored: the scores follow everything else, so the plain layout (and size) is a prefix
GreedyWS carve_greedy(Arena& ar, const qtx_config& c, int B, int S, int max_len,
                      bool scored = false) {
  GreedyWS g;
  const int D = c.d_model;
  g.enc = carve_scratch(ar, c, (long)B * S);
  g.dec = carve_scratch(ar, c, B);
  g.cross = carve_cross(ar, c, (long)B * S);
  // the cross values regrouped once per decode (layer stride: B * ceil(S/4) * 4 * D bytes)
  int8_t* cvg = ar.take<int8_t>((size_t)c.n_layers * B * ((S + 3) & ~3) * D);
  for (int l = 0; l < c.n_layers; ++l) {
    g.cvg.push_back(cvg ? cvg + (size_t)l * B * ((S + 3) & ~3) * D : nullptr);
    g.kc.push_back(ar.take<int8_t>((size_t)B * max_len * D));
    g.skc.push_back(ar.take<float>((size_t)B * max_len));
    g.vc.push_back(ar.take<int8_t>((size_t)B * ((max_len + 3) & ~3) * D));
    g.svc.push_back(ar.take<float>((size_t)B * max_len));
  }
  g.memory = ar.take<float>((size_t)B * S * D);
  g.xo = ar.take<float>((size_t)B * D);
  g.logits = ar.take<float>((size_t)B * c.tgt_vocab);
  g.step = ar.take<int>(4);
  g.pmax_a = ar.take<float>((size_t)8 * B);
  g.pmax_f = ar.take<float>((size_t)(c.d_ff / 16) * B);
  const Groups gr = decode_groups(B);
  g.grp.push_back(g.dec);
  for (int i = 1; i < gr.G; ++i) g.grp.push_back(carve_scratch(ar, c, gr.Bg));
  g.gsteps = ar.take<int>(4 * QTX_MAX_GROUPS);
  g.ids = ar.take<int64_t>((size_t)B * max_len);
  g.mask = ar.take<uint8_t>((size_t)B * S);
  g.rec = ar.take<float>((size_t)B * ((c.tgt_vocab + 15) / 16) * 4);
  if (scored) {
    g.top_ids = ar.take<int64_t>((size_t)B * (max_len - 1) * 2);
    g.top_logp = ar.take<float>((size_t)B * (max_len - 1) * 2);
  }
  return g;
}

// The workspace of sub-batch i (rows b0 ..): every per-sentence buffer offset by b0.
GreedyWS group_view(const GreedyWS& g, const qtx_config& c, int i, int b0, int S,
                    int max_len) {
  const long D = c.d_model;
  GreedyWS v = g;
  v.dec = g.grp[i];
  for (int l = 0; l < c.n_layers; ++l) {
    v.kc[l] += b0 * max_len * D; v.vc[l] += b0 * ((max_len + 3) & ~3) * D;
    v.skc[l] += b0 * max_len; v.svc[l] += b0 * max_len;
    v.cross.k8[l] += b0 * S * D; v.cross.v8[l] += b0 * S * D;
    v.cvg[l] += b0 * ((S + 3) & ~3) * D;
    v.cross.sk[l] += b0 * S; v.cross.sv[l] += b0 * S;
  }
  v.logits += (long)b0 * c.tgt_vocab;
  v.rec += (long)b0 * ((c.tgt_vocab + 15) / 16) * 4;
  v.pmax_a += (long)8 * b0;               // each sub-batch: its own [P][rows] block
  v.pmax_f += (long)(c.d_ff / 16) * b0;
  v.step = g.gsteps + 4 * i;
  if (g.top_ids) {
    v.top_ids += (long)b0 * (max_len - 1) * 2;
    v.top_logp += (long)b0 * (max_len - 1) * 2;
  }
  return v;
}


// ---- fused decode step (M = B rows, keys <= 128) ----------------------------------------
// Its kernels exist for the flagship shapes only: the skinny GEMM takes K = 512 or 2048
// (FFN2: K = d_ff; launch_skinny) and the argmax / top-2 tails a vocabulary of at most
// ARG_MAXV.  Every other config qtx_model_create accepts decodes with the unfused step,
// whose kernels have no such limit (greedy_run decides before anything is captured).
bool fused_step_ok(const qtx_config& c) {
  return (c.d_ff == 512 || c.d_ff == 2048) && c.tgt_vocab <= ARG_MAXV;
}

SkinnyArgs skinny(int wbits, const QLin& L, int M, int amode, int flags, float* out, long ldo) {
  SkinnyArgs s{};
  // wbits 8 on a 4-bit model: its unpacked int8 copy
  s.amode = amode; s.W = wbits == 8 ? L.w8() : L.q; s.ldw = wbits == 8 ? L.K : L.K / 2;
  s.sw = L.s; s.bias = L.b;
  s.out = out; s.ldo = ldo; s.M = M; s.N = L.N; s.K = L.K; s.flags = flags;
  return s;
}

// The beam step's tail on the step's R = B * beam rows: the selection (scores, parents, tokens,
// next inputs, position + 1, rows still live), then the caches of every layer by parent.
int beam_tail(const qtx_model* m, GreedyWS& g, int R, int max_len, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const BeamTail& b = *g.beam;
  HIPCHK(launch_beam_select(g.logits, R / b.K, b.K, c.tgt_vocab, b.eos, b.pad, max_len, g.step,
                            b.st.score, b.st.fin, b.st.len, b.st.parent, b.st.bp_par,
                            b.st.bp_tok, m->tgt_lut, m->pe, c.max_len, g.dec.x, st));
  HIPCHK(launch_beam_reorder(b.kc0, b.vc0, b.skc0, b.svc0, R / b.K, b.K, max_len, c.n_layers,
                             b.k_ls, b.v_ls, b.s_ls, b.grouped ? 1 : 0, g.step, b.st.parent, st));
  return QTX_OK;
}

// One KV-cached decoder step for every sentence, 8 kernels per layer + 2:
//   [LN+QKV] [self-attn] [O+res] [LN+Qc] [cross-attn] [Oc+res] [LN+FFN1+relu] [FFN2+res]
//   [final LN + generator] [log_softmax/argmax + next embedding + step++]
// Reads the position from g.step (device), so it can be captured once and replayed.
// t_host: the step's position when the caller knows it at launch or capture time (the
// whole decode in one graph, or eager launches), else -1
int greedy_step_fused(const qtx_model* m, GreedyWS& g, int B, int S, int max_len,
                      int64_t* ids, const uint8_t* src_mask, hipStream_t st, int t_host) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, F = c.d_ff;
  const int wb = m->dec[0].qkv.q8 && !knobs().int4_packed ? 8 : c.weight_bits;
  // the FFN hidden quantized once by its own kernel (instead of in every FFN2 workgroup's
  // prologue from FFN1's partial maxima) from 96 rows on: measured faster there despite the
  // extra launch (profiles/r05_rb_sweep.md), slower at B = 32
  const bool ffn_qkernel = knobs().ffn_qkernel || B >= 96;
  const bool fused_ln = !knobs().split_ln;
  // O / Oc form the context's per-token maximum from the rows they load (A_F32R) instead of
  // the attention's per-head maxima (QTX_ATTN_PMAX=1: the per-head maxima, A_F32Q)
  const bool own_max = !knobs().attn_pmax;
  // likewise FFN2 forms the hidden's per-token maximum itself (QTX_FFN_PMAX=1: from FFN1's
  // per-tile maxima, FFN1 with the maxima epilogue)
  const bool ffn_own = !knobs().ffn_pmax;
  // the position from the host (self-attention, argmax + embedding; the device counter then
  // neither read nor advanced) or from the device counter (QTX_DEVICE_STEP, or a step replayed
  // at several positions)
  const bool host_pos = t_host >= 0 && !knobs().device_step;
  // The tail folded into the next step's first launch (plain decode, int8 kernels, positions
  // from the host; QTX_NO_TAIL_FOLD: never): the generator also writes per-strip top-2 records,
  // and from step 1 on layer 0's LN+QKV launch decides the previous step's token from them,
  // embeds it and stores ids / x itself (launch_skinny_tok) — a step is then 49 launches.
  // Only the last step still ends with the argmax kernel.
  const bool fold = !knobs().no_tail_fold && host_pos && !g.top_ids && wb == 8 && fused_ln &&
                    !knobs().ablate && !knobs().dbg_tail && !g.no_fold && !g.beam;
  Scratch& s = g.dec;
  // Timing experiments only (wrong results): QTX_ABLATE=<bitmask> drops kernel classes
  // from the step (replaced by an empty kernel with QTX_ABLATE_NOP=1) to measure what
  // each costs inside the real graph.  1 LN, 2 QKV/Qc, 4 self-attn, 8 cross-attn,
  // 16 O/Oc, 32 FFN1, 64 h-quant, 128 FFN2, 256 tail.
  const int abl = knobs().ablate;           // always 0 outside the QTX_DIAG build
  const bool abl_nop = knobs().ablate_nop;
#define QTX_RUN(bit, launch)                   \
  do {                                         \
    if (abl & (bit)) {                         \
      if (abl_nop) HIPCHK(launch_nop(st));     \
    } else {                                   \
      HIPCHK(launch);                          \
    }                                          \
  } while (0)
  // out = epilogue(quant(LN(x)) . W^T): the LayerNorm + per-token quant is recomputed in
  // the prologue of every GEMM workgroup (4 rows each, A_LN) — cheaper than its own kernel
  // launch; QTX_SPLIT_LN=1 restores the separate LN kernel (timing experiments).
#define QTX_RUNRC(bit, expr)                   \
  do {                                         \
    if (abl & (bit)) {                         \
      if (abl_nop) HIPCHK(launch_nop(st));     \
    } else {                                   \
      RC(expr);                                \
    }                                          \
  } while (0)
  auto ln_linear = [&](const QLin& W, const float* const* ln, int flags, float* out,
                       long ldo, int bit) -> int {
    SkinnyArgs k = skinny(wb, W, B, fused_ln ? A_LN : A_I8, flags, out, ldo);
    if (flags & EPI_ROWMAX) k.pmax_out = g.pmax_f;
    if (fused_ln) {
      k.X = s.x; k.ldx = D; k.ln_a = ln[0]; k.ln_b = ln[1];
    } else {
      QTX_RUNRC(1, ln_quant(s.x, B, ln, D, s.a8, s.sa, st));
      k.A = s.a8; k.sa = s.sa;
    }
    QTX_RUN(bit, launch_skinny(k, wb, st));
    return QTX_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    SkinnyArgs a;
    if (fold && l == 0 && t_host >= 1) {
      SkinnyArgs k = skinny(wb, L.qkv, B, A_LN, 0, s.y, 3 * D);
      k.ln_a = L.ln[0][0]; k.ln_b = L.ln[0][1];
      TokArgs tk{};
      tk.rec = g.rec; tk.logits = g.logits; tk.V = c.tgt_vocab; tk.lut = m->tgt_lut;
      tk.pe = m->pe; tk.max_pos = c.max_len; tk.pos = t_host; tk.ids = ids; tk.ids_bs = max_len;
      tk.xres = s.x;
      HIPCHK(launch_skinny_tok(k, tk, st));
    } else {
      RC(ln_linear(L.qkv, L.ln[0], 0, s.y, 3 * D, 2));
    }
    DecAttnArgs at{};
    at.y = s.y; at.ldy = 3 * D; at.kv_new = 1; at.step = g.step;
    at.kc = g.kc[l]; at.vc = g.vc[l]; at.skc = g.skc[l]; at.svc = g.svc[l]; at.kv_bs = max_len;
    at.ctx = s.ctx; at.pmax = own_max ? nullptr : g.pmax_a; at.B = B;
    at.host_step1 = host_pos ? t_host + 1 : 0;
    QTX_RUN(4, launch_dec_attn(at, B, st));
    a = skinny(wb, L.o, B, own_max ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);   // quantizes ctx per token
    a.X = s.ctx; a.ldx = D; a.pmax_in = g.pmax_a; a.pmax_n = 8; a.res = s.x; a.ldr = D;
    QTX_RUN(16, launch_skinny(a, wb, st));
    RC(ln_linear(L.cq, L.ln[1], 0, s.y, D, 2));
    at = DecAttnArgs{};
    at.y = s.y; at.ldy = D; at.kv_new = 0; at.S = S; at.mask = src_mask;
    at.kc = g.cross.k8[l]; at.vc = g.cvg[l]; at.skc = g.cross.sk[l];
    at.svc = g.cross.sv[l]; at.kv_bs = S;
    at.ctx = s.ctx; at.pmax = own_max ? nullptr : g.pmax_a; at.B = B;
    QTX_RUN(8, launch_dec_attn(at, B, st));
    a = skinny(wb, L.co, B, own_max ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);
    a.X = s.ctx; a.ldx = D; a.pmax_in = g.pmax_a; a.pmax_n = 8; a.res = s.x; a.ldr = D;
    QTX_RUN(16, launch_skinny(a, wb, st));
    if (!ffn_qkernel) {   // FFN2 quantizes h itself (from its rows, or FFN1's per-tile maxima)
      RC(ln_linear(L.w1, L.ln[2], ffn_own ? EPI_RELU : EPI_RELU | EPI_ROWMAX, s.y, F, 32));
      a = skinny(wb, L.w2, B, ffn_own ? A_F32R : A_F32Q, EPI_RESIDUAL, s.x, D);
      a.X = s.y; a.ldx = F; a.pmax_in = g.pmax_f; a.pmax_n = F / 16; a.res = s.x; a.ldr = D;
      QTX_RUN(128, launch_skinny(a, wb, st));
    } else {              // one wave per row quantizes h (quant_linear.py:30-43), then FFN2
      RC(ln_linear(L.w1, L.ln[2], EPI_RELU, s.y, F, 32));
      if (F == 2048 && !knobs().hquant_rows)   // one 4-wave workgroup per row
        QTX_RUN(64, launch_quant_h2048(s.y, F, B, s.a8, s.sa, st));
      else
        QTX_RUNRC(64, quant(s.y, F, B, F, s.a8, s.sa, st));
      a = skinny(wb, L.w2, B, A_I8, EPI_RESIDUAL, s.x, D);
      a.A = s.a8; a.sa = s.sa; a.res = s.x; a.ldr = D;
      QTX_RUN(128, launch_skinny(a, wb, st));
    }
  }
  if (knobs().dbg_tail) {   // bisection aid (QTX_DIAG build): reference-shaped tail kernels
    RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
    HIPCHK(launch_generator(g.xo, D, B, m->gen_w, m->gen_b, c.tgt_vocab, g.logits, st));
    HIPCHK(launch_logsoftmax_argmax(g.logits, B, c.tgt_vocab, nullptr, ids, max_len, g.step,
                                    1, st));
    HIPCHK(launch_step_inc(g.step, st));
    HIPCHK(launch_embed(ids, max_len, B, 1, g.step, 0, m->tgt_lut, c.tgt_vocab, m->pe,
                        c.max_len, s.x, D, st));
    return QTX_OK;
  }
  QTX_RUN(256, launch_generator_mfma(s.x, D, B, m->dec_norm[0], m->dec_norm[1], m->gen_wt,
                                     m->gen_b, c.tgt_vocab, g.logits, st, fold ? g.rec : nullptr));
  if (fold && t_host + 2 < max_len) return QTX_OK;   // the next step's first launch is the tail
  if (g.beam) return beam_tail(m, g, B, max_len, st);
  if (g.top_ids)   // scored decode: the tail that also writes the step's two best (id, logp)
    QTX_RUN(256, launch_top2_embed(g.logits, B, c.tgt_vocab, ids, max_len, g.top_ids, g.top_logp,
                                   g.step, reinterpret_cast<unsigned*>(g.step + 1), m->tgt_lut,
                                   m->pe, c.max_len, s.x, st, host_pos ? t_host + 1 : 0));
  else
    QTX_RUN(256, launch_argmax_embed(g.logits, B, c.tgt_vocab, ids, max_len, g.step,
                                     reinterpret_cast<unsigned*>(g.step + 1), m->tgt_lut, m->pe,
                                     c.max_len, s.x, st, host_pos ? t_host + 1 : 0));
  return QTX_OK;
#undef QTX_RUN
#undef QTX_RUNRC
}

// The reference-shaped unfused step (any key count up to 512).
int greedy_step_unfused(const qtx_model* m, GreedyWS& g, int B, int S, int max_len,
                        int64_t* ids, const uint8_t* src_mask, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  Scratch& s = g.dec;
  if (!g.beam)   // (the beam step's input row comes from the previous step's select)
    HIPCHK(launch_embed(ids, max_len, B, 1, g.step, 0, m->tgt_lut, c.tgt_vocab, m->pe,
                        c.max_len, s.x, D, st));
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    RC(ln_quant(s.x, B, L.ln[0], D, s.a8, s.sa, st));
    RC(linear(c, L.qkv, s.a8, s.sa, B, 0, nullptr, s.y, 3 * D, st));
    RC(quant(s.y, 3 * D, B, D, s.q8, s.sq, st));
    RowArgs kr = rows_quant(s.y + D, 3 * D, B, D, g.kc[l], g.skc[l]);
    kr.rpb = 1; kr.dst_bstride = max_len; kr.dst_off_dev = g.step;
    HIPCHK(launch_rows(kr, st));
    RowArgs vr = rows_quant(s.y + 2 * D, 3 * D, B, D, g.vc[l], g.svc[l]);
    vr.rpb = 1; vr.dst_bstride = max_len; vr.dst_off_dev = g.step;
    HIPCHK(launch_rows(vr, st));
    AttnArgs a = attn_args(s, B, 1, 0, max_len);
    a.k = g.kc[l]; a.sk = g.skc[l]; a.v = g.vc[l]; a.sv = g.svc[l];
    a.sk_dev = g.step; a.sk_add = 1;
    a.dec = 1;
    HIPCHK(launch_attention(a, st));
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(linear(c, L.o, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st));
    RC(cross_attn_block(m, L, l, s, g.cross, B, 1, S, src_mask, st));
    RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, B, st));
  }
  RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
  HIPCHK(launch_generator(g.xo, D, B, m->gen_w, m->gen_b, c.tgt_vocab, g.logits, st));
  if (g.beam) return beam_tail(m, g, B, max_len, st);   // (it advances the position itself)
  if (g.top_ids)
    HIPCHK(launch_logsoftmax_top2(g.logits, B, c.tgt_vocab, ids, max_len, g.step, 1, g.top_ids,
                                  g.top_logp, max_len - 1, st));
  else
    HIPCHK(launch_logsoftmax_argmax(g.logits, B, c.tgt_vocab, nullptr, ids, max_len, g.step, 1,
                                    st));
  HIPCHK(launch_step_inc(g.step, st));
  return QTX_OK;
}


// The decoder stack over M = B * T rows: s.x holds the embedded targets, x the cross K/V
// (cross_kv); out [M, D] = the final LayerNorm's output.  f: one optional fault.
int decoder_body(const qtx_model* m, Scratch& s, const CrossKV& x, const uint8_t* src_mask,
                 const uint8_t* tgt_mask, long tm_bs, int B, int T, int S, float* out,
                 const qtx_fault* f, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  if (!row_path(c)) {
    for (int l = 0; l < c.n_layers; ++l) {
      const DecLayer& L = m->dec[l];
      auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, M, c); };
      AttnFault af;
      const bool self_f = attn_fault_for(f, 1, l, false, T, T, af);
      RC(self_attn_block(c, L.qkv, L.o, L.ln[0], s, B, T, tgt_mask, tm_bs, T, true, st,
                         fa(G_QKV), fa(G_O), self_f ? &af : nullptr));
      const bool cross_f = attn_fault_for(f, 1, l, true, T, S, af);
      RC(cross_attn_block(m, L, l, s, x, B, T, S, src_mask, st, fa(G_CQ), fa(G_CO),
                          cross_f ? &af : nullptr));
      RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, M, st, fa(G_FFN1), fa(G_FFN2)));
    }
    RC(ln_out(s.x, M, m->dec_norm, D, out, st));
    return QTX_OK;
  }
  // LayerNorm + quant of each sublayer's input fused into the previous residual GEMM
  // (as encoder_run); the last FFN2 applies the final decoder norm
  const int NL = c.n_layers;
  RC(ln_quant(s.x, M, m->dec[0].ln[0], D, s.a8, s.sa, st));
  for (int l = 0; l < NL; ++l) {
    const DecLayer& L = m->dec[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, M, c); };
    RC(row_quant(L.qkv, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_QKV)));
    AttnArgs a = attn_args(s, B, T, T, T);
    a.mask = tgt_mask; a.m_bs = tm_bs; a.m_is = T;
    a.c_ld = D;
    a.dec = 1;
    AttnFault af;
    if (attn_fault_for(f, 1, l, false, T, T, af)) {
      RC(attention_fault(a, af, M, D, s, st));
    } else {
      const hipError_t ea = knobs().no_attn_encq ? hipErrorNotSupported
                                                       : launch_attention_encq(a, s.a8, s.sa, st);
      if (ea == hipErrorNotSupported) {  // other shapes: fp32 context + quantization kernel
        HIPCHK(launch_attention(a, st));
        RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
      } else {
        HIPCHK(ea);
      }
    }
    RC(row_res_ln(L.o, s.a8, s.sa, M, s.x, L.ln[1], s.a8, s.sa, nullptr, st, fa(G_O)));
    RC(row_quant(L.cq, s.a8, s.sa, M, s.q8, s.sq, st, fa(G_CQ)));
    a = attn_args(s, B, T, S, S);
    a.k = x.k8[l]; a.sk = x.sk[l]; a.v = x.v8[l]; a.sv = x.sv[l];
    a.mask = src_mask; a.m_bs = S; a.m_is = 0;
    a.dec = 1;
    if (attn_fault_for(f, 1, l, true, T, S, af)) {
      RC(attention_fault(a, af, M, D, s, st));
    } else {
      HIPCHK(launch_attention(a, st));
      RC(quant(s.ctx, D, M, D, s.a8, s.sa, st));
    }
    RC(row_res_ln(L.co, s.a8, s.sa, M, s.x, L.ln[2], s.a8, s.sa, nullptr, st, fa(G_CO)));
    RC(row_ffn1(c, L.w1, s.a8, s.sa, M, s, st, fa(G_FFN1)));
    if (l + 1 < NL)
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->dec[l + 1].ln[0], s.a8, s.sa, nullptr, st, fa(G_FFN2)));
    else
      RC(row_res_ln(L.w2, s.h8, s.sh, M, s.x, m->dec_norm, nullptr, nullptr, out, st, fa(G_FFN2)));
  }
  return QTX_OK;
}

int greedy_run(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S, int max_len,
               int64_t start, const qtx_fault* f, hipStream_t st);

}  // namespace

extern "C" {

size_t qtx_encoder_workspace_size(const qtx_model* m, int32_t B, int32_t S) {
  return m ? enc_ws(m->cfg, B, S) : 0;
}
size_t qtx_decoder_workspace_size(const qtx_model* m, int32_t B, int32_t T, int32_t S) {
  return m ? dec_ws(m->cfg, B, T, S) : 0;
}
size_t qtx_greedy_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len) {
  if (!m) return 0;
  Arena ar;
  carve_greedy(ar, m->cfg, B, S, max_len);
  return align_up(ar.used);
}
size_t qtx_greedy_scored_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len) {
  if (!m || max_len < 1) return 0;
  Arena ar;
  carve_greedy(ar, m->cfg, B, S, max_len, true);
  return align_up(ar.used);
}

int32_t qtx_encoder_forward_fault(const qtx_model* m, const float* x, const uint8_t* src_mask,
                                  int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                                  const qtx_fault* f, void* stream) {
  if (!m || !x || !src_mask || !out || !ws) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || S <= 0 || S > 512) return fail(QTX_E_INVALID, "bad shape B=%d S=%d", B, S);
  if (ws_bytes < enc_ws(m->cfg, B, S)) return fail(QTX_E_WORKSPACE, "workspace too small");
  RC(check_fault(m, f, 0, B, S, 0));
  dfault_forget(m, ws);
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  hipStream_t st = (hipStream_t)stream;
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  if (!enc_split(B) || (f && f->kind != QTX_FAULT_NONE)) {
    Scratch s = carve_scratch(ar, m->cfg, (long)B * S);
    s.status = cst;
    return encoder_run(m, x, src_mask, B, S, out, s, st, f);
  }
  // The model's second stream and its three events are shared by every caller: the lock
  // is held across the whole record / wait sequence, so two threads' fork, lag and join
  // records cannot interleave (a wait always pairs with its own call's record).
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lk(mm->mu);
  DeviceGuard dg(mm->device);
  if (!mm->estream) {
    HIPCHK(hipStreamCreateWithFlags(&mm->estream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_lag, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&mm->ev_join, hipEventDisableTiming));
  }
  const int B0 = B / 2, B1 = B - B0;
  const long D = m->cfg.d_model;
  Scratch s0 = carve_scratch(ar, m->cfg, (long)B0 * S);
  Scratch s1 = carve_scratch(ar, m->cfg, (long)B1 * S);
  s0.status = s1.status = cst;
  // half 1 starts when half 0's first layer has passed its QKV GEMM (ev_lag)
  HIPCHK(hipEventRecord(mm->ev_fork, st));
  HIPCHK(hipStreamWaitEvent(mm->estream, mm->ev_fork, 0));
  RC(encoder_run(m, x, src_mask, B0, S, out, s0, st, nullptr, mm->ev_lag));
  HIPCHK(hipStreamWaitEvent(mm->estream, mm->ev_lag, 0));
  RC(encoder_run(m, x + (long)B0 * S * D, src_mask + (long)B0 * S, B1, S, out + (long)B0 * S * D,
                 s1, mm->estream, nullptr));
  HIPCHK(hipEventRecord(mm->ev_join, mm->estream));
  HIPCHK(hipStreamWaitEvent(st, mm->ev_join, 0));
  return QTX_OK;
}

int32_t qtx_encoder_forward(const qtx_model* m, const float* x, const uint8_t* src_mask,
                            int32_t B, int32_t S, float* out, void* ws, size_t ws_bytes,
                            void* stream) {
  return qtx_encoder_forward_fault(m, x, src_mask, B, S, out, ws, ws_bytes, nullptr, stream);
}

int32_t qtx_decoder_forward_fault(const qtx_model* m, const float* y, const float* memory,
                                  const uint8_t* src_mask, const uint8_t* tgt_mask,
                                  int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                                  float* out, void* ws, size_t ws_bytes, const qtx_fault* f,
                                  void* stream) {
  if (!m || !y || !memory || !src_mask || !tgt_mask || !out || !ws)
    return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || T <= 0 || S <= 0 || T > 512 || S > 512)
    return fail(QTX_E_INVALID, "bad shape B=%d T=%d S=%d", B, T, S);
  if (ws_bytes < dec_ws(m->cfg, B, T, S)) return fail(QTX_E_WORKSPACE, "workspace too small");
  RC(check_fault(m, f, 1, B, T, S));
  dfault_forget(m, ws);
  hipStream_t st = (hipStream_t)stream;
  const qtx_config& c = m->cfg;
  const int D = c.d_model, M = B * T;
  // no decoder kernel sets a status word (the in-launch FFN1 exchange runs on the KP
  // encoder path only), so this call neither claims nor touches the thread's word: an
  // error an earlier encode left there stays until qtx_model_check reports it
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  Scratch s = carve_scratch(ar, c, M);
  CrossKV x = carve_cross(ar, c, (long)B * S);
  RC(cross_kv(m, memory, B * S, x, st, f));
  HIPCHK(hipMemcpyAsync(s.x, y, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
  return decoder_body(m, s, x, src_mask, tgt_mask, tgt_mask_batched ? (long)T * T : 0, B, T, S, out,
                      f, st);
}

int32_t qtx_decoder_forward(const qtx_model* m, const float* y, const float* memory,
                            const uint8_t* src_mask, const uint8_t* tgt_mask,
                            int32_t tgt_mask_batched, int32_t B, int32_t T, int32_t S,
                            float* out, void* ws, size_t ws_bytes, void* stream) {
  return qtx_decoder_forward_fault(m, y, memory, src_mask, tgt_mask, tgt_mask_batched, B, T, S,
                                   out, ws, ws_bytes, nullptr, stream);
}

int32_t qtx_embed(const qtx_model* m, int32_t which, const int64_t* ids, int32_t B, int32_t T,
                  int32_t pos0, float* out, void* stream) {
  if (!m || !ids || !out) return fail(QTX_E_INVALID, "null argument");
  if (pos0 < 0 || pos0 + T > m->cfg.max_len)
    return fail(QTX_E_INVALID, "positions exceed max_len %d", m->cfg.max_len);
  const float* lut = which ? m->tgt_lut : m->src_lut;
  const int vocab = which ? m->cfg.tgt_vocab : m->cfg.src_vocab;
  HIPCHK(launch_embed(ids, T, B, T, nullptr, pos0, lut, vocab, m->pe, m->cfg.max_len, out,
                      (long)T * m->cfg.d_model, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_generator(const qtx_model* m, const float* x, int32_t M, float* logp,
                      int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !ws) return fail(QTX_E_INVALID, "null argument");
  const int V = m->cfg.tgt_vocab;
  if (ws_bytes < (size_t)M * V * sizeof(float)) return fail(QTX_E_WORKSPACE, "ws too small");
  hipStream_t st = (hipStream_t)stream;
  float* logits = (float*)ws;   // the raw logits stay in ws[0 .. M*V) for the caller
  HIPCHK(launch_generator_mfma(x, m->cfg.d_model, M, nullptr, nullptr, m->gen_wt, m->gen_b, V,
                               logits, st));
  HIPCHK(launch_logsoftmax_argmax(logits, M, V, logp, ids, 1, nullptr, 0, st));
  return QTX_OK;
}

int32_t qtx_generator_top2(const qtx_model* m, const float* x, int32_t M, int64_t* top_ids,
                           float* top_logp, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !top_ids || !top_logp || !ws) return fail(QTX_E_INVALID, "null argument");
  const int V = m->cfg.tgt_vocab;
  if (V < 2) return fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", V);
  if (M <= 0) return QTX_OK;
  if (ws_bytes < (size_t)M * V * sizeof(float)) return fail(QTX_E_WORKSPACE, "ws too small");
  hipStream_t st = (hipStream_t)stream;
  float* logits = (float*)ws;   // the raw logits stay in ws[0 .. M*V) for the caller
  HIPCHK(launch_generator_mfma(x, m->cfg.d_model, M, nullptr, nullptr, m->gen_wt, m->gen_b, V,
                               logits, st));
  HIPCHK(launch_logsoftmax_top2(logits, M, V, nullptr, 0, nullptr, 0, top_ids, top_logp, 1, st));
  return QTX_OK;
}

// the plain (scored = false: top_ids / top_logp unused) and the scored greedy decode
static int32_t greedy_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                             int32_t B, int32_t S, int32_t max_len, int64_t start, int64_t* ids,
                             bool scored, int64_t* top_ids, float* top_logp, void* ws,
                             size_t ws_bytes, const qtx_fault* f, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws ||
      (scored && max_len > 1 && (!top_ids || !top_logp)))   // (max_len 1: no step, no entry)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if (scored && c.tgt_vocab < 2)
    return fail(QTX_E_INVALID, "scored decode needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (scored && knobs().dbg_tail)
    return fail(QTX_E_UNSUPPORTED, "scored decode: not with QTX_DBG_TAIL");
  if (ws_bytes < (scored ? qtx_greedy_scored_workspace_size(m, B, S, max_len)
                         : qtx_greedy_workspace_size(m, B, S, max_len)))
    return fail(QTX_E_WORKSPACE, "workspace too small");
  if (f && f->kind != QTX_FAULT_NONE && f->module != 0)
    return fail(QTX_E_UNSUPPORTED, "greedy decode takes encoder faults (decoder faults: "
                                   "qtx_decoder_forward_fault on the step's prefix)");
  RC(check_fault(m, f, 0, B, S, 0));
  dfault_forget(m, ws);
  hipStream_t st = (hipStream_t)stream;
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  GreedyWS g = carve_greedy(ar, c, B, S, max_len, scored);
  g.enc.status = cst;
  // the decode reads the workspace's copy of src_mask and writes the workspace's ids
  // (the captured graphs then depend on the workspace only); ids go out at the end
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_run(m, g, src, B, S, max_len, start, f, st));
  HIPCHK(hipMemcpyAsync(ids, g.ids, (size_t)B * max_len * sizeof(int64_t),
                        hipMemcpyDeviceToDevice, st));
  if (scored && max_len > 1) {   // the scores likewise
    const size_t n = (size_t)B * (max_len - 1) * 2;
    HIPCHK(hipMemcpyAsync(top_ids, g.top_ids, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, g.top_logp, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return QTX_OK;
}

int32_t qtx_greedy_decode_fault(const qtx_model* m, const int64_t* src,
                                const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                int64_t start, int64_t* ids, void* ws, size_t ws_bytes,
                                const qtx_fault* f, void* stream) {
  return greedy_decode(m, src, src_mask, B, S, max_len, start, ids, false, nullptr, nullptr, ws,
                       ws_bytes, f, stream);
}

int32_t qtx_greedy_decode_scored(const qtx_model* m, const int64_t* src,
                                 const uint8_t* src_mask, int32_t B, int32_t S, int32_t max_len,
                                 int64_t start, int64_t* ids, int64_t* top_ids, float* top_logp,
                                 void* ws, size_t ws_bytes, const qtx_fault* f, void* stream) {
  return greedy_decode(m, src, src_mask, B, S, max_len, start, ids, true, top_ids, top_logp, ws,
                       ws_bytes, f, stream);
}

int32_t qtx_model_check(const qtx_model* m, void* stream) {
  if (!m) return fail(QTX_E_INVALID, "null model");
  DeviceGuard dg(m->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned v = 0;
  unsigned* word = nullptr;
  for (const CallStatus& cs : t_calls.v)
    if (cs.m == m && cs.serial == m->serial) word = m->status + 4 * cs.slot;
  // no word: this thread has made no call on m that can raise a device error (the word is
  // per thread: a check reports the calling thread's calls only)
  if (!word) return QTX_OK;
  HIPCHK(hipMemcpy(&v, word, sizeof v, hipMemcpyDeviceToHost));
  if (!v) return QTX_OK;
  HIPCHK(hipMemset(word, 0, sizeof(unsigned)));   // reported once (the thread's own word)
  return fail(QTX_E_DEVICE, "%s", status_text(v));
}

int32_t qtx_greedy_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, int32_t max_len, int64_t start, int64_t* ids,
                          void* ws, size_t ws_bytes, void* stream) {
  return qtx_greedy_decode_fault(m, src, src_mask, B, S, max_len, start, ids, ws, ws_bytes,
                                 nullptr, stream);
}

}  // extern "C"

namespace {

// whether the decode runs the fused step (else the unfused one)
bool greedy_fused(const qtx_config& c, int S, int max_len) {
  return S <= 128 && max_len <= 128 && fused_step_ok(c) && !knobs().unfused;
}

// The encode step of every decode, on the B sentences: memory = encode(src_embed(src), mask),
// the cross K/V of every layer into x and, for the fused step (cvg non-null), the cross
// values in k_dec_attn's 4-key groups.
// (captured into a hipGraph with the steps' replay — QTX_PRE_GRAPH in round 3 — it
// measured no faster: 14.34 vs 14.31 ms per B = 32 decode; the host's enqueue of these
// launches runs ahead of the GPU)
int encode_src(const qtx_model* m, GreedyWS& g, const int64_t* src, const uint8_t* mask, int B,
               int S, CrossKV& x, int8_t* cvg, const qtx_fault* f, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const long D = c.d_model;
  HIPCHK(launch_embed(src, S, B, S, nullptr, 0, m->src_lut, c.src_vocab, m->pe, c.max_len,
                      g.enc.x, S * D, st));
  RC(encoder_run(m, g.enc.x, mask, B, S, g.memory, g.enc, st, f));
  RC(cross_kv(m, g.memory, B * S, x, st));
  if (cvg) {
    const long v_ls = c.n_layers > 1 ? (long)(x.v8[1] - x.v8[0]) : 0;
    HIPCHK(launch_vgroup4(x.v8[0], v_ls, c.n_layers, B, S, cvg, (long)B * ((S + 3) & ~3) * D, st));
  }
  return QTX_OK;
}

// What precedes the steps: the encode step in place, ids[:, 0] and the step counters.
int greedy_prologue(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S,
                    int max_len, int64_t start, const qtx_fault* f, bool fused, hipStream_t st) {
  RC(encode_src(m, g, src, g.mask, B, S, g.cross, fused ? g.cvg[0] : nullptr, f, st));
  // ids[:, 0] = start ; step[0] = position 0, step[1] = arrival counter
  HIPCHK(launch_fill_col(g.ids, max_len, B, start, st));
  HIPCHK(launch_zero(g.step, 16, st));
  return QTX_OK;
}

// The fused steps of a request through the model's step-graph runner, serialised per model
// with the model's device current (the runner creates streams and events).
int run_steps(const qtx_model* m, const StepRequest& rq, hipStream_t st) {
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lock(mm->mu);
  DeviceGuard dg(mm->device);
  return mm->sg.run(rq, st);
}

int greedy_run(const qtx_model* m, GreedyWS& g, const int64_t* src, int B, int S, int max_len,
               int64_t start, const qtx_fault* f, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  const uint8_t* src_mask = g.mask;
  int64_t* ids = g.ids;
  const bool fused = greedy_fused(c, S, max_len);
  RC(greedy_prologue(m, g, src, B, S, max_len, start, f, fused, st));
  if (!fused) {
    for (int t = 0; t + 1 < max_len; ++t) RC(greedy_step_unfused(m, g, B, S, max_len, ids, src_mask, st));
    return QTX_OK;
  }
  // sub-batches: each has its own step scratch and step counter; the first decoder input
  // is tgt_embed(ys[:, 0]) at position 0, later ones come from the previous step's argmax
  const Groups gr = decode_groups(B);
  std::vector<GreedyWS> gv;
  HIPCHK(hipMemsetAsync(g.gsteps, 0, sizeof(int) * 4 * QTX_MAX_GROUPS, st));
  for (int i = 0; i < gr.G; ++i) {
    gv.push_back(group_view(g, c, i, gr.b0(i), S, max_len));
    HIPCHK(launch_embed(ids + (long)gr.b0(i) * max_len, max_len, gr.rows(i, B), 1, gv[i].step,
                        0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len, gv[i].dec.x, D, st));
  }
  if (max_len <= 1) return QTX_OK;
  // steps per graph: the whole decode in one graph by default (one graph launch); must
  // divide max_len-1 (the step position is read from device memory, so replays chain)
  int per_graph = max_len - 1;
  if (const int v = knobs().graph_steps; v > 0 && (max_len - 1) % v == 0) per_graph = v;
  StepRequest rq;
  rq.key.rows = B; rq.key.S = S; rq.key.max_len = max_len;
  rq.key.groups = gr.G;
  rq.key.anchor = g.gsteps;
  rq.key.form = g.top_ids ? StepForm::Scored : StepForm::Plain;   // the scored step: its own entry
  // a graph of the whole decode is replayed once per decode from position 0: each captured
  // step knows its position (a shorter graph replays at several)
  rq.key.host_pos = per_graph == max_len - 1;
  rq.key.joint = gr.G > 1 && knobs().group_graph;
  rq.step = [&](int i, hipStream_t s, int t) {
    return greedy_step_fused(m, gv[i], gr.rows(i, B), S, max_len, ids + (long)gr.b0(i) * max_len,
                             src_mask + (long)gr.b0(i) * S, s, t);
  };
  rq.plan = {{per_graph, (max_len - 1) / per_graph, 0}};
  rq.timed = knobs().time_graph;
  return run_steps(m, rq, st);
}

}  // namespace

// =======================================================================================
// KV-cached greedy decode with one decoder fault (include/qtx.h: qtx_greedy_decode_dfault)
// =======================================================================================
namespace {

// The workspace: the scored decode's (a prefix, so the captured steps see the same buffers
// in the plain and the scored form), then the faulty pass's scratch, the record, and the
// golden copies a resume returns.
struct DfaultWS {
  GreedyWS g;
  Scratch fs;           // the faulty full-prefix pass, B * (max_len - 1) rows
  CrossKV fx;           // its cross K/V when the fault sits in a memory K/V projection
  float* fout;          // [B * (max_len - 1), D] its output
  float* flogits;       // [B, V] the generator on each sentence's last row
  uint8_t* tmask;       // [T, T] causal mask
  int64_t* rec_ids;     // [B, 2, 2]
  float* rec_logp;
  int* changed;         // [B]
  int64_t* gold_ids;    // [B, max_len]          the golden decode, as far as it is known
  int64_t* gold_top_ids;   // [B, max_len-1, 2]  (qtx_model::DfaultHdr)
  float* gold_top_logp;
  int64_t* stamp;       // [2] the header's nonce (resume compares it with the host table's)
};

DfaultWS carve_dfault(Arena& ar, const qtx_config& c, int B, int S, int max_len) {
  DfaultWS w;
  const size_t D = c.d_model, Tm = max_len > 1 ? max_len - 1 : 1;
  w.g = carve_greedy(ar, c, B, S, max_len, true);
  w.g.no_fold = true;
  w.fs = carve_scratch(ar, c, (long)(B * Tm));
  w.fx = carve_cross(ar, c, (long)B * S);
  w.fout = ar.take<float>(B * Tm * D);
  w.flogits = ar.take<float>((size_t)B * c.tgt_vocab);
  w.tmask = ar.take<uint8_t>(Tm * Tm);
  w.rec_ids = ar.take<int64_t>((size_t)B * 4);
  w.rec_logp = ar.take<float>((size_t)B * 4);
  w.changed = ar.take<int>((size_t)B);
  w.gold_ids = ar.take<int64_t>((size_t)B * max_len);
  w.gold_top_ids = ar.take<int64_t>(B * Tm * 2);
  w.gold_top_logp = ar.take<float>(B * Tm * 2);
  w.stamp = ar.take<int64_t>(2);
  return w;
}

size_t dfault_ws(const qtx_config& c, int B, int S, int max_len) {
  Arena ar;
  carve_dfault(ar, c, B, S, max_len);
  return align_up(ar.used);
}

// KV-cached steps t0 .. t1-1 from ids[:, t0], with the decode's path selection: the unfused
// step; the fused step launched eagerly at host positions (QTX_NO_GRAPH); or the fused step
// captured at the device counter's position — graphs of QTX_GRAPH_STEPS (default 8) steps and
// of one step, so that any range is a few replays and a sweep over fault steps captures
// nothing new.  A range never crosses the fault step: the caller splits there.
int dfault_steps(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t0, int t1,
                 hipStream_t st) {
  if (t0 >= t1) return QTX_OK;
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  const bool fused = greedy_fused(c, S, max_len);
  const Groups gr = decode_groups(B);
  HIPCHK(launch_set_steps(g.step, g.gsteps, fused ? gr.G : 0, t0, st));
  if (!fused) {
    for (int t = t0; t < t1; ++t) RC(greedy_step_unfused(m, g, B, S, max_len, g.ids, g.mask, st));
    return QTX_OK;
  }
  std::vector<GreedyWS> gv;
  for (int i = 0; i < gr.G; ++i) {   // the first decoder input: tgt_embed(ids[:, t0]) at t0
    gv.push_back(group_view(g, c, i, gr.b0(i), S, max_len));
    HIPCHK(launch_embed(g.ids + (long)gr.b0(i) * max_len + t0, max_len, gr.rows(i, B), 1, nullptr,
                        t0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len, gv[i].dec.x, D, st));
  }
  StepRequest rq;
  rq.key.rows = B; rq.key.S = S; rq.key.max_len = max_len;
  rq.key.groups = gr.G;
  rq.key.anchor = g.gsteps;
  rq.key.form = g.top_ids ? StepForm::DfaultScored : StepForm::Dfault;   // this entry's own graphs
  rq.step = [&](int i, hipStream_t s, int t) {
    return greedy_step_fused(m, gv[i], gr.rows(i, B), S, max_len, g.ids + (long)gr.b0(i) * max_len,
                             g.mask + (long)gr.b0(i) * S, s, t);
  };
  const int big = knobs().graph_steps > 0 ? knobs().graph_steps : 8;
  const int nbig = big > 1 ? (t1 - t0) / big : 0, none = (t1 - t0) - nbig * big;
  if (nbig) rq.plan.push_back({big, nbig, t0});
  if (none) rq.plan.push_back({1, none, t0 + nbig * big});
  return run_steps(m, rq, st);
}

// The faulty full-prefix decoder pass of step `step` over the whole batch (the fault's row
// indexes its [B * T] tokens, T = step + 1) and the generator on each sentence's last row:
// flogits [B, V].  The body of qtx_decoder_forward_fault on this call's workspace; the
// cached cross K/V are read, never written (a memory K/V fault gets its own copy).
int dfault_pass(const qtx_model* m, DfaultWS& w, int B, int S, int max_len, const qtx_fault* f,
                int step, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model, T = step + 1;
  GreedyWS& g = w.g;
  // the scratch was carved for the longest prefix: the three projections and their scales lie
  // M = B * T rows apart, as the row GEMM writes them (carve_scratch)
  Scratch s = w.fs;
  const long M = (long)B * T;
  s.k8 = s.q8 + M * D; s.v8 = s.k8 + M * D;
  s.sk = s.sq + M; s.sv = s.sk + M;
  HIPCHK(launch_embed(g.ids, max_len, B, T, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                      s.x, (long)T * D, st));
  HIPCHK(launch_causal_mask(w.tmask, T, st));
  bool ckv_fault = false;
  for (int l = 0; l < c.n_layers; ++l)
    ckv_fault |= fault_for(f, 1, l, G_CKV, B * S, c).kind != FK_NONE;
  if (ckv_fault) RC(cross_kv(m, g.memory, B * S, w.fx, st, f));
  RC(decoder_body(m, s, ckv_fault ? w.fx : g.cross, g.mask, w.tmask, 0, B, T, S, w.fout, f, st));
  HIPCHK(launch_generator_mfma(w.fout + (long)(T - 1) * D, (long)T * D, B, nullptr, nullptr,
                               m->gen_wt, m->gen_b, c.tgt_vocab, w.flogits, st));
  return QTX_OK;
}

// the faulty top 2 into rec[:, 1, :]
int dfault_top2(const qtx_model* m, DfaultWS& w, int B, hipStream_t st) {
  HIPCHK(launch_logsoftmax_top2(w.flogits, B, m->cfg.tgt_vocab, nullptr, 0, nullptr, 0,
                                w.rec_ids + 2, w.rec_logp + 2, 2, st));
  return QTX_OK;
}

void dfault_store(const qtx_model* m, const void* ws, const qtx_model::DfaultHdr& h) {
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lk(mm->mu);
  mm->dfault[ws] = h;
}

int dfault_args(const qtx_model* m, int B, int S, int max_len, const qtx_fault* f, int fault_step) {
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if ((long)B * c.tgt_vocab >= (1L << 30) || (long)B * max_len * c.d_model >= (1L << 30))
    return fail(QTX_E_INVALID, "B * tgt_vocab and B * max_len * d_model must be below 2^30");
  if (!f || f->kind == QTX_FAULT_NONE || f->module != 1)
    return fail(QTX_E_INVALID, "the decoder-fault decode takes one decoder fault (encoder "
                               "faults: qtx_greedy_decode_fault / _scored)");
  if (fault_step < 0) return fail(QTX_E_INVALID, "fault_step %d", fault_step);
  if (c.weight_bits != 8) return fail(QTX_E_UNSUPPORTED, "fault injection needs 8-bit weights");
  if (knobs().dbg_tail) return fail(QTX_E_UNSUPPORTED, "decoder-fault decode: not with QTX_DBG_TAIL");
  return QTX_OK;
}

}  // namespace

extern "C" {

size_t qtx_greedy_dfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                        int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return dfault_ws(m->cfg, B, S, max_len);
}

int32_t qtx_greedy_decode_dfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                 int32_t B, int32_t S, int32_t max_len, int64_t start,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* f, int32_t fault_step, void* stream) {
  if (!m || !src || !src_mask || !ids || !ws) return fail(QTX_E_INVALID, "null argument");
  const bool scored = top_ids || top_logp;
  if ((scored && (!top_ids || !top_logp)) || !rec_ids != !rec_logp)
    return fail(QTX_E_INVALID, "top_ids / top_logp and rec_ids / rec_logp come in pairs");
  RC(dfault_args(m, B, S, max_len, f, fault_step));
  const qtx_config& c = m->cfg;
  if ((scored || rec_ids) && c.tgt_vocab < 2)
    return fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (ws_bytes < dfault_ws(c, B, S, max_len)) return fail(QTX_E_WORKSPACE, "workspace too small");
  const int last = max_len - 1;             // steps 0 .. last-1
  const bool applied = fault_step < last;   // else the fault's step is never run: golden
  if (applied) RC(check_fault(m, f, 1, B, fault_step + 1, S));
  hipStream_t st = (hipStream_t)stream;
  dfault_forget(m, ws);                     // no header while the workspace is rewritten
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  DfaultWS w = carve_dfault(ar, c, B, S, max_len);
  GreedyWS& g = w.g;
  g.enc.status = cst;
  if (!scored) g.top_ids = nullptr, g.top_logp = nullptr;   // the plain step and its tail
  const size_t nid = (size_t)B * max_len * sizeof(int64_t), nt = (size_t)B * last * 2;
  auto keep_gold = [&]() -> int {   // what is golden so far, for later resumes
    HIPCHK(hipMemcpyAsync(w.gold_ids, g.ids, nid, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(w.gold_top_ids, g.top_ids, nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(w.gold_top_logp, g.top_logp, nt * sizeof(float), hipMemcpyDeviceToDevice, st));
    return QTX_OK;
  };
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_prologue(m, g, src, B, S, max_len, start, nullptr, greedy_fused(c, S, max_len), st));
  RC(dfault_steps(m, g, B, S, max_len, 0, applied ? fault_step + 1 : last, st));
  if (applied) {
    const int V = c.tgt_vocab;
    if (scored) {          // the cached step's top 2 is the golden record (the campaign's out_2)
      RC(keep_gold());
      HIPCHK(launch_dfault_gold(g.top_ids, g.top_logp, last, fault_step, B, w.rec_ids, w.rec_logp, st));
    } else if (rec_ids) {  // plain form: from the cached step's logits
      HIPCHK(launch_logsoftmax_top2(g.logits, B, V, nullptr, 0, nullptr, 0, w.rec_ids, w.rec_logp, 2, st));
    }
    RC(dfault_pass(m, w, B, S, max_len, f, fault_step, st));
    if (scored || rec_ids) RC(dfault_top2(m, w, B, st));
    if (scored)
      HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, g.ids, g.top_ids,
                                g.top_logp, nullptr, st));
    else                   // the plain tail's rule (qtx_generator without log-probabilities)
      HIPCHK(launch_logsoftmax_argmax(w.flogits, B, V, nullptr, g.ids, max_len, nullptr,
                                      fault_step + 1, st));
    RC(dfault_steps(m, g, B, S, max_len, fault_step + 1, last, st));
  } else if (scored && last > 0) {
    RC(keep_gold());
  }
  HIPCHK(hipMemcpyAsync(ids, g.ids, nid, hipMemcpyDeviceToDevice, st));
  if (scored && last > 0) {
    HIPCHK(hipMemcpyAsync(top_ids, g.top_ids, nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, g.top_logp, nt * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (applied && rec_ids) {
    HIPCHK(hipMemcpyAsync(rec_ids, w.rec_ids, (size_t)B * 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(rec_logp, w.rec_logp, (size_t)B * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (scored && last > 0) {
    static std::atomic<long long> next_nonce{1};
    const long long nonce = (long long)(m->serial << 40) ^ next_nonce.fetch_add(1);
    HIPCHK(launch_fill_col(w.stamp, 1, 1, nonce, st));
    dfault_store(m, ws, qtx_model::DfaultHdr{B, S, max_len, applied ? fault_step : last - 1,
                                             !applied, ws_bytes, nonce});
  }
  return QTX_OK;
}

int32_t qtx_greedy_dfault_resume(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                                 int64_t* ids, int64_t* top_ids, float* top_logp,
                                 int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                 const qtx_fault* f, int32_t fault_step, int32_t* changed_host,
                                 void* stream) {
  if (!m || !ids || !top_ids || !top_logp || !ws || !rec_ids != !rec_logp)
    return fail(QTX_E_INVALID, "null argument");
  RC(dfault_args(m, B, S, max_len, f, fault_step));
  const qtx_config& c = m->cfg;
  if (c.tgt_vocab < 2) return fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (ws_bytes < dfault_ws(c, B, S, max_len)) return fail(QTX_E_WORKSPACE, "workspace too small");
  qtx_model::DfaultHdr h{};
  {
    qtx_model* mm = const_cast<qtx_model*>(m);
    std::lock_guard<std::mutex> lk(mm->mu);
    auto it = mm->dfault.find(ws);
    if (it == mm->dfault.end())
      return fail(QTX_E_INVALID, "resume: the workspace holds no scored decoder-fault decode of this model");
    h = it->second;
  }
  if (h.B != B || h.S != S || h.L != max_len)
    return fail(QTX_E_INVALID, "resume: the workspace was filled for B=%d S=%d max_len=%d", h.B, h.S, h.L);
  if (fault_step > h.n)
    return fail(QTX_E_INVALID, "resume: fault_step %d above the golden prefix's last step %d",
                fault_step, h.n);
  RC(check_fault(m, f, 1, B, fault_step + 1, S));
  hipStream_t st = (hipStream_t)stream;
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  DfaultWS w = carve_dfault(ar, c, B, S, max_len);
  GreedyWS& g = w.g;
  long long stamp = 0;   // the memory must still be what the header describes
  HIPCHK(hipMemcpyAsync(&stamp, w.stamp, sizeof stamp, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (stamp != h.nonce) {
    dfault_forget(m, ws);
    return fail(QTX_E_INVALID, "resume: the workspace was overwritten since its decode");
  }
  const int last = max_len - 1;
  const size_t nid = (size_t)B * max_len * sizeof(int64_t), nt = (size_t)B * last * 2;
  HIPCHK(launch_dfault_gold(w.gold_top_ids, w.gold_top_logp, last, fault_step, B, w.rec_ids,
                            w.rec_logp, st));
  RC(dfault_pass(m, w, B, S, max_len, f, fault_step, st));
  RC(dfault_top2(m, w, B, st));
  HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, nullptr, nullptr,
                            nullptr, w.changed, st));
  // the one synchronising copy: whether any sentence's token changed decides what runs next
  std::vector<int32_t> changed((size_t)B);
  HIPCHK(hipMemcpyAsync(changed.data(), w.changed, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  bool any = false;
  for (int b = 0; b < B; ++b) any |= changed[b] != 0;
  if (changed_host) std::copy(changed.begin(), changed.end(), changed_host);
  if (!any && h.gold_full) {   // a masked fault: the golden decode with the faulty entry
    HIPCHK(hipMemcpyAsync(ids, w.gold_ids, nid, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_ids, w.gold_top_ids, nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, w.gold_top_logp, nt * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, nullptr, top_ids,
                              top_logp, nullptr, st));
  } else {                     // the steps above fault_step again, from the faulty tokens
    dfault_forget(m, ws);
    HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, fault_step, max_len, g.ids, g.top_ids,
                              g.top_logp, nullptr, st));
    RC(dfault_steps(m, g, B, S, max_len, fault_step + 1, last, st));
    HIPCHK(hipMemcpyAsync(ids, g.ids, nid, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_ids, g.top_ids, nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, g.top_logp, nt * sizeof(float), hipMemcpyDeviceToDevice, st));
    h.n = fault_step;
    dfault_store(m, ws, h);
  }
  if (rec_ids) {
    HIPCHK(hipMemcpyAsync(rec_ids, w.rec_ids, (size_t)B * 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(rec_logp, w.rec_logp, (size_t)B * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return QTX_OK;
}

}  // extern "C"

// =======================================================================================
// Faults of the KV-cached decode itself: one step fault or one cache upset
// (include/qtx.h: qtx_greedy_decode_kvfault)
// =======================================================================================
namespace {

// The workspace: the scored decode's (a prefix, as DfaultWS) and the record.
struct KvfaultWS {
  GreedyWS g;
  int64_t* rec_ids;     // [B, 2, 2]
  float* rec_logp;
};

KvfaultWS carve_kvfault(Arena& ar, const qtx_config& c, int B, int S, int max_len) {
  KvfaultWS w;
  w.g = carve_greedy(ar, c, B, S, max_len, true);
  w.g.no_fold = true;
  w.rec_ids = ar.take<int64_t>((size_t)B * 4);
  w.rec_logp = ar.take<float>((size_t)B * 4);
  return w;
}

size_t kvfault_ws(const qtx_config& c, int B, int S, int max_len) {
  Arena ar;
  carve_kvfault(ar, c, B, S, max_len);
  return align_up(ar.used);
}

bool kv_attn_target(int lin) {
  return lin == QTX_LIN_QK || lin == QTX_LIN_PV || lin == QTX_LIN_CQK || lin == QTX_LIN_CPV;
}

// A step fault's coordinates against the step's own MatMuls: one query row per sentence,
// Sk = step + 1 self keys or S cross keys (include/qtx.h).  Linear targets: check_fault with
// one token row per sentence.
int kvfault_check_fault(const qtx_model* m, const qtx_fault* f, int B, int S, int step) {
  const qtx_config& c = m->cfg;
  if (!kv_attn_target(f->linear)) {
    if ((f->linear == QTX_LIN_CK || f->linear == QTX_LIN_CV) && step != 0)
      return fail(QTX_E_INVALID, "a memory K/V projection fault belongs to step 0 (step %d)", step);
    return check_fault(m, f, 1, B, 1, S);
  }
  if (f->kind < QTX_FAULT_INPUT || f->kind > QTX_FAULT_OUTPUT)
    return fail(QTX_E_INVALID, "fault kind %d", f->kind);
  if (f->layer < 0 || f->layer >= c.n_layers) return fail(QTX_E_INVALID, "fault layer %d", f->layer);
  const bool cross = f->linear == QTX_LIN_CQK || f->linear == QTX_LIN_CPV;
  const bool qk = f->linear == QTX_LIN_QK || f->linear == QTX_LIN_CQK;
  const bool in_kind = f->kind == QTX_FAULT_INPUT || f->kind == QTX_FAULT_INPUT16;
  const long sk = cross ? S : step + 1, H = c.n_heads;
  if (f->kind != QTX_FAULT_OUTPUT && (f->bit < 0 || f->bit > 7))
    return fail(QTX_E_INVALID, "fault bit %d", f->bit);
  long nr, nc, wmax;
  if (f->kind == QTX_FAULT_OUTPUT) { nr = B; nc = qk ? H * sk : H * 64; wmax = 0; }
  else if (in_kind) { nr = B; nc = qk ? H * 64 : H * sk; wmax = qk ? sk : 64; }
  else { nr = B * sk; nc = H * 64; wmax = 1L << 30; }   // a window past query row 0: no effect
  if (f->row < 0 || f->row >= nr || f->col < 0 || f->col >= nc)
    return fail(QTX_E_INVALID, "fault index (%ld, %ld) outside [%ld, %ld]", (long)f->row,
                (long)f->col, nr, nc);
  if ((f->kind == QTX_FAULT_INPUT16 || f->kind == QTX_FAULT_WEIGHT16) &&
      (f->win_len < 1 || f->win_len > 16 || f->win_start < 0 || f->win_start + f->win_len > wmax))
    return fail(QTX_E_INVALID, "fault window [%ld, +%d) outside %ld", (long)f->win_start,
                f->win_len, wmax);
  return QTX_OK;
}

// Where an upset lands: the code byte(s) or the scale word, as offsets checked against the
// caches' extents here, on the host.
struct UpsetAt { int8_t* c0; int8_t* c1; float* s; };
int kvfault_upset_at(const qtx_config& c, GreedyWS& g, const qtx_cache_upset* u, int B, int S,
                     int max_len, int step, bool fused, UpsetAt* at) {
  const long D = c.d_model;
  if (u->cache < 0 || u->cache > 3) return fail(QTX_E_INVALID, "upset cache %d", u->cache);
  if (u->layer < 0 || u->layer >= c.n_layers) return fail(QTX_E_INVALID, "upset layer %d", u->layer);
  if (u->field != 0 && u->field != 1) return fail(QTX_E_INVALID, "upset field %d", u->field);
  const bool self = u->cache < 2, is_v = u->cache & 1;
  const long per = self ? max_len : S;            // rows per sentence
  if (u->row < 0 || u->row >= (long)B * per)
    return fail(QTX_E_INVALID, "upset row %ld outside [0, %ld)", (long)u->row, (long)B * per);
  const long b = u->row / per, j = u->row % per;
  if (self && j >= step)
    return fail(QTX_E_INVALID, "upset of self-cache position %ld at step %d: not written yet", j, step);
  if (u->field == 0 ? (u->bit < 0 || u->bit > 7) : !((u->bit >= 0 && u->bit <= 22) || u->bit == 31))
    return fail(QTX_E_INVALID, "upset bit %d (codes: 0..7; scales: 0..22 and 31)", u->bit);
  if (u->col < 0 || u->col >= (u->field == 0 ? D : 1))
    return fail(QTX_E_INVALID, "upset col %d", u->col);
  if (!at) return QTX_OK;
  const int l = u->layer;
  *at = UpsetAt{nullptr, nullptr, nullptr};
  if (u->field == 1) {
    float* sc = self ? (is_v ? g.svc[l] : g.skc[l]) : (is_v ? g.cross.sv[l] : g.cross.sk[l]);
    at->s = sc + u->row;
    return QTX_OK;
  }
  const long rm = u->row * D + u->col;                                   // row-major
  const long G4 = (per + 3) / 4;
  const long grp = ((b * G4 + j / 4) * D + u->col) * 4 + j % 4;          // 4-key groups
  if (rm >= (long)B * per * D || grp >= (long)B * G4 * 4 * D) return fail(QTX_E_INVALID, "upset offset");
  if (!is_v) at->c0 = (self ? g.kc[l] : g.cross.k8[l]) + rm;
  else if (self) at->c0 = g.vc[l] + (fused ? grp : rm);                  // one layout per path
  else {
    at->c0 = g.cross.v8[l] + rm;                                         // every copy a step reads
    if (fused) at->c1 = g.cvg[l] + grp;
  }
  return QTX_OK;
}

// Step `t` of the KV-cached decode with fault f, eager, on the whole batch: the decoder input
// is tgt_embed(ids[:, t]); every layer's cache row t is (re)written from this run; the step's
// logits land in g.logits.  Built from pieces that agree bit for bit with the fused step's
// kernels: the FaultArgs-aware linear() at M = B, the row quantizers, and — on the fused
// workspace, whose values lie in 4-key groups — k_dec_attn itself for the attention.
int kvfault_step(const qtx_model* m, GreedyWS& g, int B, int S, int max_len, int t,
                 const qtx_fault* f, bool fused, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const int D = c.d_model;
  Scratch& s = g.dec;
  HIPCHK(launch_set_steps(g.step, g.gsteps, 0, t, st));
  HIPCHK(launch_embed(g.ids + t, max_len, B, 1, nullptr, t, m->tgt_lut, c.tgt_vocab, m->pe,
                      c.max_len, s.x, D, st));
  // the one query row of sentence af.b with the caches as the fused step keeps them
  auto fused_attn_fault = [&](const AttnFault& af, int l, bool cross) -> int {
    RC(quant(s.y, cross ? D : 3 * D, B, D, s.q8, s.sq, st));   // the query codes k_dec_attn formed
    const long rows = cross ? S : max_len;
    AttnArgs a{};
    a.q = s.q8; a.q_bs = D; a.q_ld = D; a.sq = s.sq; a.sq_bs = 1;
    a.k = cross ? g.cross.k8[l] : g.kc[l]; a.k_bs = rows * D; a.k_ld = D;
    a.sk = cross ? g.cross.sk[l] : g.skc[l]; a.sk_bs = rows;
    a.v = cross ? g.cvg[l] : g.vc[l];
    a.sv = cross ? g.cross.sv[l] : g.svc[l]; a.sv_bs = rows;
    if (cross) { a.mask = g.mask; a.m_bs = S; a.m_is = 0; }
    a.ctx = s.ctx; a.c_bs = D; a.c_ld = D;
    a.B = B; a.H = c.n_heads; a.Sq = 1; a.Sk = cross ? S : t + 1; a.dec = 1;
    HIPCHK(launch_dec_attn_fault(a, af, (int)((rows + 3) / 4), st));
    return QTX_OK;
  };
  for (int l = 0; l < c.n_layers; ++l) {
    const DecLayer& L = m->dec[l];
    auto fa = [&](GemmId gid) { return fault_for(f, 1, l, gid, B, c); };
    // an attention WEIGHT16 window that misses the step's only query row has no effect
    AttnFault af_self{}, af_cross{};
    auto hits = [](AttnFault& af) {
      if (af.row0 > 0 || af.row0 + af.nrows <= 0) return false;
      af.row0 = 0; af.nrows = 1;
      return true;
    };
    const bool self_f = attn_fault_for(f, 1, l, false, 1, t + 1, af_self) && hits(af_self);
    const bool cross_f = attn_fault_for(f, 1, l, true, 1, S, af_cross) && hits(af_cross);
    RC(ln_quant(s.x, B, L.ln[0], D, s.a8, s.sa, st));
    RC(linear(c, L.qkv, s.a8, s.sa, B, 0, nullptr, s.y, 3 * D, st, fa(G_QKV)));
    if (fused) {
      DecAttnArgs at{};
      at.y = s.y; at.ldy = 3 * D; at.kv_new = 1; at.step = g.step;
      at.kc = g.kc[l]; at.vc = g.vc[l]; at.skc = g.skc[l]; at.svc = g.svc[l]; at.kv_bs = max_len;
      at.ctx = s.ctx; at.B = B; at.host_step1 = t + 1;
      HIPCHK(launch_dec_attn(at, B, st));
      if (self_f) RC(fused_attn_fault(af_self, l, false));
    } else {
      RC(quant(s.y, 3 * D, B, D, s.q8, s.sq, st));
      RowArgs kr = rows_quant(s.y + D, 3 * D, B, D, g.kc[l], g.skc[l]);
      kr.rpb = 1; kr.dst_bstride = max_len; kr.dst_off = t;
      HIPCHK(launch_rows(kr, st));
      RowArgs vr = rows_quant(s.y + 2 * D, 3 * D, B, D, g.vc[l], g.svc[l]);
      vr.rpb = 1; vr.dst_bstride = max_len; vr.dst_off = t;
      HIPCHK(launch_rows(vr, st));
      AttnArgs a = attn_args(s, B, 1, t + 1, max_len);
      a.k = g.kc[l]; a.sk = g.skc[l]; a.v = g.vc[l]; a.sv = g.svc[l];
      a.dec = 1;
      HIPCHK(launch_attention(a, st));
      if (self_f) HIPCHK(launch_attn_fault_rows(a, af_self, st));
    }
    RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
    RC(linear(c, L.o, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st, fa(G_O)));
    if (fused) {
      RC(ln_quant(s.x, B, L.ln[1], D, s.a8, s.sa, st));
      RC(linear(c, L.cq, s.a8, s.sa, B, 0, nullptr, s.y, D, st, fa(G_CQ)));
      DecAttnArgs at{};
      at.y = s.y; at.ldy = D; at.kv_new = 0; at.S = S; at.mask = g.mask;
      at.kc = g.cross.k8[l]; at.vc = g.cvg[l]; at.skc = g.cross.sk[l]; at.svc = g.cross.sv[l];
      at.kv_bs = S; at.ctx = s.ctx; at.B = B;
      HIPCHK(launch_dec_attn(at, B, st));
      if (cross_f) RC(fused_attn_fault(af_cross, l, true));
      RC(quant(s.ctx, D, B, D, s.a8, s.sa, st));
      RC(linear(c, L.co, s.a8, s.sa, B, EPI_RESIDUAL, s.x, s.x, D, st, fa(G_CO)));
    } else {
      RC(cross_attn_block(m, L, l, s, g.cross, B, 1, S, g.mask, st, fa(G_CQ), fa(G_CO),
                          cross_f ? &af_cross : nullptr));
    }
    RC(ffn_block(c, L.w1, L.w2, L.ln[2], s, B, st, fa(G_FFN1), fa(G_FFN2)));
  }
  RC(ln_out(s.x, B, m->dec_norm, D, g.xo, st));
  HIPCHK(launch_generator_mfma(g.xo, D, B, nullptr, nullptr, m->gen_wt, m->gen_b, c.tgt_vocab,
                               g.logits, st));
  return QTX_OK;
}

}  // namespace

extern "C" {

size_t qtx_greedy_kvfault_workspace_size(const qtx_model* m, int32_t B, int32_t S,
                                         int32_t max_len) {
  if (!m || B <= 0 || S <= 0 || max_len < 1) return 0;
  return kvfault_ws(m->cfg, B, S, max_len);
}

int32_t qtx_greedy_decode_kvfault(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                                  int32_t B, int32_t S, int32_t max_len, int64_t start,
                                  int64_t* ids, int64_t* top_ids, float* top_logp,
                                  int64_t* rec_ids, float* rec_logp, void* ws, size_t ws_bytes,
                                  const qtx_fault* f, const qtx_cache_upset* u, int32_t step,
                                  void* stream) {
  if (!m || !src || !src_mask || !ids || !ws) return fail(QTX_E_INVALID, "null argument");
  const bool scored = top_ids || top_logp;
  if ((scored && (!top_ids || !top_logp)) || !rec_ids != !rec_logp)
    return fail(QTX_E_INVALID, "top_ids / top_logp and rec_ids / rec_logp come in pairs");
  if (!f == !u) return fail(QTX_E_INVALID, "exactly one of fault / upset");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if ((long)B * c.tgt_vocab >= (1L << 30) || (long)B * max_len * c.d_model >= (1L << 30))
    return fail(QTX_E_INVALID, "B * tgt_vocab and B * max_len * d_model must be below 2^30");
  if (f && (f->kind == QTX_FAULT_NONE || f->module != 1))
    return fail(QTX_E_INVALID, "a step fault is one decoder fault (module 1)");
  if (step < 0) return fail(QTX_E_INVALID, "step %d", step);
  if (f && c.weight_bits != 8) return fail(QTX_E_UNSUPPORTED, "fault injection needs 8-bit weights");
  if (knobs().dbg_tail) return fail(QTX_E_UNSUPPORTED, "kvfault decode: not with QTX_DBG_TAIL");
  if ((scored || rec_ids) && c.tgt_vocab < 2)
    return fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (ws_bytes < kvfault_ws(c, B, S, max_len)) return fail(QTX_E_WORKSPACE, "workspace too small");
  const int last = max_len - 1;          // steps 0 .. last-1
  const bool applied = step < last;      // else nothing runs at or after `step`: golden
  const bool fused = greedy_fused(c, S, max_len);
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  KvfaultWS w = carve_kvfault(ar, c, B, S, max_len);
  GreedyWS& g = w.g;
  UpsetAt at{};
  if (applied && f) RC(kvfault_check_fault(m, f, B, S, step));
  if (applied && u) RC(kvfault_upset_at(c, g, u, B, S, max_len, step, fused, &at));
  hipStream_t st = (hipStream_t)stream;
  dfault_forget(m, ws);
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  g.enc.status = cst;
  if (!scored) g.top_ids = nullptr, g.top_logp = nullptr;   // the plain step and its tail
  const int V = c.tgt_vocab;
  const bool rec = applied && rec_ids;
  // the top 2 of the step that just ran, into rec[:, which, :]
  auto record = [&](int which) -> int {
    if (scored)
      HIPCHK(launch_dfault_gold(g.top_ids, g.top_logp, last, step, B, w.rec_ids + 2 * which,
                                w.rec_logp + 2 * which, st));
    else
      HIPCHK(launch_logsoftmax_top2(g.logits, B, V, nullptr, 0, nullptr, 0, w.rec_ids + 2 * which,
                                    w.rec_logp + 2 * which, 2, st));
    return QTX_OK;
  };
  // cached steps t0 .. last-1; with a record, step t0's top 2 is the faulty pair
  auto run_from = [&](int t0) -> int {
    if (rec) {
      RC(dfault_steps(m, g, B, S, max_len, t0, t0 + 1, st));
      RC(record(1));
      ++t0;
    }
    return dfault_steps(m, g, B, S, max_len, t0, last, st);
  };
  HIPCHK(hipMemcpyAsync(g.mask, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(greedy_prologue(m, g, src, B, S, max_len, start, nullptr, fused, st));
  if (!applied) {
    RC(dfault_steps(m, g, B, S, max_len, 0, last, st));
  } else {
    // golden up to the step; with a record, the step itself once on the golden caches
    RC(dfault_steps(m, g, B, S, max_len, 0, rec ? step + 1 : step, st));
    if (rec) RC(record(0));
    if (u) {
      HIPCHK(launch_cache_upset(at.c0, at.c1, at.s, u->bit, st));
      RC(run_from(step));
    } else if (f->linear == QTX_LIN_CK || f->linear == QTX_LIN_CV) {
      // the one-time memory K/V projection again, with the fault: it serves every step
      RC(cross_kv(m, g.memory, B * S, g.cross, st, f));
      if (fused) {
        const long v_ls = c.n_layers > 1 ? (long)(g.cross.v8[1] - g.cross.v8[0]) : 0;
        HIPCHK(launch_vgroup4(g.cross.v8[0], v_ls, c.n_layers, B, S, g.cvg[0],
                              (long)B * ((S + 3) & ~3) * c.d_model, st));
      }
      RC(run_from(0));
    } else {
      RC(kvfault_step(m, g, B, S, max_len, step, f, fused, st));
      if (scored || rec)
        HIPCHK(launch_logsoftmax_top2(g.logits, B, V, nullptr, 0, nullptr, 0, w.rec_ids + 2,
                                      w.rec_logp + 2, 2, st));
      if (scored)
        HIPCHK(launch_dfault_tail(w.rec_ids, w.rec_logp, B, step, max_len, g.ids, g.top_ids,
                                  g.top_logp, nullptr, st));
      else                   // the plain tail's rule (qtx_generator without log-probabilities)
        HIPCHK(launch_logsoftmax_argmax(g.logits, B, V, nullptr, g.ids, max_len, nullptr, step + 1,
                                        st));
      RC(dfault_steps(m, g, B, S, max_len, step + 1, last, st));
    }
  }
  HIPCHK(hipMemcpyAsync(ids, g.ids, (size_t)B * max_len * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  if (scored && last > 0) {
    const size_t nt = (size_t)B * last * 2;
    HIPCHK(hipMemcpyAsync(top_ids, g.top_ids, nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, g.top_logp, nt * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (rec) {
    HIPCHK(hipMemcpyAsync(rec_ids, w.rec_ids, (size_t)B * 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(rec_logp, w.rec_logp, (size_t)B * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return QTX_OK;
}

}  // extern "C"

// =======================================================================================
// Beam-search decode with EOS stop (include/qtx.h: qtx_beam_decode)
// =======================================================================================
namespace {

// (BeamWS / carve_beam / beam_ws, the workspace: qtx_carve.h)

// What precedes the steps: the encoder and the cross K/V GEMM once on the B sentences, their
// results replicated to the B * K hypotheses, the search state and the first decoder input.
int beam_prologue(const qtx_model* m, BeamWS& w, const int64_t* src, int B, int K, int S,
                  int64_t start, bool fused, hipStream_t st) {
  const qtx_config& c = m->cfg;
  const long D = c.d_model, S4 = (S + 3) & ~3;
  GreedyWS& g = w.g;
  RC(encode_src(m, g, src, w.mask_b, B, S, w.cross_b, fused ? w.cvg_b : nullptr, nullptr, st));
  for (int l = 0; l < c.n_layers; ++l) {
    HIPCHK(launch_beam_rep(w.cross_b.k8[l], g.cross.k8[l], B, K, S * D, st));
    if (fused)
      HIPCHK(launch_beam_rep(w.cvg_b + (size_t)l * B * S4 * D, g.cvg[l], B, K, S4 * D, st));
    else
      HIPCHK(launch_beam_rep(w.cross_b.v8[l], g.cross.v8[l], B, K, S * D, st));
    HIPCHK(launch_beam_rep(w.cross_b.sk[l], g.cross.sk[l], B, K, S * 4L, st));
    HIPCHK(launch_beam_rep(w.cross_b.sv[l], g.cross.sv[l], B, K, S * 4L, st));
  }
  HIPCHK(launch_beam_rep(w.mask_b, g.mask, B, K, S, st));
  const BeamState& bs = w.tail.st;
  HIPCHK(launch_beam_init(B, K, bs.score, bs.fin, bs.len, bs.parent, g.step, st));
  HIPCHK(launch_fill_col(bs.ids0, 1, B * K, start, st));
  HIPCHK(launch_embed(bs.ids0, 1, B * K, 1, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                      g.dec.x, D, st));
  return QTX_OK;
}

// n more beam steps at the device counter's position, with dfault_steps' path selection: the
// unfused step or eager fused steps (QTX_NO_GRAPH), else captured graphs — one of `big` steps
// when n == big, else n replays of the one-step graph.  One group: no sub-batches.
int beam_steps(const qtx_model* m, BeamWS& w, int R, int S, int max_len, int n, int big,
               bool fused, hipStream_t st) {
  GreedyWS& g = w.g;
  if (!fused) {
    for (int t = 0; t < n; ++t) RC(greedy_step_unfused(m, g, R, S, max_len, nullptr, g.mask, st));
    return QTX_OK;
  }
  // the beam step's own graphs: the select's eos / pad are baked into the captured launch
  const BeamTail& bt = w.tail;
  StepRequest rq;
  rq.key.rows = R; rq.key.S = S; rq.key.max_len = max_len;
  rq.key.anchor = g.step;
  rq.key.form = StepForm::Beam;
  rq.key.beam_k = bt.K; rq.key.eos = bt.eos; rq.key.pad = bt.pad;
  rq.step = [&](int, hipStream_t s, int t) {
    return greedy_step_fused(m, g, R, S, max_len, nullptr, g.mask, s, t);
  };
  const int per = n == big ? big : 1;
  rq.plan = {{per, n / per, -1}};
  return run_steps(m, rq, st);
}

}  // namespace

extern "C" {

size_t qtx_beam_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t max_len,
                               int32_t beam) {
  if (!m || B <= 0 || S <= 0 || max_len < 1 || beam < 1 || beam > BEAM_MAXK) return 0;
  return beam_ws(m->cfg, B, beam, S, max_len);
}

int32_t qtx_beam_decode(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                        int32_t B, int32_t S, int32_t max_len, int32_t beam, int64_t start,
                        int64_t eos, int64_t pad, int32_t early_exit, int64_t* hyp_ids,
                        float* hyp_score, int32_t* hyp_len, int32_t* steps_run, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!m || !src || !src_mask || !hyp_ids || !hyp_score || !hyp_len || !ws)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  RC(check_decode_shape(c, B, S, max_len));
  if (const int lim = beam_limits(B, beam, c.tgt_vocab, start, eos, pad); lim != QTX_OK)
    return fail(lim, "beam decode: 1 <= beam <= 8, beam <= tgt_vocab, start / eos / pad inside "
                     "the vocabulary, eos != pad, B * beam * tgt_vocab < 2^30 (beam=%d eos=%lld "
                     "pad=%lld)", beam, (long long)eos, (long long)pad);
  if ((long)B * beam * max_len * c.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "beam decode: B * beam * max_len * d_model must be below 2^30");
  if (knobs().dbg_tail) return fail(QTX_E_UNSUPPORTED, "beam decode: not with QTX_DBG_TAIL");
  if (ws_bytes < beam_ws(c, B, beam, S, max_len)) return fail(QTX_E_WORKSPACE, "workspace too small");
  dfault_forget(m, ws);
  hipStream_t st = (hipStream_t)stream;
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  BeamWS w = carve_beam(ar, c, B, beam, S, max_len);
  w.tail.eos = (int)eos; w.tail.pad = (int)pad;
  const int R = B * beam;
  // every config decodes: the fused step where the greedy decode of R rows would take it
  const bool fused = greedy_fused(c, S, max_len);
  w.tail.grouped = fused;
  w.g.beam = &w.tail;
  w.g.enc.status = cst;
  HIPCHK(hipMemcpyAsync(w.mask_b, src_mask, (size_t)B * S, hipMemcpyDeviceToDevice, st));
  RC(beam_prologue(m, w, src, B, beam, S, start, fused, st));
  // the steps in chunks of QTX_GRAPH_STEPS (default 8); with early_exit the rows still live
  // are read back after each chunk (one 4-byte synchronising copy) and the decode stops at 0
  const int total = max_len - 1, big = knobs().graph_steps > 0 ? knobs().graph_steps : 8;
  int run = 0;
  while (run < total) {
    const int n = std::min(big, total - run);
    RC(beam_steps(m, w, R, S, max_len, n, big, fused, st));
    run += n;
    if (early_exit && run < total) {
      int live = 1;
      HIPCHK(hipMemcpyAsync(&live, w.g.step + 3, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (live == 0) break;
    }
  }
  const BeamState& bs = w.tail.st;
  HIPCHK(launch_beam_backtrack(bs.bp_par, bs.bp_tok, B, beam, max_len, run, start, pad, hyp_ids, st));
  HIPCHK(hipMemcpyAsync(hyp_score, bs.score, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(hyp_len, bs.len, (size_t)R * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (steps_run) *steps_run = run;
  return QTX_OK;
}

int32_t qtx_beam_select(const qtx_model* m, const float* logits, int32_t B, int32_t beam,
                        int64_t eos, int64_t pad, int32_t max_len, int32_t* step_dev,
                        float* score, int32_t* fin, int32_t* len, int32_t* parent,
                        int32_t* bp_par, int32_t* bp_tok, float* x_next, void* stream) {
  if (!m || !logits || !step_dev || !score || !fin || !len || !parent || !bp_par || !bp_tok ||
      !x_next)
    return fail(QTX_E_INVALID, "null argument");
  if (max_len < 1 || max_len > 512) return fail(QTX_E_INVALID, "max_len %d", max_len);
  if (const int lim = beam_limits(B, beam, m->cfg.tgt_vocab, 0, eos, pad); lim != QTX_OK)
    return fail(lim, "beam select: beam %d, eos %lld, pad %lld, tgt_vocab %d", beam,
                (long long)eos, (long long)pad, m->cfg.tgt_vocab);
  HIPCHK(launch_beam_select(logits, B, beam, m->cfg.tgt_vocab, (int)eos, (int)pad, max_len,
                            step_dev, score, fin, len, parent, bp_par, bp_tok, m->tgt_lut, m->pe,
                            m->cfg.max_len, x_next, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_beam_reorder(int8_t* kc, int8_t* vc, float* skc, float* svc, int32_t B, int32_t beam,
                         int32_t max_len, int32_t n_layers, int64_t k_ls, int64_t v_ls,
                         int64_t s_ls, int32_t v_grouped, const int32_t* step_dev,
                         const int32_t* parent, void* stream) {
  if (!kc || !vc || !skc || !svc || !step_dev || !parent) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || beam < 1 || beam > BEAM_MAXK || max_len < 1 || max_len > 512 || n_layers < 1)
    return fail(QTX_E_INVALID, "bad shape B=%d beam=%d max_len=%d layers=%d", B, beam, max_len,
                n_layers);
  const BeamGeom g{max_len, v_grouped ? 1 : 0};
  if (k_ls < (int64_t)B * beam * g.k_row() || v_ls < (int64_t)B * beam * g.v_row() ||
      s_ls < (int64_t)B * beam * g.s_row() || k_ls % 16 || v_ls % 16 || !aligned16(kc) ||
      !aligned16(vc))
    return fail(QTX_E_INVALID, "beam reorder: layer strides below B * beam rows, or codes not "
                               "16-byte aligned");
  HIPCHK(launch_beam_reorder(kc, vc, skc, svc, B, beam, max_len, n_layers, k_ls, v_ls, s_ls,
                             g.grouped, step_dev, parent, (hipStream_t)stream));
  return QTX_OK;
}

}  // extern "C"

// =======================================================================================
// Teacher-forced target scoring (include/qtx.h: qtx_score_targets)
// =======================================================================================
namespace {

// One generator chunk's logits at the model-level call: at most 64 MiB, there only to bound
// the workspace whatever R * T is.  Larger chunks measured faster all the way to one launch
// (cfg2's shape, 2272 rows, V = 4444: generator + tail 1.043 / 0.371 / 0.235 / 0.204 ms with
// chunks of 64 / 256 / 928 / all rows, profiles/score_bench.md).
constexpr size_t SCORE_CHUNK_BYTES = (size_t)64 << 20;

// Rows of logits per generator launch that `bytes` of workspace hold: a multiple of 16 (the
// generator's row block) with chunk * V below 2^30 (its 32-bit offsets), at most M; 0 when
// not even 16 rows fit.
int score_chunk(size_t bytes, int V, long M) {
  size_t rows = bytes / (4 * (size_t)V);
  rows = std::min(rows, (size_t)(((1L << 30) - 1) / V)) & ~(size_t)15;
  if (rows < 16) return 0;
  return (int)std::min(rows, (size_t)M);
}

// what the model-level call reserves for a chunk's logits
size_t score_logits_bytes(int V, long M) {
  const size_t rows = std::max((size_t)16, (SCORE_CHUNK_BYTES / (4 * (size_t)V)) & ~(size_t)15);
  return std::min(rows, ((size_t)M + 15) & ~(size_t)15) * (size_t)V * 4;
}

// The generator on x [M, D] (the final LayerNorm already applied) in chunks of `chunk` rows,
// each followed by k_lsm_score on the chunk's logits; label of row g: y[(g / y_t) * y_l + g % y_t].
int score_rows_run(const qtx_model* m, const float* x, long M, const int64_t* y, int y_t, int y_l,
                   float* tok_logp, int* rank, int64_t* top_ids, float* top_logp, float* logits,
                   int chunk, hipStream_t st) {
  const qtx_config& c = m->cfg;
  for (long r0 = 0; r0 < M; r0 += chunk) {
    const int n = (int)std::min((long)chunk, M - r0);
    HIPCHK(launch_generator_mfma(x + r0 * c.d_model, c.d_model, n, nullptr, nullptr, m->gen_wt,
                                 m->gen_b, c.tgt_vocab, logits, st));
    HIPCHK(launch_lsm_score(logits, n, c.tgt_vocab, y, r0, y_t, y_l, tok_logp, rank, top_ids,
                            top_logp, st));
  }
  return QTX_OK;
}

struct ScoreWS {
  Scratch enc, dec;     // B * S source rows; R * T target rows
  CrossKV cross;        // the B sentences' golden cross K/V
  CrossKV fcross;       // a faulty trial's own copy (encoder fault, CK / CV fault)
  CrossKV rcross;       // tgt_per_src > 1: the golden ones replicated to the R rows
  float* memory;        // [B * S, D] golden
  float* fmemory;       // an encoder-fault trial's
  uint8_t* rmask;       // [R, S] the source mask per row (tgt_per_src > 1)
  uint8_t* tmask;       // [R, T, T] (pad < 0: [T, T])
  float* out;           // [R * T, D] the decoder's output
  float* logits;        // one chunk
  size_t logits_bytes;
};

ScoreWS carve_score(Arena& ar, const qtx_config& c, long B, long S, long L, long K, long nf) {
  ScoreWS w;
  const size_t D = c.d_model, NL = c.n_layers, R = (size_t)(B * K), T = (size_t)(L - 1);
  const size_t Ms = (size_t)(B * S);
  w.enc = carve_scratch(ar, c, (long)Ms);
  w.dec = carve_scratch(ar, c, (long)(R * T));
  w.cross = carve_cross(ar, c, (long)Ms);
  w.memory = ar.take<float>(Ms * D);
  w.fmemory = nullptr;
  if (nf > 0) {
    w.fcross = carve_cross(ar, c, (long)Ms);
    w.fmemory = ar.take<float>(Ms * D);
  }
  w.rmask = nullptr;
  if (K > 1) {   // the layout of carve_cross (tile 2 l + {0: K, 1: V}), R * S rows
    w.rcross.am8 = nullptr; w.rcross.sam = nullptr; w.rcross.y = nullptr;
    int8_t* kv = ar.take<int8_t>(2 * NL * R * S * D);
    float* sc = ar.take<float>(2 * NL * R * S);
    for (size_t l = 0; l < NL; ++l) {
      w.rcross.k8.push_back(kv ? kv + 2 * l * R * S * D : nullptr);
      w.rcross.v8.push_back(kv ? kv + (2 * l + 1) * R * S * D : nullptr);
      w.rcross.sk.push_back(sc ? sc + 2 * l * R * S : nullptr);
      w.rcross.sv.push_back(sc ? sc + (2 * l + 1) * R * S : nullptr);
    }
    w.rmask = ar.take<uint8_t>(R * S);
  }
  w.tmask = ar.take<uint8_t>(R * T * T);
  w.out = ar.take<float>(R * T * D);
  w.logits_bytes = score_logits_bytes(c.tgt_vocab, (long)(R * T));
  w.logits = ar.take<float>(w.logits_bytes / 4);
  return w;
}

size_t score_ws(const qtx_config& c, long B, long S, long L, long K, long nf) {
  Arena ar;
  carve_score(ar, c, B, S, L, K, nf);
  return align_up(ar.used);
}

}  // namespace

extern "C" {

size_t qtx_score_workspace_size(const qtx_model* m, int32_t B, int32_t S, int32_t L,
                                int32_t tgt_per_src, int32_t n_faults) {
  if (!m || B <= 0 || S <= 0 || L < 2 || tgt_per_src < 1 || n_faults < 0) return 0;
  return score_ws(m->cfg, B, S, L, tgt_per_src, n_faults);
}

int32_t qtx_score_targets(const qtx_model* m, const int64_t* src, const uint8_t* src_mask,
                          int32_t B, int32_t S, const int64_t* tgt, int32_t L,
                          int32_t tgt_per_src, int64_t pad, const qtx_fault* faults,
                          int32_t n_faults, float* tok_logp, int32_t* rank, int64_t* top_ids,
                          float* top_logp, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !src || !src_mask || !tgt || !tok_logp || !rank || !ws)
    return fail(QTX_E_INVALID, "null argument");
  if (!top_ids != !top_logp) return fail(QTX_E_INVALID, "top_ids and top_logp come as a pair");
  const qtx_config& c = m->cfg;
  const int K = tgt_per_src, T = L - 1;
  if (bad_decode_shape(c, B, S, T) || K < 1)
    return fail(QTX_E_INVALID, "bad shape B=%d S=%d L=%d tgt_per_src=%d", B, S, L, K);
  if (c.tgt_vocab < 2) return fail(QTX_E_INVALID, "scoring needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (n_faults < 0 || (n_faults > 0 && !faults))
    return fail(QTX_E_INVALID, "n_faults %d without a fault array", n_faults);
  const long Rl = (long)B * K;
  if (Rl * T * c.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "target scoring: B * tgt_per_src * (L - 1) * d_model must be "
                                   "below 2^30");
  if (n_faults > 0) {
    if (c.weight_bits != 8) return fail(QTX_E_UNSUPPORTED, "fault injection needs 8-bit weights");
    if (K != 1) return fail(QTX_E_UNSUPPORTED, "fault trials need tgt_per_src == 1 (%d)", K);
    for (int n = 0; n < n_faults; ++n) {
      const qtx_fault* f = faults + n;
      if (f->kind == QTX_FAULT_NONE) return fail(QTX_E_INVALID, "fault %d: kind NONE", n);
      if (f->module == 0) RC(check_fault(m, f, 0, B, S, 0));
      else if (f->module == 1) RC(check_fault(m, f, 1, B, T, S));
      else return fail(QTX_E_INVALID, "fault %d: module %d", n, f->module);
    }
  }
  if (ws_bytes < score_ws(c, B, S, L, K, n_faults))
    return fail(QTX_E_WORKSPACE, "workspace too small");
  dfault_forget(m, ws);
  hipStream_t st = (hipStream_t)stream;
  Arena ar;
  ar.base = (uint8_t*)ws; ar.cap = ws_bytes;
  unsigned* cst = nullptr;
  RC(call_status_begin(m, &cst, st));
  ScoreWS w = carve_score(ar, c, B, S, L, K, n_faults);
  w.enc.status = cst;
  const int D = c.d_model, R = (int)Rl, Ms = B * S;
  const long M = (long)R * T;
  auto embed_src = [&]() -> int {
    HIPCHK(launch_embed(src, S, B, S, nullptr, 0, m->src_lut, c.src_vocab, m->pe, c.max_len,
                        w.enc.x, (long)S * D, st));
    return QTX_OK;
  };
  // the golden encoder pass and cross K/V, once on the B sentences (greedy_prologue's)
  RC(embed_src());
  RC(encoder_run(m, w.enc.x, src_mask, B, S, w.memory, w.enc, st, nullptr));
  RC(cross_kv(m, w.memory, Ms, w.cross, st));
  const CrossKV* gx = &w.cross;
  const uint8_t* rmask = src_mask;
  if (K > 1) {   // row r reads the cross K/V and the source mask of sentence r / K
    for (int l = 0; l < c.n_layers; ++l) {
      HIPCHK(launch_beam_rep(w.cross.k8[l], w.rcross.k8[l], B, K, (long)S * D, st));
      HIPCHK(launch_beam_rep(w.cross.v8[l], w.rcross.v8[l], B, K, (long)S * D, st));
      HIPCHK(launch_beam_rep(w.cross.sk[l], w.rcross.sk[l], B, K, S * 4L, st));
      HIPCHK(launch_beam_rep(w.cross.sv[l], w.rcross.sv[l], B, K, S * 4L, st));
    }
    HIPCHK(launch_beam_rep(src_mask, w.rmask, B, K, S, st));
    gx = &w.rcross;
    rmask = w.rmask;
  }
  long tm_bs = 0;
  if (pad >= 0) {
    HIPCHK(launch_std_mask(tgt, R, L, pad, w.tmask, st));
    tm_bs = (long)T * T;
  } else {
    HIPCHK(launch_causal_mask(w.tmask, T, st));
  }
  for (int n = 0; n <= n_faults; ++n) {   // trial 0 golden, trial n: faults[n - 1]
    const qtx_fault* f = n ? faults + n - 1 : nullptr;
    const CrossKV* x = gx;
    if (f && f->module == 0) {   // the encoder and the cross K/V again, into the trial's own buffers
      RC(embed_src());
      RC(encoder_run(m, w.enc.x, src_mask, B, S, w.fmemory, w.enc, st, f));
      RC(cross_kv(m, w.fmemory, Ms, w.fcross, st));
      x = &w.fcross;
      f = nullptr;
    } else if (f) {              // a memory K / V projection fault: its own cross copy
      bool ckv_fault = false;
      for (int l = 0; l < c.n_layers; ++l)
        ckv_fault |= fault_for(f, 1, l, G_CKV, Ms, c).kind != FK_NONE;
      if (ckv_fault) {
        RC(cross_kv(m, w.memory, Ms, w.fcross, st, f));
        x = &w.fcross;
      }
    }
    HIPCHK(launch_embed(tgt, L, R, T, nullptr, 0, m->tgt_lut, c.tgt_vocab, m->pe, c.max_len,
                        w.dec.x, (long)T * D, st));
    RC(decoder_body(m, w.dec, *x, rmask, w.tmask, tm_bs, R, T, S, w.out, f, st));
    const long o = (long)n * M;
    RC(score_rows_run(m, w.out, M, tgt + 1, T, L, tok_logp + o, rank + o,
                      top_ids ? top_ids + 2 * o : nullptr, top_logp ? top_logp + 2 * o : nullptr,
                      w.logits, score_chunk(w.logits_bytes, c.tgt_vocab, M), st));
  }
  return QTX_OK;
}

int32_t qtx_score_logits(const float* logits, const int64_t* y, int32_t M, int32_t V,
                         float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                         void* stream) {
  if (!logits || !y || !tok_logp || !rank) return fail(QTX_E_INVALID, "null argument");
  if (!top_ids != !top_logp) return fail(QTX_E_INVALID, "top_ids and top_logp come as a pair");
  if (V < 2) return fail(QTX_E_INVALID, "scoring needs V >= 2 (%d)", V);
  if (M <= 0) return QTX_OK;
  HIPCHK(launch_lsm_score(logits, M, V, y, 0, 1, 1, tok_logp, rank, top_ids, top_logp,
                          (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_score_rows(const qtx_model* m, const float* x, int32_t M, const int64_t* y,
                       float* tok_logp, int32_t* rank, int64_t* top_ids, float* top_logp,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!m || !x || !y || !tok_logp || !rank || !ws) return fail(QTX_E_INVALID, "null argument");
  if (!top_ids != !top_logp) return fail(QTX_E_INVALID, "top_ids and top_logp come as a pair");
  const int V = m->cfg.tgt_vocab;
  if (V < 2) return fail(QTX_E_INVALID, "scoring needs tgt_vocab >= 2 (%d)", V);
  if (M <= 0) return QTX_OK;
  if ((long)M * m->cfg.d_model >= (1L << 30))
    return fail(QTX_E_UNSUPPORTED, "score rows: M * d_model must be below 2^30");
  const int chunk = score_chunk(ws_bytes, V, M);
  if (!chunk) return fail(QTX_E_WORKSPACE, "ws holds fewer than 16 rows of logits");
  return score_rows_run(m, x, M, y, 1, 1, tok_logp, rank, top_ids, top_logp, (float*)ws, chunk,
                        (hipStream_t)stream);
}

}  // extern "C"

extern "C" {

// ---- per-op entry points ---------------------------------------------------------------
int32_t qtx_row_quant(const float* x, int32_t rows, int32_t D, float qmax, int8_t* q,
                      float* s, void* stream) {
  if (!x || !q || !s) return fail(QTX_E_INVALID, "null argument");
  RowArgs a = rows_quant(x, D, rows, D, q, s);
  a.qmax = qmax;
  hipError_t e = launch_rows(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "D=%d unsupported", D);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_layernorm_quant(const float* x, const float* a, const float* b, int32_t rows,
                            int32_t D, float* y, int8_t* q, float* s, void* stream) {
  if (!x || !a || !b || (!y && !q)) return fail(QTX_E_INVALID, "null argument");
  RowArgs r{};
  r.x = x; r.ldx = D; r.rows = rows; r.D = D; r.ln_a = a; r.ln_b = b;
  r.yout = y; r.ldy = D; r.q = q; r.ldq = D; r.s = s; r.qmax = 127.0f;
  r.rpb = rows > 0 ? rows : 1;
  hipError_t e = launch_rows(r, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "D=%d unsupported", D);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_linear_i8(const int8_t* A, const float* sa, const void* W, const float* sw,
                      const float* bias, int32_t M, int32_t N, int32_t K, int32_t weight_bits,
                      int32_t flags, const float* res, float* out, void* stream) {
  if (!A || !sa || !W || !sw || !bias || !out) return fail(QTX_E_INVALID, "null argument");
  if ((flags & EPI_RESIDUAL) && !res) return fail(QTX_E_INVALID, "residual flag without res");
  if (K % 64) return fail(QTX_E_UNSUPPORTED, "K=%d not a multiple of 64", K);
  GemmArgs g{};
  g.A = A; g.lda = K; g.sa = sa; g.W = (const int8_t*)W;
  g.ldw = weight_bits == 8 ? K : K / 2; g.sw = sw; g.bias = bias;
  g.out = out; g.ldo = N; g.res = res; g.ldr = N;
  g.M = M; g.N = N; g.K = K; g.flags = flags;
  hipError_t e = launch_gemm(g, weight_bits, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "weight_bits=%d", weight_bits);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_linear_rows(const qtx_row_gemm* a, void* stream) {
  if (!a || !a->A || !a->sa || !a->W || !a->sw || !a->bias) return fail(QTX_E_INVALID, "null argument");
  RowGemmArgs g{};
  g.A = a->A; g.lda = a->K; g.sa = a->sa; g.W = a->W; g.ldw = a->K; g.sw = a->sw;
  g.bias = a->bias; g.M = a->M; g.N = a->N; g.K = a->K; g.epi = a->epi;
  g.out8 = a->out8; g.ldo8 = a->ldo8; g.o8_ts = a->o8_ts; g.os = a->os; g.os_ts = a->os_ts;
  g.res = a->res; g.xout = a->xout; g.ln_a = a->ln_a; g.ln_b = a->ln_b;
  g.lnq = a->lnq; g.lns = a->lns; g.lnout = a->lnout;
  g.pmax_out = a->pmax_out; g.pmax_in = a->pmax_in; g.pmax_n = a->pmax_n; g.kp = a->kp;
  g.status = reinterpret_cast<unsigned*>(a->status);
  g.part = a->part; g.ksplit = a->ksplit;
  if (g.ksplit > 1 && (g.epi != RE_RES_LN || g.kp != 1 || !g.part || (g.ksplit & (g.ksplit - 1)) ||
                       g.ksplit > 8))
    return fail(QTX_E_INVALID, "ksplit %d: epi 1 with kp 1, a power of two <= 8, and part", g.ksplit);
  if (g.ksplit > 1 && (g.K % 64 || (g.K / 64) % (4 * g.ksplit)))   // launch_gemm_row's split
    return fail(QTX_E_INVALID, "ksplit %d needs K / 64 a multiple of 4 * ksplit (K=%d)", g.ksplit, g.K);
  const bool ok = (g.epi == RE_QUANT && g.out8 && g.os) ||
                  (g.epi == RE_RES_LN && g.res && g.xout && g.ln_a && g.ln_b &&
                   (g.lnq ? g.lns != nullptr : g.lnout != nullptr)) ||
                  (g.epi == RE_RELU_PMAX && g.pmax_out) ||
                  (g.epi == RE_RELU_QUANT_PMAX && g.out8 && g.os &&
                   (g.kp == 3 || g.kp == 5 ? g.pmax_out != nullptr : (g.pmax_in && g.pmax_n > 0)));
  if (!ok) return fail(QTX_E_INVALID, "operands missing for epi %d", g.epi);
  // A, W and out8 move in 16-byte vectors (k_gemm_row: plain stores; the WS kernels: buffer
  // stores through a descriptor of M * ldo8 bytes), so their bases and the out8 strides must
  // be multiples of 16 and a row must hold its tile — checked here, before any launch
  if (!aligned16(g.A) || !aligned16(g.W))
    return fail(QTX_E_INVALID, "A / W must be 16-byte aligned");
  if (g.epi == RE_QUANT || g.epi == RE_RELU_QUANT_PMAX) {
    const long row = g.epi == RE_QUANT ? 512 : g.N;
    if (!aligned16(g.out8) || g.ldo8 < row || g.ldo8 % 16 || (g.kp && g.epi != RE_QUANT && g.ldo8 % 64))
      return fail(QTX_E_INVALID, "out8 must be 16-byte aligned with ldo8 %% 16 == 0 (KP: %% 64) "
                                 "and ldo8 >= %ld (ldo8=%ld)", row, (long)g.ldo8);
    if (g.epi == RE_QUANT && (g.o8_ts % 16 || g.o8_ts < 0 || g.os_ts < 0))
      return fail(QTX_E_INVALID, "o8_ts must be a non-negative multiple of 16, os_ts >= 0 "
                                 "(o8_ts=%ld os_ts=%ld)", (long)g.o8_ts, (long)g.os_ts);
  }
  const hipError_t e = g.kp == 3 || g.kp == 5 ? launch_gemm_wsx(g, (hipStream_t)stream)
                       : g.kp == 2 || g.kp == 4 ? launch_gemm_ws(g, (hipStream_t)stream)
                                   : launch_gemm_row(g, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(QTX_E_UNSUPPORTED, "rows GEMM: N=%d K=%d epi=%d kp=%d", g.N, g.K, g.epi, g.kp);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_pack_w_kp(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream) {
  if (!W || !out) return fail(QTX_E_INVALID, "null argument");
  const hipError_t e = launch_pack_w_kp(W, N, K, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "pack_w_kp N=%d K=%d", N, K);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_ffn_rows(const qtx_ffn_args* a, void* stream) {
  if (!a || !a->A || !a->sa || !a->wf || !a->sw1 || !a->b1 || !a->sw2 || !a->b2 || !a->x ||
      !a->ln_a || !a->ln_b || (a->lnq ? !a->lns : !a->lnout))
    return fail(QTX_E_INVALID, "null argument");
  FfnArgs g{};
  g.A = a->A; g.sa = a->sa; g.wf = a->wf; g.sw1 = a->sw1; g.b1 = a->b1; g.sw2 = a->sw2;
  g.b2 = a->b2; g.x = a->x; g.ln_a = a->ln_a; g.ln_b = a->ln_b; g.lnq = a->lnq;
  g.lns = a->lns; g.lnout = a->lnout; g.M = a->M; g.F = a->F;
  const hipError_t e = launch_ffn_fused(g, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "ffn_rows: F=%d", a->F);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_pack_ffn(const int8_t* W1, const int8_t* W2, int32_t F, int8_t* out, void* stream) {
  if (!W1 || !W2 || !out) return fail(QTX_E_INVALID, "null argument");
  const hipError_t e = launch_pack_ffn(W1, W2, F, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "pack_ffn F=%d", F);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_pack_w_ws(const int8_t* W, int32_t N, int32_t K, int8_t* out, void* stream) {
  if (!W || !out) return fail(QTX_E_INVALID, "null argument");
  const hipError_t e = launch_pack_w_ws(W, N, K, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "pack_w_ws N=%d K=%d", N, K);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_skinny_linear(int32_t amode, const int8_t* A, const float* sa, const float* X,
                          int64_t ldx, const float* ln_a, const float* ln_b,
                          const float* pmax_in, int32_t pmax_n, const void* W, const float* sw,
                          const float* bias, int32_t M, int32_t N, int32_t K,
                          int32_t weight_bits, int32_t flags, const float* res, float* out,
                          float* pmax_out, void* stream) {
  if (!W || !sw || !bias || !out) return fail(QTX_E_INVALID, "null argument");
  if ((amode == A_I8 && (!A || !sa)) || (amode == A_LN && (!X || !ln_a || !ln_b)) ||
      (amode == A_F32Q && (!X || !pmax_in || pmax_n <= 0 || pmax_n > 128)) ||
      (amode == A_F32R && !X) || amode < 0 || amode > 3)
    return fail(QTX_E_INVALID, "operands missing for amode %d", amode);
  if (((flags & EPI_RESIDUAL) && !res) || ((flags & EPI_ROWMAX) && !pmax_out))
    return fail(QTX_E_INVALID, "flags need res / pmax_out");
  // the A / X rows and the W fragments are read in 16-byte vectors (8-byte for 4-bit W)
  if (!aligned16(W) || (amode == A_I8 ? !aligned16(A) : (!aligned16(X) || ldx < K || ldx % 4)))
    return fail(QTX_E_INVALID, "skinny: A / X / W must be 16-byte aligned, ldx %% 4 == 0 and "
                               "ldx >= K (ldx=%ld)", (long)ldx);
  SkinnyArgs g{};
  g.amode = amode; g.A = A; g.sa = sa; g.X = X; g.ldx = ldx; g.ln_a = ln_a; g.ln_b = ln_b;
  g.pmax_in = pmax_in; g.pmax_n = pmax_n;
  g.W = (const int8_t*)W; g.ldw = weight_bits == 8 ? K : K / 2;
  g.sw = sw; g.bias = bias; g.out = out; g.ldo = N; g.res = res; g.ldr = N;
  g.pmax_out = pmax_out; g.M = M; g.N = N; g.K = K; g.flags = flags;
  hipError_t e = launch_skinny(g, weight_bits, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(QTX_E_UNSUPPORTED, "skinny: N=%d K=%d amode=%d bits=%d", N, K, amode, weight_bits);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_decode_attention(int32_t kv_new, const float* y, int64_t ldy, int8_t* kc,
                             int8_t* vc, float* skc, float* svc, int32_t kv_bs,
                             const int32_t* step_dev, int32_t S, const uint8_t* mask,
                             int32_t B, float* ctx, float* pmax, void* stream) {
  if (!y || !kc || !vc || !skc || !svc || !ctx || !pmax)
    return fail(QTX_E_INVALID, "null argument");
  if (kv_new ? (!step_dev || kv_bs <= 0 || kv_bs > 128)
             : (!mask || S <= 0 || S > 128 || S > kv_bs))
    return fail(QTX_E_INVALID, "decode attention: bad step/mask/S/kv_bs");
  // y rows and the cached key / value rows are read in 16-byte vectors
  if (!aligned16(y) || !aligned16(kc) || !aligned16(vc) || ldy % 4 || ldy < (kv_new ? 1536 : 512))
    return fail(QTX_E_INVALID, "decode attention: y / kc / vc must be 16-byte aligned, "
                               "ldy %% 4 == 0 and ldy >= the row width (ldy=%ld)", (long)ldy);
  DecAttnArgs a{};
  a.y = y; a.ldy = ldy; a.kc = kc; a.vc = vc; a.skc = skc; a.svc = svc; a.kv_bs = kv_bs;
  a.step = step_dev; a.S = S; a.mask = mask; a.kv_new = kv_new;
  a.ctx = ctx; a.pmax = pmax; a.B = B;
  HIPCHK(launch_dec_attn(a, B, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_debug_graph_stats(const qtx_model* m, int32_t* entries, int64_t* captures) {
  if (!m || !entries || !captures) return fail(QTX_E_INVALID, "null argument");
  qtx_model* mm = const_cast<qtx_model*>(m);
  std::lock_guard<std::mutex> lock(mm->mu);
  *entries = (int32_t)mm->sg.entries();
  *captures = mm->sg.captures();
  return QTX_OK;
}

int32_t qtx_debug_nop(void* stream) {
  HIPCHK(launch_nop((hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_decode_generator(const qtx_model* m, const float* x, int32_t M, float* logits,
                             float* rec, void* stream) {
  if (!m || !x || !logits) return fail(QTX_E_INVALID, "null argument");
  if (M <= 0) return QTX_OK;
  if (!aligned16(x) || (rec && !aligned16(rec)))
    return fail(QTX_E_INVALID, "x / rec must be 16-byte aligned");
  const hipError_t e = launch_generator_mfma(x, m->cfg.d_model, M, m->dec_norm[0], m->dec_norm[1],
                                             m->gen_wt, m->gen_b, m->cfg.tgt_vocab, logits,
                                             (hipStream_t)stream, rec);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "M * tgt_vocab >= 2^30");
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_decode_argmax_embed(const qtx_model* m, const float* logits, int32_t M,
                                int64_t* ids, int64_t ids_bs, int32_t* step_dev,
                                float* x_next, void* stream) {
  if (!m || !logits || !ids || !step_dev || !x_next) return fail(QTX_E_INVALID, "null argument");
  if (M <= 0) return QTX_OK;
  const qtx_config& c = m->cfg;
  const hipError_t e = launch_argmax_embed(logits, M, c.tgt_vocab, ids, ids_bs, step_dev,
                                           reinterpret_cast<unsigned*>(step_dev + 1),
                                           m->tgt_lut, m->pe, c.max_len, x_next,
                                           (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "tgt_vocab %d", c.tgt_vocab);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_decode_top2_embed(const qtx_model* m, const float* logits, int32_t M, int64_t* ids,
                              int64_t ids_bs, int64_t* top_ids, float* top_logp,
                              int32_t* step_dev, float* x_next, void* stream) {
  if (!m || !logits || !ids || !top_ids || !top_logp || !step_dev || !x_next)
    return fail(QTX_E_INVALID, "null argument");
  const qtx_config& c = m->cfg;
  if (c.tgt_vocab < 2) return fail(QTX_E_INVALID, "top 2 needs tgt_vocab >= 2 (%d)", c.tgt_vocab);
  if (M <= 0) return QTX_OK;
  const hipError_t e = launch_top2_embed(logits, M, c.tgt_vocab, ids, ids_bs, top_ids, top_logp,
                                         step_dev, reinterpret_cast<unsigned*>(step_dev + 1),
                                         m->tgt_lut, m->pe, c.max_len, x_next,
                                         (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(QTX_E_UNSUPPORTED, "tgt_vocab %d", c.tgt_vocab);
  HIPCHK(e);
  return QTX_OK;
}

int32_t qtx_pack_int4(const int8_t* q, int32_t N, int32_t K, uint8_t* packed, void* stream) {
  if (!q || !packed || K % 2) return fail(QTX_E_INVALID, "bad argument");
  HIPCHK(launch_pack_int4(q, N, K, packed, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_attention_trace(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                            const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                            int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                            float* ctx, float* qk_acc, float* p_codes, int32_t dec, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx) return fail(QTX_E_INVALID, "null argument");
  if (Sk <= 0 || Sk > 512 || Sq <= 0 || B <= 0 || H <= 0)
    return fail(QTX_E_UNSUPPORTED, "Sk=%d (max 512) Sq=%d B=%d H=%d", Sk, Sq, B, H);
  const long D = (long)H * 64;
  AttnArgs a{};
  a.q = q; a.q_bs = Sq * D; a.q_ld = D; a.sq = sq; a.sq_bs = Sq;
  a.k = k; a.k_bs = Sk * D; a.k_ld = D; a.sk = sk; a.sk_bs = Sk;
  a.v = v; a.v_bs = Sk * D; a.v_ld = D; a.sv = sv; a.sv_bs = Sk;
  a.mask = mask; a.m_bs = m_bs; a.m_is = m_is;
  a.ctx = ctx; a.c_bs = Sq * D; a.c_ld = D;
  a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk;
  a.dec = dec != 0;
  HIPCHK(launch_attn_trace(a, qk_acc, p_codes, (hipStream_t)stream));
  return QTX_OK;
}

int32_t qtx_attention_i8_quant(const int8_t* q, const float* sq, const int8_t* k,
                               const float* sk, const int8_t* v, const float* sv,
                               const uint8_t* key_mask, int32_t B, int32_t S, int8_t* ctx8,
                               float* sctx, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx8 || !sctx) return fail(QTX_E_INVALID, "null argument");
  if (B <= 0 || S <= 0 || S > 128) return fail(QTX_E_UNSUPPORTED, "S=%d (1..128)", S);
  const long D = 512;
  AttnArgs a{};
  a.q = q; a.q_bs = S * D; a.q_ld = D; a.sq = sq; a.sq_bs = S;
  a.k = k; a.k_bs = S * D; a.k_ld = D; a.sk = sk; a.sk_bs = S;
  a.v = v; a.v_bs = S * D; a.v_ld = D; a.sv = sv; a.sv_bs = S;
  a.mask = key_mask; a.m_bs = S; a.m_is = 0;
  a.c_bs = S * D; a.c_ld = D;
  a.B = B; a.H = 8; a.Sq = S; a.Sk = S;
  HIPCHK(launch_attention_encq(a, ctx8, sctx, (hipStream_t)stream, true));
  return QTX_OK;
}

int32_t qtx_attention_i8(const int8_t* q, const float* sq, const int8_t* k, const float* sk,
                         const int8_t* v, const float* sv, const uint8_t* mask, int64_t m_bs,
                         int64_t m_is, int32_t B, int32_t H, int32_t Sq, int32_t Sk,
                         float* ctx, int32_t dec, void* stream) {
  if (!q || !sq || !k || !sk || !v || !sv || !ctx) return fail(QTX_E_INVALID, "null argument");
  if (Sk <= 0 || Sk > 512 || Sq <= 0) return fail(QTX_E_UNSUPPORTED, "Sk=%d (max 512)", Sk);
  const long D = (long)H * 64;
  AttnArgs a{};
  a.q = q; a.q_bs = Sq * D; a.q_ld = D; a.sq = sq; a.sq_bs = Sq;
  a.k = k; a.k_bs = Sk * D; a.k_ld = D; a.sk = sk; a.sk_bs = Sk;
  a.v = v; a.v_bs = Sk * D; a.v_ld = D; a.sv = sv; a.sv_bs = Sk;
  a.mask = mask; a.m_bs = m_bs; a.m_is = m_is;
  a.ctx = ctx; a.c_bs = Sq * D; a.c_ld = D;
  a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk;
  a.dec = dec != 0;
  HIPCHK(launch_attention(a, (hipStream_t)stream));
  return QTX_OK;
}

}  // extern "C"
