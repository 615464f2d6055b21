// qtx_model.hip — the model handle of the C-ABI (include/qtx.h): its loader, the calling
// thread's error text and device status words, and the frame and argument rules every
// model-level entry starts with (qtx_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "qtx_host.h"

#ifdef QTX_DIAG
namespace qtx {   // csrc/diag/qtx_wsgemm_diag.hip
hipError_t launch_pack_w_ws32(const int8_t* W, int N, int K, int8_t* out, hipStream_t st);
}
#endif

namespace qtx {

// the calling thread's last error text: defined here and nowhere else, written by fail()
static thread_local std::string g_err;

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

int stepgraph_hip_error(const char* what, hipError_t e) {
  return fail(QTX_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

// A call that rewrites a workspace drops the decoder-fault decode's header for it: a later
// qtx_greedy_dfault_resume on that memory is refused.
void dfault_forget(const qtx_model* mc, const void* ws) {
  qtx_model* m = const_cast<qtx_model*>(mc);
  std::lock_guard<std::mutex> lk(m->mu);
  m->dfault.erase(ws);
}

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
void release_slot(const CallStatus& c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  auto it = g_live.find(c.serial);
  if (it == g_live.end() || it->second != c.m) return;   // the model is gone
  qtx_model* m = it->second;
  std::lock_guard<std::mutex> lk2(m->slot_mu);
  m->slot_used[c.slot] = false;
}
struct ThreadCalls {
  std::vector<CallStatus> v;
  ~ThreadCalls() {
    for (const CallStatus& c : v) release_slot(c);
  }
};
// the calling thread's claimed slots: defined here and nowhere else, reached through
// held_status_word / thread_status_word
static thread_local ThreadCalls t_calls;

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

// ---- the argument rules and the frame of a model-level entry (qtx_host.h) ---------------
bool bad_decode_shape(const qtx_config& c, int B, int S, int T) {
  return B <= 0 || S <= 0 || S > 512 || T < 1 || T > 512 || T > c.max_len || S > c.max_len;
}
int check_decode_shape(const qtx_config& c, int B, int S, int max_len) {
  if (bad_decode_shape(c, B, S, max_len))
    return fail(QTX_E_INVALID, "bad shape B=%d S=%d max_len=%d", B, S, max_len);
  return QTX_OK;
}
int frame_begin(const qtx_model* m, void* ws, size_t ws_bytes, hipStream_t st, bool claim_status,
                CallFrame* f) {
  dfault_forget(m, ws);
  f->ar = ws_arena(ws, ws_bytes);
  f->status = nullptr;
  return claim_status ? call_status_begin(m, &f->status, st) : QTX_OK;
}

int copy_out(const int64_t* ws_ids, const int64_t* ws_top_ids, const float* ws_top_logp, int B,
             int max_len, int64_t* ids, int64_t* top_ids, float* top_logp, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(ids, ws_ids, (size_t)B * max_len * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  if (top_ids && max_len > 1) {
    const size_t n = (size_t)B * (max_len - 1) * 2;
    HIPCHK(hipMemcpyAsync(top_ids, ws_top_ids, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top_logp, ws_top_logp, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return QTX_OK;
}
int copy_out_record(const int64_t* ws_rec_ids, const float* ws_rec_logp, int B, int64_t* rec_ids,
                    float* rec_logp, hipStream_t st) {
  if (!rec_ids) return QTX_OK;
  HIPCHK(hipMemcpyAsync(rec_ids, ws_rec_ids, (size_t)B * 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(rec_logp, ws_rec_logp, (size_t)B * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return QTX_OK;
}

// ---- model layout ---------------------------------------------------------------------
// Linear order per layer follows qtx/weights.py:linear_names():
//   enc: self_attn.linears.0..3, w_1, w_2        (6 linears, 12 tensors)
//   dec: self_attn.linears.0..3, src_attn.linears.0..3, w_1, w_2   (10 linears)
int enc_tensor_base(const qtx_config& c, int L) { return 12 * L; }
int dec_tensor_base(const qtx_config& c, int L) { return 12 * c.n_layers + 20 * L; }
int norm_tensor_base(const qtx_config& c) { return 32 * c.n_layers; }

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

}  // namespace qtx

using namespace qtx;

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

int32_t qtx_model_check(const qtx_model* m, void* stream) {
  if (!m) return fail(QTX_E_INVALID, "null model");
  DeviceGuard dg(m->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned v = 0;
  unsigned* word = held_status_word(m);
  // no word: this thread has made no call on m that can raise a device error (the word is
  // per thread: a check reports the calling thread's calls only)
  if (!word) return QTX_OK;
  HIPCHK(hipMemcpy(&v, word, sizeof v, hipMemcpyDeviceToHost));
  if (!v) return QTX_OK;
  HIPCHK(hipMemset(word, 0, sizeof(unsigned)));   // reported once (the thread's own word)
  return fail(QTX_E_DEVICE, "%s", status_text(v));
}

}  // extern "C"
