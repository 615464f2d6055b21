// qtx_ws.h — the parts the weight-stationary K = 512 GEMMs are written from (qtx_wsgemm.hip and
// the diagnostic-only variants in diag/qtx_wsgemm_diag.hip; DESIGN.md §4 "Anatomy of a
// weight-stationary kernel"): layout constants, the LDS-DMA statements, work assignment, the
// resident-W prologue, the per-block plumbing (top wait, A-block issue, fragment fetches), y
// and its row maxima, the asm MFMA statements with their hazard padding and the pinned MFMA
// block, and the in-launch exchange of slice row maxima.  Each exists once, here; a kernel is
// a schedule over them.
#pragma once
#include "qtx_common.h"
#include "qtx_kernels.h"

namespace qtx {

constexpr int WS_K = 512, WS_R = 64;
constexpr int WS_STAGE = WS_R * WS_K;          // 32 KB: one A row block in fragment order
constexpr int WS_SR = 5;                        // K steps of W held in registers (rest: LDS)
constexpr int WS_WL = 8 * (8 - WS_SR) * 4 * 1024;   // W's LDS part: 96 KB

// Raw buffer stores with the hardware range check (a store at or past `bytes` is dropped):
// the epilogue's stores are then unconditional, so every wave issues the same known number
// of them and the next block's top can wait with a counted vmcnt instead of draining them.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ws_rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0,
                                           (int)(bytes < 0x7fffffffL ? bytes : 0x7fffffffL),
                                           0x00020000);
}
typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int WP_R = 32, WP_STAGE = WP_R * WS_K;    // 16 KB A stage

// Scheduling pattern for the compiler's IGroupLP: NM times {one MFMA, NV VALU} over the
// current scheduling region, so the epilogue arithmetic of the previous block is spread
// between this block's MFMAs instead of running before or after them (the matrix pipe
// and the vector issue then overlap: tools/probe_mfma_valu.hip)
template <int NM, int NV>
__device__ __forceinline__ void interleave() {
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);
  }
}
// s_waitcnt immediates (gfx9 encoding: vmcnt bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8)
constexpr int WAIT_VM(int n) { return (n & 15) | ((n >> 4) << 14) | 0x70 | 0xF00; }
constexpr int WAIT_LGKM0 = 0xC07F;

// ---- LDS-DMA: 16 / 4 bytes per lane, global -> LDS at the wave-uniform base lds_dst + the
// lane's offset.  Issued from inline asm so that the compiler does not track it (it would wait
// vmcnt(0) before any read of a stage with a DMA in flight); completion is waited for by
// hand (ws_top_wait).  M0 = the LDS destination, saved, set and restored inside the statement.
__device__ __forceinline__ void lds_dma16(const int8_t* gsrc, const uint8_t* lds_dst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds_dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
__device__ __forceinline__ void lds_dma4(const float* gsrc, const float* lds_dst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds_dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
               "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

// ---- work assignment: which 512-column slice t and which first row block r0 a workgroup
// takes; it then walks the row blocks r0, r0 + wpt, ... (WsWalk)
// By blockIdx.  XG: the nsl column-slice workgroups of a row group on one XCD (blockIdx % 8
// under round-robin placement — speed only), dispatched together, so a row block's A is
// fetched from HBM once and read from L2 by the other slices: of the first 8 * nsl * A
// workgroups, XCD x, slot j -> slice j % nsl of row group 8 * (j / nsl) + x; the rest (fewer
// than 8 * nsl) in blockIdx order after them.  XG = 0: slice = blockIdx % nsl.
template <int XG>
__device__ __forceinline__ void ws_assign(int nsl, int& t, int& r0) {
  t = blockIdx.x % nsl, r0 = blockIdx.x / nsl;
  if (XG) {
    const int b = blockIdx.x, A = gridDim.x / (8 * nsl), aligned = 8 * nsl * A;
    if (b < aligned) {
      const int j = b >> 3;
      t = j % nsl;
      r0 = 8 * (j / nsl) + (b & 7);
    } else {
      t = (b - aligned) % nsl;
      r0 = 8 * A + (b - aligned) / nsl;
    }
  }
}
// By arrival ticket (the one-pass FFN1 kernels, whose 4 slice workgroups of a row group wait
// for each other): the started workgroups always hold the lowest tickets, so groups whose 4
// tickets have all started run to completion and free their CUs, whatever else shares the
// GPU (another launch of the same kernel included): no co-residency assumption, no deadlock.
// The slices of a row group sit at tickets 8 apart: workgroups start about in blockIdx order
// and are dealt round-robin to the 8 XCDs, so the 4 partners mostly share an XCD (speed
// only); a group is complete once its highest ticket has started (any 25 started tickets
// hold one).  The ticket counter follows the nb row blocks' granules (WsExchange).
__device__ __forceinline__ void ws_assign_ticket(unsigned long long* gran, int nb, int& t, int& r0) {
  __shared__ int ticket;
  if (threadIdx.x == 0)
    ticket = (int)atomicAdd(reinterpret_cast<unsigned*>(gran + 4L * 32 * nb), 1u);
  __syncthreads();
  const int q = ticket;
  t = (q >> 3) & 3, r0 = (q & 7) + 8 * (q >> 5);
}
// The workgroup's row blocks: block k of its nblk is row block rb(k) (clamped: past the last
// one the last is named again, so every iteration issues the same DMAs and stores).
struct WsWalk {
  int r0, wpt, nblk;
  __device__ __forceinline__ WsWalk(int r0_, int wpt_, int nb) : r0(r0_), wpt(wpt_), nblk((nb - r0_ + wpt_ - 1) / wpt_) {}
  __device__ __forceinline__ int rb(int k) const { return r0 + min(k, nblk - 1) * wpt; }
};

// ---- fragments: piece p (1 KB in MFMA operand lane order) of an LDS area
__device__ __forceinline__ v4i ws_piece(const uint8_t* base, int p, int lane) {
  return *reinterpret_cast<const v4i*>(base + (p << 10) + lane * 16);
}
// W fragment j of K step s: K steps below SR from registers, the rest from W's LDS part
// (NJ fragments per K step, 32 / NJ K steps: 4 x 8 with the 16x16x64 MFMA, 2 x 16 with 32x32x32)
template <int SR, int NJ>
__device__ __forceinline__ v4i ws_bfrag(const v4i (&wr)[SR][NJ], const uint8_t* wl, int wave, int lane, int s, int j) {
  return s < SR ? wr[s < SR ? s : 0][j] : ws_piece(wl, (wave * (32 / NJ - SR) + s - SR) * NJ + j, lane);
}

// ---- resident W: this wave's fragments of slice t (64 columns, all of K; 32 KB in the WS /
// WS32 layout), resident for the whole launch.  The prologue is three statements in this order:
//   ws_load_w(wr, wl, g, t, wave, lane)   K steps 0..SR-1 into registers (K-step order: the
//                                         first MFMAs wait only for the first loads), the
//                                         rest into LDS (wl) by DMA; DMA_FIRST: the DMAs first
//   ws_fill_sw(swl, g, t, wave, lane)     the slice's sw [512], then bias [512] into LDS
//   ws_hold_w(wr)                         the registers consumed: otherwise the compiler's wait
//                                         for them lands at the top of the block loop, where
//                                         vmcnt(0) would also wait for the next block's DMA
//                                         every iteration
template <bool DMA_FIRST = false, int SR, int NJ>
__device__ __forceinline__ void ws_load_w(v4i (&wr)[SR][NJ], uint8_t* wl, const RowGemmArgs& g, int t, int wave, int lane) {
  constexpr int NS = 32 / NJ;
  const int8_t* wsrc = g.W + ((long)(t * 8 + wave) << 15);
  const v4i* ws = reinterpret_cast<const v4i*>(wsrc) + lane;
  if constexpr (DMA_FIRST) {
#pragma unroll
    for (int p = 0; p < (NS - SR) * NJ; ++p)
      lds_dma16(wsrc + ((SR * NJ + p) << 10) + lane * 16, wl + ((wave * (NS - SR) * NJ + p) << 10));
  }
#pragma unroll
  for (int s = 0; s < SR; ++s)
#pragma unroll
    for (int j = 0; j < NJ; ++j) wr[s][j] = ws[(s * NJ + j) * 64];
  if constexpr (!DMA_FIRST) {
#pragma unroll
    for (int p = 0; p < (NS - SR) * NJ; ++p)
      lds_dma16(wsrc + ((SR * NJ + p) << 10) + lane * 16, wl + ((wave * (NS - SR) * NJ + p) << 10));
  }
}
__device__ __forceinline__ void ws_fill_sw(float* swl, const RowGemmArgs& g, int t, int wave, int lane) {
  if (wave < 4) {                                  // wave w: 128 floats of each
    const int c = 128 * wave + 2 * lane;
    *reinterpret_cast<float2*>(swl + c) = *reinterpret_cast<const float2*>(g.sw + 512 * t + c);
    *reinterpret_cast<float2*>(swl + 512 + c) = *reinterpret_cast<const float2*>(g.bias + 512 * t + c);
  }
}
template <int SR, int NJ>
__device__ __forceinline__ void ws_hold_w(const v4i (&wr)[SR][NJ]) {
#pragma unroll
  for (int s = 0; s < SR; ++s)
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(wr[s][j]));
}

// ---- block plumbing
// The top of a block: this wave's DMA of the block retired, then every wave's part visible.
// VM_CNT_ORDER (qtx_common.h): a store issued after the DMA may retire before it, so a
// counted vmcnt that leaves the previous epilogue's stores in flight could release the
// barrier with the DMA still in flight — the wait is vmcnt(0).  (Compiler-visible waits: its
// own wait insertion then knows what they retired.)
__device__ __forceinline__ void ws_top_wait() {
  __builtin_amdgcn_s_waitcnt(WAIT_VM(0));
  __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
  __builtin_amdgcn_s_barrier();
}
// The 3 stores per wave of an iteration that has no block to quantize yet (range 0: dropped),
// so every iteration has the same vector-memory operations
__device__ __forceinline__ void ws_dummy_stores(const RowGemmArgs& g) {
  const __amdgpu_buffer_rsrc_t nul = ws_rsrc(g.out8, 0L);
#pragma unroll
  for (int d2 = 0; d2 < 3; ++d2) __builtin_amdgcn_raw_buffer_store_b32(0u, nul, 0, 0, 0);
}
// Row block rb (16 NF rows) of A into the stage st by LDS-DMA: wave w moves K step w of the
// NF row fragments (pieces of 8 KP lines).  With SA (NF = 2) also, into sa_slot, the block's 32 row
// scales, per wave (lanes 32-63 repeat them): no global load in the loop whose wait the
// compiler would count past the DMA (its counted vmcnt does not see the asm DMAs, so it
// would also wait for them).
template <int NF, bool SA>
__device__ __forceinline__ void ws_issue(const RowGemmArgs& g, uint8_t* st, float* sa_slot, int rb, int wave, int lane) {
  const int f = lane & 15, gq = lane >> 4;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const long row = min(rb * (16 * NF) + 16 * i + f, g.M - 1);
    lds_dma16(g.A + kp_off(row, 64 * wave + 16 * gq, WS_K), st + ((wave * NF + i) << 10));
  }
  if (SA) lds_dma4(g.sa + min(rb * (16 * NF) + (lane & (16 * NF - 1)), g.M - 1), sa_slot);
}
// red [2][8 waves][32]: the waves' partial row maxima of the blocks of k's parity
__device__ __forceinline__ float* ws_redb(float* red0, int k) { return red0 + (k & 1) * 8 * WP_R; }
// the slice's maximum of a row over its 8 waves' partials (complete after a barrier)
__device__ __forceinline__ float ws_slice_max(const float* red, int row) {
  float m = red[row];
#pragma unroll
  for (int w = 1; w < 8; ++w) m = fmaxf(m, red[w * WP_R + row]);
  return m;
}

// ---- y = ((float(acc) * sa[m]) * sw[n]) + b[n] of a 32-row block (lane: token rows 16i + f,
// columns cs + 4j + e -> y[i][4j + e]; sr: the two rows' scales, swl: sw and bias in LDS) and
// the wave's partial row maxima into red.  The max rule: |y| (Q/K/V), or with RELU_MAX y
// from 0 — the maximum of the ReLU'd row, y itself staying pre-ReLU (the one-pass FFN1,
// whose codes take the ReLU in their conversion, pack4_relu_u8).
template <bool RELU_MAX>
__device__ __forceinline__ void ws_form_y(const v4i (&acc)[2][4], const float (&sr)[2], const float* swl, float* red,
                                          float (&y)[2][16], int wave, int lane) {
  const int f = lane & 15, cs = 64 * wave + 16 * (lane >> 4);
  float am[2] = {0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 s4 = *reinterpret_cast<const float4*>(swl + cs + 4 * j);
    const float4 b4 = *reinterpret_cast<const float4*>(swl + 512 + cs + 4 * j);
    const float swj[4] = {s4.x, s4.y, s4.z, s4.w}, bj[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[i][4 * j + e] = ((float)acc[i][j][e] * sr[i]) * swj[e] + bj[e];
        am[i] = fmaxf(am[i], RELU_MAX ? y[i][4 * j + e] : fabsf(y[i][4 * j + e]));
      }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float a = am[i];
    a = fmaxf(a, __shfl_xor(a, 16));
    a = fmaxf(a, __shfl_xor(a, 32));
    red[wave * WP_R + 16 * i + f] = a;      // the 4 lane groups store the same value
  }
}

// Z: the block's first K step, accumulator from the inline constant 0.  (Zeroing it with
// VALU instead needs wait states before the MFMA reads it, which the compiler inserts only
// for MFMAs it knows about, not for these asm statements.)
template <bool Z, typename T>
__device__ __forceinline__ void mfma_pin(v4i& acc, const v4i& w, const v4i& a, float before, T& after) {
  // operands: %0 acc, %1 after (outputs first), %2 w, %3 a, %4 before
  if constexpr (Z)
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %2, %3, 0" : "=&v"(acc), "+v"(after) : "v"(w), "v"(a), "v"(before));
  else
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %2, %3, %0" : "+v"(acc), "+v"(after) : "v"(w), "v"(a), "v"(before));
}
template <bool Z>
__device__ __forceinline__ void mfma_asm(v4i& acc, const v4i& w, const v4i& a) {
  if constexpr (Z)
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(a));
  else
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(a));
}

// After the last asm MFMA of a block: the compiler tracks no wait states for asm MFMAs, so
// pad their results before anything reads them (every acc is an operand here, so no read,
// copy or spill of one moves above the pad).
__device__ __forceinline__ void mfma_settle(v4i (&acc)[2][4]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 4"
               : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]),
                 "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
}

// ---- the pinned MFMA block: the 64 MFMAs of a 32-row block (A stage cur) into acc, as asm
// statements (they keep their order; the compiler's list scheduler would put them back to
// back), and with Q the quantization of an earlier block kq (its y) between them in a fixed
// order: one output after every second MFMA, pinned by operands the asm text does not
// touch — the output LAG places back is an input of the MFMA, the next output's y an output
// of it, so the quantization's VALU fills the issue slots the matrix pipe leaves free.
//   scales(kq, bq, iq)       the rows' divisor and reciprocal per row fragment
//   cvt(y, bq, iq)           one output's conversion (the value the pack takes)
//   pack(t0, t1, t2, t3)     4 converted outputs -> 4 code bytes
//   store_row(kq, ii, d)     the lane's 16 codes of row fragment ii
template <int LAG, int SR, typename S, typename C, typename P, typename R>
__device__ __forceinline__ void ws_mfma_block(v4i (&acc)[2][4], const v4i (&wr)[SR][4], const uint8_t* cur,
                                              const uint8_t* wl, int wave, int lane, bool Q, int kq, float (&y)[2][16],
                                              const S& scales, const C& cvt, const P& pack, const R& store_row) {
  float bq[2] = {0.0f, 0.0f}, iq[2] = {0.0f, 0.0f};
  if (Q) scales(kq, bq, iq);
  float hist[3] = {0.0f, 0.0f, 0.0f}, tq[4];   // results of the last outputs, newest first
  uint32_t d[4];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    v4i a[2], b[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = ws_piece(cur, s * 2 + i, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = ws_bfrag(wr, wl, wave, lane, s, j);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = s * 8 + i * 4 + j;             // MFMA slot 0..63
        if (!Q || (n & 1) == 0) {
          if (s == 0) mfma_asm<true>(acc[i][j], b[j], a[i]);
          else mfma_asm<false>(acc[i][j], b[j], a[i]);
        } else {
          // quantized output o of block kq: row fragment ii, column group jj, element e
          const int o = n >> 1, ii = o >> 4, jj = (o >> 2) & 3, e = o & 3;
          float yv = y[ii][4 * jj + e];
          if (s == 0) mfma_pin<true>(acc[i][j], b[j], a[i], hist[LAG - 1], yv);
          else mfma_pin<false>(acc[i][j], b[j], a[i], hist[LAG - 1], yv);
          tq[e] = cvt(yv, bq[ii], iq[ii]);
          hist[2] = hist[1]; hist[1] = hist[0]; hist[0] = tq[e];
          if (e == 3) {
            d[jj] = pack(tq[0], tq[1], tq[2], tq[3]);
            if (jj == 3) store_row(kq, ii, d);
          }
        }
      }
  }
  mfma_settle(acc);
}

// ---- the in-launch exchange of slice row maxima (the one-pass FFN1: ReLU + per-token
// quantization over all 2048 columns without a row-max pre-pass).  The 4 workgroups holding
// the 4 slices of a row group (ws_assign_ticket) hand each other their rows' maxima over the
// slice: for each 32-row block one data-tagged 8-byte granule {tag 1, value} per row and
// slice, one relaxed agent-scope store each, read by the 3 partners with relaxed agent-scope
// loads (no flag, no fence: the tag travels with the value).  Scratch (g.pmax_out, zeroed
// before every launch; launch_gemm_wsx and tests/test_gpu_status.py know it): granules
// [nb][4 slices][32 rows] u64, the ticket counter, the status word.
// Every wait is bounded (lim polls): one that times out sets DEV_E_EXCHANGE_TIMEOUT in
// *status, which the host turns into an error — a block quantized from a partial maximum is
// never silent.
struct WsExchange {
  unsigned long long* gran;
  unsigned* status;
  unsigned lim;        // polls per wait (g.spin_limit)
  int t;               // this workgroup's slice
  int drop_slice;      // the test hook (QTX_WSX_DROP_SLICE) that withholds one slice's maxima
                       // so that its partners' waits time out; -1 in production
  int row;             // the lane's row of a block (lane & 31)
  __device__ __forceinline__ long gidx(int rb, int tt) const { return ((long)rb * 4 + tt) * 32 + row; }
  // this slice's maxima of row block rb (m: the lane's row); lanes 0-31 of one wave call it
  __device__ __forceinline__ void publish(int rb, float m) const {
    if (t != drop_slice)
      __hip_atomic_store(gran + gidx(rb, t), (1ull << 32) | __float_as_uint(m), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  // the row's maximum over all 4 slices: this slice's mloc, then the partners' granules
  __device__ __forceinline__ float full_max(int rb, float mloc) const {
    float m = mloc;
    for (unsigned spin = 0;; ++spin) {
      bool ok = true;
      float mx = mloc;
#pragma unroll
      for (int d = 1; d < 4; ++d) {
        const unsigned long long v = __hip_atomic_load(gran + gidx(rb, (t + d) & 3), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        ok &= (v >> 32) == 1ull;
        mx = fmaxf(mx, __uint_as_float((unsigned)v));
      }
      if (__all(ok)) { m = mx; break; }
      if (spin >= lim) {                            // bounded: never hang, never silent
        if ((threadIdx.x & 63) == 0)
          __hip_atomic_fetch_or(status, DEV_E_EXCHANGE_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    return m;
  }
};

#ifdef QTX_DIAG
// The asm MFMA statements of the diagnostic variants.  W in AGPRs (k_gemm_wsa / k_gemm_wsa2: the
// "a" constraint), 8 accumulators per wave and block:
template <bool Z, typename T>
__device__ __forceinline__ void mfma_pin_a(v4i& acc, const v4i& w, const v4i& a, float before, T& after) {
  if constexpr (Z)
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %2, %3, 0" : "=&v"(acc), "+v"(after) : "a"(w), "v"(a), "v"(before));
  else
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %2, %3, %0" : "+v"(acc), "+v"(after) : "a"(w), "v"(a), "v"(before));
}
template <bool Z>
__device__ __forceinline__ void mfma_asm_a(v4i& acc, const v4i& w, const v4i& a) {
  if constexpr (Z)
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(a));
  else
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(a));
}
__device__ __forceinline__ void mfma_settle8(v4i (&acc)[8]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 4"
               : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]),
                 "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]));
}
// The same statements for v_mfma_i32_32x32x32_i8 (k_gemm_wsq32 / k_gemm_wsy32): 16 accumulators
// per lane, 16 passes, so the settle pad is 24 wait states.
template <bool Z, typename T>
__device__ __forceinline__ void mfma32_pin(v16i& acc, const v4i& w, const v4i& a, float before, T& after) {
  if constexpr (Z)
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %2, %3, 0" : "=&v"(acc), "+v"(after) : "v"(w), "v"(a), "v"(before));
  else
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %2, %3, %0" : "+v"(acc), "+v"(after) : "v"(w), "v"(a), "v"(before));
}
template <bool Z>
__device__ __forceinline__ void mfma32_asm(v16i& acc, const v4i& w, const v4i& a) {
  if constexpr (Z)
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(a));
  else
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(a));
}
__device__ __forceinline__ void mfma32_settle(v16i (&acc)[2]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+v"(acc[0]), "+v"(acc[1]));
}

// qtx_wsgemm_diag.hip (diagnostic build only): the measured-negative weight-stationary
// variants the knobs select (QTX_WSQ=2/3/4, QTX_WSA2, QTX_WSY=0); hipErrorNotSupported when
// they select none
hipError_t launch_gemm_ws_diag(const RowGemmArgs& g, dim3 grid, hipStream_t st);
hipError_t launch_gemm_wsx_diag(const RowGemmArgs& a, int ng, hipStream_t st);
// k_gemm_wsq32 / k_gemm_wsy32 (RowGemmArgs kp = 4 / 5: W in the WS32 layout)
hipError_t launch_gemm_ws32_diag(const RowGemmArgs& g, dim3 grid, hipStream_t st);
hipError_t launch_gemm_wsy32_diag(const RowGemmArgs& a, int ng, hipStream_t st);
hipError_t launch_pack_w_ws32(const int8_t* W, int N, int K, int8_t* out, hipStream_t st);
#endif

}  // namespace qtx
