// qtx_rowfault.hip — the kernels of the trials decode (include/qtx.h qtx_greedy_decode_kvtrials,
// qtx_linear_i8_rowfaults): the M = B GEMM that gives every row its own fault, and the masked
// copy of a step's top 2 into the record.  The host schedule is csrc/qtx_trials.hip.
#include "qtx_common.h"
#include "qtx_kernels.h"

namespace qtx {

// =====================================================================================
// k_gemm_rowfault: int8 x int8 -> int32 on v_mfma_i32_16x16x64_i8 for a few rows (M = the
// decode's batch).  Block tile 32 x 32, 4 waves as 2 x 2, one 16x16 fragment per wave; the
// operands go from global memory straight into the MFMA's registers (lane l supplies row
// l & 15, bytes k = 16 * (l >> 4) .. +15 of the 64-byte K step, on A and on W alike, so the
// dot product is exact for any hardware k order): at these M the A tile is a few KB that every
// workgroup re-reads from L2, and W is read once per 32 rows.  Four K steps are in flight.
// Epilogue: k_gemm's (qtx_kernels.hip), with the fault taken per row from the table — row r
// sees tab[r] alone, and only where the entry names this (step, layer, gemm).
// =====================================================================================
__global__ __launch_bounds__(256) void k_gemm_rowfault(GemmArgs g, const RowFault* tab, int step,
                                                       int layer, int gemm) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const int bm0 = blockIdx.y * 32 + wm * 16, bn0 = blockIdx.x * 32 + wn * 16;
  const int8_t* ap = g.A + (long)min(bm0 + fr, g.M - 1) * g.lda + fg * 16;
  const int8_t* wp = g.W + (long)min(bn0 + fr, g.N - 1) * g.ldw + fg * 16;

  v4i acc = v4i{0, 0, 0, 0};
  const int nk = g.K / 64;
  for (int kt = 0; kt < nk; kt += 4) {
    v4i af[4], bf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (kt + u < nk) {
        af[u] = *reinterpret_cast<const v4i*>(ap + (long)(kt + u) * 64);
        bf[u] = *reinterpret_cast<const v4i*>(wp + (long)(kt + u) * 64);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (kt + u < nk) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[u], bf[u], acc, 0, 0, 0);
  }

  // epilogue: C/D layout col = lane & 15, row = (lane >> 4) * 4 + e
  const bool relu = g.flags & EPI_RELU, resid = g.flags & EPI_RESIDUAL;
  const int col = bn0 + fr;
  if (col >= g.N) return;
  const float swc = g.sw[col], bc = g.bias[col];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = bm0 + fg * 4 + e;
    if (row >= g.M) continue;
    int a = acc[e];
    RowFault f{};
    if (tab) f = tab[row];
    const bool hit = f.kind != FK_NONE && f.step == step && f.layer == layer && f.gemm == gemm;
    const bool f_in = hit && f.kind == FK_INPUT, f_w = hit && f.kind == FK_WEIGHT;
    const bool f_out = hit && f.kind == FK_OUTPUT;
    int delta = 0;
    if (f_in || f_w) {
      const int8_t orig = f_in ? g.A[(long)row * g.lda + f.col] : g.W[(long)f.wrow * g.ldw + f.col];
      delta = (int)(int8_t)(orig ^ (1 << f.bit)) - (int)orig;
    }
    if (f_in && col >= f.lo && col < f.hi) a += delta * (int)g.W[(long)col * g.ldw + f.col];
    if (f_w && col == f.wrow) a += delta * (int)g.A[(long)row * g.lda + f.col];
    float y = ((float)a * g.sa[row]) * swc + bc;
    if (f_out && col == f.col) y = f.value + bc;
    if (relu) y = y > 0.0f ? y : 0.0f;
    if (resid) y = g.res[(long)row * g.ldr + col] + y;
    g.out[(long)row * g.ldo + col] = y;
  }
}

hipError_t launch_gemm_rowfault(const GemmArgs& g, const RowFault* tab, int step, int layer,
                                int gemm, hipStream_t st) {
  if (g.M <= 0 || g.N <= 0) return hipSuccess;
  if (g.K <= 0 || g.K % 64 != 0 || g.lda % 16 != 0 || g.ldw % 16 != 0 ||
      (reinterpret_cast<uintptr_t>(g.A) & 15) || (reinterpret_cast<uintptr_t>(g.W) & 15))
    return hipErrorInvalidValue;
  const dim3 grid((g.N + 31) / 32, (g.M + 31) / 32);
  k_gemm_rowfault<<<grid, dim3(256), 0, st>>>(g, tab, step, layer, gemm);
  return hipGetLastError();
}

// k_trial_record: one lane per sentence; the rows whose trial sits at `step` copy that step's
// entry of top_ids / top_logp [B][top_bs][2] into rec[b][which][:] (rec [B][2][2])
__global__ __launch_bounds__(64) void k_trial_record(int B, int step, int top_bs, int which,
                                                     const int* tstep, const int64_t* top_ids,
                                                     const float* top_logp, int64_t* rec_ids,
                                                     float* rec_logp) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || step >= top_bs || tstep[b] != step) return;
  const int e = 2 * (b * top_bs + step), r = 4 * b + 2 * which;
  rec_ids[r] = top_ids[e]; rec_ids[r + 1] = top_ids[e + 1];
  rec_logp[r] = top_logp[e]; rec_logp[r + 1] = top_logp[e + 1];
}

hipError_t launch_trial_record(const int64_t* top_ids, const float* top_logp, long top_bs,
                               int step, int B, const int* tstep, int which, int64_t* rec_ids,
                               float* rec_logp, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (step < 0 || step >= top_bs || (long)B * top_bs >= (1L << 29) || (which != 0 && which != 1))
    return hipErrorInvalidValue;
  k_trial_record<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(B, step, (int)top_bs, which, tstep,
                                                          top_ids, top_logp, rec_ids, rec_logp);
  return hipGetLastError();
}

}  // namespace qtx
