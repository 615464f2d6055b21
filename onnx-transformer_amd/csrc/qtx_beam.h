// qtx_beam.h — the beam-search decode's host-side bookkeeping that has no GPU in it: the
// geometry of a hypothesis' K/V cache regions (what k_beam_reorder moves per step, shared by
// the kernel, its launcher and the host checks) and the carving of the per-hypothesis search
// state.  Plain C++ (tools/beam_host_check.cpp runs it under the host sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QTX_HD __host__ __device__
#else
#define QTX_HD
#endif

namespace qtx {

constexpr int BEAM_MAXK = 8;

// One hypothesis' (row's) self K/V cache of one layer is four contiguous regions:
//   K codes  [max_len][512]                              16-byte chunks
//   V codes  grouped (fused step):  [ceil(max_len/4)][512][4]   (k_dec_attn's 4-key groups)
//            plain (unfused step):  [max_len][512]
//   the two scale vectors [max_len] float                4-byte chunks
// After n positions are valid (0 .. n-1) only this prefix of each region moves: n * 512 bytes of
// K, ceil(n / 4) groups (or n rows) of V, n floats of each scale vector.
struct BeamGeom {
  int max_len;
  int grouped;
  QTX_HD long k_row() const { return (long)max_len * 512; }                        // bytes
  QTX_HD long v_row() const {
    return grouped ? (long)((max_len + 3) / 4) * 2048 : (long)max_len * 512;
  }
  QTX_HD long s_row() const { return max_len; }                                    // floats
  QTX_HD int clamp(int n) const { return n < 0 ? 0 : (n > max_len ? max_len : n); }
  QTX_HD long k16(int n) const { return (long)clamp(n) * 32; }                      // 16-byte chunks
  QTX_HD long v16(int n) const {
    return grouped ? (long)((clamp(n) + 3) / 4) * 128 : (long)clamp(n) * 32;
  }
  QTX_HD long s4(int n) const { return clamp(n); }
  // chunks (threads) of one (layer, sentence) at n valid positions: K, V, then both scales
  QTX_HD long chunks(int n) const { return k16(n) + v16(n) + 2 * s4(n); }
  // Chunk (thread) i of a (layer, sentence) at n valid positions -> the region it owns a piece
  // of and the piece's offset inside one row's region: bytes for the codes (a 16-byte chunk),
  // floats for the scales (one float).  BEAM_NONE: past the prefix, nothing to move.  What
  // k_beam_reorder and the host check both index with.
  struct Chunk { int region; long off; };
  QTX_HD Chunk locate(int n, long i) const;
};
enum { BEAM_K = 0, BEAM_V = 1, BEAM_SK = 2, BEAM_SV = 3, BEAM_NONE = -1 };
QTX_HD inline BeamGeom::Chunk BeamGeom::locate(int n, long i) const {
  const long nk = k16(n), nv = v16(n), ns = s4(n);
  if (i < 0) return {BEAM_NONE, 0};
  if (i < nk) return {BEAM_K, i * 16};
  i -= nk;
  if (i < nv) return {BEAM_V, i * 16};
  i -= nv;
  if (i < ns) return {BEAM_SK, i};
  i -= ns;
  if (i < ns) return {BEAM_SV, i};
  return {BEAM_NONE, 0};
}

// The search state of R = B * beam rows (include/qtx.h, beam search): carved from an arena
// with `template <class T> T* take(size_t n)`.
struct BeamState {
  float* score;      // [R]
  int* fin;          // [R]
  int* len;          // [R]
  int* parent;       // [R] the latest step's parent slot (0 .. beam-1) of every row
  int* bp_par;       // [max_len-1][R] every step's parent slots ...
  int* bp_tok;       // [max_len-1][R] ... and tokens (back-pointers: k_beam_backtrack)
  int64_t* ids0;     // [R] the start symbol (the first decoder input)
};

template <class A>
BeamState carve_beam_state(A& ar, int B, int beam, int max_len) {
  const size_t R = (size_t)B * beam, T = max_len > 1 ? max_len - 1 : 1;
  BeamState s;
  s.score = ar.template take<float>(R);
  s.fin = ar.template take<int>(R);
  s.len = ar.template take<int>(R);
  s.parent = ar.template take<int>(R);
  s.bp_par = ar.template take<int>(T * R);
  s.bp_tok = ar.template take<int>(T * R);
  s.ids0 = ar.template take<int64_t>(R);
  return s;
}

// The argument limits of the beam decode (include/qtx.h): 0 ok, 1 invalid, 4 unsupported —
// the qtx_status values, checked before anything is launched.
inline int beam_limits(int B, int beam, int V, long long start, long long eos, long long pad) {
  if (B <= 0 || beam < 1 || beam > BEAM_MAXK || beam > V) return 1;
  if (start < 0 || start >= V || eos < 0 || eos >= V || pad < 0 || pad >= V || eos == pad) return 1;
  // (V, B * beam < 2^21: the select's 32-bit embedding offsets, 16 * (row * 128 + q))
  if ((long long)B * beam * V >= (1LL << 30) || V >= (1 << 21) || (long long)B * beam >= (1LL << 21))
    return 4;
  return 0;
}

}  // namespace qtx
