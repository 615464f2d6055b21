// carve_host_check.cpp — the decode and scoring workspaces' carving (csrc/qtx_carve.h:
// carve_greedy, group_view, carve_dfault, carve_kvfault, carve_score and their *_ws sizes) under
// the host sanitizers: a stand-alone program, no GPU and no HIP in it.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I onnx-transformer_amd/csrc tools/carve_host_check.cpp -o /tmp/carve_host_check && /tmp/carve_host_check
// For every workspace (greedy plain and scored, dfault, kvfault, score) and every shape of the
// grid below it carves an allocation of exactly *_ws bytes and checks: every region inside the
// allocation, no two overlapping, every region written over its whole extent (ASan: no byte
// past the end), the int8 code buffers the kernels read in 16-byte vectors 16-byte aligned, the
// plain greedy layout pointer for pointer a prefix of the scored one and the scored one a
// prefix of DfaultWS and KvfaultWS, and for two sub-batches the group_views' per-sentence
// regions disjoint and inside the parent's.  A table of sizes pins the layouts' byte counts
// (`--table` prints the rows in the table's form).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qtx_carve.h"

using namespace qtx;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// One carved region: [p, p + bytes); code: an int8 buffer read in 16-byte vectors.
struct Region { const char* name; uint8_t* p; size_t bytes; };
struct Regions {
  std::vector<Region> v;
  template <class T>
  void add(const char* name, T* p, size_t n, bool code = false) {
    CHECK(p != nullptr);
    CHECK(reinterpret_cast<uintptr_t>(p) % alignof(T) == 0);
    if (code) CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0);
    if (n) v.push_back({name, reinterpret_cast<uint8_t*>(p), n * sizeof(T)});
  }
  // inside [base, base + bytes), pairwise disjoint, each written with its own tag and read back
  void verify(uint8_t* base, size_t bytes) const {
    std::vector<Region> s = v;
    std::sort(s.begin(), s.end(), [](const Region& a, const Region& b) { return a.p < b.p; });
    for (size_t i = 0; i < s.size(); ++i) {
      CHECK(s[i].p >= base && s[i].p + s[i].bytes <= base + bytes);
      if (i + 1 < s.size() && s[i].p + s[i].bytes > s[i + 1].p) {
        std::fprintf(stderr, "regions %s and %s overlap\n", s[i].name, s[i + 1].name);
        std::exit(1);
      }
    }
    for (size_t i = 0; i < v.size(); ++i) std::memset(v[i].p, (int)(i + 1), v[i].bytes);
    for (size_t i = 0; i < v.size(); ++i)
      for (size_t e = 0; e < v[i].bytes; ++e) CHECK(v[i].p[e] == (uint8_t)(i + 1));
  }
};

// an allocation of exactly `bytes` (a multiple of 256), aligned as a device allocation is
struct Block {
  Arena ar;
  explicit Block(size_t bytes) {
    CHECK(bytes % 256 == 0);
    ar.base = static_cast<uint8_t*>(std::aligned_alloc(256, bytes ? bytes : 256));
    ar.cap = bytes;
    CHECK(ar.base);
  }
  ~Block() { std::free(ar.base); }
  void spent() const { CHECK(ar.used <= ar.cap && ar.cap - ar.used < 256); }
};

static void add_scratch(Regions& r, const Scratch& s, const qtx_config& c, size_t M) {
  const size_t D = c.d_model, F = c.d_ff, Y = 3 * D > F ? 3 * D : F;
  r.add("x", s.x, M * D);
  r.add("a8", s.a8, (M + 1) * (D > F ? D : F), true);
  r.add("sa", s.sa, M);
  r.add("y", s.y, M * Y);
  r.add("q8", s.q8, M * D, true); r.add("k8", s.k8, M * D, true); r.add("v8", s.v8, M * D, true);
  r.add("sq", s.sq, M); r.add("sk", s.sk, M); r.add("sv", s.sv, M);
  r.add("ctx", s.ctx, M * D);
  r.add("h8", s.h8, (M + 1) * F, true);
  r.add("sh", s.sh, M);
  r.add("pmax", s.pmax, (F / 512 + 1) * M);
  CHECK(s.k8 == s.q8 + M * D && s.v8 == s.k8 + M * D && s.sk == s.sq + M && s.sv == s.sk + M);
}

// rows: the K/V rows of every layer (Ms, or R * S of the replicated form); full: with the
// quantized memory and the fp32 GEMM scratch (not in the rows-only form)
static void add_cross(Regions& r, const CrossKV& x, const qtx_config& c, size_t rows, bool full) {
  const size_t D = c.d_model, L = c.n_layers;
  if (full) {
    r.add("am8", x.am8, rows * D, true);
    r.add("sam", x.sam, rows);
    r.add("cy", x.y, rows * 2 * D);
  } else {
    CHECK(!x.am8 && !x.sam && !x.y);
  }
  CHECK(x.k8.size() == L && x.v8.size() == L && x.sk.size() == L && x.sv.size() == L);
  for (size_t l = 0; l < L; ++l) {
    r.add("cross.k8", x.k8[l], rows * D, true);
    r.add("cross.v8", x.v8[l], rows * D, true);
    r.add("cross.sk", x.sk[l], rows);
    r.add("cross.sv", x.sv[l], rows);
    // one row GEMM writes all layers' K/V: tile 2 l + {0: K, 1: V}
    CHECK(x.k8[l] == x.k8[0] + 2 * l * rows * D && x.v8[l] == x.k8[l] + rows * D);
    CHECK(x.sk[l] == x.sk[0] + 2 * l * rows && x.sv[l] == x.sk[l] + rows);
  }
}

static void add_greedy(Regions& r, const GreedyWS& g, const qtx_config& c, const Groups& gr, int B,
                       int S, int max_len, bool scored) {
  const size_t D = c.d_model, L = c.n_layers, F = c.d_ff, V = c.tgt_vocab;
  const size_t Ms = (size_t)B * S, S4 = (size_t)(S + 3) / 4 * 4, ML4 = (size_t)(max_len + 3) / 4 * 4;
  add_scratch(r, g.enc, c, Ms);
  add_scratch(r, g.dec, c, B);
  add_cross(r, g.cross, c, Ms, true);
  CHECK(g.cvg.size() == L && g.kc.size() == L && g.vc.size() == L && g.skc.size() == L && g.svc.size() == L);
  for (size_t l = 0; l < L; ++l) {
    r.add("cvg", g.cvg[l], B * S4 * D, true);
    r.add("kc", g.kc[l], (size_t)B * max_len * D, true);
    r.add("skc", g.skc[l], (size_t)B * max_len);
    r.add("vc", g.vc[l], B * ML4 * D, true);
    r.add("svc", g.svc[l], (size_t)B * max_len);
    CHECK(g.cvg[l] == g.cvg[0] + l * B * S4 * D);   // launch_vgroup4's layer stride
  }
  r.add("memory", g.memory, Ms * D);
  r.add("xo", g.xo, B * D);
  r.add("logits", g.logits, B * V);
  r.add("step", g.step, 4);
  r.add("pmax_a", g.pmax_a, (size_t)8 * B);
  r.add("pmax_f", g.pmax_f, (F / 16) * B);
  CHECK((int)g.grp.size() == gr.G && g.grp[0].x == g.dec.x);
  for (int i = 1; i < gr.G; ++i) add_scratch(r, g.grp[i], c, gr.Bg);
  r.add("gsteps", g.gsteps, 4 * QTX_MAX_GROUPS);
  r.add("ids", g.ids, (size_t)B * max_len);
  r.add("mask", g.mask, Ms);
  r.add("rec", g.rec, B * ((V + 15) / 16) * 4);
  if (scored) {
    r.add("top_ids", g.top_ids, (size_t)B * (max_len - 1) * 2);
    r.add("top_logp", g.top_logp, (size_t)B * (max_len - 1) * 2);
  } else {
    CHECK(!g.top_ids && !g.top_logp);
  }
}

static void same_scratch(const Scratch& a, const Scratch& b) {
  CHECK(a.x == b.x && a.a8 == b.a8 && a.sa == b.sa && a.y == b.y && a.q8 == b.q8 && a.sq == b.sq);
  CHECK(a.k8 == b.k8 && a.sk == b.sk && a.v8 == b.v8 && a.sv == b.sv && a.ctx == b.ctx);
  CHECK(a.h8 == b.h8 && a.sh == b.sh && a.pmax == b.pmax);
}

// a's layout is pointer for pointer that of b (b may hold the scores on top)
static void same_greedy(const GreedyWS& a, const GreedyWS& b) {
  same_scratch(a.enc, b.enc);
  same_scratch(a.dec, b.dec);
  CHECK(a.cross.am8 == b.cross.am8 && a.cross.sam == b.cross.sam && a.cross.y == b.cross.y);
  CHECK(a.cross.k8 == b.cross.k8 && a.cross.v8 == b.cross.v8 && a.cross.sk == b.cross.sk && a.cross.sv == b.cross.sv);
  CHECK(a.cvg == b.cvg && a.kc == b.kc && a.vc == b.vc && a.skc == b.skc && a.svc == b.svc);
  CHECK(a.memory == b.memory && a.xo == b.xo && a.logits == b.logits && a.rec == b.rec);
  CHECK(a.step == b.step && a.pmax_a == b.pmax_a && a.pmax_f == b.pmax_f && a.gsteps == b.gsteps);
  CHECK(a.ids == b.ids && a.mask == b.mask && a.grp.size() == b.grp.size());
  for (size_t i = 0; i < a.grp.size(); ++i) same_scratch(a.grp[i], b.grp[i]);
}

// The sub-batches' views: each per-sentence buffer of view i covers rows b0(i) .. of the
// parent's, the views' ranges ascend without overlap and end inside the parent's.
static void views_case(const GreedyWS& g, const qtx_config& c, const Groups& gr, int B, int S,
                       int max_len) {
  const size_t D = c.d_model, V = c.tgt_vocab;
  const size_t S4 = (size_t)(S + 3) / 4 * 4, ML4 = (size_t)(max_len + 3) / 4 * 4;
  std::vector<GreedyWS> v;
  for (int i = 0; i < gr.G; ++i) v.push_back(group_view(g, c, i, gr.b0(i), S, max_len));
  int covered = 0;
  for (int i = 0; i < gr.G; ++i) {
    CHECK(gr.rows(i, B) > 0 && gr.b0(i) == covered);
    covered += gr.rows(i, B);
    CHECK(v[i].dec.x == g.grp[i].x && v[i].step == g.gsteps + 4 * i);
  }
  CHECK(covered == B);
  // per: bytes per sentence
  auto part = [&](auto field, size_t per) {
    for (int i = 0; i < gr.G; ++i) {
      const uint8_t* lo = reinterpret_cast<const uint8_t*>(field(v[i]));
      const uint8_t* p0 = reinterpret_cast<const uint8_t*>(field(g));
      CHECK(lo == p0 + (size_t)gr.b0(i) * per);   // hence disjoint, ascending, inside B * per
      CHECK(lo + (size_t)gr.rows(i, B) * per <= p0 + (size_t)B * per);
      if (i + 1 < gr.G)
        CHECK(lo + (size_t)gr.rows(i, B) * per <= reinterpret_cast<const uint8_t*>(field(v[i + 1])));
    }
  };
  for (int l = 0; l < c.n_layers; ++l) {
    part([l](const GreedyWS& w) { return w.kc[l]; }, max_len * D);
    part([l](const GreedyWS& w) { return w.vc[l]; }, ML4 * D);
    part([l](const GreedyWS& w) { return w.skc[l]; }, max_len * 4);
    part([l](const GreedyWS& w) { return w.svc[l]; }, max_len * 4);
    part([l](const GreedyWS& w) { return w.cross.k8[l]; }, S * D);
    part([l](const GreedyWS& w) { return w.cross.v8[l]; }, S * D);
    part([l](const GreedyWS& w) { return w.cross.sk[l]; }, S * 4);
    part([l](const GreedyWS& w) { return w.cross.sv[l]; }, S * 4);
    part([l](const GreedyWS& w) { return w.cvg[l]; }, S4 * D);
  }
  part([](const GreedyWS& w) { return w.logits; }, V * 4);
  part([](const GreedyWS& w) { return w.rec; }, (V + 15) / 16 * 16);
  part([](const GreedyWS& w) { return w.pmax_a; }, 8 * 4);
  part([](const GreedyWS& w) { return w.pmax_f; }, (size_t)(c.d_ff / 16) * 4);
  if (g.top_ids) {
    part([](const GreedyWS& w) { return w.top_ids; }, (size_t)(max_len - 1) * 2 * 8);
    part([](const GreedyWS& w) { return w.top_logp; }, (size_t)(max_len - 1) * 2 * 4);
  }
}

struct Sizes { size_t plain, scored, dfault, kvfault, score; };

// T = max_len target positions per row for the scoring (L = max_len + 1 tokens)
static Sizes sizes_of(const qtx_config& c, const Groups& gr, int B, int S, int max_len, int K, int nf) {
  return Sizes{greedy_ws(c, gr, B, S, max_len), greedy_ws(c, gr, B, S, max_len, true),
               dfault_ws(c, gr, B, S, max_len), kvfault_ws(c, gr, B, S, max_len),
               score_ws(c, B, S, max_len + 1, K, nf)};
}

static void decode_case(const qtx_config& c, const Groups& gr, int B, int S, int max_len) {
  const Sizes z = sizes_of(c, gr, B, S, max_len, 1, 0);
  CHECK(z.plain <= z.scored && z.scored <= z.kvfault && z.kvfault <= z.dfault);
  GreedyWS scored;
  {
    Block b(z.scored);
    scored = carve_greedy(b.ar, c, gr, B, S, max_len, true);
    b.spent();
    Regions r;
    add_greedy(r, scored, c, gr, B, S, max_len, true);
    r.verify(b.ar.base, z.scored);
    views_case(scored, c, gr, B, S, max_len);
    // the plain layout on the same memory: a prefix, pointer for pointer
    Arena again;
    again.base = b.ar.base; again.cap = z.plain;
    const GreedyWS plain = carve_greedy(again, c, gr, B, S, max_len);
    CHECK(again.used <= z.plain && z.plain - again.used < 256);
    same_greedy(plain, scored);
    CHECK(reinterpret_cast<uint8_t*>(scored.top_ids) >= b.ar.base + again.used);
    Regions rp;
    add_greedy(rp, plain, c, gr, B, S, max_len, false);
    rp.verify(b.ar.base, z.plain);
    views_case(plain, c, gr, B, S, max_len);
  }
  const size_t D = c.d_model, Tm = max_len > 1 ? max_len - 1 : 1;
  {
    Block b(z.dfault);
    const DfaultWS w = carve_dfault(b.ar, c, gr, B, S, max_len);
    b.spent();
    Arena again;
    again.base = b.ar.base; again.cap = z.scored;
    const GreedyWS g = carve_greedy(again, c, gr, B, S, max_len, true);
    same_greedy(g, w.g);
    CHECK(g.top_ids == w.g.top_ids && g.top_logp == w.g.top_logp && w.g.no_fold);
    Regions r;
    add_greedy(r, w.g, c, gr, B, S, max_len, true);
    add_scratch(r, w.fs, c, B * Tm);
    add_cross(r, w.fx, c, (size_t)B * S, true);
    r.add("fout", w.fout, B * Tm * D);
    r.add("flogits", w.flogits, (size_t)B * c.tgt_vocab);
    r.add("tmask", w.tmask, Tm * Tm);
    r.add("rec_ids", w.rec_ids, (size_t)B * 4);
    r.add("rec_logp", w.rec_logp, (size_t)B * 4);
    r.add("changed", w.changed, (size_t)B);
    r.add("gold_ids", w.gold_ids, (size_t)B * max_len);
    r.add("gold_top_ids", w.gold_top_ids, B * Tm * 2);
    r.add("gold_top_logp", w.gold_top_logp, B * Tm * 2);
    r.add("stamp", w.stamp, 2);
    r.verify(b.ar.base, z.dfault);
  }
  {
    Block b(z.kvfault);
    const KvfaultWS w = carve_kvfault(b.ar, c, gr, B, S, max_len);
    b.spent();
    Arena again;
    again.base = b.ar.base; again.cap = z.scored;
    const GreedyWS g = carve_greedy(again, c, gr, B, S, max_len, true);
    same_greedy(g, w.g);
    CHECK(g.top_ids == w.g.top_ids && g.top_logp == w.g.top_logp && w.g.no_fold);
    Regions r;
    add_greedy(r, w.g, c, gr, B, S, max_len, true);
    r.add("rec_ids", w.rec_ids, (size_t)B * 4);
    r.add("rec_logp", w.rec_logp, (size_t)B * 4);
    r.verify(b.ar.base, z.kvfault);
  }
  {   // the trials decode: KvfaultWS a prefix, then the table, the steps and the eager pair
    const size_t bytes = kvtrials_ws(c, gr, B, S, max_len);
    CHECK(bytes >= z.kvfault);
    Block b(bytes);
    const KvtrialsWS w = carve_kvtrials(b.ar, c, gr, B, S, max_len);
    b.spent();
    Arena again;
    again.base = b.ar.base; again.cap = z.kvfault;
    const KvfaultWS k = carve_kvfault(again, c, gr, B, S, max_len);
    same_greedy(k.g, w.k.g);
    CHECK(k.rec_ids == w.k.rec_ids && k.rec_logp == w.k.rec_logp && w.k.g.no_fold);
    Regions r;
    add_greedy(r, w.k.g, c, gr, B, S, max_len, true);
    r.add("rec_ids", w.k.rec_ids, (size_t)B * 4);
    r.add("rec_logp", w.k.rec_logp, (size_t)B * 4);
    r.add("tab", w.tab, (size_t)B * 10);
    r.add("tstep", w.tstep, (size_t)B);
    r.add("pair_ids", w.pair_ids, (size_t)B * 4);
    r.add("pair_logp", w.pair_logp, (size_t)B * 4);
    r.verify(b.ar.base, bytes);
  }
  {   // the encoder trials decode: the scored greedy decode a prefix, then the token-row table
    const size_t bytes = enctrials_ws(c, gr, B, S, max_len);
    CHECK(bytes >= z.scored);
    Block b(bytes);
    const EnctrialsWS w = carve_enctrials(b.ar, c, gr, B, S, max_len);
    b.spent();
    Arena again;
    again.base = b.ar.base; again.cap = z.scored;
    const GreedyWS g = carve_greedy(again, c, gr, B, S, max_len, true);
    same_greedy(g, w.g);
    CHECK(g.top_ids == w.g.top_ids && g.top_logp == w.g.top_logp && !w.g.no_fold);
    Regions r;
    add_greedy(r, w.g, c, gr, B, S, max_len, true);
    r.add("tab", w.tab, (size_t)B * S * 10);
    r.verify(b.ar.base, bytes);
  }
}

static void score_case(const qtx_config& c, int B, int S, int T, int K, int nf) {
  const size_t bytes = score_ws(c, B, S, T + 1, K, nf);
  Block b(bytes);
  const ScoreWS w = carve_score(b.ar, c, B, S, T + 1, K, nf);
  b.spent();
  const size_t D = c.d_model, Ms = (size_t)B * S, R = (size_t)B * K;
  Regions r;
  add_scratch(r, w.enc, c, Ms);
  add_scratch(r, w.dec, c, R * T);
  add_cross(r, w.cross, c, Ms, true);
  r.add("memory", w.memory, Ms * D);
  if (nf > 0) {
    add_cross(r, w.fcross, c, Ms, true);
    r.add("fmemory", w.fmemory, Ms * D);
  } else {
    CHECK(!w.fmemory && w.fcross.k8.empty());
  }
  if (K > 1) {
    add_cross(r, w.rcross, c, R * S, false);
    r.add("rmask", w.rmask, R * S);
  } else {
    CHECK(!w.rmask && w.rcross.k8.empty());
  }
  r.add("tmask", w.tmask, R * T * T);
  r.add("out", w.out, R * T * D);
  CHECK(w.logits_bytes >= 16 * (size_t)c.tgt_vocab * 4 && w.logits_bytes % 4 == 0);
  r.add("logits", w.logits, w.logits_bytes / 4);
  r.verify(b.ar.base, bytes);
}

// {src_vocab, tgt_vocab, n_layers, d_model, d_ff, n_heads, max_len, bits}
static qtx_config config(int F, int NL) { return qtx_config{97, 97, NL, 512, F, 8, 64, 8}; }

// The layouts' sizes in bytes.  The rows were printed (`--table`) by the carving functions as
// they stood in qtx_api.hip, moved to qtx_carve.h unchanged (only the sub-batch split became a
// parameter), before any later edit of them: a change of these numbers is a change of every
// caller's workspace.
struct Pin { int F, NL, B, G, S, max_len, K, nf; Sizes z; };
static const Pin kPins[] = {
    {256, 1, 1, 1, 1, 1, 1, 0, {46336, 46336, 71424, 46848, 45568}},
    {256, 1, 1, 1, 5, 2, 2, 1, {129792, 130304, 177920, 130816, 219904}},
    {256, 2, 3, 1, 5, 6, 1, 0, {438528, 439040, 763392, 439552, 598272}},
    {256, 2, 3, 2, 8, 6, 2, 0, {657152, 657664, 1042176, 658176, 1158400}},
    {2048, 1, 1, 1, 1, 1, 1, 1, {64000, 64000, 97792, 64512, 71168}},
    {2048, 1, 1, 1, 8, 2, 1, 0, {245760, 246272, 319488, 246784, 262144}},
    {2048, 1, 3, 2, 5, 6, 2, 1, {534784, 535296, 928512, 535808, 1280512}},
    {2048, 2, 1, 1, 5, 6, 2, 0, {189952, 190464, 331776, 190976, 411136}},
    {2048, 2, 3, 1, 1, 2, 1, 1, {186880, 187392, 276224, 187904, 243712}},
    {2048, 2, 3, 2, 5, 6, 1, 0, {584448, 584960, 993536, 585472, 782848}},
    {2048, 2, 3, 2, 8, 1, 2, 1, {796928, 796928, 1025792, 797440, 1085952}},
    {2048, 2, 3, 2, 8, 6, 2, 1, {824576, 825088, 1293824, 825600, 1698048}},
};

int main(int argc, char** argv) {
  const bool table = argc > 1 && !std::strcmp(argv[1], "--table");
  if (table) {
    const int rows[][8] = {{256, 1, 1, 1, 1, 1, 1, 0},  {256, 1, 1, 1, 5, 2, 2, 1},
                           {256, 2, 3, 1, 5, 6, 1, 0},  {256, 2, 3, 2, 8, 6, 2, 0},
                           {2048, 1, 1, 1, 1, 1, 1, 1}, {2048, 1, 1, 1, 8, 2, 1, 0},
                           {2048, 1, 3, 2, 5, 6, 2, 1}, {2048, 2, 1, 1, 5, 6, 2, 0},
                           {2048, 2, 3, 1, 1, 2, 1, 1}, {2048, 2, 3, 2, 5, 6, 1, 0},
                           {2048, 2, 3, 2, 8, 1, 2, 1}, {2048, 2, 3, 2, 8, 6, 2, 1}};
    for (const auto& p : rows) {
      const Sizes z = sizes_of(config(p[0], p[1]), split_groups(p[2], p[3]), p[2], p[4], p[5], p[6], p[7]);
      std::printf("    {%d, %d, %d, %d, %d, %d, %d, %d, {%zu, %zu, %zu, %zu, %zu}},\n", p[0], p[1], p[2],
                  p[3], p[4], p[5], p[6], p[7], z.plain, z.scored, z.dfault, z.kvfault, z.score);
    }
    return 0;
  }
  CHECK(split_groups(3, 2).G == 2 && split_groups(3, 2).Bg == 2 && split_groups(3, 2).rows(1, 3) == 1);
  CHECK(split_groups(1, 2).G == 1 && split_groups(5, 4).G == 3 && split_groups(8, 9).G == QTX_MAX_GROUPS);
  for (int F : {256, 2048})
    for (int NL : {1, 2}) {
      const qtx_config c = config(F, NL);
      for (int B : {1, 3})
        for (int S : {1, 5, 8})
          for (int max_len : {1, 2, 6}) {
            for (int G = 1; G <= (B > 1 ? 2 : 1); ++G)
              decode_case(c, split_groups(B, G), B, S, max_len);
            for (int K : {1, 2})
              for (int nf : {0, 1}) score_case(c, B, S, max_len, K, nf);
          }
    }
  for (const Pin& p : kPins) {
    const Sizes z = sizes_of(config(p.F, p.NL), split_groups(p.B, p.G), p.B, p.S, p.max_len, p.K, p.nf);
    CHECK(z.plain == p.z.plain && z.scored == p.z.scored && z.dfault == p.z.dfault);
    CHECK(z.kvfault == p.z.kvfault && z.score == p.z.score);
  }
  CHECK(sizeof(kPins) / sizeof(kPins[0]) == 12);
  std::puts("carve host checks ok");
  return 0;
}
