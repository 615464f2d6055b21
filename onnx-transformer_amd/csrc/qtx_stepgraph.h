// qtx_stepgraph.h — the step-graph runner: what turns "run these decode steps" into hipGraph
// captures and replays for every driver of the KV-cached step (greedy, decoder-fault and beam
// decodes: qtx_api.hip, qtx_fault.hip, qtx_search.hip).  A driver hands over a typed key, a step callback and a plan; the
// runner owns the sub-batch streams, the fork / join events and the cache of captured graphs.
// Host code only.  The caller serialises run() per model (qtx_model::mu) with the model's
// device current.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <functional>
#include <map>
#include <tuple>
#include <vector>

#include "../../include/qtx.h"
#include "qtx_carve.h"   // QTX_MAX_GROUPS
#include "qtx_knobs.h"

namespace qtx {

// Records a failed HIP call as the thread's last error and returns QTX_E_HIP (qtx_model.hip).
int stepgraph_hip_error(const char* what, hipError_t e);

#define SG_HIP(expr)                                                       \
  do {                                                                     \
    const hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) return ::qtx::stepgraph_hip_error(#expr, e_);    \
  } while (0)

// Which driver's step a graph holds: each bakes other launches or other buffers into it.
enum class StepForm { Plain, Scored, Dfault, DfaultScored, Beam };

// What a captured graph depends on.  The caller's ids and src_mask are staged through
// workspace buffers around each replay, so the shapes, the workspace (anchor) and the
// switches identify it: callers that allocate fresh id / mask tensors still hit the cache.
struct StepGraphKey {
  int rows = 0, S = 0, max_len = 0;
  int groups = 1;                   // sub-batch groups
  int per = 0;                      // steps per graph (filled in from the plan's segment)
  const void* anchor = nullptr;     // the step counters baked into the capture
  StepForm form = StepForm::Plain;
  bool host_pos = false;            // captured at host positions, else at the device counter
  bool joint = false;               // the groups as branches of ONE graph (QTX_GROUP_GRAPH)
  int beam_k = 0, eos = 0, pad = 0; // beam only
  int knobs_gen = 0;                // knobs_generation(): every switch a captured step reads
  auto tie() const {
    return std::tie(rows, S, max_len, groups, per, anchor, form, host_pos, joint, beam_k, eos, pad,
                    knobs_gen);
  }
  bool operator<(const StepGraphKey& o) const { return tie() < o.tie(); }
};

// `replays` graphs of `per` steps each; t0: the host position of the segment's first step,
// -1 where the host does not know it (the step then reads the device counter).
struct StepSegment { int per, replays, t0; };

struct StepRequest {
  StepGraphKey key;   // all but per and knobs_gen
  // one step of group i enqueued on the stream, at host position t (-1: the device counter's)
  std::function<int(int i, hipStream_t, int t)> step;
  std::vector<StepSegment> plan;
  bool timed = false;   // QTX_TIME_GRAPH: the replays of group 0 timed to stderr
};

class StepGraphs {
 public:
  static constexpr size_t kMaxEntries = 16;

  // Runs the plan on st: eager launches under QTX_NO_GRAPH, else replays of cached graphs,
  // capturing the missing ones first.
  int run(const StepRequest& rq, hipStream_t st) {
    const int G = rq.key.groups;
    if (!ev_in_) SG_HIP(hipEventCreateWithFlags(&ev_in_, hipEventDisableTiming));
    for (int i = 0; i < G; ++i)
      if (!gstream_[i]) {
        SG_HIP(hipStreamCreateWithFlags(&gstream_[i], hipStreamNonBlocking));
        SG_HIP(hipEventCreateWithFlags(&ev_out_[i], hipEventDisableTiming));
      }
    const bool eager = knobs().no_graph;
    std::vector<Entry*> ent;
    if (const int rc = eager ? QTX_OK : resolve(rq, ent)) return rc;
    // One sub-batch (or one joint graph): on the caller's stream itself (a graph captured on
    // one stream can be launched on any).  Several: fork to the model's streams, join back.
    const bool fork = G > 1 && (eager || !rq.key.joint);
    hipStream_t ls[QTX_MAX_GROUPS];
    for (int i = 0; i < G; ++i) ls[i] = fork ? gstream_[i] : st;
    if (fork) {
      SG_HIP(hipEventRecord(ev_in_, st));
      for (int i = 0; i < G; ++i) SG_HIP(hipStreamWaitEvent(ls[i], ev_in_, 0));
    }
    hipEvent_t tg0 = nullptr, tg1 = nullptr;
    if (rq.timed && !eager) {
      SG_HIP(hipEventCreate(&tg0));
      SG_HIP(hipEventCreate(&tg1));
      SG_HIP(hipEventRecord(tg0, ls[0]));
    }
    int steps = 0;
    for (size_t k = 0; k < rq.plan.size(); ++k) {
      const StepSegment& sg = rq.plan[k];
      for (int r = 0; r < sg.replays; ++r) {
        if (eager) {
          for (int t = 0; t < sg.per; ++t)
            for (int i = 0; i < G; ++i)
              if (const int rc = rq.step(i, ls[i], sg.t0 < 0 ? -1 : sg.t0 + r * sg.per + t)) return rc;
        } else {
          const std::vector<hipGraphExec_t>& ex = ent[k]->execs;
          for (size_t i = 0; i < ex.size(); ++i) SG_HIP(hipGraphLaunch(ex[i], ls[i]));
        }
      }
      steps += sg.per * sg.replays;
    }
    if (tg0) {
      float ms = 0.0f;
      SG_HIP(hipEventRecord(tg1, ls[0]));
      SG_HIP(hipEventSynchronize(tg1));
      SG_HIP(hipEventElapsedTime(&ms, tg0, tg1));
      fprintf(stderr, "qtx: decode graphs %.3f ms (%d steps, group 0)\n", ms, steps);
      (void)hipEventDestroy(tg0);
      (void)hipEventDestroy(tg1);
    }
    if (fork)
      for (int i = 0; i < G; ++i) {
        SG_HIP(hipEventRecord(ev_out_[i], ls[i]));
        SG_HIP(hipStreamWaitEvent(st, ev_out_[i], 0));
      }
    // completion markers of the entries' replays (after the join: every sub-batch)
    for (Entry* e : ent) {
      if (!e->done) SG_HIP(hipEventCreateWithFlags(&e->done, hipEventDisableTiming));
      SG_HIP(hipEventRecord(e->done, st));
    }
    return QTX_OK;
  }

  // an exec may still be running on a caller's stream: wait for its last replay first
  void clear() {
    for (auto& kv : graphs_) {
      if (kv.second.done) {
        (void)hipEventSynchronize(kv.second.done);
        (void)hipEventDestroy(kv.second.done);
      }
      for (hipGraphExec_t e : kv.second.execs) (void)hipGraphExecDestroy(e);
    }
    graphs_.clear();
  }

  void destroy() {
    for (hipStream_t s : gstream_)
      if (s) (void)hipStreamSynchronize(s);
    clear();
    if (ev_in_) (void)hipEventDestroy(ev_in_);
    for (int i = 0; i < QTX_MAX_GROUPS; ++i) {
      if (ev_out_[i]) (void)hipEventDestroy(ev_out_[i]);
      if (gstream_[i]) (void)hipStreamDestroy(gstream_[i]);
    }
  }

  size_t entries() const { return graphs_.size(); }
  long long captures() const { return captures_; }   // graphs instantiated so far, one per exec

 private:
  struct Entry {
    std::vector<hipGraphExec_t> execs;   // one graph per sub-batch, or the one joint graph
    hipEvent_t done = nullptr;           // recorded after the entry's last replay
  };

  // The plan's entries, one per segment.  The plan is resolved as a set: when a missing graph
  // would not fit under the cap, the cache is cleared once, before anything is captured, so
  // no capture of this call evicts an entry the call replays.
  int resolve(const StepRequest& rq, std::vector<Entry*>& ent) {
    std::vector<StepGraphKey> keys;
    size_t missing = 0;
    for (const StepSegment& sg : rq.plan) {
      StepGraphKey k = rq.key;
      k.per = sg.per;
      k.knobs_gen = knobs_generation();
      bool seen = graphs_.count(k) != 0;
      for (const StepGraphKey& o : keys) seen = seen || o.tie() == k.tie();
      missing += seen ? 0 : 1;
      keys.push_back(k);
    }
    if (missing && graphs_.size() + missing > kMaxEntries) clear();
    for (size_t k = 0; k < keys.size(); ++k) {
      auto it = graphs_.find(keys[k]);
      if (it == graphs_.end()) {
        const int G = rq.key.groups;
        Entry e;
        int rc = rq.key.joint ? capture(rq, rq.plan[k], 0, G, e.execs) : QTX_OK;
        for (int i = 0; i < G && !rq.key.joint && rc == QTX_OK; ++i)
          rc = capture(rq, rq.plan[k], i, i + 1, e.execs);
        if (rc != QTX_OK) {
          for (hipGraphExec_t x : e.execs) (void)hipGraphExecDestroy(x);
          return rc;
        }
        it = graphs_.emplace(keys[k], std::move(e)).first;
      }
      ent.push_back(&it->second);
    }
    return QTX_OK;
  }

  // One graph of the segment's steps for groups i0 .. i1-1, captured on group i0's stream.
  // The separate form captures one group per graph; the joint form (QTX_GROUP_GRAPH,
  // diagnostic build) all groups as independent branches of one graph, forked and joined
  // inside the capture.  The capture is always ended and the graph destroyed; the step's own
  // status wins over the HIP error of a capture it broke.
  int capture(const StepRequest& rq, const StepSegment& sg, int i0, int i1,
              std::vector<hipGraphExec_t>& execs) {
    hipStream_t s0 = gstream_[i0];
    SG_HIP(hipStreamBeginCapture(s0, hipStreamCaptureModeThreadLocal));
    int rc = QTX_OK;
    hipError_t e = i1 - i0 > 1 ? hipEventRecord(ev_in_, s0) : hipSuccess;
    for (int i = i0 + 1; i < i1 && e == hipSuccess; ++i) e = hipStreamWaitEvent(gstream_[i], ev_in_, 0);
    for (int t = 0; t < sg.per && rc == QTX_OK && e == hipSuccess; ++t)
      for (int i = i0; i < i1 && rc == QTX_OK; ++i)
        rc = rq.step(i, gstream_[i], rq.key.host_pos ? sg.t0 + t : -1);
    for (int i = i0 + 1; i < i1 && e == hipSuccess; ++i) {   // (after a failed step too)
      e = hipEventRecord(ev_out_[i], gstream_[i]);
      if (e == hipSuccess) e = hipStreamWaitEvent(s0, ev_out_[i], 0);
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const hipError_t e_end = hipStreamEndCapture(s0, &graph);
    if (e == hipSuccess) e = e_end;
    if (rc == QTX_OK && e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc != QTX_OK) return rc;
    SG_HIP(e);
    execs.push_back(exec);
    ++captures_;
    return QTX_OK;
  }

  hipStream_t gstream_[QTX_MAX_GROUPS] = {};
  hipEvent_t ev_in_ = nullptr, ev_out_[QTX_MAX_GROUPS] = {};
  std::map<StepGraphKey, Entry> graphs_;
  long long captures_ = 0;
};

#undef SG_HIP

}  // namespace qtx
