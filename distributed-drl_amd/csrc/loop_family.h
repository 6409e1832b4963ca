// The captured learner loops (loop.hip: SAC1 on ddrl_loop_*; dqn_loop.hip: Double-DQN / SQN on ddrl_dqn_loop_*), written once
// over the learner's four operations: the capture bracket, the linear body of a graph, the family of graphs and the driver of
// a call.  What is captured and in which order a call consumes it is decided in loop_plan.h.  Internal to libddrl_hip.so — not
// part of the C-ABI.
#pragma once
#include "ddrl_common.h"
#include "loop_plan.h"

#include <cstdint>
#include <vector>

namespace ddrl_family {

// What a learner supplies; `ctx` is its loop handle.
struct Ops {
    void *ctx;
    int (*sample_into)(void *ctx, int set, bool eager, void *stream);     // stand-alone sampler launch into input set `set`
    int (*update)(void *ctx, int set, bool draw_next, void *stream);      // one update on `set`; draw_next: + the draw into the other set
    int (*opt_sync)(void *ctx, void *stream);                             // put the double-buffered optimizer state on copy 0
    void (*note_replayed)(void *ctx, int64_t n);                          // host bookkeeping after n replayed updates; may be nullptr
};

// One captured length and its variants exec[pre][start][tail] (loop_plan.h); unreachable variants stay nullptr
struct Graph { int len; hipGraphExec_t exec[2][2][2]; };

struct Loop {
    int per_graph = 0;
    std::vector<Graph> family;   // ddrl_plan::lengths(per_graph), in that order
    bool captured = false;
    int parity = 0;              // input set of the next eager update: they keep alternating among themselves
    int nodes[2] = {0, 0};       // kernel / other nodes of the full-length, head-sampled, non-tail graph
};

// `n` updates in a row: sample(start) as a kernel (head-sampled) or drawn by the replay before (pre-sampled); sample(i + 1) rides
// inside update i, the last update's only in a tail-sampling graph.  No store can interleave inside one graph, nor between two
// replays of one call, so this equals the sequential sample -> update order.
static inline int linear_body(const Ops &ops, int n, int pre, int start, int tail, bool eager, void *stream) {
    int rc = pre ? DDRL_OK : ops.sample_into(ops.ctx, start, eager, stream);
    for (int i = 0; i < n && rc == DDRL_OK; ++i) rc = ops.update(ops.ctx, (start + i) & 1, i + 1 < n || tail, stream);
    return rc;
}

// One eager update: a head-sampled body of one on the next input set, its draw asking the ring as an eager call does
static inline int one_update(const Ops &ops, Loop &st, void *stream) {
    st.parity ^= 1;
    return linear_body(ops, 1, 0, st.parity ^ 1, 0, true, stream);
}

// Capture linear_body(n, pre, start, tail) on `cs` and instantiate it.  counts != nullptr: its kernel / other node counts
static inline int capture(const Ops &ops, hipStream_t cs, int n, int pre, int start, int tail, hipGraphExec_t *exec, int *counts) {
    hipGraph_t graph = nullptr;
    int rc = ops.opt_sync(ops.ctx, (void *)cs);   // the graph starts on copy 0 of the optimizer state ...
    if (rc != DDRL_OK) return rc;
    DDRL_HIP_CHECK(hipStreamSynchronize(cs));   // one-time: the capture stream may not be the caller's
    DDRL_HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    rc = linear_body(ops, n, pre, start, tail, false, (void *)cs);
    if (rc == DDRL_OK) rc = ops.opt_sync(ops.ctx, (void *)cs);   // ... and ends on it (a copy node when n is odd)
    const hipError_t e2 = hipStreamEndCapture(cs, &graph);
    if (rc != DDRL_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e2 != hipSuccess) {
        ddrl::set_error("graph capture failed: %s", hipGetErrorString(e2));
        if (graph) (void)hipGraphDestroy(graph);
        return DDRL_ERR_HIP;
    }
    if (counts) {
        size_t nn = 0;
        hipError_t e = hipGraphGetNodes(graph, nullptr, &nn);
        std::vector<hipGraphNode_t> nodes(nn);
        if (e == hipSuccess && nn) e = hipGraphGetNodes(graph, nodes.data(), &nn);
        counts[0] = counts[1] = 0;
        for (size_t i = 0; i < nn && e == hipSuccess; ++i) {
            hipGraphNodeType t;
            e = hipGraphNodeGetType(nodes[i], &t);
            if (e == hipSuccess) ++counts[t == hipGraphNodeTypeKernel ? 0 : 1];
        }
        if (e != hipSuccess) {
            ddrl::set_error("reading the captured graph's nodes failed: %s", hipGetErrorString(e));
            (void)hipGraphDestroy(graph);
            return DDRL_ERR_HIP;
        }
    }
    const hipError_t e3 = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e3 != hipSuccess) {
        *exec = nullptr;
        ddrl::set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e3));
        return DDRL_ERR_HIP;
    }
    return DDRL_OK;
}

static inline void destroy(Loop &st) {
    for (auto &g : st.family)
        for (int v = 0; v < 8; ++v)
            if (g.exec[v >> 2][(v >> 1) & 1][v & 1]) (void)hipGraphExecDestroy(g.exec[v >> 2][(v >> 1) & 1][v & 1]);
    st.family.clear();
    st.captured = false;
}

// The whole family, or nothing: a failure destroys the graphs already built.
// COST: the lengths sum to < 3 x per_graph and each has up to 4 variants (8 where per_graph is odd), so the one-time capture holds
// up to 12 x per_graph updates (24 x where odd) of five (SAC1) or six (DQN / SQN) kernel nodes each, against per_graph with a
// single graph: 450 SAC1 updates in 26 graphs at 50, where the first capturing call takes what it took with the single graph
// (26.5 ms).  It grows linearly: ~33 000 updates / ~164 000 nodes at the accepted maximum of 4096, a size nothing here runs at.
static inline int capture_family(const Ops &ops, Loop &st, hipStream_t cs) {
    for (int len : ddrl_plan::lengths(st.per_graph)) st.family.push_back(Graph{len, {}});
    for (auto &g : st.family)
        for (int v = 0; v < 8; ++v) {
            const int pre = v >> 2, start = (v >> 1) & 1, tail = v & 1;
            if (!ddrl_plan::variant_needed(st.per_graph, g.len, pre, start, tail)) continue;
            const bool full_head = g.len == st.per_graph && v == 0;
            const int rc = capture(ops, cs, g.len, pre, start, tail, &g.exec[pre][start][tail], full_head ? st.nodes : nullptr);
            if (rc != DDRL_OK) { destroy(st); return rc; }
        }
    st.captured = true;
    return DDRL_OK;
}

// Launch what ddrl_plan::plan lays out for `left` updates; `left` goes down by what was launched, also when a launch fails
static inline int replay(const Loop &st, int64_t &left, hipStream_t s) {
    for (const ddrl_plan::Step &p : ddrl_plan::plan(st.per_graph, left)) {
        const Graph &g = st.family[p.index];
        hipGraphExec_t exec = g.exec[p.pre][p.start][p.tail];
        DDRL_REQUIRE(exec != nullptr, "no captured graph for this replay (internal)");
        DDRL_HIP_CHECK(hipGraphLaunch(exec, s));
        left -= g.len;
    }
    return DDRL_OK;
}

// n_updates sample + update iterations on `stream`.  The first call of at least per_graph updates captures the family; from then
// on every update of a call runs from a graph.  per_graph == 0, and shorter calls before the capture, run eagerly.
static inline int run(const Ops &ops, Loop &st, int64_t n_updates, void *stream) {
    hipStream_t s = ddrl::as_stream(stream);
    int64_t left = n_updates;
    if (st.per_graph > 0 && (st.captured || left >= st.per_graph)) {
        if (!st.captured) {
            // one eager update first: surfaces EMPTY_BUFFER / argument errors outside the capture
            int rc = one_update(ops, st, stream);
            if (rc != DDRL_OK) return rc;
            left -= 1;
            hipStream_t cs = s, own = nullptr;
            if (cs == nullptr) {  // the legacy null stream cannot be captured
                DDRL_HIP_CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
                DDRL_HIP_CHECK(hipDeviceSynchronize());
                cs = own;
            }
            rc = capture_family(ops, st, cs);
            if (own) (void)hipStreamDestroy(own);
            if (rc != DDRL_OK) return rc;
        }
        if (left > 0) {  // eager updates since the last replay (this handle's, or the learner's own step) may have left the optimizer state on copy 1
            const int rc2 = ops.opt_sync(ops.ctx, stream);
            if (rc2 != DDRL_OK) return rc2;
        }
        const int64_t before = left;
        const int rc3 = replay(st, left, s);   // greedy, head-sampled first, tail-sampling all but the last
        if (ops.note_replayed) ops.note_replayed(ops.ctx, before - left);
        if (rc3 != DDRL_OK) return rc3;
    }
    for (; left > 0; --left) {
        const int rc = one_update(ops, st, stream);
        if (rc != DDRL_OK) return rc;
    }
    return DDRL_OK;
}

}  // namespace ddrl_family
