// DQN / SQN learner hot loop: `batch = replay_buffer.sample_batch(B); agent.train(batch, cnt)` (algos/dqn/train.py:66-76 on
// algos/dqn/actor_learner.py:110-119; algos/sqn likewise), n iterations per call with no host work per update — the discrete
// counterpart of loop.hip.  Every cursor, the ring's MT19937 state and the optimizer state live on the device, so the sequence is
// captured ONCE into a family of hipGraphs (loop_family.h: `updates_per_graph` and every power of two below it, variants by
// pre-sampled / starting input set / tail-sampling) and replayed; a call consumes its updates greedily, so after the capture no
// update runs eagerly.  An update here is ddrl_dqn_step's launches WITHOUT the staging one: the sampler writes the padded images
// of one of the learner's two input sets directly, and consecutive updates alternate between the sets, so the sampler of update
// u + 1 never overwrites what update u still reads — it rides as one more workgroup of update u's head launch (dqn.hip:
// k_dqn_head_sample).  Only a call's first update opens with a stand-alone sampler launch and only its last one draws nothing (the
// caller may store into the ring before the next call): no store can fall inside a call, so the result equals the sequential
// sample -> update order, bit for bit (tests/test_gpu_dqn_loop.py).  One branch only: no fork modes, no side streams.
// A captured update is 6 kernel nodes (7 eager launches minus the staging one); a head-sampled graph of n updates 6 n + 1, plus a
// copy node of the optimizer state where n is odd.
#include "ddrl_common.h"
#include "loop_family.h"

// internal (dqn.hip)
int ddrl_dqn_internal_loop_check(ddrl_dqn_t *h, ddrl_replay_t *replay);   // the loop's envelope; changes nothing
int ddrl_dqn_internal_sample_into(ddrl_dqn_t *h, ddrl_replay_t *replay, int set, bool rows, void *stream);   // stand-alone sampler launch into input set `set`
int ddrl_dqn_internal_update(ddrl_dqn_t *h, int set, ddrl_replay_t *ride, float *loss_d, void *stream);     // one update on `set`; ride: + the draw into the other set
int ddrl_dqn_internal_opt_sync(ddrl_dqn_t *h, void *stream);              // put the double-buffered optimizer state on copy 0
void ddrl_dqn_internal_note_updates(ddrl_dqn_t *h, long long n);        // host flags after n replayed updates (the acting forward repacks)
// internal (replay.hip)
bool ddrl_replay_internal_has_feed(ddrl_replay_t *h);

struct ddrl_dqn_loop {
    ddrl_dqn_t *learner;
    ddrl_replay_t *replay;
    int per_graph;
    float *loss_d;
    std::vector<ddrl_family::Graph> family;
    bool captured;
    int parity;            // input set of the next eager update
    int nodes[2];          // kernel / other nodes of the full-length, head-sampled, non-tail graph
};

static int one_update(ddrl_dqn_loop *h, void *stream) {
    const int set = h->parity;
    h->parity ^= 1;
    int rc = ddrl_dqn_internal_sample_into(h->learner, h->replay, set, true, stream);   // (an empty ring surfaces here)
    if (rc != DDRL_OK) return rc;
    return ddrl_dqn_internal_update(h->learner, set, nullptr, h->loss_d, stream);
}

// Capture `n` updates as variant (pre, start, tail) of ddrl_family::Graph.  counts != nullptr: its kernel / other node counts
static int capture(ddrl_dqn_loop *h, hipStream_t cs, int n, int pre, int start, int tail, hipGraphExec_t *exec, int *counts) {
    hipGraph_t graph = nullptr;
    int rc = ddrl_dqn_internal_opt_sync(h->learner, (void *)cs);   // the graph starts on copy 0 of the optimizer state ...
    if (rc != DDRL_OK) return rc;
    DDRL_HIP_CHECK(hipStreamSynchronize(cs));   // one-time: the capture stream may not be the caller's
    DDRL_HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    // sample(0) as a kernel (head-sampled) or drawn by the replay before (pre-sampled); sample(i + 1) rides inside update i, the last
    // update's only in a tail-sampling graph
    if (!pre) rc = ddrl_dqn_internal_sample_into(h->learner, h->replay, start, false, (void *)cs);
    for (int i = 0; i < n && rc == DDRL_OK; ++i)
        rc = ddrl_dqn_internal_update(h->learner, (start + i) & 1, (i + 1 < n || tail) ? h->replay : nullptr, h->loss_d, (void *)cs);
    if (rc == DDRL_OK) rc = ddrl_dqn_internal_opt_sync(h->learner, (void *)cs);   // ... and ends on it (a copy node when n is odd)
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

// The whole family, or nothing: a failure destroys the graphs already built
static int capture_family(ddrl_dqn_loop *h, hipStream_t cs) {
    h->family = ddrl_family::lengths(h->per_graph);
    for (auto &g : h->family)
        for (int v = 0; v < 8; ++v) {
            const int pre = v >> 2, start = (v >> 1) & 1, tail = v & 1;
            if (!ddrl_family::variant_needed(true, h->per_graph, g.len, pre, start, tail)) continue;
            const bool full_head = g.len == h->per_graph && v == 0;
            const int rc = capture(h, cs, g.len, pre, start, tail, &g.exec[pre][start][tail], full_head ? h->nodes : nullptr);
            if (rc != DDRL_OK) { ddrl_family::destroy(h->family); return rc; }
        }
    h->captured = true;
    return DDRL_OK;
}

extern "C" {

int ddrl_dqn_loop_create(ddrl_dqn_loop_t **out, ddrl_dqn_t *learner, ddrl_replay_t *replay, int32_t updates_per_graph, float *loss_d) {
    DDRL_REQUIRE(out && learner && replay, "NULL pointer");
    DDRL_REQUIRE(updates_per_graph >= 0 && updates_per_graph <= 4096, "updates_per_graph must be in [0, 4096]");
    const int rc = ddrl_dqn_internal_loop_check(learner, replay);
    if (rc != DDRL_OK) return rc;
    ddrl_dqn_loop *h = new ddrl_dqn_loop();
    h->learner = learner; h->replay = replay; h->per_graph = updates_per_graph; h->loss_d = loss_d;
    h->captured = false; h->parity = 0; h->nodes[0] = h->nodes[1] = 0;
    *out = h;
    return DDRL_OK;
}

int ddrl_dqn_loop_destroy(ddrl_dqn_loop_t *h) {
    if (!h) return DDRL_OK;
    ddrl_family::destroy(h->family);
    delete h;
    return DDRL_OK;
}

int ddrl_dqn_loop_info(ddrl_dqn_loop_t *h, int32_t *info_h) {
    DDRL_REQUIRE(h != nullptr && info_h != nullptr, "NULL pointer");
    info_h[0] = h->per_graph; info_h[1] = h->captured ? 1 : 0; info_h[2] = h->nodes[0]; info_h[3] = h->nodes[1];
    return DDRL_OK;
}

int ddrl_dqn_loop_run(ddrl_dqn_loop_t *h, int64_t n_updates, void *stream) {
    DDRL_REQUIRE(h != nullptr && n_updates >= 0, "bad handle / n_updates");
    if (ddrl_replay_internal_has_feed(h->replay)) {
        ddrl::set_error("ddrl_dqn_loop_run: the ring has a feed plan attached (ddrl_replay_set_feed): the DQN / SQN loop's sampler does not follow one");
        return DDRL_ERR_UNSUPPORTED;
    }
    hipStream_t s = ddrl::as_stream(stream);
    int64_t left = n_updates;
    if (h->per_graph > 0 && (h->captured || left >= h->per_graph)) {   // (the first call of at least per_graph updates captures)
        if (!h->captured) {
            // one eager update first: surfaces EMPTY_BUFFER / argument errors outside the capture
            int rc = one_update(h, stream);
            if (rc != DDRL_OK) return rc;
            left -= 1;
            hipStream_t cs = s, own = nullptr;
            if (cs == nullptr) {  // the legacy null stream cannot be captured
                DDRL_HIP_CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
                DDRL_HIP_CHECK(hipDeviceSynchronize());
                cs = own;
            }
            rc = capture_family(h, cs);
            if (own) (void)hipStreamDestroy(own);
            if (rc != DDRL_OK) return rc;
        }
        if (left > 0) {  // eager updates since the last replay (this handle's, or ddrl_dqn_step's) may have left the optimizer state on copy 1
            const int rc2 = ddrl_dqn_internal_opt_sync(h->learner, stream);
            if (rc2 != DDRL_OK) return rc2;
        }
        const int64_t before = left;
        const int rc3 = ddrl_family::replay(h->family, true, left, s);   // greedy, head-sampled first, tail-sampling all but the last
        ddrl_dqn_internal_note_updates(h->learner, before - left);
        if (rc3 != DDRL_OK) return rc3;
    }
    for (; left > 0; --left) {
        const int rc = one_update(h, stream);
        if (rc != DDRL_OK) return rc;
    }
    return DDRL_OK;
}

}  // extern "C"
