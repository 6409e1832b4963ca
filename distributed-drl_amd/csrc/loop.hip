// Learner hot loop: `while True: batch = replay_buffer.sample_batch(B); agent.train(batch)`
// (algos/sac1/sac1.py:146-148; example/dsac.py:142-144 with example/model.py:92-101), n iterations
// per call with no host work per update.  Built on the public C-ABI only: the replay gathers
// straight into one of the learner's two input sets, the noise comes from the learner's device
// counter, and because every cursor / RNG state / optimizer state lives on the device the
// sequence of updates is captured ONCE into hipGraphs and replayed (an eager launch stream would
// be host-bound at ~3.5 us per kernel, MI355X guide "graph-replay-floor").
// A FAMILY of lengths is captured — `updates_per_graph` and every power of two below it — and a
// call consumes its updates greedily: full-size replays, then the binary decomposition of the
// rest, so after the capture no update runs eagerly (a caller that cuts its updates at every push
// leaves a different remainder each call).  Consecutive updates alternate between the learner's
// two input sets, so the sampler of update u+1 never overwrites what update u still reads: it
// rides in update u's forward launch, and that chain carries on ACROSS the replays of one call —
// only a call's first replay opens with a stand-alone sampler launch, and only its last one ends
// without a draw (the caller may store into the ring before the next call).  bench.py at N = 1:
// 92.30 -> 91.38 ms per 2048-update step (profiles/loop_graph_family_before_after.txt).  Optionally
// (DDRL_LOOP_FORK) the sampler runs on a forked graph branch of the full-size graph and overlaps
// the previous update — the job of the reference's `Cache` prefetch process
// (algos/sac1/sac1.py:103-130).
#include "ddrl_common.h"
#include "loop_family.h"

#include <cstdlib>
#include <cstring>
#include <vector>

// internal (sac1.hip): put the learner's double-buffered optimizer state on copy 0
int ddrl_sac1_internal_opt_sync(ddrl_sac1_t *h, void *stream);
// internal (sac1.hip): sample_batch into input set `set` of the learner — ddrl_replay_sample for a transition ring, ddrl_replay_sample_nstep
// with the learner's gamma for an n-step window ring (algos/sac1/sac_ray.py:40-51)
int ddrl_sac1_internal_sample_into(ddrl_sac1_t *h, ddrl_replay_t *replay, int set, void *stream);

struct ddrl_loop {
    ddrl_sac1_t *learner;
    ddrl_replay_t *replay;
    int per_graph;
    uint32_t seed;
    float *buf[2][8];
    int batch;
    using Graph = ddrl_family::Graph;   // one captured length and its variants exec[pre][start][tail] (loop_family.h); eager updates keep
                                        // alternating on `parity` among themselves
    std::vector<Graph> family;  // per_graph, then the powers of two below it, descending
    bool chain;                 // the sampler chain runs across replays (off under DDRL_LOOP_FORK: every replay head-sampled, no tail draw)
    bool captured;
    int parity;  // input set of the next eager update
};

static int sample_into(ddrl_loop *h, int set, void *stream) {
    return ddrl_sac1_internal_sample_into(h->learner, h->replay, set, stream);   // (h->buf[set] is the learner's input set `set`)
}

static int update_from(ddrl_loop *h, int set, void *stream) {
    float **b = h->buf[set];
    int rc = ddrl_sac1_fill_noise(h->learner, h->seed, stream);  // arms in-kernel noise generation
    if (rc != DDRL_OK) return rc;
    return ddrl_sac1_step(h->learner, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
}

static int one_update(ddrl_loop *h, void *stream) {
    const int set = h->parity;
    h->parity ^= 1;
    int rc = sample_into(h, set, stream);
    if (rc != DDRL_OK) return rc;
    return update_from(h, set, stream);
}

static int grads_from(ddrl_loop *h, int set, void *stream) {
    float **b = h->buf[set];
    int rc = ddrl_sac1_fill_noise(h->learner, h->seed, stream);
    if (rc != DDRL_OK) return rc;
    return ddrl_sac1_compute_grads(h->learner, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr,
                                   stream);
}

static int fork_mode() {
    const char *fk = getenv("DDRL_LOOP_FORK");
    return !fk ? 0 : (strcmp(fk, "all") == 0 ? 2 : 1);
}

static bool variant_needed(const ddrl_loop *h, int len, int pre, int start, int tail) {
    return ddrl_family::variant_needed(h->chain, h->per_graph, len, pre, start, tail);
}

static void destroy_family(ddrl_loop *h) {
    ddrl_family::destroy(h->family);
    h->captured = false;
}

// Capture `n` updates as variant (pre, start, tail) of ddrl_loop::Graph.  mode 0: one branch; the sampler of update u+1 rides
// inside update u (ddrl_sac1_step_and_sample: an extra workgroup of a forward launch on the fused path, of the Adam
// kernel otherwise).
// Experimental overlap modes (bit-identical results, both measured SLOWER on MI355X — a kernel
// starting or ending on another branch costs the kernel running beside it more than it hides):
//   DDRL_LOOP_FORK=adam  sampler of update u+1 beside the Adam/polyak kernel of update u (105 us)
//   DDRL_LOOP_FORK=all   sampler of update u+1 anywhere beside update u (99 us)
static int capture(ddrl_loop *h, hipStream_t main_s, int n, int mode, int pre, int start, int tail, hipGraphExec_t *exec) {
    hipStream_t side = nullptr;
    const int n_ev = mode != 0 ? n + 1 : 0;   // the fork modes' branch events
    std::vector<hipEvent_t> e_smp(n_ev), e_upd(n_ev), e_grad(n_ev);
    hipEvent_t e_fork = nullptr;
    if (mode != 0) {
        DDRL_HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        DDRL_HIP_CHECK(hipEventCreateWithFlags(&e_fork, hipEventDisableTiming));
    }
    for (int i = 0; i < n_ev; ++i) {
        DDRL_HIP_CHECK(hipEventCreateWithFlags(&e_smp[i], hipEventDisableTiming));
        DDRL_HIP_CHECK(hipEventCreateWithFlags(&e_upd[i], hipEventDisableTiming));
        DDRL_HIP_CHECK(hipEventCreateWithFlags(&e_grad[i], hipEventDisableTiming));
    }
    hipGraph_t graph = nullptr;
    int rc = ddrl_sac1_internal_opt_sync(h->learner, (void *)main_s);  // the graph starts on copy 0 of the optimizer state ...
    if (rc != DDRL_OK) return rc;
    DDRL_HIP_CHECK(hipStreamSynchronize(main_s));  // one-time: the capture stream may not be the caller's
    DDRL_HIP_CHECK(hipStreamBeginCapture(main_s, hipStreamCaptureModeThreadLocal));
    hipError_t e = hipSuccess;
#define HE(x) do { if (e == hipSuccess && rc == DDRL_OK) e = (x); } while (0)
#define RC(x) do { if (e == hipSuccess && rc == DDRL_OK) rc = (x); } while (0)
    if (mode == 0) {
        // sample(0) as a kernel (head-sampled) or drawn by the replay before (pre-sampled); sample(i+1) rides inside update i,
        // the last update's only in a tail-sampling graph.  No store can interleave inside one graph, nor between two replays
        // of one ddrl_loop_run call, so this equals the sequential sample -> update order.
        if (!pre) RC(sample_into(h, start, (void *)main_s));
        for (int i = 0; i < n; ++i) {
            const int set = (start + i) & 1;
            RC(ddrl_sac1_fill_noise(h->learner, h->seed, (void *)main_s));
            if (i + 1 < n || tail) {
                RC(ddrl_sac1_step_and_sample(h->learner, set, h->replay, set ^ 1, (void *)main_s));
            } else {
                float **b = h->buf[set];
                RC(ddrl_sac1_step(h->learner, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr,
                                  (void *)main_s));
            }
        }
    } else if (mode == 2) {
        HE(hipEventRecord(e_fork, main_s));
        HE(hipStreamWaitEvent(side, e_fork, 0));
        for (int i = 0; i < n; ++i) {
            if (i >= 2) HE(hipStreamWaitEvent(side, e_upd[i - 2], 0));  // set i&1 was last read by update i-2
            RC(sample_into(h, i & 1, (void *)side));
            HE(hipEventRecord(e_smp[i], side));
            HE(hipStreamWaitEvent(main_s, e_smp[i], 0));
            RC(update_from(h, i & 1, (void *)main_s));
            HE(hipEventRecord(e_upd[i], main_s));
        }
    } else {
        // sample(0) inline; then for each update: grads(i) -> [fork: sample(i+1)] || apply(i) -> join
        RC(sample_into(h, 0, (void *)main_s));
        for (int i = 0; i < n; ++i) {
            RC(grads_from(h, i & 1, (void *)main_s));
            if (i + 1 < n) {
                HE(hipEventRecord(e_grad[i], main_s));
                HE(hipStreamWaitEvent(side, e_grad[i], 0));
                RC(sample_into(h, (i + 1) & 1, (void *)side));
                HE(hipEventRecord(e_smp[i + 1], side));
            }
            RC(ddrl_sac1_apply_grads(h->learner, (void *)main_s));
            if (i + 1 < n) HE(hipStreamWaitEvent(main_s, e_smp[i + 1], 0));
        }
    }
    RC(ddrl_sac1_internal_opt_sync(h->learner, (void *)main_s));  // ... and ends on it (a copy node when n is odd)
#undef HE
#undef RC
    // every side-branch node is an ancestor of a main-stream node: the branch is joined
    hipError_t e2 = hipStreamEndCapture(main_s, &graph);
    for (int i = 0; i < n_ev; ++i) { (void)hipEventDestroy(e_smp[i]); (void)hipEventDestroy(e_upd[i]); (void)hipEventDestroy(e_grad[i]); }
    if (e_fork) (void)hipEventDestroy(e_fork);
    if (side) (void)hipStreamDestroy(side);
    if (rc != DDRL_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || e2 != hipSuccess) {
        ddrl::set_error("graph capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        if (graph) (void)hipGraphDestroy(graph);
        return DDRL_ERR_HIP;
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

// The whole family, or nothing: a failure destroys the graphs already built.  The fork modes shape the per_graph-sized graph only.
// COST: the lengths sum to < 3 x per_graph and each has up to 4 variants (8 where per_graph is odd), so the one-time capture holds
// up to 12 x per_graph updates (24 x where odd) of five kernel nodes each, against per_graph before: 450 updates in 26 graphs at 50,
// where the first capturing call takes what it took with the single graph (26.5 ms).  It grows linearly: ~33 000 updates /
// ~164 000 nodes at the accepted maximum of 4096, a size nothing here runs at.
static int capture_family(ddrl_loop *h, hipStream_t main_s) {
    const int mode = fork_mode();
    h->chain = mode == 0;
    h->family = ddrl_family::lengths(h->per_graph);
    for (auto &g : h->family)
        for (int v = 0; v < 8; ++v) {
            const int pre = v >> 2, start = (v >> 1) & 1, tail = v & 1;
            if (!variant_needed(h, g.len, pre, start, tail)) continue;
            const int rc = capture(h, main_s, g.len, g.len == h->per_graph ? mode : 0, pre, start, tail, &g.exec[pre][start][tail]);
            if (rc != DDRL_OK) { destroy_family(h); return rc; }
        }
    h->captured = true;
    return DDRL_OK;
}

extern "C" {

int ddrl_loop_create(ddrl_loop_t **out, ddrl_sac1_t *learner, ddrl_replay_t *replay, int32_t updates_per_graph,
                     uint32_t noise_seed) {
    DDRL_REQUIRE(out && learner && replay, "NULL pointer");
    DDRL_REQUIRE(updates_per_graph >= 0 && updates_per_graph <= 4096, "updates_per_graph must be in [0, 4096]");
    ddrl_loop *h = new ddrl_loop();
    h->learner = learner; h->replay = replay; h->per_graph = updates_per_graph; h->seed = noise_seed;
    h->chain = false; h->captured = false; h->parity = 0;
    int rc = ddrl_sac1_input_buffers(learner, 0, h->buf[0]);
    if (rc == DDRL_OK) rc = ddrl_sac1_input_buffers(learner, 1, h->buf[1]);
    if (rc != DDRL_OK) { delete h; return rc; }
    h->batch = ddrl_sac1_batch(learner);
    *out = h;
    return DDRL_OK;
}

int ddrl_loop_destroy(ddrl_loop_t *h) {
    if (!h) return DDRL_OK;
    destroy_family(h);
    delete h;
    return DDRL_OK;
}

int ddrl_loop_run(ddrl_loop_t *h, int64_t n_updates, void *stream) {
    DDRL_REQUIRE(h != nullptr && n_updates >= 0, "bad handle / n_updates");
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
        if (left > 0) {  // eager updates since the last replay may have left the optimizer state on copy 1
            const int rc2 = ddrl_sac1_internal_opt_sync(h->learner, stream);
            if (rc2 != DDRL_OK) return rc2;
        }
        const int rc3 = ddrl_family::replay(h->family, h->chain, left, s);   // greedy, head-sampled first, tail-sampling all but the last
        if (rc3 != DDRL_OK) return rc3;
    }
    for (; left > 0; --left) {
        int rc = one_update(h, stream);
        if (rc != DDRL_OK) return rc;
    }
    return DDRL_OK;
}

}  // extern "C"
