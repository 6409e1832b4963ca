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
// rides in update u's forward launch — the job of the reference's `Cache` prefetch process
// (algos/sac1/sac1.py:103-130) — and that chain carries on ACROSS the replays of one call:
// only a call's first replay opens with a stand-alone sampler launch, and only its last one ends
// without a draw (the caller may store into the ring before the next call).  bench.py at N = 1:
// 92.30 -> 91.38 ms per 2048-update step (profiles/loop_graph_family_before_after.txt).
// Every graph is one chain of nodes.  This file is the SAC1 learner's four operations and the C
// entry points; the capture, the family and the driver of a call are loop_family.h, shared with
// dqn_loop.hip.
#include "ddrl_common.h"
#include "loop_family.h"

// internal (sac1.hip): put the learner's double-buffered optimizer state on copy 0
int ddrl_sac1_internal_opt_sync(ddrl_sac1_t *h, void *stream);
// internal (sac1.hip): sample_batch into input set `set` of the learner — ddrl_replay_sample for a transition ring, ddrl_replay_sample_nstep
// with the learner's gamma for an n-step window ring (algos/sac1/sac_ray.py:40-51)
int ddrl_sac1_internal_sample_into(ddrl_sac1_t *h, ddrl_replay_t *replay, int set, void *stream);

struct ddrl_loop {
    ddrl_sac1_t *learner;
    ddrl_replay_t *replay;
    uint32_t seed;
    float *buf[2][8];   // buf[set] is the learner's input set `set`
    ddrl_family::Loop st;
};

// The sampler of the next update rides inside this one (ddrl_sac1_step_and_sample: an extra workgroup of a forward launch on the
// fused path, of the Adam kernel otherwise)
static int update(void *ctx, int set, bool draw_next, void *stream) {
    ddrl_loop *h = (ddrl_loop *)ctx;
    const int rc = ddrl_sac1_fill_noise(h->learner, h->seed, stream);  // arms in-kernel noise generation
    if (rc != DDRL_OK) return rc;
    if (draw_next) return ddrl_sac1_step_and_sample(h->learner, set, h->replay, set ^ 1, stream);
    float **b = h->buf[set];
    return ddrl_sac1_step(h->learner, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
}

static ddrl_family::Ops ops_of(ddrl_loop *h) {
    using L = ddrl_loop;
    return {h,
            [](void *c, int set, bool, void *s) { return ddrl_sac1_internal_sample_into(((L *)c)->learner, ((L *)c)->replay, set, s); },
            update,
            [](void *c, void *s) { return ddrl_sac1_internal_opt_sync(((L *)c)->learner, s); },
            nullptr};   // no host bookkeeping after a replay
}

extern "C" {

int ddrl_loop_create(ddrl_loop_t **out, ddrl_sac1_t *learner, ddrl_replay_t *replay, int32_t updates_per_graph,
                     uint32_t noise_seed) {
    DDRL_REQUIRE(out && learner && replay, "NULL pointer");
    DDRL_REQUIRE(updates_per_graph >= 0 && updates_per_graph <= 4096, "updates_per_graph must be in [0, 4096]");
    ddrl_loop *h = new ddrl_loop();
    h->learner = learner; h->replay = replay; h->st.per_graph = updates_per_graph; h->seed = noise_seed;
    int rc = ddrl_sac1_input_buffers(learner, 0, h->buf[0]);
    if (rc == DDRL_OK) rc = ddrl_sac1_input_buffers(learner, 1, h->buf[1]);
    if (rc != DDRL_OK) { delete h; return rc; }
    *out = h;
    return DDRL_OK;
}

int ddrl_loop_destroy(ddrl_loop_t *h) {
    if (!h) return DDRL_OK;
    ddrl_family::destroy(h->st);
    delete h;
    return DDRL_OK;
}

int ddrl_loop_run(ddrl_loop_t *h, int64_t n_updates, void *stream) {
    DDRL_REQUIRE(h != nullptr && n_updates >= 0, "bad handle / n_updates");
    return ddrl_family::run(ops_of(h), h->st, n_updates, stream);
}

}  // extern "C"
