// DQN / SQN learner hot loop: `batch = replay_buffer.sample_batch(B); agent.train(batch, cnt)` (algos/dqn/train.py:66-76 on
// algos/dqn/actor_learner.py:110-119; algos/sqn likewise), n iterations per call with no host work per update — the discrete
// counterpart of loop.hip.  Every cursor, the ring's MT19937 state and the optimizer state live on the device, so the sequence is
// captured ONCE into a family of hipGraphs (loop_plan.h: `updates_per_graph` and every power of two below it, variants by
// pre-sampled / starting input set / tail-sampling) and replayed; a call consumes its updates greedily, so after the capture no
// update runs eagerly.  An update here is ddrl_dqn_step's launches WITHOUT the staging one: the sampler writes the padded images
// of one of the learner's two input sets directly, and consecutive updates alternate between the sets, so the sampler of update
// u + 1 never overwrites what update u still reads — it rides as one more workgroup of update u's head launch (dqn.hip:
// k_dqn_head_sample).  Only a call's first update opens with a stand-alone sampler launch and only its last one draws nothing (the
// caller may store into the ring before the next call); the result equals the sequential sample -> update order, bit for bit
// (loop_family.h: linear_body; tests/test_gpu_dqn_loop.py).
// A captured update is 6 kernel nodes (7 eager launches minus the staging one); a head-sampled graph of n updates 6 n + 1, plus a
// copy node of the optimizer state where n is odd.  This file is the learner's four operations and the C entry points; the
// capture, the family and the driver of a call are loop_family.h, shared with loop.hip.
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
    float *loss_d;
    ddrl_family::Loop st;
};

// Eager draws ask the ring for rows (an empty ring surfaces there), captured ones do not
static ddrl_family::Ops ops_of(ddrl_dqn_loop *h) {
    using L = ddrl_dqn_loop;
    return {h,
            [](void *c, int set, bool eager, void *s) { return ddrl_dqn_internal_sample_into(((L *)c)->learner, ((L *)c)->replay, set, eager, s); },
            [](void *c, int set, bool draw_next, void *s) {
                return ddrl_dqn_internal_update(((L *)c)->learner, set, draw_next ? ((L *)c)->replay : nullptr, ((L *)c)->loss_d, s);
            },
            [](void *c, void *s) { return ddrl_dqn_internal_opt_sync(((L *)c)->learner, s); },
            [](void *c, int64_t n) { ddrl_dqn_internal_note_updates(((L *)c)->learner, n); }};
}

extern "C" {

int ddrl_dqn_loop_create(ddrl_dqn_loop_t **out, ddrl_dqn_t *learner, ddrl_replay_t *replay, int32_t updates_per_graph, float *loss_d) {
    DDRL_REQUIRE(out && learner && replay, "NULL pointer");
    DDRL_REQUIRE(updates_per_graph >= 0 && updates_per_graph <= 4096, "updates_per_graph must be in [0, 4096]");
    const int rc = ddrl_dqn_internal_loop_check(learner, replay);
    if (rc != DDRL_OK) return rc;
    ddrl_dqn_loop *h = new ddrl_dqn_loop();
    h->learner = learner; h->replay = replay; h->st.per_graph = updates_per_graph; h->loss_d = loss_d;
    *out = h;
    return DDRL_OK;
}

int ddrl_dqn_loop_destroy(ddrl_dqn_loop_t *h) {
    if (!h) return DDRL_OK;
    ddrl_family::destroy(h->st);
    delete h;
    return DDRL_OK;
}

int ddrl_dqn_loop_info(ddrl_dqn_loop_t *h, int32_t *info_h) {
    DDRL_REQUIRE(h != nullptr && info_h != nullptr, "NULL pointer");
    info_h[0] = h->st.per_graph; info_h[1] = h->st.captured ? 1 : 0; info_h[2] = h->st.nodes[0]; info_h[3] = h->st.nodes[1];
    return DDRL_OK;
}

int ddrl_dqn_loop_run(ddrl_dqn_loop_t *h, int64_t n_updates, void *stream) {
    DDRL_REQUIRE(h != nullptr && n_updates >= 0, "bad handle / n_updates");
    if (ddrl_replay_internal_has_feed(h->replay)) {
        ddrl::set_error("ddrl_dqn_loop_run: the ring has a feed plan attached (ddrl_replay_set_feed): the DQN / SQN loop's sampler does not follow one");
        return DDRL_ERR_UNSUPPORTED;
    }
    return ddrl_family::run(ops_of(h), h->st, n_updates, stream);
}

}  // extern "C"
