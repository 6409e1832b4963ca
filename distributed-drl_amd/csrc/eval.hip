// The test worker's evaluation episodes as ONE launch: `Actor.test` (algos/sac1/actor_learner.py:199-218) and `Model.test_agent`
// (example/model.py:106-118) walk n deterministic episodes — get_action(o, deterministic) then env.step(a), one after the other.
// An episode is a strictly serial chain of one policy row and one env step, and the episodes are independent of each other:
// one workgroup plays one episode from reset to its end without the host, n episodes are n workgroups.  Nothing crosses
// workgroups (no ticket, no fence, no spin-wait).
//
// The policy row is the arithmetic of k_act_one (actor.hip) statement for statement, so that with -ffp-contract=off it yields the same
// bits as the get_action launch the host loop issues per step: layer-1 units summed in input order on the bias; layer 2 as 16 slices
// of ceil(h1 / 16) contraction rows per column, each summed in row order from zero, the 16 slice sums added in slice order on the
// bias; head partials per group of 16 columns in column order from zero, the groups added in group order, then the head bias; then
// ddrl_pol::policy_row with eps = 0.  Only the assignment of (column, slice) sums to threads differs: a wave takes 64 consecutive
// columns of one contraction row per load (256 contiguous bytes) instead of 16 columns of four slices.
// The env step is Env::physics plus the bookkeeping of k_env_step (lander.hip), run by one lane with the env state in registers.
// The kernel body is a template over the env type (eval_episodes.h); this file instantiates it for Env, the one-body lander.
#include "eval_episodes.h"

extern "C" {

int ddrl_policy_eval(const ddrl_sac1_config_t *cfg, const float *pi_flat_d, int32_t n_episodes, uint32_t env_seed, uint32_t first_episode,
                     int32_t max_ep_len, double *ret_d, int32_t *len_d, float *trace_d, void *stream) {
    DDRL_REQUIRE(cfg != nullptr && pi_flat_d != nullptr && ret_d != nullptr && len_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(cfg->obs_dim == 8 && cfg->act_dim == 2, "the lander has 8 observations and 2 actions");
    DDRL_REQUIRE(n_episodes >= 1 && max_ep_len >= 1, "n_episodes and max_ep_len must be >= 1");
    DDRL_REQUIRE(cfg->hidden1 >= 1 && cfg->hidden2 >= 1, "hidden sizes must be >= 1");
    DDRL_REQUIRE(max_ep_len < (1 << 24) && (uint64_t)first_episode + (uint64_t)n_episodes <= (1u << 24),
                 "max_ep_len and the episode index must stay exact in float32");
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(trace_d) & 15) == 0, "trace_d must be 16-byte aligned");
    if (cfg->hidden1 > 512 || cfg->hidden2 > 512) {
        ddrl::set_error("ddrl_policy_eval: hidden width > 512 (the envelope of ddrl_actor_act_one): step a host env instead");
        return DDRL_ERR_UNSUPPORTED;
    }
    EvalArgs a = eval_args_of(*cfg, pi_flat_d);
    a.ret = ret_d; a.len = len_d; a.trace = trace_d;
    a.max_ep_len = max_ep_len;
    a.seed = env_seed; a.first = first_episode;
    eval_launch<Env>(a, n_episodes, ddrl::as_stream(stream));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

}  // extern "C"
