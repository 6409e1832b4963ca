// The DQN / SQN test worker's evaluation episodes as ONE launch: `Actor.test` (algos/dqn/actor_learner.py:230-251,
// algos/sqn/actor_learner.py:229-250) walks n episodes — get_action(o) then env.step(a), one after the other.  The discrete counterpart
// of k_eval_episodes (eval.hip), with the same decomposition: an episode is a strictly serial chain of one Q row, one selection and
// one env step, the episodes are independent of each other, so one workgroup plays one episode from reset to its end without the
// host and n episodes are n workgroups.  Nothing crosses workgroups (no ticket, no fence, no spin-wait).
//
// The Q row is the main network q1 (SQN: q1 only, as ddrl_dqn_act), 8 -> h1 -> h2 -> A, relu on both hidden layers, a linear head.
// Summation order (the library is built with -ffp-contract=off, so tests/_discrete_eval_trace.py::q_row32 restates it exactly):
//   layer 1   unit j: the bias, then + x[q] * W1[q][j] for q = 0 .. 7 in input order; relu
//   layer 2   column c: 16 slices of per = ceil(h1 / 16) contraction rows (slice s = rows s * per .. min(s * per + per, h1) - 1, empty
//             past h1), each summed in row order from zero; the 16 slice sums added in slice order on the bias; relu
//   head      output a: partials per group of 16 columns (group b = columns 16 b .. 16 b + 15 below h2) in column order from zero, the
//             groups added in group order from zero, then + the head bias
// As in k_eval_episodes a wave takes 64 consecutive columns of one contraction row of W2 per load (256 contiguous bytes, out of L2),
// the layer-1 operands and the env state stay in registers, the hidden layers and the partials live in LDS.
// Selection is ddrl_sel::select_row<8> (dqn_select.h), the function k_dqn_select and k_env_step_q call: step t of episode e of the call
// owns u0 = U(seed, ctr + 2 (e * max_ep_len + t)) and u1 = U(seed, ctr + 2 (e * max_ep_len + t) + 1) of ddrl_uniform_fill's generator.
// The env step is ddrl_sel::lander_action, then Env::physics plus the bookkeeping of k_env_step (lander.hip), run by one lane.
// The kernel body is a template over the env type (eval_episodes.h); this file instantiates it for Env, the one-body lander.
#include "eval_episodes.h"

extern "C" {

int ddrl_dqn_eval(const ddrl_dqn_config_t *cfg, const float *q_flat_d, int32_t n_episodes, uint32_t env_seed, uint32_t first_episode,
                  int32_t max_ep_len, int mode, float greedy_prob, uint32_t noise_seed, uint64_t noise_ctr, double *ret_d, int32_t *len_d,
                  float *trace_d, void *stream) {
    DDRL_REQUIRE(cfg != nullptr && q_flat_d != nullptr && ret_d != nullptr && len_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(cfg->obs_dim == 8 && cfg->n_actions >= 1, "the lander has 8 observations; n_actions must be >= 1");
    DDRL_REQUIRE(n_episodes >= 1 && max_ep_len >= 1, "n_episodes and max_ep_len must be >= 1");
    DDRL_REQUIRE(cfg->hidden1 >= 1 && cfg->hidden2 >= 1, "hidden sizes must be >= 1");
    DDRL_REQUIRE(max_ep_len <= (1 << 24) && (uint64_t)first_episode + (uint64_t)n_episodes <= (1u << 24),
                 "max_ep_len and the episode index must stay exact in float32");
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(trace_d) & 15) == 0, "trace_d must be 16-byte aligned");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    DDRL_REQUIRE(cfg->variant == DDRL_DDQN || (cfg->variant == DDRL_SQN && cfg->alpha > 0.0), "variant must be DDRL_DDQN or DDRL_SQN with alpha > 0");
    if (cfg->hidden1 > 512 || cfg->hidden2 > 512) {
        ddrl::set_error("ddrl_dqn_eval: hidden width > 512 (the kernel's LDS layout): step a host env instead");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (cfg->n_actions > ddrl_sel::MAXQ) {
        ddrl::set_error("ddrl_dqn_eval: n_actions > %d (ddrl_sel::select_row<8>): step a host env instead", ddrl_sel::MAXQ);
        return DDRL_ERR_UNSUPPORTED;
    }
    EvalQArgs a = eval_q_args_of(*cfg, q_flat_d);
    a.ret = ret_d; a.len = len_d; a.trace = trace_d;
    a.max_ep_len = max_ep_len;
    a.deterministic = mode == DDRL_ACT_DETERMINISTIC;
    a.greedy_prob = greedy_prob;
    a.seed = env_seed; a.first = first_episode; a.noise_seed = noise_seed; a.noise_ctr = noise_ctr;
    eval_q_launch<Env>(a, n_episodes, ddrl::as_stream(stream));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

}  // extern "C"
