// Evaluation episodes fed from HANDLES (ddrl_env_eval_policy / ddrl_env_eval_q / ddrl_env_eval_results), and the instantiations of the
// evaluation kernels for the ARTICULATED lander: k_eval_episodes<Env3, .> and k_eval_episodes_q<Env3, .> (bodies: eval_episodes.h).
// One workgroup of 256 threads per episode, as on the one-body lander: the policy / Q row on all threads in the summation order
// stated in eval.hip / eval_q.hip, then ONE lane runs Env3::reset / Env3::physics (env3_device.h: the three bodies, the joint rows and
// the eight contact points in registers, `vit` velocity and up to `pit` position sweeps) and the bookkeeping of k_env3_step (env3.hip):
// eplen, epret, ended = done_env || eplen >= max_ep_len.  The discrete kernel maps its pick through ddrl_sel::lander_action first.
// k_env3_step runs under __launch_bounds__(64) to keep that state in VGPRs; a 256-thread workgroup is one wave per SIMD, so each wave
// still has the whole register file.  The compiler's report is in profiles/eval3_resource_usage.txt.
// The env handle NAMES the model (kind, iteration counts, seed, max_ep_len, device) and owns the results block; its state block,
// statistics and observations are neither read nor written.  The weights come out of the agent handle (ddrl_actor_get_weights: the
// newest installed version; ddrl_dqn_export(MAIN): q1 leads the flat vector) into a staging vector the env handle owns, one pack
// launch in front of the episodes' launch on the same stream.  The results-block reservation and the common argument check are
// eval_host.h's, shared with walker_eval.hip (the walker's episodes: ddrl_env_eval_policy_walker).
// A translation unit of its own, as env3.hip and rollout3.hip: eval.hip's and eval_q.hip's kernels compile exactly as before.
#include "ddrl_common.h"
#include "env3_device.h"
#include "env_handle.h"
#include "eval_episodes.h"
#include "eval_host.h"

extern "C" {

int ddrl_env_eval_policy(ddrl_env_t *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode, int32_t want_trace, void *stream) {
    const char *what = "ddrl_env_eval_policy";
    if (const int rc = eval_common_check(what, h, actor, n_episodes, first_episode, [&] {
            return ddrl_env_refuse(h, DDRL_TAKES_LANDERS, what, nullptr);   // no lander kernel holds the walker: ddrl_env_eval_policy_walker
        })) return rc;
    ddrl_sac1_config_t cfg;
    int adev = -1;
    if (const int rc = ddrl_actor_internal_config(actor, &cfg, &adev)) return rc;
    if (adev != h->device) {
        ddrl::set_error("%s: bad argument: the actor lives on device %d, the env handle on device %d", what, adev, h->device);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.obs_dim != 8 || cfg.act_dim != 2) {
        ddrl::set_error("%s: bad argument: the lander has 8 observations and 2 actions (actor: %d -> %d)", what, cfg.obs_dim, cfg.act_dim);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.hidden1 < 1 || cfg.hidden2 < 1 || cfg.hidden1 > 512 || cfg.hidden2 > 512) {
        ddrl::set_error("%s: hidden width outside [1, 512] (the envelope of ddrl_actor_act_one): step a host env instead", what);
        return DDRL_ERR_UNSUPPORTED;
    }
    int64_t n_pi = 0, n_q = 0;
    if (const int rc = ddrl_sac1_param_counts(&cfg, &n_pi, &n_q)) return rc;
    ddrl::DeviceGuard g(h->device);
    if (const int rc = eval_reserve(h, what, n_episodes, want_trace ? EV_ROW : 0, (size_t)n_pi)) return rc;
    if (const int rc = ddrl_actor_get_weights(actor, h->ev_w, stream)) return rc;
    double *ret = reinterpret_cast<double *>(h->ev_block);
    int *len = reinterpret_cast<int *>(h->ev_block + h->ev_len_off);
    float *trace = want_trace ? reinterpret_cast<float *>(h->ev_block + h->ev_trace_off) : nullptr;
    if (h->kind == DDRL_ENV_ARTICULATED) {
        EvalArgs a = eval_args_of(cfg, h->ev_w);
        a.ret = ret; a.len = len; a.trace = trace;
        a.max_ep_len = h->max_ep_len;
        a.seed = h->seed; a.first = first_episode;
        a.vit = h->vit; a.pit = h->pit;
        eval_launch<Env3>(a, n_episodes, ddrl::as_stream(stream));
        DDRL_LAUNCH_CHECK();
    } else {   // the very launch of ddrl_policy_eval, fed from the handles
        if (const int rc = ddrl_policy_eval(&cfg, h->ev_w, n_episodes, h->seed, first_episode, h->max_ep_len, ret, len, trace, stream)) return rc;
    }
    h->ev_n = n_episodes; h->ev_row = want_trace ? EV_ROW : 0;
    return DDRL_OK;
}

int ddrl_env_eval_q(ddrl_env_t *h, ddrl_dqn_t *dqn, int32_t n_episodes, uint32_t first_episode, int mode, float greedy_prob,
                    uint32_t noise_seed, uint64_t noise_ctr, int32_t want_trace, void *stream) {
    const char *what = "ddrl_env_eval_q";
    if (const int rc = eval_common_check(what, h, dqn, n_episodes, first_episode, [&] {
            return ddrl_env_refuse(h, DDRL_TAKES_LANDERS, what, nullptr);   // no Q-network evaluation holds the walker
        })) return rc;
    ddrl_dqn_config_t cfg;
    int adev = -1;
    if (const int rc = ddrl_dqn_internal_config(dqn, &cfg, &adev)) return rc;
    if (adev != h->device) {
        ddrl::set_error("%s: bad argument: the Q network lives on device %d, the env handle on device %d", what, adev, h->device);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.obs_dim != 8 || cfg.n_actions < 1) {
        ddrl::set_error("%s: bad argument: the lander has 8 observations (Q network: %d -> %d)", what, cfg.obs_dim, cfg.n_actions);
        return DDRL_ERR_BAD_ARG;
    }
    if (mode != DDRL_ACT_SAMPLE && mode != DDRL_ACT_DETERMINISTIC) {
        ddrl::set_error("%s: bad argument: mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC", what);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.n_actions > ddrl_sel::MAXQ) {
        ddrl::set_error("%s: n_actions > %d (ddrl_sel::select_row<8>): step a host env instead", what, ddrl_sel::MAXQ);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (cfg.hidden1 < 1 || cfg.hidden2 < 1 || cfg.hidden1 > 512 || cfg.hidden2 > 512) {
        ddrl::set_error("%s: hidden width outside [1, 512] (the kernel's LDS layout): step a host env instead", what);
        return DDRL_ERR_UNSUPPORTED;
    }
    int64_t n_main = 0;
    if (const int rc = ddrl_dqn_param_count(&cfg, &n_main)) return rc;
    ddrl::DeviceGuard g(h->device);
    if (const int rc = eval_reserve(h, what, n_episodes, want_trace ? EQ_ROW : 0, (size_t)n_main)) return rc;
    if (const int rc = ddrl_dqn_export(dqn, DDRL_SAC1_MAIN, h->ev_w, stream)) return rc;
    double *ret = reinterpret_cast<double *>(h->ev_block);
    int *len = reinterpret_cast<int *>(h->ev_block + h->ev_len_off);
    float *trace = want_trace ? reinterpret_cast<float *>(h->ev_block + h->ev_trace_off) : nullptr;
    if (h->kind == DDRL_ENV_ARTICULATED) {
        EvalQArgs a = eval_q_args_of(cfg, h->ev_w);
        a.ret = ret; a.len = len; a.trace = trace;
        a.max_ep_len = h->max_ep_len;
        a.deterministic = mode == DDRL_ACT_DETERMINISTIC;
        a.greedy_prob = greedy_prob;
        a.seed = h->seed; a.first = first_episode; a.noise_seed = noise_seed; a.noise_ctr = noise_ctr;
        a.vit = h->vit; a.pit = h->pit;
        eval_q_launch<Env3>(a, n_episodes, ddrl::as_stream(stream));
        DDRL_LAUNCH_CHECK();
    } else {   // the very launch of ddrl_dqn_eval, fed from the handles
        if (const int rc = ddrl_dqn_eval(&cfg, h->ev_w, n_episodes, h->seed, first_episode, h->max_ep_len, mode, greedy_prob, noise_seed,
                                         noise_ctr, ret, len, trace, stream)) return rc;
    }
    h->ev_n = n_episodes; h->ev_row = want_trace ? EQ_ROW : 0;
    return DDRL_OK;
}

int ddrl_env_eval_results(ddrl_env_t *h, void **ret, void **len, void **trace, int32_t *n_episodes, int32_t *max_ep_len, int32_t *trace_row) {
    DDRL_REQUIRE(h != nullptr, "ddrl_env_eval_results: handle is NULL");
    DDRL_REQUIRE(h->ev_n > 0 && h->ev_block != nullptr,
                 "ddrl_env_eval_results: no evaluation has run on this handle (ddrl_env_eval_policy / ddrl_env_eval_q first)");
    if (ret) *ret = h->ev_block;
    if (len) *len = h->ev_block + h->ev_len_off;
    if (trace) *trace = h->ev_row ? h->ev_block + h->ev_trace_off : nullptr;
    if (n_episodes) *n_episodes = h->ev_n;
    if (max_ep_len) *max_ep_len = h->max_ep_len;
    if (trace_row) *trace_row = h->ev_row;
    return DDRL_OK;
}

}  // extern "C"
