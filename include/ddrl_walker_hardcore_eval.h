/* C ABI of libddrl_hip.so, the Hardcore walker's evaluation entry point beside include/ddrl.h, include/ddrl_walker.h (the walker's
 * wrapped step), include/ddrl_walker_eval.h (the grass walker's evaluation episodes) and include/ddrl_walker_hardcore.h (the walker's
 * terrain modes): the evaluation episodes of the bipedal walker on the HARDCORE terrain on the device.  Conventions, status codes,
 * ddrl_last_error(), the stream contract and the memory contract are ddrl.h's; include this header instead of, or after, ddrl.h. */
#ifndef DDRL_WALKER_HARDCORE_EVAL_H
#define DDRL_WALKER_HARDCORE_EVAL_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_env_eval_policy_walker (ddrl_walker_eval.h) on the HARDCORE terrain (an env handle of ddrl_env_create_walker with terrain =
 * DDRL_WALKER_TERRAIN_HARDCORE, ddrl_walker_hardcore.h; kernel k_walker_hc_eval, csrc/walker_hardcore_eval.hip): n_episodes
 * deterministic evaluation episodes as ONE launch, one workgroup per episode.  Arguments, rules, the stream contract and the results
 * are ddrl_env_eval_policy_walker's.  The env handle names the model (seed, max_ep_len, iteration counts, device) and owns the results
 * block and the weight staging vector; its state block, statistics and observations are neither read nor written.  The weights come
 * out of the actor handle (ddrl_actor_get_weights on `stream`, in front of the episodes' launch); the actor is not changed.  Episode e
 * is the (first_episode + e)-th episode a host loop plays on a Hardcore walker handle of one env with the same seed, max_ep_len and
 * iteration counts (ddrl_env_reset, then ddrl_actor_act_one in deterministic mode + ddrl_env_step per step), bit for bit: its
 * terrain — stumps, pits, stairs — is generated per episode inside the kernel.
 * Results: ddrl_env_eval_results (ddrl.h) — ret[e] the float64 sum of the float32 step rewards in step order, len[e] int32; with
 * want_trace != 0 a trace of trace_row = 32 floats per step: obs[24] acted on, act[4], rew, ended, then two zeros; rows past an
 * episode's end are zero.  The first call on a handle, and a call that needs a larger block than the last, allocates (and so
 * synchronises the device); a call that fits only launches.
 * Refused before any launch with nothing written, the message starting "ddrl_env_eval_policy_walker_hardcore:".  DDRL_ERR_BAD_ARG: a
 * NULL handle, n_episodes < 1, first_episode + n_episodes > 2^24, the actor on another device than the env handle, an actor that is
 * not 24 -> 4.  DDRL_ERR_UNSUPPORTED: a hidden width outside [1, 512] (the envelope of ddrl_actor_act_one: step a host env instead);
 * a walker handle of the grass terrain (the message names ddrl_env_eval_policy_walker, which takes it); a one-body or an articulated
 * handle (the message ends in "use ddrl_env_eval_policy", which both landers share).  ddrl_env_eval_policy_walker keeps refusing a
 * Hardcore handle, ddrl_env_eval_policy and ddrl_env_eval_q any walker handle. */
int ddrl_env_eval_policy_walker_hardcore(ddrl_env_t *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode, int32_t want_trace,
                                         void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_WALKER_HARDCORE_EVAL_H */
