/* C ABI of libddrl_hip.so, the walker's entry points beside include/ddrl.h: what has been added for the bipedal walker
 * (DDRL_ENV_WALKER) since ddrl.h's set of declarations was closed.  Conventions, status codes, ddrl_last_error(), the stream contract
 * and the memory contract are ddrl.h's; include this header instead of, or after, ddrl.h.  (A walker handle's terrain mode:
 * include/ddrl_walker_hardcore.h; on a Hardcore handle the function below runs that terrain's kernel, contract unchanged.  The
 * walker's evaluation episodes: include/ddrl_walker_eval.h on grass, include/ddrl_walker_hardcore_eval.h on the Hardcore terrain.) */
#ifndef DDRL_WALKER_H
#define DDRL_WALKER_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_env_step_wrapped (ddrl.h) on the WALKER (an env handle of ddrl_env_create_ex, kind = DDRL_ENV_WALKER; kernel k_walker_step_wrapped,
 * specification tests/walker_wrapped_oracle.py): the Wrapper and the n-step rollout's bookkeeping statement for statement as
 * ddrl_env_step_wrapped has them, around the five-body solver with the handle's iteration counts; every physics step inside the repeat
 * is bit for bit ddrl_env_step's on this handle, and the observation is computed once, behind the last one.  The noise draws are the
 * walker's own counter streams: slots 2..5 of the stream of the step before the repeat for the four actions, 24 slots of a range of
 * its own indexed by the step behind it for the 24 observations, a stream of its own for the reset observation.
 * Memory: act_d is [n,4], read AND written (the in-place `action += ...`), 16-byte aligned (a row moves as one float4); obs2_d and
 * next_obs_d are [n,24], written only, 16-byte aligned (a row moves as six float4); rew_d and done_d are [n] floats, ended_d [n] bytes,
 * written only.  Each of the five outputs may be NULL (not written); act_d may not.  Nothing outside these extents is touched, no
 * allocation, no host synchronisation; the launch goes to `stream`.  done_d is the raw d, ended = d or ep_len >= limit_steps.
 * DDRL_ERR_BAD_ARG before any launch, with the pointer's or this function's name in ddrl_last_error() and state, statistics, outputs and
 * act_d unchanged: a NULL handle or act_d, a pointer off its 16-byte grid, action_repeat < 1, limit_steps < 1.  On a one-body or an
 * articulated handle: DDRL_ERR_UNSUPPORTED, the message starting "ddrl_env_step_wrapped_walker:" and naming the twin to use
 * (ddrl_env_step_wrapped / ddrl_env_step_wrapped_articulated), nothing launched or written.  Those two keep refusing a walker handle. */
int ddrl_env_step_wrapped_walker(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale,
                                 int32_t action_repeat, int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d,
                                 float *next_obs_d, uint8_t *ended_d, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_WALKER_H */
