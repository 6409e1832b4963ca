/* C ABI of libddrl_hip.so, the walker's terrain modes beside include/ddrl.h, include/ddrl_walker.h (the walker's wrapped step) and
 * include/ddrl_walker_eval.h (its evaluation episodes): the HARDCORE terrain — stumps, pits and stairs — as a mode of the walker kind,
 * carried on the env handle (its evaluation episodes: include/ddrl_walker_hardcore_eval.h).  Conventions, status codes, ddrl_last_error(), the stream contract and the memory contract are ddrl.h's;
 * include this header instead of, or after, ddrl.h. */
#ifndef DDRL_WALKER_HARDCORE_H
#define DDRL_WALKER_HARDCORE_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DDRL_WALKER_TERRAIN_GRASS 0    /* gym's BipedalWalker-v2 terrain: what ddrl_env_create_ex(kind = DDRL_ENV_WALKER) builds */
#define DDRL_WALKER_TERRAIN_HARDCORE 1 /* gym's BipedalWalkerHardcore-v2 terrain generator: grass with stumps, pits and stairs */
/* Rows of a Hardcore handle's state block [DDRL_ENVWH_STATE_FIELDS][n] (ddrl_env_state_fields / _get_state / _set_state): rows 0..285
 * are the grass walker's (DDRL_ENVW_STATE_FIELDS) at their indices; 286 + 2 q + (normal, tangent): the accumulated impulses of corner
 * q's wall slot; 302: the box count; 303 + 4 b + (x0, x1, y0, y1): box b of at most 40; 463 + k: the index of the box that covers
 * terrain column k (k < 200), -1 for none. */
#define DDRL_ENVWH_STATE_FIELDS 663

/* A walker handle (kind DDRL_ENV_WALKER) with a terrain mode.  terrain = DDRL_WALKER_TERRAIN_GRASS: the handle
 * ddrl_env_create_ex(kind = DDRL_ENV_WALKER, velocity_iterations, position_iterations) returns, bit for bit — same kernels, same
 * 286-row state block.  terrain = DDRL_WALKER_TERRAIN_HARDCORE: the model of tests/walker_hardcore_oracle.py (kernels
 * csrc/walker.hip, reproduced bit for bit): gym's hardcore terrain generator, axis-aligned boxes in the state block, two
 * contact slots per leg corner (floor and wall), a hull that ends the episode inside a box, lidar rays that see box edges; unpinned
 * against gym like the grass walker.
 * On a Hardcore handle ddrl_env_reset / _step / _stats / _get_state / _set_state / _state_fields (ddrl.h) and
 * ddrl_env_step_wrapped_walker (ddrl_walker.h) run that model with their memory and stream contracts unchanged (observations [n,24]
 * and actions [n,4] on the 16-byte grid); ddrl_env_state_fields returns DDRL_ENVWH_STATE_FIELDS.  The handle's kind stays
 * DDRL_ENV_WALKER, so every lander entry point refuses it as it refuses any walker handle.  ddrl_env_eval_policy_walker
 * (ddrl_walker_eval.h) returns DDRL_ERR_UNSUPPORTED on it, the message starting "ddrl_env_eval_policy_walker:" and naming the
 * hardcore terrain, nothing touched: that entry point holds the grass terrain.  The evaluation episodes of a Hardcore handle are
 * ddrl_env_eval_policy_walker_hardcore's (ddrl_walker_hardcore_eval.h), which in turn refuses a grass handle.
 * Allocates and resets every env (a host synchronisation), like ddrl_env_create_ex.
 * DDRL_ERR_BAD_ARG with *out untouched: what ddrl_env_create_ex refuses (a NULL out, n_envs < 1, max_ep_len < 1 or >= 2^24, an
 * iteration count < 1), and a terrain that is neither of the two values above. */
int ddrl_env_create_walker(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len, int32_t velocity_iterations,
                           int32_t position_iterations, int32_t terrain);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_WALKER_HARDCORE_H */
