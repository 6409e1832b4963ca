/* C ABI of libddrl_hip.so, the actor's wide direct-operand policy beside include/ddrl.h: an actor handle whose rollout forward
 * (k_actor_fwd_wide, csrc/actor_wide.h) generates layer 1 on the matrix cores from observation rows of up to 31 columns — the
 * bipedal walker's 24 observations / 4 actions, which ddrl_actor_create's direct-operand envelope (obs_dim + act_dim <= 12) leaves to
 * the row-major kernels and without a version store.  Conventions, status codes, ddrl_last_error(), the stream contract and the memory
 * contract are ddrl.h's; include this header instead of, or after, ddrl.h. */
#ifndef DDRL_ACTOR_WIDE_H
#define DDRL_ACTOR_WIDE_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_actor_create (ddrl.h) with the policy held in the WIDE direct-operand layout.  The handle is an ordinary ddrl_actor_t: every
 * ddrl_actor_* call of ddrl.h takes it — set_weights (plain and on a version store), get_weights (bit-equal to what was set), act and
 * act_one (through the lazily rebuilt row-major copy, as on any direct handle), versions_enable / _state / _adopt and act_versioned
 * (the forward launch is k_actor_fwd_wide, plain or versioned; the store, its planning launch and the finishing launch are shared with
 * the narrow handle) — and ddrl_actor_destroy frees it.  Takes no stream and no caller device memory; allocates on `device`.
 * Envelope: obs_dim <= 31, act_dim <= 4, hidden1 and hidden2 multiples of 4, hidden1 <= 512, hidden2 <= 512, max_rows a multiple of
 * 32 and <= 131040.  Inside it the handle is direct for every obs_dim 1..31.  Outside it: DDRL_ERR_UNSUPPORTED with the reason in
 * ddrl_last_error(), nothing allocated, *out untouched — never a handle that quietly acts through other kernels.  (A NULL out or
 * cfg, non-positive sizes: DDRL_ERR_BAD_ARG, as ddrl_actor_create.)
 * The fused rollout steps (ddrl_rollout_begin* and their step calls) read the narrow layout and refuse a wide handle with the
 * message they give for an actor without a direct-operand policy.  ddrl_actor_create itself is unchanged. */
int ddrl_actor_create_wide(ddrl_actor_t **out, int device, const ddrl_sac1_config_t *cfg, int64_t max_rows);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_ACTOR_WIDE_H */
