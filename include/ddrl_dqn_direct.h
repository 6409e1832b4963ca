/* C ABI of libddrl_hip.so, the Double-DQN / soft-Q learners' direct-operand update beside include/ddrl.h: the narrow update (the
 * reference's discrete learners: hidden (400, 300) at batch 128, the discrete lander's 8 observations / 4 actions) in three launches
 * instead of ddrl_dqn_create's six — every evaluation's layer 1 generated on the matrix cores from the lane's observation row and
 * layer 2 straight from a k4-interleaved W2 (k_qfwd), the row logic + the dgrad with its dZ2 operand generated in the tile (k_qmid),
 * every weight gradient with Adam + polyak in its epilogue (k_qlast); csrc/dqn_direct.hip.
 * Conventions, status codes, ddrl_last_error(), the stream contract and the memory contract are ddrl.h's. */
#ifndef DDRL_DQN_DIRECT_H
#define DDRL_DQN_DIRECT_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest obs_dim of the envelope: the narrow layer-1 generator (csrc/sac1_direct.h: four to seven MFMA steps of two input columns,
 * DFHead::pack holds steps - 4 in two bits) takes 14 input columns, and the bias is one of them. */
#define DDRL_DQN_DIRECT_MAX_OBS_DIM 13

/* ddrl_dqn_create (ddrl.h) with main, target, Adam m / v and the gradient held in the direct-operand layout.  The handle is an ordinary
 * ddrl_dqn_t: ddrl_dqn_step, _set_weights, _export / _import (external order; the gradient included), _q, _act, _versions_*, the fused
 * rollout step and ddrl_dqn_loop_* work as on any handle (the acting forward repacks from main after an update); a captured loop of n
 * updates per graph holds 3 n + 1 kernel nodes; ddrl_dqn_destroy frees it.  Takes no stream and no caller device memory.
 * Envelope: variant DDRL_DDQN or DDRL_SQN (alpha > 0), 1 <= obs_dim <= DDRL_DQN_DIRECT_MAX_OBS_DIM, 1 <= n_actions <= 8, hidden1 and
 * hidden2 multiples of 4 and <= 512, 1 <= batch <= 512.  Outside it: DDRL_ERR_UNSUPPORTED with this function's name and the reason in
 * ddrl_last_error(), nothing allocated, nothing launched, *out untouched.  (A NULL out or cfg: DDRL_ERR_BAD_ARG.)
 * ddrl_dqn_step_timed refuses the handle with DDRL_ERR_UNSUPPORTED (its stage list describes the generic launches); ddrl_dqn_step_ring
 * refuses it as it refuses every narrow handle.  ddrl_dqn_create is unchanged. */
int ddrl_dqn_create_direct(ddrl_dqn_t **out, int device, const ddrl_dqn_config_t *cfg);

/* 1 for a handle of ddrl_dqn_create_direct, 0 for one of ddrl_dqn_create. */
int ddrl_dqn_is_direct(ddrl_dqn_t *h);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_DQN_DIRECT_H */
