/* C ABI of libddrl_hip.so, the Double-DQN / soft-Q learners' direct-operand tail beside include/ddrl.h and include/ddrl_dqn_direct.h:
 * the update of a learner whose observations are wider than ddrl_dqn_create_direct takes (config 5's 28 224 pixels, or 14 and up), with
 * layer 1 on the kernels that already serve that width (k_wide / k_wide_sk of csrc/wide_l1.h from obs_dim 1024, k_gemm below) and everything
 * behind H1 on three direct-operand launches — layer 2 and the head partials of every evaluation straight from row-major H1 and a
 * k4-interleaved W2 (k_qtfwd), the row logic + the layer-2 dgrad into the row-major dZ1 the layer-1 weight gradient reads (k_qtmid), the
 * layer-2 and head weight gradients with Adam + polyak in their epilogues (k_qtlast); csrc/dqn_direct_tail.hip.  An update is
 * [stage] -> layer-1 forward -> k_qtfwd -> k_qtmid -> layer-1 wgrad -> k_qtlast -> layer-1 Adam: six kernels for ddrl_dqn_create's seven.
 * Conventions, status codes, ddrl_last_error(), the stream contract and the memory contract are ddrl.h's. */
#ifndef DDRL_DQN_DIRECT_TAIL_H
#define DDRL_DQN_DIRECT_TAIL_H

#include "ddrl.h"
#include "ddrl_dqn_direct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_dqn_create (ddrl.h) with W2, b2, W3, b3 of main, target, Adam m / v and the gradient held in the direct-operand layout; W1 / b1
 * stay in the generic one (never duplicated).  The handle is an ordinary ddrl_dqn_t: ddrl_dqn_step, ddrl_dqn_step_ring (float32 and
 * compact uint8 rings, from obs_dim 1024 as on any handle), _set_weights, _export / _import (external order; the gradient included), _q,
 * _act, _versions_* work as on any handle; ddrl_dqn_destroy frees it.  Takes no stream and no caller device memory.
 * Envelope: variant DDRL_DDQN or DDRL_SQN (alpha > 0), obs_dim >= DDRL_DQN_DIRECT_MAX_OBS_DIM + 1 (narrower: ddrl_dqn_create_direct),
 * 1 <= n_actions <= 8, hidden1 and hidden2 multiples of 4 and <= 512, 1 <= batch <= 512.  Outside it: DDRL_ERR_UNSUPPORTED with this
 * function's name and the reason in ddrl_last_error(), nothing allocated, nothing launched, *out untouched.  (A NULL out or cfg:
 * DDRL_ERR_BAD_ARG.)
 * ddrl_dqn_step_timed and ddrl_dqn_loop_create refuse the handle by name with DDRL_ERR_UNSUPPORTED (the stage list and the captured
 * loop describe other launch sequences).  ddrl_dqn_create and ddrl_dqn_create_direct are unchanged. */
int ddrl_dqn_create_direct_tail(ddrl_dqn_t **out, int device, const ddrl_dqn_config_t *cfg);

/* 1 for a handle of ddrl_dqn_create_direct_tail, 0 for any other (ddrl_dqn_is_direct answers 0 for it; ddrl_dqn_wide_sk keeps its meaning). */
int ddrl_dqn_is_direct_tail(ddrl_dqn_t *h);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_DQN_DIRECT_TAIL_H */
