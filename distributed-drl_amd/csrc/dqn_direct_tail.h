// The direct-operand tail of a Double-DQN / soft-Q learner whose layer 1 stays on the generic kernels (ddrl_dqn_create_direct_tail,
// include/ddrl_dqn_direct_tail.h): what dqn.hip calls of dqn_direct_tail.hip.  The state is opaque to dqn.hip; it owns W2, b2, W3, b3 of
// main, target, m, v and the gradient in the direct layout and everything between H1 and dZ1.  W1 / b1, H1, dZ1 and the optimizer's
// beta powers stay the handle's own.
#pragma once
#include "ddrl_common.h"

struct ddrl_dqn_tx;

// what the tail reads and writes of the handle (device memory that lives as long as the handle)
struct ddrl_dqn_tx_bind {
    const float *H1;          // [evaluation][batch][ldh1] as the layer-1 forward leaves it, column hidden1 holds 1
    int ldh1;
    float *dZ1;               // [network][batch][hidden1]: the B operand of the layer-1 weight gradient
    float *loss;              // the handle's loss word
    long long gen_off[2][3];  // W2, b2, [W3 ; b3] of network n inside a buffer of the generic layout (the stale-shadow rewrite of main)
};

// the envelope; outside it: DDRL_ERR_UNSUPPORTED with ddrl_dqn_create_direct_tail's name and the reason in ddrl_last_error()
int ddrl_dqn_tx_check(const ddrl_dqn_config_t *cfg);
int ddrl_dqn_tx_create(ddrl_dqn_tx **out, int device, const ddrl_dqn_config_t *cfg, const ddrl_dqn_tx_bind *bind);
void ddrl_dqn_tx_destroy(ddrl_dqn_tx *d);
// the tail's segments of a dense vector in external order -> buffer `which` (DDRL_SAC1_MAIN / _TARGET / _ADAM_M / _ADAM_V); and_target: main AND target
int ddrl_dqn_tx_pack(ddrl_dqn_tx *d, int which, const float *flat_d, bool and_target, hipStream_t s);
// buffer `which` (the gradient included) -> the tail's segments of a dense vector in external order; the other elements are not touched
int ddrl_dqn_tx_unpack(ddrl_dqn_tx *d, int which, float *flat_d, hipStream_t s);
// main's W2, b2, W3, b3 -> a buffer of the generic layout (one launch)
int ddrl_dqn_tx_shadow(ddrl_dqn_tx *d, float *generic_main, hipStream_t s);
// the launches between the layer-1 forward and the layer-1 weight gradient.  acts / rew / done: this update's rows; zero_words (nullable):
// n_zero polled words of a later launch of this update, cleared by the second launch
int ddrl_dqn_tx_fwd_mid(ddrl_dqn_tx *d, const float *acts, const float *rew, const float *done, int *zero_words, int n_zero, hipStream_t s);
// the last launch: W2 / b2 / W3 / b3 weight gradients, Adam (step size from `opt` as it stands: an OptState of gemm_core.h; the layer-1 Adam launch advances it) +
// polyak, the loss mean into the handle's word and loss_d (nullable)
int ddrl_dqn_tx_last(ddrl_dqn_tx *d, const void *opt, float *loss_d, hipStream_t s);
// q(x) of the main network as the last update saw it: [batch][n_actions]
const float *ddrl_dqn_tx_qrows(ddrl_dqn_tx *d);
