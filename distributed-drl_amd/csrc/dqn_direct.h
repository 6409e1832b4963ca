// The direct-operand update of a narrow Double-DQN / soft-Q learner (ddrl_dqn_create_direct, include/ddrl_dqn_direct.h): what dqn.hip
// calls of dqn_direct.hip.  The state is opaque to dqn.hip; it owns the parameters (main, target, m, v, gradient in the direct layout),
// the activation images and the launch tables, and reads the handle's two input sets in place.
#pragma once
#include "ddrl_common.h"

constexpr int DDRL_DQN_DIRECT_MAX_OBS = 13;   // the seven-step form of the narrow layer-1 generator: 14 input columns, the last one the bias

struct ddrl_dqn_dx;

// the envelope; outside it: DDRL_ERR_UNSUPPORTED with ddrl_dqn_create_direct's name and the reason in ddrl_last_error()
int ddrl_dqn_dx_check(const ddrl_dqn_config_t *cfg);
// sets[s] = (x1, x2, acts, rew, done) of input set s; observation rows of ldx floats whose column obs_dim holds 1
int ddrl_dqn_dx_create(ddrl_dqn_dx **out, int device, const ddrl_dqn_config_t *cfg, float *const sets[2][5], int ldx);
void ddrl_dqn_dx_destroy(ddrl_dqn_dx *d);
// dense external order -> buffer `which` (DDRL_SAC1_MAIN / _TARGET / _ADAM_M / _ADAM_V) of the direct layout; and_target: main AND target
int ddrl_dqn_dx_pack(ddrl_dqn_dx *d, int which, const float *flat_d, bool and_target, hipStream_t s);
// buffer `which` (the gradient included) -> dense external order; flat_d == nullptr: into the state's own flat vector, which is returned
const float *ddrl_dqn_dx_unpack(ddrl_dqn_dx *d, int which, float *flat_d, hipStream_t s);
// one update on input set `set`: three launches.  ride (nullable): the SetSampler of the next update's draw, one more workgroup of the second
int ddrl_dqn_dx_update(ddrl_dqn_dx *d, int set, const void *ride, float *loss_d, hipStream_t s);
// q(x) of the main network as the last update saw it: [batch][n_actions]
const float *ddrl_dqn_dx_qrows(ddrl_dqn_dx *d);
