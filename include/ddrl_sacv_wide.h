/* C ABI of libddrl_hip.so, the SAC-v learner's wide direct-operand update beside include/ddrl.h and include/ddrl_sac1_wide.h: the
 * learner of example/dsac.py (example/model.py: policy + twin Q + V + target V) whose update is the five-launch direct-operand
 * sequence with a layer-1 contraction over up to 32 input columns (k_dfwd_wide, csrc/sac1_wide.h; the backward launches are k_dg's
 * SAC-v job kinds over the wide layer-1 block layout, csrc/sac1_wide.hip) — a Model of the bipedal walker's 24 observations / 4
 * actions, which ddrl_sac1_create's direct-operand envelope (obs_dim + act_dim <= 12) leaves to the generic kernels.
 * Conventions, status codes, ddrl_last_error(), the stream contract and the memory contract are ddrl.h's. */
#ifndef DDRL_SACV_WIDE_H
#define DDRL_SACV_WIDE_H

#include "ddrl_sac1_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_sac1_create (ddrl.h) for variant DDRL_SAC_V with the policy, q1, q2, V and target V held in the WIDE direct-operand layout
 * (V and target V contract over obs_dim + 1 columns; main, target, m, v and the gradient share the layout).  The handle is an
 * ordinary ddrl_sac1_t: ddrl_sac1_step, _step_host, _step_and_sample (a transition ring or an n-step window ring; the sampler rides in
 * the second forward launch where ddrl_sac1_create's direct SAC-v handle lets it ride, else it is a launch of its own), the captured
 * learner loop, _set_weights / _get_weights, _export / _import of main, target, m, v and the gradient in external order, _fill_noise,
 * _opt_*, _input_buffers, the four losses and the q1 / q2 / logp_pi outputs work as on any handle; ddrl_sac1_is_wide and
 * ddrl_sac1_is_fused answer 1; ddrl_sac1_destroy frees it.  Takes no stream and no caller device memory; allocates on `device`.
 * Envelope: variant DDRL_SAC_V, 1 <= act_dim <= 4, obs_dim + act_dim <= 31, hidden1 and hidden2 multiples of 4 and <= 512,
 * batch <= 512.  Outside it (DDRL_SAC1 included: that learner is ddrl_sac1_create_wide's): DDRL_ERR_UNSUPPORTED with this function's
 * name and the reason in ddrl_last_error(), nothing allocated, nothing launched, *out untouched.  (A NULL out or cfg, non-positive
 * sizes: DDRL_ERR_BAD_ARG, as ddrl_sac1_create.)
 * The split API — ddrl_sac1_compute_grads, _apply_grads, _compute_grads_and_sample, _apply_grads_and_sample — refuses the handle
 * with DDRL_ERR_UNSUPPORTED and the called function's name, as it refuses every wide handle.  ddrl_sac1_create and
 * ddrl_sac1_create_wide are unchanged. */
int ddrl_sacv_create_wide(ddrl_sac1_t **out, int device, const ddrl_sac1_config_t *cfg);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_SACV_WIDE_H */
