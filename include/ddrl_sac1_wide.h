/* C ABI of libddrl_hip.so, the SAC1 learner's wide direct-operand update beside include/ddrl.h: a learner handle whose update is the
 * five-launch direct-operand sequence with a layer-1 contraction over up to 32 input columns (k_dfwd_wide, csrc/sac1_wide.h; the
 * backward launches are k_dg over the wide layer-1 block layout, csrc/sac1_wide.hip) — the bipedal walker's 24 observations / 4
 * actions, which ddrl_sac1_create's direct-operand envelope (obs_dim + act_dim <= 12) leaves to the nine-launch generic kernels.
 * Conventions, status codes, ddrl_last_error(), the stream contract and the memory contract are ddrl.h's; include this header instead
 * of, or after, ddrl.h. */
#ifndef DDRL_SAC1_WIDE_H
#define DDRL_SAC1_WIDE_H

#include "ddrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ddrl_sac1_create (ddrl.h) with policy and twin Q held in the WIDE direct-operand layout.  The handle is an ordinary ddrl_sac1_t:
 * ddrl_sac1_step, _step_host, _step_and_sample (a transition ring or an n-step window ring; the sampler rides in the second forward
 * launch where ddrl_sac1_create's direct handle lets it ride, else it is a launch of its own), the captured learner loop, _set_weights /
 * _get_weights, _export / _import of main, target, m, v and the gradient in external order, _fill_noise, _opt_*, _input_buffers and the
 * loss / q1 / q2 / logp_pi outputs work as on any handle; ddrl_sac1_is_fused answers 1; ddrl_sac1_destroy frees it.
 * Takes no stream and no caller device memory; allocates on `device`.
 * Envelope: variant DDRL_SAC1, 1 <= act_dim <= 4, obs_dim + act_dim <= 31, hidden1 and hidden2 multiples of 4 and <= 512,
 * batch <= 512.  Outside it: DDRL_ERR_UNSUPPORTED with this function's name and the reason in ddrl_last_error(), nothing allocated,
 * nothing launched, *out untouched — never a handle that quietly updates through other kernels.  (A NULL out or cfg, non-positive
 * sizes: DDRL_ERR_BAD_ARG, as ddrl_sac1_create.)
 * The split API — ddrl_sac1_compute_grads, _apply_grads, _compute_grads_and_sample, _apply_grads_and_sample, which serve the
 * data-parallel run — refuses a wide handle with DDRL_ERR_UNSUPPORTED and the called function's name.  ddrl_sac1_create itself is
 * unchanged. */
int ddrl_sac1_create_wide(ddrl_sac1_t **out, int device, const ddrl_sac1_config_t *cfg);

/* 1: `h` came from ddrl_sac1_create_wide; 0: from ddrl_sac1_create; DDRL_ERR_BAD_ARG: NULL. */
int ddrl_sac1_is_wide(ddrl_sac1_t *h);

#ifdef __cplusplus
}
#endif

#endif /* DDRL_SAC1_WIDE_H */
