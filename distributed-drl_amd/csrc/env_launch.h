// Every env model's launch functions as env.hip's model table reaches them, declared once: the one-body lander's (lander.hip), the
// articulated lander's (env3.hip, rollout3*.hip), the walker's (walker.hip) and the n-step fused step's (rollout_nstep.hip).
// Host side only, and no device header: a translation unit that includes this sees no kernel code it did not see before.
// Internal to libddrl_hip.so.  The callers have checked the arguments and selected the device; vit / pit are the handle's iteration
// counts (the one-body model has none and ignores them: its launches take them so that one table row type holds all three models).
#pragma once
#include <cstdint>

struct NStepLaunch;   // rollout_nstep.h

// ---- the one-body lander (lander.hip): [n,8] observations, [n,2] actions
int ddrl_lander_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream);
int ddrl_lander_launch_step(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                            float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
int ddrl_lander_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                    float obs_noise, float reward_scale, int repeat, float *obs2_d, float *rew_d, float *done_d,
                                    float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
// the observations of the envs' present state into obs_d[n][8] (no reset, no step): the fused begin calls
int ddrl_lander_launch_obs(float *S, long long n, uint32_t seed, float *obs_d, void *stream);
// the fused steps: `args` points to a RolloutArgs / RolloutQArgs (rollout_args.h).  The structs have internal linkage in each
// translation unit, so they cross the boundary as bytes.  versioned selects the instantiation with the version store (slot / newest /
// vp are read then only)
int ddrl_lander_launch_step_pi(const void *args, int vit, int pit, void *stream);
int ddrl_lander_launch_step_q(const void *args, int versioned, int vit, int pit, void *stream);
// ... and the n-step fused step (rollout_nstep.hip).  ddrl_nstep_launch_begin is every lander's begin launch (it reads the queues only):
// obs_d[n][8] = the newest entry of every env's o_queue (the observation its worker holds); rdy_d[i] = readiness of t_queue[i] (i < n)
int ddrl_nstep_launch_step(const NStepLaunch &a, void *stream);
int ddrl_nstep_launch_begin(const float *qo, long long n, int Ln, float *obs_d, const int *t_queue, int save_freq, uint8_t *rdy_d, void *stream);

// ---- the articulated lander: reset / step (env3.hip), the fused steps (rollout3.hip, rollout3_q.hip; `args` as above, the
// RolloutQArgs with its three mirrors set), the wrapped step and the n-step fused step with Env3's solver in the middle (rollout3_nstep.hip)
int ddrl_env3_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream);
int ddrl_env3_launch_step(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                          float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
int ddrl_env3_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                  float obs_noise, float reward_scale, int repeat, float *obs2_d, float *rew_d, float *done_d,
                                  float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
int ddrl_rollout3_launch_obs(const float *S, long long n, float *obs_d, void *stream);   // Env3::obs of every env's state
int ddrl_rollout3_launch_step(const void *args, int vit, int pit, void *stream);
int ddrl_rollout3_launch_step_q(const void *args, int versioned, int vit, int pit, void *stream);
int ddrl_nstep3_launch_step(const NStepLaunch &a, int vit, int pit, void *stream);

// ---- the walker (walker.hip): [n,24] observations, [n,4] actions.  hardcore selects the terrain mode's instantiation: 0 the grass
// walker (state block [DDRL_ENVW_STATE_FIELDS][n]), 1 the Hardcore terrain ([DDRL_ENVWH_STATE_FIELDS][n])
int ddrl_walker_launch_reset(int hardcore, float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d,
                             void *stream);
int ddrl_walker_launch_step(int hardcore, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                            float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
int ddrl_walker_launch_step_wrapped(int hardcore, float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d,
                                    float act_noise, float obs_noise, float reward_scale, int action_repeat, float *obs2_d, float *rew_d,
                                    float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
