// Batched BIPEDAL WALKER (DDRL_ENV_WALKER): the kernels behind ddrl_env_reset / ddrl_env_step / ddrl_env_step_wrapped_walker for a
// handle of ddrl_env_create_ex(kind = 3) or ddrl_env_create_walker (include/ddrl_walker_hardcore.h).  Each is a template over the
// TERRAIN MODE HC of WalkerT<HC> (walker_device.h, where the model and its solver are): <0> the grass walker, specified by
// tests/walker_oracle.py, <1> the HARDCORE terrain, specified by tests/walker_hardcore_oracle.py; the wrapped step's specification is
// tests/walker_wrapped_oracle.py on either class.  All are reproduced BIT-EXACTLY.
//   k_walker_reset          the reset of the masked envs
//   k_walker_step           env.step and the episode bookkeeping of k_env_step (example/dsac.py:102-127)
//   k_walker_step_wrapped   k_env3_step_wrapped (rollout3_nstep.hip) statement for statement over WalkerT: `Wrapper(env, obs_noise,
//                           act_noise, reward_scale, action_repeat)` of algos/sac1/hyperparams.py:107-134 around env.step plus the n-step
//                           rollout's episode bookkeeping (algos/sac1/sac_ray.py:212-216, 238-258)
// One lane per env, state as struct-of-arrays [DDRL_ENVW_STATE_FIELDS][n] ([DDRL_ENVWH_STATE_FIELDS][n] on the Hardcore terrain;
// coalesced per-field loads / stores), observations [n,24] and actions [n,4] moved as float4.
// The Gauss-Seidel sweeps are a serial chain per env (gym's budget: 180 velocity and up to 60 position sweeps over 4 joints and 8 or 16
// contact slots), so the launch is latency-bound: one wave per workgroup spreads the envs over as many CUs as there are waves, and
// __launch_bounds__(64) leaves the register allocator the whole file.  What does not fit it lives in LDS as [field][lane] (27 KiB per
// workgroup on grass, 43 KiB on the Hardcore terrain), never in scratch memory (profiles/walker_resource_usage.txt,
// walker_wrapped_resource_usage.txt, walker_hardcore_resource_usage.txt).
// A step kernel holds ONE inlined physics step: the reset of an env whose episode ended (build() + one zero-action step) is one more
// trip through the same run-time loop, not a second inlined copy, and so are the wrapped step's `repeat` action trips.  The wrapped step
// computes the observation — the lidar's 14 terrain loads and 130 ray tests — behind an env's LAST action trip and behind its reset
// trip only, never per sub-step: obs() is a pure function of the state, so the result is the one `repeat` plain steps give.  That, and
// one state load / store where they make `repeat`, is where the launch does less work than they do (profiles/walker_wrapped_time.txt).
// Across the solver it carries, beyond k_walker_step's registers, the reward sum and the env's trip count; the reward is formed on the
// last action trip (every earlier assignment of hyperparams.py:134 is overwritten), and "no observation noise" is the uniform test
// repeat == 1 (:132-133 is the only branch that clears it).  The Wrapper's scalars are wave-uniform.
#include "ddrl_common.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "walker_device.h"
#include "env_launch.h"

namespace {

static_assert(NFWH == DDRL_ENVWH_STATE_FIELDS, "walker_device.h's Hardcore rows are the header's");

constexpr uint32_t RESET_NOISE_STREAM = 0xFFFFFFEFu;   // as lander.hip: the Wrapper's reset-observation noise (hyperparams.py:119-121)
// The observation noise behind PSTEP st1 is drawn at "step" OBS_NOISE_STEP0 + 2 st1, indices 0..23: 32 hash inputs per PSTEP value in a
// range of their own (0x40000000 + 32 st1 + k).  The landers' layout (indices 4.. of step st1) does not carry over to 24 observations:
// the block would reach into step st1 + 1, where an early break draws again under the same episode seed (tests/walker_wrapped_oracle.py).
constexpr uint32_t OBS_NOISE_STEP0 = 0x04000000u;

__device__ __forceinline__ void put_obs24(float *dst, long long i, const float *o) {
    float4 *p = reinterpret_cast<float4 *>(dst + i * WOBS);
#pragma unroll
    for (int k = 0; k < WOBS / 4; ++k) p[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

// episode statistics: wave reduction, one atomic per wave that saw an episode end (a lane with i >= n brings zeros)
__device__ __forceinline__ void put_stats(long long n_end, long long len_end, double ret_end, EnvStats *stats) {
    for (int off = 32; off >= 1; off >>= 1) {
        n_end += __shfl_xor(n_end, off);
        len_end += __shfl_xor(len_end, off);
        ret_end += __shfl_xor(ret_end, off);
    }
    if ((threadIdx.x & 63) == 0 && n_end > 0) {
        atomicAdd((unsigned long long *)&stats->episodes, (unsigned long long)n_end);
        atomicAdd((unsigned long long *)&stats->len_sum, (unsigned long long)len_end);
        atomicAdd(&stats->ret_sum, ret_end);
    }
}

template <int HC>
__global__ void __launch_bounds__(64) k_walker_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask,
                                                     float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ float wl[WalkerT<HC>::LFIELDS][64];
    if (i >= n) return;
    WalkerT<HC> e;
    e.L = &wl[0][threadIdx.x];
    e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
    e.load(S, n, i);
    if (!mask || mask[i]) {
        const float zero[WACT] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool d;
        e.build();
        (void)e.physics(zero, d);
        e.store(S, i);
    }
    if (obs_out) {
        float o[WOBS];
        e.obs(o);
        put_obs24(obs_out, i, o);
    }
}

template <int HC>
__global__ void __launch_bounds__(64) k_walker_step(float *S, long long n, uint32_t seed, float max_ep_len, int vit, int pit,
                                                    const float *act, float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                    uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    __shared__ float wl[WalkerT<HC>::LFIELDS][64];
    if (i < n) {
        WalkerT<HC> e;
        e.L = &wl[0][threadIdx.x];
        e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
        e.load(S, n, i);
        const float4 a4 = *reinterpret_cast<const float4 *>(act + i * WACT);
        float a[WACT] = {a4.x, a4.y, a4.z, a4.w};
        float o[WOBS];
        // trip 0: the step and its bookkeeping; trip 1, for an env whose episode ended: the zero-action step inside env.reset()
        for (int trip = 0;; ++trip) {
            bool done_env;
            const float rew = e.physics(a, done_env);
            e.obs(o);
            if (trip == 1) break;
            e.eplen = e.eplen + 1.0f;                       // example/dsac.py:104
            e.epret = e.epret + rew;                        // :103
            const bool limit = e.eplen >= max_ep_len;
            const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);  // :109
            const bool ended = done_env || limit;                              // :118
            if (obs2) put_obs24(obs2, i, o);
            if (rew_out) rew_out[i] = rew;
            if (done_out) done_out[i] = done_store;
            if (ended_out) ended_out[i] = ended ? 1 : 0;
            if (!ended) break;
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.build();                                      // :127
#pragma unroll
            for (int k = 0; k < WACT; ++k) a[k] = 0.0f;
        }
        if (next_obs) put_obs24(next_obs, i, o);
        e.store(S, i);
    }
    put_stats(n_end, len_end, ret_end, stats);
}

template <int HC>
__global__ void __launch_bounds__(64) k_walker_step_wrapped(float *S, long long n, uint32_t seed, float limit_steps, int vit, int pit,
                                                            float *act, float act_noise, float obs_noise, float reward_scale, int repeat,
                                                            float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                            uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    __shared__ float wl[WalkerT<HC>::LFIELDS][64];
    if (i < n) {
        WalkerT<HC> e;
        e.L = &wl[0][threadIdx.x];
        e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
        e.load(S, n, i);
        const uint32_t st0 = (uint32_t)e.pstep;
        const float4 a4 = *reinterpret_cast<const float4 *>(act + i * WACT);
        float a[WACT] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int c = 0; c < WACT; ++c) a[c] = a[c] + act_noise * (-2.0f * e.rng(st0, 2 + c) + 1.0f);   // hyperparams.py:124
        // `action += ...` mutates the caller's array: the rollout queues the NOISY action
        *reinterpret_cast<float4 *>(act + i * WACT) = make_float4(a[0], a[1], a[2], a[3]);
        float o[WOBS];
        float r = 0.0f;
        int k = 0;
        bool reset_trip = false;
        // trips 0 .. k_last: Wrapper.step's repeat loop (:126-133); one more, for an env whose episode ended: the zero-action step
        // inside env.reset()
        for (;;) {
            bool d;
            const float rk = e.physics(a, d);
            float rew = 0.0f;
            if (!reset_trip) {
                r = r + rk;
                k = k + 1;
                const bool brk_done = d && repeat != 1;                       // :130-131 (the reward is dropped)
                if (!brk_done && repeat != 1 && k < repeat) continue;
                rew = brk_done ? 0.0f : (repeat == 1 ? r : reward_scale * r);  // :132-133 (no noise, no scale) / :134 when the loop runs out
            }
            e.obs(o);
            if (reset_trip) {
#pragma unroll
                for (int j = 0; j < WOBS; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(RESET_NOISE_STREAM, j) + 1.0f);  // :119-121
                break;
            }
            if (repeat != 1) {
                const uint32_t st1 = OBS_NOISE_STEP0 + 2u * (uint32_t)e.pstep;
#pragma unroll
                for (int j = 0; j < WOBS; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(st1, j) + 1.0f);
            }
            e.eplen = e.eplen + 1.0f;                                         // sac_ray.py:216
            e.epret = e.epret + rew;                                          // :215
            const bool ended = d || e.eplen >= limit_steps;                   // :252
            if (obs2) put_obs24(obs2, i, o);
            if (rew_out) rew_out[i] = rew;
            if (done_out) done_out[i] = d ? 1.0f : 0.0f;                      // raw d (the time-limit override is commented out, :221)
            if (ended_out) ended_out[i] = ended ? 1 : 0;
            if (!ended) break;
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.build();
#pragma unroll
            for (int c = 0; c < WACT; ++c) a[c] = 0.0f;
            reset_trip = true;
        }
        if (next_obs) put_obs24(next_obs, i, o);
        e.store(S, i);
    }
    put_stats(n_end, len_end, ret_end, stats);
}

}  // namespace

// ---- internal (env.hip: the ddrl_env_* entry points of a walker handle; hardcore = the handle's terrain mode) ------------------
int ddrl_walker_launch_reset(int hardcore, float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d,
                             void *stream) {
    const unsigned grid = (unsigned)((n + 63) / 64);
    if (!hardcore)
        k_walker_reset<0><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, vit, pit, mask_d, obs_d);
    else
        k_walker_reset<1><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, vit, pit, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_walker_launch_step(int hardcore, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                            float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    const unsigned grid = (unsigned)((n + 63) / 64);
    EnvStats *st = reinterpret_cast<EnvStats *>(stats_d);
    if (!hardcore)
        k_walker_step<0><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d,
                                                                   next_obs_d, ended_d, st);
    else
        k_walker_step<1><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d,
                                                                   next_obs_d, ended_d, st);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_walker_launch_step_wrapped(int hardcore, float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d,
                                    float act_noise, float obs_noise, float reward_scale, int action_repeat, float *obs2_d, float *rew_d,
                                    float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    const unsigned grid = (unsigned)((n + 63) / 64);
    EnvStats *st = reinterpret_cast<EnvStats *>(stats_d);
    if (!hardcore)
        k_walker_step_wrapped<0><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)limit_steps, vit, pit, act_d, act_noise, obs_noise,
                                                                           reward_scale, action_repeat, obs2_d, rew_d, done_d, next_obs_d,
                                                                           ended_d, st);
    else
        k_walker_step_wrapped<1><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)limit_steps, vit, pit, act_d, act_noise, obs_noise,
                                                                           reward_scale, action_repeat, obs2_d, rew_d, done_d, next_obs_d,
                                                                           ended_d, st);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
