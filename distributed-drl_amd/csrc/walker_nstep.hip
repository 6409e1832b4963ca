// The n-step worker's env launch on the BIPEDAL WALKER (ddrl_env_step_wrapped_walker):
//   k_walker_step_wrapped   k_env3_step_wrapped (rollout3_nstep.hip) statement for statement over Walker (walker_device.h): `Wrapper(env,
//                           obs_noise, act_noise, reward_scale, action_repeat)` of algos/sac1/hyperparams.py:107-134 around env.step plus
//                           the n-step rollout's episode bookkeeping (algos/sac1/sac_ray.py:212-216, 238-258).  The specification it
//                           reproduces BIT-EXACTLY is tests/walker_wrapped_oracle.py.  One lane per env, one wave per workgroup and the
//                           sweeps' read-only fields in LDS, as k_walker_step (walker.hip).
// The kernel holds ONE inlined Walker::physics and ONE inlined Walker::obs: the `repeat` action trips and the zero-action trip inside the
// reset of an env whose episode ended (build() + one step) are trips of the same run-time loop, and the observation — the lidar's 14
// terrain loads and 130 ray tests — is computed behind an env's LAST action trip and behind its reset trip only, never per sub-step:
// obs() is a pure function of the state, so the result is the one `repeat` plain steps give.  That, and one state load / store where
// they make `repeat`, is where the launch does less work than they do (profiles/walker_wrapped_time.txt).
// Across the solver the kernel carries, beyond k_walker_step's registers, the reward sum and the env's trip count; the reward is formed
// on the last action trip (every earlier assignment of hyperparams.py:134 is overwritten), and "no observation noise" is the uniform
// test repeat == 1 (:132-133 is the only branch that clears it).  The Wrapper's scalars are wave-uniform.
// profiles/walker_wrapped_resource_usage.txt holds the compiler's report (no scratch, no VGPR spill).
// A translation unit of its own: the kernels of walker.hip, lander.hip, env3.hip and rollout*.hip compile exactly as before.
#include "ddrl_common.h"
#include "walker_device.h"
#include "env_launch.h"

namespace {

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

__global__ void __launch_bounds__(64) k_walker_step_wrapped(float *S, long long n, uint32_t seed, float limit_steps, int vit, int pit,
                                                            float *act, float act_noise, float obs_noise, float reward_scale, int repeat,
                                                            float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                            uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    __shared__ float wl[W_LDS_FIELDS][64];
    if (i < n) {
        Walker e;
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
    // episode statistics: wave reduction, one atomic per wave that saw an episode end (a lane with i >= n brings zeros)
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

}  // namespace

// ---- internal (env.hip: ddrl_env_step_wrapped_walker) -----------------------------------------------------------------------------
int ddrl_walker_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                    float obs_noise, float reward_scale, int action_repeat, float *obs2_d, float *rew_d, float *done_d,
                                    float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_walker_step_wrapped<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)limit_steps, vit, pit, act_d, act_noise, obs_noise, reward_scale, action_repeat, obs2_d, rew_d, done_d, next_obs_d,
        ended_d, reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
