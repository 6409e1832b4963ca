// The BIPEDAL WALKER on the HARDCORE terrain (include/ddrl_walker_hardcore.h): the kernels behind ddrl_env_reset / ddrl_env_step /
// ddrl_env_step_wrapped_walker for a handle of ddrl_env_create_walker(terrain = DDRL_WALKER_TERRAIN_HARDCORE).
//   k_walker_hc_reset          k_walker_reset (walker.hip)
//   k_walker_hc_step           k_walker_step (walker.hip)
//   k_walker_hc_step_wrapped   k_walker_step_wrapped (walker_nstep.hip)
// each statement for statement over WalkerT<1> (walker_device.h) where its twin runs WalkerT<0>: the model and its solver exist once, in
// that header, and the terrain mode is its compile-time parameter; what stands here is the twins' episode bookkeeping, the Wrapper and
// the statistics.  The specification the three reproduce BIT-EXACTLY is tests/walker_hardcore_oracle.py (the wrapped step:
// tests/walker_wrapped_oracle.py's step_wrapped on that class).  State block [DDRL_ENVWH_STATE_FIELDS][n].
// One lane per env, one wave per workgroup, __launch_bounds__(64); bodies and the accumulated impulses of the 16 contact slots in
// registers, what a sweep only reads in LDS as [field][lane] (W_LDS_FIELDS_H = 172 fields, 43 KiB per workgroup), never in scratch
// memory (profiles/walker_hardcore_resource_usage.txt); ONE inlined physics step per kernel, the reset trip sharing the loop body, and
// one lidar pass per wrapped step.
// A translation unit of its own: the kernels of walker.hip, walker_nstep.hip and walker_eval.hip compile exactly as before.
#include "ddrl_common.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "walker_device.h"
#include "env_launch.h"

namespace {

static_assert(NFWH == DDRL_ENVWH_STATE_FIELDS, "walker_device.h's Hardcore rows are the header's");

constexpr uint32_t RESET_NOISE_STREAM = 0xFFFFFFEFu;   // as walker_nstep.hip
constexpr uint32_t OBS_NOISE_STEP0 = 0x04000000u;      // as walker_nstep.hip

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

__global__ void __launch_bounds__(64) k_walker_hc_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask,
                                                        float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ float wl[W_LDS_FIELDS_H][64];
    if (i >= n) return;
    WalkerHardcore e;
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

__global__ void __launch_bounds__(64) k_walker_hc_step(float *S, long long n, uint32_t seed, float max_ep_len, int vit, int pit,
                                                       const float *act, float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                       uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    __shared__ float wl[W_LDS_FIELDS_H][64];
    if (i < n) {
        WalkerHardcore e;
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
            e.eplen = e.eplen + 1.0f;
            e.epret = e.epret + rew;
            const bool limit = e.eplen >= max_ep_len;
            const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);
            const bool ended = done_env || limit;
            if (obs2) put_obs24(obs2, i, o);
            if (rew_out) rew_out[i] = rew;
            if (done_out) done_out[i] = done_store;
            if (ended_out) ended_out[i] = ended ? 1 : 0;
            if (!ended) break;
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.build();
#pragma unroll
            for (int k = 0; k < WACT; ++k) a[k] = 0.0f;
        }
        if (next_obs) put_obs24(next_obs, i, o);
        e.store(S, i);
    }
    put_stats(n_end, len_end, ret_end, stats);
}

__global__ void __launch_bounds__(64) k_walker_hc_step_wrapped(float *S, long long n, uint32_t seed, float limit_steps, int vit, int pit,
                                                               float *act, float act_noise, float obs_noise, float reward_scale,
                                                               int repeat, float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                               uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    __shared__ float wl[W_LDS_FIELDS_H][64];
    if (i < n) {
        WalkerHardcore e;
        e.L = &wl[0][threadIdx.x];
        e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
        e.load(S, n, i);
        const uint32_t st0 = (uint32_t)e.pstep;
        const float4 a4 = *reinterpret_cast<const float4 *>(act + i * WACT);
        float a[WACT] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int c = 0; c < WACT; ++c) a[c] = a[c] + act_noise * (-2.0f * e.rng(st0, 2 + c) + 1.0f);
        // `action += ...` mutates the caller's array: the rollout queues the NOISY action
        *reinterpret_cast<float4 *>(act + i * WACT) = make_float4(a[0], a[1], a[2], a[3]);
        float o[WOBS];
        float r = 0.0f;
        int k = 0;
        bool reset_trip = false;
        // trips 0 .. k_last: Wrapper.step's repeat loop; one more, for an env whose episode ended: the zero-action step inside env.reset()
        for (;;) {
            bool d;
            const float rk = e.physics(a, d);
            float rew = 0.0f;
            if (!reset_trip) {
                r = r + rk;
                k = k + 1;
                const bool brk_done = d && repeat != 1;
                if (!brk_done && repeat != 1 && k < repeat) continue;
                rew = brk_done ? 0.0f : (repeat == 1 ? r : reward_scale * r);
            }
            e.obs(o);
            if (reset_trip) {
#pragma unroll
                for (int j = 0; j < WOBS; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(RESET_NOISE_STREAM, j) + 1.0f);
                break;
            }
            if (repeat != 1) {
                const uint32_t st1 = OBS_NOISE_STEP0 + 2u * (uint32_t)e.pstep;
#pragma unroll
                for (int j = 0; j < WOBS; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(st1, j) + 1.0f);
            }
            e.eplen = e.eplen + 1.0f;
            e.epret = e.epret + rew;
            const bool ended = d || e.eplen >= limit_steps;
            if (obs2) put_obs24(obs2, i, o);
            if (rew_out) rew_out[i] = rew;
            if (done_out) done_out[i] = d ? 1.0f : 0.0f;
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

// ---- internal (env.hip: the ddrl_env_* entry points of a Hardcore walker handle) -----------------------------------------------
int ddrl_walker_hc_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream) {
    k_walker_hc_reset<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, vit, pit, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_walker_hc_launch_step(float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d, float *obs2_d,
                               float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_walker_hc_step<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d, reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_walker_hc_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                       float obs_noise, float reward_scale, int action_repeat, float *obs2_d, float *rew_d, float *done_d,
                                       float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_walker_hc_step_wrapped<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)limit_steps, vit, pit, act_d, act_noise, obs_noise, reward_scale, action_repeat, obs2_d, rew_d, done_d, next_obs_d,
        ended_d, reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
