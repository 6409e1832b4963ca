// Batched BIPEDAL WALKER (DDRL_ENV_WALKER): the kernels behind ddrl_env_reset / ddrl_env_step for a handle of
// ddrl_env_create_ex(kind = 3).  One lane per env, state as struct-of-arrays [DDRL_ENVW_STATE_FIELDS][n] (coalesced per-field loads /
// stores), observations [n,24] and actions [n,4] moved as float4, the same episode bookkeeping as k_env_step (example/dsac.py:102-127).
// The model and its solver are in walker_device.h; the specification both reproduce BIT-EXACTLY is tests/walker_oracle.py.
// The Gauss-Seidel sweeps are a serial chain per env (gym's budget: 180 velocity and up to 60 position sweeps over 4 joints and 8 contact
// points), so the launch is latency-bound: one wave per workgroup spreads the envs over as many CUs as there are waves, and
// __launch_bounds__(64) leaves the register allocator the whole file.  What does not fit it lives in LDS, never in scratch memory
// (profiles/walker_resource_usage.txt).  The step kernel holds ONE instance of the physics step: the reset of an env whose episode ended
// is a second trip through the same loop body, not a second inlined copy.
// These kernels live in a translation unit of their own so that lander.hip's and env3.hip's kernels compile exactly as before.
#include "ddrl_common.h"
#include "walker_device.h"
#include "env_launch.h"

namespace {

__device__ __forceinline__ void put_obs24(float *dst, long long i, const float *o) {
    float4 *p = reinterpret_cast<float4 *>(dst + i * WOBS);
#pragma unroll
    for (int k = 0; k < WOBS / 4; ++k) p[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

__global__ void __launch_bounds__(64) k_walker_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask,
                                                     float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ float wl[W_LDS_FIELDS][64];
    if (i >= n) return;
    Walker e;
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

__global__ void __launch_bounds__(64) k_walker_step(float *S, long long n, uint32_t seed, float max_ep_len, int vit, int pit,
                                                    const float *act, float *obs2, float *rew_out, float *done_out, float *next_obs,
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
    // episode statistics: wave reduction, one atomic per wave that saw an episode end
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

// ---- internal (env.hip: the ddrl_env_* entry points of a walker handle) ------------------------------------------------------
int ddrl_walker_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream) {
    k_walker_reset<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, vit, pit, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_walker_launch_step(float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d, float *obs2_d,
                            float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_walker_step<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d, reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
