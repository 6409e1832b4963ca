// Batched ARTICULATED lander (DDRL_ENV_ARTICULATED): the kernels behind ddrl_env_reset / ddrl_env_step / ddrl_env_step_discrete for
// a handle of ddrl_env_create_ex(kind = 1).  One lane per env, state as struct-of-arrays [DDRL_ENV3_STATE_FIELDS][n] (coalesced
// per-field loads / stores), the same episode bookkeeping as k_env_step (example/dsac.py:102-127).  The model and its solver are in
// env3_device.h; the specification both reproduce BIT-EXACTLY is tests/lander3_oracle.py.
// The Gauss-Seidel sweeps are a serial chain per env (gym's budget: 180 velocity and up to 60 position sweeps over 2 joints and 8
// contact points), so the launch is latency-bound: one wave per workgroup spreads the envs over as many CUs as there are waves, and
// __launch_bounds__(64) leaves the register allocator the whole file (the bodies, joint rows and contact points stay in VGPRs: no
// scratch — profiles/lander3_resource_usage.txt).
// These kernels live in a translation unit of their own so that lander.hip's kernels compile exactly as before.
#include "ddrl_common.h"
#include "env3_device.h"
#include "dqn_select.h"
#include "env_launch.h"

namespace {

__device__ __forceinline__ void put_obs(float *dst, long long i, const float *o) {
    float4 *p = reinterpret_cast<float4 *>(dst + i * 8);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(64) k_env3_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask,
                                                   float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Env3 e;
    e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
    e.load(S, n, i);
    float o[8];
    if (!mask || mask[i]) {
        e.reset(o);
        e.store(S, n, i);
    } else {
        e.obs(o);
    }
    if (obs_out) put_obs(obs_out, i, o);
}

// DISCRETE: act[n] holds gym's discrete action index as float32, mapped through ddrl_sel::lander_action onto the hull's engines
template <bool DISCRETE>
__global__ void __launch_bounds__(64) k_env3_step(float *S, long long n, uint32_t seed, float max_ep_len, int vit, int pit,
                                                  const float *act, float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                  uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    if (i < n) {
        Env3 e;
        e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
        e.load(S, n, i);
        float o[8];
        bool done_env;
        float2 a;
        if (DISCRETE) ddrl_sel::lander_action(act[i], a.x, a.y);
        else a = *reinterpret_cast<const float2 *>(act + i * 2);
        const float rew = e.physics(a.x, a.y, done_env, o);
        e.eplen = e.eplen + 1.0f;                       // example/dsac.py:104
        e.epret = e.epret + rew;                        // :103
        const bool limit = e.eplen >= max_ep_len;
        const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);  // :109
        const bool ended = done_env || limit;                              // :118
        if (obs2) put_obs(obs2, i, o);
        if (rew_out) rew_out[i] = rew;
        if (done_out) done_out[i] = done_store;
        if (ended_out) ended_out[i] = ended ? 1 : 0;
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);                                 // :127
        }
        if (next_obs) put_obs(next_obs, i, o);
        e.store(S, n, i);
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

// ---- internal (env.hip: the ddrl_env_* entry points of an articulated handle) ------------------------------------------------
int ddrl_env3_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream) {
    k_env3_reset<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, vit, pit, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_env3_launch_step(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                          float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    const unsigned grid = (unsigned)((n + 63) / 64);
    EnvStats *st = reinterpret_cast<EnvStats *>(stats_d);
    if (discrete)
        k_env3_step<true><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d,
                                                                    next_obs_d, ended_d, st);
    else
        k_env3_step<false><<<grid, 64, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, vit, pit, act_d, obs2_d, rew_d, done_d,
                                                                     next_obs_d, ended_d, st);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
