// The n-step worker's two env launches on the ARTICULATED lander (ddrl_env_step_wrapped_articulated, ddrl_rollout_step_nstep_articulated):
//   k_env3_step_wrapped   k_env_step_wrapped (lander.hip) statement for statement over Env3 (env3_device.h): `Wrapper(env, obs_noise,
//                         act_noise, reward_scale, action_repeat)` of algos/sac1/hyperparams.py:107-134 around env.step plus the n-step
//                         rollout's episode bookkeeping (algos/sac1/sac_ray.py:212-216, 238-258).  One lane per env, one wave per
//                         workgroup as k_env3_step (env3.hip): the sweeps are one serial chain per env.
//   k_env3_step_nstep     the six phases of k_env_step_nstep (a to f in rollout_nstep.hip's header comment) with the three-body solver in
//                         phase b.  The readiness ranking and phases c, d and f are rollout_nstep_device.h's — the code k_env_step_nstep
//                         runs, not a copy; ddrl_nstep_launch_begin / k_nstep_begin (rollout_nstep.hip) serve the begin call unchanged.
// The solver already fills the register file (k_env3_step: 256 VGPRs and AGPRs as spill space, no scratch), so k_env3_step_nstep is
// ordered as k_env3_step_pi (rollout3.hip): the policy head — partials, bias, normal_at, policy_row — is finished BEFORE the env state
// is loaded, and only the noisy action, the reward sum and the ranking's total cross physics(): the action must (the repeat loop and
// the window tail need it), the total is wave-uniform and sits in a scalar register, the env's slot is read again behind the solver.
// The launch's arguments are a hundred scalar registers' worth (queues, ring, mirrors, plan tables), and everything behind the solver
// needs them: held in SGPRs they are spilled into VGPR lanes across the solver, and those VGPRs were what tipped the kernel into a
// private segment.  So lane 0 PARKS the argument struct in LDS (s_a, published by the ranking's barrier) and phases c to f read it
// there; only the Wrapper's scalars stay in registers across the solver.
// The repeat loop is a run-time loop around ONE inlined Env3::physics (a second one sits in Env3::reset, as in every step kernel of this
// model).  profiles/lander3_nstep_rollout_resource_usage.txt holds the compiler's report (no scratch).
// As in k_env_step_nstep only the ring ticket and the version counts (ver_plan_tail) cross workgroups: no spin, no fence.
// A translation unit of its own: the kernels of lander.hip, env3.hip, rollout_nstep.hip and rollout3.hip compile exactly as before.
#include "ddrl_common.h"
#include "policy_row.h"
#include "replay_device.h"
#include "env3_device.h"
#include "version_plan.h"
#include "rollout_nstep.h"
#include "rollout_nstep_device.h"
#include "env_launch.h"

namespace {

constexpr uint32_t RESET_NOISE_STREAM = 0xFFFFFFEFu;   // as lander.hip: the Wrapper's reset-observation noise (hyperparams.py:119-121)

__device__ __forceinline__ void put_obs(float *dst, long long i, const float *o) {
    float4 *p = reinterpret_cast<float4 *>(dst + i * 8);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(64) k_env3_step_wrapped(float *S, long long n, uint32_t seed, float limit_steps, int vit, int pit, float *act,
                                                          float act_noise, float obs_noise, float reward_scale, int repeat,
                                                          float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                          uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    if (i < n) {
        Env3 e;
        e.seed = seed; e.id = (uint32_t)i; e.vit = vit; e.pit = pit;
        e.load(S, n, i);
        float o[8];
        bool done_env = false;
        const uint32_t st0 = (uint32_t)e.pstep;
        const float2 a = *reinterpret_cast<const float2 *>(act + i * 2);
        const float a0 = a.x + act_noise * (-2.0f * e.rng(st0, 2) + 1.0f);   // hyperparams.py:124
        const float a1 = a.y + act_noise * (-2.0f * e.rng(st0, 3) + 1.0f);
        *reinterpret_cast<float2 *>(act + i * 2) = make_float2(a0, a1);       // `action += ...` mutates the caller's array: the rollout queues the NOISY action
        float r = 0.0f, rew = 0.0f;
        bool noisy = true;
#pragma nounroll
        for (int k = 0; k < repeat; ++k) {                                    // :126-133
            const float rk = e.physics(a0, a1, done_env, o);
            r = r + rk;
            if (done_env && repeat != 1) { rew = 0.0f; break; }               // :130-131 (the reward is dropped)
            if (repeat == 1) { rew = r; noisy = false; break; }               // :132-133 (no noise, no scale)
            rew = reward_scale * r;                                           // :134 when the loop runs out
        }
        if (noisy) {
            const uint32_t st1 = (uint32_t)e.pstep;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(st1, 4 + j) + 1.0f);
        }
        e.eplen = e.eplen + 1.0f;                                             // sac_ray.py:216
        e.epret = e.epret + rew;                                              // :215
        const bool ended = done_env || e.eplen >= limit_steps;                // :252
        if (obs2) put_obs(obs2, i, o);
        if (rew_out) rew_out[i] = rew;
        if (done_out) done_out[i] = done_env ? 1.0f : 0.0f;                   // raw d (the time-limit override is commented out, :221)
        if (ended_out) ended_out[i] = ended ? 1 : 0;
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = o[j] + obs_noise * (-2.0f * e.rng(RESET_NOISE_STREAM, j) + 1.0f);  // hyperparams.py:119-121
        }
        if (next_obs) put_obs(next_obs, i, o);
        e.store(S, n, i);
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

struct NStep3Launch {
    NStepLaunch r;
    int vit, pit;
};

__global__ void __launch_bounds__(64) k_env3_step_nstep(NStep3Launch k) {
    const NStepLaunch &a = k.r;
    extern __shared__ float4 s_win[];            // 64 x (Ln + 1) x 2 float4
    __shared__ long long s_ptr;
    __shared__ long long s_row[64];
    __shared__ NStepLaunch s_a;                  // the arguments, parked for what runs behind the solver
    const int lane = threadIdx.x;
    if (lane == 0) { s_ptr = a.rs->ptr; s_a = a; }
    const long long n = a.n, i0 = (long long)blockIdx.x * 64, i = i0 + lane;
    const bool valid = i < n;
    const int ne = (int)(n - i0 < 64 ? n - i0 : 64);
    // ---- the readiness ranking (nothing in this launch writes the bytes it reads): the ring row of every ready env
    int base = 0, total_v = 0;
    DDRL_NSTEP_READY_ROWS(a, n, i0, i, valid, lane, s_ptr, s_row, base, total_v)
    const int total = __builtin_amdgcn_readfirstlane(total_v);   // (every lane holds the same sum: a scalar register across the solver)
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;
    const NStepLaunch &b = s_a;                  // (read behind the ranking's barrier only)
    float o2[8], o[8];
    float a0 = 0.f, a1 = 0.f, rew = 0.f;
    bool done_env = false, ended = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) { o2[j] = 0.f; o[j] = 0.f; }
    if (valid) {
        // ---- a. the policy head (k_env_step_nstep's statements: act_dim 2), finished before the env state is loaded
        {
            const int nq = (a.nt2 + 3) >> 2;
            float4 hm[2][4], hl[2][4];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int qq = q < nq ? q : 0;
                    hm[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)c * n + i) * 16 + 4 * qq);
                    hl[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)(2 + c) * n + i) * 16 + 4 * qq);
                }
            const int cur_slot = a.slot ? a.slot[i] : 0;
            const long long voff = a.versioned ? (long long)cur_slot * a.vstride : 0;
            float mu[4], ls[4], ev[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float sm = 0.f, sl = 0.f;
                if (c < 2) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (q < nq) {  // n-tile order; slots beyond nt2 hold 0
                            const float4 m4 = hm[c < 2 ? c : 0][q], l4 = hl[c < 2 ? c : 0][q];
                            sm += m4.x; sm += m4.y; sm += m4.z; sm += m4.w;
                            sl += l4.x; sl += l4.y; sl += l4.z; sl += l4.w;
                        }
                    }
                }
                const int cc = c < 2 ? c : 0;
                mu[c] = sm + a.bmu[voff + cc];
                ls[c] = sl + a.bls[voff + cc];
                ev[c] = c >= 2 ? 0.f : ddrl_pol::normal_at(a.noise_seed, a.noise_ctr + (unsigned long long)(i * 2 + c));
            }
            const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, 2, a.scale);
            a0 = pr.act[0]; a1 = pr.act[1];
        }
        // ---- b. Wrapper.step + the rollout's episode bookkeeping (k_env3_step_wrapped)
        Env3 e;
        e.seed = a.seed; e.id = (uint32_t)i; e.vit = k.vit; e.pit = k.pit;
        e.load(a.S, n, i);
        const uint32_t st0 = (uint32_t)e.pstep;
        a0 = a0 + a.act_noise * (-2.0f * e.rng(st0, 2) + 1.0f);              // hyperparams.py:124
        a1 = a1 + a.act_noise * (-2.0f * e.rng(st0, 3) + 1.0f);
        float r = 0.0f;
        bool noisy = true;
#pragma nounroll
        for (int kk = 0; kk < a.repeat; ++kk) {                              // :126-133
            const float rk = e.physics(a0, a1, done_env, o);
            r = r + rk;
            if (done_env && a.repeat != 1) { rew = 0.0f; break; }            // :130-131 (the reward is dropped)
            if (a.repeat == 1) { rew = r; noisy = false; break; }            // :132-133 (no noise, no scale)
            rew = a.reward_scale * r;                                        // :134 when the loop runs out
        }
        if (noisy) {
            const uint32_t st1 = (uint32_t)e.pstep;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = o[j] + a.obs_noise * (-2.0f * e.rng(st1, 4 + j) + 1.0f);
        }
        e.eplen = e.eplen + 1.0f;                                            // sac_ray.py:216
        e.epret = e.epret + rew;                                             // :215
        ended = done_env || e.eplen >= b.limit_steps;                        // :252
#pragma unroll
        for (int j = 0; j < 8; ++j) o2[j] = o[j];
        // ---- e. episode end
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = o[j] + b.obs_noise * (-2.0f * e.rng(RESET_NOISE_STREAM, j) + 1.0f);  // hyperparams.py:119-121
        }
        e.store(b.S, n, i);
        // (the env's slot is read again here rather than carried across the solver; nothing has written it since phase a)
        if (b.vcnt) my_slot = (ended && b.adopt) ? *b.newest : (b.slot ? b.slot[i] : 0);
        if (ended && b.slot && b.adopt) b.slot[i] = *b.newest;               // sac_ray.py:259-262
        nstep_queue_tick(b, i, ended);                                       // ---- c. t_queue, and the NEXT step's readiness
        DDRL_NSTEP_MIRRORS(b, i, o, o2, a0, a1, rew, done_env, ended)        // ---- f. the next observation and the mirrors
    }
    // ---- c. + d. the windows: slide, append, store the ready rows, start the ended envs' queues anew
    nstep_windows(b, i0, ne, s_win, s_row, lane, valid, o2, o, a0, a1, rew, done_env, ended);
    // the statistics, the next forward's plan and the ring ticket
    DDRL_NSTEP_FINISH(b, n, i, lane, n_end, len_end, ret_end, my_slot, s_ptr, total)
}

}  // namespace

// ---- internal (env.hip: ddrl_env_step_wrapped_articulated / ddrl_rollout_step_nstep_articulated) --------------------------------
int ddrl_env3_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                  float obs_noise, float reward_scale, int repeat, float *obs2_d, float *rew_d, float *done_d,
                                  float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_env3_step_wrapped<<<(unsigned)((n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)limit_steps, vit, pit, act_d, act_noise, obs_noise, reward_scale, repeat, obs2_d, rew_d, done_d, next_obs_d, ended_d,
        reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_nstep3_launch_step(const NStepLaunch &a, int vit, int pit, void *stream) {
    const size_t lds = (size_t)64 * (a.Ln + 1) * 8 * sizeof(float);
    const NStep3Launch k{a, vit, pit};
    k_env3_step_nstep<<<(unsigned)((a.n + 63) / 64), 64, lds, ddrl::as_stream(stream)>>>(k);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
