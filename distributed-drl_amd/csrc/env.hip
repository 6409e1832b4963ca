// Batched lander environment: one thread per environment, state as struct-of-arrays
// [DDRL_ENV_STATE_FIELDS][n] in HBM (coalesced per-field loads/stores).  Stands where the
// reference calls gym's LunarLanderContinuous-v2 env.step / env.reset
// (example/dsac.py:78-79,102,127) and fuses the worker's per-step episode bookkeeping
// (example/dsac.py:102-127: ep_len/ep_ret, "time limit is not a terminal", reset at episode end).
//
// The dynamics are this build's own Box2D-style rigid-body model — see oracle/env_oracle.py for
// the specification; this kernel reproduces that restatement BIT-EXACTLY: float32, no FMA
// contraction (-ffp-contract=off), correctly rounded sqrt/divide, polynomial sin/cos shared with
// the oracle, counter-hash RNG.  Every arithmetic statement below mirrors one line of the oracle.
#include "ddrl_common.h"
#include "../../include/ddrl_walker.h"
#include "policy_row.h"
#include "replay_device.h"
#include "env_device.h"
#include "env_handle.h"
#include "dqn_select.h"
#include "version_plan.h"
#include "rollout_nstep.h"
#include "rollout_args.h"

namespace {

__global__ void __launch_bounds__(256) k_env_reset(float *S, long long n, uint32_t seed, const uint8_t *mask, float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.seed = seed; e.id = (uint32_t)i;
    e.load(S, n, i);
    float o[8];
    if (!mask || mask[i]) {
        e.reset(o);
        e.store(S, n, i);
    } else {
        e.obs(o);
    }
    if (obs_out) {
        float4 *p = reinterpret_cast<float4 *>(obs_out + i * 8);
        p[0] = make_float4(o[0], o[1], o[2], o[3]);
        p[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
}

// DISCRETE: act[n] holds gym's discrete action index as float32 (ddrl_env_step_discrete), mapped through ddrl_sel::lander_action
template <bool DISCRETE>
__global__ void __launch_bounds__(256) k_env_step(float *S, long long n, uint32_t seed, float max_ep_len, const float *act,
                                                  float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                  uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    if (i < n) {
        Env e;
        e.seed = seed; e.id = (uint32_t)i;
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
        if (obs2) {
            float4 *p = reinterpret_cast<float4 *>(obs2 + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
        if (rew_out) rew_out[i] = rew;
        if (done_out) done_out[i] = done_store;
        if (ended_out) ended_out[i] = ended ? 1 : 0;
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);                                 // :127
        }
        if (next_obs) {
            float4 *p = reinterpret_cast<float4 *>(next_obs + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
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

// `Wrapper(env, obs_noise, act_noise, reward_scale, action_repeat)` of algos/sac1/hyperparams.py:107-134
// around env.step, plus the n-step rollout's episode bookkeeping (algos/sac1/sac_ray.py:212-216,
// 238-258: ep_len counts WRAPPED steps, the episode ends on d or ep_len >= limit_steps, the stored
// done is the raw d).  The wrapper's np.random.random noise is the env's counter generator
// (slots 2.. of the per-step stream; a stream of its own for the reset observation).
constexpr uint32_t RESET_NOISE_STREAM = 0xFFFFFFEFu;
__global__ void __launch_bounds__(256) k_env_step_wrapped(float *S, long long n, uint32_t seed, float limit_steps, float *act,
                                                          float act_noise, float obs_noise, float reward_scale, int repeat,
                                                          float *obs2, float *rew_out, float *done_out, float *next_obs,
                                                          uint8_t *ended_out, EnvStats *stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    if (i < n) {
        Env e;
        e.seed = seed; e.id = (uint32_t)i;
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
        if (obs2) {
            float4 *p = reinterpret_cast<float4 *>(obs2 + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
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
        if (next_obs) {
            float4 *p = reinterpret_cast<float4 *>(next_obs + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
        e.store(S, n, i);
    }
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


// ------------------------------------------------------------------------------------------
// Fused rollout step (RolloutDevice.step = num_envs iterations of example/dsac.py:96-130 in the policy phase):
//   a = agent.get_action(o)      the policy-head partials of the forward launch in front of this kernel are summed in
//                                n-tile order, tanh-squashed with the counter-hash noise (ddrl_pol::policy_row)
//   o2, r, d, _ = env.step(a)    the physics above
//   replay_buffer.store(o, a, r, o2, d)   straight into ring row (ptr + i) % capacity — the n stores in env order,
//                                like ddrl_replay_store; the last block to finish advances the cursor
//   o = o2 (or env.reset())      written into the actor's observation buffer for the next forward launch
// One thread per env: no exchange between threads except the cursor ticket.
// ------------------------------------------------------------------------------------------
template <int NH>  // head partial rows fetched per env: 4 (act_dim <= 2) or 8
__global__ void __launch_bounds__(64) k_env_step_pi(RolloutArgs a) {
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = a.rs->ptr;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;       // the version this env acts on at the NEXT step
    if (i < n) {
        // ---- loads first: head partials (mu heads 0..act-1, log_std heads act..2act-1), the acted-on observation, the env state
        const int nq = (a.nt2 + 3) >> 2;  // float4 groups of a partial row that hold tiles
        // (two statically indexed register arrays: one array indexed by `c + act` would live in scratch memory)
        constexpr int NA = NH / 2;
        float4 hm[NA][4], hl[NA][4];
#pragma unroll
        for (int c = 0; c < NA; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cm = c < a.act ? c : 0, qq = q < nq ? q : 0;
                hm[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)cm * n + i) * 16 + 4 * qq);
                hl[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)(a.act + cm) * n + i) * 16 + 4 * qq);
            }
        float o1[8];
        {
            const float4 *p = reinterpret_cast<const float4 *>(a.obs + i * 8);
            const float4 u = p[0], v = p[1];
            o1[0] = u.x; o1[1] = u.y; o1[2] = u.z; o1[3] = u.w; o1[4] = v.x; o1[5] = v.y; o1[6] = v.z; o1[7] = v.w;
        }
        Env e;
        e.seed = a.seed; e.id = (uint32_t)i;
        e.load(a.S, n, i);
        float mu[4], ls[4], ev[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float sm = 0.f, sl = 0.f;
            if (c < NA) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < nq) {  // n-tile order; slots beyond nt2 hold 0
                        const float4 m4 = hm[c < NA ? c : 0][q], l4 = hl[c < NA ? c : 0][q];
                        sm += m4.x; sm += m4.y; sm += m4.z; sm += m4.w;
                        sl += l4.x; sl += l4.y; sl += l4.z; sl += l4.w;
                    }
                }
            }
            const int cc = c < a.act ? c : 0;
            const long long voff = a.slot ? (long long)a.slot[i] * a.vstride : 0;
            mu[c] = sm + a.bmu[voff + cc];
            ls[c] = sl + a.bls[voff + cc];
            ev[c] = (a.deterministic || c >= a.act) ? 0.f : ddrl_pol::normal_at(a.noise_seed, a.noise_ctr + (unsigned long long)(i * a.act + c));
        }
        const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, a.act, a.scale);
        const float a0 = a.deterministic ? tanhf(mu[0]) * a.scale : pr.act[0];
        const float a1 = a.act > 1 ? (a.deterministic ? tanhf(mu[1]) * a.scale : pr.act[1]) : 0.f;
        // ---- env.step + the worker's bookkeeping (as k_env_step)
        float o[8];
        bool done_env;
        const float rew = e.physics(a0, a1, done_env, o);
        e.eplen = e.eplen + 1.0f;                       // example/dsac.py:104
        e.epret = e.epret + rew;                        // :103
        const bool limit = e.eplen >= a.max_ep_len;
        const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);  // :109
        const bool ended = done_env || limit;                              // :118
        // ---- replay_buffer.store(o, a, r, o2, d): ring arrays {obs1, obs2, acts, rews, done}
        const long long cap = a.ring.capacity;
        if (i >= n - cap) {  // rows that a later store of the same batch would overwrite are skipped (n > capacity)
            const long long row = (s_ptr + i) % cap;
            float4 *p1 = reinterpret_cast<float4 *>(a.ring.a[0] + row * 8), *p2 = reinterpret_cast<float4 *>(a.ring.a[1] + row * 8);
            p1[0] = make_float4(o1[0], o1[1], o1[2], o1[3]); p1[1] = make_float4(o1[4], o1[5], o1[6], o1[7]);
            p2[0] = make_float4(o[0], o[1], o[2], o[3]); p2[1] = make_float4(o[4], o[5], o[6], o[7]);
            *reinterpret_cast<float2 *>(a.ring.a[2] + row * 2) = make_float2(a0, a1);
            a.ring.a[3][row] = rew;
            a.ring.a[4][row] = done_store;
        }
        if (a.act_out) *reinterpret_cast<float2 *>(a.act_out + i * 2) = make_float2(a0, a1);
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);                                 // :127
            if (a.slot) a.slot[i] = *a.newest;          // :129-130  weights = ps.pull(keys); agent.set_weights(keys, weights)
        }
        if (a.vcnt) my_slot = ended ? *a.newest : a.slot[i];
        {
            float4 *p = reinterpret_cast<float4 *>(a.obs + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
            if (a.next_obs_out) {
                float4 *q = reinterpret_cast<float4 *>(a.next_obs_out + i * 8);
                q[0] = p[0]; q[1] = p[1];
            }
        }
        e.store(a.S, n, i);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        n_end += __shfl_xor(n_end, off);
        len_end += __shfl_xor(len_end, off);
        ret_end += __shfl_xor(ret_end, off);
    }
    if ((threadIdx.x & 63) == 0 && n_end > 0) {
        atomicAdd((unsigned long long *)&a.stats->episodes, (unsigned long long)n_end);
        atomicAdd((unsigned long long *)&a.stats->len_sum, (unsigned long long)len_end);
        atomicAdd(&a.stats->ret_sum, ret_end);
    }
    // the next forward's plan (ver_plan_tail, version_plan.h): the grouping, the ring ticket — the last block to finish advances the ring
    // cursor (every block has read rs->ptr before its ticket) — and, in that last workgroup, the forward's workgroup table
    const VerPlan vp{a.vcnt, a.perm, a.perm2d_off, a.vtiles, a.vs, a.n_slots, a.col_tiles, a.wg_slots, a.vt_cap};
    ver_plan_tail(vp, my_slot, i, n, RingTicket{a.rs, a.ring, s_ptr, n});
}

// ------------------------------------------------------------------------------------------
// Fused DISCRETE rollout step (RolloutDeviceDQN.step = num_envs iterations of worker_rollout_dqn's policy phase,
// algos/dqn/train.py:253-274), the sibling of k_env_step_pi for the Double-DQN / SQN actors:
//   a = agent.get_action(o)      the Q-head partials of the forward launch in front of this kernel summed in column-tile order + bias
//                                (ddrl_sel::q_row_from_partials), one index selected per env (ddrl_sel::select_row: the device function
//                                ddrl_dqn_act's selection kernel runs), two uniforms of the counter generator per env
//   o2, r, d, _ = env.step(a)    the physics above on gym's discrete action table (ddrl_sel::lander_action)
//   replay_buffer.store(o, a, r, o2, d)   into ring row (ptr + i) % capacity of a (obs1[8], obs2[8], acts, rews, done) ring, env order;
//                                the last block to finish advances the cursor (ring_commit)
//   o = o2 (or env.reset())      written into the forward's observation buffer for the next forward launch
// One thread per env; no exchange between threads except the cursor ticket, and — as in k_env_step_pi, for the reason documented
// there — no __threadfence() in front of it: nothing but the ticket crosses workgroups inside this launch.
// ------------------------------------------------------------------------------------------
// (RolloutQArgs: rollout_args.h, shared with the articulated lander's k_env3_step_q, rollout3_q.hip.)
// VER: a version store is live.  The plain instantiation is the kernel without one: no slot load, no static LDS for the table build.
template <int NH, bool VER>
__global__ void __launch_bounds__(64) k_env_step_q(RolloutQArgs a) {
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = a.rs->ptr;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;       // the version this env acts on at the NEXT step
    if (i < n) {
        float q[ddrl_sel::MAXQ];
        if (VER) my_slot = a.slot[i];
        ddrl_sel::q_row_from_partials<NH>(a.hp, n, i, a.A, a.half, a.nt2, a.b_lo, a.b_hi, VER ? (long long)my_slot * a.vstride : 0ll, q);
        float o1[8];
        {
            const float4 *p = reinterpret_cast<const float4 *>(a.obs + i * 8);
            const float4 u = p[0], v = p[1];
            o1[0] = u.x; o1[1] = u.y; o1[2] = u.z; o1[3] = u.w; o1[4] = v.x; o1[5] = v.y; o1[6] = v.z; o1[7] = v.w;
        }
        Env e;
        e.seed = a.seed; e.id = (uint32_t)i;
        e.load(a.S, n, i);
        const float u0 = ddrl_sel::uniform_at(a.noise_seed, a.noise_ctr + 2ull * (unsigned long long)i);
        const float u1 = ddrl_sel::uniform_at(a.noise_seed, a.noise_ctr + 2ull * (unsigned long long)i + 1ull);
        const float act = (float)ddrl_sel::select_row(q, a.A, a.sqn, a.deterministic, a.greedy_prob, a.alpha, u0, u1);
        float a0, a1;
        ddrl_sel::lander_action(act, a0, a1);
        // ---- env.step + the worker's bookkeeping (as k_env_step)
        float o[8];
        bool done_env;
        const float rew = e.physics(a0, a1, done_env, o);
        e.eplen = e.eplen + 1.0f;
        e.epret = e.epret + rew;
        const bool limit = e.eplen >= a.max_ep_len;
        const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);
        const bool ended = done_env || limit;
        // ---- replay_buffer.store(o, a, r, o2, d)
        const long long cap = a.ring.capacity;
        if (i >= n - cap) {  // rows that a later store of the same batch would overwrite are skipped (n > capacity)
            const long long row = (s_ptr + i) % cap;
            float4 *p1 = reinterpret_cast<float4 *>(a.ring.a[0] + row * 8), *p2 = reinterpret_cast<float4 *>(a.ring.a[1] + row * 8);
            p1[0] = make_float4(o1[0], o1[1], o1[2], o1[3]); p1[1] = make_float4(o1[4], o1[5], o1[6], o1[7]);
            p2[0] = make_float4(o[0], o[1], o[2], o[3]); p2[1] = make_float4(o[4], o[5], o[6], o[7]);
            a.ring.a[2][row] = act;
            a.ring.a[3][row] = rew;
            a.ring.a[4][row] = done_store;
        }
        if (a.act_out) a.act_out[i] = act;
        if (a.q_out) {
#pragma unroll
            for (int c = 0; c < ddrl_sel::MAXQ; ++c)
                if (c < a.A) a.q_out[i * a.A + c] = q[c];
        }
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);
            if (VER) { my_slot = *a.newest; a.slot[i] = my_slot; }   // train.py:251-252  weights = ps.pull(keys); agent.set_weights(keys, weights)
        }
        {
            float4 *p = reinterpret_cast<float4 *>(a.obs + i * 8);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
            if (a.next_obs_out) {
                float4 *qn = reinterpret_cast<float4 *>(a.next_obs_out + i * 8);
                qn[0] = p[0]; qn[1] = p[1];
            }
        }
        e.store(a.S, n, i);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        n_end += __shfl_xor(n_end, off);
        len_end += __shfl_xor(len_end, off);
        ret_end += __shfl_xor(ret_end, off);
    }
    if ((threadIdx.x & 63) == 0 && n_end > 0) {
        atomicAdd((unsigned long long *)&a.stats->episodes, (unsigned long long)n_end);
        atomicAdd((unsigned long long *)&a.stats->len_sum, (unsigned long long)len_end);
        atomicAdd(&a.stats->ret_sum, ret_end);
    }
    if constexpr (VER) {   // the grouping, the ring ticket and the next forward's workgroup table: the function k_env_step_pi calls
        ver_plan_tail(a.vp, my_slot, i, n, RingTicket{a.rs, a.ring, s_ptr, n});
        return;
    }
    // the last block to finish advances the ring cursor (every block has read rs->ptr before its ticket)
    __syncthreads();
    if (threadIdx.x == 0) (void)ddrl_replay_dev::ring_commit(a.rs, a.ring, s_ptr, n);
}

__global__ void __launch_bounds__(256) k_env_obs(float *S, long long n, uint32_t seed, float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.seed = seed; e.id = (uint32_t)i;
    e.load(S, n, i);
    float o[8];
    e.obs(o);
    float4 *p = reinterpret_cast<float4 *>(obs_out + i * 8);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
}

}  // namespace

// struct ddrl_env: env_handle.h (shared with eval3.hip, whose evaluation entry points own the handle's results block)

// the articulated model's launches (env3.hip)
int ddrl_env3_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream);
int ddrl_env3_launch_step(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d,
                          float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
// the walker's launches (walker.hip): [n,24] observations, [n,4] actions
int ddrl_walker_launch_reset(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream);
int ddrl_walker_launch_step(float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d, float *obs2_d,
                            float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
// ... and its wrapped step (walker_nstep.hip)
int ddrl_walker_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                                    float obs_noise, float reward_scale, int action_repeat, float *obs2_d, float *rew_d, float *done_d,
                                    float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);

// Memory contract (include/ddrl.h): the env family's kernels move an observation row as two float4 and a continuous action row as one
// float2, so caller pointers to [n,8] observations must be 16-byte aligned and to [n,2] actions 8-byte aligned.  Checked here, before
// any launch: a pointer off that grid is refused with its name in ddrl_last_error() and nothing is touched.  (NULL passes: optional.)
#define DDRL_REQUIRE_ALIGNED(p, bytes) \
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(p) & (uintptr_t)((bytes) - 1)) == 0, #p " must be " #bytes "-byte aligned")

// the entry points whose kernels hold the one-body model refuse an articulated handle before they touch anything
#define DDRL_ONE_BODY_ONLY(h, what)                                                                                                   \
    do {                                                                                                                              \
        DDRL_REFUSE_WALKER(h, what);                                                                                                  \
        if ((h)->kind != DDRL_ENV_ONE_BODY) {                                                                                         \
            ::ddrl::set_error("%s: not built for the articulated lander (DDRL_ENV_ARTICULATED); its kernel holds the one-body model — " \
                              "use ddrl_env_step / ddrl_env_step_discrete with the unfused act and store calls", what);                \
            return DDRL_ERR_UNSUPPORTED;                                                                                              \
        }                                                                                                                             \
    } while (0)

// the articulated pair (ddrl_rollout_begin_articulated / _step_articulated) refuses a one-body handle before it touches anything
#define DDRL_ARTICULATED_ONLY(h, what, instead)                                                                                       \
    do {                                                                                                                              \
        DDRL_REFUSE_WALKER(h, what);                                                                                                  \
        if ((h)->kind != DDRL_ENV_ARTICULATED) {                                                                                      \
            ::ddrl::set_error("%s: built for the articulated lander (DDRL_ENV_ARTICULATED); this handle holds the one-body model — " \
                              "use %s", what, instead);                                                                               \
            return DDRL_ERR_UNSUPPORTED;                                                                                              \
        }                                                                                                                             \
    } while (0)
// ---- what the fused rollout entry points below share on the host.  (The kernels are kept apart on purpose.)
// "A five-array float32 transition ring (obs1[8], obs2[8], acts[w], rews, done)": what a ring is not, for the caller to report in its own
// status and words.
enum RingFault { RING_FITS = 0, RING_ROW_SHAPE, RING_COMPACT };
static RingFault transition_ring_fault(const ddrl_replay_dev::RingPtrs &r, int w) {
    if (r.n_arr != 5 || r.w[0] != 8 || r.w[1] != 8 || r.w[2] != w || r.w[3] != 1 || r.w[4] != 1) return RING_ROW_SHAPE;
    return (r.kind[0] || r.kind[1]) ? RING_COMPACT : RING_FITS;
}
static const char *const RING_COMPACT_MSG = "the fused rollout step stores into float32 rings only (not a compact uint8 ring)";

// the observations of the envs' present state into the forward's rows (ddrl_rollout_begin, ddrl_rollout_begin_discrete)
static int launch_env_obs(ddrl_env_t *h, float *obs, void *stream) {
    ddrl::DeviceGuard g(h->device);
    k_env_obs<<<(unsigned)((h->n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->S, h->n, h->seed, obs);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

// The version store's side of ONE vector step of every fused loop, around `step(versioned, fused_plan)` — the entry point's own forward,
// argument patch and launch.  versioned: once no install has happened for `horizon` steps (max_ep_len, or the wrapped step's
// limit_steps) every env has been through an episode end and acts on the newest version — the plain launch on the handle's current
// weights is then the same computation.  fused_plan: the next forward's plan rides in this launch (base offsets of the row lists must
// fit the records' int).  Behind the launch plan_fresh says whether the launch's own tail has planned for the envs its episode ends
// moved to the newest version, or the next forward has to.
template <class Step>
static int rollout_versioned_step(const ddrl_version_view &ver, long long n, long long horizon, Step step) {
    const bool store = ver.n_slots > 0;
    const bool versioned = store && *ver.steps_since_install < horizon;
    const bool fused_plan = versioned && ver.vcnt != nullptr && ver.perm2d_off + (long long)ver.n_slots * n < (1ll << 31) && n / 32 <= 1024;
    if (store) *ver.steps_since_install += 1;
    if (const int rc = step(versioned, fused_plan)) return rc;
    if (versioned) *ver.plan_fresh = fused_plan;
    return DDRL_OK;
}
// ... and the plan's tables as the launch takes them: k_env_step_q as they stand, the other argument structs field by field
static VerPlan ver_plan_of(const ddrl_version_view &ver, bool fused_plan, int col_tiles) {
    return VerPlan{fused_plan ? ver.vcnt : nullptr, ver.perm, ver.perm2d_off, ver.vtiles, ver.vs, ver.n_slots, col_tiles, ver.wg_slots, ver.vt_cap};
}
template <class Args>
static void set_ver_plan(Args &a, const VerPlan &p) {
    a.vcnt = p.vcnt; a.perm = p.perm; a.perm2d_off = p.perm2d_off; a.vtiles = p.vtiles; a.vs = p.vs;
    a.n_slots = p.n_slots; a.col_tiles = p.col_tiles; a.wg_slots = p.wg_slots; a.vt_cap = p.vt_cap;
}

// the one-body continuous step's envelope: DDRL_ERR_BAD_ARG
static int rollout_check(ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_replay_dev::SamplerView &rv, int32_t n_steps) {
    DDRL_REQUIRE(v.ok, "actor has no direct-operand policy (shape outside the envelope): use ddrl_actor_act + ddrl_env_step + ddrl_replay_store");
    DDRL_REQUIRE(v.obs_dim == 8 && v.act <= 2 && h->n <= v.max_rows && h->n % 32 == 0 && v.device == h->device,
                 "actor / env mismatch (obs_dim 8, act_dim <= 2, n_envs a multiple of 32 within max_rows, same device)");
    const RingFault rf = transition_ring_fault(rv.ring, 2);
    DDRL_REQUIRE(rf != RING_ROW_SHAPE, "replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)");
    DDRL_REQUIRE(rf != RING_COMPACT, RING_COMPACT_MSG);
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(v.ver.n_slots == 0 || h->n == v.max_rows, "an actor with a version store steps exactly max_rows envs");
    return DDRL_OK;
}
// the articulated pair's envelope (rv: the step's ring): DDRL_ERR_UNSUPPORTED with the function's name
static int rollout3_check(const char *what, ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_replay_dev::SamplerView *rv) {
    const char *why = nullptr;
    if (!v.ok) why = "the actor has no direct-operand policy (shape outside the envelope)";
    else if (v.obs_dim != 8 || v.act > 2) why = "the actor must have obs_dim 8 and act_dim <= 2";
    else if (h->n % 32 != 0 || h->n > v.max_rows) why = "n_envs must be a multiple of 32 within the actor's max_rows";
    else if (v.ver.n_slots > 0 && h->n != v.max_rows) why = "an actor with a version store steps exactly max_rows envs";
    else if (v.device != h->device) why = "actor and envs must live on one device";
    else if (rv) {
        const RingFault rf = transition_ring_fault(rv->ring, 2);
        if (rf == RING_ROW_SHAPE) why = "the replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)";
        else if (rf == RING_COMPACT) why = RING_COMPACT_MSG;
        else if (rv->device != h->device) why = "the replay ring lives on another device than the envs";
    }
    if (!why) return DDRL_OK;
    ddrl::set_error("%s: %s; use ddrl_actor_act + ddrl_env_step + ddrl_replay_store", what, why);
    return DDRL_ERR_UNSUPPORTED;
}

// The continuous fused step behind ddrl_rollout_step (one-body lander: k_env_step_pi) and ddrl_rollout_step_articulated (rollout3.hip:
// k_env3_step_pi), behind the entry point's own envelope: n_steps times the loop body of worker_rollout — the forward, `launch(a)`, the
// host's bookkeeping.  `launch` issues the env-step kernel of the handle's model on a filled RolloutArgs.
template <class Launch>
static int rollout_step_loop(ddrl_env_t *h, ddrl_actor_t *actor, const ddrl_actor_rollout_view &v, ddrl_replay_t *replay,
                             const ddrl_replay_dev::SamplerView &rv, int32_t n_steps, uint32_t noise_seed, uint64_t noise_ctr,
                             int deterministic, float *act_out_d, float *next_obs_out_d, void *stream, Launch launch) {
    ddrl::DeviceGuard g(h->device);
    RolloutArgs a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.max_ep_len = (float)h->max_ep_len; a.stats = h->stats;
    a.obs = v.obs; a.hp = v.hp; a.act = v.act; a.nt2 = v.nt2; a.scale = v.scale;
    a.deterministic = deterministic; a.noise_seed = noise_seed; a.vstride = v.ver.vstride;
    a.rs = rv.state; a.ring = rv.ring; a.act_out = act_out_d; a.next_obs_out = next_obs_out_d;
    for (int k = 0; k < n_steps; ++k) {  // the loop body of worker_rollout, n_steps times with the weights the actor holds
        const int rc = rollout_versioned_step(v.ver, h->n, h->max_ep_len, [&](bool versioned, bool fused_plan) -> int {
            a.slot = versioned ? v.ver.slot : nullptr;
            a.newest = versioned ? &v.ver.vs->newest : nullptr;
            a.bmu = versioned ? v.vbmu : v.bmu; a.bls = versioned ? v.vbls : v.bls;
            set_ver_plan(a, ver_plan_of(v.ver, fused_plan, v.nt2));
            if (const int frc = ddrl_actor_internal_forward(actor, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = noise_ctr + (uint64_t)k * (uint64_t)h->n * (uint64_t)v.act;
            return launch(a);
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_store(replay, h->n);
    }
    return DDRL_OK;
}

// The discrete fused step behind ddrl_rollout_step_discrete (one-body lander: k_env_step_q) and ddrl_rollout_step_discrete_articulated
// (rollout3_q.hip: k_env3_step_q), behind the entry point's own envelope: n_steps times the loop body of worker_rollout_dqn — the
// pending repack, the forward, `launch(a, versioned)`, the host's bookkeeping.  `launch` issues the env-step kernel of the handle's model
// on a filled RolloutQArgs.
template <class Launch>
static int rollout_discrete_step_loop(ddrl_env_t *h, ddrl_dqn_t *dqn, const ddrl_dqn_rollout_view &v, ddrl_replay_t *replay,
                                      const ddrl_replay_dev::SamplerView &rv, int32_t n_steps, int mode, float greedy_prob, uint32_t seed,
                                      uint64_t ctr, float *act_out_d, float *q_out_d, float *next_obs_out_d, void *stream, Launch launch) {
    ddrl::DeviceGuard g(h->device);
    RolloutQArgs a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.max_ep_len = (float)h->max_ep_len; a.stats = h->stats;
    a.obs = v.obs; a.hp = v.hp; a.b_lo = v.b_lo; a.b_hi = v.b_hi; a.A = v.n_actions; a.half = v.half; a.nt2 = v.nt2; a.sqn = v.sqn;
    a.deterministic = mode == DDRL_ACT_DETERMINISTIC; a.greedy_prob = greedy_prob; a.alpha = v.alpha; a.noise_seed = seed;
    a.rs = rv.state; a.ring = rv.ring; a.act_out = act_out_d; a.q_out = q_out_d; a.next_obs_out = next_obs_out_d;
    for (int k = 0; k < n_steps; ++k) {   // ddrl_rollout_step's loop body
        // a learner step's pending repack is an install: before steps_since_install is read
        if (const int rc = ddrl_dqn_internal_repack(dqn, stream)) return rc;
        const int rc = rollout_versioned_step(v.ver, h->n, h->max_ep_len, [&](bool versioned, bool fused_plan) -> int {
            if (const int frc = ddrl_dqn_internal_forward(dqn, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = ctr + (uint64_t)k * 2ull * (uint64_t)h->n;
            if (versioned) {
                a.b_lo = v.vb_lo; a.b_hi = v.vb_hi; a.slot = v.ver.slot; a.newest = &v.ver.vs->newest; a.vstride = v.ver.vstride;
                a.vp = ver_plan_of(v.ver, fused_plan, v.nt2);
            } else {
                a.b_lo = v.b_lo; a.b_hi = v.b_hi;
            }
            return launch(a, versioned);
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_store(replay, h->n);
    }
    return DDRL_OK;
}

extern "C" {

int ddrl_env_create(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len) {
    return ddrl_env_create_ex(out, device, n_envs, seed, max_ep_len, nullptr);
}

int ddrl_env_create_ex(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len, const ddrl_env_model_t *model) {
    DDRL_REQUIRE(out != nullptr && n_envs > 0 && max_ep_len > 0, "bad out/n_envs/max_ep_len");
    DDRL_REQUIRE(max_ep_len < (1 << 24), "max_ep_len must stay exact in float32");
    const int kind = model ? model->kind : DDRL_ENV_ONE_BODY;
    DDRL_REQUIRE(kind == DDRL_ENV_ONE_BODY || kind == DDRL_ENV_ARTICULATED || kind == DDRL_ENV_WALKER,
                 "model kind must be DDRL_ENV_ONE_BODY, DDRL_ENV_ARTICULATED or DDRL_ENV_WALKER");
    DDRL_REQUIRE(kind == DDRL_ENV_ONE_BODY || (model->velocity_iterations >= 1 && model->position_iterations >= 1),
                 "the articulated model and the walker need velocity_iterations >= 1 and position_iterations >= 1");
    const int NF = kind == DDRL_ENV_WALKER ? DDRL_ENVW_STATE_FIELDS : kind == DDRL_ENV_ARTICULATED ? DDRL_ENV3_STATE_FIELDS : DDRL_ENV_STATE_FIELDS;
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_env *h = new ddrl_env();
    h->device = device; h->n = n_envs; h->seed = seed; h->max_ep_len = max_ep_len; h->S = nullptr; h->stats = nullptr;
    h->kind = kind; h->fields = NF;
    h->vit = kind != DDRL_ENV_ONE_BODY ? model->velocity_iterations : 0;
    h->pit = kind != DDRL_ENV_ONE_BODY ? model->position_iterations : 0;
    if (hipMalloc((void **)&h->S, (size_t)NF * n_envs * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&h->stats, sizeof(EnvStats)) != hipSuccess) {
        ddrl::set_error("hipMalloc failed for %lld envs", (long long)n_envs);
        ddrl_env_destroy(h);
        return DDRL_ERR_NOMEM;
    }
    DDRL_HIP_CHECK(hipMemset(h->S, 0, (size_t)NF * n_envs * sizeof(float)));
    DDRL_HIP_CHECK(hipMemset(h->stats, 0, sizeof(EnvStats)));
    if (kind == DDRL_ENV_WALKER) {
        if (const int rc = ddrl_walker_launch_reset(h->S, h->n, h->seed, h->vit, h->pit, nullptr, nullptr, nullptr)) return rc;
    } else if (kind == DDRL_ENV_ARTICULATED) {
        if (const int rc = ddrl_env3_launch_reset(h->S, h->n, h->seed, h->vit, h->pit, nullptr, nullptr, nullptr)) return rc;
    } else {
        k_env_reset<<<(unsigned)((n_envs + 255) / 256), 256, 0, nullptr>>>(h->S, h->n, h->seed, nullptr, nullptr);
        DDRL_LAUNCH_CHECK();
    }
    DDRL_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = h;
    return DDRL_OK;
}

int ddrl_env_destroy(ddrl_env_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    (void)hipFree(h->S); (void)hipFree(h->stats);
    (void)hipFree(h->ev_block); (void)hipFree(h->ev_w);   // the evaluation results block and weight staging (eval3.hip)
    (void)hipFree(h->ro_block);                           // the articulated discrete rollout step's mirrors
    delete h;
    return DDRL_OK;
}

int ddrl_env_reset(ddrl_env_t *h, const uint8_t *mask_d, float *obs_d, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE_ALIGNED(obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    if (h->kind == DDRL_ENV_WALKER) return ddrl_walker_launch_reset(h->S, h->n, h->seed, h->vit, h->pit, mask_d, obs_d, stream);
    if (h->kind == DDRL_ENV_ARTICULATED) return ddrl_env3_launch_reset(h->S, h->n, h->seed, h->vit, h->pit, mask_d, obs_d, stream);
    k_env_reset<<<(unsigned)((h->n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->S, h->n, h->seed, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_env_step(ddrl_env_t *h, const float *act_d, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d,
                  uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, "NULL handle or action pointer");
    DDRL_REQUIRE_ALIGNED(act_d, 8);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    if (h->kind == DDRL_ENV_WALKER) {   // an [n,4] action row moves as one float4
        DDRL_REQUIRE_ALIGNED(act_d, 16);
        return ddrl_walker_launch_step(h->S, h->n, h->seed, h->max_ep_len, h->vit, h->pit, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d,
                                       h->stats, stream);
    }
    if (h->kind == DDRL_ENV_ARTICULATED)
        return ddrl_env3_launch_step(0, h->S, h->n, h->seed, h->max_ep_len, h->vit, h->pit, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d,
                                     h->stats, stream);
    k_env_step<false><<<(unsigned)((h->n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(
        h->S, h->n, h->seed, (float)h->max_ep_len, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d, h->stats);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_env_step_discrete(ddrl_env_t *h, const float *act_idx_d, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d,
                           uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_idx_d != nullptr, "NULL handle or action pointer");
    DDRL_REFUSE_WALKER(h, "ddrl_env_step_discrete");
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    if (h->kind == DDRL_ENV_ARTICULATED)
        return ddrl_env3_launch_step(1, h->S, h->n, h->seed, h->max_ep_len, h->vit, h->pit, act_idx_d, obs2_d, rew_d, done_d, next_obs_d,
                                     ended_d, h->stats, stream);
    k_env_step<true><<<(unsigned)((h->n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(
        h->S, h->n, h->seed, (float)h->max_ep_len, act_idx_d, obs2_d, rew_d, done_d, next_obs_d, ended_d, h->stats);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_env_step_wrapped(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale, int32_t action_repeat,
                          int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d,
                          void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, "NULL pointer");
    DDRL_ONE_BODY_ONLY(h, "ddrl_env_step_wrapped");
    DDRL_REQUIRE_ALIGNED(act_d, 8);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    DDRL_REQUIRE(action_repeat >= 1 && limit_steps >= 1, "action_repeat and limit_steps must be >= 1");
    ddrl::DeviceGuard g(h->device);
    k_env_step_wrapped<<<(unsigned)((h->n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(
        h->S, h->n, h->seed, (float)limit_steps, act_d, act_noise, obs_noise, reward_scale, action_repeat, obs2_d, rew_d, done_d, next_obs_d,
        ended_d, h->stats);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

// ... on the articulated lander (kernel: rollout3_nstep.hip, k_env3_step_wrapped); the iteration counts are the handle's
int ddrl_env_step_wrapped_articulated(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale,
                                      int32_t action_repeat, int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d,
                                      float *next_obs_d, uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, "NULL pointer");
    DDRL_ARTICULATED_ONLY(h, "ddrl_env_step_wrapped_articulated", "ddrl_env_step_wrapped");
    DDRL_REQUIRE_ALIGNED(act_d, 8);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    DDRL_REQUIRE(action_repeat >= 1 && limit_steps >= 1, "action_repeat and limit_steps must be >= 1");
    ddrl::DeviceGuard g(h->device);
    return ddrl_env3_launch_step_wrapped(h->S, h->n, h->seed, limit_steps, h->vit, h->pit, act_d, act_noise, obs_noise, reward_scale,
                                         action_repeat, obs2_d, rew_d, done_d, next_obs_d, ended_d, h->stats, stream);
}

// ... on the walker (kernel: walker_nstep.hip, k_walker_step_wrapped): [n,4] actions as one float4, [n,24] observations as six
int ddrl_env_step_wrapped_walker(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale, int32_t action_repeat,
                                 int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d,
                                 void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, "ddrl_env_step_wrapped_walker: NULL handle or act_d");
    if (h->kind != DDRL_ENV_WALKER) {
        ::ddrl::set_error("ddrl_env_step_wrapped_walker: built for the walker (DDRL_ENV_WALKER); this handle holds %s — use %s",
                          h->kind == DDRL_ENV_ARTICULATED ? "the articulated lander" : "the one-body model",
                          h->kind == DDRL_ENV_ARTICULATED ? "ddrl_env_step_wrapped_articulated" : "ddrl_env_step_wrapped");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE_ALIGNED(act_d, 16);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    DDRL_REQUIRE(action_repeat >= 1 && limit_steps >= 1, "ddrl_env_step_wrapped_walker: action_repeat and limit_steps must be >= 1");
    ddrl::DeviceGuard g(h->device);
    return ddrl_walker_launch_step_wrapped(h->S, h->n, h->seed, limit_steps, h->vit, h->pit, act_d, act_noise, obs_noise, reward_scale,
                                           action_repeat, obs2_d, rew_d, done_d, next_obs_d, ended_d, h->stats, stream);
}

int ddrl_rollout_begin(ddrl_env_t *h, ddrl_actor_t *actor, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_begin");
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    DDRL_REQUIRE(v.ok, "actor has no direct-operand policy (shape outside the envelope): use ddrl_actor_act + ddrl_env_step + ddrl_replay_store");
    DDRL_REQUIRE(v.obs_dim == 8 && h->n <= v.max_rows && v.device == h->device, "actor / env mismatch (obs_dim 8, max_rows >= n_envs, same device)");
    return launch_env_obs(h, v.obs, stream);
}

int ddrl_rollout_step(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_replay_t *replay, int32_t n_steps, uint32_t noise_seed, uint64_t noise_ctr,
                      int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && replay != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_step");
    DDRL_REQUIRE_ALIGNED(act_out_d, 8);
    DDRL_REQUIRE_ALIGNED(next_obs_out_d, 16);
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    if (const int rc = rollout_check(h, v, rv, n_steps)) return rc;
    return rollout_step_loop(h, actor, v, replay, rv, n_steps, noise_seed, noise_ctr, deterministic, act_out_d, next_obs_out_d, stream,
                             [&](const RolloutArgs &a) -> int {
                                 // one wave per workgroup: 4096 envs spread over 64 CUs instead of 16 (the kernel is a chain of dependent latencies)
                                 if (a.act <= 2) k_env_step_pi<4><<<(unsigned)((h->n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(a);
                                 else k_env_step_pi<8><<<(unsigned)((h->n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(a);
                                 DDRL_LAUNCH_CHECK();
                                 return DDRL_OK;
                             });
}

// ---- the same pair on the articulated lander (kernels: rollout3.hip)
int ddrl_rollout_begin_articulated(ddrl_env_t *h, ddrl_actor_t *actor, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_begin_articulated", "ddrl_rollout_begin");
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    if (const int rc = rollout3_check("ddrl_rollout_begin_articulated", h, v, nullptr)) return rc;
    ddrl::DeviceGuard g(h->device);
    return ddrl_rollout3_launch_obs(h->S, h->n, v.obs, stream);
}

int ddrl_rollout_step_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_replay_t *replay, int32_t n_steps, uint32_t noise_seed,
                                  uint64_t noise_ctr, int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && replay != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_step_articulated", "ddrl_rollout_step");
    DDRL_REQUIRE_ALIGNED(act_out_d, 8);
    DDRL_REQUIRE_ALIGNED(next_obs_out_d, 16);
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    if (const int rc = rollout3_check("ddrl_rollout_step_articulated", h, v, &rv)) return rc;
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    return rollout_step_loop(h, actor, v, replay, rv, n_steps, noise_seed, noise_ctr, deterministic, act_out_d, next_obs_out_d, stream,
                             [&](const RolloutArgs &a) -> int { return ddrl_rollout3_launch_step(&a, h->vit, h->pit, stream); });
}

// the discrete fused step's envelope: 0, or the status with the reason in ddrl_last_error()
static int rollout_discrete_check(ddrl_env_t *h, const ddrl_dqn_rollout_view &v) {
    if (!v.ok) {
        ddrl::set_error("fused discrete rollout step: %s; use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store", v.why ? v.why : "no acting forward");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (v.obs_dim != 8 || v.n_actions > ddrl_sel::MAXQ || h->n % 32 != 0 || h->n > v.batch) {
        ddrl::set_error("fused discrete rollout step needs obs_dim 8, n_actions <= 8 and n_envs a multiple of 32 within the handle's batch "
                        "(obs_dim %d, n_actions %d, n_envs %lld, batch %d); use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store",
                        v.obs_dim, v.n_actions, h->n, v.batch);
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(v.device == h->device, "the learner / actor handle lives on another device than the envs");
    return DDRL_OK;
}

int ddrl_rollout_begin_discrete(ddrl_env_t *h, ddrl_dqn_t *dqn, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_begin_discrete");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout_discrete_check(h, v)) return rc;
    return launch_env_obs(h, v.obs, stream);
}

int ddrl_rollout_step_discrete(ddrl_env_t *h, ddrl_dqn_t *dqn, ddrl_replay_t *replay, int32_t n_steps, int mode, float greedy_prob,
                               uint32_t seed, uint64_t ctr, float *act_out_d, float *q_out_d, float *next_obs_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr && replay != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_step_discrete");
    DDRL_REQUIRE_ALIGNED(next_obs_out_d, 16);
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout_discrete_check(h, v)) return rc;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    DDRL_REQUIRE(rv.device == h->device, "the replay ring lives on another device than the envs");
    const RingFault rf = transition_ring_fault(rv.ring, 1);
    DDRL_REQUIRE(rf != RING_ROW_SHAPE, "replay row shape must be (obs1[8], obs2[8], acts, rews, done)");
    DDRL_REQUIRE(rf != RING_COMPACT, RING_COMPACT_MSG);
    if (v.ver.n_slots > 0 && h->n != v.rows) {
        ddrl::set_error("fused discrete rollout step: a handle with a version store steps exactly the acting forward's %lld rows (n_envs %lld)", v.rows, h->n);
        return DDRL_ERR_BAD_ARG;
    }
    const unsigned grid = (unsigned)((h->n + 63) / 64);
    hipStream_t s = ddrl::as_stream(stream);
    return rollout_discrete_step_loop(h, dqn, v, replay, rv, n_steps, mode, greedy_prob, seed, ctr, act_out_d, q_out_d, next_obs_out_d, stream,
                                      [&](const RolloutQArgs &a, bool versioned) -> int {
                                          if (versioned) {
                                              if (v.n_actions <= 4) k_env_step_q<4, true><<<grid, 64, 0, s>>>(a);
                                              else k_env_step_q<8, true><<<grid, 64, 0, s>>>(a);
                                          } else {
                                              if (v.n_actions <= 4) k_env_step_q<4, false><<<grid, 64, 0, s>>>(a);
                                              else k_env_step_q<8, false><<<grid, 64, 0, s>>>(a);
                                          }
                                          DDRL_LAUNCH_CHECK();
                                          return DDRL_OK;
                                      });
}

// ---- the same pair on the articulated lander (kernel: rollout3_q.hip).  Handles only: the step's mirrors are a block the env handle
// owns (env_handle.h), allocated by the first begin call that passes the envelope and handed out by ddrl_env_rollout_mirrors.
// The envelope (rv: the step's ring): DDRL_ERR_UNSUPPORTED with the function's name
static int rollout3_discrete_check(const char *what, ddrl_env_t *h, const ddrl_dqn_rollout_view &v, const ddrl_replay_dev::SamplerView *rv) {
    const char *why = nullptr;
    if (!v.ok) why = v.why ? v.why : "no acting forward";
    else if (v.obs_dim != 8 || v.n_actions > ddrl_sel::MAXQ) why = "the handle must have obs_dim 8 and n_actions <= 8";
    else if (h->n % 32 != 0 || h->n > v.batch) why = "n_envs must be a multiple of 32 within the handle's batch";
    else if (v.ver.n_slots > 0 && h->n != v.rows) why = "a handle with a version store steps exactly the acting forward's rows";
    else if (v.device != h->device) why = "the learner / actor handle lives on another device than the envs";
    else if (rv) {
        const RingFault rf = transition_ring_fault(rv->ring, 1);
        if (rf == RING_ROW_SHAPE) why = "the replay row shape must be (obs1[8], obs2[8], acts, rews, done)";
        else if (rf == RING_COMPACT) why = RING_COMPACT_MSG;
        else if (rv->device != h->device) why = "the replay ring lives on another device than the envs";
    }
    if (!why) return DDRL_OK;
    ddrl::set_error("%s: %s; use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store", what, why);
    return DDRL_ERR_UNSUPPORTED;
}

int ddrl_rollout_begin_discrete_articulated(ddrl_env_t *h, ddrl_dqn_t *dqn, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_begin_discrete_articulated", "ddrl_rollout_begin_discrete");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout3_discrete_check("ddrl_rollout_begin_discrete_articulated", h, v, nullptr)) return rc;
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const size_t n = (size_t)h->n;
    if (!h->ro_block) {   // the first begin call inside the envelope: the mirror block, zeroed
        float *p = nullptr;
        if (hipMalloc((void **)&p, n * (8 + DDRL_ROLLOUT_MIRROR_Q + 1) * sizeof(float)) != hipSuccess) {
            ddrl::set_error("ddrl_rollout_begin_discrete_articulated: hipMalloc failed for the mirrors of %lld envs", h->n);
            return DDRL_ERR_NOMEM;
        }
        DDRL_HIP_CHECK(hipMemsetAsync(p, 0, n * (8 + DDRL_ROLLOUT_MIRROR_Q + 1) * sizeof(float), s));
        h->ro_block = p;
    }
    h->ro_actions = v.n_actions;
    // the envs' current observations into the forward's rows and into the next-observation mirror: what the next step acts on
    if (const int rc = ddrl_rollout3_launch_obs(h->S, h->n, v.obs, stream)) return rc;
    DDRL_HIP_CHECK(hipMemcpyAsync(h->ro_block, v.obs, n * 8 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DDRL_OK;
}

int ddrl_rollout_step_discrete_articulated(ddrl_env_t *h, ddrl_dqn_t *dqn, ddrl_replay_t *replay, int32_t n_steps, int mode,
                                           float greedy_prob, uint32_t seed, uint64_t ctr, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr && replay != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_step_discrete_articulated", "ddrl_rollout_step_discrete");
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    if (const int rc = rollout3_discrete_check("ddrl_rollout_step_discrete_articulated", h, v, &rv)) return rc;
    DDRL_REQUIRE(h->ro_block != nullptr, "ddrl_rollout_step_discrete_articulated: no ddrl_rollout_begin_discrete_articulated on this env handle yet");
    h->ro_actions = v.n_actions;
    const long long n = h->n;
    float *next_obs = h->ro_block, *q = next_obs + n * 8, *act = q + n * DDRL_ROLLOUT_MIRROR_Q;
    return rollout_discrete_step_loop(h, dqn, v, replay, rv, n_steps, mode, greedy_prob, seed, ctr, act, q, next_obs, stream,
                                      [&](const RolloutQArgs &a, bool versioned) -> int {
                                          return ddrl_rollout3_launch_step_q(&a, versioned ? 1 : 0, h->vit, h->pit, stream);
                                      });
}

int ddrl_env_rollout_mirrors(ddrl_env_t *h, const float **act, const float **q, const float **next_obs, int32_t *n_envs, int32_t *n_actions) {
    DDRL_REQUIRE(h != nullptr, "ddrl_env_rollout_mirrors: handle is NULL");
    DDRL_REFUSE_WALKER(h, "ddrl_env_rollout_mirrors");
    DDRL_REQUIRE(h->ro_block != nullptr, "ddrl_env_rollout_mirrors: no ddrl_rollout_begin_discrete_articulated on this env handle yet");
    const float *b = h->ro_block;
    if (next_obs) *next_obs = b;
    if (q) *q = b + h->n * 8;
    if (act) *act = b + h->n * (8 + DDRL_ROLLOUT_MIRROR_Q);
    if (n_envs) *n_envs = (int32_t)h->n;
    if (n_actions) *n_actions = h->ro_actions;
    return DDRL_OK;
}

// the fused n-step step's envelope (kernel: rollout_nstep.hip): 0, or the status with the reason in ddrl_last_error().  Nothing is
// launched or written before it has passed.
static int rollout_nstep_check(ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_winq_view &q) {
    if (h->n % 32 != 0) {   // (first: an actor for such a row count has no direct-operand policy either, which says less)
        ddrl::set_error("fused n-step rollout step needs n_envs a multiple of 32 (n_envs %lld); use the unfused calls", h->n);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (!v.ok) {
        ddrl::set_error("fused n-step rollout step: the actor has no direct-operand policy (shape outside the envelope); use "
                        "ddrl_actor_act + ddrl_env_step_wrapped + ddrl_winq_push + ddrl_replay_store_masked_ex");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (v.obs_dim != 8 || v.act != 2 || h->n % 32 != 0 || h->n > v.max_rows || (v.ver.n_slots > 0 && h->n != v.max_rows)) {
        ddrl::set_error("fused n-step rollout step needs obs_dim 8, act_dim 2 and n_envs a multiple of 32 within the actor's max_rows (all of "
                        "them with a version store): obs_dim %d, act_dim %d, n_envs %lld, max_rows %lld", v.obs_dim, v.act, h->n, v.max_rows);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (q.n != h->n || q.obs != 8 || q.act != 2) {
        ddrl::set_error("fused n-step rollout step: the window queues hold %lld envs of obs_dim %d, act_dim %d; the envs are %lld of 8 and 2",
                        q.n, q.obs, q.act, h->n);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (q.Ln > DDRL_NSTEP_FUSED_MAX_LN) {
        ddrl::set_error("fused n-step rollout step: Ln %d is above DDRL_NSTEP_FUSED_MAX_LN (%d: the workgroup's windows are staged in LDS); use "
                        "the unfused calls", q.Ln, DDRL_NSTEP_FUSED_MAX_LN);
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(v.device == h->device && q.device == h->device, "actor, window queues and envs must live on one device");
    return DDRL_OK;
}
static int rollout_nstep_ring_check(ddrl_env_t *h, const ddrl_winq_view &q, const ddrl_replay_dev::SamplerView &rv) {
    const ddrl_replay_dev::RingPtrs &r = rv.ring;
    if (r.n_arr != 4) {
        ddrl::set_error("fused n-step rollout step stores into a four-array window ring {o, a, r, d}; this ring has %d arrays", r.n_arr);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (r.kind[0] || r.kind[1] || r.kind[2] || r.kind[3]) {
        ddrl::set_error("fused n-step rollout step stores into float32 rings only (not a compact uint8 ring)");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (r.w[0] != (q.Ln + 1) * 8 || r.w[1] != q.Ln * 2 || r.w[2] != q.Ln || r.w[3] != q.Ln) {
        ddrl::set_error("fused n-step rollout step: the ring's rows {%d, %d, %d, %d} are not the queues' windows {(Ln+1)*8, Ln*2, Ln, Ln} at Ln %d",
                        r.w[0], r.w[1], r.w[2], r.w[3], q.Ln);
        return DDRL_ERR_UNSUPPORTED;
    }
    const unsigned long long al_o = reinterpret_cast<unsigned long long>(r.a[0]) | reinterpret_cast<unsigned long long>(q.o);
    const unsigned long long al_a = reinterpret_cast<unsigned long long>(r.a[1]) | reinterpret_cast<unsigned long long>(q.a);
    if (r.capacity >= (1ll << 31) || (al_o & 15ull) || (al_a & 7ull)) {
        ddrl::set_error("fused n-step rollout step: ring capacity must be below 2^31 and the window arrays vector-aligned");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(rv.device == h->device, "the window ring lives on another device than the envs");
    return DDRL_OK;
}

// ---- what the two n-step pairs (one-body: rollout_nstep.hip; articulated: rollout3_nstep.hip) share behind their own kind test:
// the begin call — envelope, then the observation rows and the readiness bytes from the queues (no env state is read) ...
static int rollout_nstep_begin(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_winq_view q = ddrl_winq_internal_view(winq);
    if (const int rc = rollout_nstep_check(h, v, q)) return rc;
    ddrl::DeviceGuard g(h->device);
    return ddrl_nstep_launch_begin(q.o, h->n, q.Ln, v.obs, q.t, q.save_freq, q.rdy[*q.parity], stream);
}
// ... and the step driver: argument checks, envelope, then n_steps times the loop body of worker_rollout — the versioned / plain
// forward choice, the env-step kernel of the handle's model on the filled NStepLaunch, the parity flip
static int rollout_nstep_step_loop(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                                   float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                                   int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr,
                                   const ddrl_rollout_nstep_out_t *out, void *stream) {
    DDRL_REQUIRE(n_steps >= 1 && action_repeat >= 1 && limit_steps >= 1, "n_steps, action_repeat and limit_steps must be >= 1");
    if (out) {
        DDRL_REQUIRE_ALIGNED(out->act, 8);
        DDRL_REQUIRE_ALIGNED(out->obs2, 16);
        DDRL_REQUIRE_ALIGNED(out->next_obs, 16);
    }
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_winq_view q = ddrl_winq_internal_view(winq);
    if (const int rc = rollout_nstep_check(h, v, q)) return rc;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(window_ring);
    if (const int rc = rollout_nstep_ring_check(h, q, rv)) return rc;
    ddrl::DeviceGuard g(h->device);
    NStepLaunch a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.stats = h->stats;
    a.limit_steps = (float)limit_steps; a.act_noise = act_noise; a.obs_noise = obs_noise; a.reward_scale = reward_scale;
    a.repeat = action_repeat; a.adopt = adopt_at_episode_end ? 1 : 0;
    a.obs = v.obs; a.hp = v.hp; a.nt2 = v.nt2; a.scale = v.scale; a.noise_seed = noise_seed;
    const bool store = v.ver.n_slots > 0;
    a.slot = store ? v.ver.slot : nullptr;
    a.newest = store ? &v.ver.vs->newest : nullptr;
    a.vstride = v.ver.vstride;
    a.qo = q.o; a.qa = q.a; a.qr = q.r; a.qd = q.d; a.qt = q.t; a.Ln = q.Ln; a.save_freq = q.save_freq;
    a.rs = rv.state; a.ring = rv.ring;
    if (out) {
        a.act_out = out->act; a.obs2_out = out->obs2; a.rew_out = out->rew; a.done_out = out->done; a.next_obs_out = out->next_obs;
        a.ended_out = out->ended;
    }
    for (int k = 0; k < n_steps; ++k) {   // the loop body of worker_rollout, n_steps times with the weights the actor holds
        // the horizon is the wrapped step's limit (ddrl_actor_act_versioned makes the same test)
        const int rc = rollout_versioned_step(v.ver, h->n, limit_steps, [&](bool versioned, bool fused_plan) -> int {
            a.versioned = versioned ? 1 : 0;
            a.bmu = versioned ? v.vbmu : v.bmu; a.bls = versioned ? v.vbls : v.bls;
            set_ver_plan(a, ver_plan_of(v.ver, fused_plan, v.nt2));
            if (const int frc = ddrl_actor_internal_forward(actor, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = noise_ctr + (uint64_t)k * (uint64_t)h->n * 2ull;
            a.rdy_in = q.rdy[*q.parity]; a.rdy_out = q.rdy[1 - *q.parity];
            const int lrc = h->kind == DDRL_ENV_ARTICULATED ? ddrl_nstep3_launch_step(a, h->vit, h->pit, stream) : ddrl_nstep_launch_step(a, stream);
            if (lrc) return lrc;
            *q.parity = 1 - *q.parity;
            if (!versioned && store && a.adopt) *v.ver.plan_fresh = false;   // an unplanned launch moved envs: the next forward plans
            return DDRL_OK;
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_masked_store(window_ring);   // the row count is known on the device only
    }
    return DDRL_OK;
}

int ddrl_rollout_begin_nstep(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_begin_nstep");
    return rollout_nstep_begin(h, actor, winq, stream);
}

int ddrl_rollout_step_nstep(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                            float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                            int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr, const ddrl_rollout_nstep_out_t *out,
                            void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr && window_ring != nullptr, "NULL handle");
    DDRL_ONE_BODY_ONLY(h, "ddrl_rollout_step_nstep");
    return rollout_nstep_step_loop(h, actor, winq, window_ring, n_steps, act_noise, obs_noise, reward_scale, action_repeat, limit_steps,
                                   adopt_at_episode_end, noise_seed, noise_ctr, out, stream);
}

// ---- the same pair on the articulated lander (kernel: rollout3_nstep.hip): only the kind test is its own: the envelope, the begin
// launch (it reads the queues only) and the step driver, which launches the kernel of the handle's model, are the one-body pair's
int ddrl_rollout_begin_nstep_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_begin_nstep_articulated", "ddrl_rollout_begin_nstep");
    return rollout_nstep_begin(h, actor, winq, stream);
}

int ddrl_rollout_step_nstep_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                                        float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                                        int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr,
                                        const ddrl_rollout_nstep_out_t *out, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr && window_ring != nullptr, "NULL handle");
    DDRL_ARTICULATED_ONLY(h, "ddrl_rollout_step_nstep_articulated", "ddrl_rollout_step_nstep");
    return rollout_nstep_step_loop(h, actor, winq, window_ring, n_steps, act_noise, obs_noise, reward_scale, action_repeat, limit_steps,
                                   adopt_at_episode_end, noise_seed, noise_ctr, out, stream);
}

int ddrl_env_stats(ddrl_env_t *h, int64_t *episodes_h, double *ret_sum_h, int64_t *len_sum_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    EnvStats st;
    DDRL_HIP_CHECK(hipMemcpyAsync(&st, h->stats, sizeof(st), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipMemsetAsync(h->stats, 0, sizeof(EnvStats), s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    if (episodes_h) *episodes_h = st.episodes;
    if (ret_sum_h) *ret_sum_h = st.ret_sum;
    if (len_sum_h) *len_sum_h = st.len_sum;
    return DDRL_OK;
}

int ddrl_env_state_fields(ddrl_env_t *h) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    return h->fields;
}

int ddrl_env_get_state(ddrl_env_t *h, float *state_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && state_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    DDRL_HIP_CHECK(hipMemcpyAsync(state_d, h->S, (size_t)h->fields * h->n * sizeof(float), hipMemcpyDeviceToDevice, ddrl::as_stream(stream)));
    return DDRL_OK;
}

int ddrl_env_set_state(ddrl_env_t *h, const float *state_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && state_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    DDRL_HIP_CHECK(hipMemcpyAsync(h->S, state_d, (size_t)h->fields * h->n * sizeof(float), hipMemcpyDeviceToDevice, ddrl::as_stream(stream)));
    return DDRL_OK;
}

}  // extern "C"
