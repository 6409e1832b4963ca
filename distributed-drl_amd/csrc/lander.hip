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
#include "policy_row.h"
#include "replay_device.h"
#include "env_device.h"
#include "dqn_select.h"
#include "version_plan.h"
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

// ---- internal (env.hip: the ddrl_env_* and ddrl_rollout_* entry points of a one-body handle) --------------------------------------
// (The kernel templates are instantiated below in the order env.hip's entry points used to name them — k_env_step<false> before <true>,
// k_env_step_q<., true> before <., false> — which is the order they stand in the code object.)
#include "env_launch.h"

int ddrl_lander_launch_reset(float *S, long long n, uint32_t seed, int, int, const uint8_t *mask_d, float *obs_d, void *stream) {
    k_env_reset<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(S, n, seed, mask_d, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_lander_launch_step(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int, int, const float *act_d, float *obs2_d,
                            float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    EnvStats *st = reinterpret_cast<EnvStats *>(stats_d);
    if (!discrete)
        k_env_step<false><<<grid, 256, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, act_d, obs2_d, rew_d, done_d, next_obs_d,
                                                                     ended_d, st);
    else
        k_env_step<true><<<grid, 256, 0, ddrl::as_stream(stream)>>>(S, n, seed, (float)max_ep_len, act_d, obs2_d, rew_d, done_d, next_obs_d,
                                                                    ended_d, st);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_lander_launch_step_wrapped(float *S, long long n, uint32_t seed, int limit_steps, int, int, float *act_d, float act_noise,
                                    float obs_noise, float reward_scale, int repeat, float *obs2_d, float *rew_d, float *done_d,
                                    float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream) {
    k_env_step_wrapped<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(
        S, n, seed, (float)limit_steps, act_d, act_noise, obs_noise, reward_scale, repeat, obs2_d, rew_d, done_d, next_obs_d, ended_d,
        reinterpret_cast<EnvStats *>(stats_d));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_lander_launch_obs(float *S, long long n, uint32_t seed, float *obs_d, void *stream) {
    k_env_obs<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(S, n, seed, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_lander_launch_step_pi(const void *args, int, int, void *stream) {
    const RolloutArgs &a = *static_cast<const RolloutArgs *>(args);
    // one wave per workgroup: 4096 envs spread over 64 CUs instead of 16 (the kernel is a chain of dependent latencies)
    if (a.act <= 2) k_env_step_pi<4><<<(unsigned)((a.n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(a);
    else k_env_step_pi<8><<<(unsigned)((a.n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(a);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_lander_launch_step_q(const void *args, int versioned, int, int, void *stream) {
    const RolloutQArgs &a = *static_cast<const RolloutQArgs *>(args);
    const unsigned grid = (unsigned)((a.n + 63) / 64);
    hipStream_t s = ddrl::as_stream(stream);
    if (versioned) {
        if (a.A <= 4) k_env_step_q<4, true><<<grid, 64, 0, s>>>(a);
        else k_env_step_q<8, true><<<grid, 64, 0, s>>>(a);
    } else {
        if (a.A <= 4) k_env_step_q<4, false><<<grid, 64, 0, s>>>(a);
        else k_env_step_q<8, false><<<grid, 64, 0, s>>>(a);
    }
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
