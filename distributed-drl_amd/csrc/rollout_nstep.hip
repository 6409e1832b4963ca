// Fused n-step rollout step (RolloutDeviceNStep._step_once = num_envs iterations of worker_rollout of the n-step driver,
// algos/sac1/sac_ray.py:208-262, in the policy phase), the sibling of k_env_step_pi / k_env_step_q (lander.hip) for the window-queue worker.
// Behind the actor's forward launch, ONE kernel does per env, in this order, what the unfused sequence does in seven launches:
//   a.  a = agent.get_action(o)       head partials summed in n-tile order + the bias of the env's version slot, counter-hash noise,
//                                     ddrl_pol::policy_row (k_actor_finish of actor.hip; the head of k_env_step_pi)
//   b.  o2, r, d = Wrapper.step(a)    k_env_step_wrapped of lander.hip, statement for statement (hyperparams.py:122-134, sac_ray.py:212-221)
//   c.  the queues                    k_winq_push of winq.hip: the o / a / r / d windows slide by one and take (o2, noisy a, r, d);
//                                     ready = t >= Ln && t % save_freq == 0; t += 1 (sac_ray.py:229-248)
//   d.  replay_buffer.store(queues)   ready envs: the window becomes ring row (ptr + rank) % capacity, rank = ready envs of smaller index
//                                     (k_mask_scan + k_store_masked of replay.hip, skip rule included); the last workgroup commits the cursor
//   e.  episode end                   stats, epi += 1, reset, reset-observation noise, k_winq_begin (o[Ln] = next_obs, t = 1) and, if
//                                     adopt_at_episode_end, slot[i] = newest (sac_ray.py:199-207, 252-262)
//   f.  o = next_obs                  into the actor's forward buffer and the mirrors; ver_plan_tail writes the next versioned forward's plan
//
// THE RANK ACROSS WORKGROUPS, WITHOUT WAITING.  An env's readiness depends only on its t_queue BEFORE the launch, but this launch rewrites
// t_queue, so readiness is read from bytes the launch does not write: the queue handle holds two uint8 arrays rdy[2].  The launch of
// parity p reads rdy[p] (written by the previous launch, or by ddrl_rollout_begin_nstep from t_queue) and writes rdy[1 - p] with the NEXT
// step's readiness (from the t it has just computed); the host flips the parity per launch.  Every workgroup counts the bytes of the
// envs in front of it (its base rank) and all of them (the total, for the skip rule and the cursor) itself: n bytes out of L2, sixteen
// per lane and pass.  No scan launch, no look-back, no spin: nothing in this kernel waits on another workgroup.  As in k_env_step_pi,
// only two things cross workgroups inside the launch: the ring ticket and the version counts (ver_plan_tail) — hence no __threadfence().
//
// One wave per workgroup (the physics is a chain of dependent latencies: 4096 envs spread over 64 CUs).  The window traffic — at Ln = 8,
// 104 floats slid and 104 stored per env — is done by the wave together: the 64 envs' rows are contiguous in every queue array, so the
// wave reads them in whole vectors into LDS already shifted (every global read happens before the barrier, every write after it: no
// read-after-write hazard between lanes), adds the new entries, copies ready rows to the ring, patches in the episode starts and
// writes the block back, all coalesced.  One LDS buffer serves the four arrays in turn.
#include "ddrl_common.h"
#include "policy_row.h"
#include "replay_device.h"
#include "env_device.h"
#include "version_plan.h"
#include "rollout_nstep.h"
#include "rollout_nstep_device.h"
#include "env_launch.h"

namespace {

constexpr uint32_t RESET_NOISE_STREAM = 0xFFFFFFEFu;   // as lander.hip: the Wrapper's reset-observation noise (hyperparams.py:119-121)
// (NStepTicket, slide_store and the env-agnostic phases: rollout_nstep_device.h, shared with k_env3_step_nstep of rollout3_nstep.hip)
__global__ void __launch_bounds__(64) k_env_step_nstep(NStepLaunch a) {
    extern __shared__ float4 s_win[];            // 64 x (Ln + 1) x 2 float4
    __shared__ long long s_ptr;
    __shared__ long long s_row[64];
    const int lane = threadIdx.x;
    if (lane == 0) s_ptr = a.rs->ptr;
    const long long n = a.n, i0 = (long long)blockIdx.x * 64, i = i0 + lane;
    const bool valid = i < n;
    const int ne = (int)(n - i0 < 64 ? n - i0 : 64);
    // ---- the readiness ranking (nothing in this launch writes the bytes it reads): the ring row of every ready env
    int base = 0, total = 0;
    DDRL_NSTEP_READY_ROWS(a, n, i0, i, valid, lane, s_ptr, s_row, base, total)
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;
    float o2[8], o[8];
    float a0 = 0.f, a1 = 0.f, rew = 0.f;
    bool done_env = false, ended = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) { o2[j] = 0.f; o[j] = 0.f; }
    if (valid) {
        // ---- a. the policy head (k_env_step_pi<4>'s: act_dim 2)
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
        Env e;
        e.seed = a.seed; e.id = (uint32_t)i;
        e.load(a.S, n, i);
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
        // ---- b. Wrapper.step + the rollout's episode bookkeeping (k_env_step_wrapped)
        const uint32_t st0 = (uint32_t)e.pstep;
        a0 = pr.act[0] + a.act_noise * (-2.0f * e.rng(st0, 2) + 1.0f);    // hyperparams.py:124
        a1 = pr.act[1] + a.act_noise * (-2.0f * e.rng(st0, 3) + 1.0f);
        float r = 0.0f;
        bool noisy = true;
        for (int k = 0; k < a.repeat; ++k) {                                 // :126-133
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
        ended = done_env || e.eplen >= a.limit_steps;                        // :252
#pragma unroll
        for (int j = 0; j < 8; ++j) o2[j] = o[j];
        // ---- e. episode end
        if (ended) {
            n_end = 1; len_end = (long long)e.eplen; ret_end = (double)e.epret;
            e.epi = e.epi + 1.0f;
            e.reset(o);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = o[j] + a.obs_noise * (-2.0f * e.rng(RESET_NOISE_STREAM, j) + 1.0f);  // hyperparams.py:119-121
            if (a.slot && a.adopt) a.slot[i] = *a.newest;                    // sac_ray.py:259-262
        }
        if (a.vcnt) my_slot = (ended && a.adopt) ? *a.newest : cur_slot;
        e.store(a.S, n, i);
        nstep_queue_tick(a, i, ended);                                       // ---- c. t_queue, and the NEXT step's readiness
        DDRL_NSTEP_MIRRORS(a, i, o, o2, a0, a1, rew, done_env, ended)        // ---- f. the next observation and the mirrors
    }
    // ---- c. + d. the windows: slide, append, store the ready rows, start the ended envs' queues anew
    nstep_windows(a, i0, ne, s_win, s_row, lane, valid, o2, o, a0, a1, rew, done_env, ended);
    // the statistics, the next forward's plan and the ring ticket
    DDRL_NSTEP_FINISH(a, n, i, lane, n_end, len_end, ret_end, my_slot, s_ptr, total)
}

// ddrl_rollout_begin_nstep: the observation every env's worker holds (the newest entry of its o_queue) into the forward's buffer, and the
// readiness bytes of the first fused launch from t_queue
__global__ void __launch_bounds__(256) k_nstep_begin(const float *__restrict__ qo, long long n, int Ln, float *__restrict__ obs, const int *__restrict__ t,
                                                     int save_freq, uint8_t *__restrict__ rdy) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 *src = reinterpret_cast<const float4 *>(qo + (i * (Ln + 1) + Ln) * 8);
    float4 *dst = reinterpret_cast<float4 *>(obs + i * 8);
    dst[0] = src[0]; dst[1] = src[1];
    const int ti = t[i];
    rdy[i] = (ti >= Ln && ti % save_freq == 0) ? 1 : 0;
}

}  // namespace

int ddrl_nstep_launch_step(const NStepLaunch &a, void *stream) {
    const size_t lds = (size_t)64 * (a.Ln + 1) * 8 * sizeof(float);
    k_env_step_nstep<<<(unsigned)((a.n + 63) / 64), 64, lds, ddrl::as_stream(stream)>>>(a);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_nstep_launch_begin(const float *qo, long long n, int Ln, float *obs_d, const int *t_queue, int save_freq, uint8_t *rdy_d, void *stream) {
    k_nstep_begin<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(qo, n, Ln, obs_d, t_queue, save_freq, rdy_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
