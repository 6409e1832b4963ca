// Fused rollout step on the ARTICULATED lander (ddrl_rollout_begin_articulated / ddrl_rollout_step_articulated): k_env_step_pi's
// (lander.hip) vector step of worker_rollout's policy phase (example/dsac.py:96-130) with Env3's solver (env3_device.h) in the middle —
//   a = agent.get_action(o)      the forward launch's head partials, summed in column-tile order, plus the head bias of the env's own
//                                version slot, through ddrl_pol::policy_row: head_load / head_action (rollout_args.h),
//                                k_env_step_pi's statements in its order, so the same partials give the same action
//   o2, r, d, _ = env.step(a)    Env3::physics and the worker's bookkeeping as k_env3_step (env3.hip) does it
//   replay_buffer.store(o, a, r, o2, d)   ring row (ptr + i) % capacity, env order; the last workgroup to finish advances the cursor
//   o = o2 (or env.reset()), and at an episode end weights = ps.pull(keys): slot[i] = *newest
// and the next versioned forward's plan (ver_plan_tail, version_plan.h).
// The solver already fills the register file (k_env3_step: 256 VGPRs and AGPRs as spill space, no scratch), so the phases are ordered
// for it: everything of the policy phase is consumed BEFORE the env state is loaded — the ring row is known before the step, so o1 and
// the action go to the ring and to the act mirror first — and only i, the row, the slot and the step's outputs cross physics();
// o2, r and d are written behind it.  profiles/lander3_rollout_resource_usage.txt holds the compiler's report (no scratch, no spill).
// A translation unit of its own, as env3.hip: lander.hip's and env3.hip's kernels compile exactly as before.
#include "ddrl_common.h"
#include "env3_device.h"
#include "rollout_args.h"
#include "env_launch.h"

namespace {

struct Rollout3Args {
    RolloutArgs r;
    int vit, pit;
};

__global__ void __launch_bounds__(64) k_env3_step_pi(Rollout3Args k) {
    const RolloutArgs &a = k.r;
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = a.rs->ptr;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;       // the version this env acts on at the NEXT step
    if (i < n) {
        // ---- policy phase: get_action, and the half of the stored row that is known before the step
        const long long cap = a.ring.capacity;
        const bool keep = i >= n - cap;   // rows that a later store of the same batch would overwrite are skipped (n > capacity)
        const long long row = keep ? (s_ptr + i) % cap : 0;
        float a0, a1;
        {
            HeadPartials<2> hd;
            head_load<2>(a, i, hd);
            const float4 *p = reinterpret_cast<const float4 *>(a.obs + i * 8);
            const float4 u = p[0], v = p[1];
            const float2 pa = head_action<2>(a, i, hd);
            a0 = pa.x; a1 = pa.y;
            if (keep) {
                float4 *p1 = reinterpret_cast<float4 *>(a.ring.a[0] + row * 8);
                p1[0] = u; p1[1] = v;
                *reinterpret_cast<float2 *>(a.ring.a[2] + row * 2) = pa;
            }
            if (a.act_out) *reinterpret_cast<float2 *>(a.act_out + i * 2) = pa;
        }
        // ---- env.step + the worker's bookkeeping (as k_env3_step)
        Env3 e;
        e.seed = a.seed; e.id = (uint32_t)i; e.vit = k.vit; e.pit = k.pit;
        e.load(a.S, n, i);
        float o[8];
        bool done_env;
        const float rew = e.physics(a0, a1, done_env, o);
        e.eplen = e.eplen + 1.0f;                       // example/dsac.py:104
        e.epret = e.epret + rew;                        // :103
        const bool limit = e.eplen >= a.max_ep_len;
        const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);  // :109
        const bool ended = done_env || limit;                              // :118
        // ---- the rest of replay_buffer.store(o, a, r, o2, d): ring arrays {obs1, obs2, acts, rews, done}
        if (keep) {
            float4 *p2 = reinterpret_cast<float4 *>(a.ring.a[1] + row * 8);
            p2[0] = make_float4(o[0], o[1], o[2], o[3]); p2[1] = make_float4(o[4], o[5], o[6], o[7]);
            a.ring.a[3][row] = rew;
            a.ring.a[4][row] = done_store;
        }
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
    // episode statistics: wave reduction, one atomic per wave that saw an episode end (a lane with i >= n brings zeros)
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
    // cursor (every block has read rs->ptr before its ticket) — and, in that last workgroup, the forward's workgroup table.  As in
    // k_env_step_pi, and for the reason given in version_plan.h, no __threadfence() in front of it.
    const VerPlan vp{a.vcnt, a.perm, a.perm2d_off, a.vtiles, a.vs, a.n_slots, a.col_tiles, a.wg_slots, a.vt_cap};
    ver_plan_tail(vp, my_slot, i, n, RingTicket{a.rs, a.ring, s_ptr, n});
}

// the articulated counterpart of k_env_obs: the observation of every env's state as it stands
__global__ void __launch_bounds__(256) k_env3_obs(const float *S, long long n, float *obs_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Env3 e;   // (Env3::obs reads the hull origin, the hull's velocities and angle and the two contact flags)
    e.px = S[PX * n + i]; e.py = S[PY * n + i];
    e.hull.vx = S[VX * n + i]; e.hull.vy = S[VY * n + i]; e.hull.ang = S[ANG * n + i]; e.hull.om = S[OM * n + i];
    e.c1 = S[C1 * n + i]; e.c2 = S[C2 * n + i];
    float o[8];
    e.obs(o);
    float4 *p = reinterpret_cast<float4 *>(obs_out + i * 8);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
}

}  // namespace

// ---- internal (env.hip: ddrl_rollout_begin_articulated / ddrl_rollout_step_articulated) -----------------------------------------
int ddrl_rollout3_launch_step(const void *args, int vit, int pit, void *stream) {
    const Rollout3Args k{*static_cast<const RolloutArgs *>(args), vit, pit};
    // one wave per workgroup, as k_env3_step: the sweeps are one serial chain per env
    k_env3_step_pi<<<(unsigned)((k.r.n + 63) / 64), 64, 0, ddrl::as_stream(stream)>>>(k);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_rollout3_launch_obs(const float *S, long long n, float *obs_d, void *stream) {
    k_env3_obs<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(S, n, obs_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
