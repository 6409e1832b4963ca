// Fused DISCRETE rollout step on the ARTICULATED lander (ddrl_rollout_begin_discrete_articulated / ddrl_rollout_step_discrete_articulated):
// k_env_step_q's (lander.hip) vector step of worker_rollout_dqn's policy phase (algos/dqn/train.py:253-274) with Env3's solver
// (env3_device.h) in the middle, as k_env3_step_pi (rollout3.hip) is k_env_step_pi's —
//   a = agent.get_action(o)      the Q-head partials of the forward launch in front of this kernel summed in column-tile order, plus the
//                                head bias of the env's own version slot (ddrl_sel::q_row_from_partials), two uniforms of the counter
//                                generator per env, ddrl_sel::select_row, ddrl_sel::lander_action: k_env_step_q's statements in its
//                                order, so the same partials give the same row and the same index
//   o2, r, d, _ = env.step(a)    Env3::physics and the worker's bookkeeping as k_env3_step (env3.hip) does it
//   replay_buffer.store(o, a, r, o2, d)   ring row (ptr + i) % capacity of a (obs1[8], obs2[8], acts, rews, done) ring, env order; the
//                                last workgroup to finish advances the cursor
//   o = o2 (or env.reset()), and at an episode end weights = ps.pull(keys): slot[i] = *newest (train.py:249-252)
// and the next versioned forward's plan (ver_plan_tail, version_plan.h).
// The phases are ordered for the register file, as rollout3.hip's header explains: the solver alone fills it (k_env3_step: 256 VGPRs
// and AGPRs as spill space, no scratch), so everything of the policy phase — the Q row, the uniforms, o1 — is consumed BEFORE the env
// state is loaded: the ring row is known before the step, so o1 and the action index go to the ring, and the index and the Q row to
// the mirrors, first; only i, the ring row, the slot and a0 / a1 cross physics(); o2, r and d are written behind it.
// profiles/lander3_discrete_rollout_resource_usage.txt holds the compiler's report for the four instantiations (no scratch).
// The three mirrors (the last step's action indices [n], Q rows [n][A], next observations [n][8]) are the env handle's own block
// (env_handle.h) and always written: 52 B per env beside a 66-field state load and store.
// A translation unit of its own, as env3.hip and rollout3.hip: every other kernel compiles exactly as before.
#include "ddrl_common.h"
#include "env3_device.h"
#include "dqn_select.h"
#include "rollout_args.h"
#include "env_launch.h"

namespace {

struct Rollout3QArgs {
    RolloutQArgs r;
    int vit, pit;
};

// NH: head partial rows fetched per env, 4 (n_actions <= 4) or 8.  VER: a version store is live (as k_env_step_q's).
template <int NH, bool VER>
__global__ void __launch_bounds__(64) k_env3_step_q(Rollout3QArgs k) {
    const RolloutQArgs &a = k.r;
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = a.rs->ptr;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    long long n_end = 0, len_end = 0;
    double ret_end = 0.0;
    int my_slot = 0;       // the version this env acts on: at this step in front of the episode end, at the NEXT step behind it
    if (i < n) {
        // ---- policy phase: get_action, the mirrors of it, and the half of the stored row that is known before the step
        const long long cap = a.ring.capacity;
        const bool keep = i >= n - cap;   // rows that a later store of the same batch would overwrite are skipped (n > capacity)
        const long long row = keep ? (s_ptr + i) % cap : 0;
        float a0, a1;
        {
            float q[ddrl_sel::MAXQ];
            if (VER) my_slot = a.slot[i];
            ddrl_sel::q_row_from_partials<NH>(a.hp, n, i, a.A, a.half, a.nt2, a.b_lo, a.b_hi, VER ? (long long)my_slot * a.vstride : 0ll, q);
            const float4 *p = reinterpret_cast<const float4 *>(a.obs + i * 8);
            const float4 u = p[0], v = p[1];
            const float u0 = ddrl_sel::uniform_at(a.noise_seed, a.noise_ctr + 2ull * (unsigned long long)i);
            const float u1 = ddrl_sel::uniform_at(a.noise_seed, a.noise_ctr + 2ull * (unsigned long long)i + 1ull);
            const float act = (float)ddrl_sel::select_row(q, a.A, a.sqn, a.deterministic, a.greedy_prob, a.alpha, u0, u1);
            ddrl_sel::lander_action(act, a0, a1);
            if (keep) {
                float4 *p1 = reinterpret_cast<float4 *>(a.ring.a[0] + row * 8);
                p1[0] = u; p1[1] = v;
                a.ring.a[2][row] = act;
            }
            a.act_out[i] = act;
#pragma unroll
            for (int c = 0; c < ddrl_sel::MAXQ; ++c)
                if (c < a.A) a.q_out[i * a.A + c] = q[c];
        }
        // ---- env.step + the worker's bookkeeping (as k_env3_step)
        Env3 e;
        e.seed = a.seed; e.id = (uint32_t)i; e.vit = k.vit; e.pit = k.pit;
        e.load(a.S, n, i);
        float o[8];
        bool done_env;
        const float rew = e.physics(a0, a1, done_env, o);
        e.eplen = e.eplen + 1.0f;
        e.epret = e.epret + rew;
        const bool limit = e.eplen >= a.max_ep_len;
        const float done_store = limit ? 0.0f : (done_env ? 1.0f : 0.0f);
        const bool ended = done_env || limit;
        // ---- the rest of replay_buffer.store(o, a, r, o2, d)
        if (keep) {
            float4 *p2 = reinterpret_cast<float4 *>(a.ring.a[1] + row * 8);
            p2[0] = make_float4(o[0], o[1], o[2], o[3]); p2[1] = make_float4(o[4], o[5], o[6], o[7]);
            a.ring.a[3][row] = rew;
            a.ring.a[4][row] = done_store;
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
            float4 *qn = reinterpret_cast<float4 *>(a.next_obs_out + i * 8);
            qn[0] = p[0]; qn[1] = p[1];
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
    // As in k_env_step_q, and for the reason given in version_plan.h, no __threadfence() in front of either tail.
    if constexpr (VER) {   // the grouping, the ring ticket and the next forward's workgroup table
        ver_plan_tail(a.vp, my_slot, i, n, RingTicket{a.rs, a.ring, s_ptr, n});
        return;
    }
    // the last block to finish advances the ring cursor (every block has read rs->ptr before its ticket)
    __syncthreads();
    if (threadIdx.x == 0) (void)ddrl_replay_dev::ring_commit(a.rs, a.ring, s_ptr, n);
}

}  // namespace

// ---- internal (env.hip: ddrl_rollout_step_discrete_articulated) -----------------------------------------------------------------------
int ddrl_rollout3_launch_step_q(const void *args, int versioned, int vit, int pit, void *stream) {
    const Rollout3QArgs k{*static_cast<const RolloutQArgs *>(args), vit, pit};
    // one wave per workgroup, as k_env3_step: the sweeps are one serial chain per env
    const unsigned grid = (unsigned)((k.r.n + 63) / 64);
    hipStream_t s = ddrl::as_stream(stream);
    if (versioned) {
        if (k.r.A <= 4) k_env3_step_q<4, true><<<grid, 64, 0, s>>>(k);
        else k_env3_step_q<8, true><<<grid, 64, 0, s>>>(k);
    } else {
        if (k.r.A <= 4) k_env3_step_q<4, false><<<grid, 64, 0, s>>>(k);
        else k_env3_step_q<8, false><<<grid, 64, 0, s>>>(k);
    }
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}
