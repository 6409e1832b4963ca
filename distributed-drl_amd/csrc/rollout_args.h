// What the continuous fused rollout step's two kernels share: k_env_step_pi (lander.hip, the one-body lander) and k_env3_step_pi
// (rollout3.hip, the articulated lander) take the same arguments, finish get_action from the forward's head partials by the same
// statements and pass the same ring ticket to ver_plan_tail (version_plan.h) — and what the DISCRETE step's two kernels share likewise:
// k_env_step_q (lander.hip) and k_env3_step_q (rollout3_q.hip) take one RolloutQArgs and the same ticket.  Internal linkage throughout, as env_device.h: each
// translation unit compiles its own copy, and lander.hip's kernels compile to the code they compiled to with the two structs in the file.
#pragma once
#include "ddrl_common.h"
#include "policy_row.h"
#include "replay_device.h"
#include "env_device.h"
#include "version_plan.h"

namespace {

// The ring ticket of a fused launch in the form ver_plan_tail (version_plan.h) calls it: the cursor state, the ring and the two numbers BY
// COPY.  (A lambda that captures the kernel's argument struct by reference does the same thing, and changed the scalar address arithmetic
// the compiler emits for EVERY kernel of this file, the untouched ones included.)
struct RingTicket {
    ddrl_replay_dev::RingState *rs;
    ddrl_replay_dev::RingPtrs ring;
    long long ptr, n;
    __device__ bool operator()() const { return ddrl_replay_dev::ring_commit(rs, ring, ptr, n); }
};
struct RolloutArgs {
    float *S;
    long long n;
    uint32_t seed;
    float max_ep_len;
    EnvStats *stats;
    // policy
    float *obs;            // [n][obs_dim] in / out (actor's buffer)
    const float *hp;       // [8][n][16]
    const float *bmu, *bls;
    int act, nt2;
    float scale;
    int deterministic;
    uint32_t noise_seed;
    unsigned long long noise_ctr;
    // version store of the actor (nullable): env i acts on slot[i] (bmu / bls are slot 0's then, slot s is vstride floats further)
    // and adopts the newest version where its episode ends — the reference worker's pull at episode end (example/dsac.py:127-130)
    int *slot;
    const int *newest;
    long long vstride;
    // ... and the NEXT forward's plan, written by this launch (nullable: vcnt): every env counts itself into its slot's group and files
    // itself in that group's row list; the last workgroup to finish turns the counts into the forward's workgroup table (what
    // k_version_plan does as a launch of its own, 7-11 us between this launch and the forward that waits for it)
    int *vcnt;             // [VER_MAX_SLOTS], zero on entry, zero again on exit
    int *perm;             // row lists: group s at perm[perm2d_off + s * n ..)
    long long perm2d_off;
    VerTile *vtiles;
    VerState *vs;
    int n_slots, col_tiles, wg_slots, vt_cap;
    // replay ring
    ddrl_replay_dev::RingState *rs;
    ddrl_replay_dev::RingPtrs ring;
    // optional mirrors for the host-side objects
    float *act_out, *next_obs_out;
};

// The DISCRETE fused rollout step's arguments: k_env_step_q (lander.hip, the one-body lander) and k_env3_step_q (rollout3_q.hip, the
// articulated lander) take the same struct, as the continuous pair takes RolloutArgs.
struct RolloutQArgs {
    float *S;
    long long n;
    uint32_t seed;
    float max_ep_len;
    EnvStats *stats;
    float *obs;            // [n][8] in / out (the forward's buffer)
    const float *hp;       // [8][n][16]
    const float *b_lo, *b_hi;
    int A, half, nt2, sqn, deterministic;
    float greedy_prob, alpha;
    uint32_t noise_seed;
    unsigned long long noise_ctr;
    ddrl_replay_dev::RingState *rs;
    ddrl_replay_dev::RingPtrs ring;
    float *act_out, *q_out, *next_obs_out;   // mirrors: [n], [n][A], [n][8] (k_env_step_q: each optional; k_env3_step_q: the env handle's block)
    // version store of the acting forward (k_env_step_q<.., true> only; behind everything the plain kernel reads): env i acts on slot[i]
    // (b_lo / b_hi are slot 0's then, slot s is vstride floats further) and adopts the newest version where its episode ends — the
    // reference worker's pull at the episode boundary (algos/dqn/train.py:249-252) — and the NEXT forward's plan (vp.vcnt nullable)
    int *slot;
    const int *newest;
    long long vstride;
    VerPlan vp;
};

// get_action's last step for env i, in two halves so that a kernel can issue its other loads between them: k_env_step_pi's own
// statements in k_env_step_pi's order, so that the same partials give the same action.  (k_env_step_pi keeps them inline: calling
// these two functions there changed that kernel's register allocation, and lander.hip's kernels are to compile as they did.)
// head_load: the forward launch's head partials (mu heads 0..act-1, log_std heads act..2act-1), NA = 2 (act_dim <= 2) or 4 action
// columns.  (Two statically indexed register arrays: one array indexed by `c + act` would live in scratch memory.)
template <int NA>
struct HeadPartials {
    float4 hm[NA][4], hl[NA][4];
};
template <int NA>
__device__ __forceinline__ void head_load(const RolloutArgs &a, long long i, HeadPartials<NA> &h) {
    const long long n = a.n;
    const int nq = (a.nt2 + 3) >> 2;  // float4 groups of a partial row that hold tiles
#pragma unroll
    for (int c = 0; c < NA; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cm = c < a.act ? c : 0, qq = q < nq ? q : 0;
            h.hm[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)cm * n + i) * 16 + 4 * qq);
            h.hl[c][q] = *reinterpret_cast<const float4 *>(a.hp + ((long long)(a.act + cm) * n + i) * 16 + 4 * qq);
        }
}
// head_action: the partials summed in n-tile order, the head bias of the env's own version slot, ddrl_pol::policy_row on element
// i * act + c of the counter stream (tanh(mu) when deterministic); the second component is 0 for act_dim 1
template <int NA>
__device__ __forceinline__ float2 head_action(const RolloutArgs &a, long long i, const HeadPartials<NA> &h) {
    const int nq = (a.nt2 + 3) >> 2;
    float mu[4], ls[4], ev[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float sm = 0.f, sl = 0.f;
        if (c < NA) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < nq) {  // n-tile order; slots beyond nt2 hold 0
                    const float4 m4 = h.hm[c < NA ? c : 0][q], l4 = h.hl[c < NA ? c : 0][q];
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
    return make_float2(a0, a1);
}

}  // namespace

// (The launch functions that take these structs as bytes: env_launch.h.)
