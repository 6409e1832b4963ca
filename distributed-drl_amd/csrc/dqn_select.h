// Row-local action selection of the discrete actors, shared by the selection kernel of ddrl_dqn_act (dqn.hip) and the fused
// discrete rollout step (lander.hip: k_env_step_q), so that the two paths cannot drift:
//   Double-DQN  algos/dqn/actor_learner.py:194-201   argmax q with probability greedy_prob, a uniform random action otherwise
//   SQN         algos/sqn/core.py:30-42              argmax of / one draw from softmax(q1 / alpha) (tf.random.multinomial there, an
//                                                    inverse CDF in float32 on the counter generator's uniform here)
// plus what dqn.hip shows of a learner handle to env.hip (internal to libddrl_hip.so).
#pragma once
#include "ddrl_common.h"
#include "policy_row.h"

namespace ddrl_sel {

constexpr int MAXQ = 8;   // n_actions of the acting forward: the DFH = 8 head rows of k_actor_fwd

// element c of ddrl_uniform_fill(lo = 0, hi = 1, seed, counter 0): identical integer arithmetic in oracle/noise_oracle.py
__device__ __forceinline__ float uniform_at(uint32_t seed, unsigned long long c) {
    return ddrl::u01(ddrl::hash3(seed, (uint32_t)c, 2u * (uint32_t)(c >> 32)));
}

// One row.  q[c] for c < A (A <= M; the array is indexed with unrolled constants only: it stays in registers).  M = MAXQ on the acting
// forward's partials, 16 (the head kernel's limit) where ddrl_dqn_act selects on the generic head's Q image.
//   deterministic            first index of the row maximum (np.argmax)
//   Double-DQN (!sqn)        u0 < greedy_prob: first index of the maximum; else min((int)floorf(u1 * A), A - 1)
//   SQN sampling             p_k = expf((q_k - max q) / alpha); cumulative sums in index order, total = the last of them;
//                            the smallest k with u0 * total < cum_k, the last index when none is
template <int M>
__device__ __forceinline__ int select_row(const float (&q)[M], int A, int sqn, int deterministic, float greedy_prob, float alpha,
                                          float u0, float u1) {
    int best = 0;
    float bv = q[0];
#pragma unroll
    for (int c = 1; c < M; ++c)
        if (c < A && q[c] > bv) { bv = q[c]; best = c; }
    if (deterministic) return best;
    if (!sqn) {
        if (u0 < greedy_prob) return best;
        const int r = (int)floorf(u1 * (float)A);
        return r < A - 1 ? r : A - 1;
    }
    float cum[M], run = 0.f;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        if (c < A) run = run + expf((q[c] - bv) / alpha);
        cum[c] = run;
    }
    const float t = u0 * run;
    int pick = A - 1;
#pragma unroll
    for (int c = M - 1; c >= 0; --c)
        if (c < A && t < cum[c]) pick = c;
    return pick;
}

// The Q row of env / observation row i out of the head partials of a k_actor_fwd launch over n rows ([8][n][16]: head c = action c,
// one slot per 32-wide column tile of layer 2, slots beyond nt2 hold 0).  Summation order, on which the oracle check of the acting
// path rests: inside a partial as k_actor_fwd states it (layer-2 K blocks in order inside a wave, waves 0..3 in the combine, bias +
// relu, the tile's columns 0..31 in the head dot), then the partials in column-tile order, then the head bias.
// NH = head rows fetched: 4 (n_actions <= 4) or 8.  All loads are issued before the first sum.
// boff: where this row's head biases lie behind b_lo / b_hi — 0, or slot * vstride with a version store (b_lo / b_hi are slot 0's then).
template <int NH>
__device__ __forceinline__ void q_row_from_partials(const float *__restrict__ hp, long long n, long long i, int A, int half, int nt2,
                                                    const float *__restrict__ b_lo, const float *__restrict__ b_hi, long long boff,
                                                    float (&q)[MAXQ]) {
    const int nq = (nt2 + 3) >> 2;   // float4 groups of a partial row that hold tiles
    float4 v[NH][4];
    float b[NH];
#pragma unroll
    for (int c = 0; c < NH; ++c) {
        const int cm = c < A ? c : 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) v[c][g] = *reinterpret_cast<const float4 *>(hp + ((long long)cm * n + i) * 16 + 4 * (g < nq ? g : 0));
        b[c] = cm < half ? b_lo[boff + cm] : b_hi[boff + cm - half];
    }
#pragma unroll
    for (int c = 0; c < MAXQ; ++c) {
        float s = 0.f;
        if (c < NH) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g < nq) { const float4 x = v[c < NH ? c : 0][g]; s += x.x; s += x.y; s += x.z; s += x.w; }
            s = s + b[c < NH ? c : 0];
        }
        q[c] = c < A ? s : 0.f;
    }
}

// gym's discrete LunarLander-v2 action table on the continuous lander's clip rules (oracle/env_oracle.py:125-144):
// 0 noop (0, 0), 1 left engine (0, -1), 2 main engine (1, 0), 3 right engine (0, +1); the index is (int)value clamped to [0, 3]
__device__ __forceinline__ void lander_action(float act_idx, float &a0, float &a1) {
    int k = (int)act_idx;
    k = k < 0 ? 0 : (k > 3 ? 3 : k);
    a0 = k == 2 ? 1.0f : 0.0f;
    a1 = k == 1 ? -1.0f : (k == 3 ? 1.0f : 0.0f);
}

}  // namespace ddrl_sel

// What the fused discrete rollout step (env.hip) needs from a learner / actor handle of dqn.hip.
struct ddrl_dqn_rollout_view {
    int ok, device;         // ok = 0: the handle has no acting forward (`why` says what keeps the shape outside the envelope)
    const char *why;
    float *obs;             // [rows][8]: the observations the next forward launch acts on
    const float *hp;        // head partials of the last forward launch [8][n][16]: head c = action c
    const float *b_lo, *b_hi;   // head biases: action c < half at b_lo[c], the others at b_hi[c - half]
    int obs_dim, n_actions, half, nt2, batch, sqn;
    float alpha;
    // version store of the acting forward (ddrl_dqn_versions_enable): the inner actor's, and the head biases of slot 0 of its slab
    long long rows;         // rows of the acting forward: a store steps exactly that many envs
    ddrl_version_view ver;
    const float *vb_lo, *vb_hi;
};
ddrl_dqn_rollout_view ddrl_dqn_internal_view(ddrl_dqn_t *h);
// a learner step moved the parameters: the operand copy is packed again — with a version store that is an install,
// so the fused step calls this before it asks the store whether the step is versioned (ddrl_actor_internal_step_begin)
int ddrl_dqn_internal_repack(ddrl_dqn_t *h, void *stream);
// the acting forward of rows [0, n) of the view's observation buffer (repacks first, like the above); versioned: every env against the
// version in its slot (ddrl_actor_internal_forward)
int ddrl_dqn_internal_forward(ddrl_dqn_t *h, long long n, void *stream, int versioned);
