// The kernel bodies of the evaluation episodes, as templates over the env type: k_eval_episodes (the continuous policy; header text
// in eval.hip) and k_eval_episodes_q (the DQN / SQN Q network; header text in eval_q.hip).  E = Env (env_device.h, the one-body lander)
// is instantiated in eval.hip / eval_q.hip, E = Env3 (env3_device.h, the articulated lander) in eval3.hip: a translation unit of its
// own, as env3.hip and rollout3.hip, so that the one-body instantiations compile as they did with the bodies in their files.
// The decomposition is the same for both: one workgroup per episode, nothing crosses workgroups; the policy / Q row in its stated
// summation order on all 256 threads; then ONE lane runs E::physics plus the bookkeeping of k_env_step / k_env3_step (eplen, epret,
// ended = done_env || eplen >= max_ep_len) with the env state in registers.  The episode loop's only exit is the block-uniform
// s_ended flag, and eplen counts every step: the loop ends after at most max_ep_len steps whatever the actions are.
// Written for -ffp-contract=off; write no fmaf here.  Internal linkage throughout, as env_device.h.
#pragma once
#include "ddrl_common.h"
#include "policy_row.h"
#include "env_device.h"
#include "dqn_select.h"

namespace {

struct EvalArgs {
    const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wls, *bls;   // the flat external-order policy vector (act_dim 2, obs_dim 8)
    double *ret;        // [n] sum of the float32 step rewards in step order, accumulated in float64 (the host loop's `ep_ret += r`)
    int *len;           // [n]
    float *trace;       // nullable [n][max_ep_len][12]: obs[8] acted on, act[2], rew, ended; rows past the end are zero
    int h1, h2, max_ep_len;
    float scale, eps0;  // eps0 = 0: the noise element of a deterministic action (a kernel argument: the row math is not folded around it)
    uint32_t seed, first;
    int vit, pit;       // the articulated model's iteration counts (Env3 only; behind everything the one-body kernel reads)
};

constexpr int EV_ROW = 12;

// the model's run-time parameters: an env type with iteration counts (Env3) takes them, the one-body Env has none
template <class E>
__device__ __forceinline__ auto eval_set_model(E &e, int vit, int pit, int) -> decltype(e.vit, void()) { e.vit = vit; e.pit = pit; }
template <class E>
__device__ __forceinline__ void eval_set_model(E &, int, int, long) {}

template <class E, int NJ>   // NJ = ceil(h2 / 64): column chunks of one lane
__global__ void __launch_bounds__(256) k_eval_episodes(EvalArgs a) {
    __shared__ float xs[8];
    __shared__ float h1s[512];
    __shared__ float ps[16][512];
    __shared__ float v2[512];
    __shared__ float wh[4][512];   // head kernels by output: mu 0, mu 1, log_std 0, log_std 1
    __shared__ float part[32][4];
    __shared__ int s_ended;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h1 = a.h1, h2 = a.h2;
    const int per = (h1 + 15) >> 4, ng = (h2 + 15) >> 4;
    // operands that stay in registers for the whole episode: this thread's two layer-1 units, their biases, its two layer-2 biases
    const int j0 = tid < h1 ? tid : 0, j1 = tid + 256 < h1 ? tid + 256 : 0;
    float u0[8], u1[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { u0[q] = a.W1[(long long)q * h1 + j0]; u1[q] = a.W1[(long long)q * h1 + j1]; }
    const float b1a = a.b1[j0], b1b = a.b1[j1];
    const float b2a = a.b2[tid < h2 ? tid : 0], b2b = a.b2[tid + 256 < h2 ? tid + 256 : 0];
    for (int i = tid; i < 2 * h2; i += 256) {
        wh[i & 1][i >> 1] = a.Wmu[i];
        wh[2 + (i & 1)][i >> 1] = a.Wls[i];
    }
    E e;
    e.seed = a.seed; e.id = 0u; e.epi = (float)(a.first + blockIdx.x);
    eval_set_model(e, a.vit, a.pit, 0);
    if (tid == 0) {
        float o[8];
        e.reset(o);
#pragma unroll
        for (int q = 0; q < 8; ++q) xs[q] = o[q];
    }
    float *trow = a.trace ? a.trace + (long long)blockIdx.x * a.max_ep_len * EV_ROW : nullptr;
    double ret = 0.0;
    int len = 0;
    __syncthreads();
    for (;;) {
        {   // layer 1: units tid and tid + 256 in input order
            float acc0 = b1a, acc1 = b1b;
#pragma unroll
            for (int q = 0; q < 8; ++q) { acc0 += xs[q] * u0[q]; acc1 += xs[q] * u1[q]; }
            if (tid < h1) h1s[tid] = fmaxf(acc0, 0.f);
            if (tid + 256 < h1) h1s[tid + 256] = fmaxf(acc1, 0.f);
        }
        __syncthreads();
        // layer 2: wave w takes slices 4 w .. 4 w + 3, lane l the columns l + 64 j
#pragma unroll 1
        for (int si = 0; si < 4; ++si) {
            const int s = wave * 4 + si;
            const int k0 = s * per, k1 = k0 + per < h1 ? k0 + per : h1;
            float acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
            const int cl = (NJ - 1) * 64 + lane < h2 ? (NJ - 1) * 64 + lane : 0;   // the last chunk is the ragged one
#pragma unroll 4
            for (int k = k0; k < k1; ++k) {
                const float h = h1s[k];
                const float *row = a.W2 + (long long)k * h2;
                float w[NJ];
#pragma unroll
                for (int j = 0; j < NJ - 1; ++j) w[j] = row[j * 64 + lane];
                w[NJ - 1] = row[cl];
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] += h * w[j];   // k order
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j * 64 + lane < h2) ps[s][j * 64 + lane] = acc[j];
        }
        __syncthreads();
        for (int c = tid; c < h2; c += 256) {
            float sum = c == tid ? b2a : b2b;
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += ps[q][c];   // slice order
            v2[c] = fmaxf(sum, 0.f);
        }
        __syncthreads();
        if (tid < ng * 4) {   // head partials of one group of 16 columns, one output per thread
            const int b = tid >> 2, t = tid & 3;
            float sum = 0.f;
            for (int q = 0; q < 16; ++q) {
                const int cc = b * 16 + q;
                if (cc < h2) sum += v2[cc] * wh[t][cc];
            }
            part[b][t] = sum;
        }
        __syncthreads();
        len += 1;
        if (tid == 0) {
            float mu[4] = {0.f, 0.f, 0.f, 0.f}, ls[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {a.eps0, a.eps0, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                float sm = 0.f, sl = 0.f;
                for (int b = 0; b < ng; ++b) {   // group order
                    sm += part[b][o];
                    sl += part[b][2 + o];
                }
                mu[o] = sm + a.bmu[o]; ls[o] = sl + a.bls[o];
            }
            const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, 2, a.scale);
            const float a0 = pr.act[0], a1 = pr.act[1];
            float o[8];
            bool done_env;
            const float rew = e.physics(a0, a1, done_env, o);
            e.eplen = e.eplen + 1.0f;                       // as k_env_step (example/dsac.py:103-104)
            e.epret = e.epret + rew;
            const bool ended = done_env || e.eplen >= (float)a.max_ep_len;
            ret += (double)rew;
            if (trow) {
                float4 *p = reinterpret_cast<float4 *>(trow + (long long)(len - 1) * EV_ROW);
                p[0] = make_float4(xs[0], xs[1], xs[2], xs[3]);
                p[1] = make_float4(xs[4], xs[5], xs[6], xs[7]);
                p[2] = make_float4(a0, a1, rew, ended ? 1.0f : 0.0f);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) xs[q] = o[q];
            s_ended = ended ? 1 : 0;
        }
        __syncthreads();
        if (s_ended) break;   // block-uniform
    }
    if (tid == 0) { a.ret[blockIdx.x] = ret; a.len[blockIdx.x] = len; }
    if (trow)
        for (long long i = (long long)len * EV_ROW + tid; i < (long long)a.max_ep_len * EV_ROW; i += 256) trow[i] = 0.f;
}

struct EvalQArgs {
    const float *W1, *b1, *W2, *b2, *W3, *b3;   // q1 of the flat main vector (dqn.param_specs order), obs_dim 8
    double *ret;        // [n] sum of the float32 step rewards in step order, accumulated in float64 (the host loop's `ep_ret += r`)
    int *len;           // [n]
    float *trace;       // nullable [n][max_ep_len][20]: obs[8] acted on, q[8] (zeros beyond A), action index, rew, ended, 0
    int h1, h2, A, max_ep_len;
    int sqn, deterministic;
    float greedy_prob, alpha;
    uint32_t seed, first, noise_seed;
    unsigned long long noise_ctr;
    int vit, pit;       // the articulated model's iteration counts (Env3 only; behind everything the one-body kernel reads)
};

constexpr int EQ_ROW = 20;
constexpr int EQ_A = ddrl_sel::MAXQ;   // 8 head outputs at most

template <class E, int NJ>   // NJ = ceil(h2 / 64): column chunks of one lane
__global__ void __launch_bounds__(256) k_eval_episodes_q(EvalQArgs a) {
    __shared__ float xs[8];
    __shared__ float h1s[512];
    __shared__ float ps[16][512];
    __shared__ float v2[512];
    __shared__ float wh[EQ_A][512];   // head kernel by output
    __shared__ float part[32][EQ_A];
    __shared__ int s_ended;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h1 = a.h1, h2 = a.h2, A = a.A;
    const int per = (h1 + 15) >> 4, ng = (h2 + 15) >> 4;
    // operands that stay in registers for the whole episode: this thread's two layer-1 units, their biases, its two layer-2 biases
    const int j0 = tid < h1 ? tid : 0, j1 = tid + 256 < h1 ? tid + 256 : 0;
    float u0[8], u1[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { u0[q] = a.W1[(long long)q * h1 + j0]; u1[q] = a.W1[(long long)q * h1 + j1]; }
    const float b1a = a.b1[j0], b1b = a.b1[j1];
    const float b2a = a.b2[tid < h2 ? tid : 0], b2b = a.b2[tid + 256 < h2 ? tid + 256 : 0];
    float b3r[EQ_A];
#pragma unroll
    for (int c = 0; c < EQ_A; ++c) b3r[c] = a.b3[c < A ? c : 0];
    for (int i = tid; i < h2 * A; i += 256) wh[i % A][i / A] = a.W3[i];
    E e;
    e.seed = a.seed; e.id = 0u; e.epi = (float)(a.first + blockIdx.x);
    eval_set_model(e, a.vit, a.pit, 0);
    if (tid == 0) {
        float o[8];
        e.reset(o);
#pragma unroll
        for (int q = 0; q < 8; ++q) xs[q] = o[q];
    }
    float *trow = a.trace ? a.trace + (long long)blockIdx.x * a.max_ep_len * EQ_ROW : nullptr;
    const unsigned long long ctr0 = a.noise_ctr + 2ull * ((unsigned long long)blockIdx.x * (unsigned long long)a.max_ep_len);
    double ret = 0.0;
    int len = 0;
    __syncthreads();
    for (;;) {
        {   // layer 1: units tid and tid + 256 in input order
            float acc0 = b1a, acc1 = b1b;
#pragma unroll
            for (int q = 0; q < 8; ++q) { acc0 += xs[q] * u0[q]; acc1 += xs[q] * u1[q]; }
            if (tid < h1) h1s[tid] = fmaxf(acc0, 0.f);
            if (tid + 256 < h1) h1s[tid + 256] = fmaxf(acc1, 0.f);
        }
        __syncthreads();
        // layer 2: wave w takes slices 4 w .. 4 w + 3, lane l the columns l + 64 j
#pragma unroll 1
        for (int si = 0; si < 4; ++si) {
            const int s = wave * 4 + si;
            const int k0 = s * per, k1 = k0 + per < h1 ? k0 + per : h1;
            float acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
            const int cl = (NJ - 1) * 64 + lane < h2 ? (NJ - 1) * 64 + lane : 0;   // the last chunk is the ragged one
#pragma unroll 4
            for (int k = k0; k < k1; ++k) {
                const float h = h1s[k];
                const float *row = a.W2 + (long long)k * h2;
                float w[NJ];
#pragma unroll
                for (int j = 0; j < NJ - 1; ++j) w[j] = row[j * 64 + lane];
                w[NJ - 1] = row[cl];
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] += h * w[j];   // k order
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j * 64 + lane < h2) ps[s][j * 64 + lane] = acc[j];
        }
        __syncthreads();
        for (int c = tid; c < h2; c += 256) {
            float sum = c == tid ? b2a : b2b;
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += ps[q][c];   // slice order
            v2[c] = fmaxf(sum, 0.f);
        }
        __syncthreads();
        if (tid < ng * EQ_A) {   // head partials of one group of 16 columns, one output per thread
            const int b = tid >> 3, t = tid & 7;
            float sum = 0.f;
            if (t < A)
                for (int q = 0; q < 16; ++q) {
                    const int cc = b * 16 + q;
                    if (cc < h2) sum += v2[cc] * wh[t][cc];
                }
            part[b][t] = sum;
        }
        __syncthreads();
        len += 1;
        if (tid == 0) {
            float qv[EQ_A];
#pragma unroll
            for (int c = 0; c < EQ_A; ++c) {
                float s = 0.f;
                for (int b = 0; b < ng; ++b) s += part[b][c];   // group order
                qv[c] = c < A ? s + b3r[c] : 0.f;
            }
            const unsigned long long c0 = ctr0 + 2ull * (unsigned long long)(len - 1);
            const float r0 = ddrl_sel::uniform_at(a.noise_seed, c0), r1 = ddrl_sel::uniform_at(a.noise_seed, c0 + 1ull);
            const int pick = ddrl_sel::select_row<EQ_A>(qv, A, a.sqn, a.deterministic, a.greedy_prob, a.alpha, r0, r1);
            float a0, a1;
            ddrl_sel::lander_action((float)pick, a0, a1);
            float o[8];
            bool done_env;
            const float rew = e.physics(a0, a1, done_env, o);
            e.eplen = e.eplen + 1.0f;                       // as k_env_step (example/dsac.py:103-104)
            e.epret = e.epret + rew;
            const bool ended = done_env || e.eplen >= (float)a.max_ep_len;
            ret += (double)rew;
            if (trow) {
                float4 *p = reinterpret_cast<float4 *>(trow + (long long)(len - 1) * EQ_ROW);
                p[0] = make_float4(xs[0], xs[1], xs[2], xs[3]);
                p[1] = make_float4(xs[4], xs[5], xs[6], xs[7]);
                p[2] = make_float4(qv[0], qv[1], qv[2], qv[3]);
                p[3] = make_float4(qv[4], qv[5], qv[6], qv[7]);
                p[4] = make_float4((float)pick, rew, ended ? 1.0f : 0.0f, 0.0f);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) xs[q] = o[q];
            s_ended = ended ? 1 : 0;
        }
        __syncthreads();
        if (s_ended) break;   // block-uniform
    }
    if (tid == 0) { a.ret[blockIdx.x] = ret; a.len[blockIdx.x] = len; }
    if (trow)
        for (long long i = (long long)len * EQ_ROW + tid; i < (long long)a.max_ep_len * EQ_ROW; i += 256) trow[i] = 0.f;
}

// one launch of n workgroups on the instantiation for h2's column chunks
template <class E>
static void eval_launch(const EvalArgs &a, int n_episodes, hipStream_t s) {
    const unsigned g = (unsigned)n_episodes;
    switch ((a.h2 + 63) / 64) {
        case 1: k_eval_episodes<E, 1><<<g, 256, 0, s>>>(a); break;
        case 2: k_eval_episodes<E, 2><<<g, 256, 0, s>>>(a); break;
        case 3: k_eval_episodes<E, 3><<<g, 256, 0, s>>>(a); break;
        case 4: k_eval_episodes<E, 4><<<g, 256, 0, s>>>(a); break;
        case 5: k_eval_episodes<E, 5><<<g, 256, 0, s>>>(a); break;
        case 6: k_eval_episodes<E, 6><<<g, 256, 0, s>>>(a); break;
        case 7: k_eval_episodes<E, 7><<<g, 256, 0, s>>>(a); break;
        default: k_eval_episodes<E, 8><<<g, 256, 0, s>>>(a); break;
    }
}
template <class E>
static void eval_q_launch(const EvalQArgs &a, int n_episodes, hipStream_t s) {
    const unsigned g = (unsigned)n_episodes;
    switch ((a.h2 + 63) / 64) {
        case 1: k_eval_episodes_q<E, 1><<<g, 256, 0, s>>>(a); break;
        case 2: k_eval_episodes_q<E, 2><<<g, 256, 0, s>>>(a); break;
        case 3: k_eval_episodes_q<E, 3><<<g, 256, 0, s>>>(a); break;
        case 4: k_eval_episodes_q<E, 4><<<g, 256, 0, s>>>(a); break;
        case 5: k_eval_episodes_q<E, 5><<<g, 256, 0, s>>>(a); break;
        case 6: k_eval_episodes_q<E, 6><<<g, 256, 0, s>>>(a); break;
        case 7: k_eval_episodes_q<E, 7><<<g, 256, 0, s>>>(a); break;
        default: k_eval_episodes_q<E, 8><<<g, 256, 0, s>>>(a); break;
    }
}

// the argument structs from a flat weight vector: the policy in ddrl_actor_get_weights' order, q1 of ddrl_dqn_export(MAIN)'s
static EvalArgs eval_args_of(const ddrl_sac1_config_t &cfg, const float *pi_flat) {
    const long long h1 = cfg.hidden1, h2 = cfg.hidden2;
    EvalArgs a{};
    a.W1 = pi_flat; a.b1 = a.W1 + 8 * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2;
    a.Wmu = a.b2 + h2; a.bmu = a.Wmu + 2 * h2; a.Wls = a.bmu + 2; a.bls = a.Wls + 2 * h2;
    a.h1 = (int)h1; a.h2 = (int)h2;
    a.scale = (float)cfg.act_scale; a.eps0 = 0.0f;
    return a;
}
static EvalQArgs eval_q_args_of(const ddrl_dqn_config_t &cfg, const float *q_flat) {
    const long long h1 = cfg.hidden1, h2 = cfg.hidden2, A = cfg.n_actions;
    EvalQArgs a{};
    a.W1 = q_flat; a.b1 = a.W1 + 8 * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2; a.W3 = a.b2 + h2; a.b3 = a.W3 + h2 * A;
    a.h1 = (int)h1; a.h2 = (int)h2; a.A = (int)A;
    a.sqn = cfg.variant == DDRL_SQN; a.alpha = (float)cfg.alpha;
    return a;
}

}  // namespace

// What the handle-fed entry points (eval3.hip) ask of the agent handles: the configuration and the device (actor.hip, dqn.hip)
int ddrl_actor_internal_config(ddrl_actor_t *h, ddrl_sac1_config_t *cfg_out, int *device_out);
int ddrl_dqn_internal_config(ddrl_dqn_t *h, ddrl_dqn_config_t *cfg_out, int *device_out);
