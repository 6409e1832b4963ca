// The DQN / SQN test worker's evaluation episodes as ONE launch: `Actor.test` (algos/dqn/actor_learner.py:230-251,
// algos/sqn/actor_learner.py:229-250) walks n episodes — get_action(o) then env.step(a), one after the other.  The discrete counterpart
// of k_eval_episodes (eval.hip), with the same decomposition: an episode is a strictly serial chain of one Q row, one selection and
// one env step, the episodes are independent of each other, so one workgroup plays one episode from reset to its end without the
// host and n episodes are n workgroups.  Nothing crosses workgroups (no ticket, no fence, no spin-wait).
//
// The Q row is the main network q1 (SQN: q1 only, as ddrl_dqn_act), 8 -> h1 -> h2 -> A, relu on both hidden layers, a linear head.
// Summation order (the library is built with -ffp-contract=off, so tests/_discrete_eval_trace.py::q_row32 restates it exactly):
//   layer 1   unit j: the bias, then + x[q] * W1[q][j] for q = 0 .. 7 in input order; relu
//   layer 2   column c: 16 slices of per = ceil(h1 / 16) contraction rows (slice s = rows s * per .. min(s * per + per, h1) - 1, empty
//             past h1), each summed in row order from zero; the 16 slice sums added in slice order on the bias; relu
//   head      output a: partials per group of 16 columns (group b = columns 16 b .. 16 b + 15 below h2) in column order from zero, the
//             groups added in group order from zero, then + the head bias
// As in k_eval_episodes a wave takes 64 consecutive columns of one contraction row of W2 per load (256 contiguous bytes, out of L2),
// the layer-1 operands and the env state stay in registers, the hidden layers and the partials live in LDS.
// Selection is ddrl_sel::select_row<8> (dqn_select.h), the function k_dqn_select and k_env_step_q call: step t of episode e of the call
// owns u0 = U(seed, ctr + 2 (e * max_ep_len + t)) and u1 = U(seed, ctr + 2 (e * max_ep_len + t) + 1) of ddrl_uniform_fill's generator.
// The env step is ddrl_sel::lander_action, then Env::physics plus the bookkeeping of k_env_step (env.hip), run by one lane.
#include "ddrl_common.h"
#include "policy_row.h"
#include "env_device.h"
#include "dqn_select.h"

namespace {

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
};

constexpr int EQ_ROW = 20;
constexpr int EQ_A = ddrl_sel::MAXQ;   // 8 head outputs at most

template <int NJ>   // ceil(h2 / 64): column chunks of one lane
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
    Env e;
    e.seed = a.seed; e.id = 0u; e.epi = (float)(a.first + blockIdx.x);
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

}  // namespace

extern "C" {

int ddrl_dqn_eval(const ddrl_dqn_config_t *cfg, const float *q_flat_d, int32_t n_episodes, uint32_t env_seed, uint32_t first_episode,
                  int32_t max_ep_len, int mode, float greedy_prob, uint32_t noise_seed, uint64_t noise_ctr, double *ret_d, int32_t *len_d,
                  float *trace_d, void *stream) {
    DDRL_REQUIRE(cfg != nullptr && q_flat_d != nullptr && ret_d != nullptr && len_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(cfg->obs_dim == 8 && cfg->n_actions >= 1, "the lander has 8 observations; n_actions must be >= 1");
    DDRL_REQUIRE(n_episodes >= 1 && max_ep_len >= 1, "n_episodes and max_ep_len must be >= 1");
    DDRL_REQUIRE(cfg->hidden1 >= 1 && cfg->hidden2 >= 1, "hidden sizes must be >= 1");
    DDRL_REQUIRE(max_ep_len <= (1 << 24) && (uint64_t)first_episode + (uint64_t)n_episodes <= (1u << 24),
                 "max_ep_len and the episode index must stay exact in float32");
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(trace_d) & 15) == 0, "trace_d must be 16-byte aligned");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    DDRL_REQUIRE(cfg->variant == DDRL_DDQN || (cfg->variant == DDRL_SQN && cfg->alpha > 0.0), "variant must be DDRL_DDQN or DDRL_SQN with alpha > 0");
    if (cfg->hidden1 > 512 || cfg->hidden2 > 512) {
        ddrl::set_error("ddrl_dqn_eval: hidden width > 512 (the kernel's LDS layout): step a host env instead");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (cfg->n_actions > ddrl_sel::MAXQ) {
        ddrl::set_error("ddrl_dqn_eval: n_actions > %d (ddrl_sel::select_row<8>): step a host env instead", ddrl_sel::MAXQ);
        return DDRL_ERR_UNSUPPORTED;
    }
    const long long h1 = cfg->hidden1, h2 = cfg->hidden2, A = cfg->n_actions;
    EvalQArgs a{};
    a.W1 = q_flat_d; a.b1 = a.W1 + 8 * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2; a.W3 = a.b2 + h2; a.b3 = a.W3 + h2 * A;
    a.ret = ret_d; a.len = len_d; a.trace = trace_d;
    a.h1 = (int)h1; a.h2 = (int)h2; a.A = (int)A; a.max_ep_len = max_ep_len;
    a.sqn = cfg->variant == DDRL_SQN; a.deterministic = mode == DDRL_ACT_DETERMINISTIC;
    a.greedy_prob = greedy_prob; a.alpha = (float)cfg->alpha;
    a.seed = env_seed; a.first = first_episode; a.noise_seed = noise_seed; a.noise_ctr = noise_ctr;
    hipStream_t s = ddrl::as_stream(stream);
    const unsigned g = (unsigned)n_episodes;
    switch ((h2 + 63) / 64) {
        case 1: k_eval_episodes_q<1><<<g, 256, 0, s>>>(a); break;
        case 2: k_eval_episodes_q<2><<<g, 256, 0, s>>>(a); break;
        case 3: k_eval_episodes_q<3><<<g, 256, 0, s>>>(a); break;
        case 4: k_eval_episodes_q<4><<<g, 256, 0, s>>>(a); break;
        case 5: k_eval_episodes_q<5><<<g, 256, 0, s>>>(a); break;
        case 6: k_eval_episodes_q<6><<<g, 256, 0, s>>>(a); break;
        case 7: k_eval_episodes_q<7><<<g, 256, 0, s>>>(a); break;
        default: k_eval_episodes_q<8><<<g, 256, 0, s>>>(a); break;
    }
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

}  // extern "C"
