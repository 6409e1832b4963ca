// The test worker's evaluation episodes as ONE launch: `Actor.test` (algos/sac1/actor_learner.py:199-218) and `Model.test_agent`
// (example/model.py:106-118) walk n deterministic episodes — get_action(o, deterministic) then env.step(a), one after the other.
// An episode is a strictly serial chain of one policy row and one env step, and the episodes are independent of each other:
// one workgroup plays one episode from reset to its end without the host, n episodes are n workgroups.  Nothing crosses
// workgroups (no ticket, no fence, no spin-wait).
//
// The policy row is the arithmetic of k_act_one (sac1.hip) statement for statement, so that with -ffp-contract=off it yields the same
// bits as the get_action launch the host loop issues per step: layer-1 units summed in input order on the bias; layer 2 as 16 slices
// of ceil(h1 / 16) contraction rows per column, each summed in row order from zero, the 16 slice sums added in slice order on the
// bias; head partials per group of 16 columns in column order from zero, the groups added in group order, then the head bias; then
// ddrl_pol::policy_row with eps = 0.  Only the assignment of (column, slice) sums to threads differs: a wave takes 64 consecutive
// columns of one contraction row per load (256 contiguous bytes) instead of 16 columns of four slices.
// The env step is Env::physics plus the bookkeeping of k_env_step (env.hip), run by one lane with the env state in registers.
#include "ddrl_common.h"
#include "policy_row.h"
#include "env_device.h"

namespace {

struct EvalArgs {
    const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wls, *bls;   // the flat external-order policy vector (act_dim 2, obs_dim 8)
    double *ret;        // [n] sum of the float32 step rewards in step order, accumulated in float64 (the host loop's `ep_ret += r`)
    int *len;           // [n]
    float *trace;       // nullable [n][max_ep_len][12]: obs[8] acted on, act[2], rew, ended; rows past the end are zero
    int h1, h2, max_ep_len;
    float scale, eps0;  // eps0 = 0: the noise element of a deterministic action (a kernel argument: the row math is not folded around it)
    uint32_t seed, first;
};

constexpr int EV_ROW = 12;

template <int NJ>   // ceil(h2 / 64): column chunks of one lane
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
    Env e;
    e.seed = a.seed; e.id = 0u; e.epi = (float)(a.first + blockIdx.x);
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

}  // namespace

extern "C" {

int ddrl_policy_eval(const ddrl_sac1_config_t *cfg, const float *pi_flat_d, int32_t n_episodes, uint32_t env_seed, uint32_t first_episode,
                     int32_t max_ep_len, double *ret_d, int32_t *len_d, float *trace_d, void *stream) {
    DDRL_REQUIRE(cfg != nullptr && pi_flat_d != nullptr && ret_d != nullptr && len_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(cfg->obs_dim == 8 && cfg->act_dim == 2, "the lander has 8 observations and 2 actions");
    DDRL_REQUIRE(n_episodes >= 1 && max_ep_len >= 1, "n_episodes and max_ep_len must be >= 1");
    DDRL_REQUIRE(cfg->hidden1 >= 1 && cfg->hidden2 >= 1, "hidden sizes must be >= 1");
    DDRL_REQUIRE(max_ep_len < (1 << 24) && (uint64_t)first_episode + (uint64_t)n_episodes <= (1u << 24),
                 "max_ep_len and the episode index must stay exact in float32");
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(trace_d) & 15) == 0, "trace_d must be 16-byte aligned");
    if (cfg->hidden1 > 512 || cfg->hidden2 > 512) {
        ddrl::set_error("ddrl_policy_eval: hidden width > 512 (the envelope of ddrl_actor_act_one): step a host env instead");
        return DDRL_ERR_UNSUPPORTED;
    }
    const long long h1 = cfg->hidden1, h2 = cfg->hidden2;
    EvalArgs a{};
    a.W1 = pi_flat_d; a.b1 = a.W1 + 8 * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2;
    a.Wmu = a.b2 + h2; a.bmu = a.Wmu + 2 * h2; a.Wls = a.bmu + 2; a.bls = a.Wls + 2 * h2;
    a.ret = ret_d; a.len = len_d; a.trace = trace_d;
    a.h1 = (int)h1; a.h2 = (int)h2; a.max_ep_len = max_ep_len;
    a.scale = (float)cfg->act_scale; a.eps0 = 0.0f;
    a.seed = env_seed; a.first = first_episode;
    hipStream_t s = ddrl::as_stream(stream);
    const unsigned g = (unsigned)n_episodes;
    switch ((h2 + 63) / 64) {
        case 1: k_eval_episodes<1><<<g, 256, 0, s>>>(a); break;
        case 2: k_eval_episodes<2><<<g, 256, 0, s>>>(a); break;
        case 3: k_eval_episodes<3><<<g, 256, 0, s>>>(a); break;
        case 4: k_eval_episodes<4><<<g, 256, 0, s>>>(a); break;
        case 5: k_eval_episodes<5><<<g, 256, 0, s>>>(a); break;
        case 6: k_eval_episodes<6><<<g, 256, 0, s>>>(a); break;
        case 7: k_eval_episodes<7><<<g, 256, 0, s>>>(a); break;
        default: k_eval_episodes<8><<<g, 256, 0, s>>>(a); break;
    }
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

}  // extern "C"
