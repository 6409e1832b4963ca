// Evaluation episodes of the BIPEDAL WALKER on the device, fed from handles: ddrl_env_eval_policy_walker (include/ddrl_walker_eval.h),
// read back by ddrl_env_eval_results (eval3.hip).  One workgroup of 256 threads per episode, nothing crosses workgroups, as
// k_eval_episodes (eval_episodes.h) on the landers:
//   * the policy row on all threads: k_act_one's arithmetic (actor.hip) statement for statement at d0 = 24, act = 4 — layer-1 units
//     summed on the bias in input order; layer 2 as 16 slices of ceil(h1 / 16) rows per column, each summed in row order from zero and
//     added in slice order on the bias; the eight head partials (mu 0..3, log_std 0..3) per group of 16 columns, each summed in column
//     order from zero, added in group order, then the head bias, then ddrl_pol::policy_row with the noise elements eps0 = 0.  So a
//     step's action is bit for bit what Actor.get_action(o, deterministic=True) returns for the same observation;
//   * then ONE lane runs Walker (walker_device.h, unchanged) as k_walker_reset / k_walker_step run it (walker.hip): seed = the handle's,
//     id = 0, epi = first_episode + blockIdx.x; build(), one zero-action physics(), obs(); per step eplen += 1, epret += rew,
//     ended = done_env || eplen >= max_ep_len.  Episode e is the (first_episode + e)-th a host env.BipedalWalker of the handle's seed,
//     max_ep_len and iteration counts plays.
// The kernel holds ONE inlined physics(): the reset's zero-action step is the first trip through the loop body, whose policy row it
// skips.  The loop's only exit is the block-uniform s_ended flag and eplen counts every trip behind the first, so the kernel ends after
// at most max_ep_len steps whatever the weights are.
// Walker's pointers: with n = 1, Sc and T point at `col`, a state-block column in LDS (the 200 terrain heights of the episode and the
// fields build() writes through Sc); the handle's state block is neither read nor written.  Walker::L is lane 0's column of the
// sweep fields [W_LDS_FIELDS][64] (27 KiB), which are written and read inside physics() only; the 32 KiB of layer-2 slice sums are dead
// from the head partials to the next layer 2, and barriers stand between the two uses — they share their bytes (`big`), which keeps the
// static LDS under 64 KiB.  No scratch, no spilled VGPRs: profiles/walker_eval_resource_usage.txt.
// Compiled with -ffp-contract=off; write no fmaf here.  A translation unit of its own: no other file's kernels depend on it.
#include "ddrl_common.h"
#include "../../include/ddrl_walker_eval.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "policy_row.h"
#include "walker_device.h"
#include "env_handle.h"
#include "eval_host.h"

namespace {

constexpr int WE_ROW = 32;   // a trace row: obs[24] acted on, act[4], rew, ended, 0, 0

struct WalkerEvalArgs {
    const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wls, *bls;   // the flat external-order policy vector (obs_dim 24, act_dim 4)
    double *ret;        // [n] sum of the float32 step rewards in step order, accumulated in float64 (the host loop's `ep_ret += r`)
    int *len;           // [n]
    float *trace;       // nullable [n][max_ep_len][32]; rows past the end are zero
    int h1, h2, max_ep_len;
    float scale, eps0;  // eps0 = 0: the noise element of a deterministic action (a kernel argument: the row math is not folded around it)
    uint32_t seed, first;
    int vit, pit;
};

constexpr int WE_PS = 16 * 512;   // floats of the layer-2 slice sums ...
static_assert(W_LDS_FIELDS * 64 <= WE_PS, "... which the walker's sweep fields share");

// layer 2 for NJ = ceil(h2 / 64) column chunks per lane: wave w takes slices 4 w .. 4 w + 3, lane l the columns l + 64 j
template <int NJ>
__device__ __forceinline__ void we_layer2(const float *W2, const float *h1s, float *ps, int h1, int h2, int per, int wave, int lane) {
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
            const float *row = W2 + (long long)k * h2;
            float w[NJ];
#pragma unroll
            for (int j = 0; j < NJ - 1; ++j) w[j] = row[j * 64 + lane];
            w[NJ - 1] = row[cl];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] += h * w[j];   // k order
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j * 64 + lane < h2) ps[s * 512 + j * 64 + lane] = acc[j];
    }
}

__global__ void __launch_bounds__(256) k_walker_eval(WalkerEvalArgs a) {
    __shared__ float xs[WOBS];
    __shared__ float h1s[512];
    __shared__ float big[WE_PS];     // ps[16][512] from layer 2 to the slice sums' addition; Walker's sweep fields inside physics()
    __shared__ float v2[512];
    __shared__ float wh[8][512];     // head kernels by output: mu 0..3, log_std 0..3
    __shared__ float part[32][8];
    __shared__ float col[NFW];       // the episode's state-block column (n = 1): what build() writes through Sc, the terrain at WT0
    __shared__ int s_ended;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h1 = a.h1, h2 = a.h2;
    const int per = (h1 + 15) >> 4, ng = (h2 + 15) >> 4, nj = (h2 + 63) >> 6;
    // operands that stay in registers for the whole episode: this thread's two layer-1 units, their biases, its two layer-2 biases
    const int j0 = tid < h1 ? tid : 0, j1 = tid + 256 < h1 ? tid + 256 : 0;
    float u0[WOBS], u1[WOBS];
#pragma unroll
    for (int q = 0; q < WOBS; ++q) { u0[q] = a.W1[(long long)q * h1 + j0]; u1[q] = a.W1[(long long)q * h1 + j1]; }
    const float b1a = a.b1[j0], b1b = a.b1[j1];
    const float b2a = a.b2[tid < h2 ? tid : 0], b2b = a.b2[tid + 256 < h2 ? tid + 256 : 0];
    for (int i = tid; i < 4 * h2; i += 256) {
        wh[i & 3][i >> 2] = a.Wmu[i];
        wh[4 + (i & 3)][i >> 2] = a.Wls[i];
    }
    Walker e;
    float act[WACT] = {0.0f, 0.0f, 0.0f, 0.0f};   // lane 0's: zero for the reset's trip, then the policy row's
    if (tid == 0) {
        e.L = big; e.Sc = col; e.T = col + WT0; e.n = 1;
        e.seed = a.seed; e.id = 0u; e.vit = a.vit; e.pit = a.pit;
        e.epi = (float)(a.first + blockIdx.x);
        e.build();
        s_ended = 0;
    }
    float *trow = a.trace ? a.trace + (long long)blockIdx.x * a.max_ep_len * WE_ROW : nullptr;
    double ret = 0.0;
    int len = 0;
    // trip 0: the zero-action step inside env.reset(); trip t >= 1: step t of the episode, acted on with the row computed behind trip t - 1
    for (;;) {
        if (tid == 0) {
            bool done_env;
            const float rew = e.physics(act, done_env);
            float o[WOBS];
            e.obs(o);
            if (len > 0) {
                e.eplen = e.eplen + 1.0f;                       // as k_walker_step (example/dsac.py:103-104)
                e.epret = e.epret + rew;
                const bool ended = done_env || e.eplen >= (float)a.max_ep_len;
                ret += (double)rew;
                if (trow) {
                    float4 *p = reinterpret_cast<float4 *>(trow + (long long)(len - 1) * WE_ROW);
#pragma unroll
                    for (int k = 0; k < WOBS / 4; ++k) p[k] = make_float4(xs[4 * k], xs[4 * k + 1], xs[4 * k + 2], xs[4 * k + 3]);
                    p[6] = make_float4(act[0], act[1], act[2], act[3]);
                    p[7] = make_float4(rew, ended ? 1.0f : 0.0f, 0.0f, 0.0f);
                }
                s_ended = ended ? 1 : 0;
            }
#pragma unroll
            for (int q = 0; q < WOBS; ++q) xs[q] = o[q];
        }
        __syncthreads();
        if (s_ended) break;   // block-uniform
        {   // layer 1: units tid and tid + 256 in input order
            float acc0 = b1a, acc1 = b1b;
#pragma unroll
            for (int q = 0; q < WOBS; ++q) { acc0 += xs[q] * u0[q]; acc1 += xs[q] * u1[q]; }
            if (tid < h1) h1s[tid] = fmaxf(acc0, 0.f);
            if (tid + 256 < h1) h1s[tid + 256] = fmaxf(acc1, 0.f);
        }
        __syncthreads();
        switch (nj) {   // block-uniform
            case 1: we_layer2<1>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 2: we_layer2<2>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 3: we_layer2<3>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 4: we_layer2<4>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 5: we_layer2<5>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 6: we_layer2<6>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            case 7: we_layer2<7>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
            default: we_layer2<8>(a.W2, h1s, big, h1, h2, per, wave, lane); break;
        }
        __syncthreads();
        for (int c = tid; c < h2; c += 256) {
            float sum = c == tid ? b2a : b2b;
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += big[q * 512 + c];   // slice order
            v2[c] = fmaxf(sum, 0.f);
        }
        __syncthreads();   // from here to the next layer 2 `big` is the walker's
        if (tid < ng * 8) {   // head partials of one group of 16 columns, one output per thread
            const int b = tid >> 3, t = tid & 7;
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
            float mu[4], ls[4], ev[4] = {a.eps0, a.eps0, a.eps0, a.eps0};
#pragma unroll
            for (int o = 0; o < WACT; ++o) {
                float sm = 0.f, sl = 0.f;
                for (int b = 0; b < ng; ++b) {   // group order
                    sm += part[b][o];
                    sl += part[b][WACT + o];
                }
                mu[o] = sm + a.bmu[o]; ls[o] = sl + a.bls[o];
            }
            const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, WACT, a.scale);
#pragma unroll
            for (int o = 0; o < WACT; ++o) act[o] = pr.act[o];
        }
    }
    if (tid == 0) { a.ret[blockIdx.x] = ret; a.len[blockIdx.x] = len; }
    if (trow)
        for (long long i = (long long)len * WE_ROW + tid; i < (long long)a.max_ep_len * WE_ROW; i += 256) trow[i] = 0.f;
}

}  // namespace

extern "C" {

int ddrl_env_eval_policy_walker(ddrl_env_t *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode, int32_t want_trace,
                                void *stream) {
    const char *what = "ddrl_env_eval_policy_walker";
    if (const int rc = eval_common_check(what, h, actor, n_episodes, first_episode, [&]() -> int {
            if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_WALKER, what, "ddrl_env_eval_policy")) return rc;   // a lander handle: the landers' entry point
            if (h->terrain != DDRL_WALKER_TERRAIN_GRASS) {   // k_walker_eval keeps the episode's terrain in LDS and builds grass only
                ddrl::set_error("%s: not built for the hardcore terrain (ddrl_env_create_walker, DDRL_WALKER_TERRAIN_HARDCORE): the "
                                "evaluation kernel holds the grass terrain — step a host env instead", what);
                return DDRL_ERR_UNSUPPORTED;
            }
            return DDRL_OK;
        })) return rc;
    ddrl_sac1_config_t cfg;
    int adev = -1;
    if (const int rc = ddrl_actor_internal_config(actor, &cfg, &adev)) return rc;
    if (adev != h->device) {
        ddrl::set_error("%s: bad argument: the actor lives on device %d, the env handle on device %d", what, adev, h->device);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.obs_dim != WOBS || cfg.act_dim != WACT) {
        ddrl::set_error("%s: bad argument: the walker has 24 observations and 4 actions (actor: %d -> %d)", what, cfg.obs_dim, cfg.act_dim);
        return DDRL_ERR_BAD_ARG;
    }
    if (cfg.hidden1 < 1 || cfg.hidden2 < 1 || cfg.hidden1 > 512 || cfg.hidden2 > 512) {
        ddrl::set_error("%s: hidden width outside [1, 512] (the envelope of ddrl_actor_act_one): step a host env instead", what);
        return DDRL_ERR_UNSUPPORTED;
    }
    int64_t n_pi = 0, n_q = 0;
    if (const int rc = ddrl_sac1_param_counts(&cfg, &n_pi, &n_q)) return rc;
    ddrl::DeviceGuard g(h->device);
    if (const int rc = eval_reserve(h, what, n_episodes, want_trace ? WE_ROW : 0, (size_t)n_pi)) return rc;
    if (const int rc = ddrl_actor_get_weights(actor, h->ev_w, stream)) return rc;
    const long long h1 = cfg.hidden1, h2 = cfg.hidden2;
    WalkerEvalArgs a{};
    a.W1 = h->ev_w; a.b1 = a.W1 + WOBS * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2;
    a.Wmu = a.b2 + h2; a.bmu = a.Wmu + WACT * h2; a.Wls = a.bmu + WACT; a.bls = a.Wls + WACT * h2;
    a.ret = reinterpret_cast<double *>(h->ev_block);
    a.len = reinterpret_cast<int *>(h->ev_block + h->ev_len_off);
    a.trace = want_trace ? reinterpret_cast<float *>(h->ev_block + h->ev_trace_off) : nullptr;
    a.h1 = (int)h1; a.h2 = (int)h2; a.max_ep_len = h->max_ep_len;
    a.scale = (float)cfg.act_scale; a.eps0 = 0.0f;
    a.seed = h->seed; a.first = first_episode;
    a.vit = h->vit; a.pit = h->pit;
    k_walker_eval<<<(unsigned)n_episodes, 256, 0, ddrl::as_stream(stream)>>>(a);
    DDRL_LAUNCH_CHECK();
    h->ev_n = n_episodes; h->ev_row = want_trace ? WE_ROW : 0;
    return DDRL_OK;
}

}  // extern "C"
