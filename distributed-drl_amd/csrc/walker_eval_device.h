// The walker's evaluation episode, ONE text for both terrain modes: the episode loop and the policy row of k_walker_eval
// (walker_eval.hip: WalkerT<0>, the grass terrain) and k_walker_hc_eval (walker_hardcore_eval.hip: WalkerT<1, 1>, the Hardcore terrain),
// each of which is the text of walker_eval_body.h between the braces of a kernel of its own translation unit; what that text needs at
// file scope (the arguments, layer 2); and what the two entry points do on the host behind their own guards (walker_eval_prepare).
// One workgroup of 256 threads per episode, nothing crosses workgroups, as k_eval_episodes (eval_episodes.h) on the landers:
//   * the policy row on all threads: k_act_one's arithmetic (actor.hip) statement for statement at d0 = 24, act = 4 — layer-1 units
//     summed on the bias in input order; layer 2 as 16 slices of ceil(h1 / 16) rows per column, each summed in row order from zero and
//     added in slice order on the bias; the eight head partials (mu 0..3, log_std 0..3) per group of 16 columns, each summed in column
//     order from zero, added in group order, then the head bias, then ddrl_pol::policy_row with the noise elements eps0 = 0.  So a
//     step's action is bit for bit what Actor.get_action(o, deterministic=True) returns for the same observation;
//   * then ONE lane runs the terrain's WalkerT (walker_device.h, unchanged) as the terrain's reset / step kernels run it
//     (walker.hip): seed = the handle's, id = 0, epi = first_episode + blockIdx.x; build(), one zero-action physics(), obs();
//     per step eplen += 1, epret += rew, ended = done_env || eplen >= max_ep_len.  Episode e is the (first_episode + e)-th a host
//     env.BipedalWalker of the handle's seed, max_ep_len, iteration counts and terrain plays.
// The kernel holds ONE inlined physics(): the reset's zero-action step is the first trip through the loop body, whose policy row it
// skips.  The loop's only exit is the block-uniform s_ended flag and eplen counts every trip behind the first, so the kernel ends after
// at most max_ep_len steps whatever the weights are.
// The walker's pointers: with n = 1, Sc and T (Hardcore: B and Cc too) point into `col`, a state-block column in LDS — NFW floats on
// grass (the 200 terrain heights of the episode and the fields build() writes through Sc), NFWH on the Hardcore terrain (behind them
// the box count, the box table and the per-column box index its generator writes and its contacts, hull test and lidar read); the
// handle's state block is neither read nor written.  WalkerT::L is the one lane's column of the sweep fields — [W_LDS_FIELDS][64] on
// grass (27 KiB, lane 0's column), [W_LDS_FIELDS_H][1] on the Hardcore terrain (688 bytes) — which are written and read inside
// physics() only; the 32 KiB of layer-2 slice sums are dead from the head partials to the next layer 2, and barriers stand between the
// two uses — they share their bytes (`big`), which keeps the static LDS under 64 KiB.
// Compiled with -ffp-contract=off; write no fused multiply-add here.  Internal linkage throughout.
#pragma once
#include "ddrl_common.h"
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

// What both entry points do behind eval_common_check and their own kind and terrain guards, in front of their launch: the actor's
// device and shape, the envelope of the hidden widths, the results block and the weight staging (eval_reserve), the weights out of the
// actor handle on `stream`, the kernel's arguments.  Refuses with `what` in front and nothing written.  The caller holds a
// ddrl::DeviceGuard on the handle's device around this call and its launch.
int walker_eval_prepare(const char *what, ddrl_env *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode, int32_t want_trace,
                        void *stream, WalkerEvalArgs &a) {
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
    if (const int rc = eval_reserve(h, what, n_episodes, want_trace ? WE_ROW : 0, (size_t)n_pi)) return rc;
    if (const int rc = ddrl_actor_get_weights(actor, h->ev_w, stream)) return rc;
    const long long h1 = cfg.hidden1, h2 = cfg.hidden2;
    a = WalkerEvalArgs{};
    a.W1 = h->ev_w; a.b1 = a.W1 + WOBS * h1; a.W2 = a.b1 + h1; a.b2 = a.W2 + h1 * h2;
    a.Wmu = a.b2 + h2; a.bmu = a.Wmu + WACT * h2; a.Wls = a.bmu + WACT; a.bls = a.Wls + WACT * h2;
    a.ret = reinterpret_cast<double *>(h->ev_block);
    a.len = reinterpret_cast<int *>(h->ev_block + h->ev_len_off);
    a.trace = want_trace ? reinterpret_cast<float *>(h->ev_block + h->ev_trace_off) : nullptr;
    a.h1 = (int)h1; a.h2 = (int)h2; a.max_ep_len = h->max_ep_len;
    a.scale = (float)cfg.act_scale; a.eps0 = 0.0f;
    a.seed = h->seed; a.first = first_episode;
    a.vit = h->vit; a.pit = h->pit;
    return DDRL_OK;
}

}  // namespace
