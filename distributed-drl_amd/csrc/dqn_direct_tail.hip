// The direct-operand tail of a Double-DQN / soft-Q learner of any observation width (ddrl_dqn_create_direct_tail,
// include/ddrl_dqn_direct_tail.h).  Layer 1 stays where it is (k_wide / k_gemm forward, k_wide_sk / launch_wide_wgrad / k_gemm weight
// gradient, k_adam_polyak over [W1 ; b1]); everything between H1 and dZ1 is three launches:
//   k_qtfwd   layer 2 and the head partials of every evaluation (DDQN: q(x), q(x2), q_targ(x2); SQN: q1(x), q1(x2), q2(x), q1_targ(x2),
//             q2_targ(x2)).  One workgroup = a 32 x 32 tile of one evaluation on v_mfma_f32_32x32x2_f32, the contraction (hidden1) dealt
//             to the four waves in 8-deep groups (group g to wave g % 4: hidden1 = 64 still feeds every wave).  Nothing is generated and
//             no GEMM operand goes through LDS: lane (row, half) reads H1[row][8 g + 4 half ..] as ONE float4 out of the row-major image
//             layer 1 left (ldh1 % 4 == 0: 16-byte aligned), lane (column, half) the matching float4 of the k4-interleaved W2 — element e
//             of the two is MFMA step e of the group.  A wave's groups go four at a time (a 32-deep block of its share): the next block's
//             eight requests are issued in front of this block's sixteen MFMAs, ping-pong in registers.  Epilogue as k_qfwd's: fixed-order
//             LDS combine of the waves, bias + relu, H2c4 / H2r4 of the differentiated evaluations, head partials against [W3 ; b3].
//   k_qtmid   k_qmid's row prologue (q_rows: partials in column-tile order + b3, arg-max / soft value, backup, dq, loss partials, q rows)
//             and a tile of the dgrad with dZ2 generated in the tile; its output is NOT consumed by a generated layer-1 wgrad but stored
//             row-major, relu mask of H1 applied, as dZ1 [network][batch][hidden1]: the B operand k_wide_sk / k_gemm read.  One more
//             workgroup: the W3 snapshot and the polled words of this update's k_wide_sk (k_dqn_head's duty on the generic path).
//   k_qtlast  [H1 | 1]^T dZ2 into both W2 images and b2, [H2 | 1]^T dQ into [W3 ; b3], TF1 Adam + polyak in the epilogues; the batch in
//             8-deep groups over the waves, fixed-order LDS combine; + the loss mean in row-tile order.  It runs behind the dgrad (it
//             steps the W2 / W3 the dgrad reads) and behind the layer-1 wgrad, which reads dZ1 and x only: stream order, any
//             position after k_qtmid is correct, and the last one keeps the parameters of an update stepped back to back.
// The W2 wgrad's A operand is ROW-MAJOR H1, read directly: lane (unit, half) takes its four batch rows of a group as four dword requests,
// each one contiguous over the 32 units of the half-wave (128 bytes).  The alternative — k_qtfwd leaving the [row / 4][unit][4] image
// k_qlast reads — would make k_qtfwd re-store an array layer 1 has just written (one more 32 x hidden1 image store per row tile, on a
// column tile that has to be chosen and balanced) to turn four coalesced requests into one in a loop of at most 16 groups per wave; and
// column hidden1 of the row-major image already holds the 1 of the bias row.
// The optimizer's books are NOT kept here: k_qtlast takes its step size from the handle's OptState as it stands, the same beta powers the
// layer-1 k_adam_polyak launch behind it reads and then advances — one set of books for both optimizer paths.
// Every cross-workgroup sum has a fixed order; no spin, no wait on another workgroup: a dependency ends the launch.
// Layout of a network inside main / target / m / v / gradient: W2 [Kp/4][Np][4] | b2 [Np] | [W3 ; b3] [h2 + 1][A] | W2 dgrad image [Np/4][Kp][4].
#include "gemm_core.h"
#include "policy_row.h"
#include "dqn_direct.h"
#include "dqn_direct_tail.h"
#include "../../include/ddrl_dqn_direct.h"
#include "../../include/ddrl_dqn_direct_tail.h"

namespace {
#include "sac1_direct.h"
#include "dqn_direct_shared.h"

// what the tail's launches read beside QBArgs: the handle's row-major images
struct QTX {
    const float *H1[2];       // H1 of the differentiated evaluation of network n: [batch][ldh1], column h1 holds 1
    float *dZ1;               // [network][batch][h1]
    int ldh1;
    int *zero_words;
    int n_zero;
    const OptState *opt;
};

// ==========================================================================================
// launch 1: layer 2 + head partials
// ==========================================================================================
struct QTJob {
    int w_off;               // the network's W2 image inside the slab
    const float *H1;         // this evaluation's layer-1 output
    float *hp;               // head partials [DFH][Bp][DNT]
    float *H2c4, *H2r4;      // side outputs of a differentiated evaluation (nullable)
};
struct QTFArgs {
    const float *slab;
    int ldh1, B, Bp, K, NG, Np, h2, A, tiles_m, tiles_n, Lp2, b2_off, w3_off;   // NG: 8-deep groups per wave = Kp / 32
    QTJob job[DX_MAXEV];
};

__global__ void __launch_bounds__(256) k_qtfwd(QTFArgs a) {
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ float s_wh[DFH][32];
    const int tpj = a.tiles_m * a.tiles_n;
    int t = blockIdx.x;
    const int ji = t / tpj;
    t -= ji * tpj;
    const int nt = t / a.tiles_m, m0 = (t - nt * a.tiles_m) * 32, n0 = nt * 32;
    const QTJob &jb = a.job[ji];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int NG = a.NG;
    const float *P = a.slab + jb.w_off;
    const int rowc = m0 + l31 < a.B ? m0 + l31 : a.B - 1;   // rows of the last tile beyond the batch repeat its last row (they carry dq = 0)
    const float *hrow = jb.H1 + (long long)rowc * a.ldh1;
    const float *wcol = P + ((long long)h * a.Np + n0 + l31) * 4;
    // groups i0 .. i0 + 3 of this wave (group w + 4 i of the contraction): units 8 g + 4 h .. + 3 of the lane's row, the same units of its
    // column.  hidden1 % 4 == 0: a float4 lies wholly inside the row's units or wholly beyond them (W2's rows there are zero; H1's are not
    // this row's any more: the request goes to the row's start and the value is dropped)
    auto fetch = [&](int i0, float4 (&fa)[4], float4 (&fb)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u < NG ? i0 + u : 0, g = w + 4 * i, k = 8 * g + 4 * h;
            const bool ok = i0 + u < NG && k < a.K;
            fa[u] = *reinterpret_cast<const float4 *>(hrow + (ok ? k : 0));
            fb[u] = *reinterpret_cast<const float4 *>(wcol + (long long)(2 * g) * a.Np * 4);
            if (!ok) fa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    auto block = [&](int i0, const float4 (&fa)[4], const float4 (&fb)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < NG) {   // (wave-uniform)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(fa[u], e), f4e(fb[u], e), acc, 0, 0, 0);
            }
        }
    };
    float4 a0[4], b0[4], a1[4], b1[4];
    fetch(0, a0, b0);
    // epilogue operands: the bias group of this thread's four columns, its element of the head kernel [h2][A]
    const int hc = tid >> 5, hcol = n0 + (tid & 31);
    const bool whok = hc < a.A && hcol < a.h2;
    const float4 b4 = *reinterpret_cast<const float4 *>(P + a.b2_off + n0 + 4 * hc);
    const float whv = P[a.w3_off + (whok ? hcol * a.A + hc : 0)];
    for (int i0 = 0; i0 < NG; i0 += 8) {
        if (i0 + 4 < NG) fetch(i0 + 4, a1, b1);
        block(i0, a0, b0);
        if (i0 + 4 < NG) {
            if (i0 + 8 < NG) fetch(i0 + 8, a0, b0);
            block(i0 + 4, a1, b1);
        }
    }
    // split-K combine, bias + relu, H2 in the layouts its consumers read, head partials (the order of k_qfwd's epilogue)
    const int r = tid & 31, cg = tid >> 5;
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
    __syncthreads();
    s_wh[hc][tid & 31] = whok ? whv : 0.f;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * cg + e;
        const float s = ((red[0][r][c] + red[1][r][c]) + red[2][r][c]) + red[3][r][c];
        v[e] = fmaxf(s + f4e(b4, e), 0.f);
    }
    if (jb.H2c4) st_img(jb.H2c4 + ((long long)(n0 / 4 + cg) * a.Bp + m0 + r) * 4, make_float4(v[0], v[1], v[2], v[3]));
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) red[0][r][4 * cg + e] = v[e];
    __syncthreads();
    if (jb.H2r4) {   // (column hidden2 of the image is the ones column: never written here)
        const int c = tid & 31, rg = tid >> 5;
        if (n0 + c < a.h2)
            st_img(jb.H2r4 + ((long long)(m0 / 4 + rg) * a.Lp2 + n0 + c) * 4,
                   make_float4(red[0][4 * rg][c], red[0][4 * rg + 1][c], red[0][4 * rg + 2][c], red[0][4 * rg + 3][c]));
    }
    if (cg < a.A) {
        float s = 0.f;
#pragma unroll
        for (int col = 0; col < 32; ++col) s = fmaf(red[0][r][col], s_wh[cg][col], s);
        jb.hp[((long long)cg * a.Bp + m0 + r) * DNT + nt] = s;
    }
}

// ==========================================================================================
// launch 2: rows + layer-2 dgrad into the row-major dZ1
// ==========================================================================================
// Tile t < ntiles: rows m0 x units k0 of network n's dgrad.  Block ntiles: the W3 snapshot and the cleared words.
__global__ void __launch_bounds__(256) k_qtmid(QBArgs a, QTX x, int ntiles) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == ntiles) {
        for (int n = 0; n < a.nnet; ++n)
            for (int i = tid; i < (a.h2 + 1) * a.A; i += 256) a.w3snap[n * DX_W3S + i] = a.slab[a.main_off + n * a.PN + a.w3_off + i];
        for (int i = tid; i < x.n_zero; i += 256) x.zero_words[i] = 0;
        return;
    }
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ float s_q[DX_MAXEV][DFH][32];
    __shared__ float s_dq[2][32], s_loss[32];
    __shared__ int s_ai[32];
    __shared__ float s_w3[512 * DFH];
    int t = blockIdx.x;
    const int per = a.tiles_m * a.ct, n = t / per;
    t -= n * per;
    const int kt = t / a.tiles_m, mt = t - kt * a.tiles_m, m0 = mt * 32, k0 = kt * 32;
    const int lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *P = a.slab + a.main_off + n * a.PN;
    // the relu mask of this thread's four outputs (rows m0 + 4 rg + e of unit k0 + c), requested in front of everything else
    const int c = tid & 31, rg = tid >> 5, kc = k0 + c < a.h1 ? k0 + c : a.h1 - 1;
    float mk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = m0 + 4 * rg + e;
        mk[e] = x.H1[n][(long long)(row < a.B ? row : a.B - 1) * x.ldh1 + kc];
    }
    for (int i = tid; i < a.h2 * a.A; i += 256) s_w3[i] = P[a.w3_off + i];
    q_rows(a, m0, s_q, s_dq, s_ai, s_loss);
    if (n == 0 && kt == 0) {   // what the row tile leaves for the last launch and for the caller
        if (tid < 32) {
            const int row = m0 + tid;
            a.dq[row] = s_dq[0][tid]; a.dq[a.Bp + row] = s_dq[1][tid]; a.ai[row] = s_ai[tid];
        }
        for (int i = tid; i < 32 * a.A; i += 256) {
            const int r = i / a.A, cc = i - r * a.A;
            if (m0 + r < a.B) a.qrows[(long long)(m0 + r) * a.A + cc] = s_q[0][cc][r];
        }
        if (tid == 0) {
            float p = 0.f;
            for (int r = 0; r < 32; ++r) p += s_loss[r];
            a.part[mt] = p;
        }
    }
    // dZ1[row][k] = sum_j dZ2[row][j] W2[k][j]: the contraction (hidden2) in 8-deep groups over the waves; A generated from H2c4
    const float dqr = s_dq[n][l31];
    const int ar = s_ai[l31];
    const float *hc4 = a.H2c4[n] + (long long)(m0 + l31) * 4, *wd = P + a.w2d_off + (long long)(k0 + l31) * 4;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int G = a.Np >> 3;
#pragma unroll 4
    for (int g = w; g < G; g += 4) {
        const float4 hv = *reinterpret_cast<const float4 *>(hc4 + (long long)(2 * g + h) * a.Bp * 4);
        const float4 bv = *reinterpret_cast<const float4 *>(wd + (long long)(2 * g + h) * a.Kp * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 8 * g + 4 * h + e;
            const float wv = s_w3[(j < a.h2 ? j : a.h2 - 1) * a.A + ar];
            const float av = (f4e(hv, e) > 0.f && j < a.h2) ? dqr * wv : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, f4e(bv, e), acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
    __syncthreads();
    float *out = x.dZ1 + (long long)n * a.B * a.h1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // one row of 32 consecutive units per half-wave store
        const int row = m0 + 4 * rg + e;
        const float s = ((red[0][4 * rg + e][c] + red[1][4 * rg + e][c]) + red[2][4 * rg + e][c]) + red[3][4 * rg + e][c];
        if (row < a.B && k0 + c < a.h1) out[(long long)row * a.h1 + k0 + c] = mk[e] > 0.f ? s : 0.f;
    }
}

// ==========================================================================================
// launch 3: layer-2 and head weight gradients, Adam + polyak, the loss mean
// ==========================================================================================
// Per network: mt2 * nt2 tiles of the layer-2 wgrad (hidden1 + 1 rows: the bias), ht workgroups of the head wgrad; the last block: the loss mean.
__global__ void __launch_bounds__(256) k_qtlast(QBArgs a, QTX x, int mt2, int ht) {
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ float s_dq[512];
    __shared__ int s_ai[512];
    __shared__ float s_w3[512 * DFH];
    const int tid = threadIdx.x;
    const int per = mt2 * a.nt2 + ht;
    int t = blockIdx.x;
    if (t == a.nnet * per) {   // the loss mean, row tiles in order
        if (tid == 0) {
            float tot = 0.f;
            for (int b = 0; b < a.tiles_m; ++b) tot += a.part[b];
            const float l = (0.5f / (float)a.B) * tot;
            a.loss_out[0] = l;
            if (a.loss_out2) a.loss_out2[0] = l;
        }
        return;
    }
    const int n = t / per;
    t -= n * per;
    // this update's step size from the powers as they stand (ApplyAdam; k_adam_polyak's expression): the layer-1 launch advances them
    const float al = a.lr * sqrtf(1.0f - x.opt->b2p_q) / (1.0f - x.opt->b1p_q);
    const long long nb = (long long)n * a.PN;
    for (int i = tid; i < a.Bp; i += 256) { s_dq[i] = a.dq[n * a.Bp + i]; s_ai[i] = a.ai[i]; }
    if (t >= mt2 * a.nt2) {
        __syncthreads();
        w3_wgrad_step(a, n, t - mt2 * a.nt2, s_dq, s_ai, al);
        return;
    }
    // [dW2 ; db2] = [H1 | 1]^T dZ2, both W2 images: A out of the row-major H1 (rows beyond the batch repeat the last one: their dZ2 is zero),
    // B = dZ2 generated from the H2r4 image (its relu mask), dq, the action rows and the W3 snapshot in LDS
    for (int i = tid; i < a.h2 * a.A; i += 256) s_w3[i] = a.w3snap[n * DX_W3S + i];
    __syncthreads();
    const int it = t / a.nt2, i0 = it * 32, j0 = (t - it * a.nt2) * 32;
    const int lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *hcol = x.H1[n] + (i0 + l31 <= a.h1 ? i0 + l31 : a.h1);
    const float *Bimg = a.H2r4[n] + (long long)(j0 + l31) * 4;
    const int G = a.Bp >> 3, jn = j0 + l31, jc = jn < a.h2 ? jn : a.h2 - 1;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int g = w; g < G; g += 4) {
        const int r0 = 8 * g + 4 * h;
        float av[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = hcol[(long long)(r0 + e < a.B ? r0 + e : a.B - 1) * x.ldh1];
        const float4 bv = *reinterpret_cast<const float4 *>(Bimg + (long long)(2 * g + h) * a.Lp2 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float wv = s_w3[jc * a.A + s_ai[r0 + e]];
            const float b = (f4e(bv, e) > 0.f && jn < a.h2) ? s_dq[r0 + e] * wv : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
    __syncthreads();
    const int j = tid & 31, ig = tid >> 5;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = 4 * ig + e, k = i0 + i, c = j0 + j;
        const float g = ((red[0][i][j] + red[1][i][j]) + red[2][i][j]) + red[3][i][j];
        if (c < a.h2 && k <= a.h1) {
            const long long idx = nb + (k < a.h1 ? a.w2f_off + ((long long)(k >> 2) * a.Np + c) * 4 + (k & 3) : a.b2_off + c);
            const float p = step1(a, idx, g, al);
            if (k < a.h1) a.slab[a.main_off + nb + a.w2d_off + ((long long)(c >> 2) * a.Kp + k) * 4 + (c & 3)] = p;
        }
    }
}

}  // namespace

struct ddrl_dqn_tx {
    int device;
    ddrl_dqn_config_t cfg;
    int nnet, nsegs, nsegs_ext;      // segments in all; those an export walks (the dgrad image is a second home of W2)
    float *slab;
    float *buf[5];                   // main, target, m, v, gradient
    Seg *segs_d, *shadow_d;          // external order <-> direct layout; generic layout <- direct layout (ext = the generic offset)
    QTFArgs F;
    QBArgs Bk;
    QTX X;
    int fwd_tiles, mid_tiles, last_tiles, mt2, ht;
};

int ddrl_dqn_tx_check(const ddrl_dqn_config_t *c) {
    const char *why = nullptr;
    if (c->variant != DDRL_DDQN && c->variant != DDRL_SQN) why = "variant must be DDRL_DDQN or DDRL_SQN";
    else if (c->variant == DDRL_SQN && !(c->alpha > 0.0)) why = "DDRL_SQN needs alpha > 0";
    else if (c->obs_dim <= DDRL_DQN_DIRECT_MAX_OBS_DIM) why = "obs_dim <= 13 belongs to ddrl_dqn_create_direct (its layer 1 is generated on the matrix cores)";
    else if (c->n_actions < 1 || c->n_actions > DFH) why = "n_actions outside [1, 8] (head slots per evaluation)";
    else if (c->hidden1 < 4 || c->hidden2 < 4 || c->hidden1 % 4 || c->hidden2 % 4) why = "hidden sizes must be positive multiples of 4";
    else if (c->hidden1 > 512 || c->hidden2 > 32 * DNT) why = "hidden sizes over 512";
    else if (c->batch < 1 || c->batch > 4 * DGMAX * 8) why = "batch outside [1, 512] (a wgrad tile contracts the whole batch)";
    if (!why) return DDRL_OK;
    ddrl::set_error("ddrl_dqn_create_direct_tail: %s", why);
    return DDRL_ERR_UNSUPPORTED;
}

int ddrl_dqn_tx_create(ddrl_dqn_tx **out, int device, const ddrl_dqn_config_t *cfg, const ddrl_dqn_tx_bind *bind) {
    if (const int rc = ddrl_dqn_tx_check(cfg)) return rc;
    ddrl_dqn_tx *d = new ddrl_dqn_tx();
    d->device = device; d->cfg = *cfg;
    const int B = cfg->batch, o = cfg->obs_dim, A = cfg->n_actions, h1 = cfg->hidden1, h2 = cfg->hidden2;
    const bool sqn = cfg->variant == DDRL_SQN;
    const int nnet = d->nnet = sqn ? 2 : 1, nev = sqn ? 5 : 3;
    const int Bp = rup32(B), Kp = rup32(h1), Np = rup32(h2), Lp2 = Np + 32, nt2 = Np / 32, ct = Kp / 32, tiles_m = Bp / 32;
    const int w2f_off = 0, b2_off = Kp * Np, w3_off = b2_off + Np, w2d_off = w3_off + (int)pad4((long long)(h2 + 1) * A);
    const int PN = (w2d_off + Np * Kp + 63) & ~63;
    std::vector<Seg> segs, dup, shadow;
    const long long per_ext = (long long)o * h1 + h1 + (long long)h1 * h2 + h2 + (long long)h2 * A + A;
    for (int n = 0; n < nnet; ++n) {
        const long long nb = (long long)n * PN;
        long long ext = n * per_ext + (long long)o * h1 + h1;   // ([W1 ; b1] stay in the handle's generic buffers)
        segs.push_back(Seg{ext, nb + w2f_off, (long long)h1 * h2, h2, Np, 1, 0});
        dup.push_back(Seg{ext, nb + w2d_off, (long long)h1 * h2, h2, Kp, DX_SEG_W2D, 0}); ext += (long long)h1 * h2;
        segs.push_back(Seg{ext, nb + b2_off, h2, 0, 0, 0, 0}); ext += h2;
        segs.push_back(Seg{ext, nb + w3_off, (long long)h2 * A + A, 0, 0, 0, 0});   // (W3 and b3 are neighbours in every order)
        for (int k = 0; k < 3; ++k) {
            Seg sh = segs[segs.size() - 3 + k];
            sh.ext = bind->gen_off[n][k];
            shadow.push_back(sh);
        }
    }
    d->nsegs_ext = (int)segs.size();
    segs.insert(segs.end(), dup.begin(), dup.end());
    d->nsegs = (int)segs.size();
    size_t fl = 0;
    auto reserve = [&](size_t cnt) { const size_t off = fl; fl += (cnt + 63) & ~(size_t)63; return off; };
    const size_t NT = (size_t)nnet * PN;
    size_t o_buf[5];
    for (int k = 0; k < 5; ++k) o_buf[k] = reserve(NT);
    const long long HP = (long long)DFH * Bp * DNT;
    const size_t o_hp = reserve((size_t)nev * HP), o_H2c = reserve((size_t)2 * Np * Bp), o_H2r = reserve((size_t)2 * Bp * Lp2), o_dq = reserve((size_t)2 * Bp),
                 o_ai = reserve(Bp), o_q = reserve((size_t)B * A), o_part = reserve(tiles_m), o_snap = reserve((size_t)2 * DX_W3S),
                 o_segs = reserve((segs.size() * sizeof(Seg) + 3) / 4), o_shadow = reserve((shadow.size() * sizeof(Seg) + 3) / 4);
    (void)reserve(256);
    hipError_t e = hipMalloc((void **)&d->slab, fl * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d->slab, 0, fl * sizeof(float));
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc of %zu bytes failed in ddrl_dqn_create_direct_tail: %s", fl * sizeof(float), hipGetErrorString(e));
        delete d;
        return DDRL_ERR_NOMEM;
    }
    float *S = d->slab;
    for (int k = 0; k < 5; ++k) d->buf[k] = S + o_buf[k];
    d->segs_d = reinterpret_cast<Seg *>(S + o_segs);
    d->shadow_d = reinterpret_cast<Seg *>(S + o_shadow);
    hipError_t ec = hipMemcpy(d->segs_d, segs.data(), segs.size() * sizeof(Seg), hipMemcpyHostToDevice);
    if (ec == hipSuccess) ec = hipMemcpy(d->shadow_d, shadow.data(), shadow.size() * sizeof(Seg), hipMemcpyHostToDevice);
    for (int n = 0; n < 2; ++n) k_dx_ones<<<(Bp + 255) / 256, 256>>>(S + o_H2r + (size_t)n * Bp * Lp2, Bp, Lp2, h2);
    if (ec == hipSuccess) ec = hipGetLastError();
    if (ec == hipSuccess) ec = hipDeviceSynchronize();
    if (ec != hipSuccess) {
        ddrl::set_error("ddrl_dqn_create_direct_tail: %s", hipGetErrorString(ec));
        ddrl_dqn_tx_destroy(d);
        return DDRL_ERR_HIP;
    }
    // evaluations (parameter copy, network): DDQN q(x), q(x2), q_targ(x2); SQN q1(x), q1(x2), q2(x), q1_targ(x2), q2_targ(x2) — the order of the
    // handle's H1 image
    const int targ[5] = {0, 0, sqn ? 0 : 1, 1, 1}, net[5] = {0, 0, sqn ? 1 : 0, 0, 1};
    const int gev[2] = {0, 2};
    const long long BH1 = (long long)B * bind->ldh1;
    d->mt2 = (h1 + 1 + 31) / 32; d->ht = (h2 + 1 + 31) / 32;
    d->fwd_tiles = nev * tiles_m * nt2; d->mid_tiles = nnet * tiles_m * ct; d->last_tiles = nnet * (d->mt2 * nt2 + d->ht) + 1;
    QTFArgs &F = d->F;
    F = QTFArgs{};
    F.slab = S; F.ldh1 = bind->ldh1; F.B = B; F.Bp = Bp; F.K = h1; F.NG = Kp / 32; F.Np = Np; F.h2 = h2; F.A = A; F.tiles_m = tiles_m; F.tiles_n = nt2; F.Lp2 = Lp2;
    F.b2_off = b2_off; F.w3_off = w3_off;
    QBArgs &Q = d->Bk;
    Q = QBArgs{};
    QTX &X = d->X;
    X = QTX{};
    for (int ev = 0; ev < nev; ++ev) {
        QTJob &j = F.job[ev];
        j.w_off = (int)(o_buf[targ[ev]] + (size_t)net[ev] * PN); j.H1 = bind->H1 + ev * BH1; j.hp = S + o_hp + ev * HP;
        Q.b3_abs[ev] = j.w_off + w3_off + h2 * A;
    }
    for (int n = 0; n < nnet; ++n) {
        QTJob &j = F.job[gev[n]];
        j.H2c4 = S + o_H2c + (size_t)n * Np * Bp; j.H2r4 = S + o_H2r + (size_t)n * Bp * Lp2;
        Q.H2c4[n] = j.H2c4; Q.H2r4[n] = j.H2r4; X.H1[n] = j.H1;
    }
    X.dZ1 = bind->dZ1; X.ldh1 = bind->ldh1;
    Q.slab = S; Q.hp = S + o_hp;
    Q.dq = S + o_dq; Q.qrows = S + o_q; Q.part = S + o_part; Q.w3snap = S + o_snap; Q.ai = reinterpret_cast<int *>(S + o_ai);
    Q.loss_out = bind->loss;
    Q.B = B; Q.Bp = Bp; Q.h1 = h1; Q.h2 = h2; Q.Kp = Kp; Q.Np = Np; Q.A = A; Q.Lp2 = Lp2; Q.nnet = nnet; Q.nev = nev; Q.sqn = sqn ? 1 : 0;
    Q.tiles_m = tiles_m; Q.ct = ct; Q.nt2 = nt2;
    Q.PN = PN; Q.main_off = (int)o_buf[0]; Q.targ_off = (int)o_buf[1]; Q.m_off = (int)o_buf[2]; Q.v_off = (int)o_buf[3]; Q.g_off = (int)o_buf[4];
    Q.w2f_off = w2f_off; Q.b2_off = b2_off; Q.w3_off = w3_off; Q.w2d_off = w2d_off;
    Q.lr = (float)cfg->lr; Q.b1 = (float)cfg->beta1; Q.b2 = (float)cfg->beta2; Q.eps = (float)cfg->adam_eps;
    Q.pk = (float)cfg->polyak; Q.pk1 = (float)(1.0 - cfg->polyak); Q.gamma = (float)cfg->gamma; Q.alpha = (float)cfg->alpha;
    *out = d;
    return DDRL_OK;
}

void ddrl_dqn_tx_destroy(ddrl_dqn_tx *d) {
    if (!d) return;
    (void)hipFree(d->slab);
    delete d;
}

static float *tx_buffer(ddrl_dqn_tx *d, int which) {
    return which == DDRL_SAC1_MAIN ? d->buf[0] : which == DDRL_SAC1_TARGET ? d->buf[1] : which == DDRL_SAC1_ADAM_M ? d->buf[2] :
           which == DDRL_SAC1_ADAM_V ? d->buf[3] : which == DDRL_SAC1_GRAD ? d->buf[4] : nullptr;
}

int ddrl_dqn_tx_pack(ddrl_dqn_tx *d, int which, const float *flat_d, bool and_target, hipStream_t s) {
    float *dst = tx_buffer(d, which);
    DDRL_REQUIRE(dst != nullptr && which != DDRL_SAC1_GRAD, "unknown or read-only buffer id");
    k_dx_pack<<<dim3(64, (unsigned)d->nsegs), 256, 0, s>>>(d->segs_d, flat_d, dst, and_target ? d->buf[1] : nullptr, 1);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_dqn_tx_unpack(ddrl_dqn_tx *d, int which, float *flat_d, hipStream_t s) {
    const float *src = tx_buffer(d, which);
    DDRL_REQUIRE(src != nullptr, "unknown buffer id");
    k_dx_pack<<<dim3(64, (unsigned)d->nsegs_ext), 256, 0, s>>>(d->segs_d, src, flat_d, nullptr, 0);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_dqn_tx_shadow(ddrl_dqn_tx *d, float *generic_main, hipStream_t s) {
    k_dx_pack<<<dim3(64, (unsigned)d->nsegs_ext), 256, 0, s>>>(d->shadow_d, d->buf[0], generic_main, nullptr, 0);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_dqn_tx_fwd_mid(ddrl_dqn_tx *d, const float *acts, const float *rew, const float *done, int *zero_words, int n_zero, hipStream_t s) {
    QBArgs Q = d->Bk;
    Q.acts = acts; Q.rew = rew; Q.done = done;
    QTX X = d->X;
    X.zero_words = zero_words; X.n_zero = zero_words ? n_zero : 0;
    k_qtfwd<<<d->fwd_tiles, 256, 0, s>>>(d->F);
    k_qtmid<<<d->mid_tiles + 1, 256, 0, s>>>(Q, X, d->mid_tiles);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_dqn_tx_last(ddrl_dqn_tx *d, const void *opt, float *loss_d, hipStream_t s) {
    QBArgs Q = d->Bk;
    Q.loss_out2 = loss_d;
    QTX X = d->X;
    X.opt = static_cast<const OptState *>(opt);
    k_qtlast<<<d->last_tiles, 256, 0, s>>>(Q, X, d->mt2, d->ht);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

const float *ddrl_dqn_tx_qrows(ddrl_dqn_tx *d) { return d->Bk.qrows; }
