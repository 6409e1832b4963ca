// The direct-operand update of a narrow Double-DQN / soft-Q learner (ddrl_dqn_create_direct, include/ddrl_dqn_direct.h): three launches.
//   k_qfwd   every evaluation (DDQN: q(x), q(x2), q_targ(x2); SQN: q1(x), q1(x2), q2(x), q1_targ(x2), q2_targ(x2)) as a job: layer 1
//            generated transposed on v_mfma_f32_32x32x2_f32 from the lane's observation row, relu in registers, layer 2 straight from
//            the k4-interleaved W2 (sac1_direct.h: dkloop, the K loop of k_dfwd), head partials of n_actions outputs into hp[DFH][B][DNT];
//            the differentiated evaluations leave H1r4 / H2c4 / H2r4 and the input-row image, spread as h1_owned / side_aug_tile spread them.
//   k_qmid   per workgroup the row prologue (head partials summed in column-tile order + b3, the reference's row logic — head_body's
//            statements of dqn.hip —, dq per row) and a tile of the dgrad dZ1 = dZ2 W2^T .* (H1 > 0) whose A operand is generated in the
//            tile: dZ2 = dq[row] * W3[j][a_row] * (H2 > 0); + loss partials, q rows, dq / action rows for the last launch, the W3
//            snapshot and the optimizer's books (one workgroup), and the next update's sampler workgroup (dqn_sample.h).
//   k_qlast  every weight gradient with Adam + polyak in its epilogue: [x | 1]^T dZ1 over the input-row image into the layer-1 block
//            array, H1^T dZ2 (dZ2 generated again, from the W3 snapshot) into BOTH k4-interleaved W2 images, [H2 | 1]^T dQ; the batch
//            contracted in 8-deep groups over the four waves, fixed-order LDS combine; + the loss mean in workgroup order.
// The layer-2 and head wgrads step W2 / W3, which the dgrad and the generated dZ2 read: they run in the launch BEHIND the dgrad (SAC1's
// "mid" launch double-buffers the dgrad image instead, and a learner loop alternates its copies per update; an eager ddrl_dqn_step
// has no such alternation), and the head kernel they generate from is the snapshot k_qmid took.  Every cross-workgroup sum has a fixed
// order; no flat optimizer launch, no head-dgrad launch, no dZ2 image.
// Layout of a network inside main / target / m / v / gradient (sac1_layout.h's direct layout for an observation-only network with an
// n_actions-wide head): [W1 ; b1] block array (w1y_index) | W2 [Kp/4][Np][4] | b2 [Np] | [W3 ; b3] [h2 + 1][A] | W2 dgrad image [Np/4][Kp][4].
#include "gemm_core.h"
#include "policy_row.h"
#include "dqn_direct.h"
#include "../../include/ddrl_dqn_direct.h"

namespace {
#include "sac1_direct.h"
#include "dqn_sample.h"
#include "dqn_direct_shared.h"   // the segment kinds, k_dx_pack, QBArgs, q_rows, step1, w3_wgrad_step: shared with dqn_direct_tail.hip

// ==========================================================================================
// launch 1: forward
// ==========================================================================================
struct QFJob {
    int w_off, x2;           // the network's [W1 ; b1] block array inside the slab; the job reads obs2
    float *hp;               // head partials [DFH][Bp][DNT]
    float *H1r4, *H2c4, *H2r4, *xr4;   // side outputs of a differentiated evaluation (nullable)
};
struct QFArgs {
    const float *slab, *x1, *x2;
    int ldx, d0, B, Bp, K, Np, h2, A, tiles_m, tiles_n, Lp1, Lp2, b2_off, w3_off;
    QFJob job[DX_MAXEV];
};
template <int NS>
__global__ void __launch_bounds__(256) k_qfwd(QFArgs a) {
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float tr[4][32 * 36];
    __shared__ float s_wh[DFH][32];
    const int tpj = a.tiles_m * a.tiles_n;
    int t = blockIdx.x;
    const int ji = t / tpj;
    t -= ji * tpj;
    const int nt = t / a.tiles_m, m0 = (t - nt * a.tiles_m) * 32, n0 = nt * 32;
    const QFJob &jb = a.job[ji];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int K = a.K, Np = a.Np;
    const float *W1 = a.slab + jb.w_off, *W2p = W1 + ((K + 31) & ~31) * 16;
    // this wave's 32-unit blocks: the waves at the END get the extra (possibly partial) block (as k_dfwd)
    const int nblk = (K + 31) >> 5, bs = nblk >> 2, rem = nblk & 3;
    const int nb = bs + (w >= 4 - rem ? 1 : 0);
    const int b0 = w * bs + (w > 4 - rem ? w - (4 - rem) : 0);
    // the layer-1 input: lane (row, h) holds input column d_slot(s, h) for step s; column d0 of the row is the physical 1 of the bias
    const int rowc = m0 + l31 < a.B ? m0 + l31 : a.B - 1;   // rows of the last tile beyond the batch repeat its last row (they carry dq = 0)
    const float *xrow = (jb.x2 ? a.x2 : a.x1) + (long long)rowc * a.ldx;
    float xin[1][7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int d = d_slot(s, h);
        const float v = xrow[d <= a.d0 ? d : 0];
        xin[0][s] = d <= a.d0 ? v : 0.f;
    }
    DOps ops;
    const DSrc src{W1, W2p, Np, b0, nb, n0};
    constexpr int PRE = DDRL_DPRE0;
#pragma unroll
    for (int bi = 0; bi < PRE; ++bi) dops_load_block(ops, src, bi, lane);
    // epilogue operands: the bias group of this thread's four columns, its element of the head kernel [h2][A]
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float whv = 0.f;
    const float *b2p = W1 + a.b2_off + n0 + 4 * (tid >> 5);
    const int hc = tid >> 5, hcol = n0 + (tid & 31);
    const bool whok = hc < a.A && hcol < a.h2;
    const int who = a.w3_off + (whok ? hcol * a.A + hc : 0);
    auto epilogue_operands = [&]() {
        b4 = *reinterpret_cast<const float4 *>(b2p);
        whv = W1[who];
    };
    if (DDRL_DMID == -2) epilogue_operands();
    floatx16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
    float *h1r4 = jb.H1r4;
    const int h1own = h1r4 ? h1_owned(b0, nb, nt, a.tiles_n) : 0;
    dkloop<NS, 1, PRE>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
    // the input-row image [row / 4][32][4] of the layer-1 wgrad, one column tile of the row tile (rows beyond the batch: zero)
    if (jb.xr4 && nt == side_aug_tile(a.tiles_n)) {
        const int D1 = a.d0 + 1;
        for (int idx = tid; idx < 32 * D1; idx += 256) {
            const int r = idx / D1, d = idx - r * D1, row = m0 + r;
            const float v = row < a.B ? a.x1[(long long)row * a.ldx + d] : 0.f;
            jb.xr4[((long long)(row >> 2) * 32 + d) * 4 + (row & 3)] = v;
        }
    }
    // split-K combine, bias + relu, H2 in the layouts its consumers read, head partials (the order of k_dfwd's epilogue)
    const int r = tid & 31, cg = tid >> 5;
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[0][q];
    __syncthreads();
    s_wh[tid >> 5][tid & 31] = whok ? whv : 0.f;
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
// launches 2 and 3: backward
// ==========================================================================================
// Tile t < ntiles: rows m0 x units k0 of network n's dgrad.  Block ntiles: the W3 snapshot and the optimizer's books.  Block ntiles + 1
// (launched when the next update's draw rides here): the sampler.
__global__ void __launch_bounds__(256) k_qmid(QBArgs a, SetSampler m, int ntiles) {
    if ((int)blockIdx.x == ntiles + 1) { sample_into_set(m); return; }
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == ntiles) {
        for (int n = 0; n < a.nnet; ++n)
            for (int i = tid; i < (a.h2 + 1) * a.A; i += 256) a.w3snap[n * DX_W3S + i] = a.slab[a.main_off + n * a.PN + a.w3_off + i];
        if (tid == 0) {   // this update's step size from the powers as they stand (ApplyAdam), then the powers of the next one
            DxOpt o = *a.opt;
            o.al = a.lr * sqrtf(1.0f - o.b2p) / (1.0f - o.b1p);
            o.b1p *= a.b1; o.b2p *= a.b2; o.t += 1;
            *a.opt = o;
        }
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
    for (int i = tid; i < a.h2 * a.A; i += 256) s_w3[i] = P[a.w3_off + i];
    q_rows(a, m0, s_q, s_dq, s_ai, s_loss);
    if (n == 0 && kt == 0) {   // what the row tile leaves for the last launch and for the caller
        if (tid < 32) {
            const int row = m0 + tid;
            a.dq[row] = s_dq[0][tid]; a.dq[a.Bp + row] = s_dq[1][tid]; a.ai[row] = s_ai[tid];
        }
        for (int i = tid; i < 32 * a.A; i += 256) {
            const int r = i / a.A, c = i - r * a.A;
            if (m0 + r < a.B) a.qrows[(long long)(m0 + r) * a.A + c] = s_q[0][c][r];
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
    {   // relu mask of H1, the image the layer-1 wgrad reads: [row / 4][unit][4]
        const int c = tid & 31, rg = tid >> 5;
        const long long off = ((long long)(m0 / 4 + rg) * a.Lp1 + k0 + c) * 4;
        const float4 mk = *reinterpret_cast<const float4 *>(a.H1r4[n] + off);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = ((red[0][4 * rg + e][c] + red[1][4 * rg + e][c]) + red[2][4 * rg + e][c]) + red[3][4 * rg + e][c];
            v[e] = f4e(mk, e) > 0.f ? s : 0.f;
        }
        if (k0 + c < a.h1) *reinterpret_cast<float4 *>(a.dZ1r4[n] + off) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// One 32 x 32 tile C = A^T B contracted over the batch rows, both operands as [row / 4][column][4] images: wave w takes the 8-deep
// groups w, w + 4, ...; GEN: B = dZ2 generated from the H2r4 image (its relu mask), dq, the action rows and the W3 snapshot in LDS.
template <bool GEN>
__device__ __forceinline__ void wgrad_tile(const QBArgs &a, const float *Aimg, int lda, int i0, const float *Bimg, int ldb, int j0, const float *s_dq,
                                           const int *s_ai, const float *s_w3, float (&red)[4][32][33]) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int G = a.Bp >> 3, jn = j0 + l31, jc = jn < a.h2 ? jn : a.h2 - 1;
#pragma unroll 4
    for (int g = w; g < G; g += 4) {
        const float4 av = *reinterpret_cast<const float4 *>(Aimg + ((long long)(2 * g + h) * lda + i0 + l31) * 4);
        const float4 bv = *reinterpret_cast<const float4 *>(Bimg + ((long long)(2 * g + h) * ldb + j0 + l31) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float b = f4e(bv, e);
            if (GEN) {
                const int row = 8 * g + 4 * h + e;
                const float wv = s_w3[jc * a.A + s_ai[row]];
                b = (b > 0.f && jn < a.h2) ? s_dq[row] * wv : 0.f;
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(av, e), b, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
    __syncthreads();
}

// Per network: mt2 * nt2 tiles of the layer-2 wgrad (hidden1 + 1 rows: the bias), ct tiles of the layer-1 wgrad, ht workgroups of the
// head wgrad; the last block: the loss mean.
__global__ void __launch_bounds__(256) k_qlast(QBArgs a, int mt2, int ht) {
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ float s_dq[512];
    __shared__ int s_ai[512];
    __shared__ float s_w3[512 * DFH];
    const int tid = threadIdx.x;
    const int per = mt2 * a.nt2 + a.ct + ht;
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
    const float al = a.opt->al;
    const long long nb = (long long)n * a.PN;
    for (int i = tid; i < a.Bp; i += 256) { s_dq[i] = a.dq[n * a.Bp + i]; s_ai[i] = a.ai[i]; }
    const int j = tid & 31, ig = tid >> 5;
    if (t < mt2 * a.nt2) {          // [dW2 ; db2] = [H1 | 1]^T dZ2, both W2 images
        for (int i = tid; i < a.h2 * a.A; i += 256) s_w3[i] = a.w3snap[n * DX_W3S + i];
        __syncthreads();
        const int it = t / a.nt2, i0 = it * 32, j0 = (t - it * a.nt2) * 32;
        wgrad_tile<true>(a, a.H1r4[n], a.Lp1, i0, a.H2r4[n], a.Lp2, j0, s_dq, s_ai, s_w3, red);
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
        return;
    }
    t -= mt2 * a.nt2;
    if (t < a.ct) {                 // [dW1 ; db1] = [x | 1]^T dZ1 into the layer-1 block array
        __syncthreads();
        const int j0 = t * 32;
        wgrad_tile<false>(a, a.xr4, 32, 0, a.dZ1r4[n], a.Lp1, j0, s_dq, s_ai, s_w3, red);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 4 * ig + e, u = j0 + j;
            const float g = ((red[0][d][j] + red[1][d][j]) + red[2][d][j]) + red[3][d][j];
            if (d <= a.d0 && u < a.h1) step1(a, nb + w1y_index(d, u), g, al);
        }
        return;
    }
    t -= a.ct;
    __syncthreads();
    w3_wgrad_step(a, n, t, s_dq, s_ai, al);   // [dW3 ; db3] = [H2 | 1]^T dQ, dQ[row][c] = dq[row] (c == a_row): rows in order
}

}  // namespace

struct ddrl_dqn_dx {
    int device;
    ddrl_dqn_config_t cfg;
    int nnet, nsegs, nsegs_ext;      // segments in all; those an export walks (the dgrad image is a second home of W2)
    long long total_ext;
    float *slab, *flat;
    float *buf[5];                   // main, target, m, v, gradient
    Seg *segs_d;
    QFArgs F[2];                     // per input set
    QBArgs Bk[2];
    int fwd_tiles, mid_tiles, last_tiles, mt2, ht, ns;
};

int ddrl_dqn_dx_check(const ddrl_dqn_config_t *c) {
    const char *why = nullptr;
    if (c->variant != DDRL_DDQN && c->variant != DDRL_SQN) why = "variant must be DDRL_DDQN or DDRL_SQN";
    else if (c->variant == DDRL_SQN && !(c->alpha > 0.0)) why = "DDRL_SQN needs alpha > 0";
    else if (c->obs_dim < 1 || c->obs_dim > DDRL_DQN_DIRECT_MAX_OBS) why = "obs_dim outside [1, 13] (the narrow layer-1 generator holds 14 input columns, the bias among them)";
    else if (c->n_actions < 1 || c->n_actions > DFH) why = "n_actions outside [1, 8] (head slots per evaluation)";
    else if (c->hidden1 < 4 || c->hidden2 < 4 || c->hidden1 % 4 || c->hidden2 % 4) why = "hidden sizes must be positive multiples of 4";
    else if (c->hidden1 > 512 || c->hidden2 > 32 * DNT) why = "hidden sizes over 512";
    else if (c->batch < 1 || c->batch > 4 * DGMAX * 8) why = "batch outside [1, 512] (a wgrad tile contracts the whole batch)";
    if (!why) return DDRL_OK;
    ddrl::set_error("ddrl_dqn_create_direct: %s", why);
    return DDRL_ERR_UNSUPPORTED;
}

int ddrl_dqn_dx_create(ddrl_dqn_dx **out, int device, const ddrl_dqn_config_t *cfg, float *const sets[2][5], int ldx) {
    if (const int rc = ddrl_dqn_dx_check(cfg)) return rc;
    ddrl_dqn_dx *d = new ddrl_dqn_dx();
    d->device = device; d->cfg = *cfg;
    const int B = cfg->batch, o = cfg->obs_dim, A = cfg->n_actions, h1 = cfg->hidden1, h2 = cfg->hidden2;
    const bool sqn = cfg->variant == DDRL_SQN;
    const int nnet = d->nnet = sqn ? 2 : 1, nev = sqn ? 5 : 3;
    const int Bp = rup32(B), Kp = rup32(h1), Np = rup32(h2), Lp1 = Kp + 32, Lp2 = Np + 32, nt2 = Np / 32, ct = Kp / 32, tiles_m = Bp / 32;
    const int w2f_off = Kp * 16, b2_off = w2f_off + Kp * Np, w3_off = b2_off + Np, w2d_off = w3_off + (int)pad4((long long)(h2 + 1) * A);
    const int PN = (w2d_off + Np * Kp + 63) & ~63;
    std::vector<Seg> segs, dup;
    long long ext = 0;
    for (int n = 0; n < nnet; ++n) {
        const long long nb = (long long)n * PN;
        segs.push_back(Seg{ext, nb, (long long)o * h1, h1, 0, 2, 0}); ext += (long long)o * h1;
        segs.push_back(Seg{ext, nb, h1, h1, 0, 2, o}); ext += h1;
        segs.push_back(Seg{ext, nb + w2f_off, (long long)h1 * h2, h2, Np, 1, 0});
        dup.push_back(Seg{ext, nb + w2d_off, (long long)h1 * h2, h2, Kp, DX_SEG_W2D, 0}); ext += (long long)h1 * h2;
        segs.push_back(Seg{ext, nb + b2_off, h2, 0, 0, 0, 0}); ext += h2;
        segs.push_back(Seg{ext, nb + w3_off, (long long)h2 * A + A, 0, 0, 0, 0}); ext += (long long)h2 * A + A;   // (W3 and b3 are neighbours in both orders)
    }
    d->nsegs_ext = (int)segs.size();
    segs.insert(segs.end(), dup.begin(), dup.end());
    d->nsegs = (int)segs.size(); d->total_ext = ext;
    size_t fl = 0;
    auto reserve = [&](size_t cnt) { const size_t off = fl; fl += (cnt + 63) & ~(size_t)63; return off; };
    const size_t NT = (size_t)nnet * PN;
    size_t o_buf[5];
    for (int k = 0; k < 5; ++k) o_buf[k] = reserve(NT);
    const long long HP = (long long)DFH * Bp * DNT;
    const size_t o_hp = reserve((size_t)nev * HP), o_H1 = reserve((size_t)2 * Bp * Lp1), o_H2c = reserve((size_t)2 * Np * Bp), o_H2r = reserve((size_t)2 * Bp * Lp2),
                 o_dZ1 = reserve((size_t)2 * Bp * Lp1), o_xr4 = reserve((size_t)Bp * 32), o_dq = reserve((size_t)2 * Bp), o_ai = reserve(Bp),
                 o_q = reserve((size_t)B * A), o_part = reserve(tiles_m), o_snap = reserve((size_t)2 * DX_W3S), o_opt = reserve(16), o_loss = reserve(4),
                 o_flat = reserve((size_t)ext), o_segs = reserve((segs.size() * sizeof(Seg) + 3) / 4);
    (void)reserve(256);
    hipError_t e = hipMalloc((void **)&d->slab, fl * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d->slab, 0, fl * sizeof(float));
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc of %zu bytes failed in ddrl_dqn_create_direct: %s", fl * sizeof(float), hipGetErrorString(e));
        delete d;
        return DDRL_ERR_NOMEM;
    }
    float *S = d->slab;
    for (int k = 0; k < 5; ++k) d->buf[k] = S + o_buf[k];
    d->flat = S + o_flat;
    d->segs_d = reinterpret_cast<Seg *>(S + o_segs);
    DxOpt os{(float)cfg->beta1, (float)cfg->beta2, 0.f, 0};
    hipError_t ec = hipMemcpy(d->segs_d, segs.data(), segs.size() * sizeof(Seg), hipMemcpyHostToDevice);
    if (ec == hipSuccess) ec = hipMemcpy(S + o_opt, &os, sizeof(os), hipMemcpyHostToDevice);
    for (int n = 0; n < 2; ++n) {
        k_dx_ones<<<(Bp + 255) / 256, 256>>>(S + o_H1 + (size_t)n * Bp * Lp1, Bp, Lp1, h1);
        k_dx_ones<<<(Bp + 255) / 256, 256>>>(S + o_H2r + (size_t)n * Bp * Lp2, Bp, Lp2, h2);
    }
    if (ec == hipSuccess) ec = hipGetLastError();
    if (ec == hipSuccess) ec = hipDeviceSynchronize();
    if (ec != hipSuccess) {
        ddrl::set_error("ddrl_dqn_create_direct: %s", hipGetErrorString(ec));
        ddrl_dqn_dx_destroy(d);
        return DDRL_ERR_HIP;
    }
    // evaluations (input, parameter copy, network): DDQN q(x), q(x2), q_targ(x2); SQN q1(x), q1(x2), q2(x), q1_targ(x2), q2_targ(x2)
    const int x2of[5] = {0, 1, sqn ? 0 : 1, 1, 1}, targ[5] = {0, 0, sqn ? 0 : 1, 1, 1}, net[5] = {0, 0, sqn ? 1 : 0, 0, 1};
    const int gev[2] = {0, 2};
    d->ns = o + 1 <= 8 ? 4 : 4 + (o + 1 - 8 + 1) / 2;   // input columns + the bias column, two per MFMA step
    d->mt2 = (h1 + 1 + 31) / 32; d->ht = (h2 + 1 + 31) / 32;
    d->fwd_tiles = nev * tiles_m * nt2; d->mid_tiles = nnet * tiles_m * ct; d->last_tiles = nnet * (d->mt2 * nt2 + ct + d->ht) + 1;
    for (int st = 0; st < 2; ++st) {
        QFArgs &F = d->F[st];
        F = QFArgs{};
        F.slab = S; F.x1 = sets[st][0]; F.x2 = sets[st][1];
        F.ldx = ldx; F.d0 = o; F.B = B; F.Bp = Bp; F.K = h1; F.Np = Np; F.h2 = h2; F.A = A; F.tiles_m = tiles_m; F.tiles_n = nt2; F.Lp1 = Lp1; F.Lp2 = Lp2;
        F.b2_off = b2_off; F.w3_off = w3_off;
        QBArgs &Q = d->Bk[st];
        Q = QBArgs{};
        for (int ev = 0; ev < nev; ++ev) {
            QFJob &j = F.job[ev];
            j.w_off = (int)(o_buf[targ[ev]] + (size_t)net[ev] * PN); j.x2 = x2of[ev]; j.hp = S + o_hp + ev * HP;
            Q.b3_abs[ev] = j.w_off + w3_off + h2 * A;
        }
        for (int n = 0; n < nnet; ++n) {
            QFJob &j = F.job[gev[n]];
            j.H1r4 = S + o_H1 + (size_t)n * Bp * Lp1; j.H2c4 = S + o_H2c + (size_t)n * Np * Bp; j.H2r4 = S + o_H2r + (size_t)n * Bp * Lp2;
            Q.H1r4[n] = j.H1r4; Q.H2c4[n] = j.H2c4; Q.H2r4[n] = j.H2r4; Q.dZ1r4[n] = S + o_dZ1 + (size_t)n * Bp * Lp1;
        }
        F.job[0].xr4 = S + o_xr4;
        Q.slab = S; Q.hp = S + o_hp; Q.acts = sets[st][2]; Q.rew = sets[st][3]; Q.done = sets[st][4];
        Q.dq = S + o_dq; Q.qrows = S + o_q; Q.part = S + o_part; Q.w3snap = S + o_snap; Q.xr4 = S + o_xr4; Q.ai = reinterpret_cast<int *>(S + o_ai);
        Q.opt = reinterpret_cast<DxOpt *>(S + o_opt); Q.loss_out = S + o_loss;
        Q.B = B; Q.Bp = Bp; Q.h1 = h1; Q.h2 = h2; Q.Kp = Kp; Q.Np = Np; Q.A = A; Q.Lp1 = Lp1; Q.Lp2 = Lp2; Q.nnet = nnet; Q.nev = nev; Q.sqn = sqn ? 1 : 0;
        Q.tiles_m = tiles_m; Q.ct = ct; Q.nt2 = nt2; Q.d0 = o;
        Q.PN = PN; Q.main_off = (int)o_buf[0]; Q.targ_off = (int)o_buf[1]; Q.m_off = (int)o_buf[2]; Q.v_off = (int)o_buf[3]; Q.g_off = (int)o_buf[4];
        Q.w2f_off = w2f_off; Q.b2_off = b2_off; Q.w3_off = w3_off; Q.w2d_off = w2d_off;
        Q.lr = (float)cfg->lr; Q.b1 = (float)cfg->beta1; Q.b2 = (float)cfg->beta2; Q.eps = (float)cfg->adam_eps;
        Q.pk = (float)cfg->polyak; Q.pk1 = (float)(1.0 - cfg->polyak); Q.gamma = (float)cfg->gamma; Q.alpha = (float)cfg->alpha;
    }
    *out = d;
    return DDRL_OK;
}

void ddrl_dqn_dx_destroy(ddrl_dqn_dx *d) {
    if (!d) return;
    (void)hipFree(d->slab);
    delete d;
}

static float *dx_buffer(ddrl_dqn_dx *d, int which) {
    return which == DDRL_SAC1_MAIN ? d->buf[0] : which == DDRL_SAC1_TARGET ? d->buf[1] : which == DDRL_SAC1_ADAM_M ? d->buf[2] :
           which == DDRL_SAC1_ADAM_V ? d->buf[3] : which == DDRL_SAC1_GRAD ? d->buf[4] : nullptr;
}

int ddrl_dqn_dx_pack(ddrl_dqn_dx *d, int which, const float *flat_d, bool and_target, hipStream_t s) {
    float *dst = dx_buffer(d, which);
    DDRL_REQUIRE(dst != nullptr && which != DDRL_SAC1_GRAD, "unknown or read-only buffer id");
    k_dx_pack<<<dim3(64, (unsigned)d->nsegs), 256, 0, s>>>(d->segs_d, flat_d, dst, and_target ? d->buf[1] : nullptr, 1);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

const float *ddrl_dqn_dx_unpack(ddrl_dqn_dx *d, int which, float *flat_d, hipStream_t s) {
    const float *src = dx_buffer(d, which);
    if (!src) { ddrl::set_error("unknown buffer id"); return nullptr; }
    float *dst = flat_d ? flat_d : d->flat;
    k_dx_pack<<<dim3(64, (unsigned)d->nsegs_ext), 256, 0, s>>>(d->segs_d, src, dst, nullptr, 0);
    if (hipGetLastError() != hipSuccess) { ddrl::set_error("k_dx_pack failed to launch"); return nullptr; }
    return dst;
}

int ddrl_dqn_dx_update(ddrl_dqn_dx *d, int set, const void *ride, float *loss_d, hipStream_t s) {
    const QFArgs &F = d->F[set];
    QBArgs Q = d->Bk[set];
    Q.loss_out2 = loss_d;
    switch (d->ns) {
        case 4: k_qfwd<4><<<d->fwd_tiles, 256, 0, s>>>(F); break;
        case 5: k_qfwd<5><<<d->fwd_tiles, 256, 0, s>>>(F); break;
        case 6: k_qfwd<6><<<d->fwd_tiles, 256, 0, s>>>(F); break;
        default: k_qfwd<7><<<d->fwd_tiles, 256, 0, s>>>(F); break;
    }
    k_qmid<<<d->mid_tiles + (ride ? 2 : 1), 256, 0, s>>>(Q, ride ? *static_cast<const SetSampler *>(ride) : SetSampler{}, d->mid_tiles);
    k_qlast<<<d->last_tiles, 256, 0, s>>>(Q, d->mt2, d->ht);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

const float *ddrl_dqn_dx_qrows(ddrl_dqn_dx *d) { return d->Bk[0].qrows; }
