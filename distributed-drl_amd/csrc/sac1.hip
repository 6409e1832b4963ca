// SAC1 learner update on gfx950 (the batched policy forward of the Actor: actor.hip).
// Replaces Learner of algos/sac1/actor_learner.py:19-229 with the network of
// algos/sac1/core.py:91-121 (policy 8->400->300->(2,2), twin Q 10->400->300->1, ReLU).
//
// One update = 8 network evaluations (policy main@x, main@x2, target@x2; Q1,Q2 main@(x,a);
// Q1 main@(x,pi); Q1,Q2 target@(x2,pi_targ)), backward of pi_loss through Q1 and of value_loss,
// two TF1-Adam steps and the polyak update.  The dense fc work (hidden1 x hidden2 layers,
// forward / dgrad / wgrad) runs on the f32-input MFMA v_mfma_f32_32x32x2_f32, which is bit-exact
// f32 FMA arithmetic (no bf16: the 1e-5 loss parity forbids it); everything else is row-local
// VALU work with wavefront-shuffle reductions.  All stages of one update are launched
// back-to-back on one stream with no host synchronisation and no host-side state, so a whole
// update (or many) can be captured in a hipGraph.
//
// Numerics kept from the reference formulae (fp contraction is OFF for this file; FMAs are
// explicit): the only re-arrangement is z = eps*std/(std+EPS) for (pi-mu)/(std+EPS)
// (core.py:31 with pi = mu + eps*std, core.py:76-77) — algebraically identical, but free of the
// catastrophic cancellation that makes the literal float32 form noisy at the 1e-5 level
// (DESIGN.md §numerics).
#include "gemm_core.h"
#include "policy_row.h"

namespace {
#include "sac1_direct.h"
}  // namespace
#include "sac1_layout.h"

namespace {
// ------------------------------------------------------------------------------------------
// K: heads, stage A — one wave per (row, eval in {pi@x, pi@x2, piT@x2, q1(x,a), q2(x,a)})
// ------------------------------------------------------------------------------------------
struct RowsA {
    const float *H2;  // [NEVAL][B][ldh2]
    NetPi pi_main, pi_targ;
    NetQ q1, q2;
    const float *e0, *e1, *e2;
    float *act0, *act2, *logp0, *logp1, *save0, *q1o, *q2o;
    // second-phase layer 1 (Q at the freshly sampled actions): slots 5, 6, 7 of H1 hold the
    // observation part x*W1[:obs] + b1 (k_l1, pre_only); this kernel adds act*W1[obs:] and the relu
    float *H1;                           // [NEVAL][B][ldh1]
    const float *Wa_q1, *Wa_q1t, *Wa_q2t;  // action rows W1[obs:obs+act, :] of main q1, target q1, target q2
    int B, h2, ldh2, act, h1, ldh1;
    float scale;
};
__device__ __forceinline__ void finish_l1(float *hx, int h1, int act, const float *__restrict__ Wa, float act_lane, int lane) {
    // hx[j] = relu(hx[j] + sum_c act[c] * Wa[c*h1 + j]); first two action dims fetched together
    float v[RV], w0[RV], w1[RV];
    const int cB = act > 1 ? 1 : 0;
    load_row(hx, h1, lane, v);
    load_row(Wa, h1, lane, w0);
    load_row(Wa + (long long)cB * h1, h1, lane, w1);
    const float a0 = __shfl(act_lane, 0), a1 = act > 1 ? __shfl(act_lane, 1) : 0.f;
#pragma unroll
    for (int i = 0; i < RV; ++i) v[i] = fmaf(a1, w1[i], fmaf(a0, w0[i], v[i]));
#pragma unroll
    for (int c = 2; c < MAXA; ++c)
        if (c < act) {
            float w[RV];
            load_row(Wa + (long long)c * h1, h1, lane, w);
            const float ac = __shfl(act_lane, c);
#pragma unroll
            for (int i = 0; i < RV; ++i) v[i] = fmaf(ac, w[i], v[i]);
        }
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const int j = lane + 64 * i;
        if (j < h1) hx[j] = fmaxf(v[i], 0.f);
    }
}
__global__ void __launch_bounds__(256) k_rows_a(RowsA a) {
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= a.B * 5) return;
    const int e = wid / a.B, r = wid - e * a.B;
    float hrow[RV];
    load_row(a.H2 + ((long long)e * a.B + r) * a.ldh2, a.h2, lane, hrow);
    if (e < 3) {
        const NetPi &p = (e == 2) ? a.pi_targ : a.pi_main;
        const float *eps = (e == 0 ? a.e0 : (e == 1 ? a.e1 : a.e2)) + (long long)r * a.act;
        const float el = eps[lane < a.act ? lane : 0];
        mask_row(hrow, a.h2, lane);
        const HeadOut o = policy_head(hrow, a.h2, a.act, p, el, a.scale, lane);
        const long long BH1 = (long long)a.B * a.ldh1;
        if (e == 0) {
            if (lane < a.act) {
                a.act0[r * a.act + lane] = o.act;
                *reinterpret_cast<float4 *>(a.save0 + ((long long)r * a.act + lane) * 4) = make_float4(o.a, o.std, o.t, o.eps);
            }
            if (lane == 0) a.logp0[r] = o.logp;
            finish_l1(a.H1 + 5 * BH1 + (long long)r * a.ldh1, a.h1, a.act, a.Wa_q1, o.act, lane);   // q1(x, pi)
        } else if (e == 1) {
            if (lane == 0) a.logp1[r] = o.logp;
        } else {
            if (lane < a.act) a.act2[r * a.act + lane] = o.act;
            finish_l1(a.H1 + 6 * BH1 + (long long)r * a.ldh1, a.h1, a.act, a.Wa_q1t, o.act, lane);  // q1T(x2, piT)
            finish_l1(a.H1 + 7 * BH1 + (long long)r * a.ldh1, a.h1, a.act, a.Wa_q2t, o.act, lane);  // q2T(x2, piT)
        }
    } else {
        const NetQ &q = (e == 3) ? a.q1 : a.q2;
        float w3[RV];
        load_row(q.W3, a.h2, lane, w3);
        const float b3 = q.b3[0];
        mask_row(hrow, a.h2, lane);
        const float v = wave_sum(dot_rv(hrow, w3)) + b3;
        if (lane == 0) (e == 3 ? a.q1o : a.q2o)[r] = v;
    }
}

// ------------------------------------------------------------------------------------------
// K: heads, stage B — Q(x,pi), target Qs, backup, losses, dq and dZ2 of the three Q paths.
// actor_learner.py:58-69.  One wave per row; deterministic block partials (summed by k_rows_c).
// ------------------------------------------------------------------------------------------
struct RowsB {
    const float *H2;
    NetQ q1, q2, q1t, q2t;
    const float *rew, *done, *logp0, *logp1, *q1o, *q2o;
    float *dZ2;  // [4][B][h2]  slots: 0 = q1(x,a), 1 = q2(x,a), 2 = q1(x,pi), 3 = pi
    float *dq4;  // [2][B][4]   (column 0 used; padded so that it is a 16-B aligned GEMM operand)
    float *loss_part;
    int B, h2, ldh2;
    float alpha, gamma;
};
__global__ void __launch_bounds__(64) k_rows_b(RowsB a) {
    // one wave = one row = one workgroup: 256 workgroups spread the row fetches over all CUs
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    float lpi = 0.f, l1 = 0.f, l2 = 0.f;
    if (r < a.B) {
        const long long BH = (long long)a.B * a.ldh2, BZ = (long long)a.B * a.h2;
        float h3[RV], h4[RV], h5[RV], h6[RV], h7[RV], w1[RV], w2[RV], w1t[RV], w2t[RV];
        // every load of the kernel up front: one memory round trip
        load_row(a.H2 + 3 * BH + (long long)r * a.ldh2, a.h2, lane, h3);
        load_row(a.H2 + 4 * BH + (long long)r * a.ldh2, a.h2, lane, h4);
        load_row(a.H2 + 5 * BH + (long long)r * a.ldh2, a.h2, lane, h5);
        load_row(a.H2 + 6 * BH + (long long)r * a.ldh2, a.h2, lane, h6);
        load_row(a.H2 + 7 * BH + (long long)r * a.ldh2, a.h2, lane, h7);
        load_row(a.q1.W3, a.h2, lane, w1);
        load_row(a.q2.W3, a.h2, lane, w2);
        load_row(a.q1t.W3, a.h2, lane, w1t);
        load_row(a.q2t.W3, a.h2, lane, w2t);
        const float rew = a.rew[r], done = a.done[r], lp0 = a.logp0[r], lp1 = a.logp1[r], q1v = a.q1o[r], q2v = a.q2o[r];
        const float b1 = a.q1.b3[0], b1t = a.q1t.b3[0], b2t = a.q2t.b3[0];
        mask_row(w1, a.h2, lane); mask_row(w1t, a.h2, lane); mask_row(w2t, a.h2, lane);
        const float q1pi = wave_sum(dot_rv(h5, w1)) + b1;
        const float q1t = wave_sum(dot_rv(h6, w1t)) + b1t;
        const float q2t = wave_sum(dot_rv(h7, w2t)) + b2t;
        const float minq = fminf(q1t, q2t);                          // actor_learner.py:59
        const float vb = minq - a.alpha * lp1;                       // :62
        const float backup = rew + (a.gamma * (1.0f - done)) * vb;   // :63
        const float e1 = backup - q1v, e2 = backup - q2v;
        lpi = a.alpha * lp0 - q1pi;                                  // :66
        l1 = e1 * e1; l2 = e2 * e2;                                  // :67-68
        const float inv_b = 1.0f / (float)a.B;
        const float dq1 = -e1 * inv_b, dq2 = -e2 * inv_b, dqp = -inv_b;
        if (lane == 0) {
            *reinterpret_cast<float4 *>(a.dq4 + (long long)r * 4) = make_float4(dq1, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(a.dq4 + ((long long)a.B + r) * 4) = make_float4(dq2, 0.f, 0.f, 0.f);
        }
        float *z0 = a.dZ2 + (long long)r * a.h2, *z1 = z0 + BZ, *z2 = z1 + BZ;
#pragma unroll
        for (int i = 0; i < RV; ++i) {
            const int j = lane + 64 * i;
            if (j < a.h2) {
                z0[j] = h3[i] > 0.f ? dq1 * w1[i] : 0.f;
                z1[j] = h4[i] > 0.f ? dq2 * w2[i] : 0.f;
                z2[j] = h5[i] > 0.f ? dqp * w1[i] : 0.f;
            }
        }
    }
    // per-row loss terms; the sum over rows is done in a fixed order by the next row kernel
    // (k_rows_c), after the kernel boundary has made them visible — no in-kernel fence needed
    if (lane == 0 && r < a.B) {
        a.loss_part[r * 3 + 0] = lpi; a.loss_part[r * 3 + 1] = l1; a.loss_part[r * 3 + 2] = l2;
    }
}

// ------------------------------------------------------------------------------------------
// K: policy-head backward — d pi_loss / d (mu_raw, log_std_raw) and dZ2 of the policy trunk
// ------------------------------------------------------------------------------------------
struct RowsC {
    const float *H2;    // eval 0 rows (stride ldh2)
    const float *dZ1q;  // dZ1 of the q1(x,pi) path: [B][h1]
    const float *W1q1;  // main q1 layer-1 kernel [(obs+act)][h1]
    NetPi pi;
    const float *save0;
    float *dhead;  // [B][ldd]
    float *dZ2pi;  // [B][h2]
    const float *loss_part;  // [loss_blocks][3] from k_rows_b
    float *losses;           // [3] pi_loss, q1_loss, q2_loss (actor_learner.py:66-68)
    int B, h1, h2, ldh2, obs, act, ldd, loss_blocks;
    float alpha, scale;
    int nl;  // loss terms per row: 3 (SAC1) or 4 (SAC-v: + v_loss)
};
// Leading scalars (preloaded SGPRs): one base pointer + offsets and packed sizes — what the row workgroups'
// first (and only) burst of loads needs; the struct behind them arrives from the cold kernarg segment later.
__global__ void __launch_bounds__(64) k_rows_c(const float *base, int dz1_off, int h2_off, int w1q_off, int wmu_off, int wls_off, int save_off,
                                               int pk_h, int pk_l, int pk_a, RowsC a) {
    const int lane = threadIdx.x;
    const int nrows = (int)((unsigned)pk_a >> 16);   // (the batch fills the upper half: 32 768 rows and more set the sign bit)
    if ((int)blockIdx.x == nrows) {  // (gridDim is a hidden-argument load)
        // reduce_mean over the batch: the extra last workgroup sums the per-row terms of k_rows_b in
        // a fixed order (lane-strided partial sums, then the xor-shuffle tree)
        const int ln = lane;
        float s3[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b0 = 0; b0 < a.loss_blocks; b0 += 64) {
            const int b = b0 + ln;
            const bool ok = b < a.loss_blocks;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float v = a.loss_part[(ok ? b : 0) * a.nl + (c < a.nl ? c : 0)];
                s3[c] += (ok && c < a.nl) ? v : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float tot = wave_sum(s3[c]);
            const float mean = tot / (float)a.B;
            if (ln == 0 && c < a.nl) a.losses[c] = c == 0 ? mean : 0.5f * mean;
        }
        return;
    }
    const int r = blockIdx.x;
    if (r >= nrows) return;
    // everything this wave needs for the first two action dims, in one burst
    float dz[RV], hrow[RV], wq0[RV], wq1[RV], wm0[RV], wl0[RV], wm1[RV], wl1[RV];
    const int ph1 = pk_h & 0xffff, ph2 = pk_h >> 16, pldh2 = pk_l & 0xffff, pobs = pk_l >> 16, pact = pk_a & 0xffff;
    const int cB = pact > 1 ? 1 : 0;
    load_row(base + dz1_off + (long long)r * ph1, ph1, lane, dz);
    load_row(base + h2_off + (long long)r * pldh2, ph2, lane, hrow);
    load_row(base + w1q_off + (long long)(pobs + 0) * ph1, ph1, lane, wq0);
    load_row(base + w1q_off + (long long)(pobs + cB) * ph1, ph1, lane, wq1);
    load_row(base + wmu_off, ph2, lane, wm0, pact, 0);
    load_row(base + wls_off, ph2, lane, wl0, pact, 0);
    load_row(base + wmu_off, ph2, lane, wm1, pact, cB);
    load_row(base + wls_off, ph2, lane, wl1, pact, cB);
    const float4 sv = *reinterpret_cast<const float4 *>(base + save_off + ((long long)r * pact + (lane < pact ? lane : 0)) * 4);
    mask_row(dz, a.h1, lane);
    float ga = 0.f;
    {
        const float s0 = wave_sum(dot_rv(dz, wq0)), s1 = wave_sum(dot_rv(dz, wq1));
        if (lane == 0) ga = s0;
        if (lane == 1 && a.act > 1) ga = s1;
    }
#pragma unroll
    for (int c = 2; c < MAXA; ++c)
        if (c < a.act) {  // act > 2: one more round trip per extra dim
            float w[RV];
            load_row(a.W1q1 + (long long)(a.obs + c) * a.h1, a.h1, lane, w);
            const float sdot = wave_sum(dot_rv(dz, w));
            if (lane == c) ga = sdot;
        }
    float dmu = 0.f, dls = 0.f;
    if (lane < a.act) {
        const float av = sv.x, std = sv.y, t = sv.z, e = sv.w;
        const float glp = a.alpha / (float)a.B;  // d pi_loss / d logp_pi
        const float om = 1.0f - av * av;
        const float cl = fminf(fmaxf(om, 0.f), 1.f);
        const float du = (ga * a.scale) * om + glp * ((2.0f * av * om) / (cl + 1e-6f));
        const float sd = std + STD_EPS;
        const float z = (e * std) / sd;
        const float dzdl = ((e * std) * STD_EPS) / (sd * sd);
        const float dl = du * (e * std) + glp * (-(z * dzdl) - 1.0f);
        dmu = du;
        dls = dl * (11.0f * (1.0f - t * t));
    }
    float gm[MAXA], gl[MAXA];
#pragma unroll
    for (int c = 0; c < MAXA; ++c) { gm[c] = __shfl(dmu, c); gl[c] = __shfl(dls, c); }
    if (lane < a.ldd) {  // dhead row = [dmu | dls | zero padding]
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < MAXA; ++c) {
            if (c < a.act && lane == c) v = gm[c];
            if (c < a.act && lane == a.act + c) v = gl[c];
        }
        a.dhead[(long long)r * a.ldd + lane] = v;
    }
    float acc[RV];
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        acc[i] = fmaf(gl[0], wl0[i], gm[0] * wm0[i]);
        if (a.act > 1) { acc[i] = fmaf(gm[1], wm1[i], acc[i]); acc[i] = fmaf(gl[1], wl1[i], acc[i]); }
    }
#pragma unroll
    for (int c = 2; c < MAXA; ++c)
        if (c < a.act) {
            float wm[RV], wl[RV];
            load_row(a.pi.Wmu, a.h2, lane, wm, a.act, c);
            load_row(a.pi.Wls, a.h2, lane, wl, a.act, c);
#pragma unroll
            for (int i = 0; i < RV; ++i) {
                acc[i] = fmaf(gm[c], wm[i], acc[i]);
                acc[i] = fmaf(gl[c], wl[i], acc[i]);
            }
        }
    float *out = a.dZ2pi + (long long)r * a.h2;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const int j = lane + 64 * i;
        if (j < a.h2) out[j] = hrow[i] > 0.f ? acc[i] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// SAC-v (example/model.py:17-76: policy + twin Q + V + target V).  Evaluations and their H1/H2 slots:
// 0 pi(x)  1 q1(x,a)  2 q2(x,a)  3 q1(x,pi)  4 q2(x,pi)  5 v(x)  6 v_targ(x2).
// ------------------------------------------------------------------------------------------
struct RowsAV {
    const float *H2;
    NetPi pi;
    NetQ q1, q2, v, vt;
    const float *e0;
    float *act0, *logp0, *save0, *q1o, *q2o, *vo, *vto;
    float *H1;
    const float *Wa_q1, *Wa_q2;  // action rows of the main q1 / q2 layer-1 kernels
    int B, h2, ldh2, act, h1, ldh1;
    float scale;
};
__global__ void __launch_bounds__(256) k_rows_a_v(RowsAV a) {
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= a.B * 5) return;
    const int k = wid / a.B, r = wid - k * a.B;
    const int e = k == 0 ? 0 : (k == 1 ? 1 : (k == 2 ? 2 : (k == 3 ? 5 : 6)));
    float hrow[RV];
    load_row(a.H2 + ((long long)e * a.B + r) * a.ldh2, a.h2, lane, hrow);
    if (k == 0) {
        const float el = a.e0[(long long)r * a.act + (lane < a.act ? lane : 0)];
        mask_row(hrow, a.h2, lane);
        const HeadOut o = policy_head(hrow, a.h2, a.act, a.pi, el, a.scale, lane);
        if (lane < a.act) {
            a.act0[r * a.act + lane] = o.act;
            *reinterpret_cast<float4 *>(a.save0 + ((long long)r * a.act + lane) * 4) = make_float4(o.a, o.std, o.t, o.eps);
        }
        if (lane == 0) a.logp0[r] = o.logp;
        const long long BH1 = (long long)a.B * a.ldh1;
        finish_l1(a.H1 + 3 * BH1 + (long long)r * a.ldh1, a.h1, a.act, a.Wa_q1, o.act, lane);  // q1(x, pi)
        finish_l1(a.H1 + 4 * BH1 + (long long)r * a.ldh1, a.h1, a.act, a.Wa_q2, o.act, lane);  // q2(x, pi)
    } else {
        const NetQ &q = k == 1 ? a.q1 : (k == 2 ? a.q2 : (k == 3 ? a.v : a.vt));
        float w3[RV];
        load_row(q.W3, a.h2, lane, w3);
        const float b3 = q.b3[0];
        mask_row(hrow, a.h2, lane);
        const float v = wave_sum(dot_rv(hrow, w3)) + b3;
        if (lane == 0) (k == 1 ? a.q1o : (k == 2 ? a.q2o : (k == 3 ? a.vo : a.vto)))[r] = v;
    }
}

// example/model.py:33-47: min double-Q, the Q and V regression targets, the four losses and their
// derivatives w.r.t. the head outputs; dZ2 slots: 0 q1(x,a)  1 q2(x,a)  2 q1(x,pi)  3 v(x)  (4 = pi)
struct RowsBV {
    const float *H2;
    NetQ q1, q2, v;
    const float *rew, *done, *logp0, *q1o, *q2o, *vo, *vto;
    float *dZ2, *dq4, *loss_part;
    int B, h2, ldh2;
    float alpha, gamma;
};
__global__ void __launch_bounds__(64) k_rows_b_v(RowsBV a) {
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    if (r >= a.B) return;
    const long long BH = (long long)a.B * a.ldh2, BZ = (long long)a.B * a.h2;
    float h1r[RV], h2r[RV], h3r[RV], h4r[RV], h5r[RV], w1[RV], w2[RV], wv[RV];
    load_row(a.H2 + 1 * BH + (long long)r * a.ldh2, a.h2, lane, h1r);
    load_row(a.H2 + 2 * BH + (long long)r * a.ldh2, a.h2, lane, h2r);
    load_row(a.H2 + 3 * BH + (long long)r * a.ldh2, a.h2, lane, h3r);
    load_row(a.H2 + 4 * BH + (long long)r * a.ldh2, a.h2, lane, h4r);
    load_row(a.H2 + 5 * BH + (long long)r * a.ldh2, a.h2, lane, h5r);
    load_row(a.q1.W3, a.h2, lane, w1);
    load_row(a.q2.W3, a.h2, lane, w2);
    load_row(a.v.W3, a.h2, lane, wv);
    const float rew = a.rew[r], done = a.done[r], lp0 = a.logp0[r], q1v = a.q1o[r], q2v = a.q2o[r], vv = a.vo[r], vt = a.vto[r];
    const float b1 = a.q1.b3[0], b2 = a.q2.b3[0];
    mask_row(w1, a.h2, lane); mask_row(w2, a.h2, lane);
    const float q1pi = wave_sum(dot_rv(h3r, w1)) + b1;
    const float q2pi = wave_sum(dot_rv(h4r, w2)) + b2;
    const float minq = fminf(q1pi, q2pi);                              // model.py:34
    const float q_backup = rew + (a.gamma * (1.0f - done)) * vt;       // :37
    const float v_backup = minq - a.alpha * lp0;                       // :38
    const float e1 = q_backup - q1v, e2 = q_backup - q2v, ev = v_backup - vv;
    const float inv_b = 1.0f / (float)a.B;
    const float dq1 = -e1 * inv_b, dq2 = -e2 * inv_b, dv = -ev * inv_b, dqp = -inv_b;
    if (lane == 0) {
        *reinterpret_cast<float4 *>(a.dq4 + (long long)r * 4) = make_float4(dq1, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(a.dq4 + ((long long)a.B + r) * 4) = make_float4(dq2, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(a.dq4 + ((long long)2 * a.B + r) * 4) = make_float4(dv, 0.f, 0.f, 0.f);
        a.loss_part[r * 4 + 0] = a.alpha * lp0 - q1pi;                 // :41
        a.loss_part[r * 4 + 1] = e1 * e1;                              // :42
        a.loss_part[r * 4 + 2] = e2 * e2;                              // :43
        a.loss_part[r * 4 + 3] = ev * ev;                              // :44
    }
    float *z0 = a.dZ2 + (long long)r * a.h2, *z1 = z0 + BZ, *z2 = z1 + BZ, *z3 = z2 + BZ;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const int j = lane + 64 * i;
        if (j < a.h2) {
            z0[j] = h1r[i] > 0.f ? dq1 * w1[i] : 0.f;
            z1[j] = h2r[i] > 0.f ? dq2 * w2[i] : 0.f;
            z2[j] = h3r[i] > 0.f ? dqp * w1[i] : 0.f;
            z3[j] = h5r[i] > 0.f ? dv * wv[i] : 0.f;
        }
    }
}

struct StageArgs {
    const float *src[8];
    float *dst[8];
    int n[8];
};
__global__ void __launch_bounds__(256) k_stage(StageArgs a) {
    const int w = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n[w]; i += gridDim.x * 256) a.dst[w][i] = a.src[w][i];
}

__global__ void k_fill_col4(float *p, long long groups, int ld, int col) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g < groups) *reinterpret_cast<float4 *>(p + (g * ld + col) * 4) = make_float4(1.f, 1.f, 1.f, 1.f);
}

__global__ void k_copy3(const float *a, const float *b, const float *c, float *oa, float *ob, float *oc, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        if (oa) oa[i] = a[i];
        if (ob) ob[i] = b[i];
        if (oc) oc[i] = c[i];
    }
}

// gradient of the fused pi layer-1 wgrad = sum of the row-tile partials (same order as in Adam)
__global__ void __launch_bounds__(256) k_reduce_parts(const float *__restrict__ part, float *__restrict__ g, long long n, long long stride,
                                                      int nparts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sacc = 0.f;  // same order of additions as k_adam_polyak
    for (int q = 0; q < nparts; ++q) sacc += part[(long long)q * stride + i];
    g[i] = sacc;
}

// the same for the direct path's layer-1 block layout: partial [q][k][j] -> gradient element w1y_index(k, j)
__global__ void __launch_bounds__(256) k_reduce_parts_w1y(const float *__restrict__ part, float *__restrict__ g, int nk, int N, int nparts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nk * N) return;
    const int k = i / N, j = i - k * N;
    float sacc = 0.f;  // tile order, as the last-arriver step of k_dg sums them
    for (int q = 0; q < nparts; ++q) sacc += part[(long long)q * nk * N + i];
    g[w1y_index(k, j)] = sacc;
}

static NetQ net_q(const float *base, const Layout &L, int q) {
    return NetQ{base + L.q_W1[q], base + L.q_b1[q], base + L.q_W2[q], base + L.q_b2[q], base + L.q_W3[q], base + L.q_b3[q]};
}
static NetQ net_v(const float *base, const Layout &L) {
    return NetQ{base + L.v_W1, base + L.v_b1, base + L.v_W2, base + L.v_b2, base + L.v_W3, base + L.v_b3};
}

}  // namespace

// ==========================================================================================
// The host-side launch state: everything the launch functions toggle at LAUNCH time.  A snapshot is a copy of it and a restore an
// assignment (ddrl_sac1_capture_begin / _abort, ddrl_sac1_step_host): an aborted capture — whose launches never ran — puts it back.
struct LaunchState {
    int opt_cur;         // opt + opt_cur is the current optimizer state, every optimizer step advances into the other copy
    int sh_cur;          // which copy of the policy dgrad image is current (the optimizer epilogue writes the other one)
    bool fuse_apply;     // this launch_grads also applies the optimizer (Adam in the wgrad epilogues)
    bool sample_armed;   // sampler riding in k_fwd<1> (ddrl_sac1_step_and_sample; its arguments: smp_rs, smp_ring, smp_set)
    // set by ddrl_sac1_fill_noise, consumed by the next compute_grads / apply_grads
    bool noise_armed;
    uint32_t noise_seed;
    unsigned int noise_pending;
    bool grad_imported;  // the gradient buffer was overwritten by import(GRAD): Adam must not re-sum partials
};

struct ddrl_sac1 {
    int device;
    ddrl_sac1_config_t cfg;
    Layout L;
    float *slab;
    float *main_p, *target_p, *m, *v, *grad;
    // two sets of input buffers: the sampler may fill set s^1 while an update reads set s
    // (order inside a set: obs1 obs2 acts rews done eps_x eps_x2 eps_t)
    float *in[2][8];
    float *H1, *H2, *dZ2, *dZ1, *xa, *xp, *part;
    float *act0, *act2, *logp0, *logp1, *save0, *q1o, *q2o, *dq4, *dhead, *loss_part, *losses;
    int ldh1, ldh2, ldxa, ldxp, ldd;
    OptState *opt;       // two copies, see LaunchState::opt_cur
    LaunchState ls;
    Seg *segs_d;
    L1Jobs l1a[2];
    GemmJobs g_fa, g_fb, g_bq, g_bpi, g_last;
    RowsA ra[2];
    RowsB rb[2];
    RowsC rc;
    RowsAV rav[2];       // SAC-v
    RowsBV rbv[2];
    float *vo, *vto;
    AdamArgs ad;
    int rows_b_blocks;
    bool fused;          // direct-operand path (sac1_direct.h) instead of the generic kernels
    DFHead fh_a[2], fh_b[2];
    DFArgs f_a[2], f_b[2];
    DGJobs dg_bq[2], dg_mid, dg_pi;
    int bq_cols;         // column tiles of the q2(x, a) dgrad that run in launch "bq" (the rest: bq_rest, a job of launch "mid")
    DGJob bq_rest;
    // direct-path activations (x4 images, see sac1_direct.h) and the dgrad images of the main layer-2 kernels
    int Lp1, Lp2;
    float *H1r4, *H2c4, *H2r4, *dZ1r4, *dzpi_c4, *dzpi_r4, *dhead_r4, *xa_r4, *da_part, *dq, *w3snap, *xp_r4;
    float *c4_pi[2], *c4_q[3];   // c4_q[2]: V (SAC-v)
    float *c4_q2b;               // second copy of c4_q[1]: double-buffered like the policy's when part of the q2(x, a) dgrad runs in launch "mid",
                                 // where the optimizer epilogue of q2's layer-2 wgrad writes the NEXT image (copy sh_cur = current, sh_cur ^ 1 = next)
    // the jobs launch_stage re-points at launch time, as build_direct numbered them
    int mid_rest_job;            // dg_mid: the q2(x, a) dgrad columns that run there (-1: none)
    int bq_q2_job;               // dg_bq: the q2(x, a) dgrad
    int mid_pi_job, mid_q2w_job; // dg_mid: the policy dgrad; q2's layer-2 wgrad
    int pi_w2_job;               // dg_pi: the policy's layer-2 wgrad
    float *xv_r4;                // SAC-v: the [x | 1] image of V's layer-1 wgrad
    int *part_cnt;       // arrival counters of the policy layer-1 partials (one per column tile)
    ddrl_replay_dev::RingState *smp_rs;
    ddrl_replay_dev::RingPtrs smp_ring;
    int smp_set;
    float *hp;           // head partials [NEVAL][DFH][B][DNT]
    bool fused_l1_wgrad;  // pi layer-1 wgrad via dgrad-epilogue partials + Adam (needs hidden1 % 4 == 0)
    // ddrl_sac1_step_host: the host-batch update as captured graphs — on this surface the ~8 HIP calls of an eager update (two copies, the
    // noise fill, five launches) cost more host time than the device needs for the update.  One graph per (host block, copy parity).
    struct HostGraph { const float *block; float *losses; uint32_t seed; int opt_cur, sh_cur; hipGraphExec_t exec; };
    std::vector<HostGraph> host_graphs;
    uint32_t *host_ctr_d;          // device copy of the noise counter a host block carries up (two words)
    struct { bool valid; LaunchState ls; } snap;   // ddrl_sac1_capture_begin: the launch state before a caller's stream capture
};

static void refresh_shadows(ddrl_sac1 *h, hipStream_t s);
int ddrl_internal_normal_fill_ctr(float *out_d, int64_t n, uint32_t seed, const uint32_t *ctr_d, uint64_t base, void *stream);   // common.hip
int ddrl_internal_host_block_up(const float *src, float *dst_d, int64_t n, float *e0, float *e1, float *e2, int64_t m, uint32_t seed,
                                const uint32_t *ctr, void *stream);                                                              // common.hip

static int sac1_free(ddrl_sac1 *h) {
    for (auto &g : h->host_graphs) (void)hipGraphExecDestroy(g.exec);
    if (h->host_ctr_d) (void)hipFree(h->host_ctr_d);
    (void)hipFree(h->slab);
    delete h;
    return DDRL_OK;
}

static int reset_opt(ddrl_sac1 *h, hipStream_t s) {
    OptState o{};
    o.b1p_pi = o.b1p_q = (float)h->cfg.beta1;
    o.b2p_pi = o.b2p_q = (float)h->cfg.beta2;
    h->ls.opt_cur = 0;
    DDRL_HIP_CHECK(hipMemcpyAsync(h->opt, &o, sizeof(o), hipMemcpyHostToDevice, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    return DDRL_OK;
}

// ------------------------------------------------------------------------------------------
// What differs between SAC1 (algos/sac1) and SAC-v (example/model.py:17-76), as data the two table builders walk
// ------------------------------------------------------------------------------------------
enum { NET_PI = 0, NET_Q1, NET_Q2, NET_V };       // the forward pack field's network ids (the value networks follow the policy at equal distances)
enum { ACT_NONE = 0, ACT_STORED, ACT_PI };        // second input of an evaluation: none, the batch's action, an action sampled by a policy evaluation

// One forward evaluation.  Its position in the list is its slot: H1 / H2 on the generic kernels, head partials on the direct ones.
// ACT_PI evaluations run in the second forward launch (generic: observation part in k_l1, finished by k_rows_a), the others in the first.
struct Eval {
    int net;
    bool x2, targ;       // reads obs2 / the target copy
    int act;
    // direct-operand kernels only
    int img = -1;        // H1r4 / H2c4 slot of the images it leaves (-1: none)
    bool r4 = false;     // leaves an H2r4 image (slot = net)
    float *ddrl_sac1::*xr4 = nullptr;   // leaves its augmented input rows there
    int pev = -1, side = 0;             // ACT_PI: the policy evaluation it takes its action from; DFJob::side
};
// A value network that is trained: its evaluation on the generic kernels, its dZ2 / dZ1 slot, its H1r4 / H2c4 slot on the direct ones
// (H2r4 slot = net; dZ1r4 / dq / w3snap / c4_q slot = position in Variant::vn)
struct ValueNet { int net, gen_ev, slot, img; };
struct Variant {
    bool sacv;
    int nl;                          // loss terms
    const Eval *gen, *dir;           // evaluations on the generic / the direct-operand kernels
    int n_gen, n_dir;
    int gen_qpi;                     // generic: the evaluation q1(x, pi(x)) (dZ slot 2), whose dgrad gives dQ/da
    int nv;
    ValueNet vn[3];                  // (the policy's dZ slot follows: nv + 1 generic, nv direct)
    bool php1;                       // DFArgs::php1 = evaluation 1
    int pev_pack, pin_pack;          // DFArgs
    int q_ev0, q_nev;                // DGJobs: the value-head evaluations
};

// SAC1, both paths: 0 pi(x) 1 pi(x2) 2 piT(x2) 3 q1(x,a) 4 q2(x,a) | 5 q1(x,pi) 6 q1T(x2,piT) 7 q2T(x2,piT)
static const Eval EV_SAC1[8] = {
    {NET_PI, false, false, ACT_NONE, 0, true, &ddrl_sac1::xp_r4},   // [x | 1] as an x4 image: A operand of the policy's layer-1 wgrad
    {NET_PI, true, false, ACT_NONE},
    {NET_PI, true, true, ACT_NONE},
    {NET_Q1, false, false, ACT_STORED, 1, true, &ddrl_sac1::xa_r4},
    {NET_Q2, false, false, ACT_STORED, 2, true},
    {NET_Q1, false, false, ACT_PI, 3, false, nullptr, 0, 1},
    {NET_Q1, true, true, ACT_PI, -1, false, nullptr, 2, 2},
    {NET_Q2, true, true, ACT_PI, -1, false, nullptr, 2, 0},
};
// SAC-v, generic kernels: 0 pi(x) 1 q1(x,a) 2 q2(x,a) | 3 q1(x,pi) 4 q2(x,pi) | 5 v(x) 6 v_targ(x2)
static const Eval EV_SACV_GEN[7] = {
    {NET_PI, false, false, ACT_NONE}, {NET_Q1, false, false, ACT_STORED}, {NET_Q2, false, false, ACT_STORED},
    {NET_Q1, false, false, ACT_PI}, {NET_Q2, false, false, ACT_PI}, {NET_V, false, false, ACT_NONE}, {NET_V, true, true, ACT_NONE},
};
// SAC-v, direct-operand kernels: 0 pi(x) 1 q1(x,a) 2 q2(x,a) 3 v(x) 4 v_targ(x2) | 5 q1(x,pi) 6 q2(x,pi)
static const Eval EV_SACV_DIR[7] = {
    {NET_PI, false, false, ACT_NONE, 0, true, &ddrl_sac1::xp_r4},
    {NET_Q1, false, false, ACT_STORED, 1, true, &ddrl_sac1::xa_r4},
    {NET_Q2, false, false, ACT_STORED, 2, true},
    {NET_V, false, false, ACT_NONE, 4, true, &ddrl_sac1::xv_r4},
    {NET_V, true, true, ACT_NONE},
    {NET_Q1, false, false, ACT_PI, 3, false, nullptr, 0, 1},   // both take the action sampled by pi(x), by the main copy from eps_x
    {NET_Q2, false, false, ACT_PI, -1, false, nullptr, 0, 0},
};
static const Variant VARIANTS[2] = {
    {false, 3, EV_SAC1, EV_SAC1, 8, 8, 5, 2, {{NET_Q1, 3, 0, 1}, {NET_Q2, 4, 1, 2}},
     true, 0 | (2 << 2) | (2 << 4),            // q1(x, pi(x)) <- evaluation 0; the target Qs <- evaluation 2 (pi_targ(x2))
     0 | ((2 | 4) << 3) | ((2 | 4) << 6),      // evaluation 0: main copy, eps_x; evaluation 2: target copy, eps_t
     3, 5},
    {true, 4, EV_SACV_GEN, EV_SACV_DIR, 7, 7, 3, 3, {{NET_Q1, 1, 0, 1}, {NET_Q2, 2, 1, 2}, {NET_V, 5, 3, 4}}, false, 0, 0, 1, 6},
};
static const Variant &variant_of(const ddrl_sac1 *h) { return VARIANTS[h->cfg.variant == DDRL_SAC_V ? 1 : 0]; }

struct NetOff { long long W1, b1, W2, b2, W3, b3; };   // a network's tensors inside a parameter buffer (the policy: no W3 / b3)
static NetOff net_off(const Layout &L, int net) {
    if (net == NET_PI) return NetOff{L.pi_W1, L.pi_b1, L.pi_W2, L.pi_b2, -1, -1};
    if (net == NET_V) return NetOff{L.v_W1, L.v_b1, L.v_W2, L.v_b2, L.v_W3, L.v_b3};
    const int q = net - NET_Q1;
    return NetOff{L.q_W1[q], L.q_b1[q], L.q_W2[q], L.q_b2[q], L.q_W3[q], L.q_b3[q]};
}

// rows of every row-indexed buffer.  Direct-operand path: a whole number of 32-row tiles; rows past the batch are padding (zero
// inputs, no loss terms, zero upstream gradients) and means run over the batch's rows
static int rows_of(const ddrl_sac1 *h) { return h->fused ? rup32(h->cfg.batch) : h->cfg.batch; }

// Element i of a buffer that only the generic path allocates.  The row tables are filled on the direct path too (it reads rc.nl and
// launches none of them): there the buffer is null and the offset alone is kept, as an integer.
static float *at(float *p, long long i) { return reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)i * sizeof(float)); }

// ---- job tables of the update on the generic kernels (gemm_core.h) ----
static int build_generic(ddrl_sac1 *h) {
    const Variant &V = variant_of(h);
    const ddrl_sac1_config_t *cfg = &h->cfg;
    const Layout &L = h->L;
    const int B = cfg->batch, o = cfg->obs_dim, a = cfg->act_dim, h1 = cfg->hidden1, h2 = cfg->hidden2;
    const float *Pm = h->main_p, *Pt = h->target_p;
    const int ldh1 = h->ldh1, ldh2 = h->ldh2;
    const long long BH1 = (long long)B * ldh1, BH2 = (long long)B * ldh2, BZ1 = (long long)B * h1, BZ2 = (long long)B * h2;
    // ---- layer-1 jobs (one table per input set) and the forward layer-2 GEMMs
    for (int st = 0; st < 2; ++st) {
        float *x = h->in[st][0], *x2 = h->in[st][1], *ac = h->in[st][2];
        L1Jobs &J = h->l1a[st];
        J.njobs = V.n_gen;
        J.noise_on = 0; J.act = a; J.n_each = B * a; J.noise_seed = 0;
        J.e0 = h->in[st][5]; J.e1 = h->in[st][6]; J.e2 = h->in[st][7]; J.opt = h->opt;
        for (int ev = 0; ev < V.n_gen; ++ev) {
            const Eval &e = V.gen[ev];
            const NetOff n = net_off(L, e.net);
            const float *P = e.targ ? Pt : Pm;
            J.job[ev] = L1Job{e.x2 ? x2 : x, e.act == ACT_STORED ? ac : nullptr, P + n.W1, P + n.b1, h->H1 + ev * BH1, nullptr,
                              o, e.act != ACT_NONE ? a : 0, B, h1, ldh1, 0, e.act == ACT_PI ? 1 : 0};
            if (ev == 0) { J.job[ev].aug_out = h->xp; J.job[ev].aug_ld = h->ldxp; }                                    // [x | 1]     : pi (and v) layer-1 wgrads
            if (e.net == NET_Q1 && e.act == ACT_STORED) { J.job[ev].aug_out = h->xa; J.job[ev].aug_ld = h->ldxa; }    // [x | a | 1] : Q layer-1 wgrads
            if (st == 0)
                gemm_add(e.act == ACT_PI ? h->g_fb : h->g_fa,
                         gemm_fwd(h->H1 + ev * BH1, ldh1, P + n.W2, P + n.b2, h->H2 + ev * BH2, ldh2, B, h1, h2));
        }
    }
    // ---- backward GEMM launches.  dZ2 / dZ1 slots: 0 q1(x,a), 1 q2(x,a), 2 q1(x,pi), 3 v(x) (SAC-v), then the policy.
    // Every bias gradient rides as the "ones column" row of its kernel's wgrad.
    float *G = h->grad;
    const int pi_slot = V.nv + 1;
    // launch "bwd Q": needs dZ2 of the value networks, dq4
    gemm_add(h->g_bq, gemm_dgrad(h->dZ2 + 2 * BZ2, Pm + L.q_W2[0], h->H1 + V.gen_qpi * BH1, ldh1, h->dZ1 + 2 * BZ1, B, h1, h2));
    for (int q = 0; q < V.nv; ++q) {
        const ValueNet &vn = V.vn[q];
        gemm_add(h->g_bq, gemm_dgrad(h->dZ2 + vn.slot * BZ2, Pm + net_off(L, vn.net).W2, h->H1 + vn.gen_ev * BH1, ldh1, h->dZ1 + vn.slot * BZ1, B, h1, h2));
    }
    for (int q = 0; q < V.nv; ++q) {
        const ValueNet &vn = V.vn[q];
        const NetOff n = net_off(L, vn.net);
        gemm_add(h->g_bq, gemm_wgrad(h->H1 + vn.gen_ev * BH1, ldh1, h1, h->dZ2 + vn.slot * BZ2, h2, h2, G + n.W2, h2, B));           // W2, b2
        gemm_add(h->g_bq, gemm_wgrad(h->H2 + vn.gen_ev * BH2, ldh2, h2, h->dq4 + (long long)q * B * 4, 4, 1, G + n.W3, 1, B));      // W3, b3
    }
    // launch "bwd pi": needs the policy's dZ2, dhead (k_rows_c) and the value networks' dZ1 (launch above)
    {
        GemmJob j = gemm_dgrad(h->dZ2 + pi_slot * BZ2, Pm + L.pi_W2, h->H1, ldh1, h->dZ1 + pi_slot * BZ1, B, h1, h2);
        h->fused_l1_wgrad = (h1 % 4 == 0) && (o + 1 <= 12) && (L.pi_W1 % 4 == 0);
        if (h->fused_l1_wgrad) { j.part_x = h->xp; j.part = h->part; j.part_nk = o + 1; j.part_ldx = h->ldxp; }
        gemm_add(h->g_bpi, j);
    }
    gemm_add(h->g_bpi, gemm_wgrad(h->H1, ldh1, h1, h->dZ2 + pi_slot * BZ2, h2, h2, G + L.pi_W2, h2, B));     // W2, b2
    gemm_add(h->g_bpi, gemm_wgrad(h->H2, ldh2, h2, h->dhead, h->ldd, a, G + L.pi_Wmu, a, B));                 // Wmu, bmu
    gemm_add(h->g_bpi, gemm_wgrad(h->H2, ldh2, h2, h->dhead + a, h->ldd, a, G + L.pi_Wls, a, B));             // Wls, bls
    for (int q = 0; q < V.nv; ++q) {                                                                          // value W1, b1
        const ValueNet &vn = V.vn[q];
        const bool v = vn.net == NET_V;
        gemm_add(h->g_bpi, gemm_wgrad(v ? h->xp : h->xa, v ? h->ldxp : h->ldxa, v ? o : o + a, h->dZ1 + vn.slot * BZ1, h1, h1, G + net_off(L, vn.net).W1, h1, B));
    }
    // launch "last" (only when the fused form is unavailable): needs the policy's dZ1
    if (!h->fused_l1_wgrad) gemm_add(h->g_last, gemm_wgrad(h->xp, h->ldxp, o, h->dZ1 + pi_slot * BZ1, h1, h1, G + L.pi_W1, h1, B));   // pi W1, b1
    return DDRL_OK;
}

// Tile counts against the 256 CUs (profiles/r05_update_experiments.txt: a launch pays +1.2 ... +2.1 us where its tile count
// crosses a multiple of 256 and is flat in between): the three Q dgrads are 3 x 104 = 312 tiles at config 2 — 56 over.  Only the
// last launch reads the dZ1 of the stored-action dgrads (the Q layer-1 wgrads), so the q2(x, a) dgrad is cut by COLUMN tiles: the
// first `keep` stay in launch "bq" (= 256 tiles), the rest run in launch "mid" (which the two Q-head wgrads leave for launch
// "pi": 464 - 20 + 56 = 500 <= 512; "pi": 190 + 20 = 210 <= 256).  A column sub-range of a dgrad is a job of its own — operand B,
// the relu mask and the output image start n_off columns further — with the same arithmetic per tile: bit-identical results.
// Returns the column tiles that stay (all of them: no split).  SAC1 only.  DDRL_BQ_SPLIT=0: never split.
static int bq_keep(int tm, int h1, int h2) {
    const int ct = (h1 + 31) / 32, T = tm * ct, ncu = 256;
    static const int want = getenv("DDRL_BQ_SPLIT") ? atoi(getenv("DDRL_BQ_SPLIT")) : 1;
    const int rm_tiles = 2 * ((h2 + 1 + 31) / 32);                                  // the two Q-head wgrads (one column tile each)
    const int mid_now = T + tm * ((h2 + 31) / 32) + 2 * ((h1 + 1 + 31) / 32) * ((h2 + 31) / 32) + rm_tiles;
    const int pi_now = ((h1 + 1 + 31) / 32) * ((h2 + 31) / 32) + rm_tiles + 3 * ct + 1;
    if (want && 3 * T > ncu && 2 * T < ncu) {
        const int k = (ncu - 2 * T) / tm, moved = (ct - k) * tm;
        if (k >= 1 && k < ct && mid_now - rm_tiles + moved <= 2 * ncu && pi_now + rm_tiles <= ncu) return k;
    }
    return ct;
}

// ---- job tables of the update on the direct-operand kernels (sac1_direct.h).  B = rows of every image (whole 32-row tiles), Bv = the
// batch.  Image slots — H1r4 / H2c4: 0 pi(x) 1 q1(x,a) 2 q2(x,a) 3 q1(x,pi) 4 v(x);  H2r4: 0 pi 1 q1 2 q2 3 v;  dZ1r4: the value
// networks, then the policy.
static int build_direct(ddrl_sac1 *h, int Bv, int B) {
    const Variant &V = variant_of(h);
    const ddrl_sac1_config_t *cfg = &h->cfg;
    const Layout &L = h->L;
    const int o = cfg->obs_dim, a = cfg->act_dim, h1 = cfg->hidden1, h2 = cfg->hidden2;
    const int Kp1 = L.Kp1, Np2 = L.Np2, nt2 = (h2 + 31) / 32, ct = (h1 + 31) / 32;
    const float *Pm = h->main_p, *Pt = h->target_p, *S = h->slab;
    DDRL_REQUIRE(!V.sacv || L.v_W1 - L.q_W1[1] == L.q_W1[1] - L.q_W1[0], "internal: the value networks must sit at equal distances");
    DDRL_REQUIRE(L.pi_bmu == pi_bmu_off(h1, Np2, h2, a) && L.pi_bls == pi_bls_off(h1, Np2, h2, a),   // (k_dfwd<1> forms these addresses itself)
                 "internal: policy-head bias offsets of the direct layout");
    {   // (k_dfwd forms the addresses of its epilogue operands — b2 and the head kernels of a job's network — itself)
        bool same = L.pi_b2 - L.pi_W1 == net_b2_off(h1, Np2) && L.pi_Wmu - L.pi_W1 == net_wh0_off(h1, Np2) && L.pi_Wls - L.pi_W1 == pi_wls_off(h1, Np2, h2, a);
        for (int q = 0; q < 2; ++q) same = same && L.q_b2[q] - L.q_W1[q] == net_b2_off(h1, Np2) && L.q_W3[q] - L.q_W1[q] == net_wh0_off(h1, Np2);
        if (V.sacv) same = same && L.v_b2 - L.v_W1 == net_b2_off(h1, Np2) && L.v_W3 - L.v_W1 == net_wh0_off(h1, Np2);
        DDRL_REQUIRE(same, "internal: epilogue-operand offsets of the direct layout");
    }
    h->fused_l1_wgrad = false;   // (direct path: the policy's layer-1 wgrad is a job of its own, no row-tile partials)
    const long long HP = (long long)DFH * B * DNT;
    const long long H1I = (long long)B * h->Lp1, H2C = (long long)Np2 * B, H2R = (long long)B * h->Lp2;
    auto steps = [](int D) { return D + 1 <= 8 ? 4 : 4 + (D + 1 - 8 + 1) / 2; };  // input columns + the bias column, two per MFMA step
    const int ns_pi = steps(o) - 4, ns_q = steps(o + a) - 4;
    // SAC1: Q1(x, a), Q2(x, a) need nothing from the policy: they run in phase 1 beside the policy-dependent evaluations (k_dfwd:
    // "stored") when the tile counts allow the per-XCD split, else in phase 0 as before.  DDRL_QXA_PHASE=0 forces phase 0.
    const int tpj_f = (B / 32) * nt2;
    static const int qxa_phase = getenv("DDRL_QXA_PHASE") ? atoi(getenv("DDRL_QXA_PHASE")) : 1;
    const bool q_late = !V.sacv && qxa_phase == 1 && (3 * tpj_f) % 8 == 0 && (2 * tpj_f) % 8 == 0;
    // SAC1: the column tiles of the q2(x, a) dgrad that stay in launch "bq"
    const int keep = V.sacv ? ct : bq_keep(B / 32, h1, h2);
    const bool split = keep < ct;
    if (!V.sacv) h->bq_cols = keep;
    // DDRL_SAC1_XIN_GENERIC=1 (debug, read per learner, here): the forward launches fill their layer-1 input rows by the generic form
    // at obs_dim == 8 too, so that one process can hold a learner of each form and compare them byte for byte
    const int xin_generic = getenv("DDRL_SAC1_XIN_GENERIC") && atoi(getenv("DDRL_SAC1_XIN_GENERIC")) != 0;
    for (int st = 0; st < 2; ++st) {
        DFHead &HA = h->fh_a[st], &HB = h->fh_b[st];
        DFArgs &FA = h->f_a[st], &FB = h->f_b[st];
        HA = DFHead{};
        HA.base = S; HA.tiles_m = B / 32; HA.tpj = (B / 32) * nt2; HA.K = h1; HA.Np = Np2; HA.B = B; HA.d0 = o;
        HA.x_off = (int)(h->in[st][0] - S);
        HA.main_off = (int)(Pm - S); HA.targ_off = (int)(Pt - S); HA.npi = (int)L.q_W1[0]; HA.perq = (int)(L.q_W1[1] - L.q_W1[0]);
        HA.hp_off = (int)(h->hp - S);
        HA.xin_generic = xin_generic;
        HB = HA;
        FA = DFArgs{};
        FA.tiles_n = nt2; FA.act = a; FA.Lp1 = h->Lp1; FA.Lp2 = h->Lp2; FA.h2 = h2;
        FA.scale = (float)cfg->act_scale;
        FA.act0 = h->act0; FA.act2 = h->act2; FA.logp0 = h->logp0; FA.logp1 = h->logp1; FA.save0 = h->save0;
        FA.php1 = V.php1 ? h->hp + 1 * HP : nullptr;
        FA.pev_pack = V.pev_pack; FA.pin_pack = V.pin_pack;
        FA.noise_on = 0; FA.n_each = Bv * a; FA.Bv = Bv; FA.noise_seed = 0;
        FA.e0 = h->in[st][5]; FA.e1 = h->in[st][6]; FA.e2 = h->in[st][7]; FA.opt = h->opt;
        FB = FA;
        // evaluation `ev` as the next job of a forward launch.  Pack field of a job: steps | obs2 << 2 | target << 3 | network << 4
        auto put = [&](DFHead &H, DFArgs &F, int ev) {
            const Eval &e = V.dir[ev];
            const NetOff n = net_off(L, e.net);
            const float *P = e.targ ? Pt : Pm;
            const bool pi = e.net == NET_PI;
            DFJob j{};
            j.b2 = P + n.b2; j.wh0 = P + (pi ? L.pi_Wmu : n.W3); j.wh1 = pi ? P + L.pi_Wls : j.wh0;
            j.nh = pi ? 2 * a : 1; j.hsplit = pi ? a : 1; j.hstride = pi ? a : 1;
            j.hp = h->hp + ev * HP;
            if (e.img >= 0) { j.H2c4 = h->H2c4 + e.img * H2C; j.H1r4 = h->H1r4 + e.img * H1I; }
            if (e.r4) j.H2r4 = h->H2r4 + e.net * H2R;
            if (e.xr4) j.xr4 = h->*e.xr4;
            if (e.pev >= 0) { j.php = h->hp + e.pev * HP; j.side = e.side; }
            const int ns = (e.net == NET_Q1 || e.net == NET_Q2) ? ns_q : ns_pi;
            H.pack |= (ns | ((e.x2 ? 1 : 0) << 2) | ((e.targ ? 1 : 0) << 3) | (e.net << 4)) << (6 * F.njobs);
            F.job[F.njobs++] = j;
        };
        for (int ev = 0; ev < V.n_dir; ++ev) {
            const int act = V.dir[ev].act;
            if (act == ACT_PI) put(HB, FB, ev);
            else if (!(q_late && act == ACT_STORED)) put(HA, FA, ev);
        }
        if (q_late) {
            for (int ev = 0; ev < V.n_dir; ++ev)
                if (V.dir[ev].act == ACT_STORED) put(HB, FB, ev);
            HB.pack |= 1 << 30;
        }
        // ---- backward launch 1: the value dgrads (slot 2 first: its dQ/da partials are what the next launch waits for)
        DGJobs &Q = h->dg_bq[st];
        Q = DGJobs{};
        Q.hp = h->hp; Q.B = B; Q.Bv = Bv; Q.sacv = V.sacv ? 1 : 0; Q.q_ev0 = V.q_ev0; Q.q_nev = V.q_nev;
        Q.b3q1 = Pm + L.q_b3[0]; Q.b3q2 = Pm + L.q_b3[1];
        if (V.sacv) { Q.b3q1t = Pm + L.v_b3; Q.b3q2t = Pt + L.v_b3; Q.vo = h->vo; Q.vto = h->vto; }
        else { Q.b3q1t = Pt + L.q_b3[0]; Q.b3q2t = Pt + L.q_b3[1]; }
        Q.rew = h->in[st][3]; Q.done = h->in[st][4]; Q.logp0 = h->logp0; Q.logp1 = h->logp1;
        Q.q1o = h->q1o; Q.q2o = h->q2o; Q.dq = h->dq; Q.loss_part = h->loss_part;
        Q.alpha = (float)cfg->alpha; Q.gamma = (float)cfg->gamma;
        auto dq_job = [&](int slot, int img, int q, float *C) {
            DGJob j{};
            j.type = DG_DGRAD_Q; j.M = B; j.N = h1; j.K = h2; j.slot = slot;
            j.A = h->H2c4 + img * H2C; j.lda = B; j.B = h->c4_q[q]; j.ldb = Kp1;
            j.gw = Pm + net_off(L, V.vn[q].net).W3; j.gdq = nullptr; j.gconst = -1.0f / (float)Bv;
            j.mask = h->H1r4 + img * H1I; j.ldmask = h->Lp1; j.C = C; j.ldc = h->Lp1; j.adam_off = -1;
            return j;
        };
        {
            DGJob j = dq_job(2, 3, 0, nullptr);   // q1(x, pi(x))
            j.wa = Pm + L.q_W1[0]; j.wa_d0 = o; j.da_part = h->da_part; j.nact = a;
            dg_add(Q, j);
        }
        for (int q = 0; q < V.nv; ++q) {
            const ValueNet &vn = V.vn[q];
            DGJob j = dq_job(vn.slot, vn.img, q, h->dZ1r4 + q * H1I);
            j.gw_snap = h->w3snap + 512 * q;   // (the W3 snapshots for the next launch's generated wgrad operands: one per value network)
            if (vn.net != NET_Q2) { dg_add(Q, j); continue; }
            if (split) j.N = keep * 32;
            h->bq_q2_job = Q.njobs;
            dg_add(Q, j);
            if (split && st == 0) {   // the rest of the columns: a job of launch "mid" (rew / done of the input set patched at launch)
                const long long noff = (long long)keep * 32 * 4;
                DGJob r = dq_job(vn.slot, vn.img, q, h->dZ1r4 + q * H1I + noff);
                r.N = h1 - keep * 32;
                r.B = h->c4_q[q] + noff;
                r.mask = h->H1r4 + vn.img * H1I + noff;
                h->bq_rest = r;
            }
        }
    }
    float *G = h->grad;
    const AdamCtx ctx{0, h->main_p, h->target_p, h->m, h->v, G, h->opt, nullptr, L.n_pi_int,
                      (float)cfg->lr, (float)cfg->beta1, (float)cfg->beta2, (float)cfg->adam_eps,
                      (float)cfg->polyak, (float)(1.0 - cfg->polyak), 0u};
    auto wgrad_j4 = [&](const float *A, const float *Bm, long long w_off, long long b_off, float *shadow) {
        DGJob j{};
        j.type = DG_WGRAD_J4; j.M = h1 + 1; j.N = h2; j.K = B;
        j.A = A; j.lda = h->Lp1; j.B = Bm; j.ldb = h->Lp2;
        j.adam_off = w_off; j.ldc = Np2; j.bias_off = b_off; j.bias_row = h1; j.shadow = shadow; j.ld_sh = Kp1;
        return j;
    };
    auto wgrad_rm = [&](const float *A, int lda, int M, const float *Bm, int ldb, int N, long long off) {
        DGJob j{};
        j.type = DG_WGRAD_RM; j.M = M; j.N = N; j.K = B; j.A = A; j.lda = lda; j.B = Bm; j.ldb = ldb; j.adam_off = off; j.ldc = N;
        return j;
    };
    auto head_wgrad = [&](int q) {   // a value network's head: W3, b3
        return wgrad_rm(h->H2r4 + V.vn[q].net * H2R, h->Lp2, h2 + 1, h->dq + (long long)q * B, 1, 1, net_off(L, V.vn[q].net).W3);
    };
    {   // ---- backward launch 2: the policy dgrad — its A operand (dZ2 of the policy trunk) generated in the tile from the dQ/da
        // partials (k_dg, bgen = 3), so it does not wait for the policy-head backward tiles, which run beside it and write the
        // images the policy wgrads of launch 3 contract over —, the value layer-2 + head wgrads (optimizer in the epilogue)
        DGJobs &M = h->dg_mid;
        M = DGJobs{};
        M.B = B; M.Bv = Bv; M.ad = ctx;
        DGJob d{};
        d.type = DG_DGRAD; d.M = B; d.N = h1; d.K = h2; d.A = h->H2c4; d.lda = B; d.B = h->c4_pi[0]; d.ldb = Kp1;   // (B: launch_stage picks the copy)
        d.bgen = 3; d.dap = h->da_part; d.nparts = ct; d.save0 = h->save0; d.wmu = Pm + L.pi_Wmu; d.wls = Pm + L.pi_Wls;
        d.nact = a; d.alpha = (float)cfg->alpha; d.scale = (float)cfg->act_scale;
        d.mask = h->H1r4; d.ldmask = h->Lp1; d.C = h->dZ1r4 + V.nv * H1I; d.ldc = h->Lp1; d.adam_off = -1;
        h->mid_pi_job = M.njobs;
        dg_add(M, d);
        DGJob rc{};
        rc.type = DG_ROWS_C; rc.M = B; rc.N = h2; rc.K = 0; rc.nact = a; rc.adam_off = -1;
        rc.h2c4 = h->H2c4; rc.dap = h->da_part; rc.nparts = ct; rc.save0 = h->save0;
        rc.wmu = Pm + L.pi_Wmu; rc.wls = Pm + L.pi_Wls; rc.dz_c4 = h->dzpi_c4; rc.dz_r4 = h->dzpi_r4; rc.dhead_r4 = h->dhead_r4;
        rc.ld_r4 = h->Lp2; rc.alpha = (float)cfg->alpha; rc.scale = (float)cfg->act_scale;
        dg_add(M, rc);
        for (int q = 0; q < V.nv; ++q) {
            const ValueNet &vn = V.vn[q];
            const NetOff n = net_off(L, vn.net);
            DGJob j = wgrad_j4(h->H1r4 + vn.img * H1I, h->H2r4 + vn.net * H2R, n.W2, n.b2, h->c4_q[q]);
            j.bgen = 1; j.gw = h->w3snap + 512 * q; j.gdq = h->dq + (long long)q * B;   // (W3 as the previous launch saw it)
            if (vn.net == NET_Q2) h->mid_q2w_job = M.njobs;
            dg_add(M, j);
        }
        h->mid_rest_job = -1;
        if (!split) {
            for (int q = 0; q < V.nv; ++q) dg_add(M, head_wgrad(q));
        } else {
            // the remaining column tiles of the q2(x, a) dgrad (see launch 1): its prologue needs the launch header of the Q dgrads
            const DGJobs &Q0 = h->dg_bq[0];
            M.hp = Q0.hp; M.sacv = 0; M.q_ev0 = Q0.q_ev0; M.q_nev = Q0.q_nev;
            M.b3q1 = Q0.b3q1; M.b3q2 = Q0.b3q2; M.b3q1t = Q0.b3q1t; M.b3q2t = Q0.b3q2t;
            M.rew = Q0.rew; M.done = Q0.done; M.logp0 = Q0.logp0; M.logp1 = Q0.logp1;   // (rew / done: launch_stage sets the input set's)
            M.q1o = Q0.q1o; M.q2o = Q0.q2o; M.dq = Q0.dq; M.loss_part = Q0.loss_part;
            M.alpha = Q0.alpha; M.gamma = Q0.gamma;
            h->mid_rest_job = M.njobs;
            dg_add(M, h->bq_rest);
        }
    }
    {   // ---- backward launch 3: the wgrads that need launch 2's outputs — policy layer 2 / heads / layer 1, value layer 1 —, loss means,
        // optimizer bookkeeping.  No hand-off inside the launch: every tile is a plain GEMM tile with its Adam epilogue.
        DGJobs &P = h->dg_pi;
        P = DGJobs{};
        P.B = B; P.Bv = Bv; P.ad = ctx;
        h->pi_w2_job = P.njobs;
        dg_add(P, wgrad_j4(h->H1r4, h->dzpi_r4, L.pi_W2, L.pi_b2, h->c4_pi[1]));   // (launch_stage picks the shadow copy)
        dg_add(P, wgrad_rm(h->H2r4, h->Lp2, h2 + 1, h->dhead_r4, 32, a, L.pi_Wmu));
        dg_add(P, wgrad_rm(h->H2r4, h->Lp2, h2 + 1, h->dhead_r4 + (long long)a * 4, 32, a, L.pi_Wls));
        for (int q = 0; q <= V.nv; ++q) {   // [W1 ; b1] of the value networks, then of the policy: they live in the layer-1 block layout
            const int net = q < V.nv ? V.vn[q].net : NET_PI;
            const bool xa = net == NET_Q1 || net == NET_Q2;
            DGJob j = wgrad_rm(xa ? h->xa_r4 : (net == NET_V ? h->xv_r4 : h->xp_r4), 32, (xa ? o + a : o) + 1, h->dZ1r4 + q * H1I, h->Lp1, h1, net_off(L, net).W1);
            j.type = DG_WGRAD_W1Y;
            dg_add(P, j);
        }
        if (split)   // the Q-head wgrads (+ Adam + polyak of W3, b3), moved here from launch "mid": nothing reads the head
                     // kernels between the two launches (the Q layer-2 wgrads of "mid" use the W3 snapshot)
            for (int q = 0; q < V.nv; ++q) dg_add(P, head_wgrad(q));
        DGJob ls{};
        ls.type = DG_LOSS; ls.M = 1; ls.N = 1; ls.K = 0; ls.adam_off = -1; ls.loss_part = h->loss_part; ls.losses = h->losses; ls.nl = V.nl;
        ls.nparts = -1;   // + the optimizer's books
        dg_add(P, ls);
    }
    return DDRL_OK;
}

// ---- row kernels of the generic path
static void build_rows(ddrl_sac1 *h) {
    const Variant &V = variant_of(h);
    const ddrl_sac1_config_t *cfg = &h->cfg;
    const Layout &L = h->L;
    const int B = rows_of(h), o = cfg->obs_dim, a = cfg->act_dim, h1 = cfg->hidden1, h2 = cfg->hidden2;
    const float *Pm = h->main_p, *Pt = h->target_p;
    const int ldh1 = h->ldh1, ldh2 = h->ldh2;
    const long long BZ1 = (long long)B * h1, BZ2 = (long long)B * h2;
    for (int st = 0; st < 2; ++st) {
        float **in = h->in[st];
        if (V.sacv) {
            h->rav[st] = RowsAV{h->H2, net_pi(Pm, L), net_q(Pm, L, 0), net_q(Pm, L, 1), net_v(Pm, L), net_v(Pt, L), in[5],
                                h->act0, h->logp0, h->save0, h->q1o, h->q2o, h->vo, h->vto, h->H1,
                                Pm + L.q_W1[0] + (long long)o * h1, Pm + L.q_W1[1] + (long long)o * h1, B, h2, ldh2, a, h1, ldh1,
                                (float)cfg->act_scale};
            h->rbv[st] = RowsBV{h->H2, net_q(Pm, L, 0), net_q(Pm, L, 1), net_v(Pm, L), in[3], in[4], h->logp0, h->q1o, h->q2o,
                                h->vo, h->vto, h->dZ2, h->dq4, h->loss_part, B, h2, ldh2, (float)cfg->alpha, (float)cfg->gamma};
        } else {
            h->ra[st] = RowsA{h->H2, net_pi(Pm, L), net_pi(Pt, L), net_q(Pm, L, 0), net_q(Pm, L, 1), in[5], in[6], in[7],
                              h->act0, h->act2, h->logp0, h->logp1, h->save0, h->q1o, h->q2o,
                              h->H1, Pm + L.q_W1[0] + (long long)o * h1, Pt + L.q_W1[0] + (long long)o * h1,
                              Pt + L.q_W1[1] + (long long)o * h1, B, h2, ldh2, a, h1, ldh1, (float)cfg->act_scale};
            h->rb[st] = RowsB{h->H2, net_q(Pm, L, 0), net_q(Pm, L, 1), net_q(Pt, L, 0), net_q(Pt, L, 1), in[3], in[4],
                              h->logp0, h->logp1, h->q1o, h->q2o, h->dZ2, h->dq4, h->loss_part, B, h2, ldh2,
                              (float)cfg->alpha, (float)cfg->gamma};
        }
    }
    h->rc = RowsC{h->H2, at(h->dZ1, 2 * BZ1), Pm + L.q_W1[0], net_pi(Pm, L), h->save0, h->dhead, at(h->dZ2, (V.nv + 1) * BZ2),
                  h->loss_part, h->losses, B, h1, h2, ldh2, o, a, h->ldd, h->rows_b_blocks, (float)cfg->alpha,
                  (float)cfg->act_scale, V.nl};
}

// ---- create, step 2: the kernel path, the parameter layout and the leading dimensions
static void init_shape(ddrl_sac1 *h) {
    const ddrl_sac1_config_t &c = h->cfg;
    h->fused = direct_ok(c);
    h->L = make_layout(c, false, h->fused);
    h->Lp1 = rup32(c.hidden1 + 1); h->Lp2 = rup32(c.hidden2 + 1);  // activation images keep room for the ones column
    // activations carry one extra physical column of ones (the bias-gradient row of the wgrads)
    h->ldh1 = (int)pad4(c.hidden1 + 1); h->ldh2 = (int)pad4(c.hidden2 + 1);
    h->ldxa = (int)pad4(c.obs_dim + c.act_dim + 1); h->ldxp = (int)pad4(c.obs_dim + 1); h->ldd = (int)pad4(2 * c.act_dim);
    h->rows_b_blocks = rows_of(h);  // per-row loss terms
    h->mid_rest_job = -1;           // (no Q dgrad columns in launch "mid" unless build_direct splits them off)
}

// ---- create, step 3: ONE slab for every buffer of the learner (parameters, optimizer state, activations, job tables): a single
// large allocation is mapped with large page fragments, so the ~30 buffers a stage touches share a handful of TLB entries instead
// of missing on one 4 KB page each.  The plan is sizes and offsets only; bind_slab points the handle's members into a base address.
struct SlabPlan {
    struct Item { float **p; size_t off; };
    std::vector<Item> items;
    size_t floats = 0, cnt_off = 0, opt_off = 0, segs_off = 0;
    size_t reserve(size_t cnt) { const size_t off = floats; floats += (cnt + 63) & ~(size_t)63; return off; }  // 256-B aligned
    void add(float *&p, size_t cnt) { items.push_back(Item{&p, reserve(cnt)}); }
};
static SlabPlan plan_slab(ddrl_sac1 *h) {
    const ddrl_sac1_config_t &c = h->cfg;
    const size_t B = (size_t)rows_of(h), o = c.obs_dim, a = c.act_dim, h1 = c.hidden1, h2 = c.hidden2;
    const size_t NT = (size_t)h->L.total_int, Kp1 = h->L.Kp1, Np2 = h->L.Np2, Lp1 = h->Lp1, Lp2 = h->Lp2;
    SlabPlan p;
    p.add(h->main_p, NT); p.add(h->target_p, NT); p.add(h->m, NT); p.add(h->v, NT); p.add(h->grad, NT);
    for (int st = 0; st < 2; ++st) {   // (ddrl_sac1_step_host takes input set 0 as one contiguous span)
        const size_t cnt[8] = {B * o, B * o, B * a, B, B, B * a, B * a, B * a};
        for (int i = 0; i < 8; ++i) p.add(h->in[st][i], cnt[i]);
    }
    p.add(h->part, ((B + 31) / 32) * (o + 1) * h1);
    if (!h->fused) {
        p.add(h->H1, NEVAL * B * h->ldh1); p.add(h->H2, NEVAL * B * h->ldh2);
        p.add(h->dZ2, 5 * B * h2); p.add(h->dZ1, 5 * B * h1);
    } else {
        // image slots: SAC1 — H1r4 / H2c4: pi(x) q1(x,a) q2(x,a) q1(x,pi); H2r4: pi q1 q2; dZ1r4: q1 q2.  SAC-v adds V to each.
        const size_t xv = c.variant == DDRL_SAC_V ? 1 : 0;
        p.add(h->H1r4, (4 + xv) * B * Lp1); p.add(h->H2c4, (4 + xv) * Np2 * B); p.add(h->H2r4, (3 + xv) * B * Lp2);
        p.add(h->dZ1r4, (3 + xv) * B * Lp1) /* q1 q2 (v) + the policy's (last slot) */; p.add(h->dzpi_c4, Np2 * B); p.add(h->dzpi_r4, B * Lp2);
        p.add(h->dhead_r4, B * 32); p.add(h->xa_r4, B * 32); p.add(h->xv_r4, B * 32); p.add(h->xp_r4, B * 32); p.add(h->da_part, 16 * B * 4);
        p.add(h->dq, 3 * B + 256); p.add(h->w3snap, 3 * 512);
        for (int i = 0; i < 2; ++i) p.add(h->c4_pi[i], Np2 * Kp1);
        for (size_t i = 0; i < 2 + xv; ++i) p.add(h->c4_q[i], Np2 * Kp1);
        p.add(h->c4_q2b, Np2 * Kp1);
    }
    p.add(h->xa, B * h->ldxa); p.add(h->xp, B * h->ldxp);
    p.add(h->act0, B * a); p.add(h->act2, B * a); p.add(h->logp0, B); p.add(h->logp1, B); p.add(h->save0, B * a * 4);
    p.add(h->q1o, B); p.add(h->q2o, B); p.add(h->vo, B); p.add(h->vto, B); p.add(h->dq4, 3 * B * 4); p.add(h->dhead, B * h->ldd);
    p.add(h->loss_part, (size_t)h->rows_b_blocks * 4); p.add(h->losses, 4);
    p.add(h->hp, (size_t)NEVAL * DFH * B * DNT);
    p.cnt_off = p.reserve(64);
    p.opt_off = p.reserve((2 * sizeof(OptState) + 3) / 4);
    p.segs_off = p.reserve((h->L.segs.size() * sizeof(Seg) + 3) / 4);
    (void)p.reserve(2048);  // readable guard behind the last buffer (unclamped tile loads, see OpPre)
    return p;
}
static void bind_slab(ddrl_sac1 *h, const SlabPlan &p, float *base) {
    h->slab = base;
    for (const auto &it : p.items) *it.p = base + it.off;
    h->opt = reinterpret_cast<OptState *>(base + p.opt_off);
    h->part_cnt = reinterpret_cast<int *>(base + p.cnt_off);
    h->segs_d = reinterpret_cast<Seg *>(base + p.segs_off);
}
static int alloc_slab(ddrl_sac1 *h, const SlabPlan &p) {
    float *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, p.floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(base, 0, p.floats * sizeof(float));
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc of %zu bytes failed in ddrl_sac1_create: %s", p.floats * sizeof(float), hipGetErrorString(e));
        if (base) (void)hipFree(base);
        return DDRL_ERR_NOMEM;
    }
    bind_slab(h, p, base);
    DDRL_HIP_CHECK(hipMemcpy(h->segs_d, h->L.segs.data(), h->L.segs.size() * sizeof(Seg), hipMemcpyHostToDevice));
    return reset_opt(h, nullptr);
}

// ---- create, step 4: the physical ones columns (never overwritten: kernels write columns < h1 / h2 / obs(+act) only)
static int fill_ones(ddrl_sac1 *h) {
    const ddrl_sac1_config_t &c = h->cfg;
    const int B = rows_of(h), o = c.obs_dim, a = c.act_dim, h1 = c.hidden1, h2 = c.hidden2;
    if (!h->fused) {
        k_fill_col<<<(NEVAL * B + 255) / 256, 256>>>(h->H1, (long long)NEVAL * B, h->ldh1, h1, 1.0f);
        k_fill_col<<<(NEVAL * B + 255) / 256, 256>>>(h->H2, (long long)NEVAL * B, h->ldh2, h2, 1.0f);
    } else {  // x4 images [row/4][ld][4]: "column" c of every row = four consecutive floats per row group
        const int xv = c.variant == DDRL_SAC_V ? 1 : 0;
        k_fill_col4<<<((4 + xv) * B / 4 + 255) / 256, 256>>>(h->H1r4, (long long)(4 + xv) * B / 4, h->Lp1, h1);
        k_fill_col4<<<((3 + xv) * B / 4 + 255) / 256, 256>>>(h->H2r4, (long long)(3 + xv) * B / 4, h->Lp2, h2);
        k_fill_col4<<<(B / 4 + 255) / 256, 256>>>(h->xa_r4, (long long)B / 4, 32, o + a);
        k_fill_col4<<<(B / 4 + 255) / 256, 256>>>(h->xv_r4, (long long)B / 4, 32, o);
        k_fill_col4<<<(B / 4 + 255) / 256, 256>>>(h->xp_r4, (long long)B / 4, 32, o);
    }
    k_fill_col<<<(B + 255) / 256, 256>>>(h->xa, B, h->ldxa, o + a, 1.0f);
    k_fill_col<<<(B + 255) / 256, 256>>>(h->xp, B, h->ldxp, o, 1.0f);
    DDRL_LAUNCH_CHECK();
    DDRL_HIP_CHECK(hipDeviceSynchronize());
    return DDRL_OK;
}

// ---- create, step 5: the job tables of the kernel path, the flat optimizer step and the launch state.  Pointer arithmetic over the
// bound slab only: nothing here touches the device.
static int build_tables(ddrl_sac1 *h) {
    const Variant &V = variant_of(h);
    const ddrl_sac1_config_t *cfg = &h->cfg;
    const Layout &L = h->L;
    const int B = rows_of(h), o = cfg->obs_dim, h1 = cfg->hidden1;
    const int rc = h->fused ? build_direct(h, cfg->batch, B) : build_generic(h);
    if (rc != DDRL_OK) return rc;
    if (h->fused && V.sacv) h->rc.nl = V.nl;   // (the direct path reads the loss count only; SAC1 has always filled its row tables there too)
    else build_rows(h);
    h->ad = AdamArgs{h->main_p, h->target_p, h->m, h->v, h->grad, h->opt, h->opt + 1, L.total_int, L.n_pi_int, 0,
                     (float)cfg->lr, (float)cfg->beta1, (float)cfg->beta2, (float)cfg->adam_eps,
                     (float)cfg->polyak, (float)(1.0 - cfg->polyak),
                     h->part, L.pi_W1 / 4, (long long)(o + 1) * h1 / 4, (long long)(o + 1) * h1 / 4,
                     h->fused_l1_wgrad ? (B + 31) / 32 : 0, 0u};
    h->ls = LaunchState{};
    return DDRL_OK;
}

extern "C" {

int ddrl_sac1_param_counts(const ddrl_sac1_config_t *cfg, int64_t *n_pi, int64_t *n_q) {
    int rc = check_cfg(cfg);
    if (rc != DDRL_OK) return rc;
    Layout L = make_layout(*cfg, false);
    if (n_pi) *n_pi = L.n_pi;
    if (n_q) *n_q = L.n_q;
    return DDRL_OK;
}

int ddrl_sac1_create(ddrl_sac1_t **out, int device, const ddrl_sac1_config_t *cfg) {
    DDRL_REQUIRE(out != nullptr, "out is NULL");
    int rc = check_cfg(cfg);                                                      // 1. check
    if (rc != DDRL_OK) return rc;
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_sac1 *h = new ddrl_sac1();  // value-initialised: every pointer/job table starts zeroed
    h->device = device;
    h->cfg = *cfg;
    init_shape(h);                                                                // 2. layout
    rc = alloc_slab(h, plan_slab(h));                                             // 3. plan and allocate the slab
    if (rc == DDRL_OK) rc = fill_ones(h);                                         // 4. the ones columns
    if (rc == DDRL_OK) rc = build_tables(h);                                      // 5. the tables
    if (rc != DDRL_OK) { sac1_free(h); return rc; }
    *out = h;
    return DDRL_OK;
}

int ddrl_sac1_destroy(ddrl_sac1_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    return sac1_free(h);
}

static float *which_buf(ddrl_sac1 *h, int which) {
    switch (which) {
        case DDRL_SAC1_MAIN: return h->main_p;
        case DDRL_SAC1_TARGET: return h->target_p;
        case DDRL_SAC1_ADAM_M: return h->m;
        case DDRL_SAC1_ADAM_V: return h->v;
        case DDRL_SAC1_GRAD: return h->grad;
        default: return nullptr;
    }
}

int ddrl_sac1_export(ddrl_sac1_t *h, int which, float *flat_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_d != nullptr, "NULL pointer");
    float *buf = which_buf(h, which);
    DDRL_REQUIRE(buf != nullptr, "unknown buffer id");
    ddrl::DeviceGuard g(h->device);
    if (which == DDRL_SAC1_GRAD && h->fused_l1_wgrad && !h->ls.grad_imported) {
        // the pi layer-1 gradient exists only as row-tile partials until Adam runs: materialise it
        const long long n = (long long)(h->cfg.obs_dim + 1) * h->cfg.hidden1;
        if (h->fused)
            k_reduce_parts_w1y<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->part, h->grad + h->L.pi_W1, h->cfg.obs_dim + 1,
                                                                                               h->cfg.hidden1, h->ad.nparts);
        else
            k_reduce_parts<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->part, h->grad + h->L.pi_W1, n, n, h->ad.nparts);
    }
    k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, buf, flat_d, nullptr, 0);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_sac1_grad_buffer(ddrl_sac1_t *h, float **grad_d, int64_t *n) {
    DDRL_REQUIRE(h != nullptr && grad_d != nullptr && n != nullptr, "NULL pointer");
    *grad_d = h->grad;
    *n = h->L.total_int;
    return DDRL_OK;
}

int ddrl_sac1_grad_finalize(ddrl_sac1_t *h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    if (h->fused_l1_wgrad && !h->ls.grad_imported) {  // the pi layer-1 gradient exists only as row-tile partials: sum them into the buffer
        const long long n = (long long)(h->cfg.obs_dim + 1) * h->cfg.hidden1;
        if (h->fused)
            k_reduce_parts_w1y<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->part, h->grad + h->L.pi_W1, h->cfg.obs_dim + 1,
                                                                                               h->cfg.hidden1, h->ad.nparts);
        else
            k_reduce_parts<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->part, h->grad + h->L.pi_W1, n, n, h->ad.nparts);
        DDRL_LAUNCH_CHECK();
    }
    h->ls.grad_imported = true;  // apply_grads takes the buffer as it is (e.g. after an in-place all-reduce)
    return DDRL_OK;
}

int ddrl_sac1_import(ddrl_sac1_t *h, int which, const float *flat_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_d != nullptr, "NULL pointer");
    float *buf = which_buf(h, which);
    DDRL_REQUIRE(buf != nullptr, "unknown buffer id");
    ddrl::DeviceGuard g(h->device);
    k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, flat_d, buf, nullptr, 1);
    if (which == DDRL_SAC1_MAIN) refresh_shadows(h, ddrl::as_stream(stream));
    DDRL_LAUNCH_CHECK();
    if (which == DDRL_SAC1_GRAD) h->ls.grad_imported = true;
    return DDRL_OK;
}

int ddrl_sac1_set_weights(ddrl_sac1_t *h, const float *flat_main_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_main_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    // copy into main AND target: Learner.set_weights runs target_init (actor_learner.py:125-127)
    k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, flat_main_d, h->main_p,
                                                                                    h->target_p, 1);
    refresh_shadows(h, ddrl::as_stream(stream));
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_sac1_get_weights(ddrl_sac1_t *h, float *flat_main_d, void *stream) {
    return ddrl_sac1_export(h, DDRL_SAC1_MAIN, flat_main_d, stream);
}

int ddrl_sac1_opt_steps(ddrl_sac1_t *h, int64_t *t_pi_h, int64_t *t_q_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    OptState o;
    hipStream_t s = ddrl::as_stream(stream);
    DDRL_HIP_CHECK(hipMemcpyAsync(&o, h->opt + h->ls.opt_cur, sizeof(o), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    if (t_pi_h) *t_pi_h = o.t_pi;
    if (t_q_h) *t_q_h = o.t_q;
    return DDRL_OK;
}

int ddrl_sac1_opt_state_get(ddrl_sac1_t *h, int64_t *t_pi_h, int64_t *t_q_h, uint64_t *noise_ctr_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    OptState o;
    hipStream_t s = ddrl::as_stream(stream);
    DDRL_HIP_CHECK(hipMemcpyAsync(&o, h->opt + h->ls.opt_cur, sizeof(o), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    if (t_pi_h) *t_pi_h = o.t_pi;
    if (t_q_h) *t_q_h = o.t_q;
    if (noise_ctr_h) *noise_ctr_h = o.noise_ctr;
    return DDRL_OK;
}

int ddrl_sac1_opt_state_set(ddrl_sac1_t *h, int64_t t_pi, int64_t t_q, uint64_t noise_ctr, void *stream) {
    DDRL_REQUIRE(h != nullptr && t_pi >= 0 && t_q >= 0, "NULL handle or negative step count");
    ddrl::DeviceGuard g(h->device);
    // beta powers as TF keeps them: a running float32 product, one multiply per applied step
    OptState o{};
    const float b1 = (float)h->cfg.beta1, b2 = (float)h->cfg.beta2;
    o.b1p_pi = b1; o.b2p_pi = b2; o.b1p_q = b1; o.b2p_q = b2;
    for (int64_t i = 0; i < t_pi; ++i) { o.b1p_pi *= b1; o.b2p_pi *= b2; }
    for (int64_t i = 0; i < t_q; ++i) { o.b1p_q *= b1; o.b2p_q *= b2; }
    o.t_pi = t_pi; o.t_q = t_q; o.noise_ctr = noise_ctr;
    hipStream_t s = ddrl::as_stream(stream);
    h->ls.opt_cur = 0;
    DDRL_HIP_CHECK(hipMemcpyAsync(h->opt, &o, sizeof(o), hipMemcpyHostToDevice, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    return DDRL_OK;
}

// Direct path: copy `copy` of the dgrad image of q2's layer-2 kernel (double-buffered only when mid_rest_job >= 0: see c4_q2b)
static float *q2_image(const ddrl_sac1 *h, int copy) { return copy ? h->c4_q2b : h->c4_q[1]; }

// Direct path: the main layer-2 kernels a stepped parameter buffer holds (offsets in it) and the current dgrad image of each
struct Shadows { int n; long long w2[4]; float *img[4]; };
static Shadows current_shadows(const ddrl_sac1 *h) {
    const Variant &V = variant_of(h);
    Shadows sh{};
    sh.w2[sh.n] = h->L.pi_W2; sh.img[sh.n++] = h->c4_pi[h->ls.sh_cur];
    for (int q = 0; q < V.nv; ++q) {
        sh.w2[sh.n] = net_off(h->L, V.vn[q].net).W2;
        sh.img[sh.n++] = (V.vn[q].net == NET_Q2 && h->mid_rest_job >= 0) ? q2_image(h, h->ls.sh_cur) : h->c4_q[q];
    }
    return sh;
}

// Direct path: the dgrad images [h2/4][h1][4] of the main layer-2 kernels, regenerated from the k4-interleaved parameters
// whenever those change outside the optimizer epilogues (set_weights / import / the flat Adam kernel).
static void refresh_shadows(ddrl_sac1 *h, hipStream_t s) {
    if (!h->fused) return;
    const Layout &L = h->L;
    const int h1 = h->cfg.hidden1, h2 = h->cfg.hidden2;
    const Shadows sh = current_shadows(h);
    ShadowJobs sj{};
    for (int i = 0; i < sh.n; ++i) { sj.j4[i] = h->main_p + sh.w2[i]; sj.c4[i] = sh.img[i]; }
    k_shadow<<<dim3((h1 + 31) / 32, (h2 / 4 + 7) / 8, sh.n), 256, 0, s>>>(sj, h1, h2, L.Np2, L.Kp1);   // one launch for all networks
}

static void launch_rows_c(ddrl_sac1 *h, hipStream_t s) {
    const RowsC &c = h->rc;
    const float *b = h->slab;
    k_rows_c<<<c.B + 1, 64, 0, s>>>(b, (int)(c.dZ1q - b), (int)(c.H2 - b), (int)(c.W1q1 - b), (int)(c.pi.Wmu - b), (int)(c.pi.Wls - b),
                                    (int)(c.save0 - b), c.h1 | (c.h2 << 16), c.ldh2 | (c.obs << 16), (int)((unsigned)c.act | ((unsigned)c.B << 16)), c);
}

// One stage of the update (input set `st`).  Stage ids as documented for ddrl_sac1_stage_time.
static void launch_stage(ddrl_sac1 *h, int stage, int st, hipStream_t s) {
    const ddrl_sac1_config_t &c = h->cfg;
    const int B = c.batch;
    const dim3 l1grid((c.hidden1 + 255) / 256, (B + L1_ROWS - 1) / L1_ROWS, 1);
    if (h->fused) {
        switch (stage) {
            case 2: h->f_a[st].opt = h->opt + h->ls.opt_cur; launch_dfwd<0>(h->fh_a[st], h->f_a[st], s); break;
            case 5: {
                DFArgs &F = h->f_b[st];
                F.do_sample = h->ls.sample_armed ? 1 : 0;
                if (h->ls.sample_armed) {
                    F.rs = h->smp_rs; F.ring = h->smp_ring; F.sample_batch = h->cfg.batch;
                    float **b = h->in[h->smp_set];
                    F.sout = ddrl_replay_dev::BatchPtrs{{b[0], b[1], b[2], b[3], b[4], nullptr}};
                }
                launch_dfwd<1>(h->fh_b[st], F, s);
                break;
            }
            case 7: {
                DGJobs &J = h->dg_bq[st];
                if (h->mid_rest_job >= 0) J.job[h->bq_q2_job].B = q2_image(h, h->ls.sh_cur);   // q2(x, a) dgrad: the current image of q2's layer-2 kernel
                launch_dg(J, s, 2);
                break;
            }
            case 8: {
                DGJobs &J = h->dg_mid;
                J.ad.on = h->ls.fuse_apply ? 1 : 0;
                J.ad.opt = h->opt + h->ls.opt_cur;
                J.job[h->mid_pi_job].B = h->c4_pi[h->ls.sh_cur];          // the policy dgrad reads this update's image of the policy's layer-2 kernel ...
                J.rew = h->dg_bq[st].rew; J.done = h->dg_bq[st].done;   // (read by the Q dgrad columns that run here, if any)
                if (h->mid_rest_job >= 0) {
                    // those columns read the CURRENT image of q2's layer-2 kernel while the optimizer epilogue of q2's layer-2 wgrad (in
                    // this launch too) writes the next one: two copies, like the policy's (found by the graph == eager test: with one copy the
                    // dgrad saw a half-stepped kernel)
                    J.job[h->mid_rest_job].B = q2_image(h, h->ls.sh_cur) + (long long)h->bq_cols * 32 * 4;
                    J.job[h->mid_q2w_job].shadow = J.ad.on ? q2_image(h, h->ls.sh_cur ^ 1) : nullptr;
                }
                launch_dg(J, s, 3);
                break;
            }
            case 9: {
                DGJobs &J = h->dg_pi;
                J.ad.on = h->ls.fuse_apply ? 1 : 0;
                J.ad.opt = h->opt + h->ls.opt_cur;
                J.job[h->pi_w2_job].shadow = h->c4_pi[h->ls.sh_cur ^ 1];  // ... the optimizer epilogue of the policy's layer-2 wgrad writes the next one
                J.ad.opt_next = h->opt + (h->ls.opt_cur ^ 1);  // the optimizer bookkeeping rides in this launch (its loss tile)
                J.ad.noise_adv = h->ls.noise_pending;
                launch_dg(J, s, 4);
                if (J.ad.on) { h->ls.opt_cur ^= 1; h->ls.sh_cur ^= 1; }
                break;
            }
            case 11: {
                const long long blocks = (h->L.total_int / 4 + 255) / 256;
                h->ad.adam_blocks = (int)blocks;
                h->ad.opt = h->opt + h->ls.opt_cur; h->ad.opt_next = h->opt + (h->ls.opt_cur ^ 1);
                h->ls.opt_cur ^= 1;
                const int nparts = h->ad.nparts;
                if (nparts > 0) {  // the policy's layer-1 gradient exists as row-tile partials: sum them into the (block-layout) gradient first
                    const int nk = h->cfg.obs_dim + 1, N = h->cfg.hidden1;
                    k_reduce_parts_w1y<<<(unsigned)((nk * N + 255) / 256), 256, 0, s>>>(h->part, h->grad + h->L.pi_W1, nk, N, nparts);
                }
                h->ad.nparts = 0;
                {   // the dgrad images of the main layer-2 kernels (what refresh_shadows would rewrite in a launch of its own) ride in the flat step
                    const Shadows sh = current_shadows(h);
                    for (int i = 0; i < sh.n; ++i) { h->ad.sh_off4[i] = sh.w2[i] >> 2; h->ad.sh_dst[i] = sh.img[i]; }
                    h->ad.n_sh = sh.n; h->ad.sh_K = h->cfg.hidden1; h->ad.sh_N = h->cfg.hidden2; h->ad.sh_Np = h->L.Np2; h->ad.sh_ld = h->L.Kp1;
                }
                k_adam_polyak<<<(unsigned)(blocks + (h->ad.do_sample ? 1 : 0)), 256, 0, s>>>(h->ad);
                h->ad.nparts = nparts; h->ad.n_sh = 0;
                break;
            }
            default: break;  // 1, 3, 4, 6, 10: folded into the launches above
        }
        return;
    }
    switch (stage) {
        case 1: h->l1a[st].opt = h->opt + h->ls.opt_cur; k_l1<<<dim3(l1grid.x, l1grid.y, h->l1a[st].njobs), 256, 0, s>>>(h->l1a[st]); break;
        case 2: launch_gemm(h->g_fa, s); break;
        case 3:
            if (c.variant == DDRL_SAC_V) k_rows_a_v<<<(B * 5 + 3) / 4, 256, 0, s>>>(h->rav[st]);
            else k_rows_a<<<(B * 5 + 3) / 4, 256, 0, s>>>(h->ra[st]);
            break;
        case 5: launch_gemm(h->g_fb, s); break;
        case 6:
            if (c.variant == DDRL_SAC_V) k_rows_b_v<<<B, 64, 0, s>>>(h->rbv[st]);
            else k_rows_b<<<B, 64, 0, s>>>(h->rb[st]);
            break;
        case 7: launch_gemm(h->g_bq, s); break;
        case 8: launch_rows_c(h, s); break;  // +1: the loss-reduction workgroup
        case 9: launch_gemm(h->g_bpi, s); break;
        case 10: if (h->g_last.total_tiles > 0) launch_gemm(h->g_last, s); break;
        case 11: {
            const long long blocks = (h->L.total_int / 4 + 255) / 256;
            h->ad.adam_blocks = (int)blocks;
            h->ad.opt = h->opt + h->ls.opt_cur; h->ad.opt_next = h->opt + (h->ls.opt_cur ^ 1);
            h->ls.opt_cur ^= 1;
            k_adam_polyak<<<(unsigned)(blocks + (h->ad.do_sample ? 1 : 0)), 256, 0, s>>>(h->ad);
            break;
        }
        default: break;  // 4: folded into stage 3
    }
}

static int launch_grads(ddrl_sac1 *h, const float *obs1, const float *obs2, const float *acts, const float *rews,
                        const float *done, const float *e0, const float *e1, const float *e2, float *losses_d, float *q1_d,
                        float *q2_d, float *logp_d, hipStream_t s) {
    const ddrl_sac1_config_t &c = h->cfg;
    const int B = c.batch;
    const float *src[8] = {obs1, obs2, acts, rews, done, e0, e1, e2};
    int st = -1;  // which input set the caller's pointers are (zero-copy), if any
    for (int cand = 0; cand < 2 && st < 0; ++cand) {
        bool same = true;
        for (int i = 0; i < 8; ++i) same = same && (src[i] == h->in[cand][i]);
        if (same) st = cand;
    }
    if (st < 0) {  // stage 0: copy the caller's batch into set 0
        st = 0;
        StageArgs sa{};
        const int n[8] = {B * c.obs_dim, B * c.obs_dim, B * c.act_dim, B, B, B * c.act_dim, B * c.act_dim, B * c.act_dim};
        for (int i = 0; i < 8; ++i) { sa.src[i] = src[i]; sa.dst[i] = h->in[0][i]; sa.n[i] = n[i]; }
        k_stage<<<dim3((unsigned)((B * c.obs_dim + 255) / 256), 8), 256, 0, s>>>(sa);
    }
    h->l1a[st].noise_on = h->ls.noise_armed ? 1 : 0;
    h->l1a[st].noise_seed = h->ls.noise_seed;
    h->f_a[st].noise_on = h->ls.noise_armed ? 1 : 0;
    h->f_a[st].noise_seed = h->ls.noise_seed;
    h->ls.noise_pending = h->ls.noise_armed ? (unsigned)(3 * B * c.act_dim) : 0u;
    h->ls.noise_armed = false;
    h->ls.grad_imported = false;
    for (int stage = 1; stage <= 10; ++stage) launch_stage(h, stage, st, s);
    DDRL_LAUNCH_CHECK();
    if (h->ls.fuse_apply) h->ls.noise_pending = 0;  // consumed by the optimizer bookkeeping of the last stage
    if (losses_d) DDRL_HIP_CHECK(hipMemcpyAsync(losses_d, h->losses, (size_t)h->rc.nl * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (q1_d || q2_d || logp_d) {
        k_copy3<<<(B + 255) / 256, 256, 0, s>>>(h->q1o, h->q2o, h->logp0, q1_d, q2_d, logp_d, B);
        DDRL_LAUNCH_CHECK();
    }
    return DDRL_OK;
}

static int launch_apply(ddrl_sac1 *h, hipStream_t s) {
    h->ad.noise_adv = h->ls.noise_pending;
    h->ls.noise_pending = 0;
    const int nparts = h->ad.nparts;
    if (h->ls.grad_imported) h->ad.nparts = 0;  // use the imported (e.g. all-reduced) gradient as is
    launch_stage(h, 11, 0, s);
    h->ad.nparts = nparts;
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_sac1_input_buffers(ddrl_sac1_t *h, int set, float **bufs_h) {
    DDRL_REQUIRE(h != nullptr && bufs_h != nullptr && (set == 0 || set == 1), "NULL pointer or set not in {0,1}");
    for (int i = 0; i < 8; ++i) bufs_h[i] = h->in[set][i];
    return DDRL_OK;
}

int ddrl_sac1_batch(ddrl_sac1_t *h) { return h ? h->cfg.batch : DDRL_ERR_BAD_ARG; }

int ddrl_sac1_is_fused(ddrl_sac1_t *h) { return h ? (h->fused ? 1 : 0) : DDRL_ERR_BAD_ARG; }
int ddrl_sac1_host_graphs(ddrl_sac1_t *h) { return h ? (int)h->host_graphs.size() : DDRL_ERR_BAD_ARG; }

int ddrl_sac1_fill_noise(ddrl_sac1_t *h, uint32_t seed, void *stream) {
    // No kernel of its own: the next compute_grads / step generates eps_x, eps_x2, eps_t inside its
    // first kernel (k_l1) from hash(seed, device counter + i) and its Adam kernel advances the counter.
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    (void)stream;
    h->ls.noise_armed = true;
    h->ls.noise_seed = seed;
    return DDRL_OK;
}

int ddrl_sac1_stage_time(ddrl_sac1_t *h, int stage, int reps, float *ms_per_launch_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && ms_per_launch_h != nullptr, "NULL pointer");
    DDRL_REQUIRE(stage >= 1 && stage <= 10 && reps > 0, "stage must be in [1,10] (idempotent stages), reps > 0");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    hipEvent_t e0, e1;
    DDRL_HIP_CHECK(hipEventCreate(&e0));
    DDRL_HIP_CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch_stage(h, stage, 0, s);
    DDRL_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) launch_stage(h, stage, 0, s);
    DDRL_HIP_CHECK(hipEventRecord(e1, s));
    DDRL_LAUNCH_CHECK();
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    DDRL_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch_h = ms / (float)reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return DDRL_OK;
}

int ddrl_sac1_compute_grads(ddrl_sac1_t *h, const float *obs1_d, const float *obs2_d, const float *acts_d,
                            const float *rews_d, const float *done_d, const float *eps_x_d, const float *eps_x2_d,
                            const float *eps_t_d, float *losses_d, float *q1_d, float *q2_d, float *logp_pi_d,
                            void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(obs1_d && obs2_d && acts_d && rews_d && done_d && eps_x_d && eps_x2_d && eps_t_d, "NULL batch/noise pointer");
    ddrl::DeviceGuard g(h->device);
    return launch_grads(h, obs1_d, obs2_d, acts_d, rews_d, done_d, eps_x_d, eps_x2_d, eps_t_d, losses_d, q1_d, q2_d,
                        logp_pi_d, ddrl::as_stream(stream));
}

int ddrl_sac1_apply_grads(ddrl_sac1_t *h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    return launch_apply(h, ddrl::as_stream(stream));
}

}  // extern "C"

// The sampler step of an update call.  *v: the sampler's view of `replay` for this learner — a transition ring of the learner's shapes as
// it is; an n-step window ring (algos/sac1/sac_ray.py:40-51) in fold-gather mode with the learner's gamma (v->ring.fold): its sampler
// hands the update kernels the folded transition (include/ddrl.h: n-step fold), so nothing downstream of the input set knows the
// difference.  *rides: the sampler can go as one extra workgroup of an update launch (`kernels_take_it`: this kernel path has such a
// launch) — the caller arms it there; else it goes behind the update as a launch of its own (learner_sample_alone).
static int learner_sampler(ddrl_sac1 *h, ddrl_replay_t *replay, bool kernels_take_it, ddrl_replay_dev::SamplerView *v, bool *rides) {
    *v = ddrl_replay_sampler_view(replay);
    *rides = false;
    if (!(v->ring.n_arr == 5 && v->ring.w[0] == h->cfg.obs_dim && v->ring.w[1] == h->cfg.obs_dim && v->ring.w[2] == h->cfg.act_dim &&
          v->ring.w[3] == 1 && v->ring.w[4] == 1)) {
        DDRL_REQUIRE(ddrl_replay_is_window_ring(replay, h->cfg.obs_dim, h->cfg.act_dim),
                     "replay row shape differs from the learner's (obs1, obs2, acts, rews, done) and is no n-step window ring of its obs / act widths");
        *v = ddrl_replay_sampler_view(replay, true, (float)h->cfg.gamma);
    }
    *rides = kernels_take_it && ddrl_replay_can_fuse(replay, *v, h->cfg.batch);
    return DDRL_OK;
}
// sample_batch into input set `set` as a launch of its own (check_cfg keeps batch * max(obs_dim, act_dim) far below the draw's 2^31)
static int learner_sample_alone(ddrl_sac1 *h, ddrl_replay_t *replay, const ddrl_replay_dev::SamplerView &v, int set, void *stream) {
    ddrl_replay_dev::BatchPtrs out;
    ddrl_replay_dev::batch_ptrs(out, h->in[set], 5);
    return ddrl_replay_draw(replay, v, h->cfg.batch, out, nullptr, stream);
}
// Internal (loop.hip): the loop's own draws (the priming draw of a graph, eager updates) into input set `set`
int ddrl_sac1_internal_sample_into(ddrl_sac1 *h, ddrl_replay_t *replay, int set, void *stream) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr && (set == 0 || set == 1), "NULL pointer or set not in {0,1}");
    ddrl_replay_dev::SamplerView v;
    bool rides;
    const int rc = learner_sampler(h, replay, false, &v, &rides);
    if (rc != DDRL_OK) return rc;
    return learner_sample_alone(h, replay, v, set, stream);
}

extern "C" {

int ddrl_sac1_apply_grads_and_sample(ddrl_sac1_t *h, ddrl_replay_t *replay, int set, void *stream) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr && (set == 0 || set == 1), "NULL pointer or set not in {0,1}");
    ddrl::DeviceGuard g(h->device);
    ddrl_replay_dev::SamplerView v;
    bool rides;
    const int vrc = learner_sampler(h, replay, true, &v, &rides);
    if (vrc != DDRL_OK) return vrc;
    if (!rides) {  // empty ring (host view) or rows too large for the one-workgroup sampler
        int rc = launch_apply(h, ddrl::as_stream(stream));
        if (rc != DDRL_OK) return rc;
        return learner_sample_alone(h, replay, v, set, stream);
    }
    h->ad.do_sample = 1;
    h->ad.sample_batch = h->cfg.batch;
    h->ad.rs = v.state;
    h->ad.ring = v.ring;
    ddrl_replay_dev::batch_ptrs(h->ad.sout, h->in[set], 5);
    const int rc = launch_apply(h, ddrl::as_stream(stream));
    h->ad.do_sample = 0;
    if (rc == DDRL_OK) ddrl_replay_note_sample(replay);
    return rc;
}

int ddrl_sac1_step(ddrl_sac1_t *h, const float *obs1_d, const float *obs2_d, const float *acts_d, const float *rews_d,
                   const float *done_d, const float *eps_x_d, const float *eps_x2_d, const float *eps_t_d,
                   float *losses_d, float *q1_d, float *q2_d, float *logp_pi_d, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    // fused path: the optimizer runs in the epilogues of the last GEMM launch — no Adam kernel
    h->ls.fuse_apply = h->fused;
    int rc = ddrl_sac1_compute_grads(h, obs1_d, obs2_d, acts_d, rews_d, done_d, eps_x_d, eps_x2_d, eps_t_d, losses_d,
                                     q1_d, q2_d, logp_pi_d, stream);
    const bool applied = h->ls.fuse_apply;
    h->ls.fuse_apply = false;
    if (rc != DDRL_OK || applied) return rc;
    return ddrl_sac1_apply_grads(h, stream);
}

// train(replay_buffer.sample_batch()) with HOST arrays (example/dsac.py:142-144; algos/sac1/sac1.py:146-148) as ONE call: the caller's
// page-locked block [obs1 | obs2 | acts | rews | done], laid out like input set 0, goes up with one asynchronous copy, the three noise
// tensors are generated in place behind it (counter-based, ddrl_normal_fill), and the update reads the input set it owns.
int ddrl_sac1_step_host(ddrl_sac1_t *h, float *block_h, int64_t n_floats, uint32_t noise_seed, uint64_t noise_ctr, float *losses_d,
                        void *stream) {
    DDRL_REQUIRE(h != nullptr && block_h != nullptr, "NULL pointer");
    const ddrl_sac1_config_t &c = h->cfg;
    const long long B = c.batch, m = B * c.act_dim;
    float **in0 = h->in[0];
    // the five items of set 0 follow one another exactly as ddrl_sac1_create lays them out: rup32(batch) rows each on the direct path
    // (the caller's block holds zeros in the padding rows), every item rounded up to 64 floats — no other buffer inside the span
    const long long Bp = h->fused ? rup32(B) : B;
    const long long w[5] = {c.obs_dim, c.obs_dim, c.act_dim, 1, 1};
    for (int j = 0; j < 4; ++j)
        DDRL_REQUIRE(in0[j + 1] - in0[j] == ((Bp * w[j] + 63) & ~63ll), "input set 0 is not one contiguous span: use ddrl_sac1_step with device pointers");
    DDRL_REQUIRE(n_floats == (in0[4] - in0[0]) + B, "block length differs from input set 0's span");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    // the noise counter travels in the two words behind the batch: a captured replay reads it from there
    uint32_t *tail = reinterpret_cast<uint32_t *>(block_h + n_floats);
    tail[0] = (uint32_t)noise_ctr; tail[1] = (uint32_t)(noise_ctr >> 32);
    if (!h->host_ctr_d) DDRL_HIP_CHECK(hipMalloc((void **)&h->host_ctr_d, 2 * sizeof(uint32_t)));
    const bool eps_contig = in0[6] - in0[5] == m && in0[7] - in0[6] == m;
    // a page-locked block is read by the device itself (one launch: batch up + noise); pageable memory goes through copies
    const float *block_dev = nullptr;
    bool resolved = false;
    auto resolve = [&]() {   // (not on the replay path: a recorded graph holds the address)
        if (resolved) return;
        resolved = true;
        hipPointerAttribute_t pa{};
        if (hipPointerGetAttributes(&pa, block_h) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer != nullptr)
            block_dev = static_cast<const float *>(pa.devicePointer);
        else (void)hipGetLastError();
    };
    auto issue = [&]() -> int {
        resolve();
        if (block_dev) {
            const int rc = ddrl_internal_host_block_up(block_dev, in0[0], n_floats, in0[5], in0[6], in0[7], m, noise_seed,
                                                       reinterpret_cast<const uint32_t *>(block_dev + n_floats), stream);
            if (rc != DDRL_OK) return rc;
            return ddrl_sac1_step(h, in0[0], in0[1], in0[2], in0[3], in0[4], in0[5], in0[6], in0[7], losses_d, nullptr, nullptr, nullptr, stream);
        }
        DDRL_HIP_CHECK(hipMemcpyAsync(in0[0], block_h, (size_t)n_floats * sizeof(float), hipMemcpyHostToDevice, s));
        DDRL_HIP_CHECK(hipMemcpyAsync(h->host_ctr_d, tail, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        int rc = DDRL_OK;
        if (eps_contig) rc = ddrl_internal_normal_fill_ctr(in0[5], 3 * m, noise_seed, h->host_ctr_d, 0, stream);
        else
            for (int i = 0; i < 3 && rc == DDRL_OK; ++i) rc = ddrl_internal_normal_fill_ctr(in0[5 + i], m, noise_seed, h->host_ctr_d, (uint64_t)(i * m), stream);
        if (rc != DDRL_OK) return rc;
        return ddrl_sac1_step(h, in0[0], in0[1], in0[2], in0[3], in0[4], in0[5], in0[6], in0[7], losses_d, nullptr, nullptr, nullptr, stream);
    };
    static const bool graphs_on = !(getenv("DDRL_HOST_GRAPH") && atoi(getenv("DDRL_HOST_GRAPH")) == 0);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (!graphs_on || !h->fused || s == nullptr || cap != hipStreamCaptureStatusNone) return issue();   // (the legacy null stream cannot be captured)
    if (h->ls.noise_armed || h->ls.sample_armed) return issue();   // a request armed through another call belongs to THIS update only: not into a graph
    for (auto &hg : h->host_graphs)
        if (hg.block == block_h && hg.losses == losses_d && hg.seed == noise_seed && hg.opt_cur == h->ls.opt_cur && hg.sh_cur == h->ls.sh_cur) {
            DDRL_HIP_CHECK(hipGraphLaunch(hg.exec, s));
            h->ls.opt_cur ^= 1; h->ls.sh_cur ^= 1;   // what the recorded launches did to the host-side state when they were recorded
            return DDRL_OK;
        }
    if (h->host_graphs.size() >= 16) return issue();   // (a caller that keeps changing blocks: eager)
    resolve();
    if (!block_dev) return issue();                    // pageable memory: the copies are not capturable
    ddrl_sac1::HostGraph hg{block_h, losses_d, noise_seed, h->ls.opt_cur, h->ls.sh_cur, nullptr};
    hipGraph_t graph = nullptr;
    // the recorded launches advance the host-side launch state without running: kept if the graph then runs once, put back if not
    const LaunchState before = h->ls;
    DDRL_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = issue();
    const hipError_t e2 = hipStreamEndCapture(s, &graph);
    if (rc != DDRL_OK || e2 != hipSuccess || graph == nullptr) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        h->ls = before;
        if (rc != DDRL_OK) return rc;                  // the update itself was refused (arguments): the same eagerly
        return issue();                                // the capture was refused: nothing ran — this update goes eagerly
    }
    const hipError_t e3 = hipGraphInstantiate(&hg.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e3 != hipSuccess) { (void)hipGetLastError(); h->ls = before; return issue(); }
    h->host_graphs.push_back(hg);
    DDRL_HIP_CHECK(hipGraphLaunch(hg.exec, s));   // (the capture recorded the update — host state advanced once — now it runs once)
    return DDRL_OK;
}

}  // extern "C"

__global__ void k_opt_copy(const OptState *src, OptState *dst) { *dst = *src; }

// Internal (loop.hip): make copy 0 of the double-buffered optimizer state the current one, so that a
// captured graph starts and ends on the same copy whatever the number of updates it holds.
int ddrl_sac1_internal_opt_sync(ddrl_sac1 *h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    if (h->ls.opt_cur == 0 && !(h->fused && h->ls.sh_cur != 0)) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    if (h->ls.opt_cur != 0) {
        k_opt_copy<<<1, 1, 0, ddrl::as_stream(stream)>>>(h->opt + 1, h->opt);
        DDRL_LAUNCH_CHECK();
        h->ls.opt_cur = 0;
    }
    if (h->fused && h->ls.sh_cur != 0) {  // same for the double-buffered dgrad image of the policy's layer-2 kernel
        DDRL_HIP_CHECK(hipMemcpyAsync(h->c4_pi[0], h->c4_pi[1], (size_t)h->L.Np2 * h->L.Kp1 * sizeof(float), hipMemcpyDeviceToDevice,
                                      ddrl::as_stream(stream)));
        if (h->mid_rest_job >= 0)      // ... and of q2's, when it is double-buffered too
            DDRL_HIP_CHECK(hipMemcpyAsync(h->c4_q[1], h->c4_q2b, (size_t)h->L.Np2 * h->L.Kp1 * sizeof(float), hipMemcpyDeviceToDevice,
                                          ddrl::as_stream(stream)));
        h->ls.sh_cur = 0;
    }
    return DDRL_OK;
}

extern "C" {

int ddrl_sac1_graph_sync(ddrl_sac1_t *h, void *stream) { return ddrl_sac1_internal_opt_sync(h, stream); }

int ddrl_sac1_capture_begin(ddrl_sac1_t *h) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    h->snap.valid = true;
    h->snap.ls = h->ls;
    return DDRL_OK;
}

int ddrl_sac1_capture_abort(ddrl_sac1_t *h) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(h->snap.valid, "ddrl_sac1_capture_abort without ddrl_sac1_capture_begin");
    h->ls = h->snap.ls;
    h->snap.valid = false;
    return DDRL_OK;
}

int ddrl_sac1_compute_grads_and_sample(ddrl_sac1_t *h, int set_in, ddrl_replay_t *replay, int set_out, void *stream) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr && (set_in == 0 || set_in == 1) && (set_out == 0 || set_out == 1) && set_in != set_out,
                 "NULL pointer, or input sets not {0,1} / not distinct");
    ddrl::DeviceGuard g(h->device);
    float **b = h->in[set_in];
    ddrl_replay_dev::SamplerView v;
    bool rides;
    const int vrc = learner_sampler(h, replay, h->fused, &v, &rides);
    if (vrc != DDRL_OK) return vrc;
    if (!rides) {  // generic kernels: the sampler as its own launch
        int rc = ddrl_sac1_compute_grads(h, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
        if (rc != DDRL_OK) return rc;
        return learner_sample_alone(h, replay, v, set_out, stream);
    }
    h->ls.sample_armed = true; h->smp_rs = v.state; h->smp_ring = v.ring; h->smp_set = set_out;
    const int rc = ddrl_sac1_compute_grads(h, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
    h->ls.sample_armed = false;
    if (rc == DDRL_OK) ddrl_replay_note_sample(replay);
    return rc;
}

int ddrl_sac1_step_and_sample(ddrl_sac1_t *h, int set_in, ddrl_replay_t *replay, int set_out, void *stream) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr && (set_in == 0 || set_in == 1) && (set_out == 0 || set_out == 1) && set_in != set_out,
                 "NULL pointer, or input sets not {0,1} / not distinct");
    ddrl::DeviceGuard g(h->device);
    float **b = h->in[set_in];
    ddrl_replay_dev::SamplerView v;
    bool rides;
    const int vrc = learner_sampler(h, replay, h->fused, &v, &rides);
    if (vrc != DDRL_OK) return vrc;
    if (!rides) {  // generic kernels: sampler beside the Adam kernel (or on its own)
        int rc = ddrl_sac1_compute_grads(h, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
        if (rc != DDRL_OK) return rc;
        return ddrl_sac1_apply_grads_and_sample(h, replay, set_out, stream);
    }
    h->ls.sample_armed = true; h->smp_rs = v.state; h->smp_ring = v.ring; h->smp_set = set_out;
    const int rc = ddrl_sac1_step(h, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], nullptr, nullptr, nullptr, nullptr, stream);
    h->ls.sample_armed = false;
    if (rc == DDRL_OK) ddrl_replay_note_sample(replay);
    return rc;
}

}  // extern "C"
