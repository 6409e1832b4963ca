// What the direct-operand updates of the discrete learners share: dqn_direct.hip (ddrl_dqn_create_direct: the narrow update) and
// dqn_direct_tail.hip (ddrl_dqn_create_direct_tail: layers 2 / 3 behind a layer 1 of any width).  The segment kinds and the pack kernel
// of the direct layout, the backward launches' argument record, the reference's row logic (head_body's statements of dqn.hip) and the
// Adam + polyak step of one element.  Included inside the including file's anonymous namespace, behind sac1_direct.h.

constexpr int DX_SEG_W2D = 4;     // Seg.mode of the dgrad image: in + ((j / 4) * ld + k) * 4 + j % 4 (gemm_core.h names 1 and 2, wide_pack.h 3)
constexpr int DX_W3S = 4160;      // floats per W3 snapshot: (512 + 1) * 8 rounded up
constexpr int DX_MAXEV = 5;
struct DxOpt { float b1p, b2p, al; int t; };   // running beta powers (TF's beta*_power), this update's step size, updates so far

__global__ void __launch_bounds__(256) k_dx_pack(const Seg *__restrict__ segs, const float *__restrict__ src, float *__restrict__ dst,
                                                 float *__restrict__ dst2, int to_internal) {
    const Seg s = segs[blockIdx.y];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += (long long)gridDim.x * 256) {
        long long ii = i;
        if (s.cols > 0) {
            const long long k = i / s.cols, j = i - k * s.cols;
            ii = s.mode == 2 ? w1y_index(s.d0 + (int)k, (int)j) : s.mode == DX_SEG_W2D ? ((j >> 2) * s.ld + k) * 4 + (j & 3) : ((k >> 2) * s.ld + j) * 4 + (k & 3);
        }
        if (to_internal) {
            const float v = src[s.ext + i];
            dst[s.in + ii] = v;
            if (dst2) dst2[s.in + ii] = v;
        } else {
            dst[s.ext + i] = src[s.in + ii];
        }
    }
}

// the ones columns of the row images (unit hidden1 of H1r4, unit hidden2 of H2r4): the bias rows of the wgrads
__global__ void __launch_bounds__(256) k_dx_ones(float *img, int rows, int ld, int col) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < rows) img[((long long)(r >> 2) * ld + col) * 4 + (r & 3)] = 1.0f;
}

struct QBArgs {
    float *slab;
    const float *hp, *acts, *rew, *done;
    float *dq, *qrows, *part, *w3snap, *xr4;
    int *ai;
    float *H1r4[2], *H2c4[2], *H2r4[2], *dZ1r4[2];
    DxOpt *opt;
    float *loss_out, *loss_out2;
    int B, Bp, h1, h2, Kp, Np, A, Lp1, Lp2, nnet, nev, sqn, tiles_m, ct, nt2, d0;
    int PN, main_off, targ_off, m_off, v_off, g_off;   // floats per network; the five buffers inside the slab
    int w2f_off, b2_off, w3_off, w2d_off;              // inside a network
    int b3_abs[DX_MAXEV];                              // b3 of the parameter copy evaluation ev ran on
    float lr, b1, b2, eps, pk, pk1, gamma, alpha;
};

// Row prologue of a mid-launch workgroup: rows m0 .. m0 + 31.  Q of every evaluation = its head partials in column-tile order + b3; then
// head_body's statements (dqn.hip).  Leaves dq per differentiated network, the action index and the loss term of each row in LDS.
__device__ __forceinline__ void q_rows(const QBArgs &a, int m0, float (&s_q)[DX_MAXEV][DFH][32], float (&s_dq)[2][32], int (&s_ai)[32], float (&s_loss)[32]) {
    const int tid = threadIdx.x;
    for (int it = tid; it < a.nev * a.A * 32; it += 256) {
        const int r = it & 31, ec = it >> 5, ev = ec / a.A, c = ec - ev * a.A;
        const float4 *p = reinterpret_cast<const float4 *>(a.hp + (((long long)ev * DFH + c) * a.Bp + m0 + r) * DNT);
        const float4 p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
        const float vv[DNT] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, p3.x, p3.y, p3.z, p3.w};
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < DNT; ++nt)
            if (nt < a.nt2) s += vv[nt];
        s_q[ev][c][r] = s + a.slab[a.b3_abs[ev] + c];
    }
    __syncthreads();
    if (tid < 32) {
        const int row = m0 + tid;
        float l = 0.f, g0 = 0.f, g1 = 0.f;
        int ai = 0;
        if (row < a.B) {
            const float p_act = a.acts[row], p_rew = a.rew[row], p_done = a.done[row];
            const int act = (int)p_act;                             // tf.cast(a_ph, tf.int32)
            const bool valid = act >= 0 && act < a.A;               // one_hot of an out-of-range index is all zeros
            ai = valid ? act : 0;
            if (!a.sqn) {
                int best = 0;
                float bv = s_q[1][0][tid];
                for (int c = 1; c < a.A; ++c) { const float v = s_q[1][c][tid]; if (v > bv) { bv = v; best = c; } }  // tf.argmax: first maximum
                const float q_value = valid ? s_q[0][ai][tid] : 0.f;
                const float backup = p_rew + (a.gamma * (1.0f - p_done)) * s_q[2][best][tid];
                const float e = backup - q_value;
                l = e * e;
                g0 = valid ? -e / (float)a.B : 0.f;
            } else {
                // pi_log = log_softmax(q1(x2) / alpha); "entropy_x2" = sum exp(pi_log) * pi_log  (core.py:32-42)
                float zmax = s_q[1][0][tid] / a.alpha;
                for (int c = 1; c < a.A; ++c) zmax = fmaxf(zmax, s_q[1][c][tid] / a.alpha);
                float se = 0.f;
                for (int c = 0; c < a.A; ++c) se += expf(s_q[1][c][tid] / a.alpha - zmax);
                const float lse = logf(se);
                float plogp = 0.f;
                for (int c = 0; c < a.A; ++c) {
                    const float pl = (s_q[1][c][tid] / a.alpha - zmax) - lse;
                    plogp += expf(pl) * pl;
                }
                float m1 = s_q[3][0][tid], m2 = s_q[4][0][tid];   // each target network's own greedy value
                for (int c = 1; c < a.A; ++c) { m1 = fmaxf(m1, s_q[3][c][tid]); m2 = fmaxf(m2, s_q[4][c][tid]); }
                const float v_backup = fminf(m1, m2) - a.alpha * plogp;                 // actor_learner.py:47-50
                const float q_backup = p_rew + (a.gamma * (1.0f - p_done)) * v_backup;
                const float e1 = q_backup - (valid ? s_q[0][ai][tid] : 0.f), e2 = q_backup - (valid ? s_q[2][ai][tid] : 0.f);
                l = e1 * e1 + e2 * e2;
                g0 = valid ? -e1 / (float)a.B : 0.f;
                g1 = valid ? -e2 / (float)a.B : 0.f;
            }
        }
        s_dq[0][tid] = g0; s_dq[1][tid] = g1; s_ai[tid] = ai; s_loss[tid] = l;
    }
    __syncthreads();
}

// Adam + polyak of one element of network `nb` (offset of the network inside a buffer), gradient kept for export
__device__ __forceinline__ float step1(const QBArgs &a, long long idx, float g, float al) {
    float *S = a.slab;
    float m = S[a.m_off + idx], v = S[a.v_off + idx], p = S[a.main_off + idx], t = S[a.targ_off + idx];
    adam1(g, m, v, p, t, 1.0f - a.b1, 1.0f - a.b2, al, a.eps, a.pk, a.pk1);
    S[a.g_off + idx] = g; S[a.m_off + idx] = m; S[a.v_off + idx] = v; S[a.main_off + idx] = p; S[a.targ_off + idx] = t;
    return p;
}

// [dW3 ; db3] = [H2 | 1]^T dQ, dQ[row][c] = dq[row] (c == a_row), of workgroup t of network n's head wgrad: thread (c = tid / 32,
// u = 32 t + tid % 32) sums the rows in order, then steps its element
__device__ __forceinline__ void w3_wgrad_step(const QBArgs &a, int n, int t, const float *s_dq, const int *s_ai, float al) {
    const int c = threadIdx.x >> 5, u = t * 32 + (threadIdx.x & 31);
    if (c < a.A && u <= a.h2) {
        const float *img = a.H2r4[n] + (long long)u * 4;
        // compensated (Kahan): one thread sums up to 512 terms that cancel (at 512 rows the plain running sum of the two-element b3
        // gradient sat at the float32 oracle's bar; the MFMA tiles split their rows over four waves and 8-deep groups instead)
        float s = 0.f, comp = 0.f;
        for (int rg = 0; rg < a.Bp / 4; ++rg) {
            const float4 hv = *reinterpret_cast<const float4 *>(img + (long long)rg * a.Lp2 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = f4e(hv, e) * (s_ai[4 * rg + e] == c ? s_dq[4 * rg + e] : 0.f) - comp;
                const float tsum = s + y;
                comp = (tsum - s) - y;
                s = tsum;
            }
        }
        step1(a, (long long)n * a.PN + a.w3_off + (long long)u * a.A + c, s, al);
    }
}
