// Discrete-action learners on the shared GEMM core: Double-DQN (algos/dqn) and soft-Q (algos/sqn).
#include <mutex>
#include "gemm_core.h"
#include "wide_l1.h"
#include "policy_row.h"
#include "dqn_select.h"

// ==========================================================================================
// Double-DQN learner (algos/dqn/actor_learner.py:19-107 on algos/dqn/core.py:40-50):
// q = mlp(obs -> h1 -> h2 -> n_actions), q_x2 = the same variables at obs2, q_next = target(obs2);
// q_target = q_next[argmax q_x2]; q_loss = 0.5 mean((r + gamma (1-d) q_target - q[a])^2);
// one Adam over main/q1, polyak over all.  Layers 1 and 2 (obs_dim is arbitrary here) are jobs of the generic MFMA GEMM kernel,
// the head (its forward for every evaluation, the reference's row logic, its dgrad) is ONE launch (k_dqn_head), Adam + polyak one
// flat launch that also finishes the loss mean: 6 launches per update (+ a staging launch when the rows cannot be read in place).
// The learner loop (dqn_loop.hip, ddrl_dqn_loop_*) runs the narrow update out of one of two input sets that its own sampler fills in
// place — those 6 launches and nothing else, the next update's draw riding in the head launch (k_dqn_head_sample).
// Wide observations (obs_dim >= 1024, config 5's 28 224) take layer 1 through the tiled kernels of wide_l1.h instead (forward split
// over K + reduce; the weight gradient as equal shares of the stage sequence, k_wide_sk), reading the caller's observation rows in place.
// variant DDRL_SQN = the soft-Q learner of algos/sqn/actor_learner.py:19-78 on algos/sqn/core.py:30-79:
// twin networks main/q1, main/q2; evaluations q1(x), q1(x2) (its softmax policy's sum p log p at x2),
// q2(x) and the targets q1_(x2), q2_(x2); v_backup = min(max q1_, max q2_) - alpha * sum p log p;
// q_loss = 0.5 mean((q_backup - q1[a])^2) + 0.5 mean((q_backup - q2[a])^2); one Adam over main/q1, main/q2.
// ==========================================================================================
namespace {

// ------------------------------------------------------------------------------------------
// k_dqn_head: everything between the layer-2 forward and the layer-2 backward in ONE launch (was: head forward as three
// k_gemm jobs, the rows kernel, the head dgrad as a k_gemm job — 31 us of launch-bound kernels at batch 512):
//   Q[ev] = [H2[ev] | 1] [W3 ; b3]              every evaluation's n_actions outputs (K = hidden2 + 1: the bias is the last row)
//   DDQN rows (actor_learner.py:40-55)           a_one_hot, q_value, argmax of the online q(x2), q_target, q_backup, q_loss, dQ
//   SQN rows (sqn/actor_learner.py:40-58)        log-softmax entropy of q1(x2), min of the targets' greedy values, q_backup, dQ1, dQ2
//   dZ2[n] = (dQ[n] W3[n]^T) .* (H2[gev[n]] > 0)
// One workgroup = HEAD_ROWS batch rows; the loss is summed over the workgroups' partials by the last one to finish, in
// workgroup order (deterministic).  The head kernels' gradient [H2 | 1]^T dQ stays a k_gemm job (now of the layer-2 backward launch).
// ------------------------------------------------------------------------------------------
constexpr int HEAD_ROWS = 4, HEAD_MAXA = 16, HEAD_MAXEV = 5;
struct HeadArgs {
    const float *H2;                 // [nev][B][ldh2], ones column at h2
    const float *W3b[HEAD_MAXEV];    // [W3 ; b3] of evaluation ev: (h2 + 1) rows of A
    const float *W3n[2];             // ... of the differentiated network n (main)
    const float *acts, *rew, *done;
    float *Q, *dQ, *dZ2, *part, *qsel;
    int *zero_words;                 // polled words of a LATER launch of this update (k_wide_sk's flags), zeroed here: n_zero ints
    int n_zero;
    int B, A, ldq, h2, ldh2, nev, nnet, sqn;
    int gev[2], nev_of_net[2];       // evaluation whose staged [W3 ; b3] is network n's main copy
    int ldw;                         // floats per staged [W3 ; b3]: (h2 + 1) * A rounded up to 4
    float gamma, alpha;
};
static size_t head_lds_bytes(const HeadArgs &a) { return ((size_t)a.nev * HEAD_ROWS * a.ldh2 + (size_t)a.nev * a.ldw) * sizeof(float); }
// the Q phase of k_dqn_head for four actions and NEV evaluations (Double-DQN: 3, SQN: 5): one wave = one batch row, the lanes
// split k; every evaluation's loads are issued together and every sum goes through the butterfly together (a cross-lane exchange
// is an LDS round trip: one chain per (evaluation, action) after the other was 5.3 us of the kernel)
template <int NEV>
__device__ __forceinline__ void head_q4(const HeadArgs &a, const float *sH, const float *sW, float *sQ, int lr, int row, int lane, int K, long long BQ) {
    float acc[NEV][4];
#pragma unroll
    for (int ev = 0; ev < NEV; ++ev) acc[ev][0] = acc[ev][1] = acc[ev][2] = acc[ev][3] = 0.f;
    for (int k = lane; k < K; k += 64) {
        float xv[NEV];
        float4 wv[NEV];
#pragma unroll
        for (int ev = 0; ev < NEV; ++ev) {
            xv[ev] = sH[((size_t)ev * HEAD_ROWS + lr) * a.ldh2 + k];
            wv[ev] = *reinterpret_cast<const float4 *>(sW + (size_t)ev * a.ldw + 4 * k);
        }
#pragma unroll
        for (int ev = 0; ev < NEV; ++ev) {
            acc[ev][0] = fmaf(xv[ev], wv[ev].x, acc[ev][0]); acc[ev][1] = fmaf(xv[ev], wv[ev].y, acc[ev][1]);
            acc[ev][2] = fmaf(xv[ev], wv[ev].z, acc[ev][2]); acc[ev][3] = fmaf(xv[ev], wv[ev].w, acc[ev][3]);
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int ev = 0; ev < NEV; ++ev)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[ev][c] += __shfl_xor(acc[ev][c], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int ev = 0; ev < NEV; ++ev) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sQ[(ev * HEAD_ROWS + lr) * HEAD_MAXA + c] = acc[ev][c];
            if (row < a.B) *reinterpret_cast<float4 *>(a.Q + ev * BQ + (long long)row * a.ldq) = make_float4(acc[ev][0], acc[ev][1], acc[ev][2], acc[ev][3]);
        }
    }
}
__device__ __forceinline__ void head_body(const HeadArgs &a) {
    // the workgroup's H2 rows and every evaluation's [W3 ; b3] are staged into LDS with ALL loads in flight at once (the first cut
    // read them inside the dot-product loops: 30 dependent round trips per wave, 30 us for 3.7 MFLOP)
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float *sH = hsm;                                        // [nev][HEAD_ROWS][ldh2]
    float *sW = hsm + (size_t)a.nev * HEAD_ROWS * a.ldh2;   // [nev][ldw]
    __shared__ float sQ[HEAD_MAXEV][HEAD_ROWS][HEAD_MAXA];
    __shared__ float sdQ[2][HEAD_ROWS][HEAD_MAXA];
    __shared__ float s_loss[HEAD_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * HEAD_ROWS;
    const long long BH = (long long)a.B * a.ldh2, BQ = (long long)a.B * a.ldq;
    const int K = a.h2 + 1;
    // the row scalars the "rows" phase needs, requested now (a cold round trip otherwise sits between two barriers)
    float p_act = 0.f, p_rew = 0.f, p_done = 0.f;
    if (tid < HEAD_ROWS && r0 + tid < a.B) { p_act = a.acts[r0 + tid]; p_rew = a.rew[r0 + tid]; p_done = a.done[r0 + tid]; }
    {
        // four loads per lane in flight per round (a plain load-store loop waits for every load before it issues the next one)
        const int l4 = a.ldh2 >> 2, n4 = a.nev * HEAD_ROWS * l4;
        for (int e0 = tid; e0 < n4; e0 += 4 * 256) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 256 * u;
                const int ec = e < n4 ? e : 0;
                const int ev = ec / (HEAD_ROWS * l4), rem = ec - ev * (HEAD_ROWS * l4), lr = rem / l4, c4 = rem - lr * l4;
                const int row = r0 + lr < a.B ? r0 + lr : a.B - 1;
                v[u] = *reinterpret_cast<const float4 *>(a.H2 + ev * BH + (long long)row * a.ldh2 + 4 * c4);
                if (r0 + lr >= a.B) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + 256 * u < n4) reinterpret_cast<float4 *>(sH)[e0 + 256 * u] = v[u];
        }
        const int nw = K * a.A, nw4 = (nw + 3) / 4;
        for (int ev = 0; ev < a.nev; ++ev) {
            const float *src = a.W3b[ev];
            if ((((unsigned long long)src) & 15ull) == 0) {   // (reads up to three floats past the bias: inside the parameter slab)
                for (int e0 = tid; e0 < nw4; e0 += 4 * 256) {
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4 *>(src)[e0 + 256 * u < nw4 ? e0 + 256 * u : 0];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (e0 + 256 * u < nw4) reinterpret_cast<float4 *>(sW + (size_t)ev * a.ldw)[e0 + 256 * u] = v[u];
                }
            } else {
                for (int e = tid; e < nw; e += 256) sW[(size_t)ev * a.ldw + e] = src[e];
            }
        }
    }
    __syncthreads();
    // ---- Q: wave w takes row w; the lanes split k, fixed-order butterfly
    {
        const int lr = w, row = r0 + lr;
        if (a.A == 4 && a.nev == 3) head_q4<3>(a, sH, sW, &sQ[0][0][0], lr, row, lane, K, BQ);
        else if (a.A == 4 && a.nev == 5) head_q4<5>(a, sH, sW, &sQ[0][0][0], lr, row, lane, K, BQ);
        else {
            for (int ev = 0; ev < a.nev; ++ev) {
                float acc[HEAD_MAXA];
#pragma unroll
                for (int c = 0; c < HEAD_MAXA; ++c) acc[c] = 0.f;
                const float *x = sH + ((size_t)ev * HEAD_ROWS + lr) * a.ldh2;
                const float *wk = sW + (size_t)ev * a.ldw;
                for (int k = lane; k < K; k += 64) {
                    const float xv = x[k];
#pragma unroll
                    for (int c = 0; c < HEAD_MAXA; ++c)
                        if (c < a.A) acc[c] = fmaf(xv, wk[k * a.A + c], acc[c]);
                }
                for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
                    for (int c = 0; c < HEAD_MAXA; ++c)
                        if (c < a.A) acc[c] += __shfl_xor(acc[c], o);
                }
                if (lane == 0) {
#pragma unroll
                    for (int c = 0; c < HEAD_MAXA; ++c)
                        if (c < a.A) {
                            sQ[ev][lr][c] = acc[c];
                            if (row < a.B) a.Q[ev * BQ + (long long)row * a.ldq + c] = acc[c];
                        }
                }
            }
        }
    }
    __syncthreads();
    // ---- rows
    if (tid < HEAD_ROWS) {
        const int row = r0 + tid;
        float l = 0.f;
        if (row < a.B) {
            const int act = (int)p_act;                             // tf.cast(a_ph, tf.int32)
            const bool valid = act >= 0 && act < a.A;               // one_hot of an out-of-range index is all zeros
            if (!a.sqn) {
                const float *q = sQ[0][tid], *qx2 = sQ[1][tid], *qn = sQ[2][tid];
                int best = 0;
                float bv = qx2[0];
                for (int c = 1; c < a.A; ++c) { const float v = qx2[c]; if (v > bv) { bv = v; best = c; } }  // tf.argmax: first maximum
                const float q_value = valid ? q[act] : 0.f;
                const float backup = p_rew + (a.gamma * (1.0f - p_done)) * qn[best];
                const float e = backup - q_value;
                l = e * e;
                const float g = -e / (float)a.B;
                for (int c = 0; c < a.ldq; ++c) {
                    const float v = (valid && c == act) ? g : 0.f;
                    if (c < HEAD_MAXA) sdQ[0][tid][c] = v;
                    a.dQ[(long long)row * a.ldq + c] = v;
                }
                if (a.qsel) a.qsel[row] = q_value;
            } else {
                const float *q1 = sQ[0][tid], *q1x2 = sQ[1][tid], *q2 = sQ[2][tid], *q1t = sQ[3][tid], *q2t = sQ[4][tid];
                // pi_log = log_softmax(q1(x2) / alpha); "entropy_x2" = sum exp(pi_log) * pi_log  (core.py:32-42)
                float zmax = q1x2[0] / a.alpha;
                for (int c = 1; c < a.A; ++c) zmax = fmaxf(zmax, q1x2[c] / a.alpha);
                float se = 0.f;
                for (int c = 0; c < a.A; ++c) se += expf(q1x2[c] / a.alpha - zmax);
                const float lse = logf(se);
                float plogp = 0.f;
                for (int c = 0; c < a.A; ++c) {
                    const float pl = (q1x2[c] / a.alpha - zmax) - lse;
                    plogp += expf(pl) * pl;
                }
                float m1 = q1t[0], m2 = q2t[0];   // q_mu_ = q_[argmax q_] = max q_ (each target network's own greedy value)
                for (int c = 1; c < a.A; ++c) { m1 = fmaxf(m1, q1t[c]); m2 = fmaxf(m2, q2t[c]); }
                const float v_backup = fminf(m1, m2) - a.alpha * plogp;                 // actor_learner.py:47-50
                const float q_backup = p_rew + (a.gamma * (1.0f - p_done)) * v_backup;
                const float e1 = q_backup - (valid ? q1[act] : 0.f), e2 = q_backup - (valid ? q2[act] : 0.f);
                l = e1 * e1 + e2 * e2;
                const float g1 = -e1 / (float)a.B, g2 = -e2 / (float)a.B;
                for (int c = 0; c < a.ldq; ++c) {
                    const bool hit = valid && c == act;
                    if (c < HEAD_MAXA) { sdQ[0][tid][c] = hit ? g1 : 0.f; sdQ[1][tid][c] = hit ? g2 : 0.f; }
                    a.dQ[(long long)row * a.ldq + c] = hit ? g1 : 0.f;
                    a.dQ[BQ + (long long)row * a.ldq + c] = hit ? g2 : 0.f;
                }
            }
        }
        s_loss[tid] = l;
    }
    __syncthreads();
    // ---- dZ2
    for (int nr = 0; nr < a.nnet * HEAD_ROWS; ++nr) {
        const int n = nr / HEAD_ROWS, lr = nr % HEAD_ROWS, row = r0 + lr;
        if (row >= a.B) continue;
        const float *wn = sW + (size_t)a.nev_of_net[n] * a.ldw;
        const float *hrow = sH + ((size_t)a.gev[n] * HEAD_ROWS + lr) * a.ldh2;
        float *out = a.dZ2 + ((long long)n * a.B + row) * a.h2;
        for (int j = tid; j < a.h2; j += 256) {
            const float *wj = wn + j * a.A;
            float v = 0.f;
            for (int c = 0; c < a.A; ++c) v = fmaf(sdQ[n][lr][c], wj[c], v);
            out[j] = hrow[j] > 0.f ? v : 0.f;
        }
    }
    if (a.zero_words)
        for (int i = blockIdx.x * 256 + tid; i < a.n_zero; i += gridDim.x * 256) a.zero_words[i] = 0;
    // ---- loss: this workgroup's rows in order; the flat Adam launch at the end of the update sums the partials in workgroup order
    // (an in-kernel last-arriver needs an L2 write-back per workgroup on this multi-XCD part: 19 us for the whole kernel)
    if (tid == 0) {
        float p = 0.f;
        for (int r = 0; r < HEAD_ROWS; ++r) p += s_loss[r];
        a.part[blockIdx.x] = p;
    }
}
__global__ void __launch_bounds__(256) k_dqn_head(HeadArgs a) { head_body(a); }

// ------------------------------------------------------------------------------------------
// The learner loop's sampler (ddrl_dqn_loop_*): `idxs = np.random.randint(0, size, B)` of the ring's own MT19937 stream
// (ddrl_replay_dev::sample_block, the draw every other path runs) and the five gathers, written where the update reads them — rows of
// ldx floats in the padded images x1 / x2 of one of the learner's two input sets (their ones column is physical and untouched), acts /
// rew / done beside them — so that an update of the loop has no staging launch.  One workgroup of 256 lanes.  The draw leaves the
// indices in `idx` (B words of the learner's slab); the gather behind the barrier reads them back: the workgroup's own stores through
// the CU's vector cache, one round trip, off every update's dependent chain (the sampler rides beside an update, see below).
// sample_block and its dense gather (replay_device.h) are used as they are: the SAC1 launches that embed them compile from unchanged
// sources.  A feed plan is not followed here (fuse_gather = 0 skips it): ddrl_dqn_loop_run refuses a fed ring.
// ------------------------------------------------------------------------------------------
struct SetSampler {
    ddrl_replay_dev::RingState *st;
    ddrl_replay_dev::RingPtrs ring;   // (obs1[obs], obs2[obs], acts, rews, done), float32
    long long *idx;
    float *x1, *x2, *acts, *rew, *done;
    int B, obs, ldx;
};
__device__ __forceinline__ void sample_into_set(const SetSampler &m) {
    const bool rows = m.st->size > 0;   // (nothing in this launch stores into the ring) an empty ring: the draw raises the sticky error
    ddrl_replay_dev::sample_block(m.st, m.ring, ddrl_replay_dev::BatchPtrs{}, m.B, m.idx, 0);
    if (!rows) return;
    __syncthreads();
    const int tid = threadIdx.x;
    const float *r1 = m.ring.a[0], *r2 = m.ring.a[1];
    if ((m.obs & 3) == 0 && ddrl_replay_dev::aligned16(r1, r2) && ddrl_replay_dev::aligned16(m.x1, m.x2)) {   // (ldx is a multiple of 4)
        const int w4 = m.obs >> 2, l4 = m.ldx >> 2;
        const float4 *s1 = reinterpret_cast<const float4 *>(r1), *s2 = reinterpret_cast<const float4 *>(r2);
        float4 *d1 = reinterpret_cast<float4 *>(m.x1), *d2 = reinterpret_cast<float4 *>(m.x2);
        for (int e = tid; e < m.B * w4; e += 256) {
            const int b = e / w4, c = e - b * w4;
            const long long r = m.idx[b] * w4 + c;
            const float4 u = s1[r], v = s2[r];
            d1[b * l4 + c] = u; d2[b * l4 + c] = v;
        }
    } else {
        for (int e = tid; e < m.B * m.obs; e += 256) {
            const int b = e / m.obs, c = e - b * m.obs;
            const long long r = m.idx[b] * m.obs + c;
            const float u = r1[r], v = r2[r];
            m.x1[b * m.ldx + c] = u; m.x2[b * m.ldx + c] = v;
        }
    }
    for (int b = tid; b < m.B; b += 256) {
        const long long r = m.idx[b];
        m.acts[b] = m.ring.a[2][r]; m.rew[b] = m.ring.a[3][r]; m.done[b] = m.ring.a[4][r];
    }
}
// a call's first draw: a launch of its own
__global__ void __launch_bounds__(256) k_dqn_sample(SetSampler m) { sample_into_set(m); }
// The sampler of update u + 1 rides in update u's HEAD launch, as the workgroup behind the head's own: it writes the other input set and
// the ring's sampler state, the head reads H2 and its own set's acts / rew / done — independent.  Why the head and not the Adam launch
// (where SAC1's generic path carries its sampler): k_adam_polyak and sample_block's gather live in the headers the SAC1 update compiles
// from; a strided gather and a second extra workgroup there would change those kernels' sources for a DQN feature.  The head launch is
// this file's own, sits in the middle of the update (the draw is done long before the next update's layer 1 asks for it), and its
// grid at the lander's batch (32 workgroups) leaves the 256 CUs mostly idle anyway.
__global__ void __launch_bounds__(256) k_dqn_head_sample(HeadArgs a, SetSampler m, int head_blocks) {
    if ((int)blockIdx.x == head_blocks) { sample_into_set(m); return; }
    head_body(a);
}

// acts / rews / done of the sampled rows (ddrl_dqn_step_ring: the observation rows stay in the ring)
__global__ void __launch_bounds__(256) k_dqn_gather3(const float *__restrict__ ra, const float *__restrict__ rr, const float *__restrict__ rd,
                                                     const long long *__restrict__ idx, float *acts, float *rew, float *done, long long *idx_out, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) {
        const long long r = idx[i];
        acts[i] = ra[r]; rew[i] = rr[r]; done[i] = rd[r];
        if (idx_out) idx_out[i] = r;
    }
}

// rows ridx[b] of a ring array -> the staged image x1 [B][ldx] (its ones column is physical and untouched): four 16-byte loads in flight per lane
__global__ void __launch_bounds__(256) k_dqn_gather_rows(const float *__restrict__ ring, const long long *__restrict__ ridx, float *__restrict__ x1, int width, int ldx) {
    const float4 *s4 = reinterpret_cast<const float4 *>(ring + ridx[blockIdx.x] * (long long)width);
    float4 *d4 = reinterpret_cast<float4 *>(x1 + (long long)blockIdx.x * ldx);
    const int w4 = width >> 2, tid = threadIdx.x;
    int e = tid;
    for (; e + 3 * 256 < w4; e += 4 * 256) {
        const float4 a0 = s4[e], a1 = s4[e + 256], a2 = s4[e + 512], a3 = s4[e + 768];
        d4[e] = a0; d4[e + 256] = a1; d4[e + 512] = a2; d4[e + 768] = a3;
    }
    for (; e < w4; e += 256) d4[e] = s4[e];
}

// the same out of a compact (uint8) ring array: one 16-byte load of 16 pixels -> four float4 stores (width % 16 == 0; exact conversion)
__global__ void __launch_bounds__(256) k_dqn_gather_rows_u8(const unsigned char *__restrict__ ring, const long long *__restrict__ ridx, float *__restrict__ x1, int width, int ldx) {
    const uint4 *s16 = reinterpret_cast<const uint4 *>(ring + ridx[blockIdx.x] * (long long)width);
    float4 *d4 = reinterpret_cast<float4 *>(x1 + (long long)blockIdx.x * ldx);
    auto put = [&](int e, const uint4 v) {
        const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            d4[4 * e + j] = make_float4((float)(d[j] & 255u), (float)((d[j] >> 8) & 255u), (float)((d[j] >> 16) & 255u), (float)(d[j] >> 24));
    };
    const int w16 = width >> 4, tid = threadIdx.x;
    int e = tid;
    for (; e + 3 * 256 < w16; e += 4 * 256) {
        const uint4 a0 = s16[e], a1 = s16[e + 256], a2 = s16[e + 512], a3 = s16[e + 768];
        put(e, a0); put(e + 256, a1); put(e + 512, a2); put(e + 768, a3);
    }
    for (; e < w16; e += 256) put(e, s16[e]);
}

__global__ void __launch_bounds__(256) k_dqn_stage(const float *o1, const float *o2, const float *ac, const float *r, const float *d,
                                                   float *x1, float *x2, float *acts, float *rew, float *done, int B, int obs, int ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B * obs) {
        const int row = i / obs, c = i - row * obs;
        x1[(long long)row * ldx + c] = o1[i];
        x2[(long long)row * ldx + c] = o2[i];
    }
    if (i < B) { acts[i] = ac[i]; rew[i] = r[i]; done[i] = d[i]; }
}

// ------------------------------------------------------------------------------------------
// The acting path (ddrl_dqn_act, ddrl_rollout_step_discrete).  The Q network obs -> h1 -> h2 -> n_actions has the shape of the SAC
// policy network with its head columns renamed, so its forward IS k_actor_fwd (sac1_direct.h, v_mfma_f32_32x32x2_f32): the handle owns
// an actor handle of shape (obs, ceil(A / 2) "actions", h1, h2) whose mu head holds Q columns [0, half) and whose log_std head holds
// columns [half, A) (a zero column pads an odd A) — head row c of the partials is action c.  k_q_to_pi writes network 0 of the main
// parameters (SQN: q1, algos/sqn/actor_learner.py:164) as that actor's flat weight vector, ddrl_actor_set_weights packs it into the
// operand layout: eagerly at ddrl_dqn_set_weights / ddrl_dqn_import(MAIN), and in front of the next acting forward after a learner step.
// ------------------------------------------------------------------------------------------
struct QPiArgs {
    const float *W1b, *W2b, *W3, *b3;   // [W1 ; b1], [W2 ; b2] (each kernel immediately followed by its bias), W3 [h2][A], b3 [A]
    float *dst;                        // W1, b1, W2, b2, Wmu [h2][half], bmu, Wls [h2][half], bls
    long long n01, n12;
    int h2, A, half;
};
__global__ void __launch_bounds__(256) k_q_to_pi(QPiArgs a) {
    const long long nh = (long long)a.h2 * a.half + a.half, total = a.n01 + a.n12 + 2 * nh;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float v;
        if (i < a.n01) v = a.W1b[i];
        else if (i < a.n01 + a.n12) v = a.W2b[i - a.n01];
        else {
            long long e = i - a.n01 - a.n12;
            const int hi = e >= nh ? 1 : 0;
            e -= hi * nh;
            const int c0 = hi * a.half;
            if (e < (long long)a.h2 * a.half) {
                const long long j = e / a.half;
                const int c = c0 + (int)(e - j * a.half);
                v = c < a.A ? a.W3[j * a.A + c] : 0.f;
            } else {
                const int c = c0 + (int)(e - (long long)a.h2 * a.half);
                v = c < a.A ? a.b3[c] : 0.f;
            }
        }
        a.dst[i] = v;
    }
}

// get_action for n rows: one lane per row.  The Q row comes out of the head partials of the acting forward (hp != nullptr; summation order:
// ddrl_sel::q_row_from_partials) or, for shapes outside that forward's envelope, out of the generic head's Q image (rows of ldq floats,
// bias included); the selection is ddrl_sel::select_row either way — the device function the fused rollout step runs.
struct SelArgs {
    const float *hp, *b_lo, *b_hi;
    const float *Q;
    long long n, hp_rows;            // rows of the call, rows of the forward launch (n rounded up to whole 32-row tiles)
    int ldq, A, half, nt2, sqn, deterministic;
    float greedy_prob, alpha;
    uint32_t seed;
    unsigned long long ctr;
    float *act_out, *q_out;
};
template <int NH>
__global__ void __launch_bounds__(64) k_dqn_select(SelArgs a) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    if (a.hp) {
        float q[ddrl_sel::MAXQ];
        ddrl_sel::q_row_from_partials<NH>(a.hp, a.hp_rows, i, a.A, a.half, a.nt2, a.b_lo, a.b_hi, 0ll, q);
        const float u0 = ddrl_sel::uniform_at(a.seed, a.ctr + 2ull * (unsigned long long)i);
        const float u1 = ddrl_sel::uniform_at(a.seed, a.ctr + 2ull * (unsigned long long)i + 1ull);
        a.act_out[i] = (float)ddrl_sel::select_row(q, a.A, a.sqn, a.deterministic, a.greedy_prob, a.alpha, u0, u1);
        if (a.q_out) {
#pragma unroll
            for (int c = 0; c < ddrl_sel::MAXQ; ++c)
                if (c < a.A) a.q_out[i * a.A + c] = q[c];
        }
        return;
    }
    // up to HEAD_MAXA actions, out of the generic head's Q image
    const float *row = a.Q + i * a.ldq;
    const float u0 = ddrl_sel::uniform_at(a.seed, a.ctr + 2ull * (unsigned long long)i);
    const float u1 = ddrl_sel::uniform_at(a.seed, a.ctr + 2ull * (unsigned long long)i + 1ull);
    float q[HEAD_MAXA];
#pragma unroll
    for (int c = 0; c < HEAD_MAXA; ++c) q[c] = row[c < a.A ? c : 0];
    const int pick = ddrl_sel::select_row(q, a.A, a.sqn, a.deterministic, a.greedy_prob, a.alpha, u0, u1);
    a.act_out[i] = (float)pick;
    if (a.q_out)
        for (int c = 0; c < a.A; ++c) a.q_out[i * a.A + c] = row[c];
}

}  // namespace

struct ddrl_dqn {
    int device;
    ddrl_dqn_config_t cfg;
    int nnet;  // 1 (DDQN) or 2 (SQN: q1, q2)
    long long W1[2], b1[2], W2[2], b2[2], W3[2], b3[2], total_int, total_ext;
    std::vector<Seg> segs;
    float *slab;
    float *main_p, *target_p, *m, *v, *grad;
    float *x1, *x2, *acts, *rew, *done, *H1, *H2, *Q, *dQ, *dZ2, *dZ1, *loss, *qsel;
    float *set1[5];       // the second input set (x1, x2, acts, rew, done) of the learner loop, narrow path only: update u reads one set while
                          // the sampler of update u + 1 fills the other (ddrl_dqn_loop_*); every other entry point lives on set 0 above
    int ldx, ldh1, ldh2, ldq;
    OptState *opt;
    int opt_cur;
    Seg *segs_d;
    GemmJobs g_f1_s1, g_b1_s1;               // the two launches that read the observation images, built on set 1
    GemmJobs g_f1, g_f2, g_f3, g_b2, g_b1;   // g_f3: the head forward as GEMM jobs, ddrl_dqn_q only (the update's head lives in k_dqn_head)
    HeadArgs head;
    float *hpart;
    long long *ring_idx;  // the sampled indices of ddrl_dqn_step_ring
    AdamArgs ad;
    bool wide;            // layer 1 on wide_l1.h
    WideArgs wf, ww[2];   // forward (all evaluations), wgrad per network
    int wf_x2[WD_MAXEV];  // which input an evaluation reads: 0 obs1, 1 obs2
    float *wpart, *wconsts;
    // stream-K layer-1 wgrad (k_wide_sk): per network the fragment table; one slab / flag array / epoch shared (the launches are stream-ordered)
    SkArgs sk[2];
    bool sk_on;
    SkFrag *sk_frags_d;
    float *sk_slab;
    int *sk_flag;
    int *sk_err_h;                   // pinned, device-visible: k_wide_sk's sticky "combine timed out" word
    long long steps_launched, poison_after;   // DDRL_SK_POISON_AFTER=n (tests): the host raises the word itself behind the n-th step's launches
    // acting path (ddrl_dqn_act / ddrl_rollout_step_discrete): nullptr when the shape is outside k_actor_fwd's envelope
    ddrl_actor_t *act_fwd, *act_sel; // two sets of observation rows / head partials: the fused rollout step's envs, ddrl_dqn_act's rows
    const char *act_why;             // ... and what keeps it outside
    float *pi_flat;                  // network 0 of main as the actor's flat weight vector (k_q_to_pi)
    long long act_rows;              // rows of either set: batch rounded up to whole 32-row tiles
    int half;                        // ceil(n_actions / 2): Q columns per head of the actor
    bool pack_stale;                 // a learner step moved main since the last pack
    bool poisoned;                   // that word was seen: the parameters carry at least one step from a wrong layer-1 gradient.  Every step / export
                                     // fails until fresh parameters arrive (set_weights, import of MAIN), so they cannot be pushed or checkpointed
};

// The stream-K combine's verdict, looked at wherever the host is about to trust the parameters: at the next step (unsynchronised: the
// steps already queued behind the failing one have run by then) and, with the stream drained, before anything is exported.
static int dqn_poison_check(ddrl_dqn *h, hipStream_t s, bool drain) {
    if (h->sk_err_h && !h->poisoned) {
        if (drain && h->sk_on) (void)hipStreamSynchronize(s);
        if (*h->sk_err_h) {
            *h->sk_err_h = 0;
            h->poisoned = true;
            h->sk_on = false;                      // from here on: the tile-per-workgroup kernel
            h->head.zero_words = nullptr; h->head.n_zero = 0;
        }
    }
    if (!h->poisoned) return DDRL_OK;
    ddrl::set_error("k_wide_sk: a split tile's partner did not publish within ~1 s (workgroups of the launch not co-resident: shared GPU or "
                    "serialising profiler?) — the layer-1 gradient of an earlier update was wrong and every later step built on it.  This learner "
                    "refuses to step or export until it is given fresh parameters (set_weights / import of the main parameters, e.g. from a "
                    "checkpoint); it then runs the tile-per-workgroup kernel (DDRL_WIDE_SK=0 selects that from the start).");
    return DDRL_ERR_HIP;
}

// Dynamic LDS of a head launch: the attribute belongs to the function (which: 0 k_dqn_head, 1 k_dqn_head_sample) on this device, not to
// the handle: it only ever grows
static int head_grant_lds(int device, int which, size_t need) {
    static size_t granted[2][64] = {{0}};
    static std::mutex granted_mu;
    std::lock_guard<std::mutex> lk(granted_mu);
    if (device >= 0 && device < 64 && need > granted[which][device]) {
        const void *fn = which ? reinterpret_cast<const void *>(k_dqn_head_sample) : reinterpret_cast<const void *>(k_dqn_head);
        const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
        if (ea != hipSuccess) {
            ddrl::set_error("hipFuncSetAttribute(%s, %zu bytes of LDS): %s", which ? "k_dqn_head_sample" : "k_dqn_head", need, hipGetErrorString(ea));
            return DDRL_ERR_HIP;
        }
        granted[which][device] = need;
    }
    return DDRL_OK;
}

extern "C" {

int ddrl_dqn_destroy(ddrl_dqn_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    (void)hipFree(h->slab);
    if (h->act_fwd) (void)ddrl_actor_destroy(h->act_fwd);
    if (h->act_sel) (void)ddrl_actor_destroy(h->act_sel);
    (void)hipFree(h->sk_frags_d); (void)hipFree(h->sk_slab); (void)hipFree(h->sk_flag);
    if (h->sk_err_h) (void)hipHostFree(h->sk_err_h);
    delete h;
    return DDRL_OK;
}

int ddrl_dqn_param_count(const ddrl_dqn_config_t *c, int64_t *n_h) {
    DDRL_REQUIRE(c != nullptr && n_h != nullptr, "NULL pointer");
    *n_h = (int64_t)c->obs_dim * c->hidden1 + c->hidden1 + (int64_t)c->hidden1 * c->hidden2 + c->hidden2 + (int64_t)c->hidden2 * c->n_actions +
           c->n_actions;
    if (c->variant == DDRL_SQN) *n_h *= 2;
    return DDRL_OK;
}

int ddrl_dqn_create(ddrl_dqn_t **out, int device, const ddrl_dqn_config_t *cfg) {
    DDRL_REQUIRE(out != nullptr && cfg != nullptr, "NULL pointer");
    DDRL_REQUIRE(cfg->obs_dim > 0 && cfg->n_actions > 0 && cfg->hidden1 > 0 && cfg->hidden2 > 0 && cfg->batch > 0, "dims must be positive");
    DDRL_REQUIRE(cfg->variant == DDRL_DDQN || (cfg->variant == DDRL_SQN && cfg->alpha > 0.0), "variant must be DDRL_DDQN, or DDRL_SQN with alpha > 0");
    DDRL_REQUIRE(cfg->n_actions <= HEAD_MAXA, "n_actions > 16 unsupported by the head kernel");
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_dqn *h = new ddrl_dqn();
    h->device = device;
    h->cfg = *cfg;
    const int B = cfg->batch, o = cfg->obs_dim, A = cfg->n_actions, h1 = cfg->hidden1, h2 = cfg->hidden2;
    {   // internal layout: every kernel immediately followed by its bias, pairs 16-B aligned (as Layout)
        long long in = 0, ext = 0;
        auto add = [&](long long &slot, long long n, bool pad_after) {
            slot = in;
            h->segs.push_back(Seg{ext, in, n});
            in += n;
            if (pad_after) in = pad4(in);
            ext += n;
        };
        h->nnet = cfg->variant == DDRL_SQN ? 2 : 1;
        for (int n = 0; n < h->nnet; ++n) {
            add(h->W1[n], (long long)o * h1, false); add(h->b1[n], h1, true); add(h->W2[n], (long long)h1 * h2, false); add(h->b2[n], h2, true);
            add(h->W3[n], (long long)h2 * A, false); add(h->b3[n], A, true);
        }
        h->total_int = in; h->total_ext = ext;
    }
    h->ldx = (int)pad4(o + 1); h->ldh1 = (int)pad4(h1 + 1); h->ldh2 = (int)pad4(h2 + 1); h->ldq = (int)pad4(A);
    size_t slab_floats = 0;
    auto reserve = [&](size_t cnt) { size_t off = slab_floats; slab_floats += (cnt + 63) & ~(size_t)63; return off; };
    struct Item { float **p; size_t off; };
    std::vector<Item> items;
#define ALLOC(ptr, cnt) items.push_back(Item{&h->ptr, reserve((size_t)(cnt))})
    const size_t NT = (size_t)h->total_int;
    ALLOC(main_p, NT); ALLOC(target_p, NT); ALLOC(m, NT); ALLOC(v, NT); ALLOC(grad, NT);
    ALLOC(x1, (size_t)B * h->ldx); ALLOC(x2, (size_t)B * h->ldx); ALLOC(acts, B); ALLOC(rew, B); ALLOC(done, B);
    ALLOC(H1, (size_t)5 * B * h->ldh1); ALLOC(H2, (size_t)5 * B * h->ldh2); ALLOC(Q, (size_t)5 * B * h->ldq); ALLOC(dQ, (size_t)2 * B * h->ldq);
    ALLOC(dZ2, (size_t)2 * B * h2); ALLOC(dZ1, (size_t)2 * B * h1); ALLOC(loss, 4); ALLOC(qsel, B);
    ALLOC(hpart, (size_t)(B + HEAD_ROWS - 1) / HEAD_ROWS + 64);
    h->half = (A + 1) / 2;
    ALLOC(pi_flat, (size_t)o * h1 + h1 + (size_t)h1 * h2 + h2 + 2 * ((size_t)h2 * h->half + h->half) + 64);
    float *ring_idx_f = nullptr;
    items.push_back(Item{&ring_idx_f, reserve((size_t)2 * B + 64)});
    h->wide = wide_applies(o, h1);
    const int nev_all = cfg->variant == DDRL_SQN ? 5 : 3;
    if (h->wide) {
        wide_plan(h->wf, nev_all, B, h1, o, true, 4, 512);
        ALLOC(wpart, wide_part_floats(h->wf)); ALLOC(wconsts, 8);
    } else {
        ALLOC(set1[0], (size_t)B * h->ldx); ALLOC(set1[1], (size_t)B * h->ldx); ALLOC(set1[2], B); ALLOC(set1[3], B); ALLOC(set1[4], B);
    }
#undef ALLOC
    const size_t opt_off = reserve((2 * sizeof(OptState) + 3) / 4);
    const size_t segs_off = reserve((h->segs.size() * sizeof(Seg) + 3) / 4);
    (void)reserve(2048);
    hipError_t e = hipMalloc((void **)&h->slab, slab_floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->slab, 0, slab_floats * sizeof(float));
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc of %zu bytes failed in ddrl_dqn_create: %s", slab_floats * sizeof(float), hipGetErrorString(e));
        delete h;
        return DDRL_ERR_NOMEM;
    }
    for (auto &it : items) *it.p = h->slab + it.off;
    h->ring_idx = reinterpret_cast<long long *>(ring_idx_f);   // (slab offsets are multiples of 64 floats: 8-byte aligned)
    h->opt = reinterpret_cast<OptState *>(h->slab + opt_off);
    h->segs_d = reinterpret_cast<Seg *>(h->slab + segs_off);
    DDRL_HIP_CHECK(hipMemcpy(h->segs_d, h->segs.data(), h->segs.size() * sizeof(Seg), hipMemcpyHostToDevice));
    {
        OptState os{};
        os.b1p_pi = os.b1p_q = (float)cfg->beta1;
        os.b2p_pi = os.b2p_q = (float)cfg->beta2;
        DDRL_HIP_CHECK(hipMemcpy(h->opt, &os, sizeof(os), hipMemcpyHostToDevice));
        h->opt_cur = 0;
    }
    if (h->wide) {
        const float c8[8] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        DDRL_HIP_CHECK(hipMemcpy(h->wconsts, c8, sizeof(c8), hipMemcpyHostToDevice));
        DDRL_HIP_CHECK(wide_prepare());
    }
    k_fill_col<<<(B + 255) / 256, 256>>>(h->x1, B, h->ldx, o, 1.0f);
    k_fill_col<<<(B + 255) / 256, 256>>>(h->x2, B, h->ldx, o, 1.0f);
    if (!h->wide) {
        k_fill_col<<<(B + 255) / 256, 256>>>(h->set1[0], B, h->ldx, o, 1.0f);
        k_fill_col<<<(B + 255) / 256, 256>>>(h->set1[1], B, h->ldx, o, 1.0f);
    }
    k_fill_col<<<(5 * B + 255) / 256, 256>>>(h->H1, 5ll * B, h->ldh1, h1, 1.0f);
    k_fill_col<<<(5 * B + 255) / 256, 256>>>(h->H2, 5ll * B, h->ldh2, h2, 1.0f);
    DDRL_LAUNCH_CHECK();
    DDRL_HIP_CHECK(hipDeviceSynchronize());
    const float *Pm = h->main_p, *Pt = h->target_p;
    const long long BH1 = (long long)B * h->ldh1, BH2 = (long long)B * h->ldh2, BQ = (long long)B * h->ldq;
    // evaluations (input, parameters, network): DDQN q(x), q(x2), q_target(x2); SQN q1(x), q1(x2), q2(x), q1_target(x2), q2_target(x2)
    const bool sqn = cfg->variant == DDRL_SQN;
    const int nev = sqn ? 5 : 3;
    const float *xin[5] = {h->x1, h->x2, sqn ? h->x1 : h->x2, h->x2, h->x2};
    const float *par[5] = {Pm, Pm, sqn ? Pm : Pt, Pt, Pt};
    const int net[5] = {0, 0, sqn ? 1 : 0, 0, 1};
    for (int ev = 0; ev < nev; ++ev) {
        const int n = net[ev];
        if (h->wide) {
            h->wf.ev[ev] = WideEval{xin[ev], par[ev] + h->W1[n], par[ev] + h->b1[n], h->H1 + ev * BH1, h->ldx};
            h->wf_x2[ev] = xin[ev] == h->x2;
        }
        gemm_add(h->g_f1, gemm_fwd(xin[ev], h->ldx, par[ev] + h->W1[n], par[ev] + h->b1[n], h->H1 + ev * BH1, h->ldh1, B, o, h1));
        if (!h->wide) gemm_add(h->g_f1_s1, gemm_fwd(h->set1[xin[ev] == h->x2 ? 1 : 0], h->ldx, par[ev] + h->W1[n], par[ev] + h->b1[n], h->H1 + ev * BH1, h->ldh1, B, o, h1));
        gemm_add(h->g_f2, gemm_fwd(h->H1 + ev * BH1, h->ldh1, par[ev] + h->W2[n], par[ev] + h->b2[n], h->H2 + ev * BH2, h->ldh2, B, h1, h2));
        GemmJob j = gemm_fwd(h->H2 + ev * BH2, h->ldh2, par[ev] + h->W3[n], par[ev] + h->b3[n], h->Q + ev * BQ, h->ldq, B, h2, A);
        j.relu = 0;
        gemm_add(h->g_f3, j);
    }
    float *G = h->grad;
    const int gev[2] = {0, 2};  // differentiated evaluation of network n: q(x) / q1(x), q2(x)
    for (int n = 0; n < h->nnet; ++n) {
        const int ev = gev[n];
        float *dQ = h->dQ + (long long)n * BQ, *dZ2 = h->dZ2 + (long long)n * B * h2, *dZ1 = h->dZ1 + (long long)n * B * h1;
        // (dZ2 = (dQ * W3^T) .* (H2 > 0) comes out of k_dqn_head) the head kernels' gradient [H2 | 1]^T dQ rides in the layer-2 backward launch
        gemm_add(h->g_b2, gemm_wgrad(h->H2 + ev * BH2, h->ldh2, h2, dQ, h->ldq, A, G + h->W3[n], A, B));
        gemm_add(h->g_b2, gemm_dgrad(dZ2, Pm + h->W2[n], h->H1 + ev * BH1, h->ldh1, dZ1, B, h1, h2));
        gemm_add(h->g_b2, gemm_wgrad(h->H1 + ev * BH1, h->ldh1, h1, dZ2, h2, h2, G + h->W2[n], h2, B));
        gemm_add(h->g_b1, gemm_wgrad(h->x1, h->ldx, o, dZ1, h1, h1, G + h->W1[n], h1, B));
        if (!h->wide) gemm_add(h->g_b1_s1, gemm_wgrad(h->set1[0], h->ldx, o, dZ1, h1, h1, G + h->W1[n], h1, B));
        if (h->wide) {   // [dW1 ; db1] = [x | 1]^T dZ1: the bias row follows the kernel in the flat gradient
            wide_plan(h->ww[n], 1, o + 1, h1, B, false, 4, 0);
            h->ww[n].ev[0] = WideEval{h->x1, dZ1, nullptr, G + h->W1[n], h->ldx};
            h->ww[n].a_rows = o; h->ww[n].consts = h->wconsts;
        }
    }
    if (h->wide) { h->wf.part = h->wpart; h->wf.consts = h->wconsts; h->wf.a_rows = B; h->wf.ldo = h->ldh1; }
    h->act_fwd = h->act_sel = nullptr; h->act_why = nullptr; h->pack_stale = true; h->act_rows = ((long long)B + 31) & ~31ll;
    h->sk_on = false; h->sk_frags_d = nullptr; h->sk_slab = nullptr; h->sk_flag = nullptr; h->sk_err_h = nullptr; h->poisoned = false;
    h->steps_launched = 0; h->poison_after = getenv("DDRL_SK_POISON_AFTER") ? atoll(getenv("DDRL_SK_POISON_AFTER")) : -1;
    if (h->wide && !(getenv("DDRL_WIDE_SK") && atoi(getenv("DDRL_WIDE_SK")) == 0)) {
        // the wgrad as equal shares of the stage sequence over <= 512 resident workgroups (two per CU) when the shape splits that way
        int ncu = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
        std::vector<SkFrag> fr;
        const int nwg = wide_plan_sk(h->ww[0], 2 * ncu, fr);
        if (nwg > 1) {
            hipError_t e2 = hipMalloc((void **)&h->sk_frags_d, fr.size() * sizeof(SkFrag));
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&h->sk_slab, (size_t)nwg * 4 * WD_NB * 16 * 64 * sizeof(float));
            if (e2 == hipSuccess) e2 = hipMalloc((void **)&h->sk_flag, (size_t)(nwg + 1) * sizeof(int));
            if (e2 == hipSuccess) e2 = hipMemset(h->sk_flag, 0, (size_t)(nwg + 1) * sizeof(int));
            if (e2 == hipSuccess) e2 = hipMemcpy(h->sk_frags_d, fr.data(), fr.size() * sizeof(SkFrag), hipMemcpyHostToDevice);
            if (e2 == hipSuccess) e2 = hipHostMalloc((void **)&h->sk_err_h, sizeof(int), hipHostMallocMapped);
            if (e2 == hipSuccess) {
                *h->sk_err_h = 0;
                for (int n = 0; n < h->nnet; ++n) {
                    h->sk[n].w = h->ww[n]; h->sk[n].frags = h->sk_frags_d; h->sk[n].slab = h->sk_slab; h->sk[n].flag = h->sk_flag;
                    h->sk[n].nwg = nwg; h->sk[n].epoch = n + 1;   // (the networks' launches of one update share the flags: one epoch each)
                    h->sk[n].err = h->sk_err_h;
                }
                h->sk_on = true;
            }
        }
    }
    {
        HeadArgs &H = h->head;
        H = HeadArgs{};
        H.H2 = h->H2;
        for (int ev = 0; ev < nev; ++ev) H.W3b[ev] = par[ev] + h->W3[net[ev]];
        for (int n = 0; n < h->nnet; ++n) { H.W3n[n] = Pm + h->W3[n]; H.gev[n] = gev[n]; H.nev_of_net[n] = gev[n]; }   // evaluation gev[n] runs on network n's main copy
        H.ldw = (int)pad4((long long)(h2 + 1) * A);
        H.acts = h->acts; H.rew = h->rew; H.done = h->done;
        H.Q = h->Q; H.dQ = h->dQ; H.dZ2 = h->dZ2; H.part = h->hpart; H.qsel = sqn ? nullptr : h->qsel;
        H.B = B; H.A = A; H.ldq = h->ldq; H.h2 = h2; H.ldh2 = h->ldh2; H.nev = nev; H.nnet = h->nnet; H.sqn = sqn ? 1 : 0;
        H.gamma = (float)cfg->gamma; H.alpha = (float)cfg->alpha;
        if (h->sk_on) { H.zero_words = h->sk_flag; H.n_zero = h->sk[0].nwg + 1; }   // this update's k_wide_sk polls them
    }
    h->ad = AdamArgs{h->main_p, h->target_p, h->m, h->v, h->grad, h->opt, h->opt + 1, h->total_int, 0, 0,
                     (float)cfg->lr, (float)cfg->beta1, (float)cfg->beta2, (float)cfg->adam_eps,
                     (float)cfg->polyak, (float)(1.0 - cfg->polyak), nullptr, 0, 0, 0, 0, 0u};
    // every exit below this point owns the slab and the stream-K buffers: failures go through ddrl_dqn_destroy
    if (head_lds_bytes(h->head) > 150 * 1024) {
        ddrl::set_error("hidden2 too wide for the head kernel's LDS staging");
        ddrl_dqn_destroy(h);
        return DDRL_ERR_BAD_ARG;
    }
    if (const int lrc = head_grant_lds(device, 0, head_lds_bytes(h->head))) {
        ddrl_dqn_destroy(h);
        return lrc;
    }
    {   // the acting forward, where k_actor_fwd takes the shape (direct_ok of sac1_layout.h on (obs, half, h1, h2))
        if (A > ddrl_sel::MAXQ) h->act_why = "n_actions > 8 (the acting forward has 8 head rows)";
        else if (o + 1 > 13 || o + h->half > 12) h->act_why = "observations too wide for the direct-operand layer 1 (obs_dim + ceil(n_actions / 2) <= 12)";
        else if (h1 % 4 || h2 % 4 || h1 > 512 || h2 > 512) h->act_why = "hidden sizes outside the direct-operand limits (multiples of 4, <= 512)";
        else if (h->act_rows > 32 * 4095) h->act_why = "batch too large for the acting forward's row tiles";
        else {
            ddrl_sac1_config_t pc{};
            pc.obs_dim = o; pc.act_dim = h->half; pc.hidden1 = h1; pc.hidden2 = h2; pc.batch = 32; pc.variant = DDRL_SAC1;
            pc.alpha = 0.1; pc.gamma = cfg->gamma; pc.lr = cfg->lr; pc.polyak = cfg->polyak; pc.beta1 = cfg->beta1; pc.beta2 = cfg->beta2;
            pc.adam_eps = cfg->adam_eps; pc.act_scale = 1.0;
            int arc = ddrl_actor_create(&h->act_fwd, device, &pc, h->act_rows);
            if (arc == DDRL_OK) arc = ddrl_actor_create(&h->act_sel, device, &pc, h->act_rows);
            if (arc != DDRL_OK) { ddrl_dqn_destroy(h); return arc; }
            if (!ddrl_actor_internal_view(h->act_fwd).ok) {
                (void)ddrl_actor_destroy(h->act_fwd); (void)ddrl_actor_destroy(h->act_sel);
                h->act_fwd = h->act_sel = nullptr;
                h->act_why = "the direct-operand kernels are switched off (DDRL_SAC1_GENERIC)";
            }
        }
    }
    *out = h;
    return DDRL_OK;
}

// network 0 of main -> the acting forwards' operand layout (three launches on `s`)
static int dqn_pack_acting(ddrl_dqn *h, hipStream_t s) {
    if (!h->act_fwd) return DDRL_OK;
    const ddrl_dqn_config_t &c = h->cfg;
    QPiArgs a{h->main_p + h->W1[0], h->main_p + h->W2[0], h->main_p + h->W3[0], h->main_p + h->b3[0], h->pi_flat,
              (long long)c.obs_dim * c.hidden1 + c.hidden1, (long long)c.hidden1 * c.hidden2 + c.hidden2, c.hidden2, c.n_actions, h->half};
    k_q_to_pi<<<128, 256, 0, s>>>(a);
    DDRL_LAUNCH_CHECK();
    int rc = ddrl_actor_set_weights(h->act_fwd, h->pi_flat, s);
    if (rc == DDRL_OK) rc = ddrl_actor_set_weights(h->act_sel, h->pi_flat, s);
    if (rc == DDRL_OK) h->pack_stale = false;
    return rc;
}

int ddrl_dqn_set_weights(ddrl_dqn_t *h, const float *flat_main_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_main_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    h->poisoned = false;   // fresh parameters (main and target)
    // main AND target: Learner.set_weights runs target_init (algos/dqn/actor_learner.py:99-101)
    k_pack<<<dim3(64, (unsigned)h->segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, flat_main_d, h->main_p, h->target_p, 1);
    DDRL_LAUNCH_CHECK();
    return dqn_pack_acting(h, ddrl::as_stream(stream));   // eagerly: a captured acting call never replays a stale pack
}

int ddrl_dqn_wide_sk(ddrl_dqn_t *h) { return h ? (h->sk_on ? 1 : 0) : DDRL_ERR_BAD_ARG; }

int ddrl_dqn_export(ddrl_dqn_t *h, int which, float *flat_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_d != nullptr, "NULL pointer");
    float *buf = which == DDRL_SAC1_MAIN ? h->main_p : which == DDRL_SAC1_TARGET ? h->target_p : which == DDRL_SAC1_ADAM_M ? h->m :
                 which == DDRL_SAC1_ADAM_V ? h->v : which == DDRL_SAC1_GRAD ? h->grad : nullptr;
    DDRL_REQUIRE(buf != nullptr, "unknown buffer id");
    ddrl::DeviceGuard g(h->device);
    if (int prc = dqn_poison_check(h, ddrl::as_stream(stream), true)) return prc;   // (drains the stream while the stream-K kernel is in use)
    k_pack<<<dim3(64, (unsigned)h->segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, buf, flat_d, nullptr, 0);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_dqn_import(ddrl_dqn_t *h, int which, const float *flat_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_d != nullptr, "NULL pointer");
    // MAIN alone (no target_init), TARGET, or an Adam slot: what a resumed learner / a test with its own targets sets
    float *buf = which == DDRL_SAC1_MAIN ? h->main_p : which == DDRL_SAC1_TARGET ? h->target_p : which == DDRL_SAC1_ADAM_M ? h->m :
                 which == DDRL_SAC1_ADAM_V ? h->v : nullptr;
    DDRL_REQUIRE(buf != nullptr, "unknown or read-only buffer id");
    ddrl::DeviceGuard g(h->device);
    if (which == DDRL_SAC1_MAIN) h->poisoned = false;   // fresh main parameters (a resumed learner imports target and moments next)
    k_pack<<<dim3(64, (unsigned)h->segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, flat_d, buf, nullptr, 1);
    DDRL_LAUNCH_CHECK();
    if (which == DDRL_SAC1_MAIN) return dqn_pack_acting(h, ddrl::as_stream(stream));
    return DDRL_OK;
}

}  // extern "C"

// The update's last launch: flat Adam + polyak out of the current copy of the optimizer state into the other one, + one workgroup: the
// loss mean from k_dqn_head's partials
static void dqn_launch_adam(ddrl_dqn_t *h, float *loss_d, hipStream_t s) {
    const int B = h->cfg.batch;
    const long long blocks = (h->total_int / 4 + 255) / 256;
    h->ad.adam_blocks = (int)blocks;
    h->ad.opt = h->opt + h->opt_cur; h->ad.opt_next = h->opt + (h->opt_cur ^ 1);
    h->opt_cur ^= 1;
    h->ad.loss_part = h->hpart; h->ad.loss_out = h->loss; h->ad.loss_out2 = loss_d; h->ad.loss_n = (B + HEAD_ROWS - 1) / HEAD_ROWS; h->ad.loss_scale = 0.5f / (float)B;
    k_adam_polyak<<<(unsigned)blocks + 1, 256, 0, s>>>(h->ad);
}

// The launches of one update.  ev != nullptr: an event after every stage (DDRL_DQN_STAGES + 1 events, ev[0] first) for
// ddrl_dqn_step_timed; the update itself is the same either way.
// ridx != nullptr: obs1_d / obs2_d are the replay ring's observation arrays and batch row r is their row ridx[r] (ddrl_dqn_step_ring).
// u8 (with ridx, 16-byte aligned arrays, obs_dim % 16 == 0): those arrays are the BYTES of a compact ring — the layer-1 forward reads them as
// they lie, the gradient's obs1 copy is converted by its gather.
static int dqn_step_launch(ddrl_dqn_t *h, const float *obs1_d, const float *obs2_d, const float *acts_d, const float *rews_d, const float *done_d,
                           float *loss_d, float *q_d, hipStream_t s, hipEvent_t *ev, const long long *ridx = nullptr, bool u8 = false) {
    const int B = h->cfg.batch, o = h->cfg.obs_dim;
    int e = 0;
    if (int prc = dqn_poison_check(h, s, false)) return prc;   // a stream-K combine of an EARLIER step gave up waiting for its partner
#define STAGE_MARK() do { if (ev) DDRL_HIP_CHECK(hipEventRecord(ev[e++], s)); } while (0)
    STAGE_MARK();
    // wide layer 1 reads the caller's observation rows in place (16-byte aligned rows: obs_dim % 4 == 0 there) and the head kernel
    // the caller's acts / rews / done: no staging launch at all; otherwise everything is staged into the padded images
    const bool in_place = h->wide && al16(obs1_d) && al16(obs2_d);
    if (!in_place) {
        const int n = B * o > B ? B * o : B;
        k_dqn_stage<<<(n + 255) / 256, 256, 0, s>>>(obs1_d, obs2_d, acts_d, rews_d, done_d, h->x1, h->x2, h->acts, h->rew, h->done, B, o, h->ldx);
    }
    STAGE_MARK();   // 0 stage
    if (h->wide) {
        WideArgs f = h->wf;
        for (int k = 0; k < f.nev; ++k) {
            f.ev[k].A = in_place ? (h->wf_x2[k] ? obs2_d : obs1_d) : (h->wf_x2[k] ? h->x2 : h->x1);
            f.ev[k].lda = in_place ? o : h->ldx;
            f.ev[k].ridx = ridx;
        }
        f.a_u8 = u8 ? 1 : 0;   // (lda = obs_dim is then the row stride in bytes)
        launch_wide_fwd(f, s);
    } else {
        launch_gemm(h->g_f1, s);
    }
    STAGE_MARK();   // 1 layer-1 forward (+ split-K reduce)
    launch_gemm(h->g_f2, s);
    STAGE_MARK();   // 2 layer-2 forward
    {
        HeadArgs H = h->head;
        if (in_place) { H.acts = acts_d; H.rew = rews_d; H.done = done_d; }
        k_dqn_head<<<(unsigned)((B + HEAD_ROWS - 1) / HEAD_ROWS), 256, head_lds_bytes(H), s>>>(H);
    }
    STAGE_MARK();   // 3 head: Q of every evaluation, backup / loss / dQ, dZ2
    STAGE_MARK();   // 4 (folded into 3)
    STAGE_MARK();   // 5 (folded into 3 and 6)
    launch_gemm(h->g_b2, s);
    STAGE_MARK();   // 6 layer-2 dgrad + wgrad
    if (h->wide) {
        // ring rows (ridx): the gradient contracts over the batch rows, so it reads a gathered copy of obs1 (the one array of the
        // batch that is still materialised: 58 MB of the 231)
        const bool direct = in_place && !ridx;
        if (ridx && u8) k_dqn_gather_rows_u8<<<B, 256, 0, s>>>(reinterpret_cast<const unsigned char *>(obs1_d), ridx, h->x1, o, h->ldx);
        else if (ridx) k_dqn_gather_rows<<<B, 256, 0, s>>>(obs1_d, ridx, h->x1, o, h->ldx);
        for (int nn = 0; nn < h->nnet; ++nn) {
            if (h->sk_on) {
                SkArgs g = h->sk[nn];
                g.w.ev[0].A = direct ? obs1_d : h->x1;
                g.w.ev[0].lda = direct ? o : h->ldx;
                launch_wide_sk(g, s);
            } else {
                WideArgs g = h->ww[nn];
                g.ev[0].A = direct ? obs1_d : h->x1;
                g.ev[0].lda = direct ? o : h->ldx;
                launch_wide_wgrad(g, s);
            }
        }
    } else {
        launch_gemm(h->g_b1, s);
    }
    STAGE_MARK();   // 7 layer-1 wgrad
    dqn_launch_adam(h, loss_d, s);
    STAGE_MARK();   // 8 flat Adam + polyak
#undef STAGE_MARK
    DDRL_LAUNCH_CHECK();
    h->pack_stale = true;   // main moved: the next acting forward repacks its operand copy first
    if (++h->steps_launched == h->poison_after && h->sk_on && h->sk_err_h) *h->sk_err_h = 1;   // (test hook: what a timed-out combine stores)
    if (q_d) DDRL_HIP_CHECK(hipMemcpy2DAsync(q_d, (size_t)h->cfg.n_actions * sizeof(float), h->Q, (size_t)h->ldq * sizeof(float),
                                             (size_t)h->cfg.n_actions * sizeof(float), (size_t)B, hipMemcpyDeviceToDevice, s));
    return DDRL_OK;
}

extern "C" {

int ddrl_dqn_step(ddrl_dqn_t *h, const float *obs1_d, const float *obs2_d, const float *acts_d, const float *rews_d, const float *done_d,
                  float *loss_d, float *q_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && obs1_d && obs2_d && acts_d && rews_d && done_d, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    return dqn_step_launch(h, obs1_d, obs2_d, acts_d, rews_d, done_d, loss_d, q_d, ddrl::as_stream(stream), nullptr);
}

int ddrl_dqn_step_ring(ddrl_dqn_t *h, ddrl_replay_t *replay, float *loss_d, float *q_d, int64_t *idx_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr, "NULL handle");
    const int B = h->cfg.batch, o = h->cfg.obs_dim;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    DDRL_REQUIRE(rv.device == h->device, "the replay ring lives on another device than the learner");
    if (!h->wide) {
        ddrl::set_error("ddrl_dqn_step_ring needs the wide layer-1 path (obs_dim >= 1024): use ddrl_replay_sample + ddrl_dqn_step");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(rv.ring.n_arr == 5 && rv.ring.w[0] == o && rv.ring.w[1] == o && rv.ring.w[2] == 1 && rv.ring.w[3] == 1 && rv.ring.w[4] == 1,
                 "the ring must be (obs1[obs_dim], obs2[obs_dim], acts, rews, done) of this learner's observation width");
    // a compact (uint8) ring: both observation arrays as bytes, whole 16-byte chunks per row (the layer-1 forward's LDS-DMA and the
    // gradient's gather load 16 bytes at a time); what this does not take goes through ddrl_replay_sample + ddrl_dqn_step
    const bool u8 = rv.ring.kind[0] == 1 && rv.ring.kind[1] == 1;
    if (!u8 && (rv.ring.kind[0] || rv.ring.kind[1])) {
        ddrl::set_error("ddrl_dqn_step_ring reads both observation arrays as float32 rows or both as uint8 rows: this ring has one compact (uint8) "
                        "and one float32 observation array; use ddrl_replay_sample + ddrl_dqn_step");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (u8 && (o % 16 != 0 || !al16(rv.ring.a[0]) || !al16(rv.ring.a[1]))) {
        ddrl::set_error("ddrl_dqn_step_ring reads a compact (uint8) ring in 16-byte chunks: obs_dim must be a multiple of 16 (and the arrays 16-byte "
                        "aligned); use ddrl_replay_sample + ddrl_dqn_step");
        return DDRL_ERR_UNSUPPORTED;
    }
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    long long *idx = h->ring_idx;
    int rc = ddrl_replay_sample_indices(replay, B, reinterpret_cast<int64_t *>(idx), stream);   // np.random.randint(0, size, B); sample_times += 1
    if (rc != DDRL_OK) return rc;
    k_dqn_gather3<<<(B + 255) / 256, 256, 0, s>>>(rv.ring.a[2], rv.ring.a[3], rv.ring.a[4], idx, h->acts, h->rew, h->done, reinterpret_cast<long long *>(idx_out_d), B);
    return dqn_step_launch(h, rv.ring.a[0], rv.ring.a[1], h->acts, h->rew, h->done, loss_d, q_d, s, nullptr, idx, u8);
}

int ddrl_dqn_step_timed(ddrl_dqn_t *h, const float *obs1_d, const float *obs2_d, const float *acts_d, const float *rews_d, const float *done_d,
                        int reps, float *stage_ms_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && obs1_d && obs2_d && acts_d && rews_d && done_d && stage_ms_h, "NULL pointer");
    DDRL_REQUIRE(reps > 0 && reps <= 64, "reps outside [1, 64]");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    constexpr int NE = DDRL_DQN_STAGES + 1;
    std::vector<hipEvent_t> ev((size_t)reps * NE);
    for (auto &e : ev) DDRL_HIP_CHECK(hipEventCreate(&e));
    int rc = DDRL_OK;
    for (int r = 0; r < reps && rc == DDRL_OK; ++r) rc = dqn_step_launch(h, obs1_d, obs2_d, acts_d, rews_d, done_d, nullptr, nullptr, s, ev.data() + (size_t)r * NE);
    if (rc == DDRL_OK) {
        DDRL_HIP_CHECK(hipStreamSynchronize(s));
        for (int k = 0; k < DDRL_DQN_STAGES; ++k) stage_ms_h[k] = 0.f;
        for (int r = 0; r < reps; ++r)
            for (int k = 0; k < DDRL_DQN_STAGES; ++k) {
                float ms = 0.f;
                DDRL_HIP_CHECK(hipEventElapsedTime(&ms, ev[(size_t)r * NE + k], ev[(size_t)r * NE + k + 1]));
                stage_ms_h[k] += ms / (float)reps;
            }
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    return rc;
}

// self.q for n <= batch observations (Actor.get_action / the learner's q output): rows of q(x) main
int ddrl_dqn_q(ddrl_dqn_t *h, const float *obs_d, int64_t n, float *q_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && obs_d != nullptr && q_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(n > 0 && n <= h->cfg.batch, "n outside [1, batch]");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const int o = h->cfg.obs_dim;
    DDRL_HIP_CHECK(hipMemcpy2DAsync(h->x1, (size_t)h->ldx * sizeof(float), obs_d, (size_t)o * sizeof(float), (size_t)o * sizeof(float), (size_t)n,
                                    hipMemcpyDeviceToDevice, s));
    if (h->wide) launch_wide_fwd(h->wf, s);   // (evaluations read the staged images here)
    else launch_gemm(h->g_f1, s);   // all three evaluations run (rows beyond n hold the previous batch): simple, off the hot path
    launch_gemm(h->g_f2, s);
    launch_gemm(h->g_f3, s);
    DDRL_LAUNCH_CHECK();
    DDRL_HIP_CHECK(hipMemcpy2DAsync(q_d, (size_t)h->cfg.n_actions * sizeof(float), h->Q, (size_t)h->ldq * sizeof(float),
                                    (size_t)h->cfg.n_actions * sizeof(float), (size_t)n, hipMemcpyDeviceToDevice, s));
    return DDRL_OK;
}

int ddrl_dqn_act(ddrl_dqn_t *h, const float *obs_d, int64_t n, int mode, float greedy_prob, uint32_t seed, uint64_t ctr, float *act_d,
                 float *q_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && obs_d != nullptr && act_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(n > 0 && n <= h->cfg.batch, "n outside [1, batch]");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const ddrl_dqn_config_t &c = h->cfg;
    SelArgs a{};
    a.n = n; a.A = c.n_actions; a.half = h->half; a.nt2 = (c.hidden2 + 31) / 32; a.sqn = c.variant == DDRL_SQN; a.deterministic = mode == DDRL_ACT_DETERMINISTIC;
    a.greedy_prob = greedy_prob; a.alpha = (float)c.alpha; a.seed = seed; a.ctr = ctr; a.act_out = act_d; a.q_out = q_out_d;
    if (h->act_fwd) {
        // its own set of observation rows and partials: the rollout's observations and everything a learner step reads stay as they are.
        // The forward runs whole 32-row tiles: the rows beyond n hold an earlier call's observations (zeros at first) and are never read
        const ddrl_actor_rollout_view v = ddrl_actor_internal_view(h->act_sel);
        if (h->pack_stale)
            if (const int rc = dqn_pack_acting(h, s)) return rc;
        DDRL_HIP_CHECK(hipMemcpyAsync(v.obs, obs_d, (size_t)n * c.obs_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
        a.hp_rows = (n + 31) & ~31ll;
        if (const int rc = ddrl_actor_internal_forward(h->act_sel, a.hp_rows, stream, 0)) return rc;
        a.hp = v.hp; a.b_lo = v.bmu; a.b_hi = v.bls;
        if (c.n_actions <= 4) k_dqn_select<4><<<(unsigned)((n + 63) / 64), 64, 0, s>>>(a);
        else k_dqn_select<8><<<(unsigned)((n + 63) / 64), 64, 0, s>>>(a);
        DDRL_LAUNCH_CHECK();
        return DDRL_OK;
    }
    // outside the acting forward's envelope (wide observations, ...): ddrl_dqn_q's launches + the selection kernel on its Q image.  The staged
    // rows, H1 / H2 / Q are scratch that every learner step rewrites before it reads them; parameters and optimizer state are not touched.
    const int o = c.obs_dim;
    DDRL_HIP_CHECK(hipMemcpy2DAsync(h->x1, (size_t)h->ldx * sizeof(float), obs_d, (size_t)o * sizeof(float), (size_t)o * sizeof(float), (size_t)n,
                                    hipMemcpyDeviceToDevice, s));
    if (h->wide) launch_wide_fwd(h->wf, s);
    else launch_gemm(h->g_f1, s);
    launch_gemm(h->g_f2, s);
    launch_gemm(h->g_f3, s);
    a.Q = h->Q; a.ldq = h->ldq;
    k_dqn_select<4><<<(unsigned)((n + 63) / 64), 64, 0, s>>>(a);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

// The version store of the acting forward the fused rollout step runs (act_fwd): the inner actor handle owns the slab, the slots and the
// planning kernels.  act_sel (ddrl_dqn_act's rows) gets none: get_actions keeps acting on the newest weights.
int ddrl_dqn_versions_enable(ddrl_dqn_t *h, int32_t n_slots, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    if (!h->act_fwd) {
        ddrl::set_error("ddrl_dqn_versions_enable: no acting forward to keep versions of: %s", h->act_why ? h->act_why : "shape outside the envelope");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(n_slots >= 2 && n_slots <= VER_MAX_SLOTS, "n_slots outside [2, 2048]");
    DDRL_REQUIRE(ddrl_actor_internal_versions(h->act_fwd) == 0, "version store already enabled");
    // slot 0 = the weights held now: a learner step's pending repack comes first
    if (const int rc = ddrl_dqn_internal_repack(h, stream)) return rc;
    return ddrl_actor_versions_enable(h->act_fwd, n_slots, stream);
}

int ddrl_dqn_versions_state(ddrl_dqn_t *h, int32_t *slot_of_env_d, int32_t *state_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(h->act_fwd != nullptr && ddrl_actor_internal_versions(h->act_fwd) > 0, "version store not enabled (ddrl_dqn_versions_enable)");
    return ddrl_actor_versions_state(h->act_fwd, slot_of_env_d, state_h, stream);
}

int ddrl_dqn_versions_adopt(ddrl_dqn_t *h, const uint8_t *ended_d, int64_t n, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(h->act_fwd != nullptr && ddrl_actor_internal_versions(h->act_fwd) > 0, "version store not enabled (ddrl_dqn_versions_enable)");
    return ddrl_actor_versions_adopt(h->act_fwd, ended_d, n, stream);
}

}  // extern "C"

// ---- internal (env.hip: ddrl_rollout_step_discrete) ---------------------------------------------------------------
// the configuration and the device, for the handle-fed evaluation entry points (eval3.hip; declared in eval_episodes.h)
int ddrl_dqn_internal_config(ddrl_dqn_t *h, ddrl_dqn_config_t *cfg_out, int *device_out) {
    if (!h) return DDRL_ERR_BAD_ARG;
    *cfg_out = h->cfg; *device_out = h->device;
    return DDRL_OK;
}

ddrl_dqn_rollout_view ddrl_dqn_internal_view(ddrl_dqn_t *h) {
    ddrl_dqn_rollout_view v{};
    if (!h) return v;
    v.device = h->device; v.why = h->act_why;
    v.obs_dim = h->cfg.obs_dim; v.n_actions = h->cfg.n_actions; v.half = h->half; v.nt2 = (h->cfg.hidden2 + 31) / 32; v.batch = h->cfg.batch;
    v.sqn = h->cfg.variant == DDRL_SQN; v.alpha = (float)h->cfg.alpha;
    if (!h->act_fwd) return v;
    const ddrl_actor_rollout_view av = ddrl_actor_internal_view(h->act_fwd);
    v.ok = 1; v.obs = av.obs; v.hp = av.hp; v.b_lo = av.bmu; v.b_hi = av.bls;
    v.rows = av.max_rows; v.ver = av.ver; v.vb_lo = av.vbmu; v.vb_hi = av.vbls;
    return v;
}

int ddrl_dqn_internal_repack(ddrl_dqn_t *h, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->act_fwd != nullptr, "no acting forward");
    if (!h->pack_stale) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    return dqn_pack_acting(h, ddrl::as_stream(stream));
}

int ddrl_dqn_internal_forward(ddrl_dqn_t *h, long long n, void *stream, int versioned) {
    if (const int rc = ddrl_dqn_internal_repack(h, stream)) return rc;
    return ddrl_actor_internal_forward(h->act_fwd, n, stream, versioned);
}

// ---- internal (dqn_loop.hip: ddrl_dqn_loop_*) ---------------------------------------------------------------------
// internal (replay.hip): the host side of a draw that one of this file's kernels performs
bool ddrl_replay_internal_has_feed(ddrl_replay_t *h);
int ddrl_replay_internal_require_rows(ddrl_replay_t *h, void *stream);

// The envelope of the learner loop: the narrow path on a five-array float32 ring of this learner's widths that the one-workgroup sampler
// can draw and gather at cfg.batch.  Changes nothing but the head kernel's LDS attribute.
int ddrl_dqn_internal_loop_check(ddrl_dqn_t *h, ddrl_replay_t *replay) {
    DDRL_REQUIRE(h != nullptr && replay != nullptr, "NULL handle");
    const int B = h->cfg.batch, o = h->cfg.obs_dim;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    DDRL_REQUIRE(rv.device == h->device, "the replay ring lives on another device than the learner");
    if (h->wide) {
        ddrl::set_error("ddrl_dqn_loop: the wide layer-1 path (obs_dim >= 1024, its stream-K weight gradient spins on flags and can poison the learner) "
                        "is kept out of graphs: use ddrl_dqn_step_ring per update");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (ddrl_replay_is_window_ring(replay, 0, 0)) {
        ddrl::set_error("ddrl_dqn_loop: an n-step window ring is not supported by the DQN / SQN learners");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(rv.ring.n_arr == 5 && rv.ring.w[0] == o && rv.ring.w[1] == o && rv.ring.w[2] == 1 && rv.ring.w[3] == 1 && rv.ring.w[4] == 1,
                 "the ring must be (obs1[obs_dim], obs2[obs_dim], acts, rews, done) of this learner's observation width");
    for (int j = 0; j < 5; ++j)
        if (rv.ring.kind[j]) {
            ddrl::set_error("ddrl_dqn_loop: a compact (uint8) ring is not supported: the loop's sampler gathers float32 rows");
            return DDRL_ERR_UNSUPPORTED;
        }
    const long long bytes = (long long)B * (2ll * o + 3) * (long long)sizeof(float);   // what ddrl_replay_can_fuse caps (an empty ring is a run-time error)
    if (B > ddrl_replay_dev::MAX_FUSED_BATCH || bytes > ddrl_replay_dev::MAX_FUSED_BYTES) {
        ddrl::set_error("ddrl_dqn_loop: batch %d x %lld bytes per row is over the one-workgroup sampler's caps (%d rows, %lld bytes)", B,
                        (2ll * o + 3) * (long long)sizeof(float), ddrl_replay_dev::MAX_FUSED_BATCH, ddrl_replay_dev::MAX_FUSED_BYTES);
        return DDRL_ERR_UNSUPPORTED;
    }
    // k_dqn_head_sample's static LDS is the head's 1.8 KB + the sampler's two MT19937 states (5 KB; with the gather out of the draw its index
    // array is gone): beside the 150 KB ddrl_dqn_create allows the head's staging it stays inside the CU's 160 KB
    return head_grant_lds(h->device, 1, head_lds_bytes(h->head));
}

static SetSampler dqn_set_sampler(ddrl_dqn_t *h, ddrl_replay_t *replay, int set) {
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    SetSampler m{};
    m.st = rv.state; m.ring = rv.ring; m.idx = h->ring_idx;
    m.x1 = set ? h->set1[0] : h->x1; m.x2 = set ? h->set1[1] : h->x2;
    m.acts = set ? h->set1[2] : h->acts; m.rew = set ? h->set1[3] : h->rew; m.done = set ? h->set1[4] : h->done;
    m.B = h->cfg.batch; m.obs = h->cfg.obs_dim; m.ldx = h->ldx;
    return m;
}

// sample_batch into input set `set` as a launch of its own.  rows: ask the ring first whether it has any (never inside a capture: the
// mirror may have to be read back)
int ddrl_dqn_internal_sample_into(ddrl_dqn_t *h, ddrl_replay_t *replay, int set, bool rows, void *stream) {
    if (rows)
        if (const int rc = ddrl_replay_internal_require_rows(replay, stream)) return rc;
    ddrl::DeviceGuard g(h->device);
    k_dqn_sample<<<1, 256, 0, ddrl::as_stream(stream)>>>(dqn_set_sampler(h, replay, set));
    DDRL_LAUNCH_CHECK();
    ddrl_replay_note_sample(replay);
    return DDRL_OK;
}

// agent.train on input set `set`: ddrl_dqn_step's launches without the staging one.  ride != nullptr: the next update's sample_batch out of
// that ring goes into the other set as one more workgroup of the head launch.
int ddrl_dqn_internal_update(ddrl_dqn_t *h, int set, ddrl_replay_t *ride, float *loss_d, void *stream) {
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const int B = h->cfg.batch;
    launch_gemm(set ? h->g_f1_s1 : h->g_f1, s);
    launch_gemm(h->g_f2, s);
    HeadArgs H = h->head;
    if (set) { H.acts = h->set1[2]; H.rew = h->set1[3]; H.done = h->set1[4]; }
    const int head_blocks = (B + HEAD_ROWS - 1) / HEAD_ROWS;
    if (ride) k_dqn_head_sample<<<(unsigned)head_blocks + 1, 256, head_lds_bytes(H), s>>>(H, dqn_set_sampler(h, ride, set ^ 1), head_blocks);
    else k_dqn_head<<<(unsigned)head_blocks, 256, head_lds_bytes(H), s>>>(H);
    launch_gemm(h->g_b2, s);
    launch_gemm(set ? h->g_b1_s1 : h->g_b1, s);
    dqn_launch_adam(h, loss_d, s);
    DDRL_LAUNCH_CHECK();
    h->pack_stale = true;   // main moved: the next acting forward repacks its operand copy first
    ++h->steps_launched;
    if (ride) ddrl_replay_note_sample(ride);
    return DDRL_OK;
}

// Make copy 0 of the double-buffered optimizer state the current one, so that a captured graph starts and ends on the same copy whatever
// the number of updates it holds (a copy node of sizeof(OptState) bytes in a graph of odd length)
int ddrl_dqn_internal_opt_sync(ddrl_dqn_t *h, void *stream) {
    if (h->opt_cur == 0) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    DDRL_HIP_CHECK(hipMemcpyAsync(h->opt, h->opt + 1, sizeof(OptState), hipMemcpyDeviceToDevice, ddrl::as_stream(stream)));
    h->opt_cur = 0;
    return DDRL_OK;
}

// `n` updates ran out of captured graphs: what their launches do to the host-side state when they are issued eagerly
void ddrl_dqn_internal_note_updates(ddrl_dqn_t *h, long long n) {
    if (n <= 0) return;
    h->pack_stale = true;
    h->steps_launched += n;
}
