// What the SAC1 learner (sac1.hip) and the actor (actor.hip) share beside the device cores: the parameter layout of a policy / twin-Q
// set (external dense order <-> padded internal, row-major or direct-operand), the shape checks, the layer-1 kernel of the generic
// path and the policy head of the one-wave-per-row kernels.  Included behind sac1_direct.h (direct_ok reads its envelope constants);
// every definition has internal linkage.
#pragma once
#include "gemm_core.h"
#include "policy_row.h"

namespace {
struct L1Job {  // H1 = relu([in0 | in1] * W1 + b1); optionally also writes the concatenated input rows
    const float *in0, *in1, *W, *b;
    float *out, *aug_out;
    int d0, d1, rows, h1, ldo, aug_ld;
    int pre_only;  // 1: out = in0 * W1[0:d0] + b1 WITHOUT relu: the observation part of a Q layer 1 whose
                   //    action part is added by k_rows_a once the action exists (second-phase evaluations)
};
constexpr int MAX_L1_JOBS = 8;
struct OptState;
struct L1Jobs {
    int njobs;
    // tf.random_normal stand-in, generated here (job 0's row blocks) instead of by a kernel of its own
    int noise_on, act, n_each;
    uint32_t noise_seed;
    float *e0, *e1, *e2;
    const OptState *opt;
    L1Job job[MAX_L1_JOBS];
};

// ------------------------------------------------------------------------------------------
// K: layer 1 (K = obs_dim or obs_dim+act_dim: tiny) — VALU, threads along the output feature.
// Input rows and the W1 column block are staged in LDS with one coalesced burst each.
// ------------------------------------------------------------------------------------------
constexpr int L1_ROWS = 16;
constexpr int L1_MAXD = 40;
__global__ void __launch_bounds__(256) k_l1(L1Jobs jobs) {
    const L1Job &jb = jobs.job[blockIdx.z];
    __shared__ float s_in[L1_ROWS][L1_MAXD];
    __shared__ float s_w[L1_MAXD][256];
    const int din = jb.pre_only ? jb.d0 : jb.d0 + jb.d1;
    const int r0 = blockIdx.y * L1_ROWS;
    if (r0 >= jb.rows) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int jc = j < jb.h1 ? j : jb.h1 - 1;
    const float bj = jb.b[jc];
    for (int k0 = 0; k0 < din; k0 += 16) {  // 16 loads in flight per round trip (din <= 16: one trip)
        float wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) wv[u] = jb.W[(long long)(k0 + u < din ? k0 + u : 0) * jb.h1 + jc];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (k0 + u < din) s_w[k0 + u][threadIdx.x] = wv[u];
    }
    for (int e = threadIdx.x; e < L1_ROWS * din; e += 256) {
        const int rr = e / din, k = e - rr * din;
        const int r = r0 + rr;
        const int rc = r < jb.rows ? r : jb.rows - 1;
        const float v = (k < jb.d0) ? jb.in0[(long long)rc * jb.d0 + k] : jb.in1[(long long)rc * jb.d1 + (k - jb.d0)];
        s_in[rr][k] = v;
        if (jb.aug_out && blockIdx.x == 0 && r < jb.rows) jb.aug_out[(long long)r * jb.aug_ld + k] = v;  // [x | a] rows for the layer-1 wgrad
    }
    if (jobs.noise_on && blockIdx.z == 0 && blockIdx.x == 0) {
        // eps_x, eps_x2, eps_t for this block's rows; element index as in one flat [3][B*act] fill
        const unsigned long long base = jobs.opt->noise_ctr;
        const int per_row = 3 * jobs.act;
        for (int e = threadIdx.x; e < L1_ROWS * per_row; e += 256) {
            const int rr = e / per_row, q = e - rr * per_row;
            const int wch = q / jobs.act, c = q - wch * jobs.act;
            const int r = r0 + rr;
            if (r < jb.rows) {
                const int k = r * jobs.act + c;
                (wch == 0 ? jobs.e0 : (wch == 1 ? jobs.e1 : jobs.e2))[k] =
                    normal_at(jobs.noise_seed, base + (unsigned long long)wch * jobs.n_each + k);
            }
        }
    }
    __syncthreads();
    float acc[L1_ROWS];
#pragma unroll
    for (int rr = 0; rr < L1_ROWS; ++rr) acc[rr] = 0.f;
    for (int k = 0; k < din; ++k) {
        const float w = s_w[k][threadIdx.x];
#pragma unroll
        for (int rr = 0; rr < L1_ROWS; ++rr) acc[rr] = fmaf(s_in[rr][k], w, acc[rr]);
    }
    if (j < jb.h1) {
#pragma unroll
        for (int rr = 0; rr < L1_ROWS; ++rr) {
            const int r = r0 + rr;
            const float v = acc[rr] + bj;
            if (r < jb.rows) jb.out[(long long)r * jb.ldo + j] = jb.pre_only ? v : fmaxf(v, 0.f);
        }
    }
}

struct NetPi { const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wls, *bls; };
struct NetQ { const float *W1, *b1, *W2, *b2, *W3, *b3; };

// One policy head for one row held by one wave (hidden2 <= 512): per-dim quantities are valid in
// lanes c < act; every lane gets logp.  core.py:49-87,104-106.  `hrow` must be mask_row()ed.
// The head-kernel rows are fetched two action dims at a time (all of them at once for act <= 2).
struct HeadOut { float act, a, std, t, logp, eps; };
__device__ __forceinline__ HeadOut policy_head(const float (&hrow)[RV], int h2, int act, const NetPi &p, float eps_lane,
                                               float scale, int lane) {
    float mu = 0.f, lsr = 0.f;
    const float bm = p.bmu[lane < act ? lane : 0], bl = p.bls[lane < act ? lane : 0];
#pragma unroll
    for (int c0 = 0; c0 < MAXA; c0 += 2)
        if (c0 < act) {  // wave-uniform
            const int c1 = c0 + 1 < act ? c0 + 1 : c0;
            float wm0[RV], wl0[RV], wm1[RV], wl1[RV];
            load_row(p.Wmu, h2, lane, wm0, act, c0);
            load_row(p.Wls, h2, lane, wl0, act, c0);
            load_row(p.Wmu, h2, lane, wm1, act, c1);
            load_row(p.Wls, h2, lane, wl1, act, c1);
            const float s0 = wave_sum(dot_rv(hrow, wm0)), s1 = wave_sum(dot_rv(hrow, wl0));
            const float s2 = wave_sum(dot_rv(hrow, wm1)), s3 = wave_sum(dot_rv(hrow, wl1));
            if (lane == c0) { mu = s0 + bm; lsr = s1 + bl; }
            if (lane == c0 + 1 && c0 + 1 < act) { mu = s2 + bm; lsr = s3 + bl; }
        }
    HeadOut o;
    o.act = 0.f; o.a = 0.f; o.std = 0.f; o.t = 0.f; o.eps = eps_lane;
    float pre = 0.f, corr = 0.f;
    if (lane < act) {
        const float t = tanhf(lsr);
        const float log_std = -20.0f + 11.0f * (t + 1.0f);  // LOG_STD_MIN + 0.5*(MAX-MIN)*(ls+1), core.py:73-74
        const float std = expf(log_std);
        const float e = eps_lane;
        const float u = mu + e * std;                          // core.py:76-77
        const float z = (e * std) / (std + STD_EPS);           // == (pi - mu)/(std + EPS), core.py:31
        pre = -0.5f * ((z * z + 2.0f * log_std) + LOG2PI);
        const float a = tanhf(u);                              // core.py:83-84
        const float om = 1.0f - a * a;
        const float cl = fminf(fmaxf(om, 0.f), 1.f);           // clip_but_pass_gradient value, core.py:35-38,86
        corr = logf(cl + 1e-6f);
        o.act = a * scale; o.a = a; o.std = std; o.t = t;
    }
    float sp = 0.f, sc = 0.f;
#pragma unroll
    for (int c = 0; c < MAXA; ++c)
        if (c < act) { sp += __shfl(pre, c); sc += __shfl(corr, c); }
    o.logp = sp - sc;
    return o;
}

// ------------------------------------------------------------------------------------------
// host side: layout
// ------------------------------------------------------------------------------------------

struct Layout {
    // internal (padded) offsets
    long long pi_W1, pi_b1, pi_W2, pi_b2, pi_Wmu, pi_bmu, pi_Wls, pi_bls;
    long long q_W1[2], q_b1[2], q_W2[2], q_b2[2], q_W3[2], q_b3[2];
    long long v_W1, v_b1, v_W2, v_b2, v_W3, v_b3;  // SAC-v only (example/model.py: 'main/v')
    long long n_pi_int, total_int;
    long long n_pi, n_q, total_ext;
    std::vector<Seg> segs;  // 20 tensors in external order
    bool direct;            // layer-2 kernels k4-interleaved [Kp1/4][Np2][4] with a zero-padded bias [Np2] (sac1_direct.h)
    int Kp1, Np2;
};

static Layout make_layout(const ddrl_sac1_config_t &c, bool pi_only, bool direct = false) {
    // Internal layout: every kernel is followed IMMEDIATELY by its bias (so that a bias gradient
    // is just one more row of the kernel's wgrad GEMM); each (kernel, bias) pair starts on a
    // 16-byte boundary.  Direct path: the layer-2 kernels are stored k4-interleaved and padded to
    // whole 32-wide tiles instead (pads are zero and stay zero: their gradient is never written).
    Layout L;
    const long long o = c.obs_dim, a = c.act_dim, h1 = c.hidden1, h2 = c.hidden2;
    L.direct = direct;
    L.Kp1 = (int)((h1 + 31) & ~31ll); L.Np2 = (int)((h2 + 31) & ~31ll);
    long long in = 0, ext = 0;
    auto add = [&](long long &slot, long long n, bool pad_after) {
        slot = in;
        L.segs.push_back(Seg{ext, in, n});
        in += n;
        if (pad_after) in = pad4(in);
        ext += n;
    };
    auto add_w2 = [&](long long &wslot, long long &bslot) {
        if (!direct) { add(wslot, h1 * h2, false); add(bslot, h2, true); return; }
        in = pad4(in);
        wslot = in;
        L.segs.push_back(Seg{ext, in, h1 * h2, (int)h2, L.Np2, 1, 0});
        in += (long long)L.Kp1 * L.Np2; ext += h1 * h2;
        bslot = in;
        L.segs.push_back(Seg{ext, in, h2});
        in += L.Np2; ext += h2;
    };
    auto add_w1 = [&](long long &wslot, long long &bslot, long long D) {  // [W1 ; b1]
        if (!direct) { add(wslot, D * h1, false); add(bslot, h1, true); return; }
        in = pad4(in);
        wslot = bslot = in;   // one block array holds the kernel rows and, as input column D, the bias
        L.segs.push_back(Seg{ext, in, D * h1, (int)h1, 0, 2, 0});
        ext += D * h1;
        L.segs.push_back(Seg{ext, in, h1, (int)h1, 0, 2, (int)D});
        ext += h1;
        in += (long long)L.Kp1 * 16;
    };
    add_w1(L.pi_W1, L.pi_b1, o); add_w2(L.pi_W2, L.pi_b2);
    add(L.pi_Wmu, h2 * a, false); add(L.pi_bmu, a, true); add(L.pi_Wls, h2 * a, false); add(L.pi_bls, a, true);
    L.n_pi_int = in;
    L.n_pi = ext;
    for (int q = 0; q < 2 && !pi_only; ++q) {
        add_w1(L.q_W1[q], L.q_b1[q], o + a); add_w2(L.q_W2[q], L.q_b2[q]);
        add(L.q_W3[q], h2, false); add(L.q_b3[q], 1, true);
    }
    L.v_W1 = L.v_b1 = L.v_W2 = L.v_b2 = L.v_W3 = L.v_b3 = -1;
    if (!pi_only && c.variant == DDRL_SAC_V) {  // vf_mlp(x): obs -> h1 -> h2 -> 1 (example/core.py:112-113)
        add_w1(L.v_W1, L.v_b1, o); add_w2(L.v_W2, L.v_b2);
        add(L.v_W3, h2, false); add(L.v_b3, 1, true);
    }
    L.total_int = in;
    L.total_ext = ext;
    L.n_q = pi_only ? 0 : (ext - L.n_pi) / 2;
    return L;
}

static NetPi net_pi(const float *base, const Layout &L) {
    return NetPi{base + L.pi_W1, base + L.pi_b1, base + L.pi_W2, base + L.pi_b2,
                 base + L.pi_Wmu, base + L.pi_bmu, base + L.pi_Wls, base + L.pi_bls};
}

template <typename T>
static hipError_t dev_alloc(T **p, size_t count) {
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e == hipSuccess) e = hipMemset(*p, 0, count * sizeof(T));
    return e;
}

static int check_cfg(const ddrl_sac1_config_t *c) {
    DDRL_REQUIRE(c != nullptr, "config is NULL");
    DDRL_REQUIRE(c->obs_dim > 0 && c->act_dim > 0 && c->hidden1 > 0 && c->hidden2 > 0 && c->batch > 0, "dims must be positive");
    DDRL_REQUIRE(c->act_dim <= MAXA, "act_dim > 8 unsupported");
    DDRL_REQUIRE(c->variant == DDRL_SAC1 || c->variant == DDRL_SAC_V, "variant must be DDRL_SAC1 or DDRL_SAC_V");
    DDRL_REQUIRE(c->batch < 65536, "batch >= 65536 unsupported (packed kernel arguments)");
    DDRL_REQUIRE(c->obs_dim + c->act_dim <= L1_MAXD, "obs_dim + act_dim > 40 unsupported by the layer-1 kernel");
    DDRL_REQUIRE(c->hidden1 <= 64 * RV && c->hidden2 <= 64 * RV, "hidden sizes > 512 unsupported by the row kernels");
    return DDRL_OK;
}

// Envelope of the direct-operand path (sac1_direct.h); everything else takes the generic kernels.  A wgrad tile of k_dg contracts
// the whole batch inside one workgroup, DGMAX 8-deep groups per wave: 4 x 16 x 8 = 512 rows (beyond that the rows were dropped).
static bool direct_ok(const ddrl_sac1_config_t &c) {
    return c.hidden1 % 4 == 0 && c.hidden2 % 4 == 0 && c.hidden1 <= 512 && c.hidden2 <= 32 * DNT &&
           c.obs_dim + c.act_dim <= 12 && 2 * c.act_dim <= DFH && c.act_dim <= 4 && c.batch <= 4 * DGMAX * 8 &&
           getenv("DDRL_SAC1_GENERIC") == nullptr;
}

}  // namespace
