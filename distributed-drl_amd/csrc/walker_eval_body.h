// The BODY of the walker's evaluation kernel, ONE text for both terrain modes, included between the braces of
//   k_walker_eval     (walker_eval.hip:          WE_HC = 0, the grass terrain,    WalkerT<0>: its sweep fields at lane stride 64)
//   k_walker_hc_eval  (walker_hardcore_eval.hip: WE_HC = 1, the Hardcore terrain, WalkerT<1, 1>: its sweep fields packed)
// behind `constexpr int WE_HC = ...;`, with the kernel's argument named `a` (WalkerEvalArgs).  No include guard and no declaration at
// file scope: what the episode needs there (the arguments, we_layer2, the host half) is walker_eval_device.h, whose header comment says
// what this loop does.  It is a text and not a function template on purpose: a function is optimised on its own before it is inlined
// into its kernel, and k_walker_eval then compiles to other registers than the ones it had (22 AGPRs and 104 spilled SGPRs against 21
// and 102); included, it is token for token the body k_walker_eval had, and compiles to it (profiles/walker_eval_resource_usage.txt).
// Compiled with -ffp-contract=off; write no fused multiply-add here.
    using W = WalkerT<WE_HC, WE_HC ? 1 : 64>;
    constexpr int WE_LS = WE_HC ? 1 : 64, WE_NCOL = WE_HC ? NFWH : NFW;
    static_assert(W::LFIELDS * WE_LS <= WE_PS, "the walker's sweep fields lie inside the layer-2 slice sums");
    __shared__ float xs[WOBS];
    __shared__ float h1s[512];
    __shared__ float big[WE_PS];     // ps[16][512] from layer 2 to the slice sums' addition; the walker's sweep fields inside physics()
    __shared__ float v2[512];
    __shared__ float wh[8][512];     // head kernels by output: mu 0..3, log_std 0..3
    __shared__ float part[32][8];
    __shared__ float col[WE_NCOL];   // the episode's state-block column (n = 1): what build() writes through Sc, the terrain at WT0
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
    W e;
    float act[WACT] = {0.0f, 0.0f, 0.0f, 0.0f};   // lane 0's: zero for the reset's trip, then the policy row's
    if (tid == 0) {
        e.L = big; e.Sc = col; e.T = col + WT0; e.n = 1;
        if constexpr (WE_HC) { e.B = col + WB0; e.Cc = col + WBC0; }
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
