// k_dfwd_wide: the two forward launches of the SAC1 and the SAC-v update for input rows of up to 31 columns (obs_dim + act_dim <= 31; the bipedal
// walker: 24 / 4) — the roles of k_dfwd<0> and k_dfwd<1> (sac1_direct.h) over the WIDE layer-1 block layout (wide_pack.h, actor_wide.h:
// 32 floats per hidden unit, input column d in MFMA step 4 (d / 8) + d % 4 of lane half (d / 4) % 2, the bias as input column D).
// Included by sac1_wide.hip inside its unnamed namespace, behind sac1_direct.h (DFHead / DFArgs / DFJob, DSrc, the side-output rules,
// relu1, st_img, kline / ktouch) and wide_pack.h.  That translation unit is compiled without the packed float32 VALU forms, so nothing
// here carries a target attribute and every helper of the narrow path inlines as it does there.
//
// WORK SPLIT  one workgroup = one 32-row tile x one 32-column tile of layer 2 of one evaluation (a job: network, parameter copy, input);
//   the four waves split hidden-1 in blocks of 32 units.  Per block a wave generates layer 1 TRANSPOSED on the matrix cores (hidden unit
//   in the register, row in the lane) from its lane's share of the input row [x | a | 1] — NQ float4 per lane, up to 16 steps of
//   v_mfma_f32_32x32x2_f32 — relu's it in registers and feeds the 16 layer-2 steps of the block; no GEMM operand passes through LDS.
//   The next block's operands (NQ float4 of [W1 ; b1], four of W2) are requested in front of this block's MFMAs.
// INPUT ROWS  lane (row, h) holds columns 8 q + 4 h .. + 3 in float4 q: whole 16-byte loads of the observation row when obs_dim % 4 == 0
//   (the walker: three per lane) and one for the stored action when act_dim == 4; by element otherwise.  Columns obs .. obs + act - 1
//   are the stored action (phase 0, Q evaluations) or the action phase 1 samples from the policy's head partials in every lane; column
//   D is the constant 1; the slots behind it are 0 and meet zero pads of the block array: the steps in between contract zeros, exactly.
// STEP COUNTS  4 (D1 / 8) + min(D1 % 8, 4) with D1 = D + 1 (wide_steps): 13 for the walker's policy (D1 = 25) and 16 for its Q networks
//   (D1 = 29: columns 24..27 are the four steps of half 0 in the last float4).  The kernel is compiled per float4 count NQ of the launch's
//   widest evaluation (the Q networks'); inside it a job runs the smallest of that NQ's K loops that covers its steps:
//   NQ 1: 4 — NQ 2: 4, 8 — NQ 3: 8, 12 — NQ 4: 13, 16.
// SIDE OUTPUTS, EPILOGUE, HEAD PARTIALS, SUMMATION ORDER  as k_dfwd (the same images in the same layouts for k_dg: H1r4 by h1_owned, the
//   augmented input rows [row / 4][32][4] and the noise by side_aug_tile / side_noise_tile; blocks in order inside a wave, waves 0..3
//   in the combine, then the bias; columns 0..31 in the head dot).  Layer 1 sums its steps 0 .. NS - 1 in order.
// NOT HERE  two row tiles per workgroup, and the stored-action evaluations riding in phase 1: phase 0 runs evaluations 0-4, phase 1
//   evaluations 5-7 (+ the next update's sampler workgroup, as in k_dfwd<1>).
// SAC-v (ddrl_sacv_create_wide; example/model.py:38-50)  the same kernel, the roles k_dfwd has on the narrow SAC-v handle, told by the
//   job table alone (sac1.hip: EV_SACV_DIR).  Tiles per job stay (batch / 32) x (hidden2 / 32), one job per evaluation:
//   phase 0 = 5 jobs: pi(x), q1(x, a), q2(x, a), v(x), v_targ(x2).  Network 3 (V) sits one network stride behind q2 in either parameter
//     copy and is an observation-only job like the policy (d1 = 0: its bias is input column obs_dim), so on the walker the two V jobs
//     and the policy run the 13-step loop of the NQ = 4 kernel beside the 16-step Q jobs.  v(x) leaves the H1r4 / H2c4 / H2r4 images of
//     V's wgrads and the [x | 1] rows (xv_r4) of its layer-1 wgrad; v_targ(x2) leaves head partials only.  The values v / v_targ
//     themselves are summed from the head partials by k_dg's first launch (its SAC-v row prologue), not here.
//   phase 1 = 2 jobs: q1(x, pi), q2(x, pi).  BOTH name evaluation 0 (pi(x), main copy, eps_x) in pev_pack / pin_pack: every workgroup
//     of either job sums that evaluation's head partials for its 32 rows and samples the action in registers — the action reaches both
//     Q networks without passing through memory; the tile of job 0 on column tile 0 also stores act0 / logp0 / save0 (side 1) for
//     the backward launches.  No evaluation at x2 needs the policy (php1 == nullptr: the `two` tile never forms).
//   Splitting 5 + 2 rather than 3 + 4 (the stored-action Q jobs in phase 1, as k_dfwd<1> takes them on the narrow SAC1 handle) keeps
//   phase 1, the launch behind the policy's head partials, at the two evaluations that need them: 160 workgroups at the walker's
//   (400, 300), batch 256 — under one per CU — against 400 in phase 0, which waits for nothing.
//   Every (NQ, steps) pair a SAC-v table produces is compiled: the observation-only jobs need wide_steps(obs + 1) <= the Q jobs'
//   wide_steps(obs + act + 1) <= 4 NQ steps, and each NQ's largest loop is 4 NQ.
#pragma once

// inside a network of the wide layout, relative to its [W1 ; b1] block array (make_layout(..., wide)): the k4-interleaved W2, b2, the head kernel(s)
__host__ __device__ __forceinline__ int wnet_w2_off(int K) { return ((K + 31) & ~31) * 32; }
__host__ __device__ __forceinline__ int wnet_b2_off(int K, int Np) { return ((K + 31) & ~31) * (32 + Np); }
__host__ __device__ __forceinline__ int wnet_wh0_off(int K, int Np) { return wnet_b2_off(K, Np) + Np; }
__host__ __device__ __forceinline__ int wpi_bmu_off(int K, int Np, int h2, int act) { return wnet_wh0_off(K, Np) + h2 * act; }
__host__ __device__ __forceinline__ int wpi_wls_off(int K, int Np, int h2, int act) { return (wpi_bmu_off(K, Np, h2, act) + act + 3) & ~3; }
__host__ __device__ __forceinline__ int wpi_bls_off(int K, int Np, int h2, int act) { return wpi_wls_off(K, Np, h2, act) + h2 * act; }

struct WOps {
    float4 bq[4][4];
    float w1[4][16];
};
// one block's operands: NQ float4 of [W1 ; b1], then its four W2 groups (issue order = order of need); blocks beyond nb re-read the last
template <int NQ>
__device__ __forceinline__ void wops_load_block(WOps &o, const DSrc &s, int bi, int lane) {
    const int l31 = lane & 31, h = lane >> 5;
    const int blk = s.b0 + (bi < s.nb ? bi : (s.nb > 0 ? s.nb - 1 : 0));
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(s.W1 + ((((long long)blk * 4 + q) * 2 + h) * 32 + l31) * 4);
        o.w1[bi][4 * q + 0] = v.x; o.w1[bi][4 * q + 1] = v.y; o.w1[bi][4 * q + 2] = v.z; o.w1[bi][4 * q + 3] = v.w;
    }
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) o.bq[bi][rq] = *reinterpret_cast<const float4 *>(s.W2p + ((long long)(blk * 8 + 2 * rq + h) * s.Np + s.n0 + l31) * 4);
}

// K loop of one wave: per block layer 1 (NS steps) -> relu -> 4 * nrq layer-2 steps; bit bi of h1own: X1 of block bi also goes to memory
// as [row / 4][unit][4] through the wave's LDS tile (dkloop's transpose)
template <int NS, int NQ, class Mid>
__device__ __forceinline__ void wkloop(WOps &o, const DSrc &src, int K, int lane, const float (&xin)[4 * NQ], floatx16 &acc,
                                       float *__restrict__ h1r4, int h1own, int Lp1, int m0, float *__restrict__ tr, Mid &&mid) {
    static_assert(NS <= 4 * NQ, "the steps of a K loop lie inside the float4s the kernel loads");
    const int l31 = lane & 31, h = lane >> 5, b0 = src.b0, nb = src.nb;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
        if (bi + 1 < 4) {
            wops_load_block<NQ>(o, src, bi + 1, lane);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (bi < nb) {
            const int u0 = (b0 + bi) * 32;
            const int nrq = (K - u0 >= 32) ? 4 : ((K - u0 + 7) >> 3);
            floatx16 x1;
#pragma unroll
            for (int r = 0; r < 16; ++r) x1[r] = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) x1 = __builtin_amdgcn_mfma_f32_32x32x2f32(o.w1[bi][s], xin[s], x1, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) x1[r] = relu1(x1[r]);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                if (rq < nrq) {  // wave-uniform
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[4 * rq + 0], o.bq[bi][rq].x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[4 * rq + 1], o.bq[bi][rq].y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[4 * rq + 2], o.bq[bi][rq].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[4 * rq + 3], o.bq[bi][rq].w, acc, 0, 0, 0);
                }
            }
            if ((h1own >> bi) & 1) {  // wave-uniform
#pragma unroll
                for (int r = 0; r < 16; ++r) tr[((r & 3) + 8 * (r >> 2) + 4 * h) * 36 + l31] = x1[r];
                wave_lds_sync();
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int rg = h + 2 * p;
                    const float4 v = *reinterpret_cast<const float4 *>(tr + l31 * 36 + 4 * rg);
                    if (u0 + l31 < K) st_img(h1r4 + ((long long)(m0 / 4 + rg) * Lp1 + u0 + l31) * 4, v);
                }
                wave_lds_sync();
            }
        }
        if (bi == 0) {  // the epilogue operands: requested behind block 0's MFMAs
            mid();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// (the scalar arguments are k_dfwd's: launch_dfwd_wide packs them the same way)
template <int PH, int NQ>
__global__ void __launch_bounds__(256) k_dfwd_wide(const float *base, int tpj_tm, int K_Np, int B_d0, int pack, int x_off, int main_off, int targ_off, int npi,
                                                   int perq, int hp_off, DFArgs a) {
    __shared__ __attribute__((aligned(16))) float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float tr[4][32 * 36];
    __shared__ float s_wh[DFH][32];
    const int tpj = tpj_tm & 0xffff, tiles_m = (tpj_tm >> 16) & 0xfff, njobs = (unsigned)tpj_tm >> 28;
    const int K = K_Np & 0xfff, Np = (K_Np >> 12) & 0xfff, h2 = Np - ((K_Np >> 24) & 31);
    const int B = B_d0 & 0xffff, d0 = (B_d0 >> 16) & 0xff, act = B_d0 >> 24;
    if (PH == 1 && (int)blockIdx.x == njobs * tpj) {  // only launched when a.do_sample: the next update's batch into the other input set
        ddrl_replay_dev::sample_block(a.rs, a.ring, a.sout, a.sample_batch, nullptr, 1);
        return;
    }
    int t;
    {   // XCD-aware, panel-major tile order (k_dfwd's: speed only)
        const int nwg = njobs * tpj, b = blockIdx.x, q = nwg >> 3, r = nwg & 7, x = b & 7;
        t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
    }
    const int ji = (t >= tpj) + (t >= 2 * tpj) + (t >= 3 * tpj) + (t >= 4 * tpj);
    t -= ji * tpj;
    const int nt = t / tiles_m, m0 = (t - nt * tiles_m) * 32, n0 = nt * 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int jp = (pack >> (6 * ji)) & 63;   // [2] input is obs2, [3] target copy, [5:4] network (the step field [1:0] is the narrow kernel's)
    const int net = (jp >> 4) & 3;
    const int d1 = PH == 1 ? act : ((net == 1 || net == 2) ? act : 0);
    const int D = d0 + d1;
    const int ns = 4 * ((D + 1) >> 3) + ((((D + 1) & 7) < 4) ? ((D + 1) & 7) : 4);   // wide_steps(D + 1)
    const int w1o = ((jp & 8) ? targ_off : main_off) + (net == 0 ? 0 : npi + (net - 1) * perq);
    const int x2_off = x_off + ((B * d0 + 63) & ~63), a_off = x2_off + ((B * d0 + 63) & ~63);
    const float *W1 = base + w1o, *W2p = W1 + wnet_w2_off(K);
    const bool first_n = nt == 0;
    const int nblk = (K + 31) >> 5, bs = nblk >> 2, rem = nblk & 3;
    const int nb = bs + (w >= 4 - rem ? 1 : 0);
    const int b0 = w * bs + (w > 4 - rem ? w - (4 - rem) : 0);

    // ---- phase 1, first: what its longest chain starts with — the policy-head partials of this tile's rows, the head biases of that
    // evaluation's parameter copy and its noise rows (k_dfwd<1>'s first load wave)
    const bool two = PH == 1 && ji == 1 && first_n && a.php1 != nullptr;  // block-uniform: pi_main @ x2 rides here (log-prob only)
    float4 hv[2][4][DNT / 4];
    float pbm[2][4], pbl[2][4], pep[2][4];
    const int pin = PH == 1 ? (a.pin_pack >> (3 * ji)) & 7 : 0;
    if (PH == 1) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pep[e][c] = 0.f;
#pragma unroll
                for (int q = 0; q < DNT / 4; ++q) hv[e][c][q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        const int bmu_o = wpi_bmu_off(K, Np, h2, act), bls_o = wpi_bls_off(K, Np, h2, act);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float *pb = base + ((e == 0 && (pin & 4)) ? targ_off : main_off);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int cc = c < d1 ? c : 0;
                pbm[e][c] = pb[bmu_o + cc];
                pbl[e][c] = pb[bls_o + cc];
            }
        }
        const long long HPq = (long long)DFH * B * DNT;
        const int eps_ld = (B * act + 63) & ~63, eps_off = a_off + eps_ld + 2 * ((B + 63) & ~63);  // items 5..7 of the input set
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 0 || two) {  // block-uniform
                const float *hp = base + hp_off + (e == 0 ? ((a.pev_pack >> (2 * ji)) & 3) : 1) * HPq;
                const float4 *p0 = reinterpret_cast<const float4 *>(hp + ((long long)(h * d1) * B + m0 + l31) * DNT);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int q = 0; q < DNT / 4; ++q) hv[e][c][q] = p0[(long long)(c < d1 ? c : 0) * B * (DNT / 4) + q];
                const float *ep = base + eps_off + (e == 0 ? (pin & 3) : 1) * eps_ld + (long long)(m0 + l31) * d1;
#pragma unroll
                for (int c = 0; c < 4; ++c) pep[e][c] = ep[c < d1 ? c : 0];
            }
        }
    }
    // ---- this lane's share of its input row: the observation float4s, then the stored action (phase 0, Q evaluations)
    float xin[4 * NQ];
    float av[4] = {0.f, 0.f, 0.f, 0.f};
    {
        const float *in0 = base + ((jp & 4) ? x2_off : x_off), *in1 = base + a_off;
        const long long row = m0 + l31;
        const float *xr = in0 + row * d0;
        const bool vec = (d0 & 3) == 0;   // launch-uniform: rows of whole float4s on a 16-byte grid (the input items are 256-byte aligned)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c0 = 8 * q + 4 * h;
            float v[4];
            if (vec) {   // c0 and d0 are multiples of 4: c0 < d0 <=> the whole float4 lies inside the row
                const float4 t4 = *reinterpret_cast<const float4 *>(xr + (c0 < d0 ? c0 : 0));
                v[0] = t4.x; v[1] = t4.y; v[2] = t4.z; v[3] = t4.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = xr[c0 + e < d0 ? c0 + e : 0];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) xin[4 * q + e] = c0 + e < d0 ? v[e] : (c0 + e == D ? 1.0f : 0.f);   // column D: the bias row
        }
        if (PH == 0 && d1 > 0) {   // block-uniform
            if (d1 == 4) {
                const float4 t4 = *reinterpret_cast<const float4 *>(in1 + row * 4);
                av[0] = t4.x; av[1] = t4.y; av[2] = t4.z; av[3] = t4.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) av[c] = in1[row * d1 + (c < d1 ? c : 0)];
            }
        }
    }
    WOps ops;
    const DSrc src{W1, W2p, Np, b0, nb, n0};
    wops_load_block<NQ>(ops, src, 0, lane);
    const DFJob &jb = a.job[ji];
    ktouch(kline<sizeof(DFJob)>(&jb) | kline<offsetof(DFArgs, do_sample)>(&a));
    // the epilogue operands (the bias group of this thread's four columns, its element of the head kernels): addresses from the scalars
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float whv = 0.f;
    const bool pinet = net == 0;
    const int nh = pinet ? 2 * act : 1, hsplit = pinet ? act : 1;
    const float *b2p = W1 + wnet_b2_off(K, Np) + n0 + 4 * (tid >> 5);
    const int wh0o = wnet_wh0_off(K, Np), wh1o = pinet ? wpi_wls_off(K, Np, h2, act) : wh0o;
    const int hc = tid >> 5, hcol = n0 + (tid & 31);
    const bool whok = hc < nh && hcol < h2;
    const int who = (hc < hsplit ? wh0o : wh1o) + (whok ? hcol * hsplit + (hc < hsplit ? hc : hc - hsplit) : 0);
    auto epilogue_operands = [&]() {
        b4 = *reinterpret_cast<const float4 *>(b2p);
        whv = W1[who];
    };
    if (PH == 1) {  // the sampled action of this tile's rows, in every lane of every wave (no LDS, no barrier)
        float hs[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // n-tile order; unused slots are 0
                float s = zero_here();
#pragma unroll
                for (int q = 0; q < DNT / 4; ++q) { s += hv[e][c][q].x; s += hv[e][c][q].y; s += hv[e][c][q].z; s += hv[e][c][q].w; }
                hs[e][c] = s;
            }
        float mu[4], ls[4], ev[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float o = __shfl_xor(hs[0][c], 32);
            mu[c] = (h ? o : hs[0][c]) + pbm[0][c];
            ls[c] = (h ? hs[0][c] : o) + pbl[0][c];
            ev[c] = pep[0][c];
        }
        const PolRow o = policy_row(mu, ls, ev, d1, a.scale);
#pragma unroll
        for (int c = 0; c < 4; ++c) av[c] = o.act[c];
        if (first_n && w == 0 && lane < 32) {
            const int row = m0 + l31;
            if (jb.side == 1) {
                a.logp0[row] = o.logp;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < d1) {
                        a.act0[row * d1 + c] = o.act[c];
                        *reinterpret_cast<float4 *>(a.save0 + ((long long)row * d1 + c) * 4) = make_float4(o.a[c], o.std[c], o.t[c], ev[c]);
                    }
            } else if (jb.side == 2) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < d1) a.act2[row * d1 + c] = o.act[c];
            }
        }
        if (two && w == 1) {  // wave-uniform
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float o2 = __shfl_xor(hs[1][c], 32);
                mu[c] = (h ? o2 : hs[1][c]) + pbm[1][c];
                ls[c] = (h ? hs[1][c] : o2) + pbl[1][c];
                ev[c] = pep[1][c];
            }
            const PolRow o1 = policy_row(mu, ls, ev, d1, a.scale);
            if (lane < 32) a.logp1[m0 + l31] = o1.logp;
        }
    }
    // the action columns obs .. obs + act - 1 of the layer-1 input (they may straddle a float4 and the two lane halves)
    if (d1 > 0) {
#pragma unroll
        for (int s = 0; s < 4 * NQ; ++s) {
            const int c = 8 * (s >> 2) + 4 * h + (s & 3) - d0;
            if (c >= 0 && c < d1) xin[s] = c == 0 ? av[0] : (c == 1 ? av[1] : (c == 2 ? av[2] : av[3]));
        }
    }
    // ---- K loop
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float *h1r4 = jb.H1r4;
    const int h1own = h1r4 ? h1_owned(b0, nb, nt, a.tiles_n) : 0;
    if (NQ == 1) wkloop<4, NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
    else if (NQ == 2) {
        if (ns <= 4) wkloop<4, NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
        else wkloop<(NQ == 2 ? 8 : 4), NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
    } else if (NQ == 3) {
        if (ns <= 8) wkloop<(NQ == 3 ? 8 : 4), NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
        else wkloop<(NQ == 3 ? 12 : 4), NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
    } else {
        if (ns <= 13) wkloop<(NQ == 4 ? 13 : 4), NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
        else wkloop<(NQ == 4 ? 16 : 4), NQ>(ops, src, K, lane, xin, acc, h1r4, h1own, a.Lp1, m0, tr[w], epilogue_operands);
    }

    // ---- the other side outputs of the row tile, one column tile each (k_dfwd's rules)
    if (nt == side_aug_tile(a.tiles_n) && (jb.aug || jb.xr4)) {  // augmented input rows of the layer-1 wgrads (their ones column is set once at create)
        for (int idx = tid; idx < 32 * D; idx += 256) {
            const int r = idx / D, d = idx - r * D;
            const long long row = m0 + r;
            const float v = d < d0 ? (base + ((jp & 4) ? x2_off : x_off))[row * d0 + d] : (base + a_off)[row * d1 + (d - d0)];
            if (jb.aug) jb.aug[row * jb.aug_ld + d] = v;
            if (jb.xr4) jb.xr4[((row >> 2) * 32 + d) * 4 + (row & 3)] = v;
        }
    }
    if (PH == 0 && a.noise_on && ji == 0 && nt == side_noise_tile(a.tiles_n)) {
        // eps_x, eps_x2, eps_t of this tile's rows; element index as in one flat [3][B*act] fill
        const unsigned long long nbase = a.opt->noise_ctr;
        const int per_row = 3 * act;
        for (int e = tid; e < 32 * per_row; e += 256) {
            const int rr = e / per_row, q = e - rr * per_row;
            const int wch = q / act, c = q - wch * act;
            const int k = (m0 + rr) * act + c;
            if (m0 + rr < a.Bv) (wch == 0 ? a.e0 : (wch == 1 ? a.e1 : a.e2))[k] = normal_at(a.noise_seed, nbase + (unsigned long long)wch * a.n_each + k);
        }
    }

    // ---- split-K combine, bias + relu, H2 in the layouts its consumers read, head partials
    const int r = tid & 31, cg = tid >> 5;
#pragma unroll
    for (int q = 0; q < 16; ++q) red[w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
    __syncthreads();
    s_wh[tid >> 5][tid & 31] = whok ? whv : 0.f;   // read behind two more barriers
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * cg + e;
        const float s = ((red[0][r][c] + red[1][r][c]) + red[2][r][c]) + red[3][r][c];
        v[e] = fmaxf(s + f4e(b4, e), 0.f);
    }
    if (jb.H2c4) st_img(jb.H2c4 + ((long long)(n0 / 4 + cg) * B + m0 + r) * 4, make_float4(v[0], v[1], v[2], v[3]));
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) red[0][r][4 * cg + e] = v[e];
    __syncthreads();
    if (jb.H2r4) {  // (column hidden2 of the image is the ones column: never written here)
        const int c = tid & 31, rg = tid >> 5;
        if (n0 + c < a.h2)
            st_img(jb.H2r4 + ((long long)(m0 / 4 + rg) * a.Lp2 + n0 + c) * 4,
                   make_float4(red[0][4 * rg][c], red[0][4 * rg + 1][c], red[0][4 * rg + 2][c], red[0][4 * rg + 3][c]));
    }
    {
        const int c = tid >> 5;
        if (c < nh) {
            float s = 0.f;
#pragma unroll
            for (int col = 0; col < 32; ++col) s = fmaf(red[0][r][col], s_wh[c][col], s);
            jb.hp[((long long)c * B + m0 + r) * DNT + nt] = s;
        }
    }
}

// Phase PH of a wide learner's forward: k_dfwd_wide by the float4 count of the widest evaluation's contraction (d1max = obs + act + 1 columns)
template <int PH>
static void launch_dfwd_wide(const DFHead &d, const DFArgs &F, hipStream_t s) {
    const int tiles_m = d.B / 32, tpj = tiles_m * F.tiles_n;
    const int grid = F.njobs * tpj + ((PH == 1 && F.do_sample) ? 1 : 0);
    const int a1 = tpj | (tiles_m << 16) | (F.njobs << 28), a2 = d.K | (d.Np << 12) | ((d.Np - F.h2) << 24), a3 = d.B | (d.d0 << 16) | (F.act << 24);
    const int nq = (wide_steps(d.d0 + F.act + 1) + 3) / 4;
    auto go = [&](auto kern) { kern<<<grid, 256, 0, s>>>(d.base, a1, a2, a3, d.pack, d.x_off, d.main_off, d.targ_off, d.npi, d.perq, d.hp_off, F); };
    if (nq <= 1) go(k_dfwd_wide<PH, 1>);
    else if (nq == 2) go(k_dfwd_wide<PH, 2>);
    else if (nq == 3) go(k_dfwd_wide<PH, 3>);
    else go(k_dfwd_wide<PH, 4>);
}
