// k_actor_fwd_wide: the rollout's policy forward for observation rows of up to 31 columns (the bipedal walker: 24 observations, 4
// actions) — k_actor_fwd's job and contract (sac1_direct.h) with a layer-1 contraction over D1 = obs_dim + 1 <= 32 input columns, and
// the layer-1 block layout that contraction reads (its index function and pack / unpack kernel: wide_pack.h).  Included by actor.hip inside its unnamed
// namespace, behind sac1_direct.h (ActFwdArgs, ANT, DFH, DNT, relu1, VerTile / VerState) and sac1_layout.h (Seg, Layout).
//
// LAYOUT  [W1 ; b1] as 32 floats per hidden unit.  Input column d (d = obs_dim: the bias) sits in MFMA step s = 4 (d / 8) + d % 4 of
//   lane half h = (d / 4) % 2, i.e. float4 q = d / 8 of half h holds columns 8 q + 4 h .. + 3.  Per block of 32 hidden units four
//   float4 per lane half; within a (block, float4, half) the 32 units are contiguous: one coalesced 512-byte segment per half-wave
//   load, like the narrow layout's (gemm_core.h, w1y_index).  Unused slots are zero and stay zero.
//   The same map read from the input side: lane (row, h) needs columns 8 q + 4 h .. + 3 of its observation row for float4 q — whole
//   16-byte loads when obs_dim % 4 == 0 (the walker's 96-byte rows: three per lane, and the bias "1.0" in the first slot of half 0's
//   fourth float4); any other obs_dim loads by element.  Steps a shape needs: 4 (D1 / 8) + min(D1 % 8, 4) — 13 for the walker, 16 at
//   most; NS is the smallest instantiated count that covers it (4, 8, 12, 13, 16), the steps in between contract zeros: exact.
//
// WORK SPLIT  as k_actor_fwd: one workgroup = one 32-row tile x up to ANT consecutive column tiles of layer 2; wave w computes layer 1
//   for ITS quarter of the hidden-1 blocks once (v_mfma_f32_32x32x2_f32, transposed: hidden units along M, rows along N) and keeps the
//   relu'd result in registers as the A operand of every column tile; the W2 groups of tile t + 1 are requested between the MFMAs of
//   the same groups of tile t; split-K combine, bias + relu and the head dot go through LDS; head partials to hp[(c rows + row) DNT + tile].
//   OCC and VER mean what they mean there (1 / 2 workgroups per CU; version table, row lists, per-slot weight offset).
//
// REGISTERS  the layer-1 operands (up to 64 of W1, 16 of input) are dead before tile 0's W2 groups are requested: the peak is the
//   column-tile loop's (64 of layer 1 + the W2 buffers + the accumulator), as in the narrow kernel (profiles/actor_wide_resource_usage.txt).
//
// SUMMATION ORDER (the kernel's own; results are held to the float64 oracle, not to k_actor_fwd)  layer 1: steps 0 .. NS - 1 in order
//   inside a block, i.e. per step the two columns of halves 0 and 1; layer 2: this wave's blocks in order, 8-unit groups in order inside
//   a block; waves 0..3 in the combine, then the bias; columns 0..31 in the head dot (fma chain); k_actor_finish adds the tiles in order.
#pragma once

#include "wide_pack.h"   // the layout's index function, its pack kernel, wide_steps, DDRL_WIDE_KERNEL
// __syncthreads() with the kernels' own target attribute (a function of another feature set is called, not inlined)
__device__ __forceinline__ DDRL_WIDE_KERNEL void wide_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int NS, int OCC, bool VER = false>
__global__ void DDRL_WIDE_KERNEL __launch_bounds__(256, OCC) k_actor_fwd_wide(ActFwdArgs a) {
    constexpr int NQ = (NS + 3) / 4;   // float4 per lane of the input row and of every layer-1 block
    // rows of 36 floats: 16-byte aligned (b128 LDS reads) and conflict-free for 16 lanes reading 4 words each
    __shared__ __attribute__((aligned(16))) float red[2][4][32][36];
    __shared__ __attribute__((aligned(16))) float red2[2][32][36];
    __shared__ __attribute__((aligned(16))) float s_wh[ANT][DFH][32];
    __shared__ __attribute__((aligned(16))) float s_b2[ANT][32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    int m0, ntiles, nt0;
    int vcount = 32, vrow = 0;
    if (!VER) {   // column tiles dealt to `ngroups` workgroups per row tile as evenly as they go
        const int ngroups = a.ngroups;
        const int rt = blockIdx.x / ngroups, grp = blockIdx.x - rt * ngroups;
        const int gbase = a.tiles_n / ngroups, gextra = a.tiles_n % ngroups;
        ntiles = gbase + (grp < gextra ? 1 : 0);
        nt0 = grp * gbase + (grp < gextra ? grp : gextra);
        m0 = rt * 32;
    } else {      // the planning launch's table: one record per workgroup, the tile's envs in its row list
        const int n_wgs = a.vs->n_wgs;
        const VerTile vt = a.vtiles[(int)blockIdx.x < a.vt_max ? blockIdx.x : 0];
        if ((int)blockIdx.x >= n_wgs) return;   // the launch covers the worst case; block-uniform
        vrow = a.perm[vt.base + l31];
        const long long off = (long long)vt.slot * a.vstride;
        a.W1 += off; a.W2p += off; a.b2 += off; a.wmu += off; a.wls += off;
        m0 = vt.base; vcount = vt.count; nt0 = vt.cols & 255; ntiles = vt.cols >> 8;
        // rows beyond the count repeat the tile's last env (__shfl's own instruction: the library function is of another feature set)
        vrow = __builtin_amdgcn_ds_bpermute(((lane & 32) + (l31 < vcount ? l31 : vcount - 1)) << 2, vrow);
    }
    const int K = a.K, Np = a.Np, d0 = a.d0;
    const int nblk = (K + 31) >> 5, bs = nblk >> 2, rem = nblk & 3;
    const int nb = bs + (w >= 4 - rem ? 1 : 0);
    const int b0 = w * bs + (w > 4 - rem ? w - (4 - rem) : 0);
    // ---- loads in the order of need: this lane's share of its input row, the layer-1 columns of this wave's blocks
    float xin[4 * NQ];
    {
        long long row = m0 + l31 < a.rows ? m0 + l31 : a.rows - 1;
        if (VER) row = vrow;
        const float *xr = a.obs + row * d0;
        const bool vec = (d0 & 3) == 0;   // launch-uniform: rows of whole float4s on a 16-byte grid
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int base = 8 * q + 4 * h;
            float v[4];
            if (vec) {   // base and d0 are multiples of 4: base < d0 <=> the whole float4 lies inside the row
                const float4 t = *reinterpret_cast<const float4 *>(xr + (base < d0 ? base : 0));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = xr[base + e < d0 ? base + e : 0];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) xin[4 * q + e] = base + e < d0 ? v[e] : (base + e == d0 ? 1.0f : 0.f);   // column d0: the bias row
        }
    }
    float w1[4][4 * NQ];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
        const int blk = b0 + (bi < nb ? bi : (nb > 0 ? nb - 1 : 0));
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(a.W1 + ((((long long)blk * 4 + q) * 2 + h) * 32 + l31) * 4);
            w1[bi][4 * q + 0] = v.x; w1[bi][4 * q + 1] = v.y; w1[bi][4 * q + 2] = v.z; w1[bi][4 * q + 3] = v.w;
        }
    }
    // OCC = 1: the W2 groups double-buffered by tile parity.  OCC = 2 (256 registers): one set, the group of tile t + 1 requested into the
    // registers of the same group of tile t right behind the MFMAs that consumed it (k_actor_fwd's plan)
    constexpr int NBUF = OCC == 2 ? 1 : 2;
    float4 bq[NBUF][4][4];
    const int lane_off = (h * Np + l31) * 4;
    auto fetch_group = [&](int buf, int t, int bi, int rq) DDRL_WIDE_KERNEL {  // one W2 group (8 hidden-1 units x 32 columns) of column tile t
        const int nt = nt0 + t < a.tiles_n ? nt0 + t : a.tiles_n - 1;
        const int u0 = (b0 + (bi < nb ? bi : (nb > 0 ? nb - 1 : 0))) * 32;
        const float *gp = a.W2p + ((long long)(u0 / 4 + 2 * rq) * Np + nt * 32) * 4;
        bq[buf][bi][rq] = *reinterpret_cast<const float4 *>(gp + lane_off);
    };
    // head kernels and biases of this workgroup's column tiles: requested now, staged into LDS behind tile 0's MFMAs
    float whv[(ANT * DFH * 32 + 255) / 256], b2v = 0.f;
#pragma unroll
    for (int i = 0; i < (ANT * DFH * 32 + 255) / 256; ++i) {
        const int e = tid + 256 * i;
        const int t = e / (DFH * 32), c = (e / 32) % DFH, col = (nt0 + t) * 32 + (e & 31);
        const bool ok = e < ANT * DFH * 32 && c < 2 * a.act && col < a.h2 && t < ntiles;
        const float *p = c < a.act ? a.wmu : a.wls;
        const float v = p[ok ? (long long)col * a.act + (c < a.act ? c : c - a.act) : 0];
        whv[i] = ok ? v : 0.f;
    }
    {
        const int t = tid >> 5, col = (nt0 + t) * 32 + (tid & 31);
        const bool ok = tid < ANT * 32 && col < Np && t < ntiles;
        const float v = a.b2[ok ? col : 0];  // (pads of b2 are zero)
        b2v = ok ? v : 0.f;
    }
    // ---- layer 1 of this wave's blocks, once: x1[bi][q] = relu(H1^T) of unit (q & 3) + 8 (q >> 2) + 4 h of the block, row l31
    floatx16 x1[4];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) x1[bi][r] = 0.f;
        if (bi < nb) {  // wave-uniform
#pragma unroll
            for (int s = 0; s < NS; ++s) x1[bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[bi][s], xin[s], x1[bi], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) x1[bi][r] = relu1(x1[bi][r]);
        }
    }
    // tile 0's W2 groups: requested behind the layer-1 MFMAs, into registers the layer-1 operands have left
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) fetch_group(0, 0, bi, rq);
    auto stage_heads = [&]() DDRL_WIDE_KERNEL {
#pragma unroll
        for (int i = 0; i < (ANT * DFH * 32 + 255) / 256; ++i) {
            const int e = tid + 256 * i;
            if (e < ANT * DFH * 32) (&s_wh[0][0][0])[e] = whv[i];
        }
        if (tid < ANT * 32) (&s_b2[0][0])[tid] = b2v;
    };
    // ---- the column tiles
    const int r = tid & 31, cg = tid >> 5;
#pragma unroll
    for (int t = 0; t < ANT; ++t) {
        if (t < ntiles) {  // block-uniform
            floatx16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                if (bi < nb) {
                    const int u0 = (b0 + bi) * 32;
                    const int nrq = (K - u0 >= 32) ? 4 : ((K - u0 + 7) >> 3);
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        if (rq < nrq) {
                            const float4 b = bq[t & (NBUF - 1)][bi][rq];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[bi][4 * rq + 0], b.x, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[bi][4 * rq + 1], b.y, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[bi][4 * rq + 2], b.z, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[bi][4 * rq + 3], b.w, acc, 0, 0, 0);
                        }
                        if (t + 1 < ANT) {  // the same group of the next column tile, requested between this group's MFMAs and the next's
                            __builtin_amdgcn_sched_barrier(0);
                            fetch_group((t + 1) & (NBUF - 1), t + 1, bi, rq);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                } else if (t + 1 < ANT) {
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) fetch_group((t + 1) & (NBUF - 1), t + 1, bi, rq);
                }
            }
            if (t == 0) stage_heads();  // requested behind tile 0's MFMAs, stored before the first barrier
            // split-K combine, bias + relu, head partials (LDS tiles double-buffered by tile parity: two barriers per tile)
#pragma unroll
            for (int q = 0; q < 16; ++q) red[t & 1][w][(q & 3) + 8 * (q >> 2) + 4 * h][l31] = acc[q];
            wide_barrier();
            {
                const float4 p0 = *reinterpret_cast<const float4 *>(&red[t & 1][0][r][4 * cg]), p1 = *reinterpret_cast<const float4 *>(&red[t & 1][1][r][4 * cg]);
                const float4 p2 = *reinterpret_cast<const float4 *>(&red[t & 1][2][r][4 * cg]), p3 = *reinterpret_cast<const float4 *>(&red[t & 1][3][r][4 * cg]);
                const float4 bb = *reinterpret_cast<const float4 *>(&s_b2[t][4 * cg]);
                float4 v;
                v.x = fmaxf((((p0.x + p1.x) + p2.x) + p3.x) + bb.x, 0.f);
                v.y = fmaxf((((p0.y + p1.y) + p2.y) + p3.y) + bb.y, 0.f);
                v.z = fmaxf((((p0.z + p1.z) + p2.z) + p3.z) + bb.z, 0.f);
                v.w = fmaxf((((p0.w + p1.w) + p2.w) + p3.w) + bb.w, 0.f);
                *reinterpret_cast<float4 *>(&red2[t & 1][r][4 * cg]) = v;
            }
            wide_barrier();
            if (cg < 2 * a.act) {
                float sum = 0.f;
#pragma unroll
                for (int c4 = 0; c4 < 8; ++c4) {
                    const float4 x = *reinterpret_cast<const float4 *>(&red2[t & 1][r][4 * c4]), y = *reinterpret_cast<const float4 *>(&s_wh[t][cg][4 * c4]);
                    sum = fmaf(x.x, y.x, sum); sum = fmaf(x.y, y.y, sum); sum = fmaf(x.z, y.z, sum); sum = fmaf(x.w, y.w, sum);
                }
                if (VER) {
                    if (r < vcount) a.hp[((long long)cg * a.rows + a.perm[m0 + r]) * DNT + nt0 + t] = sum;
                } else if (m0 + r < a.rows) a.hp[((long long)cg * a.rows + m0 + r) * DNT + nt0 + t] = sum;
            }
        }
    }
}

// k_actor_fwd_wide by the step count the shape needs (wide_steps): one instantiation per float4 count, and the walker's 13
template <int OCC, bool VERSIONED>
static void launch_actor_fwd_wide(int ns, unsigned grid, hipStream_t s, const ActFwdArgs &A) {
    if (ns <= 4) k_actor_fwd_wide<4, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else if (ns <= 8) k_actor_fwd_wide<8, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else if (ns <= 12) k_actor_fwd_wide<12, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else if (ns == 13) k_actor_fwd_wide<13, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else k_actor_fwd_wide<16, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
}
