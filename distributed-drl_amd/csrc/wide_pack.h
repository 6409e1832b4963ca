// The wide layer-1 block layout (32 floats per hidden unit, Seg mode 3) and what every holder of it shares: the index function, the
// pack / unpack kernel of its segment tables and the MFMA step count of a contraction over d1 columns.  Included by actor_wide.h (the
// actor's policy, actor.hip) and by sac1_wide.h (the learner's policy and twin Q, sac1_wide.hip), inside their unnamed namespaces, behind
// gemm_core.h (Seg) and policy_row.h (VerState).  The layout itself is described at the top of actor_wide.h.
#pragma once

// These kernels are compiled without the packed float32 VALU forms (v_pk_add / _mul / _fma_f32): single-lane operations, the
// same IEEE results; the rest of the translation unit keeps the flags it was measured with.
#if defined(__HIP_DEVICE_COMPILE__)
#define DDRL_WIDE_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define DDRL_WIDE_KERNEL
#endif
// input column d of hidden unit j in the wide layer-1 block array
__host__ __device__ __forceinline__ long long w1wide_index(int d, int j) {
    return ((((long long)(j >> 5) * 4 + (d >> 3)) * 2 + ((d >> 2) & 1)) * 32 + (j & 31)) * 4 + (d & 3);
}
constexpr int SEG_W1WIDE = 3;   // Seg.mode of a wide handle's layer-1 tensors (gemm_core.h names 1 and 2; k_pack never sees this one)

// A wide handle's k_pack.  DIR 0: wide layout -> dense flat vector;  DIR 1: flat -> wide layout;  DIR 2: flat -> the current copy AND
// the version slot k_version_plan picked (k_pack_version's form; the slots' pads stay as allocated: zero).
template <int DIR>
__global__ void DDRL_WIDE_KERNEL __launch_bounds__(256) k_pack_wide(const Seg *__restrict__ segs, const float *__restrict__ src, float *__restrict__ dst,
                                                   float *__restrict__ vslab, long long vstride, const VerState *__restrict__ vs) {
    const Seg s = segs[blockIdx.y];
    float *dst2 = DIR == 2 ? vslab + (long long)vs->target * vstride : nullptr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += (long long)gridDim.x * 256) {
        long long ii = i;
        if (s.cols > 0) {
            const long long k = i / s.cols, j = i - k * s.cols;
            ii = s.mode == SEG_W1WIDE ? w1wide_index(s.d0 + (int)k, (int)j) : ((k >> 2) * s.ld + j) * 4 + (k & 3);
        }
        if (DIR == 0) {
            dst[s.ext + i] = src[s.in + ii];
        } else {
            const float v = src[s.ext + i];
            dst[s.in + ii] = v;
            if (DIR == 2) dst2[s.in + ii] = v;
        }
    }
}

// MFMA steps of the layer-1 contraction over d1 = obs_dim + 1 columns in the layout above
static int wide_steps(int d1) { return 4 * (d1 >> 3) + ((d1 & 7) < 4 ? (d1 & 7) : 4); }
