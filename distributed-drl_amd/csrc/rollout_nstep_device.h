// The env-agnostic phases of the fused n-step rollout step, shared by its two kernels: k_env_step_nstep (rollout_nstep.hip, the
// one-body lander) and k_env3_step_nstep (rollout3_nstep.hip, the articulated lander).  The phases are lettered as in
// rollout_nstep.hip's header comment; a (the policy head) and b / e (Wrapper.step and the episode end on the env's own model) are the
// kernels' own, everything here is ONE piece of code for both:
//   DDRL_NSTEP_READY_ROWS  the readiness ranking: base rank and total from the readiness bytes, the ring row of every ready env
//   nstep_queue_tick       c. t_queue and the NEXT step's readiness byte
//   DDRL_NSTEP_MIRRORS     f. the next observation into the forward's buffer, and the mirrors
//   nstep_windows          c. + d. the four window arrays: slide, append, store the ready rows, start the ended envs' queues anew
//   DDRL_NSTEP_FINISH      the episode statistics, the next forward's plan and the ring ticket
// Internal linkage throughout, as env_device.h: each translation unit compiles its own copy, and k_env_step_nstep compiles to the code
// it compiled to with these statements in its own body.
#pragma once
#include "ddrl_common.h"
#include "replay_device.h"
#include "env_device.h"
#include "version_plan.h"
#include "rollout_nstep.h"

namespace {

// LDS at Ln = DDRL_NSTEP_FUSED_MAX_LN: 64 envs x (Ln + 1) x 8 floats = 34 KiB, + ver_plan_tail's 22.5 KiB (+ the argument struct
// k_env3_step_nstep parks, under half a KiB): inside a workgroup's 64 KiB
static_assert(64 * (DDRL_NSTEP_FUSED_MAX_LN + 1) * 8 * 4 + 24 * 1024 <= 64 * 1024, "the staged observation windows must fit the LDS");

struct NStepTicket {
    ddrl_replay_dev::RingState *rs;
    ddrl_replay_dev::RingPtrs ring;
    long long ptr, total;
    __device__ bool operator()() const { return ddrl_replay_dev::ring_commit(rs, ring, ptr, total); }
};

// One queue array of the workgroup's `ne` envs, W vectors per env, sliding by S vectors: q = the block's rows in the queue array,
// ring = the ring array, s_row[e] = ring row of env e or -1.  tail = the appended entry, tail2 = what k_winq_begin puts in its place
// where the episode ended (PATCH arrays only: the observation window).  Every lane of the wave calls it.
template <class V, int S, bool PATCH>
__device__ __forceinline__ void slide_store(V *__restrict__ q, V *__restrict__ ring, int W, int ne, V *lds, const long long *s_row, int lane,
                                            bool valid, const V (&tail)[S], bool patch, const V (&tail2)[S]) {
    const int total = ne * W, q64 = 64 / W, r64 = 64 - q64 * W;
    {
        int c = lane % W;
        for (int idx = lane; idx < total; idx += 64) {
            if (c < W - S) lds[idx] = q[idx + S];   // (idx + S stays inside the env's own row)
            c += r64;
            if (c >= W) c -= W;
        }
    }
    if (valid) {
#pragma unroll
        for (int s = 0; s < S; ++s) lds[lane * W + W - S + s] = tail[s];
    }
    __syncthreads();
    {
        int e = lane / W, c = lane - e * W;
        for (int idx = lane; idx < total; idx += 64) {
            const long long row = s_row[e];
            if (row >= 0) ring[row * W + c] = lds[idx];
            e += q64; c += r64;
            if (c >= W) { c -= W; ++e; }
        }
    }
    if (PATCH) {
        __syncthreads();
        if (valid && patch) {
#pragma unroll
            for (int s = 0; s < S; ++s) lds[lane * W + W - S + s] = tail2[s];
        }
        __syncthreads();
    }
    for (int idx = lane; idx < total; idx += 64) q[idx] = lds[idx];
    __syncthreads();   // the buffer is free for the next array
}

// The three blocks below are statement macros, not functions: as inlined functions they compile to the same instructions in another
// order and with other registers, and k_env_step_nstep's assembly is to stay what it was (the same was seen with head_load /
// head_action, rollout_args.h).  Each names every variable it touches in its parameter list; a: the kernel's NStepLaunch.
//
// ---- base rank and total from the readiness bytes of THIS step (nothing in this launch writes them); 16 envs per lane and pass,
// a chunk lies wholly in front of this workgroup's envs or not at all (i0 is a multiple of 64).  s_row[lane] = the ring row of this
// lane's env, or -1; base, total (ints the caller declares in this order, = 0): this workgroup's base rank, the launch's ready envs.  s_ptr: the workgroup's shared copy of the
// ring cursor, written by lane 0 before (the barrier in here publishes it).  Every lane of the wave runs it.
#define DDRL_NSTEP_READY_ROWS(a, n, i0, i, valid, lane, s_ptr, s_row, base, total)                                                       \
    {                                                                                                                                    \
        for (long long c0 = 0; c0 < n; c0 += 1024) {                                                                                     \
            const long long at = c0 + 16 * lane;     /* (the arrays are zero-padded to a multiple of 1024) */                            \
            const uint4 u = *reinterpret_cast<const uint4 *>(a.rdy_in + at);                                                             \
            const int cnt = __popc(u.x) + __popc(u.y) + __popc(u.z) + __popc(u.w);                                                       \
            total += cnt;                                                                                                                \
            base += at < i0 ? cnt : 0;                                                                                                   \
        }                                                                                                                                \
        for (int off = 32; off >= 1; off >>= 1) {                                                                                        \
            total += __shfl_xor(total, off);                                                                                             \
            base += __shfl_xor(base, off);                                                                                               \
        }                                                                                                                                \
        const bool ready = valid && a.rdy_in[i] != 0;                                                                                    \
        const unsigned long long rb = __ballot(ready);                                                                                   \
        const int rank = base + __popcll(rb & ((1ull << lane) - 1ull));                                                                  \
        __syncthreads();                                                                                                                 \
        /* ranks below `skip` would be overwritten later in this batch */                                                                \
        const long long cap = a.ring.capacity, skip = total > cap ? total - cap : 0;                                                     \
        s_row[lane] = (ready && rank >= skip) ? (s_ptr + rank) % cap : -1;                                                               \
    }

// ---- c. t_queue, and the NEXT step's readiness
__device__ __forceinline__ void nstep_queue_tick(const NStepLaunch a, long long i, bool ended) {
    const int t1 = ended ? 1 : a.qt[i] + 1;                              // push: t += 1; begin: t = 1
    a.qt[i] = t1;
    a.rdy_out[i] = (t1 >= a.Ln && t1 % a.save_freq == 0) ? 1 : 0;
}

// ---- f. the next observation (o[8]) into the forward's buffer and the mirrors; o2[8]: the step's observation
#define DDRL_NSTEP_MIRRORS(a, i, o, o2, a0, a1, rew, done_env, ended)                                                                    \
    {                                                                                                                                    \
        const float4 n0 = make_float4(o[0], o[1], o[2], o[3]), n1 = make_float4(o[4], o[5], o[6], o[7]);                                 \
        {                                                                                                                                \
            float4 *p = reinterpret_cast<float4 *>(a.obs + i * 8);                                                                       \
            p[0] = n0; p[1] = n1;                                                                                                        \
        }                                                                                                                                \
        if (a.next_obs_out) {                                                                                                            \
            float4 *p = reinterpret_cast<float4 *>(a.next_obs_out + i * 8);                                                              \
            p[0] = n0; p[1] = n1;                                                                                                        \
        }                                                                                                                                \
        if (a.obs2_out) {                                                                                                                \
            float4 *p = reinterpret_cast<float4 *>(a.obs2_out + i * 8);                                                                  \
            p[0] = make_float4(o2[0], o2[1], o2[2], o2[3]);                                                                              \
            p[1] = make_float4(o2[4], o2[5], o2[6], o2[7]);                                                                              \
        }                                                                                                                                \
        if (a.act_out) *reinterpret_cast<float2 *>(a.act_out + i * 2) = make_float2(a0, a1);   /* the NOISY action (`action +=`) */      \
        if (a.rew_out) a.rew_out[i] = rew;                                                                                               \
        if (a.done_out) a.done_out[i] = done_env ? 1.0f : 0.0f;   /* raw d (the time-limit override is commented out, sac_ray.py:221) */ \
        if (a.ended_out) a.ended_out[i] = ended ? 1 : 0;                                                                                 \
    }

// ---- c. + d. the windows: slide, append, store the ready rows, start the ended envs' queues anew.  Every lane of the wave calls it
// (a lane without an env brings valid = false).
__device__ __forceinline__ void nstep_windows(const NStepLaunch a, long long i0, int ne, float4 *s_win, const long long *s_row, int lane, bool valid,
                                              const float (&o2)[8], const float (&o)[8], float a0, float a1, float rew, bool done_env, bool ended) {
    const int Ln = a.Ln;
    const float4 to[2] = {make_float4(o2[0], o2[1], o2[2], o2[3]), make_float4(o2[4], o2[5], o2[6], o2[7])};
    const float4 tn[2] = {make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7])};
    slide_store<float4, 2, true>(reinterpret_cast<float4 *>(a.qo) + i0 * (Ln + 1) * 2, reinterpret_cast<float4 *>(a.ring.a[0]), (Ln + 1) * 2, ne,
                                 s_win, s_row, lane, valid, to, ended, tn);
    const float2 ta[1] = {make_float2(a0, a1)};
    slide_store<float2, 1, false>(reinterpret_cast<float2 *>(a.qa) + i0 * Ln, reinterpret_cast<float2 *>(a.ring.a[1]), Ln, ne,
                                  reinterpret_cast<float2 *>(s_win), s_row, lane, valid, ta, false, ta);
    const float tr[1] = {rew}, td[1] = {done_env ? 1.0f : 0.0f};
    slide_store<float, 1, false>(a.qr + i0 * Ln, a.ring.a[2], Ln, ne, reinterpret_cast<float *>(s_win), s_row, lane, valid, tr, false, tr);
    slide_store<float, 1, false>(a.qd + i0 * Ln, a.ring.a[3], Ln, ne, reinterpret_cast<float *>(s_win), s_row, lane, valid, td, false, td);
}

// ---- the episode statistics (wave reduction, one atomic per workgroup that saw an episode end), then the next forward's plan and the
// ring ticket: the last workgroup to finish advances the cursor by the number of ready envs (every workgroup has read rs->ptr before
// its ticket) and, with a plan riding, builds the forward's workgroup table.  n_end / len_end / ret_end are consumed.
#define DDRL_NSTEP_FINISH(a, n, i, lane, n_end, len_end, ret_end, my_slot, s_ptr, total)                                                 \
    {                                                                                                                                    \
        for (int off = 32; off >= 1; off >>= 1) {                                                                                        \
            n_end += __shfl_xor(n_end, off);                                                                                             \
            len_end += __shfl_xor(len_end, off);                                                                                         \
            ret_end += __shfl_xor(ret_end, off);                                                                                         \
        }                                                                                                                                \
        if (lane == 0 && n_end > 0) {                                                                                                    \
            EnvStats *stats = static_cast<EnvStats *>(a.stats);                                                                          \
            atomicAdd((unsigned long long *)&stats->episodes, (unsigned long long)n_end);                                                \
            atomicAdd((unsigned long long *)&stats->len_sum, (unsigned long long)len_end);                                               \
            atomicAdd(&stats->ret_sum, ret_end);                                                                                         \
        }                                                                                                                                \
        const VerPlan vp{a.vcnt, a.perm, a.perm2d_off, a.vtiles, a.vs, a.n_slots, a.col_tiles, a.wg_slots, a.vt_cap};                   \
        ver_plan_tail(vp, my_slot, i, n, NStepTicket{a.rs, a.ring, s_ptr, (long long)total});                                            \
    }

}  // namespace
