// The version store's side of an env-step launch, shared by the continuous and the discrete fused rollout step (lander.hip: k_env_step_pi,
// k_env_step_q<.., true>) so that the two paths cannot drift.  The tables it writes are those of policy_row.h (VerTile, VerState, ver_split),
// read by the versioned policy / Q forward (k_actor_fwd<.., true>, sac1_direct.h).
#pragma once
#include "policy_row.h"

// ---- the NEXT versioned forward's plan, written by an env-step launch.  Every env counts itself into its next slot's group and files itself in that
// group's row list; the last workgroup to pass the launch's ring-commit ticket turns the counts into the forward's workgroup table (what
// k_version_plan does as a launch of its own, 7-11 us between the env-step launch and the forward that waits for it).
struct VerPlan {
    int *vcnt;             // [VER_MAX_SLOTS], zero on entry, zero again on exit; nullptr: no plan rides in this launch
    int *perm;             // row lists: group s at perm[perm2d_off + s * n ..)
    long long perm2d_off;
    VerTile *vtiles;
    VerState *vs;
    int n_slots, col_tiles, wg_slots, vt_cap;
};
// One wave per workgroup (blockDim.x == 64), called by every thread of the launch at its end.  my_slot: the slot env i acts on at the NEXT
// step (i < n); `commit()` is the launch's ring ticket, run by thread 0 between the grouping and the table build: true in the last workgroup
// to finish.
template <class Commit>
__device__ __forceinline__ void ver_plan_tail(const VerPlan &a, int my_slot, long long i, long long n, Commit commit) {
    __shared__ int s_last;
    if (a.vcnt) {
        // this env's place in its group: the lanes of a wave that share a slot go as ONE atomic of their leader (a few thousand envs sit
        // on a handful of versions; all leaders' atomics leave in one instruction: one round trip whatever the number of groups)
        const int lane = threadIdx.x & 63;
        const bool valid = i < n;
        unsigned long long todo = __ballot(valid);
        int gsize = 0, rank = 0, leader = lane;
        while (todo) {
            const int ld = __ffsll((long long)todo) - 1;
            const int s0 = __builtin_amdgcn_readlane(my_slot, ld);   // (ld is wave-uniform: no trip through the LDS crossbar per group)
            const bool mine = valid && my_slot == s0;
            const unsigned long long m = __ballot(mine);
            if (mine) { gsize = __popcll(m); rank = __popcll(m & ((1ull << lane) - 1ull)); leader = ld; }
            todo &= ~m;
        }
        int base = 0;
        if (valid && lane == leader) base = atomicAdd(&a.vcnt[my_slot], gsize);
        base = __shfl(base, leader);
        if (valid) a.perm[a.perm2d_off + (long long)my_slot * n + base + rank] = (int)i;
        // (no fence: the counts are device-scope atomics whose results this wave has waited for — performed before its ticket below —
        // and nothing else crosses workgroups inside this launch: row lists, records and slots are read by the NEXT launch.  A
        // __threadfence() here writes back the L2's dirty lines — this launch's ring rows — in every workgroup: +8 us measured.)
    }
    // the last block to finish advances the ring cursor (every block has read the cursor before its ticket)
    __syncthreads();
    if (threadIdx.x == 0) s_last = commit() ? 1 : 0;
    if (!a.vcnt) return;
    __syncthreads();
    if (!s_last) return;   // block-uniform
    // ---- the last workgroup (one wave): the counts -> the next forward's workgroup table (the tables of k_version_plan, actor.hip; the
    // row lists are this launch's own: group s at perm2d_off + s * n, so a record's row-list base is known without a scatter pass)
    __shared__ int t_cnt[VER_MAX_SLOTS], t_start[VER_MAX_SLOTS];
    __shared__ unsigned short t_slot[VER_MAX_SLOTS + 1024];   // slot of row tile ti (n / 32 + live groups <= 1024 + 2048 tiles)
    const int lane = threadIdx.x;   // (the counts are read with device-scope atomic loads, behind this workgroup's own ticket)
    constexpr int PER = VER_MAX_SLOTS / 64;
    const int per = (a.n_slots + 63) >> 6;   // slots per lane (<= PER): lane l holds slots [per l, per l + per)
    int c[PER], run = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = per * lane + q;
        c[q] = (q < per && j < a.n_slots) ? __hip_atomic_load(&a.vcnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        run += (c[q] + 31) >> 5;
    }
    int incl = run;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    const int total = __shfl(incl, 63);
    // slot of every row tile: each group's first tile gets its slot number, a running maximum over the tiles fills the rest (groups lie
    // in slot order) — `chunk` tiles per lane, so the one big group of the newest version is not one lane's loop
    const int chunk = (total + 63) >> 6;
    for (int k = 0; k < chunk; ++k) t_slot[lane * chunk + k] = 0;
    __syncthreads();
    int ts = incl - run;   // first row tile of this lane's first slot
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        if (q < per) {   // wave-uniform
            const int j = per * lane + q, nt = (c[q] + 31) >> 5;
            if (j < VER_MAX_SLOTS) { t_cnt[j] = c[q]; t_start[j] = ts; }
            if (nt > 0) { t_slot[ts] = (unsigned short)j; a.vcnt[j] = 0; }   // (... and zero again for the next launch)
            ts += nt;
        }
    }
    const VerSplit sp = ver_split(total, a.col_tiles, a.wg_slots, a.vt_cap);
    if (lane == 0) { a.vs->n_tiles = total; a.vs->n_wgs = sp.n_wgs; }
    __syncthreads();
    {
        int mx = 0;
        for (int k = 0; k < chunk; ++k) mx = max(mx, (int)t_slot[lane * chunk + k]);
        int inc = mx;
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc = max(inc, u);
        }
        int runmx = __shfl_up(inc, 1);
        if (lane == 0) runmx = 0;
        for (int k = 0; k < chunk; ++k) {
            runmx = max(runmx, (int)t_slot[lane * chunk + k]);
            t_slot[lane * chunk + k] = (unsigned short)runmx;
        }
    }
    __syncthreads();
    // (one wave: every instruction counts — the divisions by the two group counts are done once, the per-record ones by reciprocal)
    const int n_long_wgs = sp.n_long * sp.g_long;
    const int gb_l = a.col_tiles / sp.g_long, ge_l = a.col_tiles % sp.g_long, gb_s = a.col_tiles / sp.g_short, ge_s = a.col_tiles % sp.g_short;
    const float inv_l = 1.0f / (float)sp.g_long, inv_s = 1.0f / (float)sp.g_short;
    const int base0 = (int)a.perm2d_off, ni = (int)n;
    for (int b = lane; b < sp.n_wgs; b += 64) {
        const bool lg = b < n_long_wgs;
        const int g = lg ? sp.g_long : sp.g_short, bb = lg ? b : b - n_long_wgs;
        const int q = (int)(((float)bb + 0.5f) * (lg ? inv_l : inv_s));   // bb / g: exact (bb < 2^20, g <= 16: the product is >= 0.03 off a whole number)
        const int ti = (lg ? 0 : sp.n_long) + q, grp = bb - q * g;
        const int j = t_slot[ti], k = ti - t_start[j], cj = t_cnt[j];
        const int gbase = lg ? gb_l : gb_s, gextra = lg ? ge_l : ge_s;
        const int ntl = gbase + (grp < gextra ? 1 : 0), nt0 = grp * gbase + (grp < gextra ? grp : gextra);
        a.vtiles[b] = VerTile{j, base0 + j * ni + 32 * k, cj - 32 * k < 32 ? cj - 32 * k : 32, nt0 | (ntl << 8)};
    }
}
