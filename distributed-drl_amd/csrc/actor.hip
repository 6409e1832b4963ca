// The actor handle (ddrl_actor_*) on gfx950: Actor.get_action of algos/sac1/actor_learner.py:195-197 on the network of
// algos/sac1/core.py:91-121, as the batched forward on the generic kernels (ddrl_actor_act), the single-row launch (ddrl_actor_act_one)
// and the direct-operand forward k_actor_fwd (sac1_direct.h) of the fused rollout steps (env.hip) and of the DQN / SQN handles' acting
// forwards (dqn.hip) — plain, or versioned: every env against the policy version it adopted at its last episode end (the version
// store: example/dsac.py:127-130).  The store's device tables are also written by the env-step launches (version_plan.h); its host
// state has ONE owner, this file (struct ddrl_actor; ddrl_actor_internal_step_begin / _end for the fused steps).
// fp contraction is OFF for this file, as for the learner's: the same formulae in the same order (sac1.hip).
#include "gemm_core.h"
#include "policy_row.h"

namespace {
#include "sac1_direct.h"
}  // namespace
#include "sac1_layout.h"

namespace {
// ------------------------------------------------------------------------------------------
// K: batched get_action — one wave per observation row (Actor.get_action, actor_learner.py:195-197)
// ------------------------------------------------------------------------------------------
struct ActArgs {
    const float *H2;
    NetPi pi;
    const float *eps;
    float *act_out;
    int rows, h2, ldh2, act, deterministic;
    float scale;
};
__global__ void __launch_bounds__(256) k_rows_act(ActArgs a) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.rows) return;
    float hrow[RV];
    load_row(a.H2 + r * a.ldh2, a.h2, lane, hrow);
    const float el = (a.deterministic || !a.eps) ? 0.f : a.eps[r * a.act + (lane < a.act ? lane : 0)];
    mask_row(hrow, a.h2, lane);
    const HeadOut o = policy_head(hrow, a.h2, a.act, a.pi, el, a.scale, lane);
    if (lane < a.act) a.act_out[r * a.act + lane] = o.act;
}

// get_action of ONE observation as one launch: every workgroup computes layer 1 (a few thousand products) and ITS 16 columns of layer 2
// — 256 threads = 16 columns x 16 slices of the contraction, combined in slice order — and leaves the head's partial sums of those
// columns; the last workgroup to finish (ticket) adds the partials in workgroup order, takes the noise elements from the counter
// (== ddrl_normal_fill) and squashes (ddrl_pol::policy_row).  One workgroup alone pulls layer 2's 480 KB through one CU (~25 us);
// the batched path is three launches behind a noise launch — a chain of four for one row, which is what a reference-style
// rollout worker pays per env step (actor_learner.py:195-197; example/dsac.py:96).
constexpr int A1_COLS = 16;
struct ActOneArgs {
    const float *obs;
    NetPi pi;
    float *act_out;
    float *part;             // [workgroups][16]: head partial sums (mu 0..act-1, log_std act..2act-1)
    unsigned int *ticket;
    int d0, h1, h2, act, deterministic;
    float scale;
    uint32_t seed;
    unsigned long long ctr;
};
__global__ void __launch_bounds__(256) k_act_one(ActOneArgs a) {
    __shared__ float xs[64];
    __shared__ float h1s[512];
    __shared__ float ps[16][A1_COLS + 1];
    __shared__ float v2[A1_COLS];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (tid < a.d0) xs[tid] = a.obs[tid];
    __syncthreads();
    const int col = tid & (A1_COLS - 1), slice = tid >> 4, c = blockIdx.x * A1_COLS + col;
    const int per = (a.h1 + 15) >> 4, k0 = slice * per, k1 = k0 + per < a.h1 ? k0 + per : a.h1;   // per <= 32
    // this thread's layer-2 operands are requested now (they do not depend on layer 1): one round trip under the layer-1 phase
    float w2[32];
    const int cc2 = c < a.h2 ? c : 0;
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const int k = k0 + q < k1 ? k0 + q : (k0 < a.h1 ? k0 : 0);
        w2[q] = a.pi.W2[(long long)k * a.h2 + cc2];
    }
    {   // layer 1: units tid and tid + 256, eight input rows per round trip for both
        const int j0 = tid < a.h1 ? tid : 0, j1 = tid + 256 < a.h1 ? tid + 256 : 0;
        float acc0 = a.pi.b1[j0], acc1 = a.pi.b1[j1];
        for (int d = 0; d < a.d0; d += 8) {
            float u0[8], u1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int dd = d + q < a.d0 ? d + q : 0;
                u0[q] = a.pi.W1[(long long)dd * a.h1 + j0]; u1[q] = a.pi.W1[(long long)dd * a.h1 + j1];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (d + q < a.d0) { acc0 += xs[d + q] * u0[q]; acc1 += xs[d + q] * u1[q]; }
        }
        if (tid < a.h1) h1s[tid] = fmaxf(acc0, 0.f);
        if (tid + 256 < a.h1) h1s[tid + 256] = fmaxf(acc1, 0.f);
    }
    __syncthreads();
    float acc = 0.f;
    if (c < a.h2) {
#pragma unroll
        for (int q = 0; q < 32; ++q)
            if (k0 + q < k1) acc += h1s[k0 + q] * w2[q];   // k order
    }
    ps[slice][col] = acc;
    __syncthreads();
    if (tid < A1_COLS) {
        const int cc = blockIdx.x * A1_COLS + tid;
        float sum = 0.f;
        if (cc < a.h2) {
            sum = a.pi.b2[cc];
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += ps[q][tid];
            sum = fmaxf(sum, 0.f);
        }
        v2[tid] = sum;
    }
    __syncthreads();
    if (tid < 2 * a.act) {   // head partials of this workgroup's columns: outputs 0..act-1 mu, act..2act-1 log_std
        const float *W = tid < a.act ? a.pi.Wmu : a.pi.Wls;
        const int o = tid < a.act ? tid : tid - a.act;
        float sum = 0.f;
        for (int q = 0; q < A1_COLS; ++q) {
            const int cc = blockIdx.x * A1_COLS + q;
            if (cc < a.h2) sum += v2[q] * W[(long long)cc * a.act + o];
        }
        a.part[blockIdx.x * 16 + tid] = sum;
    }
    __threadfence();   // the partials are out before the ticket (this launch has written nothing else)
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    __shared__ float s_part[32 * 16];
    for (int i = tid; i < (int)gridDim.x * 16; i += 256)   // every partial in ONE round trip (a serial chain of device-scope loads by one thread: +7 us)
        s_part[i] = __hip_atomic_load(&a.part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, ls[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f};
        for (int o = 0; o < a.act; ++o) {
            float sm = 0.f, sl = 0.f;
            for (unsigned b = 0; b < gridDim.x; ++b) {   // workgroup order
                sm += s_part[b * 16 + o];
                sl += s_part[b * 16 + a.act + o];
            }
            mu[o] = sm + a.pi.bmu[o]; ls[o] = sl + a.pi.bls[o];
            ev[o] = a.deterministic ? 0.f : ddrl_pol::normal_at(a.seed, a.ctr + (unsigned long long)o);
        }
        const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, a.act, a.scale);
        for (int o = 0; o < a.act; ++o) a.act_out[o] = pr.act[o];
        *a.ticket = 0u;
    }
}

}  // namespace

// ==========================================================================================
// Actor: batched Actor.get_action
// ==========================================================================================
struct ddrl_actor {
    int device = 0;
    ddrl_sac1_config_t cfg{};
    Layout L;
    float *pi_p = nullptr;  // padded internal
    float *H1 = nullptr, *H2 = nullptr;
    Seg *segs_d = nullptr;
    long long max_rows = 0;
    int ldh1 = 0, ldh2 = 0;
    // fused rollout step (ddrl_rollout_step): the policy in the direct-operand layout + the observation rows it acts on +
    // the head partials of the forward launch, in ONE slab (k_dfwd addresses everything as base + 32-bit offset)
    bool direct = false;
    Layout Ld;
    float *dslab = nullptr, *pi_d = nullptr, *obs_d = nullptr, *hp_d = nullptr;
    Seg *segs_dd = nullptr;
    // version store (ddrl_actor_versions_enable): n_slots copies of the direct-layout policy, the slot every env acts on, the
    // grouping of the envs by slot for the forward launch.  pi_d stays the newest weights.
    int n_slots = 0;
    long long vstride = 0;
    float *vslab = nullptr;
    int *slot_d = nullptr, *perm_d = nullptr;   // perm_d: the row list of every tile, [tiles][32] (+ parking space of k_version_plan)
    bool pi_p_stale = false;       // direct actors: the row-major copy (ddrl_actor_act / get_weights) is rebuilt from pi_d on demand
    float *flat_tmp = nullptr;     // ... through this dense staging vector
    VerTile *vtiles_d = nullptr;
    VerState *vs_d = nullptr;
    int vt_cap = 0;                // records of the forward's workgroup table (= the versioned forward's grid)
    float *act1_part = nullptr;    // ddrl_actor_act_one: head partials + ticket (allocated at the first call)
    int *vcnt_d = nullptr;         // envs per slot while an env-step launch counts them; all zero between launches
    long long perm2d_off = 0;      // perm_d: where the env-step launch's [n_slots][max_rows] row lists start
    int wg_slots = 0;              // resident workgroups of the two-per-CU forward: 2 x CUs (the planning launch sizes the column split for it)
    // The version store's HOST state.  Nothing outside this file reads or writes the two fields; the fused steps of env.hip go through
    // ddrl_actor_internal_step_begin / _end.  The invariant they keep:
    //   plan_fresh                     <=> the forward's workgroup table and row lists (vtiles_d, perm_d) match the envs' slots (slot_d);
    //   steps_since_install >= horizon <=> every env has been through an episode end since the last install and acts on the newest
    //                                      version (horizon: the envs' max_ep_len, or the wrapped step's limit_steps), so the plain
    //                                      forward on pi_d is the same computation as the versioned one.
    // steps_since_install   = 0         ddrl_actor_set_weights on a store (the install)
    //                       = 1 << 40   ddrl_actor_versions_enable, and from creation on (no install yet: every env is on slot 0 = pi_d)
    //                       += 1        ddrl_actor_internal_step_begin: one vector step (ddrl_actor_act_versioned, the fused steps)
    // plan_fresh            = true      ddrl_actor_set_weights on a store (its planning launch), ddrl_actor_internal_forward(versioned)
    //                                   (plans first unless already fresh)
    //                       = planned   ddrl_actor_internal_step_end: what the launch behind the forward left — true where its own tail
    //                                   planned for the envs it moved (or it moved none), false where it moved envs unplanned
    //                       = false     ddrl_actor_versions_adopt (moves envs), ddrl_actor_versions_enable, creation
    long long steps_since_install = 1ll << 40;
    bool plan_fresh = false;
};

// floats of the policy part of dslab and of one version slot (the direct-layout policy and the operand guard behind it, on a 256-byte grid)
static size_t policy_slab_floats(const Layout &Ld) { return ((size_t)Ld.total_int + 2048 + 63) & ~(size_t)63; }

// ---- version store kernels -------------------------------------------------------------------------------------------
// One workgroup.  Picks the slot the incoming weights go to: the newest slot itself when no env has adopted it yet (nobody
// can ever act on it again once a newer version exists: a worker pulls whatever the server holds at ITS episode end), else
// the lowest slot no env acts on.  n_slots >= min(n_envs, max_ep_len) + 2 always leaves one.
__global__ void __launch_bounds__(256) k_version_copy(const float *__restrict__ src, float *__restrict__ vslab, long long vstride,
                                                      const VerState *__restrict__ vs, long long n4) {
    float4 *dst = reinterpret_cast<float4 *>(vslab + (long long)vs->target * vstride);
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) dst[i] = s4[i];
}

// One workgroup: envs grouped by slot (counting sort; the order inside a group is immaterial — rows are computed
// independently), one VerTile per 32 envs of a group.
// arr[s] += 1 for every valid lane, the lane's position in its group returned.  A few thousand envs sit on a handful of versions most
// of the time: 64 lanes on ONE LDS address are 64 serialised atomics, so the lanes that share the slot of the first pending lane go
// as one atomic (four such rounds: the four largest groups of the wave, typically all of it); what is left takes its own.
__device__ __forceinline__ int ver_group_add(int *arr, int s, bool valid, int lane) {
    unsigned long long todo = __ballot(valid);
    int pos = 0;
    for (int round = 0; round < 4 && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const int s0 = __shfl(s, leader);
        const bool mine = valid && s == s0;
        const unsigned long long m = __ballot(mine);
        int base = 0;
        if (lane == leader) base = atomicAdd(&arr[s0], __popcll(m));
        base = __shfl(base, leader);
        if (mine) { pos = base + __popcll(m & ((1ull << lane) - 1ull)); valid = false; }
        todo &= ~m;
    }
    if (valid) pos = atomicAdd(&arr[s], 1);
    return pos;
}
// ONE launch (one workgroup) plans a versioned forward — and, with `install`, first picks the slot incoming weights go to.
//   pick   the newest slot itself while no env has adopted it (nobody can ever act on a superseded version that nobody holds: a worker
//          pulls whatever the server holds at ITS episode end), else the lowest slot no env acts on (n_slots >= min(n_envs, max_ep_len) + 2
//          always leaves one); sticky vs->err when none is free.  The grouping does not depend on the pick: no env sits on the target.
//   group  envs by slot (counting sort; the order inside a group is immaterial — rows are computed independently), one VerTile per 32
//          envs of a group, and the envs of tile ti at rows[32 ti .. 32 ti + count): the forward reads its tile record and its row list
//          with two INDEPENDENT loads (round 4 chained n_tiles -> tile -> dense permutation -> observation rows: four round trips before
//          the first operand).  An env's position in its group is the value its histogram atomic returned — one atomic pass, not two.
constexpr int VER_REG_ENVS = 8;   // envs per thread kept in registers across the passes (8192 envs: config 4's rollout ranks)
__global__ void __launch_bounds__(1024) k_version_plan(const int *__restrict__ slot, long long n, int n_slots, int *__restrict__ rows,
                                                       VerTile *__restrict__ tiles, VerState *vs, int install, int col_tiles, int wg_slots,
                                                       int tiles_cap) {
    __shared__ int cnt[VER_MAX_SLOTS], tstart[VER_MAX_SLOTS];
    __shared__ int wsum_t[16], s_free, s_live;
    __shared__ VerSplit s_split;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int sv[VER_REG_ENVS], pv[VER_REG_ENVS];
#pragma unroll
    for (int e = 0; e < VER_REG_ENVS; ++e) sv[e] = t + 1024 * e < n ? slot[t + 1024 * e] : 0;
    for (int j = t; j < VER_MAX_SLOTS; j += 1024) cnt[j] = 0;
    if (t == 0) { s_free = n_slots; s_live = 0; }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VER_REG_ENVS; ++e) pv[e] = ver_group_add(cnt, sv[e], t + 1024 * e < n, lane);
    for (long long i0 = 1024ll * VER_REG_ENVS; i0 < n; i0 += 1024) {   // (more envs than the registers hold: positions parked in `rows`' tail)
        const bool ok = i0 + t < n;
        const int p = ver_group_add(cnt, ok ? slot[i0 + t] : 0, ok, lane);
        if (ok) rows[32ll * (n / 32 + n_slots) + (i0 + t)] = p;
    }
    __syncthreads();
    const int newest = vs->newest;
    // exclusive scan of the groups' tile counts: two slots per thread, wave scan, wave totals
    const int c0 = cnt[2 * t], c1 = cnt[2 * t + 1];
    const int t0 = (c0 + 31) >> 5, t1 = (c1 + 31) >> 5;
    int st = t0 + t1;
    for (int o = 1; o < 64; o <<= 1) {
        const int ut = __shfl_up(st, o);
        if (lane >= o) st += ut;
    }
    if (lane == 63) wsum_t[w] = st;
    if (install) {
        int live = (c0 > 0) + (c1 > 0);
        int fr = n_slots;
        if (2 * t + 1 < n_slots && c1 == 0 && 2 * t + 1 != newest) fr = 2 * t + 1;
        if (2 * t < n_slots && c0 == 0 && 2 * t != newest) fr = 2 * t;
        for (int o = 32; o >= 1; o >>= 1) { live += __shfl_xor(live, o); fr = min(fr, __shfl_xor(fr, o)); }
        if (lane == 0) { atomicAdd(&s_live, live); atomicMin(&s_free, fr); }
    }
    __syncthreads();
    int bt = 0;
    for (int k = 0; k < w; ++k) bt += wsum_t[k];
    const int et = bt + st - (t0 + t1);   // exclusive prefix of this thread's pair
    tstart[2 * t] = et; tstart[2 * t + 1] = et + t0;
    if (t == 1023) {
        const VerSplit sp = ver_split(bt + st, col_tiles, wg_slots, tiles_cap);
        vs->n_tiles = bt + st; vs->n_wgs = sp.n_wgs; s_split = sp;
    }
    if (t == 0 && install) {
        int target = newest;
        if (cnt[newest] > 0) {
            if (s_free < n_slots) target = s_free;
            else vs->err = 1;              // sticky: no free slot (the newest one is overwritten: its envs act on fresher weights)
        }
        vs->target = target;
        vs->newest = target;
        vs->live = s_live;
    }
    __syncthreads();
    // one record per WORKGROUP of the forward (ver_split: the long workgroups of the full rounds first, the surplus tiles' short ones
    // behind them).  Tile ti belongs to the LAST slot whose first tile is <= ti (the empty slots behind it start where it ends)
    const VerSplit sp = s_split;
    const int n_long_wgs = sp.n_long * sp.g_long;
    for (int b = t; b < sp.n_wgs; b += 1024) {
        const bool lg = b < n_long_wgs;
        const int g = lg ? sp.g_long : sp.g_short, bb = lg ? b : b - n_long_wgs;
        const int ti = (lg ? 0 : sp.n_long) + bb / g, grp = bb % g;
        int lo = 0, hi = VER_MAX_SLOTS;            // first index with tstart > ti
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tstart[mid] > ti) hi = mid; else lo = mid + 1;
        }
        const int j = lo - 1, k = ti - tstart[j], c = cnt[j];
        const int gbase = col_tiles / g, gextra = col_tiles % g;   // column tiles dealt to the g workgroups as evenly as they go
        const int ntl = gbase + (grp < gextra ? 1 : 0), nt0 = grp * gbase + (grp < gextra ? grp : gextra);
        tiles[b] = VerTile{j, 32 * ti, c - 32 * k < 32 ? c - 32 * k : 32, nt0 | (ntl << 8)};
    }
#pragma unroll
    for (int e = 0; e < VER_REG_ENVS; ++e)
        if (t + 1024 * e < n) rows[32 * (tstart[sv[e]] + (pv[e] >> 5)) + (pv[e] & 31)] = t + 1024 * e;
    for (long long i0 = 1024ll * VER_REG_ENVS; i0 < n; i0 += 1024) {
        if (i0 + t < n) {
            const int p = rows[32ll * (n / 32 + n_slots) + (i0 + t)];
            rows[32 * (tstart[slot[i0 + t]] + (p >> 5)) + (p & 31)] = (int)(i0 + t);
        }
    }
}

// k_pack into the actor's current direct-layout policy AND into the version slot k_version_plan picked (one launch instead of a pack and
// a 0.5 MB copy; the slots' pads stay as allocated: zero, like the current copy's)
__global__ void __launch_bounds__(256) k_pack_version(const Seg *__restrict__ segs, const float *__restrict__ src, float *__restrict__ dst,
                                                      float *__restrict__ vslab, long long vstride, const VerState *__restrict__ vs) {
    const Seg s = segs[blockIdx.y];
    float *dst2 = vslab + (long long)vs->target * vstride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += (long long)gridDim.x * 256) {
        long long ii = i;
        if (s.cols > 0) {
            const long long k = i / s.cols, j = i - k * s.cols;
            ii = s.mode == 2 ? w1y_index(s.d0 + (int)k, (int)j) : ((k >> 2) * s.ld + j) * 4 + (k & 3);
        }
        const float v = src[s.ext + i];
        dst[s.in + ii] = v;
        dst2[s.in + ii] = v;
    }
}

// get_action from the head partials of a (versioned) forward launch — what k_env_step_pi does before it steps the physics — for callers
// that step their envs themselves (the n-step rollout: ddrl_actor_act_versioned).  One lane per row, same summation order.
struct FinishArgs {
    const float *hp;          // [8][n][16]
    const float *bmu, *bls;   // slot 0's head biases; slot s: + s * vstride (slot == nullptr: the current weights')
    const int *slot;
    long long vstride, n;
    const float *eps;         // [n][act] (nullptr when deterministic)
    float *act_out;           // [n][act]
    int act, nt2, deterministic;
    float scale;
};
__global__ void __launch_bounds__(64) k_actor_finish(FinishArgs a) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x, n = a.n;
    if (i >= n) return;
    const int nq = (a.nt2 + 3) >> 2;
    const long long voff = a.slot ? (long long)a.slot[i] * a.vstride : 0;
    float mu[4], ls[4], ev[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float sm = 0.f, sl = 0.f;
        if (c < a.act) {
            for (int q = 0; q < nq; ++q) {   // n-tile order; slots beyond nt2 hold 0
                const float4 m4 = *reinterpret_cast<const float4 *>(a.hp + ((long long)c * n + i) * 16 + 4 * q);
                const float4 l4 = *reinterpret_cast<const float4 *>(a.hp + ((long long)(a.act + c) * n + i) * 16 + 4 * q);
                sm += m4.x; sm += m4.y; sm += m4.z; sm += m4.w;
                sl += l4.x; sl += l4.y; sl += l4.z; sl += l4.w;
            }
        }
        const int cc = c < a.act ? c : 0;
        mu[c] = sm + a.bmu[voff + cc];
        ls[c] = sl + a.bls[voff + cc];
        ev[c] = (a.deterministic || c >= a.act || !a.eps) ? 0.f : a.eps[i * a.act + c];
    }
    const ddrl_pol::PolRow pr = ddrl_pol::policy_row(mu, ls, ev, a.act, a.scale);
    for (int c = 0; c < a.act; ++c) a.act_out[i * a.act + c] = a.deterministic ? tanhf(mu[c]) * a.scale : pr.act[c];
}

__global__ void __launch_bounds__(256) k_version_adopt(int *__restrict__ slot, const uint8_t *__restrict__ ended, long long n, const VerState *vs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && ended[i]) slot[i] = vs->newest;
}

extern "C" {

int ddrl_actor_create(ddrl_actor_t **out, int device, const ddrl_sac1_config_t *cfg, int64_t max_rows) {
    DDRL_REQUIRE(out != nullptr && max_rows > 0, "bad out/max_rows");
    int rc = check_cfg(cfg);
    if (rc != DDRL_OK) return rc;
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_actor *h = new ddrl_actor();
    h->device = device; h->cfg = *cfg; h->max_rows = max_rows;
    h->L = make_layout(*cfg, true);
    const size_t guard = 2048;  // floats of readable memory behind every GEMM operand (unclamped tile loads)
    hipError_t e = dev_alloc(&h->pi_p, (size_t)h->L.total_int + guard);
    h->ldh1 = (int)pad4(cfg->hidden1); h->ldh2 = (int)pad4(cfg->hidden2);
    if (e == hipSuccess) e = dev_alloc(&h->H1, (size_t)max_rows * h->ldh1 + guard);
    if (e == hipSuccess) e = dev_alloc(&h->H2, (size_t)max_rows * h->ldh2 + guard);
    if (e == hipSuccess) e = dev_alloc(&h->segs_d, h->L.segs.size());
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc failed in ddrl_actor_create: %s", hipGetErrorString(e));
        ddrl_actor_destroy(h);
        return DDRL_ERR_NOMEM;
    }
    DDRL_HIP_CHECK(hipMemcpy(h->segs_d, h->L.segs.data(), h->L.segs.size() * sizeof(Seg), hipMemcpyHostToDevice));
    {
        ddrl_sac1_config_t c2 = *cfg;
        c2.batch = 32;
        h->direct = direct_ok(c2) && max_rows % 32 == 0 && max_rows <= 32 * 4095 && cfg->obs_dim + 1 <= 13;
    }
    if (h->direct) {
        h->Ld = make_layout(*cfg, true, true);
        const size_t np = policy_slab_floats(h->Ld), no = ((size_t)max_rows * cfg->obs_dim + 63) & ~(size_t)63;
        const size_t nh = (size_t)DFH * max_rows * DNT;
        e = dev_alloc(&h->dslab, np + no + nh + 2048);
        if (e == hipSuccess) e = dev_alloc(&h->segs_dd, h->Ld.segs.size());
        if (e == hipSuccess) e = dev_alloc(&h->flat_tmp, (size_t)h->L.total_ext + 64);
        if (e != hipSuccess) {
            ddrl::set_error("hipMalloc failed in ddrl_actor_create: %s", hipGetErrorString(e));
            ddrl_actor_destroy(h);
            return DDRL_ERR_NOMEM;
        }
        h->pi_d = h->dslab; h->obs_d = h->dslab + np; h->hp_d = h->obs_d + no;
        DDRL_HIP_CHECK(hipMemcpy(h->segs_dd, h->Ld.segs.data(), h->Ld.segs.size() * sizeof(Seg), hipMemcpyHostToDevice));
    }
    *out = h;
    return DDRL_OK;
}

int ddrl_actor_destroy(ddrl_actor_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    (void)hipFree(h->dslab); (void)hipFree(h->segs_dd); (void)hipFree(h->flat_tmp);
    (void)hipFree(h->vslab); (void)hipFree(h->slot_d); (void)hipFree(h->perm_d); (void)hipFree(h->vtiles_d); (void)hipFree(h->vs_d); (void)hipFree(h->vcnt_d); (void)hipFree(h->act1_part);
    (void)hipFree(h->pi_p); (void)hipFree(h->H1); (void)hipFree(h->H2); (void)hipFree(h->segs_d);
    delete h;
    return DDRL_OK;
}

int ddrl_actor_set_weights(ddrl_actor_t *h, const float *flat_pi_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_pi_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    if (!h->direct) {
        k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, s>>>(h->segs_d, flat_pi_d, h->pi_p, nullptr, 1);
    } else if (h->n_slots > 0) {
        // version store: the new weights become the newest version, in a slot no env acts on — ONE planning launch (slot pick + the tile
        // table of the next forward) and ONE pack into the current copy and that slot (round 4: two packs, the pick, a 0.5 MB copy
        // and, in the step, the grouping: five launches)
        k_version_plan<<<1, 1024, 0, s>>>(h->slot_d, h->max_rows, h->n_slots, h->perm_d, h->vtiles_d, h->vs_d, 1, (h->cfg.hidden2 + 31) / 32, h->wg_slots, h->vt_cap);
        k_pack_version<<<dim3(64, (unsigned)h->Ld.segs.size()), 256, 0, s>>>(h->segs_dd, flat_pi_d, h->pi_d, h->vslab, h->vstride, h->vs_d);
        h->plan_fresh = true;
        h->steps_since_install = 0;
        h->pi_p_stale = true;
    } else {
        k_pack<<<dim3(64, (unsigned)h->Ld.segs.size()), 256, 0, s>>>(h->segs_dd, flat_pi_d, h->pi_d, nullptr, 1);
        h->pi_p_stale = true;   // the row-major copy only serves ddrl_actor_act / get_weights: rebuilt there
    }
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

// direct actors: the row-major policy (generic kernels of ddrl_actor_act, ddrl_actor_get_weights) from the direct-layout one, on demand
static void actor_refresh_row_major(ddrl_actor *h, hipStream_t s) {
    if (!h->pi_p_stale) return;
    k_pack<<<dim3(64, (unsigned)h->Ld.segs.size()), 256, 0, s>>>(h->segs_dd, h->pi_d, h->flat_tmp, nullptr, 0);
    k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, s>>>(h->segs_d, h->flat_tmp, h->pi_p, nullptr, 1);
    h->pi_p_stale = false;
}

int ddrl_actor_versions_enable(ddrl_actor_t *h, int32_t n_slots, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(h->direct, "version store needs the direct-operand policy (shape outside the envelope)");
    DDRL_REQUIRE(n_slots >= 2 && n_slots <= VER_MAX_SLOTS, "n_slots outside [2, 2048]");
    DDRL_REQUIRE(h->n_slots == 0, "version store already enabled");
    ddrl::DeviceGuard g(h->device);
    const long long np = (long long)policy_slab_floats(h->Ld);   // a slot = the policy part of dslab (incl. the guard)
    hipError_t e = dev_alloc(&h->vslab, (size_t)np * n_slots + 2048);
    if (e == hipSuccess) e = dev_alloc(&h->slot_d, (size_t)h->max_rows + 64);
    // row lists: the planning launch's dense [tiles][32] (+ its parking space), then the env-step launch's own [n_slots][max_rows]
    const long long perm_dense = 32ll * (h->max_rows / 32 + n_slots) + h->max_rows + 64;
    if (e == hipSuccess) e = dev_alloc(&h->perm_d, (size_t)perm_dense + (size_t)n_slots * (size_t)h->max_rows);
    if (e == hipSuccess) e = dev_alloc(&h->vcnt_d, (size_t)VER_MAX_SLOTS);
    int ncu = 256;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    }
    // the forward's workgroup table: the coarsest split of the worst-case tile count (every live version leaves one partial tile) plus
    // one round of short workgroups (ver_split)
    const int col_tiles = (h->cfg.hidden2 + 31) / 32, g2 = col_tiles < 2 ? 1 : ((col_tiles + ANT - 1) / ANT < 2 ? 2 : (col_tiles + ANT - 1) / ANT);
    const long long vt_worst = h->max_rows / 32 + (n_slots < h->max_rows ? n_slots : h->max_rows);
    const long long vt_cap = vt_worst * g2 + 2 * ncu;
    if (e == hipSuccess) e = dev_alloc(&h->vtiles_d, (size_t)vt_cap + 16);
    if (e == hipSuccess) e = dev_alloc(&h->vs_d, 2);
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc failed in ddrl_actor_versions_enable (%d slots of %lld floats): %s", n_slots, np, hipGetErrorString(e));
        return DDRL_ERR_NOMEM;
    }
    hipStream_t s = ddrl::as_stream(stream);
    // (dev_alloc zero-fills: every env on slot 0, newest = 0) slot 0 = the weights the actor holds now
    h->vstride = np;
    h->n_slots = n_slots;
    h->wg_slots = 2 * ncu;
    if (const char *ev = getenv("DDRL_VER_WG_SLOTS")) {   // tests: a small "chip", so that small env counts walk the multi-round splits
        const int v = atoi(ev);
        if (v >= 1 && v <= 2 * ncu) h->wg_slots = v;
    }
    h->vt_cap = (int)vt_cap;
    h->perm2d_off = perm_dense;
    k_version_copy<<<256, 256, 0, s>>>(h->pi_d, h->vslab, h->vstride, h->vs_d, h->vstride / 4);
    h->steps_since_install = 1ll << 40;
    h->plan_fresh = false;
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_actor_versions_state(ddrl_actor_t *h, int32_t *slot_of_env_d, int32_t *state_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->n_slots > 0, "version store not enabled");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    if (slot_of_env_d) DDRL_HIP_CHECK(hipMemcpyAsync(slot_of_env_d, h->slot_d, (size_t)h->max_rows * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (state_h) {
        VerState vs;
        DDRL_HIP_CHECK(hipMemcpyAsync(&vs, h->vs_d, sizeof(vs), hipMemcpyDeviceToHost, s));
        DDRL_HIP_CHECK(hipStreamSynchronize(s));
        state_h[0] = vs.newest; state_h[1] = vs.live; state_h[2] = vs.n_tiles; state_h[3] = vs.err;
    }
    return DDRL_OK;
}

int ddrl_actor_act_versioned(ddrl_actor_t *h, const float *obs_d, const float *eps_d, int64_t n, int deterministic, int32_t horizon_steps,
                             float *act_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && obs_d != nullptr && act_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(h->n_slots > 0 && n == h->max_rows, "version store not enabled, or n != max_rows");
    DDRL_REQUIRE(deterministic || eps_d != nullptr, "eps is required for stochastic actions");
    DDRL_REQUIRE(h->cfg.act_dim <= 4 && horizon_steps >= 1, "act_dim <= 4 and horizon_steps >= 1");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const ddrl_sac1_config_t &c = h->cfg;
    DDRL_HIP_CHECK(hipMemcpyAsync(h->obs_d, obs_d, (size_t)n * c.obs_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    const bool versioned = ddrl_actor_internal_step_begin(h, horizon_steps) != 0;
    const int rc = ddrl_actor_internal_forward(h, n, stream, versioned ? 1 : 0);
    if (rc != DDRL_OK) return rc;
    FinishArgs f{};
    f.hp = h->hp_d; f.n = n; f.eps = deterministic ? nullptr : eps_d; f.act_out = act_d; f.act = c.act_dim; f.nt2 = (c.hidden2 + 31) / 32;
    f.deterministic = deterministic; f.scale = (float)c.act_scale;
    f.slot = versioned ? h->slot_d : nullptr; f.vstride = h->vstride;
    f.bmu = (versioned ? h->vslab : h->pi_d) + h->Ld.pi_bmu; f.bls = (versioned ? h->vslab : h->pi_d) + h->Ld.pi_bls;
    k_actor_finish<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(f);
    DDRL_LAUNCH_CHECK();
    if (versioned) ddrl_actor_internal_step_end(h, 1);   // k_actor_finish moves no env: the forward's plan still holds
    return DDRL_OK;
}

int ddrl_actor_versions_adopt(ddrl_actor_t *h, const uint8_t *ended_d, int64_t n, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->n_slots > 0 && ended_d != nullptr, "version store not enabled / NULL mask");
    DDRL_REQUIRE(n > 0 && n <= h->max_rows, "n outside [1, max_rows]");
    ddrl::DeviceGuard g(h->device);
    k_version_adopt<<<(unsigned)((n + 255) / 256), 256, 0, ddrl::as_stream(stream)>>>(h->slot_d, ended_d, n, h->vs_d);
    h->plan_fresh = false;
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_actor_get_weights(ddrl_actor_t *h, float *flat_pi_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && flat_pi_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    if (h->direct) {   // straight from the direct-layout policy
        k_pack<<<dim3(64, (unsigned)h->Ld.segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_dd, h->pi_d, flat_pi_d, nullptr, 0);
        DDRL_LAUNCH_CHECK();
        return DDRL_OK;
    }
    k_pack<<<dim3(64, (unsigned)h->L.segs.size()), 256, 0, ddrl::as_stream(stream)>>>(h->segs_d, h->pi_p, flat_pi_d, nullptr, 0);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_actor_act(ddrl_actor_t *h, const float *obs_d, const float *eps_d, int64_t n, int deterministic, float *act_d,
                   void *stream) {
    DDRL_REQUIRE(h != nullptr && obs_d != nullptr && act_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(n > 0 && n <= h->max_rows, "n outside [1, max_rows]");
    DDRL_REQUIRE(deterministic || eps_d != nullptr, "eps is required for stochastic actions");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const ddrl_sac1_config_t &c = h->cfg;
    const Layout &L = h->L;
    actor_refresh_row_major(h, s);
    L1Jobs l1{};
    l1.njobs = 1;
    l1.job[0] = L1Job{obs_d, nullptr, h->pi_p + L.pi_W1, h->pi_p + L.pi_b1, h->H1, nullptr, c.obs_dim, 0, (int)n, c.hidden1, h->ldh1, 0, 0};
    k_l1<<<dim3((c.hidden1 + 255) / 256, (unsigned)((n + L1_ROWS - 1) / L1_ROWS), 1), 256, 0, s>>>(l1);
    GemmJobs gj{};
    gemm_add(gj, gemm_fwd(h->H1, h->ldh1, h->pi_p + L.pi_W2, h->pi_p + L.pi_b2, h->H2, h->ldh2, (int)n, c.hidden1, c.hidden2));
    launch_gemm(gj, s);
    ActArgs aa{h->H2, net_pi(h->pi_p, L), eps_d, act_d, (int)n, c.hidden2, h->ldh2, c.act_dim, deterministic, (float)c.act_scale};
    k_rows_act<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(aa);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_actor_act_one(ddrl_actor_t *h, const float *obs_d, uint32_t noise_seed, uint64_t noise_ctr, int deterministic, float *act_d,
                       void *stream) {
    DDRL_REQUIRE(h != nullptr && obs_d != nullptr && act_d != nullptr, "NULL pointer");
    const ddrl_sac1_config_t &c = h->cfg;
    if (c.obs_dim > 64 || c.hidden1 > 512 || c.hidden2 > 512 || c.act_dim > 4) {
        ddrl::set_error("ddrl_actor_act_one: shape outside (obs 64, hidden 512, act 4): use ddrl_actor_act");
        return DDRL_ERR_UNSUPPORTED;
    }
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    if (!h->act1_part) {   // head partials of up to 32 workgroups + the ticket
        hipError_t e = dev_alloc(&h->act1_part, (size_t)32 * 16 + 16);
        if (e != hipSuccess) { ddrl::set_error("hipMalloc failed in ddrl_actor_act_one: %s", hipGetErrorString(e)); return DDRL_ERR_NOMEM; }
    }
    actor_refresh_row_major(h, s);
    ActOneArgs a{obs_d, net_pi(h->pi_p, h->L), act_d, h->act1_part, reinterpret_cast<unsigned int *>(h->act1_part + 32 * 16),
                 c.obs_dim, c.hidden1, c.hidden2, c.act_dim, deterministic, (float)c.act_scale, noise_seed, (unsigned long long)noise_ctr};
    k_act_one<<<(unsigned)((c.hidden2 + A1_COLS - 1) / A1_COLS), 256, 0, s>>>(a);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

}  // extern "C"

// ---- internal (env.hip: ddrl_rollout_step) ------------------------------------------------------------------------
// The policy forward of the fused rollout step: layer 1 + layer 2 + head partials of `n` observation rows that sit in
// the actor's own observation buffer, as one k_dfwd launch (n / 32 x ceil(h2 / 32) tiles).  The env-step kernel behind it
// turns the partials into actions (ddrl_pol::policy_row), steps the physics and appends the transitions to the ring.
#ifdef DDRL_STAMPS
unsigned long long *g_actor_st = nullptr;
#endif
// k_actor_fwd by its layer-1 step count: ns = 4 for obs_dim + 1 <= 8, one more step per two further input columns (obs_dim + 1 <= 13)
template <int OCC, bool VERSIONED>
static void launch_actor_fwd(int ns, unsigned grid, hipStream_t s, const ActFwdArgs &A) {
    if (ns == 4) k_actor_fwd<4, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else if (ns == 5) k_actor_fwd<5, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else if (ns == 6) k_actor_fwd<6, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
    else k_actor_fwd<7, OCC, VERSIONED><<<grid, 256, 0, s>>>(A);
}
int ddrl_actor_internal_forward(ddrl_actor *h, long long n, void *stream, int versioned) {
    DDRL_REQUIRE(h != nullptr && h->direct, "actor has no direct-operand policy (shape outside the envelope)");
    DDRL_REQUIRE(n > 0 && n % 32 == 0 && n <= h->max_rows, "n must be a positive multiple of 32 within max_rows");
    ddrl::DeviceGuard g(h->device);
    const ddrl_sac1_config_t &c = h->cfg;
    const Layout &L = h->Ld;
    const int nt2 = (c.hidden2 + 31) / 32;
    ActFwdArgs A{};
    A.W1 = h->pi_d + L.pi_W1; A.W2p = A.W1 + ((c.hidden1 + 31) & ~31) * 16;   // the k4-interleaved W2 follows the layer-1 block array
    A.b2 = h->pi_d + L.pi_b2; A.wmu = h->pi_d + L.pi_Wmu; A.wls = h->pi_d + L.pi_Wls; A.obs = h->obs_d; A.hp = h->hp_d;
    A.rows = (int)n; A.K = c.hidden1; A.Np = L.Np2; A.h2 = c.hidden2; A.d0 = c.obs_dim; A.act = c.act_dim; A.tiles_n = nt2;
    A.ngroups = (nt2 + ANT - 1) / ANT;   // 10 column tiles -> 2 workgroups of 5 per row tile
#ifdef DDRL_STAMPS
    A.st = g_actor_st;
#endif
    const int D1 = c.obs_dim + 1, ns = D1 <= 8 ? 4 : 4 + (D1 - 8 + 1) / 2;
    hipStream_t s = ddrl::as_stream(stream);
    if (versioned) {
        // envs grouped by the policy version they act on; a row tile = up to 32 envs of one version.  The launch covers the worst
        // case (every live version leaves one partial tile), surplus workgroups leave at once.
        DDRL_REQUIRE(h->n_slots > 0 && n == h->max_rows, "versioned forward: store not enabled, or n != max_rows");
        if (!h->plan_fresh) k_version_plan<<<1, 1024, 0, s>>>(h->slot_d, n, h->n_slots, h->perm_d, h->vtiles_d, h->vs_d, 0, nt2, h->wg_slots, h->vt_cap);
        h->plan_fresh = true;
        A.W1 = h->vslab + L.pi_W1; A.W2p = A.W1 + ((c.hidden1 + 31) & ~31) * 16;
        A.b2 = h->vslab + L.pi_b2; A.wmu = h->vslab + L.pi_Wmu; A.wls = h->vslab + L.pi_Wls;
        A.vtiles = h->vtiles_d; A.perm = h->perm_d; A.vs = h->vs_d; A.vstride = h->vstride; A.vt_max = h->vt_cap;
        const unsigned vgrid = (unsigned)h->vt_cap;   // (the plan's workgroup count is at most that; the rest leave at once)
        launch_actor_fwd<2, true>(ns, vgrid, s, A);
        DDRL_LAUNCH_CHECK();
        return DDRL_OK;
    }
    const unsigned grid = (unsigned)(n / 32) * A.ngroups;
    if (grid > 256) launch_actor_fwd<2, false>(ns, grid, s, A);   // more than one workgroup per CU: the two-per-CU register budget
    else launch_actor_fwd<1, false>(ns, grid, s, A);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

// ---- the version store's host state, for the callers that drive a vector step themselves (ddrl_actor_act_versioned above; env.hip's
// fused steps).  One vector step = begin, the forward (ddrl_actor_internal_forward with begin's answer), the caller's own launch, end.
// begin: is this step versioned — the store is enabled and fewer than `horizon` steps have passed since the last install?  Counts the
// step (on a store).  The caller makes it BEFORE the step's launches, and behind whatever may install (ddrl_dqn_internal_repack).
int ddrl_actor_internal_step_begin(ddrl_actor *h, long long horizon) {
    if (h->n_slots == 0) return 0;
    const bool versioned = h->steps_since_install < horizon;
    h->steps_since_install += 1;
    return versioned ? 1 : 0;
}
// end: the caller's launch behind the forward returned DDRL_OK; `planned` = the forward's tables match the slots it left (its tail planned
// for the envs it moved, or it moved none).  Not called on an error return: plan_fresh stays as the forward left it.
void ddrl_actor_internal_step_end(ddrl_actor *h, int planned) { h->plan_fresh = planned != 0; }

// slots of the version store (0: not enabled)
int ddrl_actor_internal_versions(ddrl_actor *h) { return h ? h->n_slots : 0; }

// the configuration and the device, for the handle-fed evaluation entry points (eval3.hip; declared in eval_episodes.h)
int ddrl_actor_internal_config(ddrl_actor *h, ddrl_sac1_config_t *cfg_out, int *device_out) {
    if (!h) return DDRL_ERR_BAD_ARG;
    *cfg_out = h->cfg; *device_out = h->device;
    return DDRL_OK;
}

ddrl_actor_rollout_view ddrl_actor_internal_view(ddrl_actor *h) {
    ddrl_actor_rollout_view v{};
    if (!h || !h->direct) return v;
    v.ok = 1; v.obs = h->obs_d; v.hp = h->hp_d; v.bmu = h->pi_d + h->Ld.pi_bmu; v.bls = h->pi_d + h->Ld.pi_bls;
    v.ver = ddrl_version_view{h->n_slots, h, h->slot_d, h->vs_d, h->vstride, h->vcnt_d, h->perm_d, h->perm2d_off, h->vtiles_d, h->vt_cap, h->wg_slots};
    v.vbmu = h->n_slots ? h->vslab + h->Ld.pi_bmu : nullptr; v.vbls = h->n_slots ? h->vslab + h->Ld.pi_bls : nullptr;
    v.obs_dim = h->cfg.obs_dim; v.act = h->cfg.act_dim; v.nt2 = (h->cfg.hidden2 + 31) / 32; v.max_rows = h->max_rows;
    v.scale = (float)h->cfg.act_scale; v.device = h->device;
    return v;
}
