// Replay ring buffer on HBM: store (ring append with wrap), bit-exact NumPy-compatible MT19937
// uniform index sampler, row gather.  Replaces class ReplayBuffer of the reference
// (example/dsac.py:14-48, algos/sac1/sac1.py:28-63, algos/dqn/train.py:37-76).
//
// Data layout: the reference's own struct-of-arrays — obs1[N,obs] obs2[N,obs] acts[N,act] (or
// [N]) rews[N] done[N], float32, row-major — so the rings are byte-compatible with the .npy
// checkpoint of algos/dqn/train.py:82-90.  Cursor/counters and the MT19937 state live in a
// device-side RingState so that store/sample kernels can be captured in a hipGraph and replayed
// without host-side argument patching.
#include "replay_device.h"

using namespace ddrl_replay_dev;

namespace {

// ------------------------------------------------------------------------------------------
// store: n sequential ReplayBuffer.store() calls (example/dsac.py:29-37)
// grid = (blocks, 5 arrays).  Rows i < n - capacity would be overwritten later in the same
// batch, so they are skipped; every remaining destination row is unique.
// ------------------------------------------------------------------------------------------
struct StoreSrc {
    const float *a[MAX_ARRAYS];
};
__global__ void __launch_bounds__(256) k_store(RingState *st, RingPtrs ring, StoreSrc srcs, long long n) {
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = st->ptr;
    __syncthreads();
    const long long ptr = s_ptr, cap = ring.capacity;
    const long long skip = n > cap ? n - cap : 0;
    const int which = blockIdx.y;
    const float *src = srcs.a[which];
    float *dst = ring.a[which];
    const int width = ring.w[which];
    // rows [skip, n) land on distinct ring rows; ptr < cap and i - skip < cap, so one conditional
    // subtraction replaces the modulo.  32-bit index arithmetic whenever the batch allows it
    // (64-bit div/mod per element made this kernel 10x slower than the copy it is).
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ring.kind[which] == 1) {
        // compact array: 16 float32 in -> 16 bytes out per lane (4 when the row is not a whole number of 16-element groups);
        // a value that does not survive the round trip (not an integer in [0, 255], NaN) raises the sticky error — the ring
        // is opt-in for integer-valued pixels and must never change a value silently
        unsigned char *d8 = reinterpret_cast<unsigned char *>(dst);
        const int G = ((width & 15) == 0 && aligned16(dst, src)) ? 16 : 1;
        const int wg = width / G;
        const long long total = (n - skip) * wg;
        const long long base_row = (ptr + skip) % cap;
        bool bad = false;
        for (long long e = t0; e < total; e += stride) {
            const long long ri = e / wg;
            const int c = (int)(e - ri * wg);
            long long row = base_row + ri;
            if (row >= cap) row -= cap;
            const long long so = (skip + ri) * width + (long long)c * G, dof = row * width + (long long)c * G;
            if (G == 16) {
                const float4 *s4 = reinterpret_cast<const float4 *>(src + so);
                const float4 v0 = s4[0], v1 = s4[1], v2 = s4[2], v3 = s4[3];
                const float f[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
                unsigned u[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 16; ++k) u[k >> 2] |= to_u8(f[k], bad) << (8 * (k & 3));
                *reinterpret_cast<uint4 *>(d8 + dof) = make_uint4(u[0], u[1], u[2], u[3]);
            } else {
                d8[dof] = (unsigned char)to_u8(src[so], bad);
            }
        }
        if (bad) st->error = DDRL_ERR_NOT_REPRESENTABLE;
    } else {
    const bool v4 = (width & 3) == 0 && aligned16(dst, src);
    const int wv = v4 ? width >> 2 : width;  // row width in vector elements
    const long long total = (n - skip) * wv;
    const long long base_row = (ptr + skip) % cap;  // ring row of source row `skip` (skip = n - cap is unbounded: reduce it once per thread)
    if (total < 0x7fffffffll) {
        const unsigned tot = (unsigned)total, uw = (unsigned)wv, ustride = (unsigned)stride;
        for (unsigned e = (unsigned)t0; e < tot; e += ustride) {
            const unsigned ri = e / uw, c = e - ri * uw;
            long long row = base_row + ri;  // base_row < cap and ri < cap: one conditional subtraction is the modulo
            if (row >= cap) row -= cap;
            const long long so = (long long)(skip + ri) * wv + c, dof = row * wv + c;
            if (v4) reinterpret_cast<float4 *>(dst)[dof] = reinterpret_cast<const float4 *>(src)[so];
            else dst[dof] = src[so];
        }
    } else {
        for (long long e = t0; e < total; e += stride) {
            const long long ri = e / wv;
            const int c = (int)(e - ri * wv);
            const long long row = (base_row + ri) % cap;
            const long long so = (skip + ri) * wv + c, dof = row * wv + c;
            if (v4) reinterpret_cast<float4 *>(dst)[dof] = reinterpret_cast<const float4 *>(src)[so];
            else dst[dof] = src[so];
        }
    }
    }
    // last block to finish advances the cursor (every block has read st->ptr before its ticket)
    __syncthreads();
    if (threadIdx.x == 0) ring_commit(st, ring, ptr, n);
}

// ------------------------------------------------------------------------------------------
// masked store: store() for the rows with mask != 0, in row order — the n-step rollout stores a
// window only for the envs whose deque is full (algos/sac1/sac_ray.py:243-246), so the number of
// rows is known on the device only.  Pass 1 (one workgroup) ranks the selected rows, pass 2 copies.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mask_scan(const uint8_t *__restrict__ mask, long long n, int *__restrict__ rank) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (long long i0 = 0; i0 < n; i0 += 256) {
        const long long i = i0 + tid;
        const bool f = i < n && mask[i] != 0;
        const unsigned long long b = __ballot(f);
        const int pre = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wave] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { woff += (w < wave) ? s_w[w] : 0; tot += s_w[w]; }
        if (i < n) rank[i] = f ? base + woff + pre : -1;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) rank[n] = base;
}
__global__ void __launch_bounds__(256) k_store_masked(RingState *st, RingPtrs ring, StoreSrc srcs, const int *__restrict__ rank, long long n) {
    __shared__ long long s_ptr;
    if (threadIdx.x == 0) s_ptr = st->ptr;
    __syncthreads();
    const long long ptr = s_ptr, cap = ring.capacity;
    const long long total = rank[n];
    const long long skip = total > cap ? total - cap : 0;  // ranks below `skip` would be overwritten later in this batch
    const int which = blockIdx.y;
    const float *src = srcs.a[which];
    float *dst = ring.a[which];
    const int width = ring.w[which];
    const bool v4 = (width & 3) == 0 && aligned16(dst, src);
    const int wv = v4 ? width >> 2 : width;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n * wv; e += stride) {
        const long long ri = e / wv;
        const int c = (int)(e - ri * wv);
        const long long r = rank[ri];
        if (r < skip) continue;  // not selected (-1) or overwritten within the batch
        const long long row = (ptr + r) % cap;
        if (v4) reinterpret_cast<float4 *>(dst)[row * wv + c] = reinterpret_cast<const float4 *>(src)[e];
        else dst[row * wv + c] = src[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) ring_commit(st, ring, ptr, total);
}

// ------------------------------------------------------------------------------------------
// ring append: store() of every row ring `src` holds, oldest first, into ring `dst`; then `src` is emptied.  The row count is
// src's own `size`, read on the device: a staging ring filled by masked stores (k_store_masked, the fused n-step step's cursor
// commit) is committed without the host ever learning how many rows it held, and a captured node follows the counts at replay.
// grid = (blocks, n_arr), k_store's float path with a second ring in place of the flat source: source row i is
// (src.ptr - src.size + i) mod src.capacity, rows i < size - dst.capacity are skipped as in k_store.
// Ticket: dst's own done_counter, through ring_commit — the launch is one more store into dst, and nothing else may store into
// dst while it runs.  Every block reads the three cursors before its ticket; the block that draws the last ticket commits dst
// and only then zeroes src's cursor, so no block can see the emptied source.  No grid barrier, no spin.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_append_ring(RingState *st, RingPtrs ring, RingState *sst, RingPtrs sring) {
    __shared__ long long s_c[3];
    if (threadIdx.x == 0) { s_c[0] = st->ptr; s_c[1] = sst->ptr; s_c[2] = sst->size; }
    __syncthreads();
    const long long ptr = s_c[0], cap = ring.capacity, scap = sring.capacity;
    const long long n = s_c[2];
    const long long skip = n > cap ? n - cap : 0;
    const int which = blockIdx.y;
    const float *src = sring.a[which];
    float *dst = ring.a[which];
    const int width = ring.w[which];
    const bool v4 = (width & 3) == 0 && aligned16(dst, src);
    const int wv = v4 ? width >> 2 : width;
    const long long total = (n - skip) * wv;
    const long long base_row = (ptr + skip) % cap;                       // ring row of the first row that lands
    const long long sbase = ((s_c[1] - n + skip) % scap + scap) % scap;  // source row of it: oldest row + skip (n <= scap, ptr < scap)
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (scap * wv < 0x7fffffffll) {   // total <= scap * wv: decided by the capacity, the count is not known where the grid is sized
        const unsigned tot = (unsigned)total, uw = (unsigned)wv, ustride = (unsigned)stride;
        for (unsigned e = (unsigned)t0; e < tot; e += ustride) {
            const unsigned ri = e / uw, c = e - ri * uw;
            long long row = base_row + ri, srow = sbase + ri;   // ri < min(cap, scap): one conditional subtraction is the modulo
            if (row >= cap) row -= cap;
            if (srow >= scap) srow -= scap;
            const long long so = srow * wv + c, dof = row * wv + c;
            if (v4) reinterpret_cast<float4 *>(dst)[dof] = reinterpret_cast<const float4 *>(src)[so];
            else dst[dof] = src[so];
        }
    } else {
        for (long long e = t0; e < total; e += stride) {
            const long long ri = e / wv;
            const int c = (int)(e - ri * wv);
            const long long row = (base_row + ri) % cap, srow = (sbase + ri) % scap;
            const long long so = srow * wv + c, dof = row * wv + c;
            if (v4) reinterpret_cast<float4 *>(dst)[dof] = reinterpret_cast<const float4 *>(src)[so];
            else dst[dof] = src[so];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && ring_commit(st, ring, ptr, n)) { sst->ptr = 0; sst->size = 0; }
}

// ------------------------------------------------------------------------------------------
// MT19937 (NumPy legacy RandomState): seed == init_genrand
// ------------------------------------------------------------------------------------------
__global__ void k_mt_seed(RingState *st, uint32_t seed) {
    // sequential recurrence; 624 steps on one lane (a few microseconds, off the hot path)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint32_t x = seed;
        st->mt_key[0] = x;
        for (int i = 1; i < MT_N; ++i) {
            x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
            st->mt_key[i] = x;
        }
        st->mt_pos = MT_N;
    }
}

__global__ void __launch_bounds__(SAMPLE_THREADS) k_sample(RingState *st, RingPtrs ring, BatchPtrs out, int B,
                                                           long long *idx_out, int fuse_gather) {
    sample_block(st, ring, out, B, idx_out, fuse_gather);
}

// large draws that are gathered by a launch of their own: the 640-thread form of the sampler (>= 624: a whole state block per pass)
__global__ void __launch_bounds__(640) k_sample_wide(RingState *st, RingPtrs ring, BatchPtrs out, int B, long long *idx_out) {
    sample_block<640>(st, ring, out, B, idx_out, 0);
}

// n-step fold of whole windows that already lie on the device in batch order (the host `Cache` path: a sampled window batch), and the
// fold-gather for indices drawn by a launch of their own (batches beyond the one-workgroup sampler): grid-stride forms of the
// sampler's nstep_fold_gather.
struct FoldSrc {
    const float *o, *a, *r, *d;
    int Ln, od, ad;
    float gamma;
};
__global__ void __launch_bounds__(256) k_nstep_fold(FoldSrc w, BatchPtrs out, int B) {
    nstep_fold_gather(w.o, w.a, w.r, w.d, w.Ln, w.od, w.ad, w.gamma, out.a[0], out.a[1], out.a[2], out.a[3], out.a[4], (unsigned)B,
                      [](unsigned b) { return b; }, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}
__global__ void __launch_bounds__(256) k_nstep_gather(FoldSrc w, BatchPtrs out, const long long *__restrict__ idx, int B) {
    nstep_fold_gather(w.o, w.a, w.r, w.d, w.Ln, w.od, w.ad, w.gamma, out.a[0], out.a[1], out.a[2], out.a[3], out.a[4], (unsigned)B,
                      [=](unsigned b) { return idx[b]; }, blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

// Stand-alone gather for large rows (the dqn pixel shape: 2 x 112 896 B per index): one
// workgroup per (row, array) so that >= B * n_arr workgroups fill the chip; each lane keeps four
// independent 16-B loads in flight (HBM-bound random-row gather).
__global__ void __launch_bounds__(256) k_gather(RingPtrs ring, BatchPtrs out, const long long *__restrict__ idx,
                                                int B) {
    const int b = blockIdx.x, j = blockIdx.y;
    const long long row = idx[b];
    const int tid = threadIdx.x;
    const int width = ring.w[j];
    const float *src = ring.a[j] + row * width;
    float *dst = out.a[j] + (long long)b * width;
    if (ring.kind[j] == 1) {
        // compact array: one dword (four pixels) in -> one float4 out per lane, so that a wave's store instruction writes 1 KB of
        // consecutive bytes (the first cut — a 16-byte load and four float4 stores at a 64-byte lane stride — wrote partial lines:
        // 2.9 TB/s); eight loads in flight per lane.  The batch written is 4x the bytes read: the stores set the rate.
        const unsigned char *s8 = reinterpret_cast<const unsigned char *>(ring.a[j]) + row * width;
        if ((width & 3) == 0 && aligned16(out.a[j], ring.a[j])) {
            const int w4 = width >> 2;
            const unsigned *s32 = reinterpret_cast<const unsigned *>(s8);
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            auto cvt = [](unsigned u) { return make_float4((float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u), (float)(u >> 24)); };
            int e = tid;
            for (; e + 7 * 256 < w4; e += 8 * 256) {
                unsigned u[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) u[k] = s32[e + 256 * k];
#pragma unroll
                for (int k = 0; k < 8; ++k) d4[e + 256 * k] = cvt(u[k]);
            }
            for (; e < w4; e += 256) d4[e] = cvt(s32[e]);
        } else {
            for (int e = tid; e < width; e += 256) dst[e] = (float)s8[e];
        }
        return;
    }
    if ((width & 3) == 0 && aligned16(out.a[j], ring.a[j])) {
        const int w4 = width >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        int e = tid;
        for (; e + 3 * 256 < w4; e += 4 * 256) {
            const float4 a0 = s4[e], a1 = s4[e + 256], a2 = s4[e + 512], a3 = s4[e + 768];
            d4[e] = a0; d4[e + 256] = a1; d4[e + 512] = a2; d4[e + 768] = a3;
        }
        for (; e < w4; e += 256) d4[e] = s4[e];
    } else {
        for (int e = tid; e < width; e += 256) dst[e] = src[e];
    }
}

// Gather for many SMALL rows (the block a shard owner draws for a whole step: 2^18 rows of 32 B): one lane per 16-B
// (or 4-B) element, all rows of an array in one grid-stride sweep — k_gather's workgroup-per-row would be launch-bound.
__global__ void __launch_bounds__(256) k_gather_small(RingPtrs ring, BatchPtrs out, const long long *__restrict__ idx, int B) {
    const int j = blockIdx.y, width = ring.w[j];
    if (ring.kind[j] == 1) {
        const unsigned char *r8 = reinterpret_cast<const unsigned char *>(ring.a[j]);
        const unsigned total = (unsigned)B * (unsigned)width;
        for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
            const unsigned b = e / (unsigned)width, c = e - b * (unsigned)width;
            out.a[j][e] = (float)r8[idx[b] * width + c];
        }
        return;
    }
    const bool v4 = (width & 3) == 0 && aligned16(out.a[j], ring.a[j]);  // packed blocks start arrays at any float offset
    const unsigned wv = v4 ? width >> 2 : width, total = (unsigned)B * wv;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned b = e / wv, c = e - b * wv;
        const long long so = idx[b] * wv + c;
        if (v4) reinterpret_cast<float4 *>(out.a[j])[e] = reinterpret_cast<const float4 *>(ring.a[j])[so];
        else out.a[j][e] = ring.a[j][so];
    }
}

// Ring rows [row0, row0 + nrows) of one array as float32 (export) or from float32 (import): the .npy checkpoint of
// algos/dqn/train.py:82-108 is float32 whatever the storage kind.
__global__ void __launch_bounds__(256) k_rows_export(RingPtrs ring, int j, long long row0, long long nrows, float *__restrict__ out) {
    const long long total = nrows * ring.w[j], off = row0 * ring.w[j];
    const unsigned char *r8 = reinterpret_cast<const unsigned char *>(ring.a[j]);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
        out[e] = ring.kind[j] == 1 ? (float)r8[off + e] : ring.a[j][off + e];
}
__global__ void __launch_bounds__(256) k_rows_import(RingState *st, RingPtrs ring, int j, long long row0, long long nrows, const float *__restrict__ src) {
    const long long total = nrows * ring.w[j], off = row0 * ring.w[j];
    unsigned char *r8 = reinterpret_cast<unsigned char *>(ring.a[j]);
    bool bad = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const float f = src[e];
        if (ring.kind[j] == 1) r8[off + e] = (unsigned char)to_u8(f, bad);
        else ring.a[j][off + e] = f;
    }
    if (bad) st->error = DDRL_ERR_NOT_REPRESENTABLE;
}

__global__ void k_set_feed(RingState *st, Feed f) { st->feed = f; }
__global__ void k_take_error(RingState *st, int *out) { *out = st->error; st->error = 0; }
__global__ void k_add_samples(RingState *st, long long inc) { st->sample_times += inc; }

__global__ void k_set_counts(RingState *st, long long ptr, long long size, long long steps, long long samples) {
    st->ptr = ptr; st->size = size; st->steps = steps; st->sample_times = samples;
    st->done_counter = 0; st->error = 0;
}

}  // namespace

struct ddrl_replay {
    int device;
    RingPtrs ring;
    RingState *state;    // device
    long long *idx_buf;  // device scratch for indices when the caller passes none
    long long idx_cap;
    // host mirror of the counters: exact while every store/sample goes through this API
    // eagerly; refreshed from the device by ddrl_replay_counts (graph replays run ahead of it)
    long long h_ptr, h_size, h_steps, h_samples;
    bool h_dirty;        // a masked store (row count known on the device only) has run since the last refresh
    int *rank_buf;       // device scratch of the masked store
    long long rank_cap;
    uint32_t flags;
    bool feed_on;        // a feed plan is attached (ddrl_replay_set_feed): the sampler may be handed remote batches
};

static int refresh_counts(ddrl_replay *h, hipStream_t s) {
    RingState tmp;
    DDRL_HIP_CHECK(hipMemcpyAsync(&tmp, h->state, offsetof(RingState, mt_key), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    h->h_ptr = tmp.ptr; h->h_size = tmp.size; h->h_steps = tmp.steps; h->h_samples = tmp.sample_times;
    h->h_dirty = false;
    if (tmp.error != 0) {
        // a sampler that ran inside a graph / another kernel could not report to its caller: the first host call that
        // looks at the ring does (and clears the flag, so that the caller can repair the plan and go on)
        DDRL_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char *>(h->state) + offsetof(RingState, error), 0, sizeof(int), s));
        DDRL_HIP_CHECK(hipStreamSynchronize(s));
        if (tmp.error == DDRL_ERR_EMPTY_BUFFER) {
            ddrl::set_error("high <= 0");  // the sampler drew from an empty ring (the reference's ValueError)
            return DDRL_ERR_EMPTY_BUFFER;
        }
        if (tmp.error == DDRL_ERR_NOT_REPRESENTABLE) {
            ddrl::set_error("a value stored into a compact (uint8) ring array was not an integer in [0, 255]: the ring holds a clamped/truncated value there");
            return DDRL_ERR_NOT_REPRESENTABLE;
        }
        ddrl::set_error("a feed-plan entry was out of range (wrong batch size, region or batch index): that update trained on a stale input set");
        return tmp.error;
    }
    return DDRL_OK;
}

ddrl_replay_dev::SamplerView ddrl_replay_sampler_view(ddrl_replay_t *h, bool fold, float gamma) {
    ddrl_replay_dev::SamplerView v{h->state, h->ring, h->device};
    v.ring.fold = fold ? 1 : 0;
    v.ring.gamma = fold ? gamma : 0.f;
    return v;
}
// floats gathered per accepted index: the whole row of a plain view; o[0], o[Ln], a[0] and the 2 Ln reward / done scalars of a fold view
static long long view_floats(const RingPtrs &r) {
    if (r.fold) {
        const long long Ln = r.w[2];
        return 2 * (r.w[0] / (Ln + 1)) + r.w[1] / Ln + 2 * Ln;
    }
    long long t = 0;
    for (int j = 0; j < r.n_arr; ++j) t += r.w[j];
    return t;
}
static bool has_compact(const ddrl_replay *h) {
    for (int j = 0; j < h->ring.n_arr; ++j) if (h->ring.kind[j]) return true;
    return false;
}
bool ddrl_replay_can_fuse(ddrl_replay_t *h, const ddrl_replay_dev::SamplerView &v, int64_t batch) {
    const long long bytes = batch * view_floats(v.ring) * (long long)sizeof(float);
    return batch <= MAX_FUSED_BATCH && bytes <= MAX_FUSED_BYTES && (h->h_size > 0 || h->feed_on);
}
// {o[(Ln+1) obs], a[Ln act], r[Ln], d[Ln]}, all float32; obs_dim / act_dim <= 0: whatever the widths give
bool ddrl_replay_is_window_ring(ddrl_replay_t *h, int obs_dim, int act_dim) {
    const RingPtrs &r = h->ring;
    if (r.n_arr != 4 || has_compact(h)) return false;
    const int Ln = r.w[2];
    if (Ln < 1 || r.w[3] != Ln || r.w[0] % (Ln + 1) != 0 || r.w[1] % Ln != 0) return false;
    return (obs_dim <= 0 || r.w[0] == (Ln + 1) * obs_dim) && (act_dim <= 0 || r.w[1] == Ln * act_dim);
}
void ddrl_replay_note_sample(ddrl_replay_t *h) { h->h_samples += h->ring.samples_inc; }
void ddrl_replay_note_store(ddrl_replay_t *h, long long n) {  // host mirror bookkeeping for n stores (ddrl_replay_store_ex, ddrl_rollout_step)
    h->h_ptr = (h->h_ptr + n) % h->ring.capacity;
    h->h_size = (h->h_size + n > h->ring.capacity) ? h->ring.capacity : h->h_size + n;
    h->h_steps += n * h->ring.steps_inc;
}
void ddrl_replay_note_masked_store(ddrl_replay_t *h) { h->h_dirty = true; }   // as ddrl_replay_store_masked_ex leaves it (ddrl_rollout_step_nstep)

static int require_rows(ddrl_replay *h, hipStream_t s);
// Internal (dqn.hip: the DQN / SQN loop's sampler draws AND gathers in a launch of its own kernels): the host side of such a draw.
// Is a feed plan attached (that sampler does not follow one); are there rows to draw from (DDRL_ERR_EMPTY_BUFFER as every draw reports it)
bool ddrl_replay_internal_has_feed(ddrl_replay_t *h) { return h->feed_on; }
int ddrl_replay_internal_require_rows(ddrl_replay_t *h, void *stream) {
    ddrl::DeviceGuard g(h->device);
    return require_rows(h, ddrl::as_stream(stream));
}

// A draw needs rows: the mirror may lag behind graph replays / masked stores, so ask the device before reporting empty
static int require_rows(ddrl_replay *h, hipStream_t s) {
    if (h->h_size <= 0 || h->h_dirty) {
        int rc = refresh_counts(h, s);
        if (rc != DDRL_OK) return rc;
        if (h->h_size <= 0) {
            ddrl::set_error("high <= 0");  // message of the reference's ValueError
            return DDRL_ERR_EMPTY_BUFFER;
        }
    }
    return DDRL_OK;
}

// Device scratch that holds at least `need` elements (its old contents are not kept): the launches that read the old block are waited for
template <class T>
static int grow(T *&buf, long long &cap, long long need, hipStream_t s) {
    if (need <= cap) return DDRL_OK;
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    DDRL_HIP_CHECK(hipMalloc(&buf, need * sizeof(T)));
    cap = need;
    return DDRL_OK;
}

// The source table of a store and its widest row in vector elements (the grid's size); false: a source is NULL
static bool store_srcs(const ddrl_replay *h, const float *const *src_h, StoreSrc &srcs, int &widest) {
    srcs = StoreSrc{};
    widest = 1;
    for (int j = 0; j < h->ring.n_arr; ++j) {
        if (src_h[j] == nullptr) return false;
        srcs.a[j] = src_h[j];
        const int wv = (h->ring.w[j] & 3) == 0 ? h->ring.w[j] / 4 : h->ring.w[j];
        if (wv > widest) widest = wv;
    }
    return true;
}

static int launch_gather(ddrl_replay *h, const long long *idx, int64_t B, BatchPtrs out, hipStream_t s) {
    int widest = 1;
    for (int j = 0; j < h->ring.n_arr; ++j) widest = h->ring.w[j] > widest ? h->ring.w[j] : widest;
    if (widest <= 64 && B >= 4096) {  // many small rows
        long long blocks = (B * ((widest & 3) == 0 ? widest / 4 : widest) + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        k_gather_small<<<dim3((unsigned)blocks, (unsigned)h->ring.n_arr), 256, 0, s>>>(h->ring, out, idx, (int)B);
        DDRL_LAUNCH_CHECK();
        return DDRL_OK;
    }
    k_gather<<<dim3((unsigned)B, (unsigned)h->ring.n_arr), 256, 0, s>>>(h->ring, out, idx, (int)B);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

static int fold_grid(int64_t batch, int od) {
    long long blocks = (batch * ((od & 3) == 0 ? od / 4 : od) + 255) / 256;
    return (int)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}

// The one place a draw is launched: `batch` indices of view `v` (a plain ring, or a window ring's fold view), gathered into `out`
// (NULL: indices only) and written to `idx` (nullable).
//   draw + gather in one workgroup (k_sample, fuse 1): a plain batch <= MAX_FUSED_BATCH rows and <= MAX_FUSED_BYTES, a folded one
//     <= MAX_FUSED_BATCH rows whatever its bytes.  The only form that follows a feed plan (the entry points refuse the others then).
//   otherwise: the draw — 640-thread form from 2048 indices on — into `idx` or the handle's scratch, then the view's gather launch.
// The thresholds were measured one by one: they are not meant to agree.
static int launch_draw(ddrl_replay *h, const SamplerView &v, int64_t batch, const BatchPtrs *out, long long *idx, hipStream_t s) {
    const RingPtrs &r = v.ring;
    const bool fuse = out && batch <= MAX_FUSED_BATCH && (r.fold || batch * view_floats(r) * (long long)sizeof(float) <= MAX_FUSED_BYTES);
    const BatchPtrs o = out ? *out : BatchPtrs{};
    if (!fuse && !idx) {
        const int rc = grow(h->idx_buf, h->idx_cap, batch, s);
        if (rc != DDRL_OK) return rc;
        idx = h->idx_buf;
    }
    if (!fuse && batch >= 2048) k_sample_wide<<<1, 640, 0, s>>>(v.state, r, o, (int)batch, idx);
    else k_sample<<<1, SAMPLE_THREADS, 0, s>>>(v.state, r, o, (int)batch, idx, fuse ? 1 : 0);
    DDRL_LAUNCH_CHECK();
    h->h_samples += r.samples_inc;
    if (fuse || !out) return DDRL_OK;
    if (!r.fold) return launch_gather(h, idx, batch, o, s);
    const int Ln = r.w[2], od = r.w[0] / (Ln + 1), ad = r.w[1] / Ln;
    const FoldSrc w{r.a[0], r.a[1], r.a[2], r.a[3], Ln, od, ad, r.gamma};
    k_nstep_gather<<<fold_grid(batch, od), 256, 0, s>>>(w, o, idx, (int)batch);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_replay_draw(ddrl_replay_t *h, const SamplerView &v, int64_t batch, const BatchPtrs &out, int64_t *idx_d, void *stream) {
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    if (h->feed_on) {   // the plan decides per call: a fed batch is copied, a -1 entry draws (an empty ring: the sticky error)
        DDRL_REQUIRE(ddrl_replay_can_fuse(h, v, batch), "a feed plan is attached: the batch must fit the one-workgroup sampler");
    } else {
        const int rc = require_rows(h, s);
        if (rc != DDRL_OK) return rc;
    }
    return launch_draw(h, v, batch, &out, reinterpret_cast<long long *>(idx_d), s);
}

// `count` consecutive sample_batch(batch) calls through view `v` consume the index stream exactly like one draw of batch * count
// (the ring size cannot change in between: nothing else is ordered between them on this stream); the counter takes the other calls
static int sample_many(ddrl_replay *h, const SamplerView &v, int64_t batch, int64_t count, float *const *out_h, void *stream) {
    BatchPtrs out;
    DDRL_REQUIRE(batch_ptrs(out, out_h, v.ring.fold ? 5 : v.ring.n_arr), "NULL output pointer");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    int rc = require_rows(h, s);
    if (rc == DDRL_OK) rc = launch_draw(h, v, batch * count, &out, nullptr, s);
    if (rc != DDRL_OK || count == 1) return rc;
    k_add_samples<<<1, 1, 0, s>>>(h->state, (count - 1) * h->ring.samples_inc);
    DDRL_LAUNCH_CHECK();
    h->h_samples += (count - 1) * h->ring.samples_inc;
    return DDRL_OK;
}

// argument checks shared by the two folded draws; `what` names the caller in the refusal
static int check_sample_nstep(ddrl_replay *h, int64_t rows, const char *what) {
    if (!ddrl_replay_is_window_ring(h, 0, 0)) {
        ddrl::set_error("%s needs an n-step window ring {o[(Ln+1) obs], a[Ln act], r[Ln], d[Ln]} of float32 arrays", what);
        return DDRL_ERR_UNSUPPORTED;
    }
    const int Ln = h->ring.w[2], od = h->ring.w[0] / (Ln + 1), ad = h->ring.w[1] / Ln;
    DDRL_REQUIRE(rows * (od > ad ? od : ad) < 0x7fffffffll, "batch * max(obs_dim, act_dim) must be < 2^31");
    return DDRL_OK;
}

extern "C" {

int ddrl_replay_create_ex(ddrl_replay_t **out, int device, int64_t capacity, int32_t n_arrays, const int32_t *widths_h,
                          int64_t steps_inc, int64_t samples_inc) {
    return ddrl_replay_create_typed(out, device, capacity, n_arrays, widths_h, nullptr, steps_inc, samples_inc);
}

int ddrl_replay_create_typed(ddrl_replay_t **out, int device, int64_t capacity, int32_t n_arrays, const int32_t *widths_h,
                             const uint8_t *kinds_h, int64_t steps_inc, int64_t samples_inc) {
    DDRL_REQUIRE(out != nullptr && widths_h != nullptr, "NULL pointer");
    for (int j = 0; kinds_h && j < n_arrays && j < MAX_ARRAYS; ++j) DDRL_REQUIRE(kinds_h[j] <= 1, "array kind must be 0 (float32) or 1 (uint8)");
    DDRL_REQUIRE(capacity > 0 && capacity <= 0xFFFFFFFFll, "capacity must be in [1, 2^32-1]");
    DDRL_REQUIRE(n_arrays >= 1 && n_arrays <= MAX_ARRAYS, "n_arrays must be in [1, 6]");
    for (int j = 0; j < n_arrays; ++j) DDRL_REQUIRE(widths_h[j] > 0, "row widths must be positive");
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_replay *h = new ddrl_replay();
    memset(h, 0, sizeof(*h));
    h->device = device;
    h->ring.capacity = capacity;
    h->ring.n_arr = n_arrays;
    h->ring.steps_inc = steps_inc > 0 ? steps_inc : 1;
    h->ring.samples_inc = samples_inc > 0 ? samples_inc : 1;
    hipError_t e = hipSuccess;
    for (int j = 0; j < n_arrays && e == hipSuccess; ++j) {
        h->ring.w[j] = widths_h[j];
        h->ring.kind[j] = kinds_h ? kinds_h[j] : 0;
        e = hipMalloc(&h->ring.a[j], (size_t)capacity * widths_h[j] * (h->ring.kind[j] ? 1 : sizeof(float)));
    }
    if (e == hipSuccess) e = hipMalloc(&h->state, sizeof(RingState));
    h->idx_cap = 1 << 16;
    if (e == hipSuccess) e = hipMalloc(&h->idx_buf, h->idx_cap * sizeof(long long));
    if (e != hipSuccess) {
        ddrl::set_error("hipMalloc failed for a ring of %lld rows x %lld floats: %s", (long long)capacity, view_floats(h->ring),
                        hipGetErrorString(e));
        ddrl_replay_destroy(h);
        return DDRL_ERR_NOMEM;
    }
    // np.zeros for every ring (example/dsac.py:21-25)
    for (int j = 0; j < n_arrays; ++j)
        DDRL_HIP_CHECK(hipMemsetAsync(h->ring.a[j], 0, (size_t)capacity * widths_h[j] * (h->ring.kind[j] ? 1 : sizeof(float)), nullptr));
    DDRL_HIP_CHECK(hipMemsetAsync(h->state, 0, sizeof(RingState), nullptr));
    k_mt_seed<<<1, 64, 0, nullptr>>>(h->state, 0u);
    DDRL_LAUNCH_CHECK();
    DDRL_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = h;
    return DDRL_OK;
}

int ddrl_replay_create(ddrl_replay_t **out, int device, int64_t capacity, int obs_dim, int act_dim,
                       uint32_t flags) {
    DDRL_REQUIRE(obs_dim > 0 && act_dim > 0, "obs_dim/act_dim must be positive");
    DDRL_REQUIRE(!(flags & DDRL_REPLAY_ACTS_1D) || act_dim == 1, "ACTS_1D needs act_dim == 1");
    const int32_t widths[5] = {obs_dim, obs_dim, act_dim, 1, 1};  // obs1 obs2 acts rews done
    const uint8_t u8 = (flags & DDRL_REPLAY_U8_OBS) ? 1 : 0;
    const uint8_t kinds[5] = {u8, u8, 0, 0, 0};
    const int rc = ddrl_replay_create_typed(out, device, capacity, 5, widths, kinds, 1, 1);
    if (rc == DDRL_OK) (*out)->flags = flags;
    return rc;
}

int ddrl_replay_destroy(ddrl_replay_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    for (int j = 0; j < MAX_ARRAYS; ++j) (void)hipFree(h->ring.a[j]);
    (void)hipFree(h->state); (void)hipFree(h->idx_buf); (void)hipFree(h->rank_buf);
    delete h;
    return DDRL_OK;
}

int ddrl_replay_seed(ddrl_replay_t *h, uint32_t seed, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    k_mt_seed<<<1, 64, 0, ddrl::as_stream(stream)>>>(h->state, seed);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_replay_store_ex(ddrl_replay_t *h, const float *const *src_h, int64_t n, void *stream) {
    DDRL_REQUIRE(h != nullptr && src_h != nullptr, "NULL pointer");
    DDRL_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return DDRL_OK;
    StoreSrc srcs;
    int widest;
    DDRL_REQUIRE(store_srcs(h, src_h, srcs, widest), "NULL source array");
    ddrl::DeviceGuard g(h->device);
    const long long rows = n > h->ring.capacity ? h->ring.capacity : n;
    long long blocks = (rows * widest + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    k_store<<<dim3((unsigned)blocks, (unsigned)h->ring.n_arr), 256, 0, ddrl::as_stream(stream)>>>(h->state, h->ring, srcs, n);
    DDRL_LAUNCH_CHECK();
    ddrl_replay_note_store(h, n);
    return DDRL_OK;
}

int ddrl_replay_store_masked_ex(ddrl_replay_t *h, const float *const *src_h, const uint8_t *mask_d, int64_t n, void *stream) {
    DDRL_REQUIRE(h != nullptr && src_h != nullptr && mask_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(n >= 0 && n < 0x7fffffffll, "n must be in [0, 2^31)");
    DDRL_REQUIRE(!has_compact(h), "masked store into a compact (uint8) ring is not built");
    if (n == 0) return DDRL_OK;
    StoreSrc srcs;
    int widest;
    DDRL_REQUIRE(store_srcs(h, src_h, srcs, widest), "NULL source array");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const int grc = grow(h->rank_buf, h->rank_cap, n + 1, s);
    if (grc != DDRL_OK) return grc;
    k_mask_scan<<<1, 256, 0, s>>>(mask_d, n, h->rank_buf);
    long long blocks = (n * widest + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    k_store_masked<<<dim3((unsigned)blocks, (unsigned)h->ring.n_arr), 256, 0, s>>>(h->state, h->ring, srcs, h->rank_buf, n);
    DDRL_LAUNCH_CHECK();
    h->h_dirty = true;
    return DDRL_OK;
}

int ddrl_replay_append_ring(ddrl_replay_t *dst, ddrl_replay_t *src, void *stream) {
    DDRL_REQUIRE(dst != nullptr && src != nullptr, "NULL handle");
    const char *why = nullptr;
    if (dst == src) why = "source and destination are the same ring";
    else if (dst->device != src->device) why = "the two rings live on different devices";
    else if (has_compact(dst) || has_compact(src)) why = "a compact (uint8) ring on either side is not built (commit it with ddrl_replay_store_ex)";
    else if (dst->ring.n_arr != src->ring.n_arr) why = "the rings differ in their number of arrays";
    for (int j = 0; !why && j < dst->ring.n_arr; ++j)
        if (dst->ring.w[j] != src->ring.w[j]) why = "the rings differ in a row width";
    if (why) {
        ddrl::set_error("ddrl_replay_append_ring: %s", why);
        return DDRL_ERR_UNSUPPORTED;
    }
    ddrl::DeviceGuard g(dst->device);
    int widest = 1;
    for (int j = 0; j < dst->ring.n_arr; ++j) {
        const int wv = (dst->ring.w[j] & 3) == 0 ? dst->ring.w[j] / 4 : dst->ring.w[j];
        if (wv > widest) widest = wv;
    }
    // the rows src holds are counted on the device: the grid is sized for a full source (at most dst.capacity rows land) and capped;
    // the blocks beyond the true count find nothing to copy and take their ticket.  Cap 512 (x n_arr: a full wave of workgroups on
    // every CU), a quarter of k_store's: a block costs its ticket whether it copies or not, and here the host cannot shrink the
    // grid for a nearly empty source (profiles/free_running_workers.txt)
    const long long rows = src->ring.capacity > dst->ring.capacity ? dst->ring.capacity : src->ring.capacity;
    long long blocks = (rows * widest + 255) / 256;
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    k_append_ring<<<dim3((unsigned)blocks, (unsigned)dst->ring.n_arr), 256, 0, ddrl::as_stream(stream)>>>(dst->state, dst->ring, src->state,
                                                                                                         src->ring);
    DDRL_LAUNCH_CHECK();
    // host mirrors.  src is empty behind this launch whatever it held.  dst's new counters are on the device only; between two
    // refreshes the mirror is asked one thing — are there rows to draw from (require_rows, ddrl_replay_can_fuse) — and an append
    // takes none away: a ring known to hold rows needs no re-read (which would be a stream sync in front of the learner's next
    // eager draw), an empty one re-reads before it reports EMPTY_BUFFER.  ddrl_replay_counts always reads the device.
    src->h_ptr = src->h_size = 0;
    if (dst->h_size <= 0) dst->h_dirty = true;
    return DDRL_OK;
}

int ddrl_replay_store(ddrl_replay_t *h, const float *obs_d, const float *act_d, const float *rew_d,
                      const float *obs2_d, const float *done_d, int64_t n, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->ring.n_arr == 5, "not a 5-array (obs1, obs2, acts, rews, done) ring");
    const float *src[5] = {obs_d, obs2_d, act_d, rew_d, done_d};
    return ddrl_replay_store_ex(h, src, n, stream);
}

int ddrl_replay_sample_ex(ddrl_replay_t *h, int64_t batch, float *const *out_h, int64_t *idx_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && out_h != nullptr, "NULL pointer");
    DDRL_REQUIRE(batch > 0 && batch <= (1 << 24), "batch must be in [1, 2^24]");
    BatchPtrs out;
    DDRL_REQUIRE(batch_ptrs(out, out_h, h->ring.n_arr), "NULL output pointer");
    return ddrl_replay_draw(h, ddrl_replay_sampler_view(h), batch, out, idx_d, stream);
}

int ddrl_nstep_fold(const float *obs_w_d, const float *acts_w_d, const float *rews_w_d, const float *done_w_d, int64_t batch, int32_t Ln,
                    int32_t obs_dim, int32_t act_dim, float gamma, float *obs1_d, float *obs2_d, float *acts_d, float *rews_d, float *done_d,
                    void *stream) {
    BatchPtrs out;
    DDRL_REQUIRE(obs_w_d && acts_w_d && rews_w_d && done_w_d && batch_ptrs(out, obs1_d, obs2_d, acts_d, rews_d, done_d), "NULL pointer");
    DDRL_REQUIRE(Ln >= 1 && obs_dim >= 1 && act_dim >= 1, "Ln, obs_dim, act_dim must be positive");
    DDRL_REQUIRE(batch > 0 && batch <= (1 << 24) && batch * (obs_dim > act_dim ? obs_dim : act_dim) < 0x7fffffffll,
                 "batch must be in [1, 2^24] with batch * max(obs_dim, act_dim) < 2^31");
    const FoldSrc w{obs_w_d, acts_w_d, rews_w_d, done_w_d, Ln, obs_dim, act_dim, gamma};
    k_nstep_fold<<<fold_grid(batch, obs_dim), 256, 0, ddrl::as_stream(stream)>>>(w, out, (int)batch);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_replay_sample_nstep(ddrl_replay_t *h, int64_t batch, float gamma, float *obs1_d, float *obs2_d, float *acts_d, float *rews_d,
                             float *done_d, int64_t *idx_d, void *stream) {
    BatchPtrs out;
    DDRL_REQUIRE(h != nullptr && batch_ptrs(out, obs1_d, obs2_d, acts_d, rews_d, done_d), "NULL pointer");
    DDRL_REQUIRE(batch > 0 && batch <= (1 << 24), "batch must be in [1, 2^24]");
    const int rc = check_sample_nstep(h, batch, "ddrl_replay_sample_nstep");
    if (rc != DDRL_OK) return rc;
    return ddrl_replay_draw(h, ddrl_replay_sampler_view(h, true, gamma), batch, out, idx_d, stream);
}

int ddrl_replay_sample_many_nstep(ddrl_replay_t *h, int64_t batch, int64_t count, float gamma, float *const *out_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && out_h != nullptr, "NULL pointer");
    DDRL_REQUIRE(batch > 0 && count > 0 && batch * count <= (1 << 24), "batch, count must be positive with batch * count <= 2^24");
    const int rc = check_sample_nstep(h, batch * count, "ddrl_replay_sample_many_nstep");
    if (rc != DDRL_OK) return rc;
    if (h->feed_on) {
        ddrl::set_error("a feed plan is attached to this ring");
        return DDRL_ERR_UNSUPPORTED;
    }
    return sample_many(h, ddrl_replay_sampler_view(h, true, gamma), batch, count, out_h, stream);
}

int ddrl_replay_sample_indices(ddrl_replay_t *h, int64_t batch, int64_t *idx_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && idx_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(batch > 0 && batch <= (1 << 24), "batch must be in [1, 2^24]");
    DDRL_REQUIRE(!h->feed_on, "a feed plan is attached to this ring");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const int rc = require_rows(h, s);
    if (rc != DDRL_OK) return rc;
    return launch_draw(h, ddrl_replay_sampler_view(h), batch, nullptr, reinterpret_cast<long long *>(idx_d), s);
}

int ddrl_replay_sample(ddrl_replay_t *h, int64_t batch, float *obs1_d, float *obs2_d, float *acts_d,
                       float *rews_d, float *done_d, int64_t *idx_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->ring.n_arr == 5, "not a 5-array (obs1, obs2, acts, rews, done) ring");
    float *out[5] = {obs1_d, obs2_d, acts_d, rews_d, done_d};
    return ddrl_replay_sample_ex(h, batch, out, idx_d, stream);
}

int ddrl_replay_sample_many(ddrl_replay_t *h, int64_t batch, int64_t count, float *const *out_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && out_h != nullptr, "NULL pointer");
    DDRL_REQUIRE(batch > 0 && count > 0 && batch * count <= (1 << 24), "batch, count must be positive with batch * count <= 2^24");
    DDRL_REQUIRE(!h->feed_on, "a feed plan is attached to this ring");
    return sample_many(h, ddrl_replay_sampler_view(h), batch, count, out_h, stream);
}

int ddrl_replay_set_feed(ddrl_replay_t *h, const int32_t *plan_d, int32_t plan_len, int32_t batch, int32_t n_regions,
                         const float *const *region_base_h, const int32_t *region_count_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(plan_d == nullptr || (plan_len >= 0 && batch > 0 && n_regions >= 0 && n_regions <= MAX_FEED), "bad plan length / batch / region count");
    DDRL_REQUIRE(plan_d == nullptr || n_regions == 0 || (region_base_h && region_count_h), "NULL region table");
    Feed f{};
    if (plan_d) {
        f.plan = plan_d; f.pos = 0; f.len = plan_len; f.batch = batch; f.n_regions = n_regions;
        for (int r = 0; r < n_regions; ++r) {
            DDRL_REQUIRE(region_count_h[r] >= 0 && region_count_h[r] < (1 << 24) && (region_count_h[r] == 0 || region_base_h[r]), "bad region");
            f.base[r] = region_base_h[r]; f.count[r] = region_count_h[r];
        }
    }
    ddrl::DeviceGuard g(h->device);
    k_set_feed<<<1, 1, 0, ddrl::as_stream(stream)>>>(h->state, f);
    DDRL_LAUNCH_CHECK();
    h->feed_on = plan_d != nullptr;
    h->h_dirty = true;  // fed updates do not count as local samples: the mirror re-reads the device counters
    return DDRL_OK;
}

int ddrl_replay_gather_ex(ddrl_replay_t *h, const int64_t *idx_d, int64_t batch, float *const *out_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && idx_d != nullptr && out_h != nullptr, "NULL handle, index or output pointer");
    DDRL_REQUIRE(batch > 0 && batch <= (1 << 24), "batch must be in [1, 2^24]");
    BatchPtrs out;
    DDRL_REQUIRE(batch_ptrs(out, out_h, h->ring.n_arr), "NULL output pointer");
    ddrl::DeviceGuard g(h->device);
    return launch_gather(h, reinterpret_cast<const long long *>(idx_d), batch, out, ddrl::as_stream(stream));
}

int ddrl_replay_gather(ddrl_replay_t *h, const int64_t *idx_d, int64_t batch, float *obs1_d, float *obs2_d,
                       float *acts_d, float *rews_d, float *done_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && h->ring.n_arr == 5, "not a 5-array (obs1, obs2, acts, rews, done) ring");
    float *out[5] = {obs1_d, obs2_d, acts_d, rews_d, done_d};
    return ddrl_replay_gather_ex(h, idx_d, batch, out, stream);
}

int ddrl_replay_counts(ddrl_replay_t *h, int64_t *ptr_h, int64_t *size_h, int64_t *steps_h,
                       int64_t *sample_times_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    int rc = refresh_counts(h, ddrl::as_stream(stream));
    if (rc != DDRL_OK) return rc;
    if (ptr_h) *ptr_h = h->h_ptr;
    if (size_h) *size_h = h->h_size;
    if (steps_h) *steps_h = h->h_steps;
    if (sample_times_h) *sample_times_h = h->h_samples;
    return DDRL_OK;
}

int ddrl_replay_take_error(ddrl_replay_t *h, int32_t *out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && out_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    k_take_error<<<1, 1, 0, ddrl::as_stream(stream)>>>(h->state, out_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_replay_buffers_ex(ddrl_replay_t *h, float **arrays_h, int32_t *widths_h, int32_t *n_arrays_h) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    for (int j = 0; j < h->ring.n_arr; ++j) {
        if (arrays_h) arrays_h[j] = h->ring.a[j];
        if (widths_h) widths_h[j] = h->ring.w[j];
    }
    if (n_arrays_h) *n_arrays_h = h->ring.n_arr;
    return DDRL_OK;
}

int ddrl_replay_buffers(ddrl_replay_t *h, float **obs1_d, float **obs2_d, float **acts_d, float **rews_d,
                        float **done_d) {
    DDRL_REQUIRE(h != nullptr && h->ring.n_arr == 5, "not a 5-array (obs1, obs2, acts, rews, done) ring");
    if (obs1_d) *obs1_d = h->ring.a[0];
    if (obs2_d) *obs2_d = h->ring.a[1];
    if (acts_d) *acts_d = h->ring.a[2];
    if (rews_d) *rews_d = h->ring.a[3];
    if (done_d) *done_d = h->ring.a[4];
    return DDRL_OK;
}

int ddrl_replay_rows_export(ddrl_replay_t *h, int32_t array, int64_t row0, int64_t nrows, float *out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && out_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(array >= 0 && array < h->ring.n_arr && row0 >= 0 && nrows > 0 && row0 + nrows <= h->ring.capacity, "array / row range out of bounds");
    ddrl::DeviceGuard g(h->device);
    long long blocks = (nrows * h->ring.w[array] + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    k_rows_export<<<(unsigned)blocks, 256, 0, ddrl::as_stream(stream)>>>(h->ring, array, row0, nrows, out_d);
    DDRL_LAUNCH_CHECK();
    return DDRL_OK;
}

int ddrl_replay_rows_import(ddrl_replay_t *h, int32_t array, int64_t row0, int64_t nrows, const float *src_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && src_d != nullptr, "NULL pointer");
    DDRL_REQUIRE(array >= 0 && array < h->ring.n_arr && row0 >= 0 && nrows > 0 && row0 + nrows <= h->ring.capacity, "array / row range out of bounds");
    ddrl::DeviceGuard g(h->device);
    long long blocks = (nrows * h->ring.w[array] + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    k_rows_import<<<(unsigned)blocks, 256, 0, ddrl::as_stream(stream)>>>(h->state, h->ring, array, row0, nrows, src_d);
    DDRL_LAUNCH_CHECK();
    h->h_dirty = true;   // a value outside uint8 leaves the sticky error: the next host look at the ring reports it
    return DDRL_OK;
}

int ddrl_replay_set_counts(ddrl_replay_t *h, int64_t ptr, int64_t size, int64_t steps, int64_t sample_times,
                           void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE(ptr >= 0 && ptr < h->ring.capacity && size >= 0 && size <= h->ring.capacity, "ptr/size out of range");
    ddrl::DeviceGuard g(h->device);
    k_set_counts<<<1, 1, 0, ddrl::as_stream(stream)>>>(h->state, ptr, size, steps, sample_times);
    DDRL_LAUNCH_CHECK();
    h->h_ptr = ptr; h->h_size = size; h->h_steps = steps; h->h_samples = sample_times;
    return DDRL_OK;
}

int ddrl_replay_mt_state(ddrl_replay_t *h, uint32_t *key_h, int32_t *pos_h, void *stream) {
    DDRL_REQUIRE(h != nullptr && key_h != nullptr && pos_h != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    RingState tmp;
    hipStream_t s = ddrl::as_stream(stream);
    DDRL_HIP_CHECK(hipMemcpyAsync(&tmp, h->state, sizeof(RingState), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(key_h, tmp.mt_key, sizeof(tmp.mt_key));
    *pos_h = tmp.mt_pos;
    return DDRL_OK;
}

}  // extern "C"
