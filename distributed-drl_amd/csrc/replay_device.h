// Device-side pieces of the replay sampler shared by replay.hip (k_sample) and sac1.hip (the
// Adam/polyak kernel can run the NEXT update's sampler as one extra workgroup, see
// ddrl_sac1_apply_grads_and_sample).  Internal to libddrl_hip.so — not part of the C-ABI.
#pragma once
#include "ddrl_common.h"

namespace ddrl_replay_dev {

constexpr int MT_N = 624;
constexpr int MT_M = 397;
constexpr int SAMPLE_THREADS = 256;
constexpr int MAX_FUSED_BATCH = 4096;          // idx staged in LDS for the fused sample+gather
constexpr long long MAX_FUSED_BYTES = 1 << 18;  // fuse the gather when the whole batch is <= 256 KiB

constexpr int MAX_FEED = 16;

// Batches drawn on OTHER ranks' shards (partition.py): the learner's sampler follows a per-update plan held in
// device memory — entry -1 = draw from the local ring, entry (r << 24 | i) = take batch i of region r, a block of
// `count[r]` batches [obs1 | obs2 | acts | rews | done] (each array [count*B, w]) that shard owner r drew with its own
// index stream and sent in one message.  A window ring's sampler (fold view) is fed the same transition-shaped blocks: its
// owners fold on their own GPU (ddrl_replay_sample_many_nstep), a fed entry is copied as a finished batch and only -1
// entries run the fold-gather.  Lives in the ring state so that a captured graph follows a new plan without re-capture.
struct Feed {
    const int *plan;
    int pos, len, batch, n_regions;
    const float *base[MAX_FEED];
    int count[MAX_FEED];
};

struct RingState {
    long long ptr, size, steps, sample_times;
    unsigned int done_counter;  // last-block-done ticket for the store kernel
    int error;                  // sticky device-side error (sample from empty ring)
    int mt_pos;
    int pad;
    uint32_t mt_key[MT_N];
    Feed feed;                  // after the MT state: refresh_counts copies the head of the struct only
};

constexpr int MAX_ARRAYS = 6;

// A ring is a set of float32 struct-of-arrays rings that share one cursor: array j is
// [capacity][w[j]] row-major.  The SAC layouts (example/dsac.py:20-27) are the instance
// {obs1[obs], obs2[obs], acts[act], rews[1], done[1]}; the n-step window buffer of
// algos/sac1/sac_ray.py:40-51 is {buffer_o[(Ln+1)*obs], buffer_a[Ln*act], buffer_r[Ln], buffer_d[Ln]}.
// kind[j] = 1: array j is stored as uint8 (the opt-in COMPACT ring for integer-valued pixel observations, DDRL_REPLAY_U8_OBS):
// a[j] then points at capacity * w[j] BYTES.  The surface stays float32 — store converts (a value that is not an integer in
// [0, 255] sets the sticky DDRL_ERR_NOT_REPRESENTABLE), every gather converts back: bit-identical to the float32 ring on such data.
// fold = 1 (a sampler's VIEW of a window ring, never the handle's own description): the gather behind the index draw is the n-step
// fold-gather below — five learner arrays out of four window arrays, backup discount `gamma`.  Both fields sit in what was padding:
// the struct, and every kernel argument block that embeds it, keeps its size and offsets.
struct RingPtrs {
    float *a[MAX_ARRAYS];
    int w[MAX_ARRAYS];
    unsigned char kind[MAX_ARRAYS];
    unsigned char fold;
    int n_arr;
    float gamma;
    long long capacity;
    long long steps_inc, samples_inc;  // counter increments per store / per sample (sac_ray.py:68,75: num_buffers)
};

static_assert(sizeof(RingPtrs) == 112, "RingPtrs is embedded in kernel argument blocks: keep its size");

struct BatchPtrs {
    float *a[MAX_ARRAYS];
};
// The output table of a draw / gather / fold from `n` pointers, or from the five learner arrays; false: one of them is NULL
static inline bool batch_ptrs(BatchPtrs &out, float *const *p, int n) {
    out = BatchPtrs{};
    for (int j = 0; j < n; ++j) {
        if (p[j] == nullptr) return false;
        out.a[j] = p[j];
    }
    return true;
}
static inline bool batch_ptrs(BatchPtrs &out, float *obs1, float *obs2, float *acts, float *rews, float *done) {
    float *const p[5] = {obs1, obs2, acts, rews, done};
    return batch_ptrs(out, p, 5);
}

// The cursor commit of a launch that stored `n` rows from cursor `ptr` (read by every block before its ticket): the last block to
// finish advances ptr / size / steps and resets the ticket counter.  One lane per block calls it, behind the block's barrier;
// true in the block that committed.
__device__ __forceinline__ bool ring_commit(RingState *st, const RingPtrs &ring, long long ptr, long long n) {
    const unsigned total_blocks = gridDim.x * gridDim.y;
    const unsigned ticket = atomicAdd(&st->done_counter, 1u);
    if (ticket != total_blocks - 1) return false;
    const long long cap = ring.capacity;
    st->ptr = (ptr + n) % cap;
    const long long sz = st->size + n;
    st->size = sz > cap ? cap : sz;
    st->steps += n * ring.steps_inc;
    st->done_counter = 0;
    return true;
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

__device__ __forceinline__ uint32_t mt_mix(uint32_t cur, uint32_t nxt, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// Regenerate all 624 words: `mt` -> `nw` (a second LDS array: no barrier between a segment's reads and its writes).  The recurrence
// mt[k] <- f(mt[k], mt[k+1], mt[(k+397)%624]) has lag 397, so it splits into three segments whose inputs are all available in parallel:
// [0,227) reads only old words; [227,454) reads new words of segment 1; [454,624) reads new words of segment 2 (and new mt[0]
// for k = 623).  Three barriers; the caller swaps the two arrays.
__device__ __forceinline__ void mt_twist_lds(const uint32_t *mt, uint32_t *nw, int tid) {
    constexpr int S = MT_N - MT_M;   // 227
    if (tid < S) nw[tid] = mt_mix(mt[tid], mt[tid + 1], mt[tid + MT_M]);
    __syncthreads();
    const int k2 = S + tid;          // 227..453
    if (tid < S) nw[k2] = mt_mix(mt[k2], mt[k2 + 1], nw[k2 - S]);
    __syncthreads();
    const int k3 = 2 * S + tid;      // 454..623
    if (k3 < MT_N) nw[k3] = mt_mix(mt[k3], k3 == MT_N - 1 ? nw[0] : mt[k3 + 1], nw[k3 - S]);
    __syncthreads();
}

__device__ __forceinline__ bool aligned16(const void *a, const void *b) {
    return ((reinterpret_cast<unsigned long long>(a) | reinterpret_cast<unsigned long long>(b)) & 15ull) == 0;
}

// float32 -> the byte a compact (uint8) array holds: clamped to [0, 255] and truncated; `bad` is raised when the value does not
// survive the round trip (not an integer in [0, 255], NaN) — the caller turns it into the sticky DDRL_ERR_NOT_REPRESENTABLE
__device__ __forceinline__ unsigned to_u8(float f, bool &bad) {
    const unsigned b = (unsigned)(int)fminf(fmaxf(f, 0.f), 255.f);
    bad |= !((float)b == f);
    return b;
}

__device__ __forceinline__ void gather_rows(const float *__restrict__ ring, float *__restrict__ out,
                                            const unsigned *s_idx, int B, int width, int tid, int nthreads, int kind = 0) {
    if (kind == 1) {   // compact array: bytes in, float32 out
        const unsigned char *r8 = reinterpret_cast<const unsigned char *>(ring);
        for (int e = tid; e < B * width; e += nthreads) {
            const int b = e / width, c = e - b * width;
            out[e] = (float)r8[(long long)s_idx[b] * width + c];
        }
        return;
    }
    if ((width & 3) == 0 && aligned16(ring, out)) {
        const int w4 = width >> 2;
        const float4 *r4 = reinterpret_cast<const float4 *>(ring);
        float4 *o4 = reinterpret_cast<float4 *>(out);
        for (int e = tid; e < B * w4; e += nthreads) {
            const int b = e / w4, c = e - b * w4;
            o4[e] = r4[(long long)s_idx[b] * w4 + c];
        }
    } else {
        for (int e = tid; e < B * width; e += nthreads) {
            const int b = e / width, c = e - b * width;
            out[e] = ring[(long long)s_idx[b] * width + c];
        }
    }
}

// The n-step fold: window row i = o[0..Ln], a[0..Ln-1], r[0..Ln-1], d[0..Ln-1] (algos/sac1/sac_ray.py:40-51) becomes the transition
//   obs1 = o[0]   obs2 = o[Ln]   acts = a[0]   rews = sum_k c_k r[k]   done = 1 - prod_k (1 - d[k]),   c_0 = 1, c_{k+1} = c_k (1 - d[k]) gamma
// so that the update's backup rews + gamma (1 - done) v(obs2) is the n-step return cut at the first terminal.  float32, every product and
// sum rounded on its own (no contraction: the explicit _rn forms) — a NumPy float32 loop gives the same bits.
__device__ __forceinline__ void nstep_fold_row(const float *__restrict__ r, const float *__restrict__ d, int Ln, float gamma, float &rew, float &done) {
    float c = 1.f, R = 0.f, g = 1.f;
    for (int k = 0; k < Ln; ++k) {
        R = __fadd_rn(R, __fmul_rn(c, r[k]));
        g = __fmul_rn(c, __fsub_rn(1.f, d[k]));
        c = __fmul_rn(g, gamma);
    }
    rew = R;
    done = __fsub_rn(1.f, g);
}

// Fold-gather of B window rows (row of batch element b: idx_of(b)) into the five learner arrays: per row only o[0], o[Ln], a[0] and the
// 2 Ln reward / done scalars are read, not the whole window.  `tid` of `nthreads` lanes: one workgroup (the sampler) or a grid.
// B * max(od, ad) < 2^31 (host-checked for the stand-alone launches; the one-workgroup sampler has B <= MAX_FUSED_BATCH).
template <class Idx>
__device__ __forceinline__ void nstep_fold_gather(const float *__restrict__ ow, const float *__restrict__ aw, const float *__restrict__ rw,
                                                  const float *__restrict__ dw, int Ln, int od, int ad, float gamma, float *__restrict__ obs1,
                                                  float *__restrict__ obs2, float *__restrict__ acts, float *__restrict__ rews,
                                                  float *__restrict__ done, unsigned B, Idx idx_of, unsigned tid, unsigned nthreads) {
    if ((od & 3) == 0 && aligned16(ow, obs1) && aligned16(ow, obs2)) {
        const unsigned o4 = (unsigned)od >> 2;
        const long long W4 = (long long)(Ln + 1) * o4;
        const float4 *w4 = reinterpret_cast<const float4 *>(ow);
        for (unsigned e = tid; e < B * o4; e += nthreads) {
            const unsigned b = e / o4, c = e - b * o4;
            const float4 *row = w4 + (long long)idx_of(b) * W4;
            reinterpret_cast<float4 *>(obs1)[e] = row[c];
            reinterpret_cast<float4 *>(obs2)[e] = row[(unsigned)Ln * o4 + c];
        }
    } else {
        const long long W = (long long)(Ln + 1) * od;
        for (unsigned e = tid; e < B * (unsigned)od; e += nthreads) {
            const unsigned b = e / (unsigned)od, c = e - b * (unsigned)od;
            const float *row = ow + (long long)idx_of(b) * W;
            obs1[e] = row[c];
            obs2[e] = row[(unsigned)Ln * (unsigned)od + c];
        }
    }
    for (unsigned e = tid; e < B * (unsigned)ad; e += nthreads) {
        const unsigned b = e / (unsigned)ad, c = e - b * (unsigned)ad;
        acts[e] = aw[(long long)idx_of(b) * Ln * ad + c];
    }
    for (unsigned b = tid; b < B; b += nthreads) {
        const long long i = (long long)idx_of(b) * Ln;
        nstep_fold_row(rw + i, dw + i, Ln, gamma, rews[b], done[b]);
    }
}

// idxs = np.random.randint(0, size, B) (masked rejection on 32-bit draws), optionally fused with
// the five gathers when the batch is small (the SAC1 shape: 256 x 80 B).  One workgroup: the
// accept/reject compaction is a wave ballot + prefix count, the stream position advances by
// exactly the number of words NumPy would have consumed.
// NT = threads of the workgroup: SAMPLE_THREADS where the sampler rides in another kernel's launch and for batches that are
// gathered in the same workgroup; 640 for large stand-alone draws (a shard owner's block of batches): a whole 624-word state
// block per pass — one accept / compact pass and one regeneration per block instead of three passes (the pass, not the words, is
// what a one-workgroup draw pays for: 0.60 -> 0.2 ms for 262 144 indices).
template <int NT = SAMPLE_THREADS>
__device__ __forceinline__ void sample_block(RingState *st, const RingPtrs &ring, const BatchPtrs &out, int B,
                                             long long *idx_out, int fuse_gather) {
    constexpr int SAMPLE_THREADS = NT;   // (shadows the namespace constant inside this function)
    __shared__ uint32_t mt_a[MT_N], mt_b[MT_N];
    uint32_t *mt = mt_a, *mt_other = mt_b;   // (block-uniform pointers: the regeneration writes the other array, then they swap)
    __shared__ int s_wave_tot[SAMPLE_THREADS / 64];
    __shared__ int s_consumed;
    __shared__ unsigned s_idx[MAX_FUSED_BATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (fuse_gather && st->feed.plan != nullptr) {
        const int pos = st->feed.pos;
        const int p = pos < st->feed.len ? st->feed.plan[pos] : -1;
        __syncthreads();  // every lane has read the position
        if (tid == 0) st->feed.pos = pos + 1;
        if (p >= 0) {     // a batch another rank drew: copy it, consume no local draw
            const int r = p >> 24, i = p & 0xffffff;
            if (B != st->feed.batch || r >= st->feed.n_regions || i >= st->feed.count[r]) {
                if (tid == 0) st->error = DDRL_ERR_BAD_ARG;
                return;
            }
            const float *src = st->feed.base[r];
            const long long rows = (long long)st->feed.count[r] * B;
            // batch i of the region's next array ([rows, w]) -> dst[B, w]; float4 where both sides and the row counts allow
            auto copy_fed = [&](float *dst, int w) {
                const int n = B * w;
                const float *sj = src + (long long)i * n;
                if ((n & 3) == 0 && ((rows * w) & 3) == 0 && ((((unsigned long long)dst) | ((unsigned long long)src)) & 15ull) == 0) {
                    for (int e = tid; e < (n >> 2); e += SAMPLE_THREADS)
                        reinterpret_cast<float4 *>(dst)[e] = reinterpret_cast<const float4 *>(sj)[e];
                } else {
                    for (int e = tid; e < n; e += SAMPLE_THREADS) dst[e] = sj[e];
                }
                src += rows * w;
            };
            if (ring.fold) {  // a window ring's regions hold FOLDED blocks (the owner folded): the five learner arrays {od, od, ad, 1, 1}
                const int Ln = ring.w[3], od = ring.w[0] / (Ln + 1), ad = ring.w[1] / Ln;
                copy_fed(out.a[0], od);
                copy_fed(out.a[1], od);
                copy_fed(out.a[2], ad);
                copy_fed(out.a[3], 1);
                copy_fed(out.a[4], 1);
                return;
            }
#pragma unroll
            for (int j = 0; j < MAX_ARRAYS; ++j)
                if (j < ring.n_arr) copy_fed(out.a[j], ring.w[j]);
            return;
        }
    }
    const long long size = st->size;
    if (size <= 0) {  // reference: ValueError("high <= 0"); the host wrapper reports it
        if (tid == 0) st->error = DDRL_ERR_EMPTY_BUFFER;
        return;
    }
    const uint32_t rng = (uint32_t)(size - 1);
    if (rng == 0) {
        // NumPy fills with `low` and consumes no draw
        for (int i = tid; i < B; i += SAMPLE_THREADS) {
            if (idx_out) idx_out[i] = 0;
            if (fuse_gather) s_idx[i] = 0;
        }
    } else {
        uint32_t mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        for (int i = tid; i < MT_N; i += SAMPLE_THREADS) mt[i] = st->mt_key[i];
        int pos = st->mt_pos;
        bool dirty = false;
        int produced = 0;
        __syncthreads();
        while (produced < B) {
            if (pos >= MT_N) {
                mt_twist_lds(mt, mt_other, tid);
                uint32_t *t = mt; mt = mt_other; mt_other = t;
                pos = 0;
                dirty = true;
            }
            const int w = pos + tid;
            const bool valid = w < MT_N;
            const uint32_t v = valid ? (mt_temper(mt[w]) & mask) : 0xffffffffu;
            const bool acc = valid && v <= rng;
            const unsigned long long bal = __ballot(acc);
            const int rank_in_wave = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) s_wave_tot[wave] = __popcll(bal);
            __syncthreads();
            int off = 0, tot = 0;
#pragma unroll
            for (int i = 0; i < SAMPLE_THREADS / 64; ++i) {
                const int t = s_wave_tot[i];
                if (i < wave) off += t;
                tot += t;
            }
            const int rank = off + rank_in_wave;
            const int need = B - produced;
            if (acc && rank < need) {
                if (idx_out) idx_out[produced + rank] = (long long)v;
                if (fuse_gather) s_idx[produced + rank] = v;
                if (rank == need - 1) s_consumed = tid + 1;  // words consumed up to the last accepted draw
            }
            __syncthreads();
            if (tot >= need) {
                pos += s_consumed;
                produced = B;
            } else {
                pos += (MT_N - pos < SAMPLE_THREADS) ? (MT_N - pos) : SAMPLE_THREADS;
                produced += tot;
            }
            __syncthreads();
        }
        if (dirty)
            for (int i = tid; i < MT_N; i += SAMPLE_THREADS) st->mt_key[i] = mt[i];
        if (tid == 0) st->mt_pos = pos;
    }
    if (tid == 0) st->sample_times += ring.samples_inc;
    if (fuse_gather) {
        __syncthreads();
        if (ring.fold) {  // a window ring {o, a, r, d} seen by a learner: w[3] = Ln, w[0] = (Ln + 1) obs, w[1] = Ln act (host-checked)
            const int Ln = ring.w[3];
            nstep_fold_gather(ring.a[0], ring.a[1], ring.a[2], ring.a[3], Ln, ring.w[0] / (Ln + 1), ring.w[1] / Ln, ring.gamma, out.a[0], out.a[1],
                              out.a[2], out.a[3], out.a[4], (unsigned)B, [&](unsigned b) { return s_idx[b]; }, (unsigned)tid, (unsigned)SAMPLE_THREADS);
            return;
        }
#pragma unroll
        for (int j = 0; j < MAX_ARRAYS; ++j)
            if (j < ring.n_arr) gather_rows(ring.a[j], out.a[j], s_idx, B, ring.w[j], tid, SAMPLE_THREADS, ring.kind[j]);
    }
}


// What another kernel needs to run sample_block for a replay handle.
struct SamplerView {
    RingState *state;
    RingPtrs ring;
    int device;
};

}  // namespace ddrl_replay_dev

// defined in replay.hip
// the sampler's view of a ring; fold = true: of an n-step window ring in fold-gather mode with backup discount `gamma`
ddrl_replay_dev::SamplerView ddrl_replay_sampler_view(ddrl_replay_t *h, bool fold = false, float gamma = 0.f);
// can the one-workgroup sampler draw AND gather `batch` rows of this view (so that it can ride in another kernel's launch): batch and
// gathered bytes under the caps — the bytes the view's gather moves per index, not the whole windows of a fold view
bool ddrl_replay_can_fuse(ddrl_replay_t *h, const ddrl_replay_dev::SamplerView &v, int64_t batch);
// n-step window rings (algos/sac1/sac_ray.py:40-51): is this ring {o[(Ln+1) obs], a[Ln act], r[Ln], d[Ln]} of float32 arrays
bool ddrl_replay_is_window_ring(ddrl_replay_t *h, int obs_dim, int act_dim);
// sample_batch(batch) through view `v` into `out` (and idx_d, nullable) as launches of its own: ddrl_replay_sample_ex / _sample_nstep
// behind their argument checks
int ddrl_replay_draw(ddrl_replay_t *h, const ddrl_replay_dev::SamplerView &v, int64_t batch, const ddrl_replay_dev::BatchPtrs &out,
                     int64_t *idx_d, void *stream);
void ddrl_replay_note_sample(ddrl_replay_t *h);  // host mirror bookkeeping for a sample issued by another kernel
void ddrl_replay_note_store(ddrl_replay_t *h, long long n);  // ... for n stores issued by another kernel
