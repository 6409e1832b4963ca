// The sampler workgroup of the DQN / SQN learner loop, shared by the generic update (dqn.hip: k_dqn_sample, k_dqn_head_sample) and the
// direct-operand one (dqn_direct.hip: k_qmid).  Included inside the anonymous namespace of a translation unit, behind replay_device.h.
// ------------------------------------------------------------------------------------------
// The learner loop's sampler (ddrl_dqn_loop_*): `idxs = np.random.randint(0, size, B)` of the ring's own MT19937 stream
// (ddrl_replay_dev::sample_block, the draw every other path runs) and the five gathers, written where the update reads them — rows of
// ldx floats in the padded images x1 / x2 of one of the learner's two input sets (their ones column is physical and untouched), acts /
// rew / done beside them — so that an update of the loop has no staging launch.  One workgroup of 256 lanes.  The draw leaves the
// indices in `idx` (B words of the learner's slab); the gather behind the barrier reads them back: the workgroup's own stores through
// the CU's vector cache, one round trip, off every update's dependent chain (the sampler rides beside an update, see below).
// sample_block and its dense gather (replay_device.h) are used as they are: the SAC1 launches that embed them compile from unchanged
// sources.  A feed plan is not followed here (fuse_gather = 0 skips it): ddrl_dqn_loop_run refuses a fed ring.
// ------------------------------------------------------------------------------------------
struct SetSampler {
    ddrl_replay_dev::RingState *st;
    ddrl_replay_dev::RingPtrs ring;   // (obs1[obs], obs2[obs], acts, rews, done), float32
    long long *idx;
    float *x1, *x2, *acts, *rew, *done;
    int B, obs, ldx;
};
__device__ __forceinline__ void sample_into_set(const SetSampler &m) {
    const bool rows = m.st->size > 0;   // (nothing in this launch stores into the ring) an empty ring: the draw raises the sticky error
    ddrl_replay_dev::sample_block(m.st, m.ring, ddrl_replay_dev::BatchPtrs{}, m.B, m.idx, 0);
    if (!rows) return;
    __syncthreads();
    const int tid = threadIdx.x;
    const float *r1 = m.ring.a[0], *r2 = m.ring.a[1];
    if ((m.obs & 3) == 0 && ddrl_replay_dev::aligned16(r1, r2) && ddrl_replay_dev::aligned16(m.x1, m.x2)) {   // (ldx is a multiple of 4)
        const int w4 = m.obs >> 2, l4 = m.ldx >> 2;
        const float4 *s1 = reinterpret_cast<const float4 *>(r1), *s2 = reinterpret_cast<const float4 *>(r2);
        float4 *d1 = reinterpret_cast<float4 *>(m.x1), *d2 = reinterpret_cast<float4 *>(m.x2);
        for (int e = tid; e < m.B * w4; e += 256) {
            const int b = e / w4, c = e - b * w4;
            const long long r = m.idx[b] * w4 + c;
            const float4 u = s1[r], v = s2[r];
            d1[b * l4 + c] = u; d2[b * l4 + c] = v;
        }
    } else {
        for (int e = tid; e < m.B * m.obs; e += 256) {
            const int b = e / m.obs, c = e - b * m.obs;
            const long long r = m.idx[b] * m.obs + c;
            const float u = r1[r], v = r2[r];
            m.x1[b * m.ldx + c] = u; m.x2[b * m.ldx + c] = v;
        }
    }
    for (int b = tid; b < m.B; b += 256) {
        const long long r = m.idx[b];
        m.acts[b] = m.ring.a[2][r]; m.rew[b] = m.ring.a[3][r]; m.done[b] = m.ring.a[4][r];
    }
}
