"""The DQN / SQN learner iteration straight out of the COMPACT (uint8) replay ring: ddrl_dqn_step_ring on a ring whose observation arrays
are bytes — the layer-1 forward (csrc/wide_l1.h, the U8 instance of k_wide) stages the sampled rows' bytes by LDS-DMA and converts them at
the LDS read, the weight gradient contracts a gathered float32 copy of obs1 (k_dqn_gather_rows_u8), obs2 is never materialised.

uint8 -> float32 is exact and the instance keeps the float32 forward's split-K plan, B staging, k -> (stage, group, lane half, j) mapping
and MFMA order, so there is no tolerance anywhere: every comparison is torch.equal against BOTH existing paths —
the two-call form on a compact twin ring (sample_batch_device + train) and the fused call on a float32 twin ring.

Every test calls lib.ddrl_dqn_step_ring on the compact ring itself and asserts its return code: a green result through Learner.train_from
alone could be the fallback."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WHICH = ("SAC1_GRAD", "SAC1_MAIN", "SAC1_TARGET", "SAC1_ADAM_M", "SAC1_ADAM_V")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(obs_dim, hidden, batch, rows):
    class O:
        act_dim, gamma, lr, polyak, seed, alpha, save_dir = 4, 0.99, 1e-4, 0.995, 2, 0.1, "."
    O.obs_dim, O.hidden_size, O.batch_size, O.buffer_size = obs_dim, list(hidden), batch, rows
    return O


def _learner(o, variant):
    from distributed_drl_amd import dqn
    ln = (dqn.LearnerSQN if variant == "sqn" else dqn.Learner)(o, "learner")
    names, vals = ln.get_weights()
    ln.set_weights(names[:1], [vals[0] * np.float32(1.0 / 64)])      # 0..255 pixels: keep layer 1 in range
    return ln


def _transitions(gen, n, obs_dim):
    """n pixel transitions on the device: integer observations in [0, 255] (both ends present), random acts / rews / done."""
    o1 = torch.randint(0, 256, (n, obs_dim), device="cuda", generator=gen).float()
    o2 = torch.randint(0, 256, (n, obs_dim), device="cuda", generator=gen).float()
    o1[0, 0], o1[0, 1], o2[0, 0], o2[0, 1] = 0.0, 255.0, 255.0, 0.0
    a = torch.randint(0, 4, (n,), device="cuda", generator=gen).float()
    r = torch.randn(n, device="cuda", generator=gen)
    d = (torch.rand(n, device="cuda", generator=gen) < 0.05).float()
    return o1, a, r, o2, d


def _fused(ln, ring):
    """lib.ddrl_dqn_step_ring itself (not train_from, which may fall back): rc must be 0."""
    from distributed_drl_amd import _lib
    B = ln.cfg.batch
    q = torch.empty(B, ln.cfg.n_actions, dtype=torch.float32, device="cuda")
    idx = torch.empty(B, dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    rc = _lib.load().ddrl_dqn_step_ring(ln._h, ring._h, _lib.dptr(loss), _lib.dptr(q), _lib.dptr(idx), _lib.stream_ptr())
    assert rc == 0, (rc, _lib.load().ddrl_last_error())
    return loss, q, idx


def _two_call(ln, ring, it):
    b = ring.sample_batch_device(ln.cfg.batch, with_indices=True)
    loss, q = ln.train(b, it, return_outputs=True)
    return loss, q, b["idxs"]


def _three_way(ddrl, variant, obs_dim, hidden, batch, rows, stores, iters=3, seed=33, data_seed=6):
    """Twin learners on three rings of the same seed and the same stored transitions: compact fused | compact two-call | float32 fused.
    Indices equal NumPy's stream; loss, q rows, gradient, parameters, targets, both Adam moments equal across all three at every
    iteration; counters and sampler state equal at the end."""
    from distributed_drl_amd import _lib
    o = _opt(obs_dim, hidden, batch, rows)
    gen = torch.Generator(device="cuda").manual_seed(data_seed)
    chunks = [_transitions(gen, n, obs_dim) for n in stores]
    rings = [ddrl.ReplayBufferDQN(o, 0, seed=seed, compact_obs=c) for c in (True, True, False)]
    for ring in rings:
        for tr in chunks:
            ring.store_batch(*tr)
    learners = [_learner(o, variant) for _ in range(3)]
    want_idx = np.random.RandomState(seed)
    size = min(rows, sum(stores))
    for it in range(iters):
        res = [_fused(learners[0], rings[0]), _two_call(learners[1], rings[1], it), _fused(learners[2], rings[2])]
        np.testing.assert_array_equal(res[0][2].cpu().numpy(), want_idx.randint(0, size, batch))
        for k in (1, 2):
            for a, b in zip(res[0], res[k]):
                assert torch.equal(a, b), (it, k)
            for w in WHICH:
                assert torch.equal(learners[0].export(getattr(_lib, w)), learners[k].export(getattr(_lib, w))), (it, k, w)
        assert torch.isfinite(res[0][0]).all() and float(learners[0].export(_lib.SAC1_GRAD).abs().max()) > 0
    assert rings[0].get_counts() == rings[1].get_counts() == rings[2].get_counts() == (iters, sum(stores), size)
    states = [r.mt_state() for r in rings]
    for k, p in states[1:]:
        assert p == states[0][1] and (k == states[0][0]).all()
    for ring in rings:
        ring.check()
    return chunks


@pytest.mark.parametrize("variant", ["ddqn", "sqn"])
def test_config5_iteration_out_of_the_compact_ring_equals_both_existing_paths(ddrl, variant):
    """Config 5's shape (28 224 / [400, 300] / batch 512, a 1536-row ring wrapped by 2000 stores), three iterations."""
    _three_way(ddrl, variant, 84 * 84 * 4, [400, 300], 512, 1536, (1000, 1000))


# obs_dim: 1024 = 32 whole stages; 1040 = the K % 32 == 16 tail (one 16-byte chunk per row); 2064 = the tail plus more K ranges.
# batch: 128 = one whole row tile; 96 = a wave with no rows; 37 = a partial 32-row block (rows beyond a_rows from the zero block);
# 200 = two row tiles, the second partial.  hidden: [400, 300] = column tiles of 5 / 4 / 4 units; [48, 32] = two units, the second half empty.
SMALL = [("ddqn", 1024, 128, [400, 300]), ("ddqn", 1040, 128, [400, 300]), ("sqn", 2064, 128, [400, 300]),
         ("ddqn", 1040, 96, [400, 300]), ("sqn", 1040, 37, [400, 300]), ("ddqn", 2064, 200, [400, 300]),
         ("ddqn", 1024, 37, [48, 32]), ("sqn", 1040, 200, [48, 32]), ("ddqn", 2064, 96, [48, 32]),
         ("sqn", 1024, 200, [400, 300]), ("ddqn", 2064, 37, [400, 300]), ("ddqn", 1040, 128, [48, 32])]


@pytest.mark.parametrize("variant,obs_dim,batch,hidden", SMALL, ids=["%s-%d-%d-%d" % (v, o, b, h[0]) for v, o, b, h in SMALL])
def test_small_shapes_where_the_byte_staging_can_go_wrong(ddrl, variant, obs_dim, batch, hidden):
    """A 300-row ring wrapped by 450 stores; pixels include 0 and 255, and any two rows differ in EVERY 16-byte chunk, so a chunk taken
    from the wrong row or the wrong swizzle slot cannot cancel."""
    chunks = _three_way(ddrl, variant, obs_dim, hidden, batch, 300, (200, 250))
    for j in (0, 3):
        px = torch.cat([c[j] for c in chunks])[-300:].to(torch.uint8).cpu().numpy()      # what the ring holds
        assert px.min() == 0 and px.max() == 255
        for c in range(obs_dim // 16):
            assert len(np.unique(px[:, 16 * c:16 * c + 16], axis=0)) == 300, (j, c)


@pytest.mark.parametrize("variant", ["ddqn", "sqn"])
def test_compact_ring_iteration_race_screen(ddrl, variant):
    """30 repeats of the same fused update out of the compact ring at config 5's shape, parameters and target re-imported and the ring's
    sampler reseeded before each: loss, q and the whole gradient bit-identical every time.  (The byte instance's LDS double buffers are
    ordered by vmcnt + barrier only — the construction whose round-3 race passed every value test.)"""
    from distributed_drl_amd import _lib
    o = _opt(84 * 84 * 4, [400, 300], 512, 1536)
    gen = torch.Generator(device="cuda").manual_seed(11)
    ring = ddrl.ReplayBufferDQN(o, 0, seed=5, compact_obs=True)
    ring.store_batch(*_transitions(gen, 1536, o.obs_dim))
    ln = _learner(o, variant)
    main = ln.export(_lib.SAC1_MAIN).clone()
    targ = torch.roll(main, 1)                                # any target != main
    first = None
    for rep in range(30):
        ln.import_(_lib.SAC1_MAIN, main)
        ln.import_(_lib.SAC1_TARGET, targ)
        ring.seed(5)
        loss, q, idx = _fused(ln, ring)
        got = (loss.clone(), q.clone(), idx.clone(), ln.export(_lib.SAC1_GRAD))
        if first is None:
            first = got
            assert torch.isfinite(got[3]).all() and float(got[3].abs().max()) > 0
        else:
            for a, w in zip(got, first):
                assert torch.equal(a, w), rep


def test_rows_beyond_two_to_the_32_bytes(ddrl):
    """A compact ring of 153 600 rows x 28 224 bytes (4.3 GB per observation array): rows beyond 152 174 start past byte 2^32.  Every row
    is distinguishable (a random 2048-row block with the row number in its first three bytes); the fused call equals the two-call form
    on a twin ring for two iterations, and the seed is chosen from NumPy's stream so that those iterations do draw such rows."""
    from distributed_drl_amd import _lib
    obs_dim, rows, B, blk = 84 * 84 * 4, 153600, 128, 2048
    first_beyond = (1 << 32) // obs_dim + 1
    assert (first_beyond - 1) * obs_dim < (1 << 32) <= first_beyond * obs_dim and first_beyond == 152175
    seed = next(s for s in range(1000)
                if (np.concatenate([r.randint(0, rows, B) for r in [np.random.RandomState(s)] for _ in range(2)]) >= first_beyond).any())
    o = _opt(obs_dim, [48, 32], B, rows)
    gen = torch.Generator(device="cuda").manual_seed(3)
    o1, a, r, o2, d = _transitions(gen, blk, obs_dim)
    rings = [ddrl.ReplayBufferDQN(o, 0, seed=seed, compact_obs=True) for _ in range(2)]
    for c in range(rows // blk):
        n = torch.arange(c * blk, (c + 1) * blk, device="cuda")
        for k in range(3):
            o1[:, k] = ((n >> (8 * k)) & 255).float()
            o2[:, k] = 255.0 - o1[:, k]
        for ring in rings:
            ring.store_batch(o1, a, r, o2, d)
    learners = [_learner(o, "ddqn") for _ in range(2)]
    want_idx = np.random.RandomState(seed)
    beyond = 0
    for it in range(2):
        got, ref = _fused(learners[0], rings[0]), _two_call(learners[1], rings[1], it)
        np.testing.assert_array_equal(got[2].cpu().numpy(), want_idx.randint(0, rows, B))
        beyond += int((got[2] >= first_beyond).sum())
        for x, y in zip(got, ref):
            assert torch.equal(x, y), it
        for w in WHICH:
            assert torch.equal(learners[0].export(getattr(_lib, w)), learners[1].export(getattr(_lib, w))), (it, w)
    assert beyond >= 1
    assert rings[0].get_counts() == rings[1].get_counts() == (2, rows, rows)
    for ring in rings:
        ring.check()


def test_the_cases_that_still_fall_back(ddrl):
    """obs_dim % 16 != 0 on a compact ring: the direct call says DDRL_ERR_UNSUPPORTED and why, train_from still trains (the two-call form)
    and equals the float32 twin.  A compact ring that was handed a non-representable value takes the fused call and still surfaces its
    sticky error at check()."""
    from distributed_drl_amd import _lib
    lib = _lib.load()
    o = _opt(1028, [48, 32], 64, 300)
    gen = torch.Generator(device="cuda").manual_seed(8)
    tr = _transitions(gen, 300, 1028)
    cring, fring = ddrl.ReplayBufferDQN(o, 0, seed=4, compact_obs=True), ddrl.ReplayBufferDQN(o, 0, seed=4)
    cring.store_batch(*tr)
    fring.store_batch(*tr)
    la, lb = _learner(o, "ddqn"), _learner(o, "ddqn")
    assert lib.ddrl_dqn_step_ring(la._h, cring._h, None, None, None, _lib.stream_ptr()) == _lib.DDRL_ERR_UNSUPPORTED
    assert b"multiple of 16" in lib.ddrl_last_error()
    assert cring.get_counts() == (0, 300, 300)                                   # the refused call drew nothing
    for it in range(2):
        loss_a, q_a, idx_a = la.train_from(cring, it, return_outputs=True, with_indices=True)
        loss_b, q_b, idx_b = _fused(lb, fring)
        assert torch.equal(loss_a, loss_b) and torch.equal(q_a, q_b) and torch.equal(idx_a, idx_b), it
        for w in WHICH:
            assert torch.equal(la.export(getattr(_lib, w)), lb.export(getattr(_lib, w))), (it, w)
    # the sticky word of a store that the bytes cannot hold
    o = _opt(1040, [48, 32], 64, 300)
    tr = list(_transitions(gen, 300, 1040))
    tr[0][7, 100] = 0.5
    ring = ddrl.ReplayBufferDQN(o, 0, seed=4, compact_obs=True)
    ring.store_batch(*tr)
    ln = _learner(o, "ddqn")
    loss, _, _ = _fused(ln, ring)
    assert torch.isfinite(loss).all()
    with pytest.raises(ValueError, match="not an integer in"):
        ring.check()
