"""GPU: sharded replay on n-step window rings — the owner folds (ReplayBufferNStep.sample_many, ddrl_replay_sample_many_nstep) and the
learner's fold-view sampler follows a feed plan of folded blocks (set_feed on a window ring): alone, inside the learner's launches and
inside the captured loop.  The float32 reference of every folded row is tests/_nstep_fold.py (fold32); every comparison is bit-exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nstep_fold as nf  # noqa: E402

NAMES = ("obs1", "obs2", "acts", "rews", "done")
WNAMES = ("obs", "acts", "rews", "done")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(Ln=8, batch=64, obs_dim=8, act_dim=2, cap=256, num_buffers=1, seed=3):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=obs_dim, act_dim=act_dim)
    opt.Ln, opt.batch_size, opt.buffer_size, opt.num_buffers, opt.seed = Ln, batch, cap, num_buffers, seed
    return opt


def _ring(ddrl, opt, win, seed):
    rb = ddrl.ReplayBufferNStep(opt, seed=seed)
    if win is not None:
        rb.store_batch(*(torch.from_numpy(win[k]).cuda() for k in WNAMES))
    return rb


def _stored(rb):
    """The ring's windows as they lie in it (host copy): what index i of a draw means."""
    g = rb.rings()
    return {k: g["buffer_" + k[0]].cpu().numpy() for k in WNAMES}


def _fold_rows(stored, idx, gamma):
    return nf.fold32({k: v[idx] for k, v in stored.items()}, gamma)


def _packed(b):
    return np.concatenate([(b[k].cpu().numpy() if torch.is_tensor(b[k]) else np.asarray(b[k])).reshape(-1) for k in NAMES])


def _block_batch(blk, i, B, K, od, ad):
    """Batch i of a packed block of K batches, packed like a single batch."""
    out, off = [], 0
    for w in (od, od, ad, 1, 1):
        out.append(blk[off + i * B * w: off + (i + 1) * B * w])
        off += K * B * w
    return np.concatenate(out)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _fp(rb):
    key, pos = rb.mt_state()
    return pos, key.tobytes()


def _nfloats(B, od, ad):
    return B * (2 * od + ad + 2)


# ---- 1. the owner's block draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,obs_dim,Ln,cap,stores,num_buffers", [
    (37, 3, 5, 3, 256, 100, 2),     # scalar path; K B = 111 rows: obs2 / acts / rews / done start off the 16-byte grid
    (64, 5, 8, 8, 64, 100, 1),      # float4 path; 100 stores wrap the 64-slot ring
    (256, 20, 8, 8, 256, 200, 1),   # 5120 rows > the one-workgroup sampler: k_sample_wide + k_nstep_gather
    (37, 2, 8, 1, 64, 1, 2),        # one stored window: np.random.randint(0, 1, n) consumes no draw
])
def test_sample_many_equals_consecutive_folded_draws(ddrl, B, K, obs_dim, Ln, cap, stores, num_buffers):
    opt = _opt(Ln=Ln, batch=B, obs_dim=obs_dim, cap=cap, num_buffers=num_buffers)
    win = nf.windows(np.random.RandomState(stores + B), stores, Ln, obs_dim, 2, terminal="every")
    seed = 40 + B
    a, b, c = (_ring(ddrl, opt, win, seed) for _ in range(3))
    size = min(stores, cap)
    rs = np.random.RandomState(seed)
    stored = _stored(b)
    nfl = _nfloats(B, obs_dim, 2)
    for rep in range(2):
        blk = a.sample_many(B, K, torch.full((K * nfl,), -7.0, dtype=torch.float32, device="cuda")).cpu().numpy()
        if rep == 0:   # the same block with every array base off by 4 bytes as well
            base = torch.full((K * nfl + 1,), -7.0, dtype=torch.float32, device="cuda")
            _bits(c.sample_many(B, K, base[1:]).cpu().numpy(), blk, "shift 1")
        idx = rs.randint(0, size, B * K)
        seq = [b.sample_nstep_device(B, with_indices=True) for _ in range(K)]
        np.testing.assert_array_equal(np.concatenate([s["idxs"].cpu().numpy() for s in seq]), idx)
        for i in range(K):
            _bits(_block_batch(blk, i, B, K, obs_dim, 2), _packed(seq[i]), (rep, i))
            _bits(_block_batch(blk, i, B, K, obs_dim, 2), _packed(_fold_rows(stored, idx[i * B:(i + 1) * B], opt.gamma)), ("fold32", rep, i))
        assert _fp(a) == _fp(b)
        assert a.get_counts() == b.get_counts() == ((rep + 1) * K * num_buffers, stores * num_buffers, size)
    other = a.sample_many(B, 1, torch.empty(nfl, device="cuda"), gamma=0.5).cpu().numpy()   # an explicit discount
    _bits(other, _packed(b.sample_nstep_device(B, gamma=0.5)), "gamma 0.5")


# ---- 2. the learner side: a feed plan of folded blocks on a window ring ---------------------------------------------------------------
@pytest.mark.parametrize("B,obs_dim", [(64, 8), (37, 5)])
def test_feed_plan_interleaves_folded_blocks_with_local_folded_draws(ddrl, B, obs_dim):
    """tests/test_gpu_replay.py::test_feed_plan_interleaves_remote_blocks_with_local_draws on window rings.  obs 8 / B 64: the float4
    copy; obs 5 / B 37: the scalar one (K B w is no multiple of 4, the arrays of a block start off the 16-byte grid)."""
    Ln, ad = 8, 2
    opt = _opt(Ln=Ln, batch=B, obs_dim=obs_dim, cap=512)
    nfl = _nfloats(B, obs_dim, ad)
    K = [5, 3]
    owners = [_ring(ddrl, opt, nf.windows(np.random.RandomState(s), 300, Ln, obs_dim, ad, terminal="every"), seed=7 + s) for s in (1, 2)]
    blocks = [o.sample_many(B, k, torch.empty(k * nfl, dtype=torch.float32, device="cuda")) for o, k in zip(owners, K)]
    win = nf.windows(np.random.RandomState(0), 400, Ln, obs_dim, ad, terminal="some")
    local, twin = _ring(ddrl, opt, win, 9), _ring(ddrl, opt, win, 9)
    stored, rs = _stored(twin), np.random.RandomState(9)
    plan = [-1, 0 << 24 | 0, 1 << 24 | 0, -1, -1, 0 << 24 | 1, 1 << 24 | 1, 0 << 24 | 2, -1, 1 << 24 | 2, 0 << 24 | 3, 0 << 24 | 4]
    plan_d = torch.tensor(plan, dtype=torch.int32, device="cuda")

    def local_draw(what):
        got = _packed(local.sample_nstep_device(B))
        w = twin.sample_batch_device(B, with_indices=True)       # the plain window sampler of the twin: NumPy's indices, whole windows
        idx = rs.randint(0, 400, B)
        np.testing.assert_array_equal(w["idxs"].cpu().numpy(), idx)
        _bits(got, _packed(_fold_rows(stored, idx, opt.gamma)), what)

    for rep in range(2):
        local.set_feed(plan_d, B, list(zip(blocks, K)))
        for p in plan:
            if p < 0:
                local_draw("rep %d local" % rep)
            else:
                r, i = p >> 24, p & 0xffffff
                _bits(_packed(local.sample_nstep_device(B)), _block_batch(blocks[r].cpu().numpy(), i, B, K[r], obs_dim, ad), "rep %d entry %d" % (rep, p))
        assert _fp(local) == _fp(twin)                           # fed entries consumed no local draw
    local_draw("beyond the plan's end")
    assert local.get_counts()[0] == twin.get_counts()[0] == 2 * plan.count(-1) + 1   # sample_times counts local draws only
    local.set_feed(None, B, [])
    local_draw("detached")
    # the block draw stays an owner's call: refused while a plan is attached, nothing drawn
    from distributed_drl_amd import _lib
    local.set_feed(plan_d, B, list(zip(blocks, K)))
    with pytest.raises(_lib.DdrlError, match="feed plan"):
        local.sample_many(B, 2, torch.empty(2 * nfl, device="cuda"))
    local.set_feed(None, B, [])
    assert _fp(local) == _fp(twin)


# ---- 3. errors ----------------------------------------------------------------------------------------------------------------------
def _draw_into(rb, B, gamma, outs):
    from distributed_drl_amd import _lib
    return _lib.load().ddrl_replay_sample_nstep(rb._h, B, gamma, *[_lib.dptr(t) for t in outs], None, _lib.stream_ptr())


def test_bad_entries_empty_feed_ring_and_refusals(ddrl):
    from distributed_drl_amd import _lib
    B, Ln, od, ad = 64, 8, 8, 2
    opt = _opt(Ln=Ln, batch=B, cap=256)
    nfl = _nfloats(B, od, ad)
    owner = _ring(ddrl, opt, nf.windows(np.random.RandomState(1), 200, Ln, od, ad), seed=7)
    blk = owner.sample_many(B, 3, torch.empty(3 * nfl, dtype=torch.float32, device="cuda"))
    local = _ring(ddrl, opt, nf.windows(np.random.RandomState(2), 200, Ln, od, ad), seed=9)
    fp = _fp(local)
    for bad, batch in ((0 << 24 | 3, B), (1 << 24 | 0, B), (0 << 24 | 2, B + 1)):   # batch index == count; region == n_regions; another batch size
        local.set_feed(torch.tensor([bad], dtype=torch.int32, device="cuda"), batch, [(blk, 3)])
        outs = [torch.full((B * w,), -7.0, device="cuda") for w in (od, od, ad, 1, 1)]
        assert _draw_into(local, B, opt.gamma, outs) == 0           # the launch itself cannot fail (it may be a graph node)
        for t in outs:
            assert bool((t == -7.0).all())                          # output untouched
        with pytest.raises(ValueError, match="feed-plan"):
            local.get_counts()
        assert local.get_counts()[0] == 0 and _fp(local) == fp      # reported once, cleared; nothing was drawn
    local.set_feed(torch.tensor([0 << 24 | 3], dtype=torch.int32, device="cuda"), B, [(blk, 3)])
    local.sample_nstep_device(B)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    local.take_error(word)
    assert int(word.item()) == -1
    local.take_error(word)
    assert int(word.item()) == 0
    local.get_counts()
    # a dedicated learner's ring: one slot, never stored into, only ever follows the plan
    one = _opt(Ln=Ln, batch=B, cap=1)
    ghost = ddrl.ReplayBufferNStep(one)
    ghost.set_feed(torch.tensor([0 << 24 | 1, 0 << 24 | 2, -1], dtype=torch.int32, device="cuda"), B, [(blk, 3)])
    for i in (1, 2):
        _bits(_packed(ghost.sample_nstep_device(B)), _block_batch(blk.cpu().numpy(), i, B, 3, od, ad), "ghost %d" % i)
    assert ghost.get_counts() == (0, 0, 0)
    ghost.sample_nstep_device(B)                                    # the -1 entry: a local draw from the empty ring
    with pytest.raises(ValueError, match="high <= 0"):
        ghost.get_counts()
    assert ghost.get_counts() == (0, 0, 0)
    # the folded block draw is a window ring's
    tr = ddrl.ReplayBufferSAC1(od, ad, 64, seed=1)
    tr.store_batch(*(torch.zeros(4, w, device="cuda") for w in (od, ad, 1, od, 1)))
    flat = torch.empty(2 * nfl, device="cuda")
    ptrs, off = (ctypes.c_void_p * 5)(), 0
    for j, w in enumerate((od, od, ad, 1, 1)):
        ptrs[j] = flat.data_ptr() + 4 * off
        off += 2 * B * w
    rc = _lib.load().ddrl_replay_sample_many_nstep(tr._h, B, 2, 0.99, ptrs, _lib.stream_ptr())
    assert rc == _lib.DDRL_ERR_UNSUPPORTED
    assert tr.get_counts() == (0, 4, 4)                             # nothing was drawn
    with pytest.raises(ValueError, match="high <= 0"):
        ddrl.ReplayBufferNStep(opt, seed=1).sample_many(B, 2, flat)


# ---- 4. the learner on a fed window ring ----------------------------------------------------------------------------------------------
def _state(agent):
    from distributed_drl_amd import _lib
    return [agent.export(w).clone() for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)]


def _same_state(a, b, what):
    for x, y, n in zip(_state(a), _state(b), ("main", "target", "adam_m", "adam_v")):
        assert torch.equal(x, y), (what, n)


PLAN = [-1, 0 << 24 | 0, 1 << 24 | 0, -1, 0 << 24 | 1, 1 << 24 | 1, -1, 0 << 24 | 2]


def _fed_setup(ddrl, Ln, n_rings):
    """`n_rings` identical local window rings (200 windows, seed 9) and two owners' folded blocks (K = 3, 2) at batch 64."""
    B = 64
    opt = _opt(Ln=Ln, batch=B, cap=256)
    assert tuple(opt.hidden_sizes) == (400, 300)
    nfl = _nfloats(B, 8, 2)
    K = [3, 2]
    owners = [_ring(ddrl, opt, nf.windows(np.random.RandomState(s), 150, Ln, 8, 2, terminal="some"), seed=7 + s) for s in (1, 2)]
    blocks = [o.sample_many(B, k, torch.empty(k * nfl, dtype=torch.float32, device="cuda")) for o, k in zip(owners, K)]
    win = nf.windows(np.random.RandomState(0), 200, Ln, 8, 2, terminal="some")
    return opt, win, [_ring(ddrl, opt, win, 9) for _ in range(n_rings)], list(zip(blocks, K))


@pytest.mark.parametrize("n_upd", [8, 7])
def test_captured_loop_on_a_fed_window_ring_equals_eager(ddrl, n_upd):
    """ddrl_loop, two updates per graph (an eager update, whole graphs, an eager remainder where the count is even), following a plan on
    an Ln = 8 window ring == sample_nstep_device -> train_device, one at a time, on a twin ring following the same plan."""
    from distributed_drl_amd.agent import Learner
    from distributed_drl_amd.partition import _Loop
    opt, _, (ra, rb), regions = _fed_setup(ddrl, 8, 2)
    plan_d = torch.tensor(PLAN[:n_upd], dtype=torch.int32, device="cuda")
    la, lb = Learner(opt, job="learner", index=0), Learner(opt, job="learner", index=0)
    ra.set_feed(plan_d, 64, regions)
    rb.set_feed(plan_d, 64, regions)
    loop = _Loop(la, ra, 2)
    loop.run(n_upd)
    for _ in range(n_upd):
        lb.train_device(rb.sample_nstep_device(64))
    torch.cuda.synchronize()
    _same_state(la, lb, n_upd)
    assert la.opt_steps() == lb.opt_steps() == (n_upd, n_upd)
    assert ra.get_counts() == rb.get_counts() == (PLAN[:n_upd].count(-1), 200, 200)
    assert _fp(ra) == _fp(rb)


def test_fed_one_step_window_ring_equals_fed_transition_ring(ddrl):
    """Ln = 1 (the fold is the identity): the loop on a fed window ring == the loop on a fed transition ring holding the same rows, fed
    the same blocks."""
    from distributed_drl_amd.agent import Learner
    from distributed_drl_amd.partition import _Loop
    opt, win, (wr,), regions = _fed_setup(ddrl, 1, 1)
    tr = ddrl.ReplayBufferSAC1(8, 2, 256, seed=9)
    tr.store_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
                     (win["obs"][:, 0], win["acts"][:, 0], win["rews"][:, 0], win["obs"][:, 1], win["done"][:, 0])))
    plan_d = torch.tensor(PLAN[:7], dtype=torch.int32, device="cuda")
    learners = []
    for ring in (wr, tr):
        ring.set_feed(plan_d, 64, regions)
        L = Learner(opt, job="learner", index=0)
        loop = _Loop(L, ring, 2)
        loop.run(7)
        learners.append(L)
        del loop
    torch.cuda.synchronize()
    _same_state(learners[0], learners[1], "Ln 1")
    assert wr.get_counts() == tr.get_counts() == (PLAN[:7].count(-1), 200, 200)
    assert _fp(wr) == _fp(tr)


def test_data_parallel_pair_on_a_fed_window_ring_equals_the_fused_step(ddrl):
    """forward + backward with the next batch's sampler riding along (ddrl_sac1_compute_grads_and_sample) -> apply, and forward +
    backward -> apply with the sampler riding in the Adam kernel (ddrl_sac1_apply_grads_and_sample), on a fed window ring == the
    fused ddrl_sac1_step_and_sample sequence on its twin."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Learner
    lib = _lib.load()
    n_upd = 7
    opt, _, rings, regions = _fed_setup(ddrl, 8, 3)
    plan_d = torch.tensor(PLAN[:n_upd], dtype=torch.int32, device="cuda")
    nul = ctypes.c_void_p(None)
    learners = []
    for mode, ring in zip(("fused", "grads+sample", "apply+sample"), rings):
        ring.set_feed(plan_d, 64, regions)
        L = Learner(opt, job="learner", index=0)
        ins = []
        for st in range(2):
            bufs = (ctypes.c_void_p * 8)()
            _lib.check(lib.ddrl_sac1_input_buffers(L._h, st, bufs))
            ins.append([ctypes.c_void_p(bufs[i]) for i in range(8)])
        s, cur = _lib.stream_ptr(), 0
        _lib.check(lib.ddrl_replay_sample_nstep(ring._h, 64, float(L.cfg.gamma), *ins[0][:5], nul, s))
        for u in range(n_upd):
            last = u == n_upd - 1
            _lib.check(lib.ddrl_sac1_fill_noise(L._h, L._noise_seed, s))
            if mode == "fused":
                if last:   # (nothing is drawn ahead of the last update in any of the three)
                    _lib.check(lib.ddrl_sac1_step(L._h, *ins[cur], nul, nul, nul, nul, s))
                else:
                    _lib.check(lib.ddrl_sac1_step_and_sample(L._h, cur, ring._h, cur ^ 1, s))
            elif mode == "grads+sample" and not last:
                _lib.check(lib.ddrl_sac1_compute_grads_and_sample(L._h, cur, ring._h, cur ^ 1, s))
                _lib.check(lib.ddrl_sac1_grad_finalize(L._h, s))
                _lib.check(lib.ddrl_sac1_apply_grads(L._h, s))
            else:
                _lib.check(lib.ddrl_sac1_compute_grads(L._h, *ins[cur], nul, nul, nul, nul, s))
                _lib.check(lib.ddrl_sac1_grad_finalize(L._h, s))
                if last:
                    _lib.check(lib.ddrl_sac1_apply_grads(L._h, s))
                else:
                    _lib.check(lib.ddrl_sac1_apply_grads_and_sample(L._h, ring._h, cur ^ 1, s))
            cur ^= 1
        learners.append(L)
    torch.cuda.synchronize()
    for L, mode in zip(learners[1:], ("grads+sample", "apply+sample")):
        _same_state(learners[0], L, mode)
        assert L.opt_steps() == (n_upd, n_upd)
    for ring in rings:
        assert ring.get_counts() == (PLAN[:n_upd].count(-1), 200, 200) and _fp(ring) == _fp(rings[0])
