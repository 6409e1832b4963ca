"""GPU parity: HIP replay ring (through the C-ABI / Python surface) vs the oracle and the golden
vectors produced by the reference's own ReplayBuffer.  Bit-exact for indices, MT19937 state
and gathered float32 rows."""
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _fp(buf):
    key, pos = buf.mt_state()
    return {"pos": pos, "key_crc32": zlib.crc32(key.tobytes()), "key_head": [int(v) for v in key[:4]]}


def _cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_index_streams_golden(ddrl, golden_dir):
    """40 seed x size cases incl. size==1 (no draw consumed) and 4e6; stream carry-over."""
    from distributed_drl_amd import _lib
    z = np.load(os.path.join(golden_dir, "index_streams.npz"))
    meta = json.load(open(os.path.join(golden_dir, "index_streams.json")))
    cap = 4 * 10 ** 6
    buf = ddrl.ReplayBuffer(1, 1, cap)
    buf.rings()["rews_buf"].copy_(torch.arange(cap, dtype=torch.float32, device="cuda"))
    for m in meta:
        _lib.check(buf._lib.ddrl_replay_set_counts(buf._h, 0, m["size"], 0, 0, _lib.stream_ptr()))
        buf.seed(m["seed"])
        tag = "s%d_n%d" % (m["seed"], m["size"])
        a = buf.sample_batch_device(256, fresh=True, with_indices=True)
        np.testing.assert_array_equal(a["idxs"].cpu().numpy(), z[tag + "_a"].astype(np.int64), err_msg=tag)
        np.testing.assert_array_equal(a["rews"].cpu().numpy().astype(np.int64), z[tag + "_a"], err_msg=tag)
        assert _fp(buf) == m["after_256"], tag
        b = buf.sample_batch_device(100, fresh=True, with_indices=True)
        np.testing.assert_array_equal(b["idxs"].cpu().numpy(), z[tag + "_b"].astype(np.int64), err_msg=tag)
        assert _fp(buf) == m["after_100"], tag


def test_ring_states_and_gathers_golden(ddrl, golden_dir):
    from oracle.gen_golden import _transitions
    z = np.load(os.path.join(golden_dir, "ring_gather.npz"))
    meta = json.load(open(os.path.join(golden_dir, "ring_gather.json")))
    n_checked = 0
    for m in meta:
        if m["flavour"] not in ("dsac", "sac1"):
            continue
        cls = ddrl.ReplayBuffer if m["flavour"] == "dsac" else ddrl.ReplayBufferSAC1
        buf = cls(8, 2, m["cap"])
        for tr in _transitions(m["n"], 8, 2):  # per-transition store(), reference dtypes
            buf.store(*tr)
        tag = "%s_c%d_n%d" % (m["flavour"], m["cap"], m["n"])
        rings = buf.rings()
        for k in ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf"):
            np.testing.assert_array_equal(rings[k].cpu().numpy(), z[tag + "_" + k], err_msg=tag + k)
        assert (buf.ptr, buf.size) == (m["ptr"], m["size"])
        got = buf.get_counts()
        assert (list(got) if isinstance(got, tuple) else got) == m["counts_before"]
        buf.seed(7)
        for b in m["batches"]:
            d = buf.sample_batch(b["B"])
            for k, v in d.items():
                assert v.dtype == np.float32
                np.testing.assert_array_equal(v, z["%s_B%d_%s" % (tag, b["B"], k)], err_msg=tag)
            assert _fp(buf) == b["mt"]
        got = buf.get_counts()
        assert (list(got) if isinstance(got, tuple) else got) == m["counts_after"]
        n_checked += 1
    assert n_checked == 16


def test_dqn_shape_golden(ddrl, golden_dir, tmp_path):
    from oracle.gen_golden import _transitions
    z = np.load(os.path.join(golden_dir, "ring_gather.npz"))
    m = [m for m in json.load(open(os.path.join(golden_dir, "ring_gather.json"))) if m["flavour"] == "dqn"][0]

    class Opt:
        obs_dim, buffer_size, batch_size, save_dir = m["obs_dim"], m["cap"], m["B"], str(tmp_path)
    buf = ddrl.ReplayBufferDQN(Opt, 0)
    for tr in _transitions(m["n"], m["obs_dim"], 1, act_1d=True):
        buf.store(*tr, 3)
    rings = buf.rings()
    for k in ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf"):
        np.testing.assert_array_equal(rings[k].cpu().numpy(), z["dqn_c9_n13_" + k])
    buf.seed(m["seed"])
    d = buf.sample_batch()
    assert d["acts"].shape == (m["B"],)
    for k, v in d.items():
        np.testing.assert_array_equal(v, z["dqn_c9_n13_B5_" + k])
    assert list(buf.get_counts()) == m["counts_after"]
    assert _fp(buf) == m["mt"]
    # checkpoint round trip in the reference's .npy format (algos/dqn/train.py:82-108)
    buf.save()
    buf2 = ddrl.ReplayBufferDQN(Opt, 0)
    buf2.load()
    for k, t in buf2.rings().items():
        np.testing.assert_array_equal(t.cpu().numpy(), z["dqn_c9_n13_" + k])
    assert buf2.get_counts() == buf.get_counts() and buf2.ptr == buf.ptr
    infos = np.load(os.path.join(str(tmp_path), "checkpoint", "buffer_infos-0.npy"))
    assert list(infos) == [m["ptr"], m["size"], m["cap"], 13, 1]


def test_empty_buffer_raises_like_reference(ddrl):
    buf = ddrl.ReplayBuffer(8, 2, 5)
    with pytest.raises(ValueError) as e:
        buf.sample_batch(4)
    assert str(e.value) == "high <= 0"


@pytest.mark.parametrize("cap,chunks", [(1000, [1, 7, 992, 5, 1000, 999, 2500, 3]), (4096, [4096, 4096, 100]),
                                        (1000, [4, 5003, 1, 12007]), (7, [3, 100, 2])])
def test_store_batch_equals_sequential_store(ddrl, cap, chunks):
    """store_batch(n) == n sequential store() calls, incl. wrap inside a batch and n > capacity — also n many times the
    capacity with the cursor off zero (n = 5 cap + 3 at ptr = 4: the rows skipped at the front are unbounded)."""
    from oracle.replay_oracle import ReplayBufferOracle
    rs = np.random.RandomState(3)
    buf = ddrl.ReplayBufferSAC1(8, 2, cap)
    ora = ReplayBufferOracle(8, 2, cap)
    for n in chunks:
        o, o2 = rs.randn(n, 8).astype(np.float32), rs.randn(n, 8).astype(np.float32)
        a = rs.uniform(-1, 1, (n, 2)).astype(np.float32)
        r = rs.randn(n).astype(np.float32)
        d = (rs.rand(n) < 0.1).astype(np.float32)
        buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d)))
        ora.store_batch(o, a, r, o2, d)
        rings = buf.rings()
        for k in ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf"):
            np.testing.assert_array_equal(rings[k].cpu().numpy(), getattr(ora, k), err_msg="%s after n=%d" % (k, n))
        assert buf.get_counts() == ora.get_counts()
        assert buf.ptr == ora.ptr


def test_full_size_config2_sample_matches_oracle(ddrl):
    """BASELINE config 2 shape: 1M-transition ring, 4096-row stores, batch 256; indices and rows
    bit-exact vs the oracle over many consecutive batches (stream carry-over across twists)."""
    from oracle.replay_oracle import ReplayBufferOracle
    cap, n_env = 10 ** 6, 4096
    rs = np.random.RandomState(1234)
    buf = ddrl.ReplayBufferSAC1(8, 2, cap, seed=0)
    ora = ReplayBufferOracle(8, 2, cap, seed=0)
    # vectorised oracle fill (same result as sequential stores; checked above at small sizes)
    total = cap + 3 * n_env + 17
    o, o2 = rs.randn(total, 8).astype(np.float32), rs.randn(total, 8).astype(np.float32)
    a = rs.uniform(-1, 1, (total, 2)).astype(np.float32)
    r, d = rs.randn(total).astype(np.float32), (rs.rand(total) < 0.01).astype(np.float32)
    for s in range(0, total, n_env):
        e = min(s + n_env, total)
        buf.store_batch(*(torch.from_numpy(x[s:e]).cuda() for x in (o, a, r, o2, d)))
    dst = np.arange(total) % cap
    for name, src in (("obs1_buf", o), ("obs2_buf", o2), ("acts_buf", a), ("rews_buf", r), ("done_buf", d)):
        getattr(ora, name)[dst[-cap:]] = src[-cap:]
    ora.ptr, ora.size, ora.steps = total % cap, cap, total
    assert (buf.ptr, buf.size) == (ora.ptr, ora.size)
    for it in range(300):
        g = buf.sample_batch_device(256, with_indices=True)
        w = ora.sample_batch(256)
        np.testing.assert_array_equal(g["idxs"].cpu().numpy(), ora.last_idxs, err_msg="batch %d" % it)
        for k in ("obs1", "obs2", "acts", "rews", "done"):
            np.testing.assert_array_equal(g[k].cpu().numpy(), w[k])
    key, pos = buf.mt_state()
    assert pos == ora.rng.pos and (key == ora.rng.key).all()
    assert buf.get_counts() == ora.get_counts()


def test_large_row_gather_path(ddrl):
    """dqn pixel shape (config 5 row size, small capacity): non-fused index kernel + chip-wide
    gather; rows compared bit-exact; also the stand-alone gather with caller indices."""
    from oracle.replay_oracle import ReplayBufferOracle
    obs_dim, cap, B = 84 * 84 * 4, 96, 512

    class Opt:
        pass
    Opt.obs_dim, Opt.buffer_size, Opt.batch_size, Opt.save_dir = obs_dim, cap, B, "."
    buf = ddrl.ReplayBufferDQN(Opt, 0, seed=5)
    ora = ReplayBufferOracle(obs_dim, 1, cap, acts_1d=True, seed=5)
    rs = np.random.RandomState(0)
    n = 80
    o = rs.randint(0, 256, (n, obs_dim)).astype(np.float32)
    o2 = rs.randint(0, 256, (n, obs_dim)).astype(np.float32)
    a, r = rs.randint(0, 4, n).astype(np.float32), rs.randn(n).astype(np.float32)
    d = (rs.rand(n) < 0.1).astype(np.float32)
    buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d)))
    ora.store_batch(o, a, r, o2, d)
    for _ in range(3):
        g = buf.sample_batch_device(B, with_indices=True)
        w = ora.sample_batch(B)
        np.testing.assert_array_equal(g["idxs"].cpu().numpy(), ora.last_idxs)
        for k in ("obs1", "obs2", "acts", "rews", "done"):
            np.testing.assert_array_equal(g[k].cpu().numpy(), w[k])
    idx = torch.from_numpy(rs.randint(0, n, 77)).cuda()
    g = buf.gather_device(idx)
    np.testing.assert_array_equal(g["obs2"].cpu().numpy(), ora.obs2_buf[idx.cpu().numpy()])
    np.testing.assert_array_equal(g["acts"].cpu().numpy(), ora.acts_buf[idx.cpu().numpy()])


@pytest.mark.parametrize("with_indices", [False, True])
@pytest.mark.parametrize("B", [2047, 2048, 65537])
def test_wide_rows_draw_then_gather(ddrl, B, with_indices):
    """Rows too wide for the one-workgroup draw + gather (42 x 4 B x 2 per index: 2047 rows are 687 KB): the draw is a launch of its
    own — the 256-thread form below 2048 indices, the 640-thread form from 2048 on — behind it the row gather (the small-row form from
    4096 rows on); 65537 indices outgrow the handle's index scratch of 65536 when the caller passes no index buffer.  Indices, rows,
    MT19937 state and counters bit for bit those of the oracle."""
    from oracle.replay_oracle import ReplayBufferOracle
    obs_dim, cap, n = 40, 1000, 700
    buf, ora = ddrl.ReplayBufferSAC1(obs_dim, 2, cap, seed=11), ReplayBufferOracle(obs_dim, 2, cap, seed=11)
    rs = np.random.RandomState(B)
    o, o2 = rs.randn(n, obs_dim).astype(np.float32), rs.randn(n, obs_dim).astype(np.float32)
    a, r, d = rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32), (rs.rand(n) < 0.1).astype(np.float32)
    buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d)))
    for name, src in (("obs1_buf", o), ("obs2_buf", o2), ("acts_buf", a), ("rews_buf", r), ("done_buf", d)):
        getattr(ora, name)[:n] = src   # (n sequential stores into an empty ring of more than n rows)
    ora.ptr, ora.size, ora.steps = n, n, n
    for it in range(2):
        g = _cpu(buf.sample_batch_device(B, with_indices=with_indices))
        w = ora.sample_batch(B)
        if with_indices:
            np.testing.assert_array_equal(g["idxs"], ora.last_idxs, err_msg="draw %d" % it)
        for k in ("obs1", "obs2", "acts", "rews", "done"):
            np.testing.assert_array_equal(g[k], w[k], err_msg="draw %d %s" % (it, k))
    key, pos = buf.mt_state()
    assert pos == ora.rng.pos and (key == ora.rng.key).all()
    assert buf.get_counts() == ora.get_counts() == (2, n, n)


def test_parameter_server_golden(ddrl, golden_dir, tmp_path):
    import pickle
    log = json.load(open(os.path.join(golden_dir, "ps_trace.json")))
    keys = ["main/pi/dense/kernel", "main/pi/dense/bias", "main/q1/dense/kernel"]
    vals = [np.arange(6, dtype=np.float32).reshape(2, 3), np.ones(3, np.float32), np.full((2, 2), 7, np.float32)]
    ps = ddrl.ParameterServer(keys, vals)
    vals[0][0, 0] = 99.0
    assert [v.tolist() for v in ps.pull(log[0]["keys"])] == log[0]["out"]
    new = [np.full(3, 5, np.float32)]
    ps.push(keys[1:2], new)
    new[0][1] = -1.0
    assert [v.tolist() for v in ps.pull(log[1]["keys"])] == log[1]["out"]
    ps.push(["extra/key"], [np.zeros(1, np.float32)])
    assert list(ps.get_weights().keys()) == log[2]["out"]
    assert [v.tolist() for v in ps.pull(log[3]["keys"])] == log[3]["out"]
    ps.save_weights(str(tmp_path) + "/")
    w = pickle.load(open(str(tmp_path) + "/weights.pickle", "rb"))
    assert list(w.keys()) == log[2]["out"] and w[keys[1]].tolist() == [5.0, 5.0, 5.0]
    with pytest.raises(KeyError):
        ps.pull(["nope"])


def test_nstep_window_buffer_golden(ddrl, golden_dir):
    """N-step window ring (algos/sac1/sac_ray.py:34-82) on the generalised HIP ring: contents,
    wrap-around, counters and sampled windows bit-exact vs the reference's own class."""
    from oracle.gen_golden import nstep_windows
    z = np.load(os.path.join(golden_dir, "nstep.npz"))
    for m in json.load(open(os.path.join(golden_dir, "nstep.json"))):
        class Opt:
            obs_shape, act_shape, Ln = (m["obs"],), (), m["Ln"]
            buffer_size, batch_size, num_buffers = m["cap"], m["B"], m["num_buffers"]
        buf = ddrl.ReplayBufferNStep(Opt)
        for oq, aq in nstep_windows(m["n_store"], m["Ln"], m["obs"]):
            buf.store(oq, aq, 0)
        tag = "nstep_n%d" % m["n_store"]
        rings = buf.rings()
        for k in ("buffer_o", "buffer_a", "buffer_r", "buffer_d"):
            np.testing.assert_array_equal(rings[k].cpu().numpy(), z[tag + "_" + k], err_msg=k)
        buf.seed(m["seed"])
        for it in range(2):
            d = buf.sample_batch()
            for k, v in d.items():
                assert v.dtype == np.float32
                np.testing.assert_array_equal(v, z["%s_s%d_%s" % (tag, it, k)])
            assert _fp(buf) == m["mt"][it]
        assert list(buf.get_counts()) == m["counts"]
    # batched window store == sequential stores, incl. wrap inside the batch
    class Opt2:
        obs_shape, act_shape, Ln, buffer_size, batch_size, num_buffers = (8,), (2,), 8, 50, 16, 1
    b1, b2 = ddrl.ReplayBufferNStep(Opt2, seed=1), ddrl.ReplayBufferNStep(Opt2, seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    o = torch.randn(70, 9, 8, device="cuda", generator=g)
    a = torch.randn(70, 8, 2, device="cuda", generator=g)
    r, dn = torch.randn(70, 8, device="cuda", generator=g), torch.zeros(70, 8, device="cuda")
    b1.store_batch(o, a, r, dn)
    for i in range(70):
        b2.store_batch(o[i:i + 1], a[i:i + 1], r[i:i + 1], dn[i:i + 1])
    for k, v in b1.rings().items():
        assert torch.equal(v, b2.rings()[k]), k
    s1, s2 = b1.sample_batch_device(with_indices=True), b2.sample_batch_device(with_indices=True)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert s1["obs"].shape == (16, 9, 8) and s1["acts"].shape == (16, 8, 2)
    assert b1.get_counts() == (1, 70, 50)


def _filled(ddrl, seed, n=3000, cap=4096, obs=8, act=2, data_seed=0):
    rs = np.random.RandomState(data_seed)
    rb = ddrl.ReplayBufferSAC1(obs, act, cap, seed=seed)
    rb.store_batch(*(torch.from_numpy(x).cuda() for x in (
        rs.randn(n, obs).astype(np.float32), rs.uniform(-1, 1, (n, act)).astype(np.float32), np.arange(n, dtype=np.float32),
        rs.randn(n, obs).astype(np.float32), (rs.rand(n) < 0.1).astype(np.float32))))
    return rb


def _packed(b):
    return np.concatenate([b[k].reshape(-1).cpu().numpy() for k in ("obs1", "obs2", "acts", "rews", "done")])


@pytest.mark.parametrize("B,K", [(256, 9), (100, 5), (33, 4)])
def test_sample_many_equals_consecutive_sample_batches(ddrl, B, K):
    """The block a shard owner sends for one step (ddrl_replay_sample_many) = K consecutive sample_batch(B) calls: same
    indices (NumPy's stream), same rows, same counters, same sampler state afterwards."""
    a, b = _filled(ddrl, 42), _filled(ddrl, 42)
    nf = B * (2 * 8 + 2 + 2)
    flat = torch.empty(K * nf, dtype=torch.float32, device="cuda")
    blk = a.sample_many(B, K, flat).cpu().numpy()
    np.random.seed(42)
    idx = np.random.randint(0, 3000, B * K)
    np.testing.assert_array_equal(blk[K * B * 18: K * B * 19].astype(np.int64), idx)   # rews carry the ring row number
    seq = [_packed(b.sample_batch_device(B, fresh=True)) for _ in range(K)]
    for cum, w in ((0, 8), (8, 8), (16, 2), (18, 1), (19, 1)):      # array j of the block is [K * B, w]: batch i = rows [i B, (i + 1) B)
        for i in range(K):
            np.testing.assert_array_equal(blk[K * B * cum + i * B * w: K * B * cum + (i + 1) * B * w], seq[i][B * cum: B * cum + B * w])
    assert a.get_counts() == b.get_counts() == (K, 3000, 3000)
    assert _fp(a) == _fp(b)


def test_feed_plan_interleaves_remote_blocks_with_local_draws(ddrl):
    """The learner side of the sharded replay (ddrl_replay_set_feed): plan entry -1 draws from the local ring exactly as
    if the remote updates were not there; entry r << 24 | i returns batch i of region r bit for bit and consumes no local
    draw; the plan restarts with every set_feed; detaching restores the plain sampler."""
    B = 64
    nf = B * 20
    owners = [_filled(ddrl, 7, data_seed=1), _filled(ddrl, 8, data_seed=2)]
    K = [5, 3]
    blocks = [o.sample_many(B, k, torch.empty(k * nf, dtype=torch.float32, device="cuda")) for o, k in zip(owners, K)]
    local, twin = _filled(ddrl, 9), _filled(ddrl, 9)
    plan = [-1, 0 << 24 | 0, 1 << 24 | 0, -1, -1, 0 << 24 | 1, 1 << 24 | 1, 0 << 24 | 2, -1, 1 << 24 | 2, 0 << 24 | 3, 0 << 24 | 4]
    plan_d = torch.tensor(plan, dtype=torch.int32, device="cuda")
    for rep in range(2):
        local.set_feed(plan_d, B, list(zip(blocks, K)))
        for p in plan:
            got = _packed(local.sample_batch_device(B, fresh=True))
            if p < 0:
                want = _packed(twin.sample_batch_device(B, fresh=True))
            else:
                r, i = p >> 24, p & 0xffffff
                blk, k = blocks[r].cpu().numpy(), K[r]
                want = np.concatenate([blk[o * k * B + i * B * w: o * k * B + (i + 1) * B * w] for o, w in ((0, 8), (8, 8), (16, 2), (18, 1), (19, 1))])
            np.testing.assert_array_equal(got, want, err_msg="rep %d entry %d" % (rep, p))
        assert _fp(local) == _fp(twin)
    # beyond the plan's end: local draws
    np.testing.assert_array_equal(_packed(local.sample_batch_device(B, fresh=True)), _packed(twin.sample_batch_device(B, fresh=True)))
    # sample_times counts local draws only (the owners counted the fed batches)
    assert local.get_counts()[0] == twin.get_counts()[0] == 2 * plan.count(-1) + 1
    local.set_feed(None, B, [])
    np.testing.assert_array_equal(_packed(local.sample_batch_device(B, fresh=True)), _packed(twin.sample_batch_device(B, fresh=True)))
    # an empty one-row ring that only follows a plan (a dedicated learner rank): fed batches come through, a local entry
    # reports the reference's empty-buffer error
    ghost = ddrl.ReplayBufferSAC1(8, 2, 1)
    ghost.set_feed(torch.tensor([1 << 24 | 1], dtype=torch.int32, device="cuda"), B, list(zip(blocks, K)))
    got = _packed(ghost.sample_batch_device(B, fresh=True))
    blk = blocks[1].cpu().numpy()
    np.testing.assert_array_equal(got[:B * 8], blk[B * 8: 2 * B * 8])
    # the ghost's second call has no plan entry left -> a local draw from the empty ring: the launch itself cannot fail
    # (it may be a graph node), the next look at the counters raises the reference's error and clears it
    ghost.sample_batch_device(B, fresh=True)
    with pytest.raises(ValueError, match="high <= 0"):
        ghost.get_counts()
    assert ghost.get_counts() == (0, 0, 0)


def test_bad_feed_plan_entry_is_reported_not_swallowed(ddrl):
    """A plan entry that names a batch / region the step does not have leaves the output untouched on the device — the
    host must hear about it: ddrl_replay_counts returns the sticky error once, ddrl_replay_take_error moves it without
    a sync."""
    B, nf = 64, 64 * 20
    owner = _filled(ddrl, 7, data_seed=1)
    blk = owner.sample_many(B, 3, torch.empty(3 * nf, dtype=torch.float32, device="cuda"))
    local = _filled(ddrl, 9)
    for bad in (0 << 24 | 3, 1 << 24 | 0):                      # batch index == count; region index == n_regions
        local.set_feed(torch.tensor([bad], dtype=torch.int32, device="cuda"), B, [(blk, 3)])
        local.sample_batch_device(B, fresh=True)
        with pytest.raises(ValueError, match="feed-plan"):
            local.get_counts()
        local.get_counts()                                       # cleared
    local.set_feed(torch.tensor([0 << 24 | 2], dtype=torch.int32, device="cuda"), B + 1, [(blk, 3)])   # plan laid for another batch size
    local.sample_batch_device(B, fresh=True)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    local.take_error(word)
    assert int(word.item()) == -1
    local.take_error(word)
    assert int(word.item()) == 0
    local.get_counts()


@pytest.mark.parametrize("obs,act,B,K", [(3, 4, 5, 3), (3, 4, 33, 1), (4, 4, 7, 3), (5, 8, 4097, 1)])
def test_packed_blocks_at_unaligned_float_offsets(ddrl, obs, act, B, K):
    """sample_many packs the arrays back to back: an array whose width is a multiple of 4 can start at a float offset
    that is not (obs 3, act 4, K*B odd -> acts at 6 K B floats) — the gathers must not assume 16-byte alignment.  Rows
    checked against the ring at NumPy's own indices; K*B >= 4096 takes the many-small-rows gather."""
    n = 3000
    a = _filled(ddrl, 11, n=n, obs=obs, act=act)
    nf = B * (2 * obs + act + 2)
    base = torch.empty(K * nf + 1, dtype=torch.float32, device="cuda")
    for shift in (0, 1):                                         # shift 1: every array base off by 4 bytes as well
        a.seed(11)
        blk = a.sample_many(B, K, base[shift:shift + K * nf]).cpu().numpy()
        np.random.seed(11)
        idx = np.random.randint(0, n, B * K)
        g, off = a.rings(), 0
        for name, w in (("obs1_buf", obs), ("obs2_buf", obs), ("acts_buf", act), ("rews_buf", 1), ("done_buf", 1)):
            want = g[name].cpu().numpy().reshape(-1, w)[idx].reshape(-1)
            np.testing.assert_array_equal(blk[off: off + K * B * w], want, err_msg="%s shift %d" % (name, shift))
            off += K * B * w


def test_config5_rows_beyond_4gib_byte_offsets(ddrl):
    """Config 5's row shape (84 x 84 x 4 float32 = 112 896 B per observation) on a ring whose observation arrays pass 2^32
    BYTES (42 000 rows = 4.7 GB each; one MI355X holds ~1.2 M such transitions): store with wrap, NumPy's own index stream
    over the whole ring, gathered rows == ring rows at those indices, and caller-supplied indices in the rows beyond the
    4 GiB mark.  Every row is recognisable: obs1[i, c] = (i * 31 + c) mod 2^20, obs2[i, c] = obs1[i, c] + 0.5."""
    obs_dim, cap, B = 84 * 84 * 4, 42000, 512
    assert cap * obs_dim * 4 > 2 ** 32 + 2 ** 28

    class Opt:
        pass
    Opt.obs_dim, Opt.buffer_size, Opt.batch_size, Opt.save_dir = obs_dim, cap, B, "."
    buf = ddrl.ReplayBufferDQN(Opt, 0, seed=12345)
    cols = torch.arange(obs_dim, device="cuda", dtype=torch.int64)

    def rows_of(first, n):   # what source row `first + j` of the store stream holds
        i = torch.arange(first, first + n, device="cuda", dtype=torch.int64)
        x = ((i[:, None] * 31 + cols[None, :]) % (1 << 20)).float()
        return x, (i % 7).float(), (i % 1000).float() * 0.25, x + 0.5, (i % 97 == 0).float()
    total, chunk = cap + 4000, 2000          # 46 000 stores: the last 4 000 wrap over rows 0 .. 3 999
    for s in range(0, total, chunk):
        buf.store_batch(*rows_of(s, chunk))
    assert buf.get_counts() == (0, total, cap) and buf.ptr == total - cap
    src = lambda idx: np.where(idx < total - cap, idx + cap, idx)          # the store-stream row that ring row idx holds now

    def check(g, idx):
        first = torch.from_numpy(src(idx)).cuda()
        want1 = ((first[:, None] * 31 + cols[None, :]) % (1 << 20)).float()
        assert torch.equal(g["obs1"], want1) and torch.equal(g["obs2"], want1 + 0.5)
        assert torch.equal(g["acts"], (first % 7).float()) and torch.equal(g["rews"], (first % 1000).float() * 0.25)
        assert torch.equal(g["done"], (first % 97 == 0).float())
    np.random.seed(12345)
    for _ in range(3):       # sample_batch: MT19937 index kernel + the chip-wide gather
        g = buf.sample_batch_device(B, fresh=True, with_indices=True)
        idx = np.random.randint(0, cap, B)
        np.testing.assert_array_equal(g["idxs"].cpu().numpy(), idx)
        assert (idx.astype(np.int64) * obs_dim * 4 >= 2 ** 32).sum() > 10     # rows beyond the 4 GiB mark were drawn
        check(g, idx)
    hi = np.concatenate([np.arange(cap - 300, cap), [38043, 38044, 2 ** 32 // (obs_dim * 4), 2 ** 32 // (obs_dim * 4) + 1]]).astype(np.int64)
    check(buf.gather_device(torch.from_numpy(hi).cuda()), hi)                # ddrl_replay_gather at the far end of the arrays
    del buf
    torch.cuda.empty_cache()


# ---- the opt-in compact (uint8) ring for integer-valued pixel observations: config 5 at its stated capacity ----------------
class _PixOpt:
    def __init__(self, cap, obs_dim=84 * 84 * 4, B=512, save_dir="."):
        self.obs_dim, self.buffer_size, self.batch_size, self.save_dir = obs_dim, cap, B, save_dir


def _pixel_transitions(rs, n, obs_dim):
    o = rs.randint(0, 256, (n, obs_dim)).astype(np.float32)
    o2 = rs.randint(0, 256, (n, obs_dim)).astype(np.float32)
    return o, rs.randint(0, 4, n).astype(np.float32), rs.randn(n).astype(np.float32), o2, (rs.rand(n) < 0.1).astype(np.float32)


@pytest.mark.parametrize("obs_dim,cap", [(84 * 84 * 4, 40), (50, 9), (64, 300)])
def test_compact_ring_is_bit_identical_to_the_float32_ring(ddrl, tmp_path, obs_dim, cap):
    """Same stores (wrap, a batch larger than the capacity), same seed: index streams, gathered batches, ring contents, counters
    and the .npy checkpoint of the compact ring equal the float32 ring's bit for bit — and both equal the oracle.  Row widths that
    are / are not whole 16-element groups (the vector and the scalar conversion paths)."""
    from oracle.replay_oracle import ReplayBufferOracle
    rs = np.random.RandomState(3)
    f32 = ddrl.ReplayBufferDQN(_PixOpt(cap, obs_dim, 32, str(tmp_path / "f")), 0, seed=7)
    u8 = ddrl.ReplayBufferDQN(_PixOpt(cap, obs_dim, 32, str(tmp_path / "u")), 0, seed=7, compact_obs=True)
    ora = ReplayBufferOracle(obs_dim, 1, cap, acts_1d=True, seed=7)
    assert u8.compact_obs and not f32.compact_obs
    for n in (cap - 3, 7, 2 * cap + 5, 1):
        tr = _pixel_transitions(rs, n, obs_dim)
        o, a, r, o2, d = tr
        for b in (f32, u8):
            b.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d)))
        ora.store_batch(o, a, r, o2, d)
        for B in (32, 5):
            g1, g2, w = f32.sample_batch_device(B, with_indices=True), u8.sample_batch_device(B, with_indices=True), ora.sample_batch(B)
            np.testing.assert_array_equal(g2["idxs"].cpu().numpy(), ora.last_idxs)
            for k in ("obs1", "obs2", "acts", "rews", "done", "idxs"):
                assert torch.equal(g1[k], g2[k]), k
            for k in w:
                np.testing.assert_array_equal(g2[k].cpu().numpy(), w[k])
    r1, r2 = f32.rings(), u8.rings()
    for k in r1:
        assert r2[k].dtype == torch.float32 and torch.equal(r1[k], r2[k]), k
    np.testing.assert_array_equal(r2["obs2_buf"].cpu().numpy(), ora.obs2_buf)
    assert u8.get_counts() == f32.get_counts() == ora.get_counts()
    idx = torch.from_numpy(rs.randint(0, cap, 11)).cuda()
    assert torch.equal(u8.gather_device(idx)["obs1"], f32.gather_device(idx)["obs1"])
    # checkpoint: float32 .npy files in the reference's format (algos/dqn/train.py:82-108), identical bytes, and each loads into the other kind
    f32.save(); u8.save()
    for name in ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf", "buffer_infos"):
        a, b = np.load(tmp_path / "f" / "checkpoint" / ("%s-0.npy" % name)), np.load(tmp_path / "u" / "checkpoint" / ("%s-0.npy" % name))
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    back = ddrl.ReplayBufferDQN(_PixOpt(cap, obs_dim, 32, str(tmp_path / "f")), 0, seed=1, compact_obs=True)
    back.load()
    for k, t in back.rings().items():
        assert torch.equal(t, r1[k]), k
    assert back.get_counts() == f32.get_counts()


def test_compact_ring_refuses_values_it_cannot_hold(ddrl):
    """The compact ring is lossless or loud: a fractional, negative, > 255 or NaN observation raises at the next look at the ring."""
    for bad in (0.5, -1.0, 256.0, float("nan")):
        buf = ddrl.ReplayBufferDQN(_PixOpt(8, 48, 4), 0, seed=0, compact_obs=True)
        o = np.full((3, 48), 7.0, np.float32)
        z = np.zeros(3, np.float32)
        buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, z, z, o, z)))
        buf.check()
        o[1, 17] = bad
        buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, z, z, o, z)))
        with pytest.raises(ValueError, match="not an integer in"):
            buf.check()
        buf.check()   # reported once, then cleared


def test_config5_ring_at_its_stated_capacity_of_4m_transitions(ddrl):
    """BASELINE config 5: a 4 M-transition replay of 84x84x4 observations (algos/dqn/train.py:43-52; 903 GB as float32) on ONE MI355X
    as the compact ring (225.8 GB of uint8 observations).  Rows at the far end of the arrays (byte offsets beyond 100 GB), the wrap
    at 4 M, and sample_batch(512) over the full ring against NumPy's own index stream."""
    free_b, _ = torch.cuda.mem_get_info()
    cap, obs_dim = 4 * 10 ** 6, 84 * 84 * 4
    need = 2 * cap * obs_dim + 12 * cap + (2 << 30)
    if free_b < need:
        pytest.skip("needs %.0f GB of free HBM, %.0f free" % (need / 1e9, free_b / 1e9))
    buf = ddrl.ReplayBufferDQN(_PixOpt(cap), 0, seed=123, compact_obs=True)
    rs = np.random.RandomState(8)
    n = 600
    o, a, r, o2, d = _pixel_transitions(rs, n, obs_dim)
    from distributed_drl_amd import _lib
    _lib.check(buf._lib.ddrl_replay_set_counts(buf._h, cap - 400, cap - 400, cap - 400, 0, _lib.stream_ptr()))   # cursor 400 rows before the end
    buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d)))             # rows cap-400 .. cap-1, then 0 .. 199
    assert buf.get_counts() == (0, cap + 200, cap) and buf.ptr == 200
    np.testing.assert_array_equal(buf.rows(0, cap - 400, 400).cpu().numpy(), o[:400])
    np.testing.assert_array_equal(buf.rows(1, 0, 200).cpu().numpy(), o2[400:])
    g = buf.sample_batch_device(512, with_indices=True)
    want = np.random.RandomState(123).randint(0, cap, 512)
    np.testing.assert_array_equal(g["idxs"].cpu().numpy(), want)
    idx = g["idxs"].cpu().numpy()
    hit = np.nonzero((idx >= cap - 400) | (idx < 200))[0]
    for b in hit:   # (a 512-draw over 4 M rows rarely lands in the 600 stored ones; gather_device below makes sure some do)
        row = idx[b] - (cap - 400) if idx[b] >= cap - 400 else idx[b] + 400
        np.testing.assert_array_equal(g["obs1"][b].cpu().numpy(), o[row])
    sel = torch.tensor([cap - 1, cap - 400, 0, 199, cap // 2], device="cuda")
    gg = buf.gather_device(sel)
    np.testing.assert_array_equal(gg["obs1"][:4].cpu().numpy(), o[[399, 0, 400, 599]])
    np.testing.assert_array_equal(gg["obs2"][:4].cpu().numpy(), o2[[399, 0, 400, 599]])
    assert float(gg["obs1"][4].abs().max()) == 0.0
    np.testing.assert_array_equal(gg["rews"][:4].cpu().numpy(), r[[399, 0, 400, 599]])
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_interleaving_of_stores_and_samples(ddrl, tmp_path, seed):
    """Seeded fuzz of the ring's whole surface: a random walk of store_batch (1 row .. several capacities, so every wrap position and
    cursor alignment occurs), single-row store, sample_batch of random sizes (1 .. 700: both gather paths, the index kernel across MT19937
    state refills) and get_counts, on the SAC shape and on the DQN shape as float32 and compact rings at once — after every operation
    the sampled indices, the gathered batches, the counters and (every tenth operation) the whole ring equal the oracle's.
    DDRL_FUZZ_N scales the walk, DDRL_FUZZ_SEED moves it."""
    import os
    from oracle.replay_oracle import ReplayBufferOracle
    seed += 1000 * int(os.environ.get("DDRL_FUZZ_SEED", "0"))
    rs = np.random.RandomState(seed)
    n_ops = 40 * max(1, int(os.environ.get("DDRL_FUZZ_N", "6")) // 6)
    cap = int(rs.choice([5, 64, 1000, 3001]))
    obs_dim = int(rs.choice([8, 11, 48]))
    sac, sac_o = ddrl.ReplayBufferSAC1(obs_dim, 2, cap, seed=seed), ReplayBufferOracle(obs_dim, 2, cap, seed=seed)
    pix = [ddrl.ReplayBufferDQN(_PixOpt(cap, obs_dim, 32, str(tmp_path / k)), 0, seed=seed, compact_obs=(k == "u")) for k in ("f", "u")]
    pix_o = ReplayBufferOracle(obs_dim, 1, cap, acts_1d=True, seed=seed)
    dev = lambda xs: tuple(torch.from_numpy(x).cuda() for x in xs)
    for op in range(n_ops):
        kind = rs.rand()
        if kind < 0.45 or sac_o.size == 0:
            n = int(rs.choice([1, 1, 3, cap - 1 if cap > 1 else 1, cap, cap + 1, 2 * cap + 3, int(rs.randint(1, 2 * cap + 2))]))
            o, o2 = rs.randn(n, obs_dim).astype(np.float32), rs.randn(n, obs_dim).astype(np.float32)
            a, r, d = rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32), (rs.rand(n) < 0.1).astype(np.float32)
            if n == 1 and rs.rand() < 0.5:
                # the reference's own call shape (host values) in the guises a worker hands them over: arrays, float64, lists, Python /
                # NumPy scalars and bools — everything lands as the float32 the NumPy row assignment makes of it
                form = rs.randint(0, 4)
                if form == 0:
                    sac.store(o[0], a[0], r[0], o2[0], d[0])
                elif form == 1:
                    sac.store(o[0].astype(np.float64), a[0].astype(np.float64), float(r[0]), o2[0].astype(np.float64), bool(d[0]))
                elif form == 2:
                    sac.store(o[0].tolist(), a[0].tolist(), np.float64(r[0]), tuple(o2[0].tolist()), np.bool_(d[0]))
                else:
                    sac.store(o[0], a[0], np.float32(r[0]), o2[0], int(d[0]))
            else:
                sac.store_batch(*dev((o, a, r, o2, d)))
            sac_o.store_batch(o, a, r, o2, d)
            tr = _pixel_transitions(rs, n, obs_dim)
            for b in pix:
                b.store_batch(*dev(tr))
            pix_o.store_batch(*tr)
        else:
            B = int(rs.choice([1, 32, 256, 257, int(rs.randint(1, 701))]))
            got, want = sac.sample_batch_device(B, with_indices=True), sac_o.sample_batch(B)
            np.testing.assert_array_equal(got["idxs"].cpu().numpy(), sac_o.last_idxs, err_msg="op %d" % op)
            for k in want:
                np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg="op %d %s" % (op, k))
            want = pix_o.sample_batch(B)
            for b in pix:
                got = b.sample_batch_device(B, with_indices=True)
                np.testing.assert_array_equal(got["idxs"].cpu().numpy(), pix_o.last_idxs, err_msg="op %d" % op)
                for k in want:
                    np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg="op %d %s" % (op, k))
        assert sac.get_counts() == sac_o.get_counts() and sac.ptr == sac_o.ptr
        assert pix[0].get_counts() == pix[1].get_counts() == pix_o.get_counts()
        if op % 10 == 9 or op == n_ops - 1:
            for k, t in sac.rings().items():
                np.testing.assert_array_equal(t.cpu().numpy(), getattr(sac_o, k), err_msg="op %d %s" % (op, k))
            for b in pix:
                for k, t in b.rings().items():
                    np.testing.assert_array_equal(t.cpu().numpy(), getattr(pix_o, k), err_msg="op %d %s" % (op, k))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_parameter_server_random_walk(ddrl, seed):
    """Seeded fuzz of the server's surface against the oracle (example/dsac.py:51-73): pushes of random key subsets in random order —
    new keys, changed shapes, float64 / int values, the flat device path — interleaved with pulls and get_weights; values, dtypes of
    what comes back, key order and the snapshot-by-copy rule after every operation."""
    from oracle.replay_oracle import ParameterServerOracle
    rs = np.random.RandomState(seed)
    names = ["main/pi/dense/kernel", "main/pi/dense/bias", "main/q1/dense/kernel", "main/q1/dense/bias", "main/q2/dense_2/kernel"]
    shapes = [(8, 5), (5,), (10, 5), (5,), (5, 1)]
    vals = [rs.randn(*s).astype(np.float32) for s in shapes]
    ps, ora = ddrl.ParameterServer(names, vals), ParameterServerOracle(names, vals)
    known = list(names)
    for op in range(60):
        r = rs.rand()
        if r < 0.45:
            ks = [known[i] for i in rs.permutation(len(known))[:rs.randint(1, len(known) + 1)]]
            if rs.rand() < 0.2:
                ks.append("extra/%d" % op)
                known.append(ks[-1])
            new = []
            for k in ks:
                shape = ora.weights[k].shape if k in ora.weights and rs.rand() < 0.9 else (int(rs.randint(1, 7)),)
                v = rs.randn(*shape)
                new.append(v.astype(np.float32) if rs.rand() < 0.8 else v)          # float64 comes in now and then (cast like the NumPy assignment)
            ps.push(ks, new)
            ora.push(ks, [np.asarray(v, np.float32) for v in new])
            for v in new:
                v += 1.0                                                           # the caller's arrays may change afterwards: push snapshots by copy
        elif r < 0.9:
            ks = [known[i] for i in rs.permutation(len(known))[:rs.randint(1, len(known) + 1)]]
            got, want = ps.pull(ks), ora.pull(ks)
            assert len(got) == len(want)
            for g, w, k in zip(got, want, ks):
                assert g.dtype == np.float32 and g.shape == w.shape, k
                np.testing.assert_array_equal(g, w, err_msg="op %d %s" % (op, k))
            got[0][...] = -7.0                                                     # ... and pull hands out copies
            np.testing.assert_array_equal(ps.pull(ks[:1])[0], want[0])
        else:
            w = ps.get_weights()
            assert list(w.keys()) == list(ora.get_weights().keys())
            for k in w:
                np.testing.assert_array_equal(w[k], ora.weights[k], err_msg="op %d %s" % (op, k))
        if op % 7 == 6:
            # the learner's one-copy path (TrainDevice.push): the whole vector of the ORIGINAL layout lands on the flat buffer = a push of
            # every original key at its original shape (a key that had changed shape in between must come back with it)
            flat = rs.randn(sum(int(np.prod(s_)) for s_ in shapes)).astype(np.float32)
            v0 = ps.version
            ps.push_flat(torch.from_numpy(flat).cuda())
            assert ps.version > v0
            off = 0
            for k, s_ in zip(names, shapes):
                n = int(np.prod(s_))
                cur = ora.weights[k].shape                     # a same-size reshape pushed earlier keeps its shape on both sides
                ora.push([k], [flat[off:off + n].reshape(cur if int(np.prod(cur)) == n else s_)])
                off += n
            assert ps.span(names) == (0, flat.size)


def test_parameter_server_versions_cover_late_keys_and_reshaped_keys(ddrl):
    """a push that only touches late-comer keys / keys whose shape changed is still a new version (RolloutDevice.pull looks at
    the version), a reshaped key leaves the contiguous span (layout bump) and comes back with the learner's next flat push."""
    names, shapes = ["main/pi/dense/kernel", "main/pi/dense/bias"], [(8, 5), (5,)]
    ps = ddrl.ParameterServer(names, [np.ones(s, np.float32) for s in shapes])
    v, lay = ps.version, ps.layout
    ps.push(["late/key"], [np.arange(3, dtype=np.float32)])
    assert ps.version == v + 1 and ps.layout == lay
    ps.push(["main/pi/dense/bias"], [np.arange(7, dtype=np.float32)])          # another shape under an old key
    assert ps.version == v + 2 and ps.layout == lay + 1 and ps.span(names) is None
    np.testing.assert_array_equal(ps.pull(["main/pi/dense/bias"])[0], np.arange(7, dtype=np.float32))
    flat = np.arange(45, dtype=np.float32)
    ps.push_flat(torch.from_numpy(flat).cuda())
    assert ps.span(names) == (0, 45) and ps.layout == lay + 2
    np.testing.assert_array_equal(ps.pull(["main/pi/dense/bias"])[0], flat[40:])
    assert list(ps.get_weights().keys()) == names + ["late/key"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_nstep_ring_random_walk(ddrl, seed):
    """Seeded fuzz of the n-step window ring (algos/sac1/sac_ray.py:34-82) against the oracle: single-window stores out of deques,
    batched stores (wrap inside the batch, more windows than slots), masked stores (the vectorised rollout's form: rows with mask != 0,
    in row order), sample_batch and get_counts interleaved; several buffers' worth of counter increments (num_buffers)."""
    from oracle.replay_oracle import NStepReplayOracle
    rs = np.random.RandomState(seed)

    class Opt:
        obs_shape, act_shape = (int(rs.choice([3, 8])),), (int(rs.choice([1, 2])),)
        Ln, buffer_size, batch_size, num_buffers = int(rs.choice([1, 4, 8])), int(rs.choice([7, 50, 333])), int(rs.choice([1, 16, 40])), int(rs.choice([1, 3]))
    buf, ora = ddrl.ReplayBufferNStep(Opt, seed=seed), NStepReplayOracle(Opt, seed=seed)
    Ln, od, ad = Opt.Ln, Opt.obs_shape[0], Opt.act_shape[0]

    def windows(n):
        return (rs.randn(n, Ln + 1, od).astype(np.float32), rs.uniform(-1, 1, (n, Ln, ad)).astype(np.float32), rs.randn(n, Ln).astype(np.float32),
                (rs.rand(n, Ln) < 0.1).astype(np.float32))

    def ora_store(o, a, r, d, rows):
        for i in rows:
            ora.store([(o[i, k],) for k in range(Ln + 1)], [(a[i, k], r[i, k], d[i, k]) for k in range(Ln)], 0)

    for op in range(60):
        kind = rs.rand()
        if kind < 0.2 or ora.size == 0:
            o, a, r, d = windows(1)
            buf.store([(o[0, k],) for k in range(Ln + 1)], [(a[0, k], r[0, k], bool(d[0, k])) for k in range(Ln)], 0)
            ora_store(o, a, r, d, [0])
        elif kind < 0.45:
            n = int(rs.choice([1, 2, Opt.buffer_size - 1 if Opt.buffer_size > 1 else 1, Opt.buffer_size + 3, int(rs.randint(1, 2 * Opt.buffer_size))]))
            o, a, r, d = windows(n)
            buf.store_batch(*(torch.from_numpy(x).cuda() for x in (o, a, r, d)))
            ora_store(o, a, r, d, range(n))
        elif kind < 0.65:
            n = int(rs.randint(1, 100))
            o, a, r, d = windows(n)
            mask = (rs.rand(n) < 0.4).astype(np.uint8)
            buf.store_masked(*(torch.from_numpy(x).cuda() for x in (o, a, r, d)), torch.from_numpy(mask).cuda())
            ora_store(o, a, r, d, np.nonzero(mask)[0])
        else:
            got, want = buf.sample_batch(), ora.sample_batch()
            for k in want:
                np.testing.assert_array_equal(got[k], want[k], err_msg="op %d %s" % (op, k))
        assert buf.get_counts() == ora.get_counts(), op
        if op % 10 == 9:
            rings = buf.rings()
            for k in ("buffer_o", "buffer_a", "buffer_r", "buffer_d"):
                np.testing.assert_array_equal(rings[k].cpu().numpy().reshape(getattr(ora, k).shape), getattr(ora, k), err_msg="op %d %s" % (op, k))


def test_masked_store_of_more_rows_than_slots_from_a_cursor_off_zero(ddrl):
    """One masked store that selects 33 of 40 windows for a ring of 7 slots whose cursor stands at 5: the selected rows that a later one
    of the same batch overwrites are skipped inside the launch, the last 7 land behind the cursor in row order, and the cursor commit
    counts all 33."""
    from oracle.replay_oracle import NStepReplayOracle
    rs = np.random.RandomState(4)

    class Opt:
        obs_shape, act_shape = (3,), (1,)
        Ln, buffer_size, batch_size, num_buffers = 2, 7, 4, 1
    buf, ora = ddrl.ReplayBufferNStep(Opt, seed=2), NStepReplayOracle(Opt, seed=2)

    def windows(n):
        return (rs.randn(n, 3, 3).astype(np.float32), rs.uniform(-1, 1, (n, 2, 1)).astype(np.float32), rs.randn(n, 2).astype(np.float32),
                (rs.rand(n, 2) < 0.1).astype(np.float32))

    def ora_store(o, a, r, d, rows):
        for i in rows:
            ora.store([(o[i, k],) for k in range(3)], [(a[i, k], r[i, k], d[i, k]) for k in range(2)], 0)

    w = windows(5)
    buf.store_batch(*(torch.from_numpy(x).cuda() for x in w))
    ora_store(*w, range(5))
    w = windows(40)
    mask = np.ones(40, dtype=np.uint8)
    mask[[0, 3, 9, 17, 18, 30, 39]] = 0
    assert mask.sum() == 33
    buf.store_masked(*(torch.from_numpy(x).cuda() for x in w), torch.from_numpy(mask).cuda())
    ora_store(*w, np.nonzero(mask)[0])
    assert buf.get_counts() == ora.get_counts() == (0, 38, 7)
    assert buf._counts()[0] == ora.ptr == 38 % 7
    rings = buf.rings()
    for k in ("buffer_o", "buffer_a", "buffer_r", "buffer_d"):
        np.testing.assert_array_equal(rings[k].cpu().numpy().reshape(getattr(ora, k).shape), getattr(ora, k), err_msg=k)
    got, want = buf.sample_batch(), ora.sample_batch()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_prefetch_hands_out_the_same_batches_in_the_same_order():
    """ReplayBuffer.prefetch = the reference's Cache (algos/sac1/sac1.py:103-130) inside the buffer: draws run ahead on the buffer's
    stream into a ring of page-locked blocks.  One sampler, one queue: the batches, and their order, are exactly those of plain
    sample_batch calls on an identically seeded buffer; a returned batch stays intact for `hold` further calls; prefetch(0) goes back
    to fresh arrays with the sampler where the prefetcher left it."""
    import distributed_drl_amd as d
    rs = np.random.RandomState(0)
    m = 3000
    data = (rs.randn(m, 8).astype(np.float32), rs.uniform(-1, 1, (m, 2)).astype(np.float32), rs.randn(m).astype(np.float32),
            rs.randn(m, 8).astype(np.float32), (rs.rand(m) < 0.1).astype(np.float32))
    a, b = d.ReplayBufferSAC1(8, 2, 5000, seed=9), d.ReplayBufferSAC1(8, 2, 5000, seed=9)
    for rb in (a, b):
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
    a.prefetch(64, depth=6, hold=2)
    prev = None
    for it in range(25):
        got, want = a.sample_batch(64), b.sample_batch(64)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s @ %d" % (k, it))
        if prev is not None:                      # the batch of the previous call is still intact (hold = 2)
            for k in prev[1]:
                np.testing.assert_array_equal(prev[0][k], prev[1][k])
        prev = (got, {k: v.copy() for k, v in want.items()})
    assert a.get_counts()[0] == 25 + 4 and b.get_counts()[0] == 25      # depth - hold draws are in flight
    a.prefetch(0)
    for _ in range(4):
        b.sample_batch(64)                        # the draws the prefetcher had made ahead
    got, want = a.sample_batch(64), b.sample_batch(64)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])


def test_prefetch_on_its_own_stream_orders_against_stores():
    """prefetch(own_stream=True): draws on the buffer's own stream, this object's stores ordered against them by events.  With the
    prefetcher drained between a store and the draws that follow it, the batches equal plain sample_batch calls on a twin buffer that
    sees the same stores at the same positions of the index stream."""
    import distributed_drl_amd as d
    rs = np.random.RandomState(1)
    mk = lambda m: (rs.randn(m, 8).astype(np.float32), rs.uniform(-1, 1, (m, 2)).astype(np.float32), rs.randn(m).astype(np.float32),
                    rs.randn(m, 8).astype(np.float32), np.zeros(m, np.float32))
    first, more = mk(600), [mk(64) for _ in range(6)]
    a, b = d.ReplayBufferSAC1(8, 2, 700, seed=3), d.ReplayBufferSAC1(8, 2, 700, seed=3)
    for rb in (a, b):
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in first))
    D, H = 5, 2
    a.prefetch(32, depth=D, hold=H, own_stream=True)
    ahead = D - H                                    # draws in flight
    for it in range(6):
        # twin: the `ahead` draws the prefetcher made BEFORE this store, then the store, like the prefetcher's order on the device
        want = [b.sample_batch(32) for _ in range(ahead)] if it == 0 else want[-ahead:]
        got = []
        for k in range(ahead):
            got.append({kk: v.copy() for kk, v in a.sample_batch(32).items()})      # hands out a drawn batch, enqueues one more draw
            want.append(b.sample_batch(32))
        for g, w in zip(got, want[:ahead]):
            for kk in w:
                np.testing.assert_array_equal(g[kk], w[kk], err_msg="%s @ %d" % (kk, it))
        torch.cuda.synchronize()
        a._pf["stream"].synchronize()
        x = [torch.from_numpy(v).cuda() for v in more[it]]
        a.store_batch(*x); b.store_batch(*x)          # the ring wraps (700 rows): rows the next draws may pick are being replaced
    a.prefetch(0)


@pytest.mark.gpu
def test_prefetch_on_its_own_stream_orders_every_sampler_call_of_the_object():
    """The calls of the same object that move the sampler or the rows while an own-stream prefetch is on — a draw of another size,
    sample_batch_device, sample_many, seed, set_rows, stores — are ordered against the draws in flight: a mixed call sequence hands
    out exactly what the same sequence does with the prefetch on the caller's stream (one stream: program order)."""
    import distributed_drl_amd as d
    rs = np.random.RandomState(4)
    mk = lambda m: (rs.randn(m, 8).astype(np.float32), rs.uniform(-1, 1, (m, 2)).astype(np.float32), rs.randn(m).astype(np.float32),
                    rs.randn(m, 8).astype(np.float32), np.zeros(m, np.float32))
    first, more, rows = mk(900), [mk(40) for _ in range(8)], rs.randn(16, 8).astype(np.float32)

    def run(own):
        rb = d.ReplayBufferSAC1(8, 2, 1000, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in first))
        rb.prefetch(32, depth=6, hold=2, own_stream=own)
        out = []
        flat = torch.empty(3 * 48 * 20, dtype=torch.float32, device="cuda")
        for it in range(8):
            out.append(np.concatenate([v.reshape(-1) for v in rb.sample_batch(32).values()]).copy())
            if it % 2 == 0:
                out.append(np.concatenate([v.reshape(-1) for v in rb.sample_batch(48).values()]).copy())
            if it % 3 == 1:
                dv = rb.sample_batch_device(16, fresh=True, with_indices=True)
                out.append(dv["idxs"].cpu().numpy().astype(np.float32))
            if it == 3:
                out.append(rb.sample_many(48, 3, flat).cpu().numpy().copy())
            if it == 4:
                rb.seed(77)
            if it == 5:
                rb.set_rows(0, 100, torch.from_numpy(rows).cuda())
            rb.store_batch(*(torch.from_numpy(x).cuda() for x in more[it]))
        rb.prefetch(0)
        return out

    for _ in range(3):                               # (a race would show as a difference in some repeat)
        one, two = run(False), run(True)
        assert len(one) == len(two)
        for i, (x, y) in enumerate(zip(one, two)):
            np.testing.assert_array_equal(x, y, err_msg="call %d" % i)
