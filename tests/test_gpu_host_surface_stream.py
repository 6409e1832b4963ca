"""GPU: the host-array surface on a caller's stream, and the host-graph path of ddrl_sac1_step_host.

Everything the Python classes do for a reference-style caller — Learner.train(host batch), Model.train, ReplayBuffer.store /
sample_batch / prefetch, Actor.get_action, the discrete learner and actor — goes to `_lib.stream_ptr()`, which is NULL on torch's
default stream: no other test of the suite leaves that stream, so ddrl_sac1_step_host's cache of captured graphs (skipped on the
null stream, which cannot be captured) never ran.  Here every object works under `with torch.cuda.stream(s)` on a non-blocking side
stream, with a bounded gate put on the stream ahead of the calls, so that work issued to another stream would overtake what the side
stream still holds.  The gate is 10 ms: between two events on the side stream a gated host update of these shapes took 0.05 to 0.07 ms
(measured on an MI355X; the test prints the figures of its own run), so 10 ms is more than a hundred updates long.  The references
are twins driven on the default stream through device tensors with ddrl_normal_fill noise at the same counters
(tests/test_gpu_sac1.py's test_host_batch_fast_path_equals_the_device_path); every comparison is bit-exact.

ddrl_sac1_host_graphs tells that the replay ran: at least one graph after the sequence on the side stream for the direct-operand
shapes, none for the generic shape, none for the same sequence on the default stream."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402

GATE_MS = 10.0
HOST_UPDATES = 8           # of _nine_updates' nine
EPS_CTR = 1 << 40          # where the explicit noise of the in-between device update is drawn: far from the host updates' counters


@pytest.fixture(scope="module")
def ddrl():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib


class _Gates:
    """Bounded sleeps on the current stream, each between two events; check() fails a run whose gate came out short as void."""

    def __init__(self):
        self.cycles, self.ev, self.calls = int(aa.cycles_per_ms(torch.device("cuda:0")) * GATE_MS * 1.1), [], []

    def __call__(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(self.cycles)
        e1.record()
        self.ev.append((e0, e1))

    def timed(self, fn):
        """fn() between two events on the current stream: what the gated call itself takes on the device (call_ms)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.calls.append((e0, e1))

    def call_ms(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.calls]

    def check(self):
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.ev]
        assert ms and min(ms) >= GATE_MS, "a gate held its stream for %.2f ms, %.2f ms intended: the run is void" % (min(ms), GATE_MS)


class _DsacArgs:
    """What example/dsac.py:185-216 hands to Model(args)."""

    def __init__(self, batch_size=100, seed=5):
        self.obs_dim, self.act_dim = 8, 2
        self.ac_kwargs = dict(hidden_sizes=[400, 300])
        self.gamma = 0.99,
        self.polyak, self.lr, self.alpha, self.batch_size, self.seed, self.max_ep_len = 0.995, 1e-3, 0.2, batch_size, seed, 1000


def _learner(kind):
    from distributed_drl_amd.agent import HyperParameters, Learner, Model
    if kind == "model":
        return Model(_DsacArgs()), (100, 8, 2)
    o, a, hid, B = {"ref": (8, 2, (400, 300), 256), "ragged": (5, 3, (72, 44), 37), "generic": (8, 2, (50, 34), 20)}[kind]
    opt = HyperParameters(obs_dim=o, act_dim=a)
    opt.seed, opt.batch_size, opt.hidden_sizes = 5, B, hid
    return Learner(opt), (B, o, a)


def _nine_updates(_lib, agent, shape, host, gate, tmp_path):
    """Four host updates, one train(device tensors, eps=...) in between (it moves the state-copy parity against the staging blocks'
    turn: new graph keys), two host updates, save_state -> load_state into the same learner, set_weights with the current weights,
    two host updates.  host=False: the twin — every update from device tensors with ddrl_normal_fill noise at the host path's
    counters.  -> the noise counter the host path must have reached."""
    lib, (B, o, a) = agent._lib, shape
    rs, ctr = np.random.RandomState(3), 0

    def noise(at):
        e = torch.empty(3 * B * a, device="cuda")
        _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), agent._noise_seed, at, _lib.stream_ptr()))
        e = e.view(3, B, a)
        return (e[0], e[1], e[2])

    def update(from_host):
        nonlocal ctr
        batch = dict(obs1=rs.randn(B, o).astype(np.float32), obs2=rs.randn(B, o).astype(np.float32),
                     acts=rs.uniform(-1, 1, (B, a)).astype(np.float32), rews=rs.randn(B).astype(np.float32),
                     done=(rs.rand(B) < 0.1).astype(np.float32))
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in batch.items()}
        if from_host is None:                             # the in-between device update: explicit noise on both sides
            agent.train(dev, eps=noise(EPS_CTR))
            return
        if from_host:
            if gate:
                gate()
                gate.timed(lambda: agent.train(batch))
            else:
                agent.train(batch)
            for v in batch.values():
                v += 1.0                                  # the caller's arrays may change as soon as train() has returned
        else:
            agent.train(dev, eps=noise(ctr))
        ctr += 3 * B * a

    for _ in range(4):
        update(host)
    update(None)
    for _ in range(2):
        update(host)
    path = str(tmp_path / ("state_%d" % id(agent)))
    agent.save_state(path)
    agent.load_state(path)
    agent.set_weights(*agent.get_weights())
    for _ in range(2):
        update(host)
    return ctr


def _state(_lib, agent):
    out = [agent.export(w).cpu() for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)]
    return out, agent.opt_steps()


@pytest.mark.parametrize("kind", ["ref", "ragged", "generic", "model"])
def test_train_host_batch_on_a_side_stream_equals_the_device_path_and_replays_graphs(ddrl, kind, tmp_path):
    _lib = ddrl
    s, gate = aa.side_stream("cuda:0"), _Gates()
    with torch.cuda.stream(s):
        a_, shape = _learner(kind)
        ctr = _nine_updates(_lib, a_, shape, True, gate, tmp_path)
        got, steps = _state(_lib, a_)
        n_side = a_._lib.ddrl_sac1_host_graphs(a_._h)
    gate.check()
    b_, _ = _learner(kind)                                 # the twin: default stream, device tensors
    _nine_updates(_lib, b_, shape, False, None, tmp_path)
    want, steps_w = _state(_lib, b_)
    c_, _ = _learner(kind)                                 # the host path on the default stream (the null stream: never captured)
    ctr_c = _nine_updates(_lib, c_, shape, True, None, tmp_path)
    got_c, steps_c = _state(_lib, c_)
    n_default = c_._lib.ddrl_sac1_host_graphs(c_._h)
    fused = a_._lib.ddrl_sac1_is_fused(a_._h)
    print("%s: host graphs held after the sequence: %d on the side stream, %d on the default stream (fused %d)" % (kind, n_side, n_default, fused))
    print("%s: the gated host updates took %s ms on the side stream" % (kind, " ".join("%.3f" % t for t in gate.call_ms())))
    assert a_._noise_ctr == ctr == ctr_c == c_._noise_ctr == HOST_UPDATES * 3 * shape[0] * shape[2]
    assert steps == steps_w == steps_c == (9, 9)
    for name, g, gc, w in zip(("main", "target", "adam_m", "adam_v"), got, got_c, want):
        assert torch.equal(g, w), "%s after nine updates on the side stream differs from the device path's" % name
        assert torch.equal(gc, w), "%s after nine updates on the default stream differs from the device path's" % name
    assert fused == (0 if kind == "generic" else 1)
    assert n_default == 0, "the null stream cannot be captured: %d host graphs" % n_default
    if kind == "generic":
        assert n_side == 0, "the generic path stays eager: %d host graphs" % n_side
    else:
        # a key's first use captures its graph; the sequence makes HOST_UPDATES host updates, all from the learner's page-locked
        # staging blocks (no other reason to run eagerly) and below the cache limit, so fewer graphs than host updates means that at
        # least one update met a key a second time and replayed its graph
        assert 1 <= n_side < HOST_UPDATES, "no host update replayed a cached graph on the side stream: %d host graphs, %d host updates" % (
            n_side, HOST_UPDATES)


def test_the_host_graph_cache_stops_at_sixteen_keys_and_the_rest_runs_eagerly(ddrl):
    """The C ABI at the ragged shape: nine page-locked blocks in turn over 36 updates — nine is odd, so every block meets both
    state-copy parities, twice each: 18 keys.  The last two are refused by the cache and run eagerly; the result equals the twin's."""
    _lib = ddrl
    lib = _lib.load()
    B, o, a, K = 37, 5, 3, 9
    cfg = _lib.Sac1Config(obs_dim=o, act_dim=a, hidden1=72, hidden2=44, batch=B, variant=0, lr=1e-3)
    n_pi, n_q = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.ddrl_sac1_param_counts(ctypes.byref(cfg), ctypes.byref(n_pi), ctypes.byref(n_q)))
    n = n_pi.value + 2 * n_q.value
    w0 = torch.from_numpy((np.random.RandomState(21).randn(n) * 0.2).astype(np.float32)).cuda()
    rs = np.random.RandomState(7)
    batches = [[rs.randn(B, o).astype(np.float32), rs.randn(B, o).astype(np.float32), rs.uniform(-1, 1, (B, a)).astype(np.float32),
                rs.randn(B).astype(np.float32), (rs.rand(B) < 0.2).astype(np.float32)] for _ in range(K)]
    torch.cuda.synchronize()

    def make():
        h = ctypes.c_void_p()
        _lib.check(lib.ddrl_sac1_create(ctypes.byref(h), 0, ctypes.byref(cfg)))
        _lib.check(lib.ddrl_sac1_set_weights(h, _lib.dptr(w0), _lib.stream_ptr()))
        return h

    def state(h):
        out = []
        for which in range(4):
            t = torch.empty(n, device="cuda")
            _lib.check(lib.ddrl_sac1_export(h, which, _lib.dptr(t), _lib.stream_ptr()))
            out.append(t.cpu())
        return out

    s, gate = aa.side_stream("cuda:0"), _Gates()
    counts = []
    with torch.cuda.stream(s):
        h = make()
        try:
            assert lib.ddrl_sac1_is_fused(h) == 1
            bufs = (ctypes.c_void_p * 8)()
            _lib.check(lib.ddrl_sac1_input_buffers(h, 0, bufs))
            off = [(int(bufs[j]) - int(bufs[0])) // 4 for j in range(5)]
            span = off[4] + B
            blocks = []
            for arrs in batches:                            # the padding rows of the 32-row tiles stay zero
                blk = torch.zeros(span + 2, dtype=torch.float32).pin_memory()
                for j, x in enumerate(arrs):
                    blk.numpy()[off[j]:off[j] + x.size] = x.reshape(-1)
                blocks.append(blk)
            losses = torch.zeros(3, device="cuda")
            gate()
            done = [None] * K
            for u in range(4 * K):
                blk = blocks[u % K]
                if done[u % K] is not None:
                    done[u % K].synchronize()               # the call writes the noise counter behind the batch: the block's last use has run
                _lib.check(lib.ddrl_sac1_step_host(h, ctypes.c_void_p(blk.data_ptr()), span, 5, u * 3 * B * a, _lib.dptr(losses),
                                                   _lib.stream_ptr()))
                done[u % K] = torch.cuda.Event()
                done[u % K].record()
                counts.append(lib.ddrl_sac1_host_graphs(h))
            got = state(h)
        finally:
            s.synchronize()
            lib.ddrl_sac1_destroy(h)
    gate.check()
    h = make()
    try:
        for u in range(4 * K):
            dev = [torch.from_numpy(x).cuda() for x in batches[u % K]]
            e = torch.empty(3 * B * a, device="cuda")
            _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), 5, u * 3 * B * a, None))
            e = e.view(3, B * a)
            losses = torch.zeros(3, device="cuda")
            _lib.check(lib.ddrl_sac1_step(h, *[_lib.dptr(t) for t in dev], _lib.dptr(e[0]), _lib.dptr(e[1]), _lib.dptr(e[2]), _lib.dptr(losses),
                                          None, None, None, None))
        want = state(h)
    finally:
        torch.cuda.synchronize()
        lib.ddrl_sac1_destroy(h)
    print("host graphs held after each of the 36 updates:", counts)
    assert max(counts) <= 16 and counts == sorted(counts), counts
    assert counts[2 * K - 1] == 16 and counts[-1] == 16, counts          # 18 keys met by then: the cache is full and stays full
    for name, g, w in zip(("main", "target", "adam_m", "adam_v"), got, want):
        assert torch.equal(g, w), "%s after 36 updates through nine blocks differs from the device path's" % name


def _ring_surface(make, n_act, B):
    """200 single store(host arrays) calls (the page-locked row ring of 64 comes round three times behind its events), sample_batch()
    to NumPy, prefetch(B, own_stream=True) started on the current stream, three prefetched batches, get_counts()."""
    buf = make()
    rs = np.random.RandomState(11)
    for i in range(200):
        act = rs.uniform(-1, 1, 2) if n_act is None else float(rs.randint(0, n_act))
        buf.store(rs.randn(8), act, rs.randn(), rs.randn(8), bool(rs.rand() < 0.1))
    out = [buf.sample_batch(B)]
    buf.prefetch(B, depth=4, hold=2, own_stream=True)
    for _ in range(3):
        out.append({k: v.copy() for k, v in buf.sample_batch(B).items()})
    counts = buf.get_counts()
    buf.prefetch(0)
    return out, counts


@pytest.mark.parametrize("which", ["sac1", "dqn"])
def test_replay_buffer_host_surface_on_a_side_stream_equals_the_default_stream(ddrl, which):
    from distributed_drl_amd import dqn, replay
    if which == "sac1":
        make, n_act, B = (lambda: replay.ReplayBufferSAC1(8, 2, 150, seed=3)), None, 32
    else:
        opt = dqn.HyperParameters(obs_dim=8, act_dim=4)
        opt.buffer_size, opt.batch_size = 150, 32
        make, n_act, B = (lambda: replay.ReplayBufferDQN(opt, 0, seed=3)), 4, 32
    s, gate = aa.side_stream("cuda:0"), _Gates()
    with torch.cuda.stream(s):
        gate()
        got, counts = _ring_surface(make, n_act, B)
    gate.check()
    want, counts_w = _ring_surface(make, n_act, B)
    assert counts == counts_w, (counts, counts_w)
    assert len(got) == len(want) == 4
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("obs1", "obs2", "acts", "rews", "done"):
            assert np.array_equal(g[k], w[k]), "batch %d, %s: the side stream's differs from the default stream's" % (i, k)


def test_actor_get_action_on_a_side_stream_equals_the_default_stream(ddrl):
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters()
    opt.seed = 5
    obs = np.random.RandomState(2).randn(6, 8).astype(np.float32)

    def run(gate):
        actor = Actor(opt, max_rows=1)
        out = []
        for i, o in enumerate(obs):
            if gate and i % 3 == 0:
                gate()
            out.append(actor.get_action(o, deterministic=(i == 5)))      # one row in, one row out
        return np.stack(out)
    s, gate = aa.side_stream("cuda:0"), _Gates()
    with torch.cuda.stream(s):
        got = run(gate)
    gate.check()
    want = run(None)
    assert got.shape == (6, 2) and np.array_equal(got, want)


def test_discrete_learner_and_actor_on_a_side_stream_equal_the_default_stream(ddrl):
    _lib = ddrl
    from distributed_drl_amd import dqn
    opt = dqn.HyperParameters(obs_dim=8, act_dim=4)
    opt.hidden_size, opt.batch_size, opt.seed = [64, 48], 37, 5
    B = 37

    def run(gate):
        learner, actor = dqn.Learner(opt), dqn.Actor(opt)
        rs = np.random.RandomState(9)
        for i in range(5):
            batch = dict(obs1=rs.randn(B, 8).astype(np.float32), obs2=rs.randn(B, 8).astype(np.float32),
                         acts=rs.randint(0, 4, B).astype(np.float32), rews=rs.randn(B).astype(np.float32),
                         done=(rs.rand(B) < 0.1).astype(np.float32))
            if gate and i % 2 == 0:
                gate()
            learner.train(batch)                                          # host arrays
            for v in batch.values():
                v += 1.0
        actor.set_weights(*learner.get_weights())
        acts = [actor.get_action(o) for o in rs.randn(8, 8).astype(np.float32)]
        return [learner.export(w).cpu() for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)], acts
    s, gate = aa.side_stream("cuda:0"), _Gates()
    with torch.cuda.stream(s):
        got, acts = run(gate)
    gate.check()
    want, acts_w = run(None)
    assert acts == acts_w, (acts, acts_w)
    for name, g, w in zip(("main", "target", "adam_m", "adam_v"), got, want):
        assert torch.equal(g, w), "%s of the discrete learner on the side stream differs from the default stream's" % name
