"""The articulated lander's evaluation episodes on the device, fed from handles (ddrl_env_eval_policy / ddrl_env_eval_q /
ddrl_env_eval_results, csrc/eval3.hip; Actor.evaluate_env, dqn.Actor.evaluate_env / ActorSQN.evaluate_env), held to
  * the trace checks: the env half bit for bit against tests/lander3_oracle.Lander3Oracle (tests/_eval3_trace.py; tests/test_eval3_cpu.py
    shows what it sees), the policy half and the Q rows / selections by tests/_eval_trace.check_policy and
    tests/_discrete_eval_trace.check_q / check_actions as they stand, with _acting_parity's bars;
  * the stream contract of first_episode;
  * the host loop it replaces, bit for bit: Actor.test / Model.test_agent / dqn.Actor / ActorSQN on the host env and on the device
    marker, per-episode returns and lengths equal to the loop written out;
  * ddrl_policy_eval / ddrl_dqn_eval on a one-body handle, bit for bit;
and: no side effects on the lending handle or the agents, the results block's bookkeeping, every refusal (status, text, nothing
launched), the make_device door, the DdrlUnsupported fallback and a worker_test / worker_test_dqn round with opt.test_on_device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402
import _discrete_eval_trace as dt  # noqa: E402
import _eval_trace as et  # noqa: E402
import _eval3_trace as e3  # noqa: E402

pytestmark = pytest.mark.gpu

CONT, DISC = "LunarLanderContinuous-v2", "LunarLander-v2"
VIT, PIT = 8, 3


class QCase3(dt.DCase):
    """A _discrete_eval_trace.DCase plus the solver's iteration counts."""

    def __init__(self, *a, vit=VIT, pit=PIT, **kw):
        super().__init__(*a, **kw)
        self.vit, self.pit = vit, pit


Q_CASES = [
    QCase3("a-ddqn-64x48-g05-n3-len120", "ddqn", (64, 48), 3, 120, greedy=0.5, ctr=(1 << 32) - 300),      # the counter crosses 2^32
    QCase3("a-ddqn-400x300-g097-n2-len40", "ddqn", (400, 300), 2, 40, greedy=0.97, ctr=1000),
    QCase3("a-ddqn-ragged-70x44-g05-n2-len30", "ddqn", (70, 44), 2, 30, greedy=0.5, wseed=22, ctr=6),
    QCase3("a-ddqn-64x48-det-n1-len1", "ddqn", (64, 48), 1, 1, deterministic=True),
    QCase3("a-sqn-64x32-det-n2-len40", "sqn", (64, 32), 2, 40, deterministic=True, wseed=23),
    QCase3("a-sqn-64x32-sample-n2-len40", "sqn", (64, 32), 2, 40, alpha=0.1, wseed=23, ctr=250),
    QCase3("a-ddqn-64x48-g05-n2-len12-gym180x60", "ddqn", (64, 48), 2, 12, greedy=0.5, ctr=40, vit=180, pit=60),
]


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _model_kw(vit=VIT, pit=PIT):
    return dict(model="articulated", velocity_iterations=vit, position_iterations=pit)


def _marker(name, seed, max_ep_len, vit=VIT, pit=PIT, simple=False):
    from distributed_drl_amd import env
    return env.make_device(name, seed=seed, max_ep_len=max_ep_len, **({} if simple else _model_kw(vit, pit)))


def _opt(hid, max_ep_len, seed=0, **kw):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(**kw)
    opt.hidden_sizes, opt.max_ep_len, opt.seed, opt.env = tuple(hid), max_ep_len, seed, CONT
    return opt


def _actor(case, max_ep_len=None):
    from distributed_drl_amd.agent import Actor
    actor = Actor(_opt(case.hid, case.max_ep_len if max_ep_len is None else max_ep_len), max_rows=1)
    params = et.params_of(case)
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


def _q_actor(case, max_ep_len=None, max_rows=1):
    from distributed_drl_amd import dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, case.acts, list(case.hid), 0.99, 1e-3, 0.995, max_rows, case.wseed, case.alpha
    Opt.max_ep_len = case.max_ep_len if max_ep_len is None else max_ep_len
    actor = (dqn.ActorSQN if case.family == "sqn" else dqn.Actor)(Opt, "test", max_rows=max_rows)
    params = dt.params_of(case)
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))
    actor._noise_seed, actor._noise_ctr = case.nseed, case.ctr
    return actor, params


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _same_out(a, b):
    return _same_bits(a["trace"], b["trace"]) and (a["ret"] == b["ret"]).all() and (a["len"] == b["len"]).all()


# ---- 1. trace cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", e3.TRACE_CASES, ids=repr)
def test_policy_trace_passes_both_checks(ddrl, case):
    actor, params = _actor(case)
    dev = _marker(CONT, case.seed, case.max_ep_len, case.vit, case.pit)
    out = actor.evaluate_env(dev, case.n, case.first, trace=True)
    assert out["ret"].dtype == np.float64 and out["len"].dtype == np.int32 and out["trace"].dtype == np.float32
    assert out["trace"].shape == (case.n, case.max_ep_len, 12) and dev.episodes_played == 0
    e3.check_env3(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)
    et.check_policy(out, case, params)
    if case is e3.LONG_CASE:      # what tests/test_eval3_cpu.py asserts on the oracle's trace holds for the device's
        last = np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
        assert ((out["len"] < case.max_ep_len) & (last[:, 10] == -100)).any()
        rows = et.played_rows(out)[0]
        assert ((rows[:, 6] == 1) | (rows[:, 7] == 1)).any()


@pytest.mark.parametrize("case", Q_CASES, ids=repr)
def test_q_trace_passes_the_three_checks(ddrl, case):
    actor, params = _q_actor(case)
    dev = _marker(DISC, case.seed, case.max_ep_len, case.vit, case.pit)
    out = actor.evaluate_env(dev, case.n, case.first, deterministic=case.deterministic, greedy_prob=case.greedy, trace=True)
    assert out["ret"].dtype == np.float64 and out["len"].dtype == np.int32 and out["trace"].dtype == np.float32
    assert out["trace"].shape == (case.n, case.max_ep_len, 20)
    assert actor._noise_ctr == case.ctr + 2 * case.n * case.max_ep_len
    e3.check_env3_discrete(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)
    table = []
    try:
        dt.check_q(out, case, params, table=table)
    finally:
        print("\n".join(ap.format_table(table)))
    dt.check_actions(out, case)


# ---- 2. first_episode ---------------------------------------------------------------------------------------------------------------
def test_first_episode_positions_the_stream(ddrl):
    long, short = e3.FIRST_CASES
    actor, _ = _actor(long)
    dev = _marker(CONT, long.seed, long.max_ep_len)
    a = actor.evaluate_env(dev, long.n, 0, trace=True)
    b = actor.evaluate_env(dev, short.n, short.first, trace=True)
    assert _same_out({k: v[5:8] for k, v in a.items()}, b)
    assert not _same_bits(a["trace"][0:3], b["trace"])
    qcase = QCase3("a-ddqn-64x48-det-first", "ddqn", (64, 48), 8, 40, deterministic=True)
    qa, _ = _q_actor(qcase)
    qdev = _marker(DISC, qcase.seed, qcase.max_ep_len)
    a = qa.evaluate_env(qdev, 8, 0, deterministic=True, trace=True)
    b = qa.evaluate_env(qdev, 3, 5, deterministic=True, trace=True)
    assert _same_out({k: v[5:8] for k, v in a.items()}, b)
    # the default is the marker's episode count
    qdev.episodes_played = 5
    qa._noise_ctr = qcase.ctr
    assert _same_out(qa.evaluate_env(qdev, 3, deterministic=True, trace=True), b)


# ---- 3. equal to the host loop it replaces --------------------------------------------------------------------------------------------
def _host_loop(agent, env, n, max_ep_len):
    """Actor.test's episodes written out: (returns, lengths)."""
    rets, lens = [], []
    for _ in range(n):
        o, d, ep_ret, ep_len = env.reset(), False, 0, 0
        while not (d or (ep_len == max_ep_len)):
            o, r, d, _ = env.step(agent.get_action(o, True))
            ep_ret += r
            ep_len += 1
        rets.append(ep_ret)
        lens.append(ep_len)
    return rets, lens


def test_actor_test_equals_the_host_loop(ddrl):
    from distributed_drl_amd import env
    n, L, seed = 3, 48, 7
    actor, _ = _actor(e3.TRACE_CASES[0], L)
    host, loop_env = env.LunarLander(seed, L, **_model_kw()), env.LunarLander(seed, L, **_model_kw())
    dev = _marker(CONT, seed, L)
    assert isinstance(dev, env.DeviceLunarLander) and dev.model == "articulated"
    for rnd in range(2):
        want, got = actor.test(host, None, n), actor.test(dev, None, n)
        assert isinstance(got, float) and got == want, (rnd, got, want)
        assert dev.episodes_played == n * (rnd + 1)
        rets, lens = _host_loop(actor, loop_env, n, L)
        out = actor.evaluate_env(dev, n, n * rnd)
        assert "trace" not in out and out["ret"].tolist() == rets and out["len"].tolist() == lens, (rnd, out, rets, lens)
        assert want == sum(rets) / n


class _Args:
    env, obs_dim, act_dim = CONT, 8, 2
    ac_kwargs = dict(hidden_sizes=[64, 48])
    gamma = 0.99,
    polyak, lr, alpha, batch_size, seed = 0.995, 1e-3, 0.2, 32, 4
    max_ep_len = 48


def test_model_test_agent_equals_the_host_loop(ddrl):
    from distributed_drl_amd import env
    from distributed_drl_amd.agent import Model
    args, n, seed = _Args(), 3, 7
    net = Model(args)
    host, dev = env.LunarLander(seed, args.max_ep_len, **_model_kw()), _marker(CONT, seed, args.max_ep_len)
    for rnd in range(2):
        want, got = net.test_agent(host, args, n), net.test_agent(dev, args, n)
        print("Model.test_agent round %d: host %r device %r" % (rnd, want, got))
        assert got == want, (rnd, got, want)
    assert dev.episodes_played == 2 * n


def _q_loop(actor, case, host, n, first_ctr, deterministic):
    """dqn.Actor.test's episodes written out with the selection rule and the uniforms of the device call at `first_ctr`: the host
    Q row (ddrl_dqn_q), _discrete_acting.select, env.step — (returns, lengths)."""
    L = case.max_ep_len
    rets, lens = [], []
    for e in range(n):
        o, d, ep_ret, ep_len = host.reset(), False, 0, 0
        u0, u1 = da.uniforms(actor._noise_seed, first_ctr + 2 * e * L, L)
        while not d:
            q = np.array(actor._q_row(o), np.float32).reshape(1, -1)
            a = int(da.select(q, case.family, case.alpha, actor.greedy_prob, u0[ep_len:ep_len + 1], u1[ep_len:ep_len + 1], deterministic)[0])
            o, r, d, _ = host.step(a)
            ep_ret += r
            ep_len += 1
        rets.append(ep_ret)
        lens.append(ep_len)
    return rets, lens


@pytest.mark.parametrize("family,deterministic", [("ddqn", False), ("ddqn", True), ("sqn", True), ("sqn", False)])
def test_dqn_actor_equals_the_host_loop(ddrl, family, deterministic):
    """Per-episode returns and lengths of the device episodes equal the loop written out on the host env (the host's Q row, the
    selection oracle on the call's own uniforms), over two rounds, in sample and in deterministic mode; and where the class's own
    test action is deterministic (ActorSQN) test() returns equal tuples from the host env and from the marker."""
    from distributed_drl_amd import env
    n, L, seed = 3, 48, 7
    case = QCase3("loop-%s" % family, family, (64, 48) if family == "ddqn" else (64, 32), n, L, wseed=21 if family == "ddqn" else 23, ctr=500)
    actor, _ = _q_actor(case)
    host = env.LunarLanderDiscrete(seed, L, **_model_kw())
    dev = _marker(DISC, seed, L)
    assert isinstance(dev, env.DeviceLunarLanderDiscrete) and dev.action_space.n == 4
    for rnd in range(2):
        ctr = actor._noise_ctr
        out = actor.evaluate_env(dev, n, n * rnd, deterministic=deterministic)
        assert actor._noise_ctr == ctr + 2 * n * L
        rets, lens = _q_loop(actor, case, host, n, ctr, deterministic)
        assert out["ret"].tolist() == rets and out["len"].tolist() == lens, (rnd, out, rets, lens)
    if family == "sqn" and deterministic:
        host2, dev2 = env.LunarLanderDiscrete(seed, L, **_model_kw()), _marker(DISC, seed, L)
        for rnd in range(2):
            ctr = actor._noise_ctr
            want, got = actor.test(host2, n), actor.test(dev2, n)
            assert tuple(got) == tuple(want) and type(got[0]) is float, (rnd, got, want)
            assert dev2.episodes_played == n * (rnd + 1) and actor._noise_ctr == ctr + 2 * n * L


# ---- 4. a one-body handle through the new entry points ---------------------------------------------------------------------------------
def test_one_body_handle_equals_the_pointer_fed_entry_points(ddrl):
    case = et.TRACE_CASES[3]      # ragged 70x44
    actor, _ = _actor(case)
    dev = _marker(CONT, case.seed, case.max_ep_len, simple=True)
    assert dev.model == "simple"
    want = actor.evaluate(case.n, case.seed, 2, case.max_ep_len, trace=True)
    got = actor.evaluate_env(dev, case.n, 2, trace=True)
    assert _same_out(got, want)
    qcase = dt.TRACE_CASES[3]     # ddqn ragged 70x44, greedy 0.5
    qa, _ = _q_actor(qcase)
    qdev = _marker(DISC, qcase.seed, qcase.max_ep_len, simple=True)
    want = qa.evaluate(qcase.n, qcase.seed, 1, qcase.max_ep_len, deterministic=False, greedy_prob=qcase.greedy, trace=True)
    qa._noise_ctr = qcase.ctr
    got = qa.evaluate_env(qdev, qcase.n, 1, deterministic=False, greedy_prob=qcase.greedy, trace=True)
    assert _same_out(got, want)


# ---- 5. no side effects ---------------------------------------------------------------------------------------------------------------
def test_evaluation_has_no_side_effects(ddrl):
    from distributed_drl_amd import _lib, env
    case = e3.TRACE_CASES[0]
    actor, _ = _actor(case)
    lib = _lib.load()
    vecs = [env.VecLunarLander(4, seed=11, max_ep_len=9, **_model_kw()) for _ in range(2)]
    acts = [torch.tensor(np.random.RandomState(k).uniform(-1, 1, (4, 2)).astype(np.float32), device="cuda") for k in range(12)]
    for v in vecs:
        for a in acts[:10]:      # past one time limit: the statistics are off zero
            v.step(a)
    ctr, before = actor._noise_ctr, actor.get_weights_flat().clone()
    _lib.check(lib.ddrl_env_eval_policy(vecs[0]._h, actor._h, 3, 4, 1, _lib.stream_ptr()))
    plain = env.eval_results(vecs[0], 12)
    assert plain["trace"].shape == (3, 9, 12)
    assert actor._noise_ctr == ctr and torch.equal(actor.get_weights_flat(), before)
    assert torch.equal(vecs[0].get_state().view(torch.int32), vecs[1].get_state().view(torch.int32))
    outs = [[t.clone() for t in v.step(acts[10])] for v in vecs]
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert vecs[0].stats() == vecs[1].stats() and vecs[0].stats()[0] == 0
    # the same episodes from a one-env marker of that seed and model: n_envs of the lending handle does not matter
    dev = env.make_device(CONT, seed=11, max_ep_len=9, **_model_kw())
    assert _same_out(actor.evaluate_env(dev, 3, 4, trace=True), plain)
    # the DQN actor: weights untouched, the counter advances by 2 n max_ep_len
    qcase = Q_CASES[0]
    qa, _ = _q_actor(qcase)
    main = qa.export().clone()
    qa.evaluate_env(_marker(DISC, 3, 9), 2)
    assert qa._noise_ctr == qcase.ctr + 2 * 2 * 9 and torch.equal(qa.export(), main)


# ---- 6. the results block -------------------------------------------------------------------------------------------------------------
def _results(lib, h):
    from distributed_drl_amd import _lib
    p = [ctypes.c_void_p() for _ in range(3)]
    k = [ctypes.c_int32(-1) for _ in range(3)]
    rc = lib.ddrl_env_eval_results(h, *[ctypes.byref(x) for x in p + k])
    return rc, [x.value for x in p], [x.value for x in k]


def test_results_block(ddrl):
    from distributed_drl_amd import _lib, env
    case = e3.TRACE_CASES[0]
    L = 20
    actor, _ = _actor(case, L)
    lib = _lib.load()
    vec = env.VecLunarLander(1, seed=3, max_ep_len=L, **_model_kw())
    rc, _, _ = _results(lib, vec._h)
    assert rc == _lib.DDRL_ERR_BAD_ARG and b"no evaluation" in lib.ddrl_last_error()
    seen = []
    for n, trace in ((2, True), (5, False), (5, True), (2, False), (2, True)):
        _lib.check(lib.ddrl_env_eval_policy(vec._h, actor._h, n, 0, 1 if trace else 0, _lib.stream_ptr()))
        rc, (ret, ln, tr), (rn, rL, row) = _results(lib, vec._h)
        assert rc == _lib.DDRL_OK and (rn, rL, row) == (n, L, 12 if trace else 0)
        assert ret and ln and ret % 256 == 0 and ln % 16 == 0 and ln >= ret + 8 * n
        assert (tr is None) == (not trace)
        if trace:
            assert tr % 16 == 0 and tr >= ln + 4 * n
        out = env.eval_results(vec, 12)
        assert out["ret"].shape == (n,) and out["len"].shape == (n,) and ("trace" in out) == trace
        if trace:
            assert out["trace"].shape == (n, L, 12)
            for e, l in enumerate(out["len"]):
                assert out["trace"][e, :l, 11].sum() == 1 and not out["trace"][e, l:].view(np.uint32).any()
        seen.append((n, trace, ret, out))
    # the same call gives the same results, wherever the block lies; once grown for (5, trace) the block stays where it is
    assert _same_out(seen[0][3], seen[4][3]) and (seen[1][3]["ret"] == seen[2][3]["ret"]).all()
    assert seen[2][2] == seen[3][2] == seen[4][2]
    # a trace of the other row length is refused by the reader, not misread
    qa, _ = _q_actor(Q_CASES[0], L)
    _lib.check(lib.ddrl_env_eval_q(vec._h, qa._h, 2, 0, _lib.DDRL_ACT_SAMPLE, 0.5, 1, 0, 1, _lib.stream_ptr()))
    assert _results(lib, vec._h)[2] == [2, L, 20]
    with pytest.raises(_lib.DdrlError, match="20"):
        env.eval_results(vec, 12)


# ---- 7. every refusal -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ddrl):
    from distributed_drl_amd import _lib, dqn, env
    from distributed_drl_amd.agent import Actor
    case, L = e3.TRACE_CASES[0], 10
    actor, _ = _actor(case, L)
    qa, _ = _q_actor(Q_CASES[0], L)
    lib, s = _lib.load(), _lib.stream_ptr
    vec = env.VecLunarLander(1, seed=3, max_ep_len=L, **_model_kw())
    _lib.check(lib.ddrl_env_eval_policy(vec._h, actor._h, 2, 0, 1, s()))
    torch.cuda.synchronize()
    rc, (ret, ln, tr), sizes = _results(lib, vec._h)
    assert rc == _lib.DDRL_OK
    # a sentinel over the whole results block: a launch would overwrite ret, len and (rows past the end included) every trace element
    nbytes = tr + 2 * L * 12 * 4 - ret

    class _Holder:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ret), False), "version": 2}
    block = torch.as_tensor(_Holder(), device="cuda")
    block.fill_(0xA5)
    torch.cuda.synchronize()

    wide = Actor(_opt(case.hid, L, act_dim=3), max_rows=1)

    class QOpt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha, max_ep_len = 8, 9, [64, 48], 0.99, 1e-3, 0.995, 1, 1, 0.1, L
    q9 = dqn.Actor(QOpt, "test", max_rows=1)
    QOpt9 = type("QOpt9", (QOpt,), dict(obs_dim=9, act_dim=4))
    qo9 = dqn.Actor(QOpt9, "test", max_rows=1)

    pol = lambda h, a, n=2, first=0: lib.ddrl_env_eval_policy(h, a, n, first, 1, s())
    qev = lambda h, a, n=2, first=0, mode=_lib.DDRL_ACT_SAMPLE: lib.ddrl_env_eval_q(h, a, n, first, mode, 0.5, 1, 0, 1, s())
    B, U = _lib.DDRL_ERR_BAD_ARG, _lib.DDRL_ERR_UNSUPPORTED
    refusals = [
        ("policy: NULL env handle", lambda: pol(None, actor._h), B, b"NULL handle"),
        ("policy: NULL actor", lambda: pol(vec._h, None), B, b"NULL handle"),
        ("policy: n_episodes 0", lambda: pol(vec._h, actor._h, n=0), B, b"n_episodes"),
        ("policy: episode index past 2^24", lambda: pol(vec._h, actor._h, n=2, first=(1 << 24) - 1), B, b"2^24"),
        ("policy: actor 8 -> 3", lambda: pol(vec._h, wide._h), B, b"2 actions"),
        ("q: NULL env handle", lambda: qev(None, qa._h), B, b"NULL handle"),
        ("q: NULL dqn", lambda: qev(vec._h, None), B, b"NULL handle"),
        ("q: n_episodes -1", lambda: qev(vec._h, qa._h, n=-1), B, b"n_episodes"),
        ("q: episode index past 2^24", lambda: qev(vec._h, qa._h, n=1, first=1 << 24), B, b"2^24"),
        ("q: 9 observations", lambda: qev(vec._h, qo9._h), B, b"8 observations"),
        ("q: unknown mode", lambda: qev(vec._h, qa._h, mode=2), B, b"mode"),
        ("q: 9 actions", lambda: qev(vec._h, q9._h), U, b"n_actions"),
    ]
    if torch.cuda.device_count() > 1:      # handles on different devices (needs a second device to build one on)
        with torch.cuda.device(1):
            far = env.VecLunarLander(1, seed=3, max_ep_len=L, **_model_kw())
        refusals += [("policy: other device", lambda: pol(far._h, actor._h), B, b"device"), ("q: other device", lambda: qev(far._h, qa._h), B, b"device")]
    for what, call, status, word in refusals:
        rc = call()
        text = lib.ddrl_last_error()
        assert rc == status, (what, rc, text)
        assert word in text and (b"ddrl_env_eval_policy" if what.startswith("policy") else b"ddrl_env_eval_q") in text, (what, text)
    with pytest.raises(_lib.DdrlUnsupported):
        _lib.check(qev(vec._h, q9._h))
    with pytest.raises(ValueError, match="ddrl"):
        _lib.check(pol(vec._h, actor._h, n=0))
    torch.cuda.synchronize()
    assert bool((block == 0xA5).all()), "a refused call wrote into the results block"
    assert _results(lib, vec._h) == (_lib.DDRL_OK, [ret, ln, tr], sizes)      # ... and the previous results are still the handle's
    # the same calls with nothing wrong go through (the policy call fits the block: the sentinel view still points into it)
    assert pol(vec._h, actor._h) == _lib.DDRL_OK
    torch.cuda.synchronize()
    assert not bool((block[:16] == 0xA5).all())
    del block      # (the Q call's wider trace rows grow the block)
    assert qev(vec._h, qa._h) == _lib.DDRL_OK
    torch.cuda.synchronize()


# ---- 8. door, fallback, workers ---------------------------------------------------------------------------------------------------------
def test_make_device_builds_both_markers_and_make_still_refuses(ddrl):
    from distributed_drl_amd import env
    a = env.make_device(CONT, seed=4, max_ep_len=30, **_model_kw(180, 60))
    b = env.make_device(DISC, seed=4, max_ep_len=30, **_model_kw())
    c, d = env.make_device(CONT, seed=4, max_ep_len=30), env.make_device(DISC)
    assert type(a) is env.DeviceLunarLander and type(b) is env.DeviceLunarLanderDiscrete and isinstance(b, env.DeviceLunarLander)
    assert (a.model, a.velocity_iterations, a.position_iterations, a.seed, a.max_ep_len, a.on_device) == ("articulated", 180, 60, 4, 30, True)
    assert (b.model, b.velocity_iterations, b.position_iterations) == ("articulated", VIT, PIT) and b.action_space.n == 4
    assert type(c) is env.DeviceLunarLander and c.model == "simple" and type(d) is env.DeviceLunarLanderDiscrete and d.model == "simple"
    assert (env.DeviceLunarLander(5, 40).seed, env.DeviceLunarLander(5, 40).max_ep_len) == (5, 40)      # positional (seed, max_ep_len) stays
    with pytest.raises(ValueError, match="evaluation kernel"):
        env.make(CONT, on_device=True, model="articulated")
    with pytest.raises(ValueError, match="make_device"):
        env.make(DISC, on_device=True, model="articulated", seed=1)
    with pytest.raises(ValueError, match="model"):
        env.make_device(CONT, model="biped")
    with pytest.raises(RuntimeError, match="not steppable"):
        a.step(np.zeros(2))
    # the lending handle and the host env are of the marker's model
    assert a.handle().model == "articulated" and a.handle().n == 1 and a.handle().state_fields == 66 and a.handle() is a.handle()
    a.episodes_played = 3
    host = a.host_env()
    assert isinstance(host, env.LunarLander) and host._vec.model == "articulated" and float(host._vec.get_state()[13, 0]) == 3.0
    assert isinstance(b.host_env(), env.LunarLanderDiscrete)


def test_outside_the_envelope_falls_back_to_the_host_loop(ddrl, monkeypatch):
    """An Actor outside the row kernels' envelope cannot be built (ddrl_actor_create refuses hidden sizes > 512), so — as in
    tests/test_gpu_eval.py — the fallback is driven by an evaluate_env that raises what _lib.check raises for DDRL_ERR_UNSUPPORTED: the
    host env it steps instead is of the marker's model and sits at the same episode, in both rounds."""
    from distributed_drl_amd import env
    n, L, seed = 2, 30, 5
    actor, _ = _actor(e3.TRACE_CASES[0], L)
    want = actor.test(_marker(CONT, seed, L), None, 2 * n)      # the device path over the same four episodes
    host, dev = env.LunarLander(seed, L, **_model_kw()), _marker(CONT, seed, L)

    def unsupported(*a, **kw):
        raise ddrl._lib.DdrlUnsupported("ddrl error -5: outside the envelope")
    monkeypatch.setattr(actor, "evaluate_env", unsupported)
    got = []
    for rnd in range(2):     # the second round starts the fallback's host env at episode n
        h, d = actor.test(host, None, n), actor.test(dev, None, n)
        assert d == h, (rnd, d, h)
        got.append(d)
    assert dev.episodes_played == 2 * n and got[0] != got[1]
    assert (got[0] + got[1]) / 2 == pytest.approx(want, rel=1e-12)
    # the discrete actors: ActorSQN's test action is deterministic, so the host loop gives the same float twice
    qcase = Q_CASES[4]
    qa, _ = _q_actor(qcase, L)
    qhost, qdev = env.LunarLanderDiscrete(seed, L, **_model_kw()), _marker(DISC, seed, L)
    monkeypatch.setattr(qa, "evaluate_env", unsupported)
    seen = []
    for rnd in range(2):
        h, d = qa.test(qhost, n), qa.test(qdev, n)
        assert tuple(d) == tuple(h) and d[0] == d[1], (rnd, d, h)
        seen.append(d[0])
    assert qdev.episodes_played == 2 * n and seen[0] != seen[1]


def test_worker_test_round_with_test_on_device(ddrl):
    from distributed_drl_amd import env
    case = e3.TRACE_CASES[0]
    params = et.params_of(case)
    ps = ddrl.ParameterServer(list(params.keys()), list(params.values()))
    lines, lasts = {}, {}
    for on_device in (False, True):
        args = _opt(case.hid, 48, seed=9)
        args.env_model, args.env_velocity_iterations, args.env_position_iterations = "articulated", VIT, PIT
        got = lines[on_device] = []
        if on_device:
            args.test_on_device = True
            kw = {}
        else:      # the host env of the same model and seed
            kw = dict(make_env=lambda name: env.make(name, seed=9, max_ep_len=48, **_model_kw()))
        lasts[on_device] = ddrl.worker_test(ps, args, n=3, max_rounds=2, log=got.append, **kw)
        assert len(got) == 2 and all(s.startswith("AverageTestEpRet ") for s in got) and np.isfinite(lasts[on_device])
    ret = lambda s: s.split()[1]
    assert [ret(s) for s in lines[True]] == [ret(s) for s in lines[False]], lines
    assert lasts[True] == lasts[False], lasts
    assert ret(lines[True][0]) != ret(lines[True][1])      # the second round played other episodes
    # the worker built the marker itself, and without the flag nothing changes
    from distributed_drl_amd import workers
    args.test_on_device = True
    made = workers._default_test_env(args.env, args)
    assert type(made) is env.DeviceLunarLander and (made.model, made.velocity_iterations, made.position_iterations, made.seed) == ("articulated", VIT, PIT, 9)
    args.test_on_device = False
    assert type(workers._default_test_env(args.env, args)) is env.LunarLander


def test_worker_test_dqn_round_with_test_on_device(ddrl, tmp_path):
    """worker_test_dqn's printed lines from the device marker it builds under opt.test_on_device equal those from the host env of the
    same model (an SQN actor: its test action is deterministic; a counting clock makes the rate lines comparable)."""
    from distributed_drl_amd import dqn, env, workers

    class Opt:
        pass
    opt = Opt()
    opt.obs_dim, opt.act_dim, opt.hidden_size, opt.gamma, opt.lr, opt.polyak, opt.batch_size, opt.seed, opt.alpha = 8, 4, [32, 24], 0.99, 1e-3, 0.995, 16, 1, 0.1
    opt.buffer_size, opt.num_buffers, opt.num_nodes, opt.start_steps, opt.recover, opt.push_freq = 500, 1, 1, 40, False, 5
    opt.save_dir, opt.summary_dir, opt.save_interval, opt.checkpoint_freq = str(tmp_path), str(tmp_path / "tb"), 10 ** 9, 1e9
    opt.env_name, opt.exp_name, opt.num_workers, opt.a_l_ratio, opt.max_ep_len = DISC, "t", 1, 10, 40
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", VIT, PIT
    keys, values = dqn.LearnerSQN(opt, "ps").get_weights()
    ps = ddrl.ParameterServerNode(opt, keys=keys, values=values)
    node_buffer = [[ddrl.ReplayBufferDQN(opt, 0, seed=0)]]
    lines, rets = {}, {}
    for on_device in (False, True):
        opt.test_on_device = on_device
        ticks = iter(range(1, 10 ** 6))
        got = lines[on_device] = []
        kw = {} if on_device else dict(make_env=lambda: env.make(opt.env_name, seed=opt.seed, max_ep_len=opt.max_ep_len, **_model_kw()))
        rets[on_device] = workers.worker_test_dqn(ps, node_buffer, opt, node_ps=[ps], make_agent=lambda o: dqn.ActorSQN(o, job="test"),
                                                  clock=lambda: float(next(ticks)), log=got.append, wait=lambda ops, num_returns: None,
                                                  max_rounds=2, **kw)
    assert lines[True] == lines[False], lines
    assert rets[True] == rets[False] and np.isfinite(rets[True])
    value = [s for s in lines[True] if s.startswith("average test reward: ")]
    assert len(value) == 2 and value[0] != value[1]      # the second round played other episodes
