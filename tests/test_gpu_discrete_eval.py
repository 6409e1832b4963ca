"""The DQN / SQN test worker's evaluation episodes on the device (dqn.Actor.evaluate / ActorSQN.evaluate, ddrl_dqn_eval,
csrc/eval_q.hip), held to
  * the three trace checks of tests/_discrete_eval_trace.py (env half bit for bit against LanderOracle; q rows bit for bit against the
    float32 restatement of the kernel's summation order and within _acting_parity's bars of the float64 oracle; actions against the
    selection oracle on the device's own q rows and the oracle's uniforms — tests/test_discrete_eval_cpu.py shows that the checks see
    eight planted defects and that the inputs meet the conditions relied on here);
  * the stream and counter contracts (first_episode, 2 n max_ep_len uniforms per call), no side effects on the actor;
and Actor.test / ActorSQN.test on the device marker and on the host LunarLanderDiscrete, the error paths, the fallback outside the
kernel's envelope, and a worker_test_dqn round."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_eval_trace as dt  # noqa: E402

from oracle import dqn_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _actor(case, max_ep_len=None, max_rows=1):
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


def _evaluate(actor, case, n=None, first=None, trace=True):
    return actor.evaluate(case.n if n is None else n, case.seed, case.first if first is None else first, case.max_ep_len,
                          deterministic=case.deterministic, greedy_prob=case.greedy, trace=trace)


def _same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


@pytest.mark.parametrize("case", dt.TRACE_CASES + [dt.TIE_CASE] + dt.WIDE_CASES, ids=repr)
def test_trace_passes_the_three_checks(ddrl, case):
    actor, params = _actor(case)
    out = _evaluate(actor, case)
    assert out["ret"].dtype == np.float64 and out["len"].dtype == np.int32 and out["trace"].dtype == np.float32
    assert out["trace"].shape == (case.n, case.max_ep_len, 20)
    assert actor._noise_ctr == case.ctr + 2 * case.n * case.max_ep_len
    table = []
    try:
        dt.check_all(out, case, params, table=table)
    finally:
        print("\n".join(ap.format_table(table)))
    if case is dt.TIE_CASE:
        q = dt.played_rows(out)[:, 8:12]
        assert ((q[:, 1] == q[:, 2]) & (q[:, 1] >= q.max(axis=1))).sum() >= 8


def test_first_episode_positions_the_stream(ddrl):
    long, short = dt.FIRST_CASES
    actor, params = _actor(long)
    a, b = _evaluate(actor, long), _evaluate(actor, short)
    for out, case in ((a, long), (b, short)):
        dt.check_env(out, case.seed, case.first, case.max_ep_len, case.id)
        dt.check_q(out, case, params)
    assert _same_bits(a["trace"][5:8], b["trace"])
    assert (a["ret"][5:8] == b["ret"]).all() and (a["len"][5:8] == b["len"]).all()


def test_two_calls_equal_one_call_split_at_the_counter(ddrl):
    case = dt.COUNTER_CASE
    actor, params = _actor(case)
    whole = _evaluate(actor, case)
    assert actor._noise_ctr == case.ctr + 2 * 4 * case.max_ep_len
    dt.check_all(whole, case, params)
    actor._noise_ctr = case.ctr
    first = _evaluate(actor, case, n=2, first=0)
    assert actor._noise_ctr == case.ctr + 2 * 2 * case.max_ep_len
    second = _evaluate(actor, case, n=2, first=2)      # at the counter the first call left behind
    assert actor._noise_ctr == case.ctr + 2 * 4 * case.max_ep_len
    for part, got in ((slice(0, 2), first), (slice(2, 4), second)):
        assert _same_bits(whole["trace"][part], got["trace"])
        assert (whole["ret"][part] == got["ret"]).all() and (whole["len"][part] == got["len"]).all()
    assert not _same_bits(first["trace"], second["trace"])


@pytest.mark.parametrize("case", [dt.COUNTER_CASE, dt.TRACE_CASES[5]], ids=repr)
def test_evaluate_has_no_side_effects(ddrl, case):
    from distributed_drl_amd import _lib
    actor, _ = _actor(case, max_rows=32)
    actor.train(do.synthetic_batch(ap.q_cfg(ap.QCase("b", case.family, 8, case.acts, case.hid, 32)), 500), 0)      # Adam slots off zero
    obs = np.random.RandomState(4).randn(32, 8).astype(np.float32)
    which = (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M)

    def act():
        actor._noise_ctr = 4000
        q = torch.empty(32, case.acts, device="cuda")
        return actor.get_actions(obs, q_out=q).clone(), q
    a0, q0 = act()
    before = [actor.export(w).clone() for w in which]
    assert before[2].abs().max().item() > 0
    actor._noise_ctr = case.ctr
    plain = actor.evaluate(case.n, case.seed, 0, case.max_ep_len, greedy_prob=case.greedy)
    assert actor._noise_ctr == case.ctr + 2 * case.n * case.max_ep_len
    actor._noise_ctr = case.ctr
    traced = actor.evaluate(case.n, case.seed, 0, case.max_ep_len, greedy_prob=case.greedy, trace=True)
    assert "trace" not in plain and (plain["ret"] == traced["ret"]).all() and (plain["len"] == traced["len"]).all()
    for w, b in zip(which, before):
        assert torch.equal(actor.export(w), b), "export(%d) changed across evaluate" % w
    a1, q1 = act()
    assert torch.equal(a0, a1) and torch.equal(q0, q1)
    # the defaults are the class's _test_action: Double-DQN samples with greedy_prob 0.97, SQN is deterministic; max_ep_len from opt
    actor._noise_ctr = case.ctr
    default = actor.evaluate(2, case.seed)
    actor._noise_ctr = case.ctr
    explicit = actor.evaluate(2, case.seed, 0, actor.opt.max_ep_len, deterministic=case.family == "sqn", greedy_prob=0.97)
    assert (default["ret"] == explicit["ret"]).all() and default["len"].max() <= actor.opt.max_ep_len


@pytest.mark.parametrize("case", [dt.TRACE_CASES[0], dt.TRACE_CASES[4]], ids=repr)
def test_actor_test_on_the_device_marker(ddrl, case):
    """Fails without the feature: env.make("LunarLander-v2", on_device=True) returned the continuous marker, and Actor.test stepped it."""
    from distributed_drl_amd import env
    actor, _ = _actor(case)
    n, seed, L = 3, 7, case.max_ep_len
    dev = env.make("LunarLander-v2", on_device=True, seed=seed, max_ep_len=L)
    assert isinstance(dev, env.DeviceLunarLanderDiscrete) and isinstance(dev, env.DeviceLunarLander) and dev.action_space.n == 4
    assert ddrl.DeviceLunarLanderDiscrete is env.DeviceLunarLanderDiscrete
    seen = []
    for rnd in range(2):
        ctr = actor._noise_ctr
        got = actor.test(dev, n)
        assert isinstance(got, tuple) and len(got) == 2 and type(got[0]) is float and type(got[1]) is float and got[0] == got[1]
        assert dev.episodes_played == n * (rnd + 1) and actor._noise_ctr == ctr + 2 * n * L
        actor._noise_ctr = ctr
        out = actor.evaluate(n, seed, n * rnd, L)
        assert got[0] == float(np.mean(out["ret"])), (rnd, got, out)
        seen.append(got[0])
    assert seen[0] != seen[1]      # the second round played other episodes


@pytest.mark.parametrize("case", [dt.TRACE_CASES[0], dt.TRACE_CASES[4]], ids=repr)
def test_actor_test_on_the_host_lander(ddrl, case):
    """Raised AttributeError without the feature: LunarLanderDiscrete had no `rewards`."""
    from distributed_drl_amd import env
    actor, _ = _actor(case)
    host = env.make("LunarLander-v2", seed=7, max_ep_len=case.max_ep_len)
    assert isinstance(host, env.LunarLanderDiscrete) and host.rewards == [0.0]
    ret, score = actor.test(host, 2)
    assert np.isfinite(ret) and score == ret
    host.reset()
    assert host.rewards == [0.0]
    total = 0
    for k in range(5):
        total += host.step(k % 4)[1]
    assert host.rewards[0] == total and type(host.rewards[0]) is float
    host.reset()
    assert host.rewards == [0.0]


def test_error_paths(ddrl):
    from distributed_drl_amd import _lib, env
    case = dt.TRACE_CASES[0]
    actor, _ = _actor(case)
    with pytest.raises(ValueError, match="max_ep_len"):
        actor.test(env.DeviceLunarLanderDiscrete(1, case.max_ep_len + 1), 2)
    with pytest.raises(RuntimeError, match="not steppable"):
        env.DeviceLunarLanderDiscrete(1, 40).step(0)
    lib = _lib.load()
    flat = actor.export()
    ret, ln = torch.empty(4, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda")
    tr = torch.empty(4, 40, 20, device="cuda")

    def call(n=1, L=40, first=0, mode=_lib.DDRL_ACT_SAMPLE, trace=None, **cfg_fields):
        cfg = _lib.DqnConfig(8, 4, case.hid[0], case.hid[1], 1)
        for k, v in cfg_fields.items():
            setattr(cfg, k, v)
        return lib.ddrl_dqn_eval(ctypes.byref(cfg), _lib.dptr(flat), n, 0, first, L, mode, 0.97, 1, 0, _lib.dptr(ret), _lib.dptr(ln),
                                 trace, _lib.stream_ptr())
    bad = dict(obs_dim=call(obs_dim=9), n_actions=call(n_actions=0), n_episodes=call(n=0), max_ep_len=call(L=0), hidden1=call(hidden1=0),
               hidden2=call(hidden2=0), max_ep_len_inexact=call(L=(1 << 24) + 1), episode_inexact=call(n=2, first=(1 << 24) - 1),
               trace_misaligned=call(trace=ctypes.c_void_p(tr.data_ptr() + 4)), mode=call(mode=2))
    assert all(rc == _lib.DDRL_ERR_BAD_ARG for rc in bad.values()), bad
    with pytest.raises(ValueError, match="ddrl"):
        _lib.check(call(obs_dim=9))
    for fields, word in ((dict(hidden1=600), b"512"), (dict(hidden2=600), b"512"), (dict(n_actions=9), b"n_actions")):
        assert call(**fields) == _lib.DDRL_ERR_UNSUPPORTED and word in lib.ddrl_last_error(), fields
    with pytest.raises(_lib.DdrlUnsupported):
        _lib.check(call(hidden1=600))
    assert call(n=1, L=40, trace=_lib.dptr(tr)) == _lib.DDRL_OK      # ... and the same call with nothing wrong goes through
    torch.cuda.synchronize()


def test_outside_the_envelope_falls_back_to_the_host_loop(ddrl, monkeypatch):
    """ddrl_dqn_eval answers DDRL_ERR_UNSUPPORTED for a hidden width > 512 or more than 8 actions (test_error_paths).  The fallback is
    driven by an evaluate that raises what _lib.check raises for that status: the host env it steps instead must sit at the same
    episode, in both rounds.  SQN: its test action is deterministic, so the host loop gives the same float twice."""
    from distributed_drl_amd import env
    case = dt.TRACE_CASES[4]
    n, L, seed = 2, 30, 5
    actor, _ = _actor(case, L)
    host, dev = env.LunarLanderDiscrete(seed, L), env.DeviceLunarLanderDiscrete(seed, L)

    def unsupported(*a, **kw):
        raise ddrl._lib.DdrlUnsupported("ddrl error -5: outside the envelope")
    monkeypatch.setattr(actor, "evaluate", unsupported)
    got = []
    for rnd in range(2):     # the second round starts the fallback's host env at episode n
        h, d = actor.test(host, n), actor.test(dev, n)
        assert tuple(d) == tuple(h) and d[0] == d[1], (rnd, d, h)
        got.append(d[0])
    assert dev.episodes_played == 2 * n and got[0] != got[1]
    assert isinstance(dev.host_env(), env.LunarLanderDiscrete)


@pytest.mark.parametrize("on_device", [True, False])
def test_one_worker_test_dqn_round(ddrl, tmp_path, on_device):
    """worker_test_dqn on the project's own lander: the device marker, and its default make_env (the host LunarLanderDiscrete)."""
    from distributed_drl_amd import dqn, env, workers

    class Opt:
        pass
    opt = Opt()
    opt.obs_dim, opt.act_dim, opt.hidden_size, opt.gamma, opt.lr, opt.polyak, opt.batch_size, opt.seed, opt.alpha = 8, 4, [32, 24], 0.99, 1e-3, 0.995, 16, 1, 0.1
    opt.buffer_size, opt.num_buffers, opt.num_nodes, opt.start_steps, opt.recover, opt.push_freq = 500, 1, 1, 40, False, 5
    opt.save_dir, opt.summary_dir, opt.save_interval, opt.checkpoint_freq = str(tmp_path), str(tmp_path / "tb"), 10 ** 9, 1e9
    opt.env_name, opt.exp_name, opt.num_workers, opt.a_l_ratio, opt.max_ep_len = "LunarLander-v2", "t", 1, 10, 40
    keys, values = dqn.Learner(opt, "ps").get_weights()
    ps = ddrl.ParameterServerNode(opt, keys=keys, values=values)
    node_buffer = [[ddrl.ReplayBufferDQN(opt, 0, seed=0)]]
    lines = []
    kw = dict(make_env=lambda: env.make(opt.env_name, on_device=True, seed=opt.seed, max_ep_len=opt.max_ep_len)) if on_device else {}
    ret = workers.worker_test_dqn(ps, node_buffer, opt, node_ps=[ps], log=lines.append, wait=lambda ops, num_returns: None, max_rounds=1, **kw)
    assert np.isfinite(ret)
    for head in ("average test reward: ", "average test score: ", "frame freq: ", "actor_steps: ", "actor leaner ratio: ", "learner freq: "):
        assert sum(s.startswith(head) for s in lines) == 1, (head, lines)
    value = lambda head: [s for s in lines if s.startswith(head)][0][len(head):]
    assert value("average test reward: ") == str(ret) and value("average test score: ") == str(ret)
