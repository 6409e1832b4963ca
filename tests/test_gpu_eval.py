"""The test worker's evaluation episodes on the device (Actor.evaluate / ddrl_policy_eval, csrc/eval.hip), held to
  * the two trace checks of tests/_eval_trace.py (env half bit for bit against LanderOracle, policy half against the float64 oracle
    within _acting_parity's bars; tests/test_eval_cpu.py shows that the checks see five planted defects);
  * the host loop it replaces, bit for bit: Actor.test / Model.test_agent on env.LunarLander and on env.DeviceLunarLander return
    equal floats, per-episode returns and lengths equal those of the loop written out below, over two consecutive rounds on the
    same env objects (the episode count carries over);
and its error paths, its fallback outside the kernel's envelope, and a worker_test round."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_trace as et  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(hid, max_ep_len, seed=0):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.hidden_sizes, opt.max_ep_len, opt.seed, opt.env = tuple(hid), max_ep_len, seed, "LunarLanderContinuous-v2"
    return opt


def _actor(case, max_ep_len=None):
    from distributed_drl_amd.agent import Actor
    actor = Actor(_opt(case.hid, case.max_ep_len if max_ep_len is None else max_ep_len), max_rows=1)
    params = et.params_of(case)
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


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


@pytest.mark.parametrize("case", et.TRACE_CASES, ids=repr)
def test_trace_passes_both_checks(ddrl, case):
    actor, params = _actor(case)
    out = actor.evaluate(case.n, case.seed, case.first, case.max_ep_len, trace=True)
    assert out["ret"].dtype == np.float64 and out["trace"].dtype == np.float32 and out["trace"].shape == (case.n, case.max_ep_len, 12)
    et.check_env(out, case.seed, case.first, case.max_ep_len, case.id)
    et.check_policy(out, case, params)


def test_first_episode_positions_the_stream(ddrl):
    long, short = et.FIRST_CASES
    actor, params = _actor(long)
    a = actor.evaluate(long.n, long.seed, 0, long.max_ep_len, trace=True)
    b = actor.evaluate(short.n, short.seed, short.first, short.max_ep_len, trace=True)
    for out, case in ((a, long), (b, short)):
        et.check_env(out, case.seed, case.first, case.max_ep_len, case.id)
        et.check_policy(out, case, params)
    assert (a["trace"][5:8].view(np.uint32) == b["trace"].view(np.uint32)).all()
    assert (a["ret"][5:8] == b["ret"]).all() and (a["len"][5:8] == b["len"]).all()


@pytest.mark.parametrize("n,max_ep_len", [(3, 48), (2, 300)])
def test_actor_test_equals_the_host_loop(ddrl, n, max_ep_len):
    from distributed_drl_amd import env
    case = et.TRACE_CASES[0]
    actor, _ = _actor(case, max_ep_len)
    seed = 7
    host, dev, loop_env = env.LunarLander(seed, max_ep_len), env.make("LunarLanderContinuous-v2", on_device=True, seed=seed, max_ep_len=max_ep_len), env.LunarLander(seed, max_ep_len)
    assert isinstance(dev, env.DeviceLunarLander)
    for rnd in range(2):
        want, got = actor.test(host, None, n), actor.test(dev, None, n)
        assert isinstance(got, float) and got == want, (rnd, got, want)
        assert dev.episodes_played == n * (rnd + 1)
        rets, lens = _host_loop(actor, loop_env, n, max_ep_len)
        out = actor.evaluate(n, seed, n * rnd, max_ep_len)
        assert out["ret"].tolist() == rets and out["len"].tolist() == lens, (rnd, out, rets, lens)
        assert want == sum(rets) / n


class _Args:
    env, obs_dim, act_dim = "LunarLanderContinuous-v2", 8, 2
    ac_kwargs = dict(hidden_sizes=[64, 48])
    gamma = 0.99,
    polyak, lr, alpha, batch_size, seed = 0.995, 1e-3, 0.2, 32, 4
    max_ep_len = 48


def test_model_test_agent_equals_the_host_loop(ddrl):
    """Model.get_action(o, deterministic=True) is the one-launch get_action too, so the SAC-v model's host loop and the device episodes
    are the same arithmetic."""
    from distributed_drl_amd import env
    from distributed_drl_amd.agent import Model
    args, n, seed = _Args(), 3, 7
    net = Model(args)
    host, dev = env.LunarLander(seed, args.max_ep_len), env.DeviceLunarLander(seed, args.max_ep_len)
    for rnd in range(2):
        want, got = net.test_agent(host, args, n), net.test_agent(dev, args, n)
        print("Model.test_agent round %d: host %r device %r diff %.3e" % (rnd, want, got, got - want))
        assert got == want, (rnd, got, want)
    assert dev.episodes_played == 2 * n


def test_evaluate_has_no_side_effects(ddrl):
    case = et.TRACE_CASES[0]
    actor, params = _actor(case)
    ctr, before = actor._noise_ctr, actor.get_weights_flat().clone()
    plain = actor.evaluate(case.n, case.seed, 0, case.max_ep_len)
    traced = actor.evaluate(case.n, case.seed, 0, case.max_ep_len, trace=True)
    assert "trace" not in plain and (plain["ret"] == traced["ret"]).all() and (plain["len"] == traced["len"]).all()
    assert actor._noise_ctr == ctr and torch.equal(actor.get_weights_flat(), before)
    assert actor.evaluate(2, case.seed)["len"].max() <= actor.opt.max_ep_len      # max_ep_len defaults to opt.max_ep_len


def test_error_paths(ddrl):
    from distributed_drl_amd import _lib, env
    case = et.TRACE_CASES[0]
    actor, _ = _actor(case)
    with pytest.raises(ValueError, match="max_ep_len"):
        actor.test(env.DeviceLunarLander(1, case.max_ep_len + 1), None, 2)
    with pytest.raises(RuntimeError, match="not steppable"):
        env.DeviceLunarLander(1, 40).step(np.zeros(2))
    cfg = actor.opt.config()
    cfg.obs_dim = 9
    flat, ret, ln = actor.get_weights_flat(), torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    call = lambda c, n, L: lib.ddrl_policy_eval(ctypes.byref(c), _lib.dptr(flat), n, 0, 0, L, _lib.dptr(ret), _lib.dptr(ln), None, _lib.stream_ptr())
    with pytest.raises(ValueError, match="ddrl"):
        _lib.check(call(cfg, 1, 40))
    cfg = actor.opt.config()
    assert call(cfg, 0, 40) == _lib.DDRL_ERR_BAD_ARG and call(cfg, 1, 0) == _lib.DDRL_ERR_BAD_ARG
    cfg.act_dim = 3
    assert call(cfg, 1, 40) == _lib.DDRL_ERR_BAD_ARG
    cfg = actor.opt.config()
    cfg.hidden1 = 600
    assert call(cfg, 1, 40) == _lib.DDRL_ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_outside_the_envelope_falls_back_to_the_host_loop(ddrl, monkeypatch):
    """ddrl_policy_eval answers DDRL_ERR_UNSUPPORTED for a hidden width > 512 (test_error_paths) — but no Actor of that shape can be
    built (ddrl_actor_create refuses hidden sizes > 512: the row kernels' limit), so through an Actor the answer cannot occur today.
    The fallback is therefore driven by an evaluate that raises what _lib.check raises for that status: the host env it steps
    instead must sit at the same episode, in both rounds."""
    from distributed_drl_amd import env
    from distributed_drl_amd.agent import Actor
    n, max_ep_len, seed = 2, 30, 5
    with pytest.raises(ValueError, match="512"):
        Actor(_opt((600, 300), max_ep_len, seed=2), max_rows=1)
    actor, _ = _actor(et.TRACE_CASES[0], max_ep_len)
    want = [actor.test(env.DeviceLunarLander(seed, max_ep_len), None, 2 * n)]      # the device path over the same four episodes
    host, dev = env.LunarLander(seed, max_ep_len), env.DeviceLunarLander(seed, max_ep_len)

    def unsupported(*a, **kw):
        raise ddrl._lib.DdrlUnsupported("ddrl error -5: outside the envelope")
    monkeypatch.setattr(actor, "evaluate", unsupported)
    got = []
    for rnd in range(2):     # the second round starts the fallback's host env at episode n
        h, d = actor.test(host, None, n), actor.test(dev, None, n)
        assert d == h, (rnd, d, h)
        got.append(d)
    assert dev.episodes_played == 2 * n and got[0] != got[1]
    assert (got[0] + got[1]) / 2 == pytest.approx(want[0], rel=1e-12)


def test_worker_test_round_on_the_device_env(ddrl):
    from distributed_drl_amd import env
    case = et.TRACE_CASES[0]
    args = _opt(case.hid, 48, seed=1)
    params = et.params_of(case)
    ps = ddrl.ParameterServer(list(params.keys()), list(params.values()))
    lines, lasts = {}, {}
    for on_device in (False, True):
        got = lines[on_device] = []
        last = ddrl.worker_test(ps, args, n=3, max_rounds=2, log=got.append,
                                make_env=lambda name: env.make(name, on_device=on_device, seed=9, max_ep_len=args.max_ep_len))
        assert len(got) == 2 and all(s.startswith("AverageTestEpRet ") for s in got) and np.isfinite(last)
        lasts[on_device] = last
    ret = lambda s: s.split()[1]
    assert [ret(s) for s in lines[True]] == [ret(s) for s in lines[False]], lines
    assert lasts[True] == lasts[False], lasts
    assert ret(lines[True][0]) != ret(lines[True][1])      # the second round played other episodes
