"""The walker's evaluation episodes on the device, fed from handles (ddrl_env_eval_policy_walker, csrc/walker_eval.hip;
ddrl_env_eval_results; Actor.evaluate_env on an env.DeviceBipedalWalker), held to
  * the trace checks: the env half bit for bit against tests/walker_oracle.WalkerOracle (tests/_walker_eval_trace.py;
    tests/test_walker_eval_cpu.py shows what it sees), the policy half by _acting_parity.actor_reference / compare with its bars;
  * the stream contract of first_episode;
  * the host loop it replaces, bit for bit: Actor.test on the host env.BipedalWalker and on the device marker, per-episode returns and
    lengths equal to the loop written out;
and: no side effects on the lending handle or the actor, the results block's bookkeeping, every refusal (status, text, nothing
launched; the two lander kinds among them), the DdrlUnsupported fallback and a worker_test round with opt.test_on_device.

The fallback: an Actor with a hidden width of 520 cannot be built (ddrl_actor_create refuses hidden sizes > 512), so — as in
tests/test_gpu_eval3.py — it is driven by an evaluate_env that raises what _lib.check raises for DDRL_ERR_UNSUPPORTED."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _walker_eval_trace as wt  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = b"ddrl_env_eval_policy_walker"
WALKER, CONT = "BipedalWalker-v2", "LunarLanderContinuous-v2"
VIT, PIT = 8, 3


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _marker(seed, max_ep_len, vit=VIT, pit=PIT):
    from distributed_drl_amd import env
    return env.DeviceBipedalWalker(seed, max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _host(seed, max_ep_len, vit=VIT, pit=PIT):
    from distributed_drl_amd import env
    return env.make(WALKER, model="walker", seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _opt(hid, max_ep_len, seed=0, obs_dim=24, act_dim=4):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=obs_dim, act_dim=act_dim)
    opt.hidden_sizes, opt.max_ep_len, opt.seed, opt.env = tuple(hid), max_ep_len, seed, WALKER
    return opt


def _actor(case, max_ep_len=None):
    from distributed_drl_amd.agent import Actor
    actor = Actor(_opt(case.hid, case.max_ep_len if max_ep_len is None else max_ep_len), max_rows=1)
    params = wt.params_of(case)
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _same_out(a, b):
    return _same_bits(a["trace"], b["trace"]) and (a["ret"] == b["ret"]).all() and (a["len"] == b["len"]).all()


# ---- 1. trace cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wt.TRACE_CASES, ids=repr)
def test_policy_trace_passes_both_checks(ddrl, case):
    actor, params = _actor(case)
    dev = _marker(case.seed, case.max_ep_len, case.vit, case.pit)
    out = actor.evaluate_env(dev, case.n, case.first, trace=True)
    assert out["ret"].dtype == np.float64 and out["len"].dtype == np.int32 and out["trace"].dtype == np.float32
    assert out["trace"].shape == (case.n, case.max_ep_len, 32) and dev.episodes_played == 0
    wt.check_env_walker(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)
    table = []
    try:
        wt.check_policy(out, case, params, table=table)
    finally:
        print("\n".join(ap.format_table(table)))
    last = np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    # what tests/test_walker_eval_cpu.py asserts on the oracle's traces holds for the device's
    if case is wt.TERMINAL_CASE:
        assert out["len"].tolist() == [54, 54, 54] and (last[:, wt.I_REW] == -100).all() and len(set(out["ret"].tolist())) == 3
        rows = wt.played_rows(out)[0]
        assert ((rows[:, 8] == 1) | (rows[:, 13] == 1)).any()
    if case is wt.WIDE_CASE:
        assert out["len"].tolist() == [79, 79] and (last[:, wt.I_REW] == -100).all()
    if case is wt.LIMIT_CASE:
        assert (out["len"] == case.max_ep_len).all() and (last[:, wt.I_REW] != -100).all() and (last[:, wt.I_END] == 1).all()


# ---- 2. first_episode ---------------------------------------------------------------------------------------------------------------
def test_first_episode_positions_the_stream(ddrl):
    long, short = wt.FIRST_CASES
    actor, _ = _actor(long)
    dev = _marker(long.seed, long.max_ep_len)
    a = actor.evaluate_env(dev, long.n, 0, trace=True)
    b = actor.evaluate_env(dev, short.n, short.first, trace=True)
    assert _same_out({k: v[5:8] for k, v in a.items()}, b)
    assert not _same_bits(a["trace"][0:3], b["trace"])
    wt.check_env_walker(b, short.seed, short.first, short.max_ep_len, short.vit, short.pit, short.id)
    # the default is the marker's episode count
    dev.episodes_played = 5
    assert _same_out(actor.evaluate_env(dev, 3, trace=True), b)


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
    n, L, seed = 2, 30, 7
    actor, _ = _actor(wt.TRACE_CASES[0], L)
    host, loop_env = _host(seed, L), _host(seed, L)
    assert type(host) is env.BipedalWalker
    dev = _marker(seed, L)
    assert type(dev) is env.DeviceBipedalWalker and (dev.model, dev.on_device) == ("walker", True)
    seen = []
    for rnd in range(2):
        want, got = actor.test(host, None, n), actor.test(dev, None, n)
        assert isinstance(got, float) and got == want, (rnd, got, want)
        assert dev.episodes_played == n * (rnd + 1)
        rets, lens = _host_loop(actor, loop_env, n, L)
        out = actor.evaluate_env(dev, n, n * rnd)
        assert "trace" not in out and out["ret"].tolist() == rets and out["len"].tolist() == lens, (rnd, out, rets, lens)
        assert want == sum(rets) / n
        seen.append(rets)
    assert seen[0] != seen[1]      # the second round played other episodes


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------------------
def test_evaluation_has_no_side_effects(ddrl):
    from distributed_drl_amd import _lib, env
    case = wt.TRACE_CASES[0]
    actor, _ = _actor(case)
    lib = _lib.load()
    vecs = [env.VecBipedalWalker(4, seed=11, max_ep_len=9, velocity_iterations=VIT, position_iterations=PIT) for _ in range(2)]
    acts = [torch.tensor(np.random.RandomState(k).uniform(-1, 1, (4, 4)).astype(np.float32), device="cuda") for k in range(12)]
    for v in vecs:
        for a in acts[:10]:      # past one time limit: the statistics are off zero
            v.step(a)
    ctr, before = actor._noise_ctr, actor.get_weights_flat().clone()
    obs_before = vecs[0].obs.clone()
    _lib.check(lib.ddrl_env_eval_policy_walker(vecs[0]._h, actor._h, 3, 4, 1, _lib.stream_ptr()))
    plain = env.eval_results(vecs[0], 32)
    assert plain["trace"].shape == (3, 9, 32)
    assert actor._noise_ctr == ctr and torch.equal(actor.get_weights_flat(), before)
    assert torch.equal(vecs[0].get_state().view(torch.int32), vecs[1].get_state().view(torch.int32))
    assert torch.equal(vecs[0].obs.view(torch.int32), obs_before.view(torch.int32))
    outs = [[t.clone() for t in v.step(acts[10])] for v in vecs]
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert vecs[0].stats() == vecs[1].stats() and vecs[0].stats()[0] == 0
    # the same episodes from a one-env marker of that seed: n_envs of the lending handle does not matter
    assert _same_out(actor.evaluate_env(_marker(11, 9), 3, 4, trace=True), plain)


# ---- 5. the results block -------------------------------------------------------------------------------------------------------------
def _results(lib, h):
    p = [ctypes.c_void_p() for _ in range(3)]
    k = [ctypes.c_int32(-1) for _ in range(3)]
    rc = lib.ddrl_env_eval_results(h, *[ctypes.byref(x) for x in p + k])
    return rc, [x.value for x in p], [x.value for x in k]


def test_results_block(ddrl):
    from distributed_drl_amd import _lib, env
    case = wt.TRACE_CASES[0]
    L = 20
    actor, _ = _actor(case, L)
    lib = _lib.load()
    vec = env.VecBipedalWalker(1, seed=3, max_ep_len=L, velocity_iterations=VIT, position_iterations=PIT)
    rc, _, _ = _results(lib, vec._h)
    assert rc == _lib.DDRL_ERR_BAD_ARG and b"no evaluation" in lib.ddrl_last_error()
    seen = []
    for n, trace in ((2, True), (5, False), (5, True), (2, False), (2, True)):
        _lib.check(lib.ddrl_env_eval_policy_walker(vec._h, actor._h, n, 0, 1 if trace else 0, _lib.stream_ptr()))
        rc, (ret, ln, tr), (rn, rL, row) = _results(lib, vec._h)
        assert rc == _lib.DDRL_OK and (rn, rL, row) == (n, L, 32 if trace else 0)
        assert ret and ln and ret % 256 == 0 and ln % 16 == 0 and ln >= ret + 8 * n
        assert (tr is None) == (not trace)
        if trace:
            assert tr % 16 == 0 and tr >= ln + 4 * n
        out = env.eval_results(vec, 32)
        assert out["ret"].shape == (n,) and out["len"].shape == (n,) and ("trace" in out) == trace
        if trace:
            assert out["trace"].shape == (n, L, 32)
            for e, l in enumerate(out["len"]):
                assert out["trace"][e, :l, wt.I_END].sum() == 1 and not out["trace"][e, l:].view(np.uint32).any()
        seen.append((n, trace, ret, out))
    # the same call gives the same results, wherever the block lies; once grown for (5, trace) the block stays where it is
    assert _same_out(seen[0][3], seen[4][3]) and (seen[1][3]["ret"] == seen[2][3]["ret"]).all()
    assert seen[2][2] == seen[3][2] == seen[4][2]
    # a trace of another row length is refused by the reader, not misread
    with pytest.raises(_lib.DdrlError, match="32"):
        env.eval_results(vec, 12)


# ---- 6. every refusal -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ddrl):
    from distributed_drl_amd import _lib, env
    from distributed_drl_amd.agent import Actor
    case, L = wt.TRACE_CASES[0], 10
    actor, _ = _actor(case, L)
    lib, s = _lib.load(), _lib.stream_ptr
    vec = env.VecBipedalWalker(1, seed=3, max_ep_len=L, velocity_iterations=VIT, position_iterations=PIT)
    _lib.check(lib.ddrl_env_eval_policy_walker(vec._h, actor._h, 2, 0, 1, s()))
    torch.cuda.synchronize()
    rc, (ret, ln, tr), sizes = _results(lib, vec._h)
    assert rc == _lib.DDRL_OK
    # a sentinel over the whole results block: a launch would overwrite ret, len and (rows past the end included) every trace element
    nbytes = tr + 2 * L * 32 * 4 - ret

    class _Holder:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ret), False), "version": 2}
    block = torch.as_tensor(_Holder(), device="cuda")
    block.fill_(0xA5)
    torch.cuda.synchronize()

    three = Actor(_opt(case.hid, L, act_dim=3), max_rows=1)                    # 24 -> 3
    lander_actor = Actor(_opt(case.hid, L, obs_dim=8, act_dim=2), max_rows=1)  # 8 -> 2
    landers = {"one-body": env.VecLunarLander(1, seed=3, max_ep_len=L),
               "articulated": env.VecLunarLander(1, seed=3, max_ep_len=L, model="articulated", velocity_iterations=VIT, position_iterations=PIT)}
    lander_states = {k: v.get_state().clone() for k, v in landers.items()}

    pol = lambda h, a, n=2, first=0: lib.ddrl_env_eval_policy_walker(h, a, n, first, 1, s())
    B, U = _lib.DDRL_ERR_BAD_ARG, _lib.DDRL_ERR_UNSUPPORTED
    refusals = [
        ("NULL env handle", lambda: pol(None, actor._h), B, b"NULL handle"),
        ("NULL actor", lambda: pol(vec._h, None), B, b"NULL handle"),
        ("n_episodes 0", lambda: pol(vec._h, actor._h, n=0), B, b"n_episodes"),
        ("n_episodes -1", lambda: pol(vec._h, actor._h, n=-1), B, b"n_episodes"),
        ("episode index past 2^24", lambda: pol(vec._h, actor._h, n=2, first=(1 << 24) - 1), B, b"2^24"),
        ("actor 24 -> 3", lambda: pol(vec._h, three._h), B, b"24 observations and 4 actions"),
        ("actor 8 -> 2", lambda: pol(vec._h, lander_actor._h), B, b"24 observations and 4 actions"),
        ("a one-body handle", lambda: pol(landers["one-body"]._h, lander_actor._h), U, b"the one-body model"),
        ("an articulated handle", lambda: pol(landers["articulated"]._h, lander_actor._h), U, b"the articulated lander"),
    ]
    if torch.cuda.device_count() > 1:      # handles on different devices (needs a second device to build one on)
        with torch.cuda.device(1):
            far = env.VecBipedalWalker(1, seed=3, max_ep_len=L, velocity_iterations=VIT, position_iterations=PIT)
        refusals.append(("other device", lambda: pol(far._h, actor._h), B, b"device"))
    for what, call, status, word in refusals:
        rc = call()
        text = lib.ddrl_last_error()
        assert rc == status, (what, rc, text)
        assert word in text and text.startswith(NAME + b":"), (what, text)
        if "handle" in what and status == U:      # both landers share their entry point: no suffix of the model behind it
            assert text.endswith(b"use ddrl_env_eval_policy") and b"built for the walker (DDRL_ENV_WALKER)" in text, text
    with pytest.raises(_lib.DdrlUnsupported):
        _lib.check(pol(landers["articulated"]._h, lander_actor._h))
    with pytest.raises(ValueError, match="ddrl"):
        _lib.check(pol(vec._h, actor._h, n=0))
    torch.cuda.synchronize()
    assert bool((block == 0xA5).all()), "a refused call wrote into the results block"
    assert _results(lib, vec._h) == (_lib.DDRL_OK, [ret, ln, tr], sizes)      # ... and the previous results are still the handle's
    for k, v in landers.items():      # the lander handles: no results block, their state as it was
        assert _results(lib, v._h)[0] == B and torch.equal(v.get_state().view(torch.int32), lander_states[k].view(torch.int32)), k
    # the landers' entry points keep refusing a walker handle, and it has no results of theirs
    assert lib.ddrl_env_eval_policy(vec._h, actor._h, 2, 0, 1, s()) == U and b"walker" in lib.ddrl_last_error()
    assert bool((block == 0xA5).all())
    # the same call with nothing wrong goes through (it fits the block: the sentinel view still points into it)
    assert pol(vec._h, actor._h) == _lib.DDRL_OK
    torch.cuda.synchronize()
    assert not bool((block[:16] == 0xA5).all())
    del block


# ---- 7. door, fallback, workers ---------------------------------------------------------------------------------------------------------
def test_the_marker_and_the_doors_that_stay_shut(ddrl):
    from distributed_drl_amd import env
    a = env.DeviceBipedalWalker(4, 30, velocity_iterations=VIT, position_iterations=PIT)
    d = ddrl.DeviceBipedalWalker()
    assert (d.seed, d.max_ep_len, d.velocity_iterations, d.position_iterations, d.episodes_played) == (0, 1600, 180, 60, 0)
    assert (a.model, a.velocity_iterations, a.position_iterations, a.seed, a.max_ep_len, a.on_device) == ("walker", VIT, PIT, 4, 30, True)
    assert a.reset().shape == (24,) and not a.reset().any() and a.action_space.shape == (4,) and a.observation_space.shape == (24,)
    with pytest.raises(RuntimeError, match="not steppable"):
        a.step(np.zeros(4))
    for door in (lambda: env.make(WALKER, model="walker", on_device=True), lambda: env.make_device(WALKER, model="walker")):
        with pytest.raises(ValueError, match="DeviceBipedalWalker"):
            door()
    # the lending handle and the host env are of the marker's model
    assert type(a.handle()) is env.VecBipedalWalker and a.handle().n == 1 and a.handle().state_fields == 286 and a.handle() is a.handle()
    a.episodes_played = 3
    host = a.host_env()
    assert type(host) is env.BipedalWalker and float(host._vec.get_state()[13, 0]) == 3.0
    assert (host._vec.seed, host._vec.max_ep_len) == (4, 30)


def test_outside_the_envelope_falls_back_to_the_host_loop(ddrl, monkeypatch):
    """Hidden 520: see the module docstring.  The host env the fallback steps is of the marker's model and iteration counts and sits at
    the same episode, in both rounds, and the returns equal the device path's."""
    n, L, seed = 2, 30, 5
    actor, _ = _actor(wt.TRACE_CASES[0], L)
    want = actor.evaluate_env(_marker(seed, L), 2 * n, 0)["ret"].tolist()      # the device path over the same four episodes
    dev = _marker(seed, L)

    def unsupported(*a, **kw):
        raise ddrl._lib.DdrlUnsupported("ddrl error -5: ddrl_env_eval_policy_walker: hidden width outside [1, 512]")
    monkeypatch.setattr(actor, "evaluate_env", unsupported)
    from distributed_drl_amd.agent import _device_episodes
    got = []
    for rnd in range(2):     # the second round starts the fallback's host env at episode n
        got += _device_episodes(actor, dev, n, L)
        assert dev.episodes_played == n * (rnd + 1)
    assert got == want and got[:n] != got[n:]


def test_worker_test_round_with_test_on_device(ddrl):
    from distributed_drl_amd import env, workers
    case, L = wt.TRACE_CASES[0], 30
    params = wt.params_of(case)
    ps = ddrl.ParameterServer(list(params.keys()), list(params.values()))
    lines, lasts = {}, {}
    for on_device in (False, True):
        args = _opt(case.hid, L, seed=9)
        args.env_model, args.env_velocity_iterations, args.env_position_iterations = "walker", VIT, PIT
        got = lines[on_device] = []
        if on_device:
            args.test_on_device = True
            kw = {}
        else:      # the host env of the same model and seed
            kw = dict(make_env=lambda name: _host(9, L))
        lasts[on_device] = ddrl.worker_test(ps, args, n=2, max_rounds=2, log=got.append, **kw)
        assert len(got) == 2 and all(s.startswith("AverageTestEpRet ") for s in got) and np.isfinite(lasts[on_device])
    ret = lambda s: s.split()[1]
    assert [ret(s) for s in lines[True]] == [ret(s) for s in lines[False]], lines
    assert lasts[True] == lasts[False], lasts
    # the worker built the marker itself, and without the flag nothing changes
    args.test_on_device = True
    made = workers._default_test_env(args.env, args)
    assert type(made) is env.DeviceBipedalWalker
    assert (made.model, made.velocity_iterations, made.position_iterations, made.seed, made.max_ep_len) == ("walker", VIT, PIT, 9, L)
    args.test_on_device = False
    with pytest.raises(ValueError, match="model=\"walker\""):      # the host door of the bare name, as before
        workers._default_test_env(args.env, args)
    args.env_model = "simple"
    assert type(workers._default_test_env(CONT, args)) is env.LunarLander
    assert getattr(_opt(case.hid, L), "test_on_device", False) is False      # the default stays off
