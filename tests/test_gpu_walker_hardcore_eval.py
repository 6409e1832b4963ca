"""The Hardcore walker's evaluation episodes on the device, fed from handles (ddrl_env_eval_policy_walker_hardcore,
csrc/walker_hardcore_eval.hip; ddrl_env_eval_results; Actor.evaluate_env on an env.DeviceBipedalWalkerHardcore), held to
  * the trace checks: the env half bit for bit against tests/walker_hardcore_oracle.WalkerHardcoreOracle
    (tests/_walker_hardcore_eval_trace.py; tests/test_walker_hardcore_eval_cpu.py shows what it sees and what the inputs reach), the
    policy half by _acting_parity.actor_reference / compare with its bars;
  * the stream contract of first_episode;
  * the host loop it replaces, bit for bit: Actor.test on the host env.BipedalWalker(terrain="hardcore") and on the device marker;
and: no side effects on the lending handle or the actor, a fitting second call that allocates nothing, every refusal (status, text,
nothing launched; the grass walker and the two lander kinds among them), the stream case of
tests/_abi_contract_walker_hardcore_eval.py on a side stream, the DdrlUnsupported fallback and a worker_test round with
opt.test_on_device_hardcore.

The fallback: an Actor with a hidden width of 520 cannot be built (ddrl_actor_create refuses hidden sizes > 512), so — as in
tests/test_gpu_walker_eval.py — it is driven by an evaluate_env that raises what _lib.check raises for DDRL_ERR_UNSUPPORTED."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _walker_hardcore_eval_trace as ht  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = b"ddrl_env_eval_policy_walker_hardcore"
GRASS_NAME = b"ddrl_env_eval_policy_walker"
HARDCORE, CONT = "BipedalWalkerHardcore-v2", "LunarLanderContinuous-v2"
VIT, PIT = 8, 3


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _marker(seed, max_ep_len, vit=VIT, pit=PIT):
    from distributed_drl_amd import env
    return env.DeviceBipedalWalkerHardcore(seed, max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _host(seed, max_ep_len, vit=VIT, pit=PIT):
    from distributed_drl_amd import env
    return env.make(HARDCORE, model="walker", terrain="hardcore", seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit,
                    position_iterations=pit)


def _vec(n, seed, max_ep_len, terrain="hardcore"):
    from distributed_drl_amd import env
    return env.VecBipedalWalker(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=VIT, position_iterations=PIT, terrain=terrain)


def _opt(hid, max_ep_len, seed=0, obs_dim=24, act_dim=4):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=obs_dim, act_dim=act_dim)
    opt.hidden_sizes, opt.max_ep_len, opt.seed, opt.env = tuple(hid), max_ep_len, seed, HARDCORE
    return opt


def _actor(case, max_ep_len=None):
    from distributed_drl_amd.agent import Actor
    actor = Actor(_opt(case.hid, case.max_ep_len if max_ep_len is None else max_ep_len), max_rows=1)
    params = ht.params_of(case)
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _same_out(a, b):
    return _same_bits(a["trace"], b["trace"]) and (a["ret"] == b["ret"]).all() and (a["len"] == b["len"]).all()


def _both_checks(out, case, params):
    assert out["ret"].dtype == np.float64 and out["len"].dtype == np.int32 and out["trace"].dtype == np.float32
    assert out["trace"].shape == (case.n, case.max_ep_len, 32)
    ht.check_env_walker_hardcore(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)
    table = []
    try:
        ht.check_policy(out, case, params, table=table)
    finally:
        print("\n".join(ap.format_table(table)))


# ---- 1. trace cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ht.TRACE_CASES if c not in ht.FIRST_CASES], ids=repr)      # (the two first-episode cases: below)
def test_policy_trace_passes_both_checks(ddrl, case):
    actor, params = _actor(case)
    dev = _marker(case.seed, case.max_ep_len, case.vit, case.pit)
    out = actor.evaluate_env(dev, case.n, case.first, trace=True)
    assert dev.episodes_played == 0
    _both_checks(out, case, params)
    last = np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    # what tests/test_walker_hardcore_eval_cpu.py asserts on the oracle's traces holds for the device's
    if case is ht.TERMINAL_CASE:
        assert out["len"].tolist() == [54, 54, 54] and (last[:, ht.I_REW] == -100).all() and len(set(out["ret"].tolist())) == 3
    if case is ht.WIDE_CASE:
        assert out["len"].tolist() == [79, 79] and (last[:, ht.I_REW] == -100).all()
    if case in (ht.LIMIT_CASE, ht.ONE_STEP_CASE, ht.GYM_CASE):
        assert (out["len"] == case.max_ep_len).all() and (last[:, ht.I_REW] != -100).all() and (last[:, ht.I_END] == 1).all()


# ---- 2. first_episode ---------------------------------------------------------------------------------------------------------------
def test_first_episode_positions_the_stream(ddrl):
    long, short = ht.FIRST_CASES
    actor, params = _actor(long)
    dev = _marker(long.seed, long.max_ep_len)
    a = actor.evaluate_env(dev, long.n, 0, trace=True)
    b = actor.evaluate_env(dev, short.n, short.first, trace=True)
    assert _same_out({k: v[5:8] for k, v in a.items()}, b)
    assert not _same_bits(a["trace"][0:3], b["trace"])
    _both_checks(a, long, params)
    _both_checks(b, short, params)
    assert (a["len"] == long.max_ep_len).all()
    # the default is the marker's episode count
    dev.episodes_played = 5
    assert _same_out(actor.evaluate_env(dev, 3, trace=True), b)


# ---- 3. equal to the host loop it replaces --------------------------------------------------------------------------------------------
def test_actor_test_equals_the_host_loop(ddrl):
    from distributed_drl_amd import env
    n, L, seed = 4, 40, 7
    actor, _ = _actor(ht.TERMINAL_CASE, L)
    host = _host(seed, L)
    assert type(host) is env.BipedalWalker and host._vec.terrain == "hardcore"
    dev = _marker(seed, L)
    assert type(dev) is env.DeviceBipedalWalkerHardcore and (dev.model, dev.terrain, dev.on_device) == ("walker", "hardcore", True)
    seen = []
    for rnd in range(2):      # the second round continues where the first ended, on both sides
        rets = []
        for _ in range(n):     # Actor.test's episodes written out on the host env
            o, d, ep_ret, ep_len = host.reset(), False, 0, 0
            while not (d or (ep_len == L)):
                o, r, d, _ = host.step(actor.get_action(o, True))
                ep_ret += r
                ep_len += 1
            rets.append(ep_ret)
        out = actor.evaluate_env(dev, n)
        assert "trace" not in out and out["ret"].tolist() == rets, (rnd, out, rets)
        got = actor.test(dev, None, n)
        assert isinstance(got, float) and got == sum(rets) / n, (rnd, got, rets)
        assert dev.episodes_played == n * (rnd + 1)
        seen.append(rets)
    assert seen[0] != seen[1]      # the second round played other episodes
    # Actor.test on a host env of the same seed returns the first round's mean
    assert actor.test(_host(seed, L), None, n) == sum(seen[0]) / n


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------------------
def _results(lib, h):
    p = [ctypes.c_void_p() for _ in range(3)]
    k = [ctypes.c_int32(-1) for _ in range(3)]
    rc = lib.ddrl_env_eval_results(h, *[ctypes.byref(x) for x in p + k])
    return rc, [x.value for x in p], [x.value for x in k]


def test_evaluation_has_no_side_effects(ddrl):
    from distributed_drl_amd import _lib, env
    case = ht.TERMINAL_CASE
    actor, _ = _actor(case)
    lib = _lib.load()
    vecs = [_vec(4, 11, 9) for _ in range(2)]
    assert vecs[0].state_fields == 663
    acts = [torch.tensor(np.random.RandomState(k).uniform(-1, 1, (4, 4)).astype(np.float32), device="cuda") for k in range(12)]
    for v in vecs:
        for a in acts[:10]:      # past one time limit: the statistics are off zero
            v.step(a)
    probe = torch.rand(1, 24, device="cuda")
    before, pol0 = actor.get_weights_flat().clone(), actor.get_actions(probe, deterministic=True).clone()
    ctr = actor._noise_ctr
    obs_before = vecs[0].obs.clone()
    _lib.check(lib.ddrl_env_eval_policy_walker_hardcore(vecs[0]._h, actor._h, 3, 4, 1, _lib.stream_ptr()))
    plain = env.eval_results(vecs[0], 32)
    assert plain["trace"].shape == (3, 9, 32)
    assert actor._noise_ctr == ctr and torch.equal(actor.get_weights_flat(), before)
    assert torch.equal(actor.get_actions(probe, deterministic=True), pol0)
    assert torch.equal(vecs[0].get_state().view(torch.int32), vecs[1].get_state().view(torch.int32))
    assert torch.equal(vecs[0].obs.view(torch.int32), obs_before.view(torch.int32))
    # a second call that fits allocates nothing: the results block and its parts stay where they are, for fewer episodes too
    rc, where, sizes = _results(lib, vecs[0]._h)
    assert rc == _lib.DDRL_OK and sizes == [3, 9, 32]
    _lib.check(lib.ddrl_env_eval_policy_walker_hardcore(vecs[0]._h, actor._h, 3, 4, 1, _lib.stream_ptr()))
    assert _results(lib, vecs[0]._h) == (rc, where, sizes) and _same_out(env.eval_results(vecs[0], 32), plain)
    _lib.check(lib.ddrl_env_eval_policy_walker_hardcore(vecs[0]._h, actor._h, 2, 4, 0, _lib.stream_ptr()))
    assert _results(lib, vecs[0]._h)[1][0] == where[0]
    assert torch.equal(vecs[0].get_state().view(torch.int32), vecs[1].get_state().view(torch.int32))
    # the lent handle steps on bit for bit against the twin that was never lent
    outs = [[t.clone() for t in v.step(acts[10])] for v in vecs]
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(vecs[0].get_state().view(torch.int32), vecs[1].get_state().view(torch.int32))
    assert vecs[0].stats() == vecs[1].stats() and vecs[0].stats()[0] == 0
    # the same episodes from a one-env marker of that seed: n_envs of the lending handle does not matter
    assert _same_out(actor.evaluate_env(_marker(11, 9), 3, 4, trace=True), plain)


# ---- 5. every refusal -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ddrl):
    from distributed_drl_amd import _lib, env
    from distributed_drl_amd.agent import Actor
    case, L = ht.TERMINAL_CASE, 10
    actor, _ = _actor(case, L)
    lib, s = _lib.load(), _lib.stream_ptr
    vec = _vec(1, 3, L)
    _lib.check(lib.ddrl_env_eval_policy_walker_hardcore(vec._h, actor._h, 2, 0, 1, s()))
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
    grass = _vec(1, 3, L, terrain="grass")
    landers = {"one-body": env.VecLunarLander(1, seed=3, max_ep_len=L),
               "articulated": env.VecLunarLander(1, seed=3, max_ep_len=L, model="articulated", velocity_iterations=VIT, position_iterations=PIT)}
    others = dict(landers, grass=grass)
    other_states = {k: v.get_state().clone() for k, v in others.items()}

    pol = lambda h, a, n=2, first=0: lib.ddrl_env_eval_policy_walker_hardcore(h, a, n, first, 1, s())
    B, U = _lib.DDRL_ERR_BAD_ARG, _lib.DDRL_ERR_UNSUPPORTED
    refusals = [
        ("NULL env handle", lambda: pol(None, actor._h), B, b"NULL handle"),
        ("NULL actor", lambda: pol(vec._h, None), B, b"NULL handle"),
        ("n_episodes 0", lambda: pol(vec._h, actor._h, n=0), B, b"n_episodes"),
        ("n_episodes -1", lambda: pol(vec._h, actor._h, n=-1), B, b"n_episodes"),
        ("episode index past 2^24", lambda: pol(vec._h, actor._h, n=2, first=(1 << 24) - 1), B, b"2^24"),
        ("actor 24 -> 3", lambda: pol(vec._h, three._h), B, b"24 observations and 4 actions"),
        ("actor 8 -> 2", lambda: pol(vec._h, lander_actor._h), B, b"24 observations and 4 actions"),
        ("a grass walker", lambda: pol(grass._h, actor._h), U, GRASS_NAME + b" ("),
        ("a one-body handle", lambda: pol(landers["one-body"]._h, lander_actor._h), U, b"the one-body model"),
        ("an articulated handle", lambda: pol(landers["articulated"]._h, lander_actor._h), U, b"the articulated lander"),
    ]
    if torch.cuda.device_count() > 1:      # handles on different devices (needs a second device to build one on)
        with torch.cuda.device(1):
            far = _vec(1, 3, L)
        refusals.append(("other device", lambda: pol(far._h, actor._h), B, b"device"))
    for what, call, status, word in refusals:
        rc = call()
        text = lib.ddrl_last_error()
        assert rc == status, (what, rc, text)
        assert word in text and text.startswith(NAME + b":"), (what, text)
        if "handle" in what and status == U:      # both landers share their entry point: no suffix of the model behind it
            assert text.endswith(b"use ddrl_env_eval_policy") and b"built for the walker (DDRL_ENV_WALKER)" in text, text
        if what == "a grass walker":
            assert b"grass terrain" in text and b"hardcore" in text, text
    # (a hidden width outside [1, 512] cannot be built: ddrl_actor_create refuses it; the envelope test is the grass twin's text,
    # csrc/walker_eval_device.h, and its Python side is the fallback test below)
    with pytest.raises(_lib.DdrlUnsupported):
        _lib.check(pol(grass._h, actor._h))
    with pytest.raises(_lib.DdrlUnsupported):
        _lib.check(pol(landers["articulated"]._h, lander_actor._h))
    with pytest.raises(ValueError, match="ddrl"):
        _lib.check(pol(vec._h, actor._h, n=0))
    torch.cuda.synchronize()
    assert bool((block == 0xA5).all()), "a refused call wrote into the results block"
    assert _results(lib, vec._h) == (_lib.DDRL_OK, [ret, ln, tr], sizes)      # ... and the previous results are still the handle's
    for k, v in others.items():      # the other handles: no results block, their state as it was
        assert _results(lib, v._h)[0] == B and torch.equal(v.get_state().view(torch.int32), other_states[k].view(torch.int32)), k
    # the grass twin keeps refusing the Hardcore handle, the landers' entry point any walker handle; neither has results of theirs
    assert lib.ddrl_env_eval_policy_walker(vec._h, actor._h, 2, 0, 1, s()) == U
    text = lib.ddrl_last_error()
    assert text.startswith(GRASS_NAME + b":") and b"hardcore" in text and NAME in text and b"missing" not in text, text
    assert lib.ddrl_env_eval_policy(vec._h, actor._h, 2, 0, 1, s()) == U and b"walker" in lib.ddrl_last_error()
    torch.cuda.synchronize()
    assert bool((block == 0xA5).all())
    assert _results(lib, vec._h) == (_lib.DDRL_OK, [ret, ln, tr], sizes)
    # the grass twin takes the grass handle this function refused
    assert lib.ddrl_env_eval_policy_walker(grass._h, actor._h, 2, 0, 1, s()) == _lib.DDRL_OK
    # the same call with nothing wrong goes through (it fits the block: the sentinel view still points into it)
    assert pol(vec._h, actor._h) == _lib.DDRL_OK
    torch.cuda.synchronize()
    assert not bool((block[:16] == 0xA5).all())
    del block


# ---- 6. the stream contract -------------------------------------------------------------------------------------------------------------
# The gate (tests/_abi_arena.run_stream_case, as tests/test_gpu_abi_walker_eval.py): the closure — set_weights, 3 episodes of up to 6
# steps at 4 / 2 iterations as one launch, the three copies out of the results block — is the grass twin's with the Hardcore step in
# it, whose slowest closure was timed at 3.578 ms; a Hardcore env step costs 880 / 723 of a grass one (profiles/walker_hardcore_step_time.txt),
# so 10 x 3.578 x 880 / 723 = 43.55 ms holds the work queued ahead on the side stream for longer than ten of the calls under test.
# Every run measures its own gate with events; one that came out shorter fails as VOID, and a void run never passes.
GATE_MS = max(10.0, 10.0 * 3.578 * 880.0 / 723.0)


def test_stream_contract(ddrl):
    import _abi_arena as aa
    import _abi_contract_walker_hardcore_eval as ahe
    from distributed_drl_amd import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    assert sorted(ahe.STREAM_CASES) == ["env_eval_policy_walker_hardcore"]
    for cid in sorted(ahe.STREAM_CASES):
        try:
            for _ in range(3):      # tests/test_gpu_abi_stream.py's policy: a run that is void and nothing else is made again, twice at the most
                checks = aa.run_stream_case(cid, ahe.STREAM_CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
                if checks.props() != ["VOID"]:
                    break
                print("void run of %s: %s" % (cid, checks.failed))
        except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
            pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
        if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
            pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
        checks.report()


# ---- 7. fallback, workers ---------------------------------------------------------------------------------------------------------------
def test_outside_the_envelope_falls_back_to_the_host_loop(ddrl, monkeypatch):
    """Hidden 520: see the module docstring.  The host env the fallback steps is of the marker's model, terrain and iteration counts
    and sits at the same episode, in both rounds, and the returns equal the device path's."""
    from distributed_drl_amd import env
    n, L, seed = 2, 30, 5
    actor, _ = _actor(ht.TERMINAL_CASE, L)
    want = actor.evaluate_env(_marker(seed, L), 2 * n, 0)["ret"].tolist()      # the device path over the same four episodes
    dev = _marker(seed, L)
    dev.episodes_played = 3
    host = dev.host_env()
    assert type(host) is env.BipedalWalker and host._vec.terrain == "hardcore" and host._vec.state_fields == 663
    assert float(host._vec.get_state()[13, 0]) == 3.0 and (host._vec.seed, host._vec.max_ep_len) == (seed, L)
    assert type(dev.handle()) is env.VecBipedalWalker and dev.handle().n == 1 and dev.handle().terrain == "hardcore" and dev.handle() is dev.handle()
    dev.episodes_played = 0

    def unsupported(*a, **kw):
        raise ddrl._lib.DdrlUnsupported("ddrl error -5: ddrl_env_eval_policy_walker_hardcore: hidden width outside [1, 512]")
    monkeypatch.setattr(actor, "evaluate_env", unsupported)
    from distributed_drl_amd.agent import _device_episodes
    got = []
    for rnd in range(2):     # the second round starts the fallback's host env at episode n
        got += _device_episodes(actor, dev, n, L)
        assert dev.episodes_played == n * (rnd + 1)
    assert got == want and got[:n] != got[n:]


def test_worker_test_round_with_test_on_device_hardcore(ddrl):
    from distributed_drl_amd import env, workers
    case, L = ht.TERMINAL_CASE, 30
    params = ht.params_of(case)
    ps = ddrl.ParameterServer(list(params.keys()), list(params.values()))
    lines, lasts = {}, {}
    for on_device in (False, True):
        args = _opt(case.hid, L, seed=9)
        args.env_model, args.env_velocity_iterations, args.env_position_iterations, args.env_terrain = "walker", VIT, PIT, "hardcore"
        got = lines[on_device] = []
        if on_device:
            args.test_on_device_hardcore = True
            kw = {}
        else:      # the host env of the same model, terrain and seed
            kw = dict(make_env=lambda name: _host(9, L))
        lasts[on_device] = ddrl.worker_test(ps, args, n=2, max_rounds=2, log=got.append, **kw)
        assert len(got) == 2 and all(s.startswith("AverageTestEpRet ") for s in got) and np.isfinite(lasts[on_device])
    ret = lambda s: s.split()[1]
    assert [ret(s) for s in lines[True]] == [ret(s) for s in lines[False]], lines
    assert lasts[True] == lasts[False], lasts
    # a caller may pass the marker itself
    got = []
    args.test_on_device_hardcore = False
    assert ddrl.worker_test(ps, args, n=2, max_rounds=2, log=got.append, make_env=lambda name: _marker(9, L)) == lasts[True]
    assert [ret(s) for s in got] == [ret(s) for s in lines[True]]
    # the worker built the marker itself; the old flag keeps raising on this terrain
    args.test_on_device_hardcore = True
    made = workers._default_test_env(args.env, args)
    assert type(made) is env.DeviceBipedalWalkerHardcore
    assert (made.model, made.terrain, made.velocity_iterations, made.position_iterations, made.seed, made.max_ep_len) == ("walker", "hardcore", VIT, PIT, 9, L)
    args.test_on_device_hardcore, args.test_on_device = False, True
    with pytest.raises(ValueError, match="test_on_device_hardcore"):
        workers._default_test_env(args.env, args)
