"""ddrl_env_step_wrapped_walker (VecBipedalWalker.step_wrapped_walker, kernel k_walker_step_wrapped of csrc/walker.hip) BIT-EXACT
against tests/walker_wrapped_oracle.py — after every step the observation, reward, raw done, next observation, ended mask, the in-place
action and the whole 286-field state block, at the end the episode statistics — live, at gym's iteration counts, and from the crafted
starts of tests/_walker_wrapped_scenarios.py, with a census on the oracle's side of every branch of the Wrapper; the optional outputs;
its refusals, each leaving state, statistics, outputs and the action as they were; and the stream contract."""
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

LIMIT = 7
NOISE = (0.3, 0.01, 5.0)        # action noise, observation noise, reward scale
NAMES = ("obs2", "rew", "done", "next_obs", "ended")
ENTRY = "ddrl_env_step_wrapped_walker"


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    torch.cuda.set_device(0)
    return d


def _vec(n, seed, vit=8, pit=3):
    from distributed_drl_amd.env import VecBipedalWalker
    return VecBipedalWalker(n, seed=seed, max_ep_len=1 << 23, velocity_iterations=vit, position_iterations=pit)


def _pair(n, seed, vit=8, pit=3):
    from walker_wrapped_oracle import WalkerWrappedOracle
    env = _vec(n, seed, vit, pit)
    ora = WalkerWrappedOracle(n, seed=seed, max_ep_len=1 << 23, velocity_iterations=vit, position_iterations=pit)
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    return env, ora


def _check_step(env, got, a_dev, want, act, t):
    for k, g, w in zip(NAMES + ("act",), list(got) + [a_dev], list(want) + [act]):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg="step %d %s" % (t, k))


def _lockstep(env, ora, steps, repeat, limit=LIMIT, seed=1):
    """`steps` wrapped steps of the env beside the oracle under actions of U(-1.3, 1.3) (beyond the torque clip); the census of the
    oracle's side."""
    import _walker_wrapped_scenarios as wws
    n = env.n
    rs = np.random.RandomState(seed)
    census = {}
    for t in range(steps):
        act = rs.uniform(-1.3, 1.3, (n, 4)).astype(np.float32)
        a_dev = torch.from_numpy(act).cuda()
        got = env.step_wrapped_walker(a_dev, *NOISE, repeat, limit)
        w = ora.step_wrapped(act, *NOISE, repeat, limit)        # (act now holds the oracle's noisy action)
        _check_step(env, got, a_dev, w, act, t)
        np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S, err_msg="step %d state" % t)
        wws.census_of(ora, w, repeat, limit, census)
    assert env.stats() == ora.stats()
    return census


@pytest.mark.parametrize("repeat,steps", [(3, 30), (2, 10), (1, 10)])
def test_wrapped_step_equals_the_live_oracle(ddrl, repeat, steps):
    """n = 70 (a full wave and a 6-lane tail), 8 / 3 iterations, limit 7, action and observation noise on, reward scale 5."""
    env, ora = _pair(70, 5)
    census = _lockstep(env, ora, steps, repeat)
    print("repeat %d: %s" % (repeat, sorted(census.items())))
    assert census["limit_without_d"] >= 70
    assert census["bare_step" if repeat == 1 else "ran_out"] >= 70 * (steps - 1)


def test_wrapped_step_at_gyms_iteration_counts(ddrl):
    """180 / 60 sweeps: n = 16, repeat 3, 4 steps, limit 3 (the loops are run-time counts: the code of the cases above)."""
    env, ora = _pair(16, 9, 180, 60)
    census = _lockstep(env, ora, 4, 3, limit=3)
    assert census["limit_without_d"] >= 16 and census["ran_out"] >= 16 * 3


@pytest.mark.parametrize("repeat", [3, 2, 1])
def test_crafted_starts_reach_every_branch_of_the_wrapper(ddrl, repeat):
    """tests/_walker_wrapped_scenarios.py: the twelve pose classes of tests/_walker_scenarios.py and copies of its x_negative stance that
    leave the terrain at sub-step 0, 1, 2 and 3, set with set_state; two wrapped steps with the noise on, limit 5 from EPLEN 3.
    The census is taken on the ORACLE's run (tests/test_walker_wrapped_cpu.py holds the same floor without a GPU) and asserted here,
    so the comparison below cannot pass by missing a branch: the break at every k < repeat, the loop running out, the bare step of
    repeat == 1, an end by the limit without `d`, an end by `d` below the limit."""
    import _walker_wrapped_scenarios as wws
    S, steps, census, stats = wws.trajectory(repeat, 8, 3)
    need = ["bare_step"] if repeat == 1 else ["break_at_%d" % k for k in range(repeat)] + ["ran_out"]
    for k in need + ["limit_without_d", "d_before_limit"]:
        assert census.get(k, 0) >= 1, (k, census)
    env = _vec(wws.N, wws.SEED)
    env.set_state(torch.from_numpy(S))
    for t, (act_in, outs, act_out, after, _, _) in enumerate(steps):
        a_dev = torch.from_numpy(act_in).cuda()
        got = env.step_wrapped_walker(a_dev, action_repeat=repeat, limit_steps=wws.LIMIT, **wws.NOISE)
        _check_step(env, got, a_dev, outs, act_out, t)
        np.testing.assert_array_equal(env.get_state().cpu().numpy(), after, err_msg="step %d state" % t)
    assert env.stats() == stats


def _raw(lib, h, act, repeat, limit, outs, stream=None):
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return getattr(lib, ENTRY)(h, P(act), *NOISE, repeat, limit, *[P(t) for t in outs], stream)


def _outs(n, which):
    e = lambda *s: torch.full(s, 3.0, device="cuda")
    full = [e(n, 24), e(n), e(n), e(n, 24), torch.full((n,), 9, dtype=torch.uint8, device="cuda")]
    return [t if k in which else None for k, t in zip(NAMES, full)]


@pytest.mark.parametrize("which", [NAMES, (), ("rew",), ("next_obs", "ended")])
def test_every_output_is_optional(ddrl, which):
    """All five outputs, none, one, two: what is given equals the method's (all five), and action, state and statistics do not depend
    on which were given.  n = 70, limit 2: the second step resets every env."""
    from distributed_drl_amd import _lib
    lib, n = _lib.load(), 70
    env, twin = _vec(n, 4), _vec(n, 4)
    rs = np.random.RandomState(8)
    for t in range(2):
        act = torch.from_numpy(rs.uniform(-1, 1, (n, 4)).astype(np.float32)).cuda()
        a_twin, given = act.clone(), act.clone()
        want = twin.step_wrapped_walker(a_twin, *NOISE, 3, 2)
        outs = _outs(n, which)
        assert _raw(lib, env._h, act, 3, 2, outs) == 0, lib.ddrl_last_error()
        assert torch.equal(act, a_twin) and bool((act != given).all()) and float((act - given).abs().max()) <= 0.3 + 1e-6
        for k, g, w in zip(NAMES, outs, want):
            assert g is None or torch.equal(g, w), (t, k)
        assert torch.equal(env.get_state(), twin.get_state()), t
    es, ts = env.stats(), twin.stats()
    assert es == ts and es[0] == n


def test_refusals_change_nothing(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLander
    import _abi_contract_walker_nstep as aw
    lib = _lib.load()
    n = 64
    env, twin = _vec(n, 3), _vec(n, 3)
    rs = np.random.RandomState(2)
    for _ in range(2):          # up to the limit: statistics are not zero
        a = torch.from_numpy(rs.uniform(-1, 1, (n, 4)).astype(np.float32)).cuda()
        env.step_wrapped_walker(a.clone(), *NOISE, 3, 2)
        twin.step_wrapped_walker(a.clone(), *NOISE, 3, 2)
    state = env.get_state().clone()
    buf = {k: torch.full((n * 24 + 16,), 3.0, dtype=torch.float32, device="cuda") for k in ("act", "obs2", "rew", "done", "next_obs")}
    ended = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(h, name=ENTRY, act=0, obs2=0, nxt=0, repeat=3, limit=LIMIT, act_null=False):
        return getattr(lib, name)(h, None if act_null else P(buf["act"], act), *NOISE, repeat, limit, P(buf["obs2"], obs2), P(buf["rew"]),
                                  P(buf["done"]), P(buf["next_obs"], nxt), P(ended), None)

    others = (VecLunarLander(n, seed=3), VecLunarLander(n, seed=3, model="articulated", velocity_iterations=4, position_iterations=2))
    for other, twin_name in zip(others, (b"ddrl_env_step_wrapped", b"ddrl_env_step_wrapped_articulated")):
        before = other.get_state().clone()
        assert call(other._h) == _lib.DDRL_ERR_UNSUPPORTED
        msg = lib.ddrl_last_error()
        assert msg.startswith(ENTRY.encode() + b":") and msg.rstrip().endswith(b"use " + twin_name), msg
        assert torch.equal(other.get_state(), before)
        # ... and the landers' entry points keep refusing the walker
        assert call(env._h, twin_name.decode()) == _lib.DDRL_ERR_UNSUPPORTED and b"walker" in lib.ddrl_last_error()
    for meth in (env.step_wrapped, env.step_wrapped_articulated):
        with pytest.raises(_lib.DdrlUnsupported):
            meth(buf["act"][:n * 2].view(n, 2))
    refused = []
    for kw, named in ((dict(act=4), b"act_d"), (dict(act=8), b"act_d"), (dict(obs2=4), b"obs2_d"), (dict(nxt=4), b"next_obs_d"),
                      (dict(obs2=8), b"obs2_d"), (dict(repeat=0), ENTRY.encode()), (dict(limit=0), ENTRY.encode()),
                      (dict(act_null=True), ENTRY.encode())):
        assert call(env._h, **kw) == _lib.DDRL_ERR_BAD_ARG, kw
        assert named in lib.ddrl_last_error(), (kw, lib.ddrl_last_error())
        refused.append((ENTRY, named.decode()))
    assert set(aw.REFUSALS) <= set(refused)      # every refusal the contract module lists has been made
    assert call(None) == _lib.DDRL_ERR_BAD_ARG and ENTRY.encode() in lib.ddrl_last_error()
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t == 3.0).all()), k
    assert bool((ended == 9).all())
    assert torch.equal(env.get_state(), state) and torch.equal(state, twin.get_state())
    es, ts = env.stats(), twin.stats()
    assert es == ts and es[0] >= n          # every env has been through the limit: the statistics were not empty


def test_a_misaligned_action_view_is_still_updated_in_place(ddrl):
    """VecBipedalWalker.step_wrapped_walker stages a view off the 16-byte grid in an aligned copy and copies the noisy action back."""
    n = 8
    env, twin = _vec(n, 6), _vec(n, 6)
    base = torch.zeros(n * 4 + 1, device="cuda")
    view = base[1:].view(n, 4)
    assert view.data_ptr() % 16 == 4
    view.uniform_(-1, 1)
    a = view.clone()
    got = [x.clone() for x in env.step_wrapped_walker(view, *NOISE, 3, LIMIT)]
    want = twin.step_wrapped_walker(a, *NOISE, 3, LIMIT)
    assert torch.equal(view, a) and float(base[0]) == 0.0
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_wrapped_step_runs_on_the_callers_stream(ddrl):
    """The stream contract, as tests/test_gpu_walker.py holds ddrl_env_step to it: on a side stream, behind a bounded gate, the true
    actions are written over decoys and the step is issued.  A launch that went anywhere but the caller's stream would run during the
    gate, read the decoys and differ from the twin stepped with the true actions."""
    from _abi_arena import cycles_per_ms, side_stream
    n = 64
    env, twin = _vec(n, 21), _vec(n, 21)
    true = twin.sample_actions().clone()
    a_twin = true.clone()
    want = [x.clone() for x in twin.step_wrapped_walker(a_twin, *NOISE, 3, 1)]      # limit 1: every env resets
    want_state = twin.get_state().clone()
    dev = env.device
    act = torch.zeros(n, 4, device="cuda")        # the decoy: zero torque on every motor
    side = side_stream(dev)
    gate_end = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(cycles_per_ms(dev) * 20.0))   # the gate: bounded, 20 ms
        gate_end.record()
        act.copy_(true)                                      # the late write
        got = env.step_wrapped_walker(act, *NOISE, 3, 1)
        issued_inside = not gate_end.query()
    side.synchronize()                                       # the caller's stream only, not the device
    got = [x.clone() for x in got]
    assert issued_inside, "the gate was over before the step was issued: the run proves nothing"
    for name, x, y in zip(NAMES, got, want):
        assert torch.equal(x, y), name
    assert torch.equal(act, a_twin) and not torch.equal(act, true)
    assert torch.equal(env.get_state(), want_state)
    assert env.stats() == twin.stats()
