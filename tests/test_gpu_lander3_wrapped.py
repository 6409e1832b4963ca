"""ddrl_env_step_wrapped_articulated (VecLunarLander.step_wrapped_articulated, kernel k_env3_step_wrapped of csrc/rollout3_nstep.hip)
BIT-EXACT against tests/lander3_wrapped_oracle.py — after every step the observation, reward, raw done, next observation, ended mask,
the in-place action and the whole 66-field state block, at the end the episode statistics — and its refusals: a one-body handle, and
act / obs2 / next_obs off their 8 / 16-byte grid, each leaving state, statistics, outputs and the action as they were."""
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
EPLEN, VY, L0 = 10, 3, 26   # state rows (tests/lander3_oracle.py)


def _pair(n, seed, vit, pit):
    from distributed_drl_amd.env import VecLunarLander
    from lander3_wrapped_oracle import Lander3WrappedOracle
    env = VecLunarLander(n, seed=seed, max_ep_len=1 << 23, model="articulated", velocity_iterations=vit, position_iterations=pit)
    ora = Lander3WrappedOracle(n, seed=seed, max_ep_len=1 << 23, velocity_iterations=vit, position_iterations=pit)
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    return env, ora


def _lockstep(env, ora, steps, repeat, fall=None, seed=1):
    """`steps` wrapped steps of the env beside the oracle under tanh(N(0,1)) actions (`fall`: these envs keep their engines off)."""
    n = env.n
    rs = np.random.RandomState(seed)
    seen_done, seen_limit = 0, 0
    for t in range(steps):
        act = np.tanh(rs.standard_normal((n, 2))).astype(np.float32)
        if fall is not None:
            act[fall] = (-1.0, 0.0)
        a_dev = torch.from_numpy(act).cuda()
        o2, r, d, nxt, ended = env.step_wrapped_articulated(a_dev, 0.3, 0.01, 5.0, repeat, LIMIT)
        w = ora.step_wrapped(act, 0.3, 0.01, 5.0, repeat, LIMIT)        # (act now holds the oracle's noisy action)
        for k, g, want in (("obs2", o2, w[0]), ("rew", r, w[1]), ("done", d, w[2]), ("next_obs", nxt, w[3]), ("ended", ended, w[4]), ("act", a_dev, act)):
            np.testing.assert_array_equal(g.cpu().numpy(), want, err_msg="step %d %s" % (t, k))
        np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S, err_msg="step %d state" % t)
        seen_done += int((w[2] > 0).sum())
        seen_limit += int(((w[4] > 0) & ~(w[2] > 0)).sum())
    assert env.stats() == ora.stats()
    return seen_done, seen_limit


@pytest.mark.parametrize("repeat", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 37, 96])
def test_wrapped_step_equals_the_oracle(n, repeat):
    """40 steps, limit 7, action and observation noise on, reward scale 5, 8 / 3 iterations.  Every third env is on a long first episode
    and falling at 20 m/s with the engines off: it ends on the ground, inside the repeat where there is one; the others end on the limit."""
    env, ora = _pair(n, 5, 8, 3)
    fall = np.arange(n) % 3 == 0
    ora.S[EPLEN, fall] = -200.0
    for f in (VY, L0 + 3, L0 + 9):
        ora.S[f, fall] = -20.0
    env.set_state(torch.from_numpy(ora.S))
    done, limit = _lockstep(env, ora, 40, repeat, fall)
    assert done >= 1 and (limit >= 1 or n == 1)


def test_wrapped_step_at_gyms_iteration_counts():
    """180 / 60 sweeps: n = 32, repeat 3, 12 steps (the loops are run-time counts: the code of the cases above)."""
    env, ora = _pair(32, 9, 180, 60)
    _, limit = _lockstep(env, ora, 12, 3)
    assert limit >= 32


def test_refusals_change_nothing():
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLander
    lib = _lib.load()
    n = 64
    env, ora = _pair(n, 3, 8, 3)
    twin, _ = _pair(n, 3, 8, 3)
    rs = np.random.RandomState(2)
    for _ in range(LIMIT):          # up to the limit: statistics are not zero
        a = torch.from_numpy(np.tanh(rs.standard_normal((n, 2))).astype(np.float32)).cuda()
        env.step_wrapped_articulated(a.clone(), 0.3, 0.01, 5.0, 3, LIMIT)
        twin.step_wrapped_articulated(a.clone(), 0.3, 0.01, 5.0, 3, LIMIT)
    state = env.get_state().clone()
    buf = {k: torch.full((n * 8 + 16,), 3.0, dtype=torch.float32, device="cuda") for k in ("act", "obs2", "rew", "done", "next_obs")}
    ended = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(h, name, act=0, obs2=0, nxt=0):
        f = getattr(lib, name)
        return f(h, P(buf["act"], act), 0.3, 0.01, 5.0, 3, LIMIT, P(buf["obs2"], obs2), P(buf["rew"]), P(buf["done"]), P(buf["next_obs"], nxt),
                 P(ended), None)

    one_body = VecLunarLander(n, seed=3)
    ob_state = one_body.get_state().clone()
    assert call(one_body._h, "ddrl_env_step_wrapped_articulated") == _lib.DDRL_ERR_UNSUPPORTED
    msg = lib.ddrl_last_error()
    assert b"ddrl_env_step_wrapped_articulated" in msg and b"ddrl_env_step_wrapped" in msg.replace(b"ddrl_env_step_wrapped_articulated", b""), msg
    with pytest.raises(_lib.DdrlUnsupported):
        one_body.step_wrapped_articulated(buf["act"][:n * 2].view(n, 2))
    assert torch.equal(one_body.get_state(), ob_state)
    # ... and the one-body entry point keeps refusing this model
    assert call(env._h, "ddrl_env_step_wrapped") == _lib.DDRL_ERR_UNSUPPORTED
    with pytest.raises(_lib.DdrlUnsupported):
        env.step_wrapped(buf["act"][:n * 2].view(n, 2))
    for kw, named in ((dict(act=4), b"act_d"), (dict(obs2=4), b"obs2_d"), (dict(nxt=4), b"next_obs_d"), (dict(obs2=8), b"obs2_d")):
        assert call(env._h, "ddrl_env_step_wrapped_articulated", **kw) == _lib.DDRL_ERR_BAD_ARG, kw
        assert named in lib.ddrl_last_error(), (kw, lib.ddrl_last_error())
    assert call(None, "ddrl_env_step_wrapped_articulated") == _lib.DDRL_ERR_BAD_ARG
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t == 3.0).all()), k
    assert bool((ended == 9).all())
    assert torch.equal(env.get_state(), state) and torch.equal(state, twin.get_state())
    es, ts = env.stats(), twin.stats()
    assert es == ts and es[0] >= n          # every env has been through the limit: the statistics were not empty
