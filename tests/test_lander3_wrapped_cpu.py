"""CPU: the wrapped step of the ARTICULATED lander as the tests specify it (tests/lander3_wrapped_oracle.py) — the vectorised oracle
against a per-env scalar loop that restates the reference's Wrapper.step and worker loop, its two special branches, the in-place
action — and the preconditions of the GPU matrix of tests/test_gpu_lander3_nstep_rollout.py on the oracle alone: what that file asserts
"has happened" (the ring wrapped, every env ended an episode, a raw done with its dropped reward, a workgroup without a ready env in
front of one with some) does happen under its inputs.  Plus the three new C-ABI names in the ctypes table, the header and the library, and their rows in the memory-contract table."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from lander3_oracle import EPI, EPLEN, EPRET, L0, PSTEP, VY, F, Lander3Oracle   # noqa: E402
from lander3_wrapped_oracle import Lander3WrappedOracle   # noqa: E402
from oracle.env_oracle import RESET_NOISE_STREAM   # noqa: E402
import _abi_contract_lander3_nstep   # noqa: E402,F401  (its import enters the new entry points' rows in _abi_contract.TABLE)

VIT, PIT, LIMIT = 8, 3, 7


def _scalar_wrapped_step(e, action, act_noise, obs_noise, reward_scale, repeat, limit):
    """One iteration of the reference worker's loop on ONE env (a single-env Lander3Oracle whose env_ids names its random streams):
    Wrapper.step (hyperparams.py:122-134) around env.step = Lander3Oracle._physics, then sac_ray.py:212-221 and 252.  np.random.random
    is the env's counter generator: slots 2, 3 of the step's stream for the action, 4.. of the stream after the repeat for the
    observation, a stream of its own for the reset observation (oracle/env_oracle.py).  Returns (o2, r, d, next_o, ended, where)."""
    S = e.S
    u = lambda step, j: e._rng(step, j)[0]
    st0 = S[PSTEP].astype(np.uint32)
    action[0] = action[0] + F(act_noise) * (F(-2.0) * u(st0, 2) + F(1.0))          # :124 `action += ...` (the caller's array)
    action[1] = action[1] + F(act_noise) * (F(-2.0) * u(st0, 3) + F(1.0))

    def noisy(o):
        st1 = S[PSTEP].astype(np.uint32)
        return np.array([o[j] + F(obs_noise) * (F(-2.0) * u(st1, 4 + j) + F(1.0)) for j in range(8)], F)

    r = F(0.0)
    out = None
    for k in range(repeat):                                                        # :126
        reward_, done_, obs_ = e._physics(action.reshape(1, 2))                    # :127
        r = F(r + reward_[0])                                                      # :128
        if done_[0] and repeat != 1:                                               # :130-131
            out = (noisy(obs_[0]), F(0.0), True, "break at %d" % k)
            break
        if repeat == 1:                                                            # :132-133
            out = (obs_[0].copy(), r, bool(done_[0]), "bare")
            break
    if out is None:                                                                # :134
        out = (noisy(obs_[0]), F(F(reward_scale) * r), bool(done_[0]), "ran out")
    o2, rew, d, where = out
    S[EPRET] = (S[EPRET] + rew).astype(F)                                          # sac_ray.py:215
    S[EPLEN] = S[EPLEN] + F(1.0)                                                   # :216
    ended = d or bool(S[EPLEN][0] >= F(limit))                                     # :252
    next_o = o2.copy()
    if ended:
        e.episodes += 1
        e.ret_sum += float(np.float64(S[EPRET][0]))
        e.len_sum += int(S[EPLEN][0])
        S[EPI] = S[EPI] + F(1.0)
        ro = e.reset()[0]                                                          # :199-207 through Wrapper.reset (hyperparams.py:119-121)
        next_o = np.array([ro[j] + F(obs_noise) * (F(-2.0) * u(RESET_NOISE_STREAM, j) + F(1.0)) for j in range(8)], F)
    return o2, rew, d, next_o, ended, where


@pytest.mark.parametrize("repeat", [1, 2, 3])
def test_vectorised_oracle_equals_a_per_env_scalar_loop(repeat):
    """n = 5, 40 steps, limit 7.  Envs 3 and 4 start a long first episode (EPLEN far below zero) falling at 20 m/s with the engines off,
    so that they reach the ground and end INSIDE the repeat: their reward is 0.0 and their state is the state at the break; the others
    end on the limit."""
    n, steps, seed = 5, 40, 5
    vec = Lander3WrappedOracle(n, seed=seed, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
    one = []
    for i in range(n):
        e = Lander3Oracle(1, seed=seed, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
        e.env_ids = np.array([i], np.uint32)
        e.reset()
        one.append(e)
    for i in range(n):
        np.testing.assert_array_equal(one[i].S[:, 0], vec.S[:, i])    # the single envs ARE the vector's envs
    vec.S[EPLEN, 3:] = -200.0
    for f in (VY, L0 + 3, L0 + 9):                                    # hull and both legs moving down at 20 m/s
        vec.S[f, 3:] = -20.0
    for i in range(n):
        one[i].S[:, 0] = vec.S[:, i]
    rs = np.random.RandomState(7)
    seen = set()
    for t in range(steps):
        act = np.tanh(rs.standard_normal((n, 2))).astype(F)
        act[3:] = (-1.0, 0.0)                      # engines off: envs 3 and 4 fall
        a_vec = act.copy()
        o2, r, d, nxt, ended = vec.step_wrapped(a_vec, 0.3, 0.01, 5.0, repeat, LIMIT)
        for i in range(n):
            a_i = act[i].copy()
            w = _scalar_wrapped_step(one[i], a_i, 0.3, 0.01, 5.0, repeat, LIMIT)
            what = "step %d env %d" % (t, i)
            np.testing.assert_array_equal(a_vec[i], a_i, err_msg=what)
            np.testing.assert_array_equal(o2[i], w[0], err_msg=what)
            assert r[i] == w[1] and d[i] == F(w[2]) and bool(ended[i]) == w[4], what
            np.testing.assert_array_equal(nxt[i], w[3], err_msg=what)
            np.testing.assert_array_equal(vec.S[:, i], one[i].S[:, 0], err_msg=what)
            if w[2]:
                seen.add(w[5] if repeat != 1 else "done")
                assert repeat == 1 or r[i] == F(0.0)
            elif w[4]:
                seen.add("limit")
    assert vec.stats() == tuple(sum(x) for x in zip(*[e.stats() for e in one]))
    assert "limit" in seen
    if repeat == 1:
        assert "done" in seen
    else:
        assert any(s.startswith("break at") for s in seen), seen


def test_repeat_one_returns_the_bare_step():
    n = 6
    a = Lander3WrappedOracle(n, seed=2, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
    b = Lander3Oracle(n, seed=2, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
    rs = np.random.RandomState(3)
    for t in range(5):
        act = np.tanh(rs.standard_normal((n, 2))).astype(F)
        o2, r, d, nxt, ended = a.step_wrapped(act.copy(), 0.0, 0.25, 7.0, 1, 1000)   # no observation noise, no scale although both are set
        w = b.step(act)
        np.testing.assert_array_equal(o2, w[0])
        np.testing.assert_array_equal(r, w[1])
        np.testing.assert_array_equal(nxt, w[3])
        assert not ended.any()
        np.testing.assert_array_equal(a.S, b.S)


def test_the_callers_action_array_holds_the_noisy_action():
    n = 4
    e = Lander3WrappedOracle(n, seed=2, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
    act = np.full((n, 2), 0.25, F)
    st0 = e.S[PSTEP].astype(np.uint32)
    want = np.stack([F(0.25) + F(0.3) * (F(-2.0) * e._rng(st0, 2 + c) + F(1.0)) for c in (0, 1)], axis=1)
    e.step_wrapped(act, 0.3, 0.0, 1.0, 3, 1000)
    np.testing.assert_array_equal(act, want)
    assert (act != F(0.25)).all() and (np.abs(act - F(0.25)) <= F(0.3)).all()
    zero = np.full((n, 2), 0.25, F)
    e.step_wrapped(zero, 0.0, 0.0, 1.0, 3, 1000)
    assert (zero == F(0.25)).all()


# ---- the GPU matrix's preconditions ----------------------------------------------------------------------------------------------------
def _stagger(n):
    """tests/test_gpu_nstep_rollout.py::_stagger."""
    i = np.arange(n)
    phase = np.where(i < 64, 3, i % LIMIT)
    return (phase - (7 * (i % 4) + 7)).astype(np.float32)


_RUNS = {}


def _run(n):
    """50 wrapped steps of the GPU matrix's inputs on the oracle alone, once per n: per step the episode ends, raw dones and rewards."""
    if n not in _RUNS:
        e = Lander3WrappedOracle(n, seed=3, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
        e.S[EPLEN] = _stagger(n)
        rs = np.random.RandomState(1)
        ended, done, rew = [], [], []
        for _ in range(50):
            act = np.tanh(rs.standard_normal((n, 2))).astype(F)
            _, r, d, _, en = e.step_wrapped(act, 0.3, 0.01, 5.0, 3, LIMIT)
            ended.append(en.astype(bool)); done.append(d > 0); rew.append(r)
        _RUNS[n] = (np.array(ended), np.array(done), np.array(rew))
    return _RUNS[n]


@pytest.mark.parametrize("Ln,sf", [(4, 1), (4, 3), (8, 2)])
@pytest.mark.parametrize("n", [32, 96, 192])
def test_gpu_matrix_preconditions_hold_on_the_oracle(n, Ln, sf):
    ended, done, rew = _run(n)
    t = np.ones(n, int)
    rows, base_rank_steps = 0, 0
    for s in range(50):
        ready = (t >= Ln) & (t % sf == 0)
        rows += int(ready.sum())
        per_wg = [int(ready[k:k + 64].sum()) for k in range(0, n, 64)]
        base_rank_steps += any(per_wg[w] == 0 and sum(per_wg[w + 1:]) > 0 for w in range(len(per_wg)))
        t = np.where(ended[s], 1, t + 1)
    first_end = ended.argmax(axis=0)
    print("n %d Ln %d save_freq %d: %d ready rows, last first-episode end at step %d, %d raw dones, %d base-rank steps"
          % (n, Ln, sf, rows, first_end.max(), int(done.sum()), base_rank_steps))
    assert rows > 150                                           # a ring of 150 rows wraps
    assert ended.any(axis=0).all() and first_end.max() <= 34    # every env ends an episode by step 34
    assert done.any() and (rew[done] == 0.0).all()              # a raw done, with the dropped reward
    if n in (96, 192) and (Ln, sf) == (4, 3):
        assert base_rank_steps >= 1                             # a workgroup without a ready env in front of one with some


def test_three_new_names_in_the_table_the_header_and_the_library():
    import ctypes
    from distributed_drl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    twins = {"ddrl_env_step_wrapped_articulated": "ddrl_env_step_wrapped", "ddrl_rollout_begin_nstep_articulated": "ddrl_rollout_begin_nstep",
             "ddrl_rollout_step_nstep_articulated": "ddrl_rollout_step_nstep"}
    so = os.path.join(ROOT, "distributed-drl_amd", "libddrl_hip.so")
    lib = ctypes.CDLL(so) if os.path.exists(so) else None
    assert lib is not None, "libddrl_hip.so is not built"
    for name, twin in twins.items():
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin], name      # the arguments of the one-body twin
        args = lambda f: [" ".join(p.split()) for p in re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % f, hdr, flags=re.S).group(1).split(",")]
        assert args(name) == args(twin), name
        assert getattr(lib, name) is not None, name


def test_the_two_new_declarations_have_memory_contract_rows():
    """tests/test_abi_table_cpu.py's header check with tests/_abi_contract_lander3_nstep.py imported: no declaration with caller device
    memory is uncovered, the two new functions' rows name cases of that module, and every refusal it lists has a row."""
    import _abi_contract as ac
    import _abi_contract_lander3_nstep as an
    from test_abi_table_cpu import takes_device_memory, uncovered
    hdr = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    need = takes_device_memory(hdr)
    assert sorted(an.TABLE) == ["ddrl_env_step_wrapped_articulated", "ddrl_rollout_step_nstep_articulated"] and set(an.TABLE) <= set(need)
    assert "ddrl_rollout_begin_nstep_articulated" not in need          # handles only
    assert uncovered(hdr, ac.TABLE, ac.EXEMPT) == []
    without = {f: rows for f, rows in ac.TABLE.items() if f not in an.TABLE}
    assert uncovered(hdr, without, ac.EXEMPT) == sorted(an.TABLE)      # ... and these rows are what covers them
    for f, rows in an.TABLE.items():
        assert rows and ac.TABLE[f] == rows and all(cid in an.CASES and f in an.CASES[cid][1] for cid in rows), f
    assert not set(an.CASES) & set(ac.CASES)
    for f, p in an.REFUSALS:
        assert f in an.TABLE, f
