"""CPU: the wrapped step of the BIPEDAL WALKER as the tests specify it (tests/walker_wrapped_oracle.py) — the vectorised oracle against
a per-env scalar loop that restates the reference's Wrapper.step and worker loop; its bare step at repeat == 1 against
WalkerOracle.step; the reward's three forms; the state at a break; the in-place action; the hash inputs of every draw of an episode
pairwise distinct — and the preconditions of tests/test_gpu_walker_wrapped.py's crafted run on the oracle alone: every branch its census
asks for IS reached under its inputs.  Plus the new C-ABI name in its header (include/ddrl_walker.h), the ctypes table and the library, and that
header held to the memory-contract and stream rows of tests/_abi_contract_walker_nstep.py."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _walker_wrapped_scenarios as wws   # noqa: E402
from walker_oracle import ACT, EPI, EPLEN, EPRET, OBS, PSTEP, PX, F, WalkerOracle   # noqa: E402
from walker_wrapped_oracle import ACT_J0, OBS_NOISE_STEP0, RESET_NOISE_STREAM, WalkerWrappedOracle   # noqa: E402

VIT, PIT, LIMIT = 8, 3, 7
BIG = 1 << 23


def _scalar_wrapped_step(e, action, act_noise, obs_noise, reward_scale, repeat, limit):
    """One iteration of the reference worker's loop on ONE env (a single-env WalkerOracle whose env_ids names its random streams):
    Wrapper.step (hyperparams.py:122-134) around env.step = WalkerOracle._physics, then sac_ray.py:212-221 and 252.  np.random.random
    is the env's counter generator: slots 2..5 of the step's stream for the action, 24 slots of the observation range's stream after
    the repeat for the observation, a stream of its own for the reset observation.  Returns (o2, r, d, next_o, ended, where)."""
    S = e.S
    u = lambda step, j: e._rng(step, j)[0]
    st0 = S[PSTEP].astype(np.uint32)
    for c in range(ACT):
        action[c] = action[c] + F(act_noise) * (F(-2.0) * u(st0, ACT_J0 + c) + F(1.0))   # :124 `action += ...` (the caller's array)

    def noisy(o):
        st1 = np.uint32(OBS_NOISE_STEP0) + np.uint32(2) * S[PSTEP].astype(np.uint32)
        return np.array([o[j] + F(obs_noise) * (F(-2.0) * u(st1, j) + F(1.0)) for j in range(OBS)], F)

    r = F(0.0)
    out = None
    for k in range(repeat):                                                        # :126
        reward_, done_, obs_ = e._physics(action.reshape(1, ACT))                  # :127
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
        next_o = np.array([ro[j] + F(obs_noise) * (F(-2.0) * u(RESET_NOISE_STREAM, j) + F(1.0)) for j in range(OBS)], F)
    return o2, rew, d, next_o, ended, where


class _Recording(WalkerOracle):
    """A single-env WalkerOracle that notes (episode, hash input) of every draw.  With n = 1 no draw is masked away: each one is used."""
    def __init__(self, *a, **kw):
        self.draws = []
        super().__init__(*a, **kw)

    def _rng(self, step, j):
        b = (int(np.asarray(step, dtype=np.uint32).reshape(-1)[0]) * 16 + int(j)) & 0xFFFFFFFF
        self.draws.append((int(self.S[EPI][0]), b))
        return super()._rng(step, j)


def _crafted_pair(n, seed):
    """A vector oracle and its n single-env twins on the same states; envs 2.. start in the crafted x_negative stances (x = 0.04, 0.10,
    0.18, ... : `d` arrives inside the repeat), envs 0 and 1 stay on their reset state."""
    vec = WalkerWrappedOracle(n, seed=seed, max_ep_len=BIG, velocity_iterations=VIT, position_iterations=PIT)
    one = []
    for i in range(n):
        e = _Recording(1, seed=seed, max_ep_len=BIG, velocity_iterations=VIT, position_iterations=PIT)
        e.env_ids = np.array([i], np.uint32)
        e.draws = []
        e.reset()
        one.append(e)
    for i in range(n):
        np.testing.assert_array_equal(one[i].S[:, 0], vec.S[:, i])    # the single envs ARE the vector's envs
    S, _ = wws.build()
    first = wws.ws.N                                                   # the first x_negative copy; one copy per start x
    for i in range(2, n):
        vec.S[:, i] = S[:, first + (i - 2) * wws.COPIES]
        vec.S[EPLEN, i] = -200.0                                       # a long first episode: it ends on `d`, not on the limit
        one[i].S[:, 0] = vec.S[:, i]
    return vec, one


@pytest.mark.parametrize("repeat", [1, 2, 3])
def test_vectorised_oracle_equals_a_per_env_scalar_loop_and_no_two_draws_of_an_episode_share_an_input(repeat):
    """n = 6, 24 steps, limit 7, noise on.  Envs 2..5 break inside the repeat of the first steps (where there is one); all envs then
    end on the limit, again and again.  Every draw of the single-env twins — action, observation and reset noise, terrain, initial
    force — is noted with its episode: within an episode no two share a hash input (the module docstring of
    tests/walker_wrapped_oracle.py says why; this is the live check)."""
    n, steps, seed = 6, 24, 5
    vec, one = _crafted_pair(n, seed)
    rs = np.random.RandomState(7)
    seen = set()
    for t in range(steps):
        act = np.tanh(rs.standard_normal((n, ACT))).astype(F)
        act[2:] = 0.0
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
        assert {"break at %d" % k for k in range(repeat)} <= seen, seen
    for i, e in enumerate(one):
        assert len(e.draws) > 200 * 3 and len({ep for ep, _ in e.draws}) >= 3, i      # terrains of several episodes and the noise
        assert len(set(e.draws)) == len(e.draws), "env %d: two draws of one episode share a hash input" % i
        if repeat != 1:
            assert any(b >= 0xFFFFFEF0 and b < 0xFFFFFF08 for _, b in e.draws)          # the reset noise is among them


def test_reset_noise_inputs_meet_the_terrains_only_where_the_terrain_does_not_draw():
    reset_noise = {(RESET_NOISE_STREAM * 16 + k) & 0xFFFFFFFF for k in range(OBS)}
    e = _Recording(1, seed=1, velocity_iterations=1, position_iterations=1)
    terrain = {b for _, b in e.draws}                                   # what _build draws: i > 20 and the initial force
    assert len(terrain) == 179 + 1 and not terrain & reset_noise
    every_index = {(0xFFFFFFF0 * 16 + i) & 0xFFFFFFFF for i in range(201)}
    assert sorted(i for i in range(201) if ((0xFFFFFFF0 * 16 + i) & 0xFFFFFFFF) in reset_noise) == list(range(8)) and terrain <= every_index


def test_repeat_one_without_noise_is_walker_oracle_step_but_for_the_raw_done():
    """act_noise = obs_noise = 0, repeat = 1, limit_steps = max_ep_len: everything WalkerOracle.step returns and leaves, bit for bit —
    except `done`, which is the raw d here and 0 at the limit there.  Env 5 leaves the terrain (x < 0) in the very step in which
    its episode reaches the limit: the one place where the two differ."""
    n, M = 6, 4
    a = WalkerWrappedOracle(n, seed=2, max_ep_len=M, velocity_iterations=VIT, position_iterations=PIT)
    b = WalkerOracle(n, seed=2, max_ep_len=M, velocity_iterations=VIT, position_iterations=PIT)
    S, _ = wws.build()
    a.S[:, 5] = S[:, wws.ws.N]                    # x = 0.04, EPLEN 3: d and the limit at step 0
    b.S[:] = a.S
    rs = np.random.RandomState(3)
    differed = 0
    for t in range(2 * M + 1):
        act = np.tanh(rs.standard_normal((n, ACT))).astype(F)
        act[5] = 0.0
        mine = act.copy()
        o2, r, d, nxt, ended = a.step_wrapped(mine, 0.0, 0.0, 7.0, 1, M)     # no scale although it is set
        w = b.step(act)
        np.testing.assert_array_equal(mine, act)
        np.testing.assert_array_equal(o2, w[0])
        np.testing.assert_array_equal(r, w[1])
        np.testing.assert_array_equal(nxt, w[3])
        np.testing.assert_array_equal(ended, w[4])
        raw = (b.last["game_over"] | b.last["neg_x"] | b.last["finish"]).astype(F)
        np.testing.assert_array_equal(d, raw)
        np.testing.assert_array_equal(w[2], np.where(a.last_wrapper_state[EPLEN] + F(1.0) >= F(M), F(0.0), raw))
        differed += int((d != w[2]).sum())
        np.testing.assert_array_equal(a.S, b.S)
    assert differed == 1 and a.stats() == b.stats()


def _physics_twin(S, seed, act, k):
    """The block after k physics steps of `act` from S, and the rewards of those steps."""
    t = WalkerOracle(S.shape[1], seed=seed, max_ep_len=BIG, velocity_iterations=VIT, position_iterations=PIT)
    t.S[:] = S
    rews = []
    for _ in range(k):
        rews.append(t._physics(act)[0])
    return t.S.copy(), rews, t.obs()


@pytest.mark.parametrize("repeat", [2, 3])
def test_reward_forms_and_the_state_at_a_break(repeat):
    """Without noise, from the crafted block: where the loop ran out the reward is scale * (the float32 sum of the sub-steps' rewards)
    and the block is that of `repeat` physics steps; where `d` broke it at sub-step k the reward is 0.0 and the block is that of
    k + 1 physics steps, observation included; at repeat == 1 (the test above) neither scale nor noise is applied."""
    S, steps, census, _ = wws.trajectory(repeat, VIT, PIT, noisy=False)
    act_in, outs, act_out, _, behind, brk = steps[0]
    np.testing.assert_array_equal(act_in, act_out)
    o = WalkerWrappedOracle(wws.N, seed=wws.SEED, max_ep_len=BIG, velocity_iterations=VIT, position_iterations=PIT)
    o.S[:] = S
    scaled = [np.array(x) for x in o.step_wrapped(act_in.copy(), 0.0, 0.0, 5.0, repeat, wws.LIMIT)]
    assert sorted(set(brk)) == [-1] + list(range(repeat))
    for k in range(1, repeat + 1):
        blk, rews, obs = _physics_twin(S, wws.SEED, act_in, k)
        m = (brk == k - 1) | ((brk < 0) & (k == repeat))
        assert m.any()
        np.testing.assert_array_equal(behind[:, m], blk[:, m])
        np.testing.assert_array_equal(outs[0][m], obs[m])
        if k == repeat:
            out = brk < 0
            r = np.zeros(wws.N, F)
            for x in rews:
                r = (r + x).astype(F)
            np.testing.assert_array_equal(outs[1][out], r[out])                          # scale 1
            np.testing.assert_array_equal(scaled[1][out], (F(5.0) * r).astype(F)[out])   # scale 5
            assert (r[out] != 0).any()
    broke = brk >= 0
    assert (outs[1][broke] == 0).all() and (scaled[1][broke] == 0).all() and (outs[2][broke] == 1).all()
    assert (behind[PX][broke & (np.arange(wws.N) >= wws.ws.N)] < 0).all()                # the x_negative copies left on the left


def test_the_callers_action_array_holds_the_noisy_action():
    n = 5
    e = WalkerWrappedOracle(n, seed=2, max_ep_len=BIG, velocity_iterations=VIT, position_iterations=PIT)
    act = np.full((n, ACT), 0.25, F)
    st0 = e.S[PSTEP].astype(np.uint32)
    want = np.stack([F(0.25) + F(0.3) * (F(-2.0) * e._rng(st0, ACT_J0 + c) + F(1.0)) for c in range(ACT)], axis=1)
    e.step_wrapped(act, 0.3, 0.0, 1.0, 3, 1000)
    np.testing.assert_array_equal(act, want)
    assert (act != F(0.25)).all() and (np.abs(act.astype(np.float64) - 0.25) <= 0.3 + 1e-7).all()
    assert len(np.unique(act)) == act.size                       # four draws per env, none shared
    zero = np.full((n, ACT), 0.25, F)
    e.step_wrapped(zero, 0.0, 0.0, 1.0, 3, 1000)
    assert (zero == F(0.25)).all()


# ---- the GPU file's crafted run: its census floor, on the oracle alone -------------------------------------------------------------
@pytest.mark.parametrize("repeat", [1, 2, 3])
def test_the_crafted_run_reaches_every_branch_the_gpu_census_asks_for(repeat):
    _, steps, census, stats = wws.trajectory(repeat, VIT, PIT)
    print("repeat %d: %s" % (repeat, sorted(census.items())))
    assert len(steps) == wws.STEPS
    need = ["bare_step"] if repeat == 1 else ["break_at_%d" % k for k in range(repeat)] + ["ran_out"]
    for k in need + ["limit_without_d", "d_before_limit"]:
        assert census.get(k, 0) >= 1, (k, census)
    if repeat == 3:
        for k in range(3):                       # ... and each break by an x_negative copy, as built (with the action noise on)
            brk = steps[0][5][wws.ws.N:]
            assert (brk[k * wws.COPIES:(k + 1) * wws.COPIES] == k).all(), brk
    assert stats[0] >= wws.N                     # every env ends an episode within the two steps


# ---- the C ABI: name, prototype, rows -----------------------------------------------------------------------------------------------
def _headers():
    return [open(os.path.join(ROOT, "include", f)).read() for f in ("ddrl.h", "ddrl_walker.h")]


def test_the_new_name_in_its_header_the_ctypes_table_and_the_library():
    import ctypes
    from distributed_drl_amd import _lib
    hdr, hdr_w = _headers()
    name, twin = "ddrl_env_step_wrapped_walker", "ddrl_env_step_wrapped"
    so = os.path.join(ROOT, "distributed-drl_amd", "libddrl_hip.so")
    assert os.path.exists(so), "libddrl_hip.so is not built"
    lib = ctypes.CDLL(so)
    code = re.sub(r"/\*.*?\*/", "", hdr_w, flags=re.S)
    assert set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", code)) == set(_lib.SIGNATURES_WALKER) == {name}   # the header and its table, name for name
    assert not set(_lib.SIGNATURES_WALKER) & set(_lib.SIGNATURES)
    assert _lib.SIGNATURES_WALKER[name] == _lib.SIGNATURES[twin]        # the arguments of the one-body twin
    args = lambda f, h: [" ".join(p.split()) for p in re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % f, h, flags=re.S).group(1).split(",")]
    assert args(name, hdr_w) == args(twin, hdr)
    assert getattr(lib, name) is not None
    assert re.search(r'#include "ddrl.h"', hdr_w) and "ddrl_walker.h" in hdr      # each header names the other


def test_the_new_declaration_has_memory_contract_and_stream_rows():
    """tests/test_abi_table_cpu.py's checks, with its parse, on include/ddrl_walker.h against tests/_abi_contract_walker_nstep.TABLE:
    no declaration with caller device memory is uncovered and none that takes a stream, no row is for a function the header lacks,
    the rows name cases of that module, a deleted row or a new symbol fails the check, and every refusal listed has a row.  And
    include/ddrl.h's own checks hold with the module imported: it enters nothing in that header's table."""
    import _abi_contract as ac
    import _abi_contract_walker_nstep as aw
    from test_abi_table_cpu import stream_uncovered, takes_a_stream, takes_device_memory, uncovered
    hdr, hdr_w = _headers()
    need = takes_device_memory(hdr_w)
    assert sorted(need) == ["ddrl_env_step_wrapped_walker"] == takes_a_stream(hdr_w)
    assert need["ddrl_env_step_wrapped_walker"] == ["act_d", "obs2_d", "rew_d", "done_d", "next_obs_d", "ended_d"]
    assert uncovered(hdr_w, aw.TABLE, {}) == [] and stream_uncovered(hdr_w, aw.TABLE, {}) == []
    assert set(aw.TABLE) <= set(need)                                   # no row for a function that does not exist
    assert uncovered(hdr_w, {}, {}) == sorted(aw.TABLE) and stream_uncovered(hdr_w, {}, {}) == sorted(aw.TABLE)   # a deleted row fails
    grown = hdr_w.replace("#ifdef __cplusplus\n}", "int ddrl_x(float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != hdr_w and uncovered(grown, aw.TABLE, {}) == ["ddrl_x"] and stream_uncovered(grown, aw.TABLE, {}) == ["ddrl_x"]
    for f, rows in aw.TABLE.items():
        assert rows and all(cid in aw.CASES and f in aw.CASES[cid][1] for cid in rows), f
    assert sorted(c for rows in aw.TABLE.values() for c in rows) == sorted(aw.CASES)
    assert not set(aw.CASES) & set(ac.CASES) and not set(aw.CASES) & set(ac.STREAM_CASES)
    assert {p for f, p in aw.REFUSALS} == {"act_d", "obs2_d", "next_obs_d"}
    for f, p in aw.REFUSALS:
        assert f in aw.TABLE, f
    # include/ddrl.h and its table are as they were
    assert not set(aw.TABLE) & set(ac.TABLE) and not set(aw.TABLE) & set(takes_device_memory(hdr))
    assert uncovered(hdr, ac.TABLE, ac.EXEMPT) == [] and set(ac.TABLE) <= set(takes_device_memory(hdr))
    assert stream_uncovered(hdr, ac.STREAM_TABLE(), ac.STREAM_EXEMPT) == []
