"""The fused n-step rollout step on the ARTICULATED lander (ddrl_rollout_begin_nstep_articulated / ddrl_rollout_step_nstep_articulated,
csrc/rollout3_nstep.hip) and RolloutDeviceNStep's opt-in to it (opt.fused_nstep_rollout_articulated): the tests of
tests/test_gpu_nstep_rollout.py on this model, with that file's helpers.  Everything is compared bit for bit — with the unfused
sequence of the same worker (flag off: act_versioned, step_wrapped_articulated, push, masked store, adopt, begin), and with the NumPy
oracles (tests/lander3_wrapped_oracle.py, oracle/replay_oracle.py).  Every test asserts `ro._fused is True` where it claims the fused
path: nothing here passes on the fallback.  8 / 3 iterations unless stated: the solver's loops are run-time counts.
tests/test_lander3_wrapped_cpu.py shows on the oracle alone that the matrix's inputs make happen what the first test asserts."""
import ctypes
import os
import sys
from collections import deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_nstep_rollout import (EPI, EPLEN, LIMIT, _assert_same, _coded_weights, _decode_version, _perturbed, _ready_of, _snap,   # noqa: E402
                                    _stagger)
from test_gpu_nstep_rollout import _opt as _opt_one_body   # noqa: E402

VIT, PIT = 8, 3


def _opt(n, Ln, sf, fused, act_noise=0.3, start_steps=-1, seed=3, vit=VIT, pit=PIT):
    """fused: the articulated flag (True / False), or None to leave it unset."""
    opt = _opt_one_body(n, Ln, sf, True, act_noise=act_noise, start_steps=start_steps, seed=seed)
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", vit, pit
    if fused is not None:
        opt.fused_nstep_rollout_articulated = fused
    return opt


def _worker(opt, weights=None, stagger="long", ps=True):
    import distributed_drl_amd as ddrl
    from distributed_drl_amd.agent import Learner
    keys, vals = Learner(opt).get_weights()
    server = ddrl.ParameterServer(keys, vals if weights is None else weights(keys, vals)) if ps else None
    rb = ddrl.ReplayBufferNStep(opt)
    ro = ddrl.RolloutDeviceNStep(server, rb, opt)
    assert ro._versions and ro.limit_steps == LIMIT
    assert ro.env.model == getattr(opt, "env_model", "simple") and ro.env.state_fields == (66 if ro.env.model == "articulated" else 32)
    st = ro.env.get_state()
    st[EPLEN] = torch.from_numpy(_stagger(opt.num_envs)).cuda() if stagger == "long" else torch.arange(opt.num_envs, device="cuda").float() % LIMIT
    ro.env.set_state(st)
    return ro, rb, server, keys, vals


def _twins_in_lockstep(f, rbf, psf, u, rbu, psu, keys, vals, steps, Ln, sf, push=lambda s: s % 3 != 2):
    n = f.env.n
    epi0 = f.env.get_state()[EPI].cpu().numpy().copy()
    stored, base_rank_case, newest, versions_at_once = 0, 0, 0, 0
    for s in range(steps):
        ready = _ready_of(u, Ln, sf)
        stored += int(ready.sum())
        per_wg = [int(ready[k:k + 64].sum()) for k in range(0, n, 64)]
        base_rank_case += sum(1 for w in range(len(per_wg)) if per_wg[w] == 0 and sum(per_wg[w + 1:]) > 0)
        f.step()
        u.step()
        assert f._fused is True and f._fused_live and u._fused is False
        sf_, su_ = _snap(f, rbf), _snap(u, rbu)
        _assert_same(sf_, su_, "step %d" % s)
        versions_at_once = max(versions_at_once, len(set(sf_["slots"].tolist())))
        if push(s):
            newest += 1
            for ps in (psf, psu):
                ps.push(keys, _perturbed(keys, vals, newest))
    ended_all = bool((f.env.get_state()[EPI].cpu().numpy() > epi0).all())
    return stored, base_rank_case, versions_at_once, ended_all


@pytest.mark.parametrize("Ln,sf", [(4, 1), (4, 3), (8, 2)])
@pytest.mark.parametrize("n", [32, 96, 192])
def test_fused_step_equals_its_unfused_twin(n, Ln, sf):
    """Two workers from the same seeds, one with the flag off: after EVERY one of 50 vector steps the action mirror, env.obs, env.ended,
    the four queue arrays and t_queue, the 66-field state block, the four ring arrays, (ptr, size, steps), the actor's slots, `newest`
    and `out_of_slots` are equal.  Policy phase from the first step, action and observation noise, reward scale 5, a ring of 150 rows,
    a new policy version pushed after two steps out of three.  n = 32 / 96 / 192: half a wave, a ragged second workgroup, three."""
    f, rbf, psf, keys, vals = _worker(_opt(n, Ln, sf, True))
    u, rbu, psu, _, _ = _worker(_opt(n, Ln, sf, False))
    stored, base_rank_case, versions_at_once, ended_all = _twins_in_lockstep(f, rbf, psf, u, rbu, psu, keys, vals, 50, Ln, sf)
    assert stored > 150 and rbf._counts()[1] == 150     # the ring wrapped
    assert ended_all                                    # every env ended an episode
    assert versions_at_once >= 2                        # ... and envs sat on different versions at once
    if (n, Ln, sf) == (192, 4, 3):
        assert base_rank_case > 0                       # a workgroup without a ready env in front of one with some


def test_one_run_at_gyms_iteration_counts():
    """180 / 60 sweeps, n = 32, Ln 4, 12 steps: fused equals unfused after every step."""
    n, Ln, sf = 32, 4, 1
    f, rbf, psf, keys, vals = _worker(_opt(n, Ln, sf, True, vit=180, pit=60), stagger="phase")
    u, rbu, psu, _, _ = _worker(_opt(n, Ln, sf, False, vit=180, pit=60), stagger="phase")
    stored, _, _, ended_all = _twins_in_lockstep(f, rbf, psf, u, rbu, psu, keys, vals, 12, Ln, sf)
    assert stored > 0 and ended_all


def _against_the_oracles(fused):
    """act_noise = 0, so the action the worker reports is the raw one: fed to Lander3WrappedOracle.step_wrapped, with the deque
    restatement of the reference worker over NStepReplayOracle.  Mirrors at every step (fused: the kernel's; unfused: the env's
    tensors), ring arrays and counters at the end."""
    from distributed_drl_amd import _lib
    from lander3_wrapped_oracle import Lander3WrappedOracle
    from oracle.replay_oracle import NStepReplayOracle
    n, Ln, steps = 96, 4, 40
    opt = _opt(n, Ln, 1, fused, act_noise=0.0)
    ro, rb, _, _, _ = _worker(opt)
    if fused:
        assert ro._fused_ready() is True
        e = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
        m = dict(act=ro.act, obs2=e(n, 8), rew=e(n), done=e(n), next_obs=ro.env.obs, ended=ro.env.ended)
        ro._out = _lib.RolloutNStepOut(**{k: _lib.dptr(v) for k, v in m.items()})
    else:
        assert ro._fused_ready() is False
        m = dict(act=ro.act, obs2=ro.env.obs2, rew=ro.env.rew, done=ro.env.done, next_obs=ro.env.obs, ended=ro.env.ended)
    env = Lander3WrappedOracle(n, seed=opt.seed, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
    env.S[EPLEN] = _stagger(n)
    ora = NStepReplayOracle(opt)
    oq = [deque([(env.obs()[i].copy(),)], maxlen=Ln + 1) for i in range(n)]
    aq = [deque([], maxlen=Ln) for i in range(n)]
    tq = [1] * n
    for t in range(steps):
        ro.step()
        assert ro._fused is bool(fused) and ro._fused_live is bool(fused)
        act = ro.act.cpu().numpy().copy()
        o2, r, dd, nxt, ended = env.step_wrapped(act, 0.0, opt.obs_noise, opt.reward_scale, 3, LIMIT)
        for k, want in (("obs2", o2), ("rew", r), ("done", dd), ("next_obs", nxt), ("ended", ended)):
            np.testing.assert_array_equal(m[k].cpu().numpy(), want, err_msg="step %d %s" % (t, k))
        for i in range(n):
            aq[i].append((act[i].copy(), r[i], dd[i]))
            oq[i].append((o2[i].copy(),))
            if tq[i] >= Ln and tq[i] % opt.save_freq == 0:
                ora.store(oq[i], aq[i], 0)
            tq[i] += 1
            if ended[i]:
                oq[i] = deque([(nxt[i].copy(),)], maxlen=Ln + 1)
                aq[i] = deque([], maxlen=Ln)
                tq[i] = 1
    np.testing.assert_array_equal(ro.env.get_state().cpu().numpy(), env.S)
    rings = rb.rings()
    for k in ("buffer_o", "buffer_a", "buffer_r", "buffer_d"):
        np.testing.assert_array_equal(rings[k].cpu().numpy(), getattr(ora, k), err_msg=k)
    assert rb.get_counts() == ora.get_counts()
    assert ora.steps > opt.buffer_size and env.stats()[0] >= n   # the ring wrapped, episodes ended


def test_fused_step_against_the_oracles():
    _against_the_oracles(True)


def test_flag_unset_the_worker_steps_the_articulated_env_unfused():
    """opt.env_model = "articulated" with the flag unset: the worker builds the articulated env (it used to build the one-body one
    whatever opt.env_model said), stays on the unfused sequence through step_wrapped_articulated, and its ring rows are that env's
    transitions — the oracles' of the articulated model, bit for bit."""
    _against_the_oracles(None)


def test_changing_between_the_paths():
    """Five random-action steps (unfused), fused steps, one forced unfused step, fused again: equal to an all-unfused twin after every
    step (the begin call rebuilds the observation rows and the readiness bytes whenever the unfused calls have run)."""
    n, Ln, sf = 96, 4, 3
    f, rbf, psf, keys, vals = _worker(_opt(n, Ln, sf, True, start_steps=4))
    u, rbu, psu, _, _ = _worker(_opt(n, Ln, sf, False, start_steps=4))
    fused_steps = 0
    for s in range(36):
        forced = s == 20
        if forced:
            f._fused = False
        f.step()
        u.step()
        if forced:
            assert not f._fused_live
            f._fused = True
        if s < 5:
            assert f._fused is None and not f._fused_live     # random-action phase: the unfused sequence
        elif not forced:
            assert f._fused is True and f._fused_live
            fused_steps += 1
        _assert_same(_snap(f, rbf), _snap(u, rbu), "step %d" % s)
        if s % 4 == 1:
            for ps in (psf, psu):
                ps.push(keys, _perturbed(keys, vals, s))
    assert fused_steps == 30 and rbf._counts()[1] == 150 and u._fused is False


def _c_step(ro, rb, n_steps, adopt=1):
    from distributed_drl_amd import _lib
    a, opt = ro.actor, ro.opt
    _lib.check(a._lib.ddrl_rollout_step_nstep_articulated(ro.env._h, a._h, ro.winq._h, rb._h, n_steps, float(opt.act_noise), float(opt.obs_noise),
                                                          float(opt.reward_scale), 3, ro.limit_steps, adopt, a._noise_seed, a._noise_ctr,
                                                          ctypes.byref(ro._out), _lib.stream_ptr()))
    a._noise_ctr += n_steps * ro.env.n * 2


def test_four_steps_in_one_call_equal_four_calls():
    """n_steps = 4 in one C call against four calls with n_steps = 1, with a second policy version live (envs move to it at their
    episode ends inside the call), three times in a row."""
    n, Ln, sf = 96, 4, 1
    one, rb1, ps1, keys, vals = _worker(_opt(n, Ln, sf, True), stagger="phase")
    four, rb4, ps4, _, _ = _worker(_opt(n, Ln, sf, True), stagger="phase")
    for ro, ps in ((one, ps1), (four, ps4)):
        assert ro._fused_ready() is True
        ps.push(keys, _perturbed(keys, vals, 1))
        assert ro.pull()
    for rep in range(3):
        _c_step(one, rb1, 4)
        for _ in range(4):
            _c_step(four, rb4, 1)
        a, b = _snap(one, rb1), _snap(four, rb4)
        _assert_same(a, b, "call %d" % rep)
        assert a["vs"][0] == 1
    assert set(a["slots"].tolist()) == {1} and one._fused is True and four._fused is True   # limit_steps = 7 < 12 steps: every env has moved


@pytest.mark.parametrize("adopt", [True, False])
def test_adoption_on_the_fused_path(adopt):
    """Bias-coded versions, no action noise, a push after four steps out of five — every env acts on the version its own episode end
    pulled (sac_ray.py:252-262).  adopt = False: the buffer never reaches start_steps, adopt_at_episode_end stays off and no env ever
    leaves version 0."""
    n, steps = 64, 50
    opt = _opt(n, 4, 1, True, act_noise=0.0, start_steps=0 if adopt else 10 ** 9)
    opt.obs_noise, opt.reward_scale, opt.buffer_size = 0.0, 1, 4000
    ro, rb, ps, keys, vals = _worker(opt, weights=_coded_weights, stagger="phase")
    assert ro.actor.n_slots == 9
    if not adopt:
        ro.filling_steps = opt.start_steps + 1      # the policy phase, although the buffer's steps never exceed start_steps
    holds = np.zeros(n, int)
    newest, learning, seen = 0, False, set()
    for s in range(steps):
        policy_phase = ro.filling_steps > opt.start_steps
        ro.step()
        learning = learning or rb.get_counts()[1] > opt.start_steps
        if policy_phase:
            assert ro._fused is True and ro._fused_live
            used = _decode_version(ro.act.cpu().numpy())
            np.testing.assert_array_equal(used, holds, err_msg="step %d" % s)
            seen.update(used.tolist())
        ended = ro.env.ended.cpu().numpy().astype(bool)
        if learning:
            holds[ended] = newest
        if s % 5 != 4:
            newest += 1
            ps.push(keys, _coded_weights(keys, vals, newest))
    assert not ro.actor.version_state(with_slots=False)[1]["out_of_slots"]
    if adopt:
        assert len(seen) >= 10
    else:
        assert seen == {0} and not learning and (ro.actor.version_state()[0].cpu().numpy() == 0).all()


def test_the_flag_changes_nothing_on_a_one_body_worker():
    """opt.fused_nstep_rollout_articulated set with opt.env_model unset: the worker is the one-body worker — same env, fused through
    the one-body pair, the same bits as a worker without the flag."""
    import distributed_drl_amd as ddrl
    from distributed_drl_amd.agent import Learner
    n, Ln, sf = 64, 4, 1
    pair = []
    for flag in (True, None):
        opt = _opt_one_body(n, Ln, sf, True)
        if flag:
            opt.fused_nstep_rollout_articulated = True
        keys, vals = Learner(opt).get_weights()
        rb = ddrl.ReplayBufferNStep(opt)
        ro = ddrl.RolloutDeviceNStep(ddrl.ParameterServer(keys, vals), rb, opt)
        assert ro.env.model == "simple" and ro.env.state_fields == 32
        pair.append((ro, rb))
    for s in range(10):
        for ro, rb in pair:
            ro.step()
            assert ro._fused is True and ro._fused_live
            assert ro._rollout_calls()[1] is ro.actor._lib.ddrl_rollout_step_nstep
        _assert_same(_snap(*pair[0]), _snap(*pair[1]), "step %d" % s)


def test_a_worker_without_a_server():
    """ps=None (a rollout rank of partition.py): random actions while filling, then the policy phase on the fused pair."""
    n, Ln, sf = 64, 4, 1
    ro, rb, server, _, _ = _worker(_opt(n, Ln, sf, True, start_steps=3), ps=False)
    assert server is None and ro.ps is None
    for s in range(12):
        ro.step()
        if s >= 4:
            assert ro._fused is True and ro._fused_live
    assert rb.get_counts()[1] > 0 and ro.filling_steps == 4


def test_refusals_leave_everything_unchanged():
    """Outside the envelope the new pair returns the documented status with the reason in ddrl_last_error() and touches neither the
    envs, nor the queues, nor the ring, nor the actor's slots; and the one-body pair still refuses an articulated handle."""
    import distributed_drl_amd as ddrl
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Actor
    from distributed_drl_amd.env import VecLunarLander
    from distributed_drl_amd.workers import WindowQueue
    lib = _lib.load()
    n, Ln = 64, 4
    opt = _opt(n, Ln, 1, True)
    ro, rb, _, _, _ = _worker(opt)
    assert ro._fused_ready() is True
    for _ in range(6):
        ro.step()               # queues and ring hold something
    assert ro._fused is True and rb._counts()[1] > 0
    h = lambda x: None if x is None else x._h

    def step(env=ro.env, actor=ro.actor, winq=ro.winq, ring=rb, out=ro._out, f=lib.ddrl_rollout_step_nstep_articulated):
        return f(h(env), h(actor), h(winq), h(ring), 1, 0.3, 0.01, 5.0, 3, LIMIT, 1, 7, 0, None if out is None else ctypes.byref(out), None)

    def begin(env=ro.env, actor=ro.actor, winq=ro.winq, f=lib.ddrl_rollout_begin_nstep_articulated):
        return f(h(env), h(actor), h(winq), None)

    U, B = _lib.DDRL_ERR_UNSUPPORTED, _lib.DDRL_ERR_BAD_ARG
    opt48 = _opt(48, Ln, 1, True)
    opt17 = _opt(n, 17, 1, True)
    env3 = lambda k: VecLunarLander(k, seed=1, model="articulated", velocity_iterations=VIT, position_iterations=PIT)
    one_body = VecLunarLander(n, seed=1)
    ob_state = one_body.get_state().clone()
    cases = [
        ("one-body handle", dict(env=one_body), U, b"this handle holds the one-body model", True),
        ("five-array ring", dict(ring=ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)), U, b"four-array", False),
        ("queue Ln != ring Ln", dict(winq=WindowQueue(n, 5, 8, 2)), U, b"windows", False),
        ("n = 48", dict(env=env3(48), actor=Actor(opt48, max_rows=48), winq=WindowQueue(48, Ln, 8, 2)), U, b"multiple of 32", True),
        ("Ln = 17", dict(winq=WindowQueue(n, 17, 8, 2), ring=ddrl.ReplayBufferNStep(opt17)), U, b"DDRL_NSTEP_FUSED_MAX_LN", True),
        ("NULL env", dict(env=None), B, b"NULL", True),
        ("NULL actor", dict(actor=None), B, b"NULL", True),
        ("NULL queues", dict(winq=None), B, b"NULL", True),
        ("NULL ring", dict(ring=None), B, b"NULL", False),
    ]
    before = _snap(ro, rb)
    others = {}
    for name, kw, status, reason, at_begin in cases:
        ring = kw.get("ring")
        if ring is not None:
            others[name] = (ring, {k: v.clone() for k, v in ring.rings().items()}, ring._counts())
        assert step(**kw) == status, name
        msg = lib.ddrl_last_error()
        assert reason in msg, (name, msg)
        if name == "one-body handle":
            assert b"ddrl_rollout_step_nstep_articulated" in msg and b"use ddrl_rollout_step_nstep" in msg, msg
        if at_begin:
            assert begin(**{k: v for k, v in kw.items() if k != "ring"}) == status, name
            msg = lib.ddrl_last_error()
            assert reason in msg, (name, msg)
            if name == "one-body handle":
                assert b"ddrl_rollout_begin_nstep_articulated" in msg and b"use ddrl_rollout_begin_nstep" in msg, msg
    # the one-body pair still refuses an articulated handle
    assert step(f=lib.ddrl_rollout_step_nstep) == U and b"ddrl_rollout_step_nstep" in lib.ddrl_last_error()
    assert begin(f=lib.ddrl_rollout_begin_nstep) == U and b"ddrl_rollout_begin_nstep" in lib.ddrl_last_error()
    _assert_same(before, _snap(ro, rb), "after the refused calls")
    assert torch.equal(one_body.get_state(), ob_state)
    for name, (ring, rows, counts) in others.items():
        assert ring._counts() == counts, name
        for k, v in ring.rings().items():
            assert torch.equal(v, rows[k]), (name, k)
    ro.step()                    # ... and the worker goes on
    assert ro._fused is True and ro._fused_live
