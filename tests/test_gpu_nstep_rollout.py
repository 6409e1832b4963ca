"""The fused n-step rollout step (ddrl_rollout_begin_nstep / ddrl_rollout_step_nstep, csrc/rollout_nstep.hip): policy head, Wrapper'd
env step, window queues, masked window store, adoption and episode starts in the ONE launch behind the actor's forward.  Everything is
compared bit for bit — with the unfused sequence of RolloutDeviceNStep (opt.fused_nstep_rollout = False: the launches the worker
issued before), and with the NumPy oracles.  Every test asserts `ro._fused is True`: nothing here passes on the fallback.

Compared of the actor's version store: every env's slot, `newest` and `out_of_slots`.  `live` and `tiles` of version_state() describe
the most recent PLANNING pass, and the two paths plan at different moments by design (the unfused forward plans in front of itself
from the slots before the step, the fused launch plans at its end for the next forward), so these two numbers are not compared."""
import ctypes
from collections import deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LIMIT = 7          # max_ep_len 14 / action_repeat 2
EPLEN, EPI = 10, 13


def _stagger(n):
    """EPLEN per env (float32).  The first workgroup's 64 envs share one episode phase, the others walk through all seven; every env's
    first episode is 7, 14, 21 or 28 steps longer than the limit allows later ones (negative EPLEN), so that windows of Ln = 8 fill at
    all.  Checked on the CPU with oracle/env_oracle.py (50 steps, capacity 150): >= 240 ready rows in every (n, Ln, save_freq) case, every
    env ends an episode by step 31, and at n = 192, (Ln, save_freq) = (4, 3) some twenty-four steps have a workgroup without a ready env
    in front of one with some."""
    i = np.arange(n)
    phase = np.where(i < 64, 3, i % LIMIT)
    return (phase - (7 * (i % 4) + 7)).astype(np.float32)


def _opt(n, Ln, sf, fused, act_noise=0.3, start_steps=-1, seed=3):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.hidden_sizes = (64, 48)
    opt.num_envs, opt.seed, opt.Ln, opt.save_freq, opt.max_ep_len, opt.action_repeat, opt.start_steps = n, seed, Ln, sf, 14, 2, start_steps
    opt.buffer_size, opt.batch_size, opt.num_buffers = 150, 8, 1
    opt.obs_noise, opt.act_noise, opt.reward_scale = 0.01, act_noise, 5
    opt.fused_nstep_rollout = fused
    return opt


def _worker(opt, weights=None, stagger="long"):
    import distributed_drl_amd as ddrl
    from distributed_drl_amd.agent import Learner
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals if weights is None else weights(keys, vals))
    rb = ddrl.ReplayBufferNStep(opt)
    ro = ddrl.RolloutDeviceNStep(ps, rb, opt)
    assert ro._versions and ro.limit_steps == LIMIT
    st = ro.env.get_state()   # "long": _stagger; "phase": every env on the limit of 7 from its first episode on, phases 0..6
    st[EPLEN] = torch.from_numpy(_stagger(opt.num_envs)).cuda() if stagger == "long" else torch.arange(opt.num_envs, device="cuda").float() % LIMIT
    ro.env.set_state(st)
    return ro, rb, ps, keys, vals


def _t_queue(ro):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.replay import _view
    tq = ctypes.c_void_p()
    _lib.check(_lib.load().ddrl_winq_buffers(ro.winq._h, None, ctypes.byref(tq)))
    return _view(tq.value, (ro.env.n,), ro.env.device).view(torch.int32)


def _snap(ro, rb, mirrors=True):
    """Everything a vector step may touch, as host arrays."""
    c = lambda t: t.detach().cpu().numpy().copy()
    s = {}
    if mirrors:
        s.update(act=c(ro.act), obs=c(ro.env.obs), ended=c(ro.env.ended))
    for k, a in zip("oard", ro.winq.arrays):
        s["q" + k] = c(a)
    s["t"] = c(_t_queue(ro))
    s["state"] = c(ro.env.get_state())
    for k, a in rb.rings().items():
        s[k] = c(a)
    s["counts"] = np.array(rb._counts()[:3])   # ptr, size, steps
    slots, vs = ro.actor.version_state()
    s["slots"] = c(slots)
    s["vs"] = np.array([vs["newest"], int(vs["out_of_slots"])])
    return s


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _perturbed(keys, vals, v):
    rs = np.random.RandomState(100 + v)
    return [(w + (0.3 * rs.standard_normal(w.shape)).astype(np.float32) * (0.2 if w.ndim == 2 else 1.0)) for w in vals]


def _ready_of(ro, Ln, sf):
    t = _t_queue(ro).cpu().numpy()
    return (t >= Ln) & (t % sf == 0)


@pytest.mark.parametrize("Ln,sf", [(4, 1), (4, 3), (8, 2)])
@pytest.mark.parametrize("n", [32, 96, 192])
def test_fused_step_equals_its_unfused_twin(n, Ln, sf):
    """Two workers from the same seeds, one on the unfused sequence: after EVERY vector step the action mirror, env.obs, env.ended, the
    four queue arrays and t_queue, the env state block, the four ring arrays, (ptr, size, steps) and the actor's slots are equal.
    Policy phase from the first step, action and observation noise, reward scale 5, a ring of 150 rows (it wraps), a new policy version
    pushed after two steps out of three.  n = 32 / 96 / 192: half a wave, a ragged second workgroup, three workgroups."""
    steps = 50
    f, rbf, psf, keys, vals = _worker(_opt(n, Ln, sf, True))
    u, rbu, psu, _, _ = _worker(_opt(n, Ln, sf, False))
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
        if s % 3 != 2:
            newest += 1
            for ps in (psf, psu):
                ps.push(keys, _perturbed(keys, vals, newest))
    assert stored > 150 and rbf._counts()[1] == 150                                     # the ring wrapped
    assert (f.env.get_state()[EPI].cpu().numpy() > epi0).all()                          # every env ended an episode
    assert versions_at_once >= 2                                                        # ... and envs sat on different versions at once
    if (n, Ln, sf) == (192, 4, 3):
        assert base_rank_case > 0                                                       # a workgroup without a ready env in front of one with some


def test_fused_step_against_the_oracles():
    """act_noise = 0, so the action the kernel reports is the raw one: fed to LanderOracle.step_wrapped, with the deque restatement of
    test_gpu_driver.py::test_nstep_rollout_equals_per_env_reference_loop over NStepReplayOracle.  The obs2 / rew / done / ended /
    next_obs mirrors equal the oracle's at every step; ring arrays and counters are equal at the end."""
    from distributed_drl_amd import _lib
    from oracle.env_oracle import LanderOracle
    from oracle.replay_oracle import NStepReplayOracle
    n, Ln, steps = 96, 4, 40
    opt = _opt(n, Ln, 1, True, act_noise=0.0)
    ro, rb, _, _, _ = _worker(opt)
    assert ro._fused_ready() is True
    e = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    m = dict(act=ro.act, obs2=e(n, 8), rew=e(n), done=e(n), next_obs=ro.env.obs, ended=ro.env.ended)
    ro._out = _lib.RolloutNStepOut(**{k: _lib.dptr(v) for k, v in m.items()})
    env = LanderOracle(n, seed=opt.seed, max_ep_len=1 << 23)
    env.S[EPLEN] = _stagger(n)
    ora = NStepReplayOracle(opt)
    oq = [deque([(env.obs()[i].copy(),)], maxlen=Ln + 1) for i in range(n)]
    aq = [deque([], maxlen=Ln) for i in range(n)]
    tq = [1] * n
    for t in range(steps):
        ro.step()
        assert ro._fused is True and ro._fused_live
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
    rings = rb.rings()
    for k in ("buffer_o", "buffer_a", "buffer_r", "buffer_d"):
        np.testing.assert_array_equal(rings[k].cpu().numpy(), getattr(ora, k), err_msg=k)
    assert rb.get_counts() == ora.get_counts()
    assert ora.steps > opt.buffer_size and env.stats()[0] >= n   # the ring wrapped, episodes ended


def test_changing_between_the_paths():
    """Five random-action steps (unfused), fused steps, one forced unfused step, fused again: equal to an all-unfused twin after every
    step (ddrl_rollout_begin_nstep rebuilds the observation rows and the readiness bytes whenever the unfused calls have run)."""
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
            assert f._fused is None and not f._fused_live     # random-action phase: the present sequence
        elif not forced:
            assert f._fused is True and f._fused_live
            fused_steps += 1
        _assert_same(_snap(f, rbf), _snap(u, rbu), "step %d" % s)
        if s % 4 == 1:
            for ps in (psf, psu):
                ps.push(keys, _perturbed(keys, vals, s))
    assert fused_steps == 30 and rbf._counts()[1] == 150


def _c_step(ro, rb, n_steps, adopt=1):
    from distributed_drl_amd import _lib
    a, opt = ro.actor, ro.opt
    _lib.check(a._lib.ddrl_rollout_step_nstep(ro.env._h, a._h, ro.winq._h, rb._h, n_steps, float(opt.act_noise), float(opt.obs_noise),
                                              float(opt.reward_scale), 3, ro.limit_steps, adopt, a._noise_seed, a._noise_ctr,
                                              ctypes.byref(ro._out), _lib.stream_ptr()))
    a._noise_ctr += n_steps * ro.env.n * 2


def test_four_steps_in_one_call_equal_four_calls():
    """n_steps = 4 in one C call against four calls with n_steps = 1, with a second policy version live (envs move to it at their
    episode ends inside the call), twice in a row."""
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


def _coded_weights(keys, vals, v=0):
    """Policy version v as a recognisable action (tests/test_gpu_driver.py): zero kernels, mu biases 0.08 (v % 40 + 1) and
    0.08 (v // 40 + 1), log_std at its floor."""
    out = []
    for k, w in zip(keys, vals):
        w = np.zeros_like(w)
        if "pi" in k and k.endswith("dense_2/bias"):
            w[0], w[1:] = 0.08 * (v % 40 + 1), 0.08 * (v // 40 + 1)
        if "pi" in k and k.endswith("dense_3/bias"):
            w[:] = -40.0
        out.append(w)
    return out


def _decode_version(acts):
    d = [np.rint(np.arctanh(np.clip(acts[:, c], -0.9999, 0.9999)) / 0.08 - 1).astype(int) for c in (0, 1)]
    assert np.allclose(acts[:, 0], np.tanh(0.08 * (d[0] + 1)), atol=1e-6) and np.allclose(acts[:, 1], np.tanh(0.08 * (d[1] + 1)), atol=1e-6)
    return d[0] + 40 * d[1]


@pytest.mark.parametrize("adopt", [True, False])
def test_adoption_on_the_fused_path(adopt):
    """The scenario of test_gpu_driver.py::test_nstep_rollout_weight_adoption_equals_the_reference_workers with the fused path asserted
    live: bias-coded versions, no action noise, a push after four steps out of five — every env acts on the version its own episode
    end pulled (sac_ray.py:252-262).  adopt = False: the buffer never reaches start_steps, adopt_at_episode_end stays off and no env
    ever leaves version 0."""
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


def test_refusals_leave_everything_unchanged():
    """Outside the envelope the two entry points return the documented status with the reason in ddrl_last_error() and touch neither
    the envs, nor the queues, nor the ring, nor the actor's slots."""
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

    def step(env=ro.env, actor=ro.actor, winq=ro.winq, ring=rb, out=ro._out):
        h = lambda x: None if x is None else x._h
        return lib.ddrl_rollout_step_nstep(h(env), h(actor), h(winq), h(ring), 1, 0.3, 0.01, 5.0, 3, LIMIT, 1, 7, 0,
                                           None if out is None else ctypes.byref(out), None)

    def begin(env=ro.env, actor=ro.actor, winq=ro.winq):
        h = lambda x: None if x is None else x._h
        return lib.ddrl_rollout_begin_nstep(h(env), h(actor), h(winq), None)

    U, B = _lib.DDRL_ERR_UNSUPPORTED, _lib.DDRL_ERR_BAD_ARG
    opt48 = _opt(48, Ln, 1, True)
    opt17 = _opt(n, 17, 1, True)
    env3 = VecLunarLander(n, seed=1, model="articulated", velocity_iterations=4, position_iterations=2)
    cases = [
        ("articulated", dict(env=env3), U, b"articulated", True),
        ("five-array ring", dict(ring=ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)), U, b"four-array", False),
        ("compact ring", dict(ring=ddrl.ReplayBuffer(8, 2, 256, compact_obs=True)), U, b"four-array", False),
        ("queue Ln != ring Ln", dict(winq=WindowQueue(n, 5, 8, 2)), U, b"windows", False),
        ("n = 48", dict(env=VecLunarLander(48, seed=1), actor=Actor(opt48, max_rows=48), winq=WindowQueue(48, Ln, 8, 2)), U, b"multiple of 32", True),
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
        assert reason in lib.ddrl_last_error(), (name, lib.ddrl_last_error())
        if at_begin:
            assert begin(**{k: v for k, v in kw.items() if k != "ring"}) == status, name
            assert reason in lib.ddrl_last_error(), (name, lib.ddrl_last_error())
    _assert_same(before, _snap(ro, rb), "after the refused calls")
    for name, (ring, rows, counts) in others.items():
        assert ring._counts() == counts, name
        for k, v in ring.rings().items():
            assert torch.equal(v, rows[k]), (name, k)
    ro.step()                    # ... and the worker goes on
    assert ro._fused is True and ro._fused_live
