"""The fused DISCRETE rollout step on the ARTICULATED lander (ddrl_rollout_begin_discrete_articulated /
ddrl_rollout_step_discrete_articulated / ddrl_env_rollout_mirrors, kernel csrc/rollout3_q.hip) and RolloutDeviceDQN's opt-in to it
(opt.fused_discrete_rollout_articulated): transitions and ring rows BIT-EXACT against tests/lander3_oracle.py given the GPU's own
actions, the Q rows against the float64 Q oracle, the actions against the selection oracle, the fused step against the unfused
sequence bit for bit, per-env weight adoption against n reference workers, n_steps, the ring wrap, the refusals, and a run through
ActorLearnerLoop.
Every test that uses a fused worker first asserts that the worker IS fused (tests/_lander3_discrete.Worker) and that every fused step
left `_fused_live` set: a silent fallback to the unfused path fails."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402
import _discrete_versions as dv  # noqa: E402
import _lander3_discrete as l3  # noqa: E402


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


# ---- 1. bit-exact transitions given the GPU's own actions ------------------------------------------------------------------------------
def test_transitions_and_ring_rows_bit_exact_given_the_gpus_actions(ddrl):
    """96 envs = two workgroups, the second half full, the cursor ticket crossing them.  Zero kernels and head bias (1, 0, 0, 0) at
    greedy_prob 0.8: the lander mostly free-falls and crashes (the CPU oracle alone puts the first crash near step 50 and nearly every env
    on the ground by step 100; the time limit of 100 ends the few still falling, so every env resets inside the run), and the random
    branch exercises the other three table rows.  Six unfused random-action steps first, so the fused path starts through the
    _fused_live refresh; then 100 fused steps."""
    n, fused_steps, limit = 96, 100, 100
    c = l3.case("ddqn", n)
    w = l3.Worker(c, limit, dv.coded(c, 1), start_steps=5 * n, cap=(6 + fused_steps) * n + 50)
    w.roll.actor.greedy_prob = 0.8
    ora = l3.oracle(w.opt)
    l3.lockstep(w, ora, 6, fused_from=6)
    assert not w.roll._fused_live and w.roll.t == 6 * n          # the random phase ran unfused
    done, ended = l3.lockstep(w, ora, fused_steps, t0=6, fused_from=6)
    assert int((done == 1).sum()) >= n // 2                      # terminal rows went through the fused store
    acts = w.rb.rings()["acts_buf"][6 * n:(6 + fused_steps) * n].cpu().numpy()
    assert set(acts.tolist()) == {0.0, 1.0, 2.0, 3.0}
    assert l3.check_end(w, ora, 6 + fused_steps) >= n


# ---- 2. gym's iteration counts, every env at its time limit -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_the_same_at_gym_iterations_with_every_env_at_its_time_limit(ddrl, family):
    """180 / 60, 64 envs, max_ep_len 3, 7 steps, the time limits staggered on both sides: an episode ends in every step."""
    n, steps, limit = 64, 7, 3
    c = l3.case(family, n, seed=13)
    w = l3.Worker(c, limit, ap.q_params(c), vit=180, pit=60, cap=steps * n + 7)
    ora = l3.oracle(w.opt)
    w.stagger()
    ora.S[dv.EPLEN] = np.arange(n) % limit
    np.testing.assert_array_equal(w.roll.env.get_state().cpu().numpy(), ora.S)
    done, ended = l3.lockstep(w, ora, steps)
    assert ended.any(axis=1).all() and not done.any()             # the time limit ends the episode and is not a terminal (train.py)
    assert l3.check_end(w, ora, steps) == int(ended.sum()) >= 2 * n


# ---- 3. Q rows, selection and the unfused path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,hidden,seed", l3.Q_CASES)
def test_q_rows_selection_and_the_unfused_sequence(ddrl, family, hidden, seed):
    """64 envs, random weights (ap.q_params, weight seed 13), alpha 0.1, env seed 3, time limit 9, 12 steps, greedy_prob 0.5.
    Q mirror: the project's bars against the float64 Q oracle (_acting_parity.compare: twice the float32 oracle's own deviation under
    permuted summation orders, rms and element-wise).  Actions: the selection oracle on the device's own q rows and the oracle's uniforms
    (_discrete_versions.check_actions: exact for Double-DQN).  SQN: the boundary cap allows NO excluded row at n = 64, so these cases
    (weight seed 13, alpha 0.1, env seed 3, 12 steps) were chosen on the CPU — the float32 Q oracle on Lander3Oracle's observations,
    da.uniforms, the boundaries at a ten times wider margin, 1e-4: no row of any checked step is near one
    (tests/_lander3_discrete.sqn_rows_near_a_boundary; tests/test_lander3_discrete_rollout_cpu.py asserts it).
    Fused against unfused: a twin env, actor and ring driven by get_actions (ddrl_dqn_act) + env.step (ddrl_env_step_discrete) +
    store_batch with the same seed and counter: state, obs, ring rows, counters, act and q bit for bit after every step."""
    c = l3.q_case(family, hidden, seed)
    params = ap.q_params(c)
    kw = dict(seed=l3.Q_ENV_SEED, cap=l3.Q_STEPS * c.batch)
    w = l3.Worker(c, l3.Q_LIMIT, params, **kw)
    twin = l3.Worker(c, l3.Q_LIMIT, params, fused=False, flag=None, **kw)
    a, b = w.roll, twin.roll
    for r in (a, b):
        r.actor._noise_seed, r.actor._noise_ctr, r.actor.greedy_prob = l3.NOISE_SEED, 0, l3.Q_GREEDY
    b_act, b_q = torch.zeros(c.batch, device="cuda"), torch.zeros(c.batch, c.act, device="cuda")
    ck = dv.Checks()
    picked = set()
    for t in range(l3.Q_STEPS):
        label = "%s step %d" % (c.id, t)
        obs = a.env.obs.cpu().numpy().copy()
        ctr = a.actor._noise_ctr
        assert ctr == 2 * c.batch * t
        w.fused_step()
        q, act = a.q_out.cpu().numpy(), a.act.cpu().numpy()
        m_act, m_q, m_nxt = a.env.rollout_mirrors()
        assert torch.equal(m_q, a.q_out) and torch.equal(m_act, a.act) and torch.equal(m_nxt, a.env.obs), label
        ck.compare(q, ap.q_reference(c, params, obs), "q1", label)
        dv.check_actions(ck, c, q, act, l3.NOISE_SEED, ctr, l3.Q_GREEDY, label)
        picked |= set(act.tolist())
        # the unfused sequence on the twin
        o = b.env.obs.clone()
        b.actor.get_actions(o, out=b_act, q_out=b_q)
        o2, r, d, _, _ = b.env.step(b_act)
        twin.rb.store_batch(o, b_act, r, o2, d)
        got = dict(state=a.env.get_state(), obs=a.env.obs, act=a.act, q=a.q_out, **w.rb.rings())
        want = dict(state=b.env.get_state(), obs=b.env.obs, act=b_act, q=b_q, **twin.rb.rings())
        for k in want:
            assert torch.equal(got[k], want[k]), "%s: fused against unfused: %s" % (label, k)
        assert tuple(w.rb._counts()) == tuple(twin.rb._counts()), label
    assert a.actor._noise_ctr == b.actor._noise_ctr == 2 * c.batch * l3.Q_STEPS
    assert len(picked) >= 3, picked
    assert a.env.stats() == b.env.stats() and a.env.get_state()[dv.EPI].sum().item() >= c.batch   # every env through a reset
    ck.finish()


# ---- 4. per-env adoption equals n reference workers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
@pytest.mark.parametrize("n,limit,steps", [(64, 7, 40), (160, 23, 70)])
def test_each_env_acts_on_the_version_its_own_reference_worker_would_hold(ddrl, family, n, limit, steps):
    """Bias-coded versions (tests/_discrete_versions.py), staggered time limits, pushes on sac_schedule: after every step the Q mirror
    names, env by env, the version that env's own reference worker held before the step; an env whose episode ended in a step holds what
    the server held during it."""
    c = l3.case(family, n)
    w = l3.Worker(c, limit, dv.coded(c, 0), adopt="episode")
    assert w.roll._versions and w.roll.actor.n_slots == min(n, limit) + 2
    w.stagger()
    push_after = dv.sac_schedule(limit, steps)
    for s in range(steps):
        q, before = w.versioned_step()
        np.testing.assert_array_equal(dv.decode(q), before, err_msg="step %d" % s)
        np.testing.assert_array_equal(w.roll.env.rollout_mirrors()[1].cpu().numpy(), q)
        if s in push_after:
            w.push(push_after[s], dv.coded(c, push_after[s]))
    slots, st = w.roll.actor.version_state()
    slots = slots.cpu().numpy()
    assert not st["out_of_slots"] and w.max_live > 1 and w.max_live >= min(limit, 6), w.max_live
    # the actor's slot table agrees: envs share a slot exactly where their reference workers hold the same version
    pairs = set(zip(w.holds.tolist(), slots.tolist()))
    assert len(pairs) == len(set(w.holds.tolist())) == len(set(slots.tolist())), pairs
    assert w.roll.env.stats()[0] >= n * (steps // limit - 1)


# ---- 5. n_steps ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_four_steps_in_one_call_equal_four_calls_with_a_version_live(ddrl, family):
    n, limit = 64, 5
    c = l3.case(family, n, seed=13)
    v0, v1 = ap.q_params(c), ap.q_params(c, version=1)
    ws = [l3.Worker(c, limit, v0, adopt="episode", cap=8 * n) for _ in range(2)]
    for w in ws:
        assert w.roll._versions
        w.stagger()                                          # an episode ends somewhere in every step
        w.fused_step()
        w.fused_step()
        w.push(1, v1)                                        # a second version goes live inside the steps compared
    a, b = ws
    a.fused_step(4)
    for _ in range(4):
        b.fused_step()
    assert a.roll.t == b.roll.t == 6 * n and a.roll.actor._noise_ctr == b.roll.actor._noise_ctr == 6 * n * 2
    dv.same(a.snapshot(slots=True), b.snapshot(slots=True), "n_steps = 4 against 4 x n_steps = 1")
    assert len(set(a.roll.actor.version_state()[0].cpu().numpy().tolist())) == 2
    assert a.roll.env.stats() == b.roll.env.stats()
    a.fused_step()
    b.fused_step()
    dv.same(a.snapshot(slots=True), b.snapshot(slots=True), "the step after")


# ---- 6. ring wrap ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,capacity", [(96, 200), (64, 40)])
def test_ring_wrap_and_rows_a_later_store_of_the_batch_overwrites(ddrl, n, capacity):
    """(96, 200): the cursor wraps inside the third step.  (64, 40): n > capacity, only the last 40 envs of a step are stored.
    The ring equals one filled by store_batch with the oracle's transitions in the same order."""
    c = l3.case("ddqn", n, seed=13)
    w = l3.Worker(c, 40, ap.q_params(c), cap=capacity)
    w.roll.actor.greedy_prob = 0.5
    ref = ddrl.ReplayBufferDQN(w.opt, 0, seed=5)
    ora = l3.oracle(w.opt)
    for t in range(3):
        obs = ora.obs()
        np.testing.assert_array_equal(w.roll.env.obs.cpu().numpy(), obs)
        w.fused_step()
        act = w.roll.act.cpu().numpy().copy()
        o2, r, d, _, _ = ora.step(da.table_actions(act))
        ref.store_batch(*(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (obs, act, r, o2, d)))
    got, want = w.rb.rings(), ref.rings()
    for k in l3.RINGS:
        assert torch.equal(got[k], want[k]), k
    assert tuple(w.rb._counts())[:3] == tuple(ref._counts())[:3] == ((3 * n) % capacity, min(3 * n, capacity), 3 * n)
    assert w.rb.ptr == ref.ptr == (3 * n) % capacity


# ---- 7. refusals and defaults -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_untouched_defaults(ddrl):
    """Every refusal of the pair: DDRL_ERR_UNSUPPORTED, the function's name in the message (a one-body handle: the discrete pair to use
    instead), and env state, env.obs, a deterministic Q forward of fixed rows, ring counters, cursor and rows and — once it exists — the
    mirror block unchanged.  The refusal of handles on different devices runs only where a second GPU exists."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLanderDiscrete
    from distributed_drl_amd.replay import ReplayBuffer
    from distributed_drl_amd.workers import RolloutDeviceDQN
    lib = _lib.load()
    sp = _lib.stream_ptr
    BEGIN, STEP = "ddrl_rollout_begin_discrete_articulated", "ddrl_rollout_step_discrete_articulated"

    class Ring1D(ReplayBuffer):
        _acts_1d = True

    def ring(kind="1d"):
        rb = {"1d": lambda: Ring1D(8, 1, 256), "2d": lambda: ReplayBuffer(8, 2, 256), "compact": lambda: Ring1D(8, 1, 256, compact_obs=True)}[kind]()
        acts = torch.floor(torch.rand(40, 2, device="cuda") * 4) if kind == "2d" else torch.floor(torch.rand(40, device="cuda") * 4)
        obs = torch.floor(torch.rand(40, 8, device="cuda") * 200)           # integer-valued: what a compact ring represents
        rb.store_batch(obs, acts, torch.rand(40, device="cuda"), obs + 1, torch.zeros(40, device="cuda"))   # "unchanged" is not "still empty"
        return rb

    def art(n, device=None):
        return VecLunarLanderDiscrete(n, seed=4, max_ep_len=50, model="articulated", velocity_iterations=l3.VIT, position_iterations=l3.PIT, device=device)

    def actor_of(c, max_rows):
        return dv.q_actor(c, max_rows=max_rows)[0]

    lander = l3.case("ddqn", 64)
    # (what, env, actor, ring, begin refused?, a version store enabled behind a passing begin?)
    cases = [("one-body", VecLunarLanderDiscrete(64, seed=4, max_ep_len=50), actor_of(lander, 64), ring(), True, False),
             ("no acting forward", art(64), actor_of(ap.QCase("ddqn-h50", "ddqn", 8, 4, (50, 34), 64), 64), ring(), True, False),
             ("obs_dim 6", art(64), actor_of(ap.QCase("sqn-obs6", "sqn", 6, 5, (40, 28), 64, alpha=0.2), 64), ring(), True, False),
             ("n = 48", art(48), actor_of(l3.case("ddqn", 48), 48), ring(), True, False),
             ("n above the batch", art(64), actor_of(l3.case("ddqn", 32), 32), ring(), True, False),
             ("store rows != envs", art(64), actor_of(lander, 128), ring(), True, True),
             ("2-D actions", art(64), actor_of(lander, 64), ring("2d"), False, False),
             ("compact ring", art(64), actor_of(lander, 64), ring("compact"), False, False)]
    if torch.cuda.device_count() >= 2:   # handles on different devices: only where a second GPU exists (env state alone is compared)
        with torch.cuda.device(1):
            far = art(64)
            s0 = far.get_state().clone()
        near_actor, near_ring = actor_of(lander, 64), ring()
        for name, call in ((BEGIN, lambda: lib.ddrl_rollout_begin_discrete_articulated(far._h, near_actor._h, sp())),
                           (STEP, lambda: lib.ddrl_rollout_step_discrete_articulated(far._h, near_actor._h, near_ring._h, 1, 0, 0.5, 1, 0, sp()))):
            assert call() == _lib.DDRL_ERR_UNSUPPORTED and lib.ddrl_last_error().decode().startswith(name) and b"device" in lib.ddrl_last_error()
            with torch.cuda.device(1):
                assert torch.equal(far.get_state(), s0), name
    for what, env, actor, rb, begin_refused, store in cases:
        for _ in range(3):
            env.step(env.sample_actions())
        probe = torch.rand(actor.max_rows, actor.cfg.obs_dim, device=actor.device)
        calls = {STEP: lambda: lib.ddrl_rollout_step_discrete_articulated(env._h, actor._h, rb._h, 1, 0, 0.5, 1, 0, sp())}
        if begin_refused:
            calls[BEGIN] = lambda: lib.ddrl_rollout_begin_discrete_articulated(env._h, actor._h, sp())
        if store:    # without a store 64 of the 128 rows may begin and step; with one the pair steps exactly the forward's rows
            assert lib.ddrl_rollout_begin_discrete_articulated(env._h, actor._h, sp()) == 0, lib.ddrl_last_error()
            assert calls[STEP]() == 0, lib.ddrl_last_error()
            actor.enable_versions(14)
        elif not begin_refused:
            assert lib.ddrl_rollout_begin_discrete_articulated(env._h, actor._h, sp()) == 0, lib.ddrl_last_error()

        def snapshot():
            torch.cuda.synchronize()
            qq = torch.zeros(actor.max_rows, actor.cfg.n_actions, device=actor.device)
            actor.get_actions(probe, deterministic=True, q_out=qq)
            snap = [env.get_state().clone(), env.obs.clone(), qq, torch.tensor(list(rb._counts()) + [rb.ptr])]
            snap += [v.clone() for _, v in sorted(rb.rings().items())]
            try:
                snap += [m.clone() for m in env.rollout_mirrors()]
            except ValueError:
                assert begin_refused and not store, what      # no begin call has passed on this handle
            return snap

        before = snapshot()
        for name, call in calls.items():
            assert call() == _lib.DDRL_ERR_UNSUPPORTED, (what, name, lib.ddrl_last_error())
            msg = lib.ddrl_last_error().decode()
            assert msg.startswith(name), (what, name, msg)
            if what == "one-body":   # ... and says which function takes this handle
                assert name.replace("_articulated", "") in msg.replace(name, ""), msg
            after = snapshot()
            assert len(after) == len(before)
            for k, (x, y) in enumerate(zip(before, after)):
                assert torch.equal(x, y), (what, name, k)
    # n_steps < 1 and a bad mode: DDRL_ERR_BAD_ARG; ddrl_env_rollout_mirrors before any begin call: DDRL_ERR_BAD_ARG
    env, actor, rb = art(64), actor_of(lander, 64), ring()
    import ctypes
    ptrs = [ctypes.c_void_p() for _ in range(3)]
    dims = [ctypes.c_int32(), ctypes.c_int32()]
    mirrors = lambda: lib.ddrl_env_rollout_mirrors(env._h, *[ctypes.byref(x) for x in ptrs + dims])
    assert mirrors() == _lib.DDRL_ERR_BAD_ARG and b"ddrl_env_rollout_mirrors" in lib.ddrl_last_error()
    assert lib.ddrl_rollout_begin_discrete_articulated(env._h, actor._h, sp()) == 0, lib.ddrl_last_error()
    assert mirrors() == 0 and (dims[0].value, dims[1].value) == (64, 4) and all(p.value for p in ptrs) and ptrs[2].value % 16 == 0
    assert lib.ddrl_rollout_step_discrete_articulated(env._h, actor._h, rb._h, 0, 0, 0.5, 1, 0, sp()) == _lib.DDRL_ERR_BAD_ARG
    assert lib.ddrl_rollout_step_discrete_articulated(env._h, actor._h, rb._h, 1, 7, 0.5, 1, 0, sp()) == _lib.DDRL_ERR_BAD_ARG
    assert lib.ddrl_rollout_step_discrete_articulated(env._h, actor._h, rb._h, 1, 0, 0.5, 1, 0, sp()) == 0, lib.ddrl_last_error()
    # the one-body pair keeps refusing an articulated handle
    assert lib.ddrl_rollout_begin_discrete(env._h, actor._h, sp()) == _lib.DDRL_ERR_UNSUPPORTED
    # ---- the worker's defaults
    c = l3.case("ddqn", 32)
    params = ap.q_params(c)
    for kw, want in ((dict(flag=None), False), (dict(flag=False), False), (dict(flag=True), True),
                     (dict(flag=None, model="simple"), True), (dict(flag=True, model="simple"), True)):
        w = l3.Worker(c, 25, params, fused=None, **kw)
        w.roll.step()
        assert w.roll._fused is want and w.roll._fused_live is want, (kw, w.roll._fused)
    for kind in ("compact", "2d"):      # a ring the fused step does not store into: the worker stays unfused, flag or not
        opt = l3.make_opt(c, 25, flag=True)
        roll = RolloutDeviceDQN(ddrl.ParameterServer(list(params.keys()), list(params.values())), ring(kind), opt)
        assert roll._fused_ready() is False and roll._fused is False, kind


# ---- 8. through ActorLearnerLoop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_through_the_actor_learner_loop(ddrl, family):
    from distributed_drl_amd import dqn
    from distributed_drl_amd.workers import ActorLearnerLoop, RolloutDeviceDQN, TrainDeviceDQN
    n = 32
    c = l3.case(family, n)
    opt = l3.make_opt(c, 25, start_steps=0, cap=4096, seed=2)
    opt.batch_size, opt.a_l_ratio, opt.push_freq = 32, 2, 8
    L = dqn.LearnerSQN if family == "sqn" else dqn.Learner
    ps = ddrl.ParameterServer(*L(opt).get_weights())
    rb = ddrl.ReplayBufferDQN(opt, 0, seed=4)
    roll = RolloutDeviceDQN(ps, rb, opt)
    assert roll._fused_ready() is True and roll._fused is True
    trainer = TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0))
    w0 = trainer.agent.export().clone()
    loop = ActorLearnerLoop(roll, trainer, opt)
    loop.run(4)
    torch.cuda.synchronize()
    assert roll._fused is True and roll._fused_live and roll.t == 4 * n
    assert rb.get_counts() == (4 * n // 2, 4 * n, 4 * n) and loop.sample_times == 4 * n // 2
    w1 = trainer.agent.export()
    assert torch.isfinite(w1).all() and not torch.equal(w0, w1)
