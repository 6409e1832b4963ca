"""The discrete rollout's version store: RolloutDeviceDQN(adopt="episode") — ddrl_dqn_versions_enable / _state / _adopt, the versioned
Q forward and k_env_step_q<.., true> — acts, for every env and every step, on exactly the weights that env's own reference worker would hold
(algos/dqn/train.py:249-252: env.reset(), ps.pull, agent.set_weights once per episode, for that env only).

REFERENCES  which version: the `holds` bookkeeping of tests/_discrete_versions.py on bias-coded versions, exactly; the Q rows of real
            networks: the float64 forward of tests/_acting_parity.py under its compare(..., "q1") rule, per live version; the actions: the
            NumPy selection on the device's own q rows (exact for Double-DQN; SQN sampling: the boundary exclusion, capped at 1 % of the rows);
            env, ring and counters: oracle/env_oracle.LanderOracle and oracle/replay_oracle.ReplayBufferOracle fed the device's actions, bit
            for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402
import _discrete_versions as dv  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


# ---- 1. equals N reference workers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
@pytest.mark.parametrize("n,limit,steps,wg_slots", [(64, 7, 60, None), (160, 23, 90, None), (1024, 37, 64, 24), (4096, 70, 170, None)])
def test_discrete_rollout_equals_n_reference_workers_in_the_weights_each_env_acts_on(ddrl, monkeypatch, family, n, limit, steps, wg_slots):
    """Bias-coded versions make the version behind every Q row readable.  Pushes land between vector steps: a burst, one per step for
    limit + 3 steps, a pause longer than limit (the single-version launch pair), then at random; the time limits are staggered, so episodes
    end in every step, env by env, and up to min(n, limit) + 1 versions are live at once.  160 envs: partial row tiles; 1024 envs on a
    24-workgroup "chip" (DDRL_VER_WG_SLOTS): the env-step launch's table build walks the multi-round split of ver_split."""
    if wg_slots is not None:
        monkeypatch.setenv("DDRL_VER_WG_SLOTS", str(wg_slots))
    c = dv.case(family, n)
    w = dv.Worker(c, limit, dv.coded(c, 0))
    assert w.roll._versions and w.roll.actor.n_slots == min(n, limit) + 2
    push_after = dv.sac_schedule(limit, steps)
    for s in range(steps):
        q = w.step()
        np.testing.assert_array_equal(dv.decode(q), w.holds_before, err_msg="step %d" % s)
        if s in push_after:
            w.push(push_after[s], dv.coded(c, push_after[s]))
    _, st = w.roll.actor.version_state()
    assert not st["out_of_slots"]
    assert w.max_live >= min(limit, 6), w.max_live
    assert w.roll.env.stats()[0] >= n * (steps // limit - 1)


# ---- 2. real networks: every version's own Q function --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,limit,steps,hidden", [("ddqn", 96, 9, 30, (400, 300)), ("sqn", 256, 11, 16, (64, 32))])
def test_versioned_discrete_rollout_matches_each_versions_own_q_function(ddrl, family, n, limit, steps, hidden):
    """A new random parameter set is pushed every second step.  Per step: the Q rows of every live version's envs against that version's
    float64 forward; the actions against the selection oracle on the device's own q rows; env state, next-observation mirror, ring rows
    and counters bit for bit against the oracles fed the device's actions.  (400, 300): ragged column tiles."""
    from oracle.env_oracle import LanderOracle
    from oracle.replay_oracle import ReplayBufferOracle
    c = dv.case(family, n, hidden=hidden, alpha=0.1, seed=12)
    vers = {0: ap.q_params(c)}
    cap = n * steps
    w = dv.Worker(c, limit, vers[0], cap=cap)
    assert w.roll._versions
    w.roll.actor.greedy_prob = 0.5                     # Double-DQN: both branches of the coin flip
    ora, rbo = LanderOracle(n, seed=int(w.opt.seed), max_ep_len=limit), ReplayBufferOracle(8, 1, cap, acts_1d=True)
    ora.S[dv.EPLEN] = np.arange(n) % limit
    np.testing.assert_array_equal(w.roll.env.get_state().cpu().numpy(), ora.S)
    ck = dv.Checks()
    o, n_ended = ora.obs(), 0
    for s in range(steps):
        seed, ctr = w.roll.actor._noise_seed, w.roll.actor._noise_ctr
        q = w.step()
        act = w.roll.act.cpu().numpy()
        label = "%s versions step %d" % (c.id, s)
        for v in sorted(set(w.holds_before.tolist())):
            rows = np.nonzero(w.holds_before == v)[0]
            ck.compare(q[rows], ap.q_reference(c, vers[v], o[rows]), "q1", "%s version %d" % (label, v))
        dv.check_actions(ck, c, q, act, seed, ctr, 0.5, label)
        o2, r, d, nxt, ended = ora.step(da.table_actions(act))
        rbo.store_batch(o, act, r, o2, d)
        n_ended += int(ended.sum())
        g = {k: x.cpu().numpy() for k, x in w.rb.rings().items()}
        rows = np.arange(rbo.size)
        for k, want in (("obs1_buf", rbo.obs1_buf), ("obs2_buf", rbo.obs2_buf), ("acts_buf", rbo.acts_buf), ("rews_buf", rbo.rews_buf), ("done_buf", rbo.done_buf)):
            np.testing.assert_array_equal(g[k][rows], want[rows], err_msg="%s: %s" % (label, k))
        np.testing.assert_array_equal(w.roll.env.obs.cpu().numpy(), nxt, err_msg=label + ": next-observation mirror")
        np.testing.assert_array_equal(w.roll.env.get_state().cpu().numpy(), ora.S, err_msg=label + ": env state block")
        assert tuple(w.rb._counts())[:3] == (rbo.ptr, rbo.size, rbo.steps), label
        o = nxt
        if s % 2 == 0:
            vers[w.newest + 1] = ap.q_params(c, version=w.newest + 1)
            w.push(w.newest + 1, vers[w.newest + 1])
    assert len(set(w.holds.tolist())) >= 3 and n_ended >= n
    ge, _, gl = w.roll.env.stats()
    assert (ge, gl) == (ora.episodes, ora.len_sum)
    assert not w.roll.actor.version_state(with_slots=False)[1]["out_of_slots"]
    ck.finish()


# ---- 3. store enabled, nothing pushed ----------------------------------------------------------------------------------------------------
def _run_snapshot(w, steps, push_same_at=None, params=None):
    for s in range(steps):
        if push_same_at == s:
            w.push(1, params)
        w.step()
    r = w.rb.rings()
    return dict(state=w.roll.env.get_state().cpu().numpy(), counts=tuple(w.rb._counts()), act=w.roll.act.cpu().numpy(), q=w.roll.q_out.cpu().numpy(),
                obs=w.roll.env.obs.cpu().numpy(), **{k: v.cpu().numpy().copy() for k, v in r.items()})


@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_store_enabled_and_nothing_pushed_is_the_step_rollout_bit_for_bit(ddrl, family):
    """adopt="episode" against adopt="step" on the same seeds and initial weights (real ones: non-zero head biases), 64 envs, time limit 12,
    30 steps: ring arrays, env state and the act / q mirrors bit-identical."""
    c = dv.case(family, 64, seed=13)
    params = ap.q_params(c)
    runs = {}
    for adopt in ("episode", "step"):
        w = dv.Worker(c, 12, params, adopt=adopt, cap=64 * 30)
        assert w.roll._versions == (adopt == "episode")
        runs[adopt] = _run_snapshot(w, 30)
    dv.same(runs["episode"], runs["step"], "adopt='episode' with nothing pushed against adopt='step'")
    assert len(set(runs["step"]["acts_buf"].tolist())) == 4


@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_a_second_version_with_the_same_weights_is_the_step_rollout_bit_for_bit(ddrl, family):
    """The same pair of runs with the initial weights pushed AGAIN after step 3: in the "episode" run they are version 1 in a slot of its
    own, the envs move to it one by one (slot 0's and slot 1's bias offsets, the versioned forward, mixed row tiles), and every row is
    computed as the plain launch computes it — a row's partials do not depend on the tile it sits in."""
    c = dv.case(family, 64, seed=13)
    params = ap.q_params(c)
    runs = {}
    for adopt in ("episode", "step"):
        w = dv.Worker(c, 12, params, adopt=adopt, cap=64 * 30)
        runs[adopt] = _run_snapshot(w, 30, push_same_at=4, params=params)
        if adopt == "episode":
            slots, st = w.roll.actor.version_state()
            assert st["newest"] == 1 and (slots.cpu().numpy() == 1).all()      # every env has been through an episode end since
    dv.same(runs["episode"], runs["step"], "version 1 = version 0's weights against adopt='step'")


# ---- 4. n_steps = 4 in one call equals four calls, a version live --------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_four_steps_in_one_call_equal_four_calls_with_a_version_live(ddrl, family):
    c = dv.case(family, 64, seed=13)
    v1 = ap.q_params(c, version=1)
    a, b = dv.Fused(c, 1000, 64, 12), dv.Fused(c, 1000, 64, 12)
    for f in (a, b):
        assert f.begin() == 0, f.lib.ddrl_last_error()
        f.actor.enable_versions(14)
        f.actor.set_weights(list(v1.keys()), list(v1.values()))
        assert f.step() == 0 and f.step() == 0, f.lib.ddrl_last_error()
        slots = f.actor.version_state()[0].cpu().numpy()
        assert set(slots.tolist()) == {0, 1}, slots                  # some envs have adopted the version, others have not
    assert a.step(4) == 0, a.lib.ddrl_last_error()
    for _ in range(4):
        assert b.step(1) == 0, b.lib.ddrl_last_error()
    assert a.ctr == b.ctr
    dv.same(a.snapshot(slots=True), b.snapshot(slots=True), "n_steps = 4 against 4 x n_steps = 1")
    assert a.step(1) == 0 and b.step(1) == 0
    dv.same(a.snapshot(slots=True), b.snapshot(slots=True), "the step after")


# ---- 5. the random-action phase adopts too --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_random_phase_adopts_at_episode_ends(ddrl, family):
    """start_steps = 3 n: four vector steps of random actions (t <= start_steps), a push after each of them, time limit 5, staggered.  From the
    first policy-phase step on every env acts on the version its own worker pulled at its last episode end, random phase included."""
    n, limit = 64, 5
    c = dv.case(family, n)
    w = dv.Worker(c, limit, dv.coded(c, 0), start_steps=3 * n)
    assert w.roll._versions
    for s in range(4):
        assert w.step() is None and w.roll._fused_live is False
        w.push(s + 1, dv.coded(c, s + 1))
    assert len(set(w.holds.tolist())) >= 3, w.holds          # the random phase left several versions live
    for s in range(4, 12):
        q = w.step()
        np.testing.assert_array_equal(dv.decode(q), w.holds_before, err_msg="step %d" % s)
        if s == 5:
            w.push(5, dv.coded(c, 5))
    assert w.roll._fused_live and not w.roll.actor.version_state(with_slots=False)[1]["out_of_slots"]


# ---- 6. get_actions beside a live store -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_get_actions_beside_a_live_store_acts_on_the_newest_version(ddrl, family):
    n, limit = 64, 9
    c = dv.case(family, n)
    w = dv.Worker(c, limit, dv.coded(c, 0))
    for s in range(3):
        q = w.step()
        np.testing.assert_array_equal(dv.decode(q), w.holds_before, err_msg="step %d" % s)
        w.push(s + 1, dv.coded(c, s + 1))
    q = w.step()                                            # pulls version 3
    np.testing.assert_array_equal(dv.decode(q), w.holds_before)
    assert len(set(w.holds.tolist())) >= 3, w.holds
    slots0, st0 = w.roll.actor.version_state()
    qq = torch.full((n, 4), float("nan"), device="cuda")
    obs = torch.from_numpy(ap.q_inputs(c)).cuda()
    w.roll.actor.get_actions(obs, q_out=qq)
    np.testing.assert_array_equal(dv.decode(qq.cpu().numpy()), np.full(n, 3))    # the newest version's rows, whatever slot an env is on
    slots1, st1 = w.roll.actor.version_state()
    assert torch.equal(slots0, slots1) and st0 == st1
    for s in range(4, 8):
        q = w.step()
        np.testing.assert_array_equal(dv.decode(q), w.holds_before, err_msg="step %d, after get_actions" % s)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_version_store_refusals(ddrl):
    from distributed_drl_amd import _lib
    lib = _lib.load()
    sp = _lib.stream_ptr
    # a handle without an acting forward: wide observations
    wide = [c for c in ap.Q_CASES if c.id == "ddqn-wide-1028"][0]
    actor, _ = dv.q_actor(wide)
    assert lib.ddrl_dqn_versions_enable(actor._h, 8, sp()) == _lib.DDRL_ERR_UNSUPPORTED
    assert b"observations too wide" in lib.ddrl_last_error(), lib.ddrl_last_error()
    c = dv.case("ddqn", 64)
    actor, _ = dv.q_actor(c)
    ended = torch.zeros(64, dtype=torch.uint8, device="cuda")
    state = (ctypes.c_int32 * 4)()
    # before enable
    assert lib.ddrl_dqn_versions_state(actor._h, None, state, sp()) != 0 and b"not enabled" in lib.ddrl_last_error()
    assert lib.ddrl_dqn_versions_adopt(actor._h, _lib.dptr(ended), 64, sp()) != 0 and b"not enabled" in lib.ddrl_last_error()
    # n_slots outside [2, 2048]
    for bad in (1, 2049):
        assert lib.ddrl_dqn_versions_enable(actor._h, bad, sp()) != 0 and b"[2, 2048]" in lib.ddrl_last_error()
    assert lib.ddrl_dqn_versions_enable(actor._h, 2, sp()) == 0, lib.ddrl_last_error()
    # twice
    assert lib.ddrl_dqn_versions_enable(actor._h, 4, sp()) != 0 and b"already enabled" in lib.ddrl_last_error()
    assert lib.ddrl_dqn_versions_state(actor._h, None, state, sp()) == 0 and list(state) == [0, 0, 0, 0]
    assert lib.ddrl_dqn_versions_adopt(actor._h, _lib.dptr(ended), 64, sp()) == 0
    # a fused step with a store and n_envs != the acting forward's rows: refused, nothing changed
    f = dv.Fused(c, 1000, 64, 12, max_rows=128)
    assert f.begin() == 0 and f.step() == 0, f.lib.ddrl_last_error()      # without a store 64 of the 128 rows may step
    f.actor.enable_versions(14)
    before = f.snapshot()
    assert f.step() != 0 and b"version store" in f.lib.ddrl_last_error(), f.lib.ddrl_last_error()
    dv.same(before, f.snapshot(), "refused n_envs != rows")
