"""GPU parity of the ARTICULATED lander (csrc/env3_device.h) on the crafted-state scenarios of tests/_lander3_scenarios.py: the
start block is injected into VecLunarLander(model="articulated") and into tests/lander3_oracle.py, the scenario's actions are run on
both, and the five outputs of every step, the final state block and stats() are compared BIT FOR BIT — on states the live matrix of
tests/test_gpu_lander3.py never reaches (rest and the sleep counter, the far side of both joint limits, all eight corners, slopes,
chunk boundaries and the clamped end segments, every hull vertex's crash, |angle| in the tens of radians), with the classes of a
scenario interleaved inside every wave.  tests/test_lander3_scenarios_cpu.py holds the floor under what the scenarios reach.
Then one mixed scenario through the other launch paths that compile env3_device.h: the discrete step, the fused continuous rollout
step (csrc/rollout3.hip) and the fused discrete one (csrc/rollout3_q.hip), bit-exact given the GPU's own actions.  The evaluation
kernels (csrc/eval3.hip: ddrl_env_eval_policy / ddrl_env_eval_q) are not here: they play whole episodes from the reset and read no
state block, so a crafted state cannot be handed to them through the API."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _lander3_scenarios as Z   # noqa: E402
from test_lander3_scenarios_cpu import check_invariants   # noqa: E402

NAMES = ("obs2", "rew", "done", "next_obs", "ended")
TABLE = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], np.float32)   # ddrl_env_step_discrete's action table


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _env(scn, cls=None):
    from distributed_drl_amd.env import VecLunarLander
    S0, _, (vit, pit, max_ep_len) = scn
    env = (cls or VecLunarLander)(S0.shape[1], seed=Z.SEED, max_ep_len=max_ep_len, model="articulated", velocity_iterations=vit,
                                  position_iterations=pit)
    env.set_state(torch.from_numpy(S0).cuda())
    return env


def _compare(env, outs, run, what):
    """Device outputs collected per step (cloned, no sync until here) against the oracle's run."""
    final = env.get_state().cpu().numpy()
    for t, (got, want) in enumerate(zip(outs, run["outs"])):
        for name, gv, wv in zip(NAMES, got, want):
            np.testing.assert_array_equal(gv.cpu().numpy(), wv, err_msg="%s: %s at step %d" % (what, name, t))
    np.testing.assert_array_equal(final, run["final"], err_msg=what)
    ge, gr, gl = env.stats()
    we, wr, wl = run["stats"]
    assert (ge, gl) == (we, wl) and ge == sum(int(w[4].sum()) for w in run["outs"]), what
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr)), what
    check_invariants(final, None, (what, "kernel's final state"))


@pytest.mark.parametrize("name", list(Z.SCENARIOS))
def test_scenario_bit_exact_vs_oracle(ddrl, name):
    scn = Z.SCENARIOS[name]()
    env = _env(scn)
    acts = torch.from_numpy(scn[1]).cuda()
    outs, states = [], []
    for t in range(acts.shape[0]):
        outs.append([x.clone() for x in env.step(acts[t])])
        states.append(env.get_state())
    run = Z.oracle_run(name)
    _compare(env, outs, run, name)
    # the exact invariants on the kernel's own state after every step; where no episode ended it is the oracle's after-state
    for t, s in enumerate(states):
        s = s.cpu().numpy()
        check_invariants(s, None, (name, t))
        keep = ~run["outs"][t][4].astype(bool)
        np.testing.assert_array_equal(s[Z.L3.K0:Z.L3.K0 + 16][:, keep], run["last"][t]["state"][Z.L3.K0:Z.L3.K0 + 16][:, keep])
        check_invariants(np.ascontiguousarray(s[:, keep]), run["last"][t]["on"][:, keep], (name, t, "contact mask"))


def test_mixed_through_the_discrete_step(ddrl):
    """ddrl_env_step_discrete from the mixed start block: random table indices, the resting classes (env id % 8 < 2) on index 0."""
    from distributed_drl_amd.env import VecLunarLanderDiscrete
    S0, acts, model = Z.SCENARIOS["mixed"]()
    T, n = acts.shape[:2]
    idx = np.random.RandomState(9).randint(0, 4, (T, n))
    idx[:, np.arange(n) % 8 < 2] = 0
    scn = (S0, TABLE[idx], model)
    env = _env(scn, VecLunarLanderDiscrete)
    dev = torch.from_numpy(idx.astype(np.float32)).cuda()
    outs = [[x.clone() for x in env.step(dev[t])] for t in range(T)]
    run = Z.run_oracle(scn)
    _compare(env, outs, run, "mixed, discrete step")
    assert Z.waves_with_contact_rest_exit_and_free_lane(run) > 0


def _inject(roll, S0, ora):
    """The crafted block into a rollout worker's env and into its oracle; the next fused step runs its begin call again, as after
    any ddrl_env_set_state issued outside the fused path."""
    ora.S[:] = S0
    roll.env.set_state(torch.from_numpy(S0).cuda())
    roll.env.obs.copy_(torch.from_numpy(ora.obs()).cuda())
    roll._fused_live = False


def test_mixed_through_the_fused_rollout_step(ddrl):
    """ddrl_rollout_step_articulated (csrc/rollout3.hip) from the mixed start block, engines off (the free-fall policy): transitions
    and ring rows bit-exact given the GPU's actions, and the replayed oracle's census shows contact, a rest exit and a lane without
    contact in one wave."""
    import test_gpu_lander3_rollout as R
    S0, acts, (vit, pit, max_ep_len) = Z.SCENARIOS["mixed"]()
    T, n = acts.shape[:2]
    opt = R._opt(n, max_ep_len, seed=Z.SEED, vit=vit, pit=pit)
    keys, vals = R._weights(opt)
    cap = T * n + 50
    roll, rb, _ = R._worker(ddrl, opt, (keys, R._free_fall(keys, vals)), cap)
    assert roll._fused_ready() is True
    ora = R._oracle(opt)
    _inject(roll, S0, ora)
    rec = Z.record_steps(ora)
    R._lockstep(roll, rb, ora, T, cap)
    R._check_end(roll, rb, ora, T, cap)
    assert Z.waves_with_contact_rest_exit_and_free_lane(rec) > 0
    check_invariants(roll.env.get_state().cpu().numpy(), None, "fused rollout")


def test_mixed_through_the_fused_discrete_rollout_step(ddrl):
    """ddrl_rollout_step_discrete_articulated (csrc/rollout3_q.hip) from the mixed start block: zero kernels and head bias
    (1, 0, 0, 0), greedy — index 0, engines off."""
    import _discrete_versions as dv
    import _lander3_discrete as l3
    S0, acts, (vit, pit, max_ep_len) = Z.SCENARIOS["mixed"]()
    T, n = acts.shape[:2]
    c = l3.case("ddqn", n)
    w = l3.Worker(c, max_ep_len, dv.coded(c, 1), cap=T * n + 50, seed=Z.SEED, vit=vit, pit=pit)
    w.roll.actor.greedy_prob = 1.0
    ora = l3.oracle(w.opt)
    _inject(w.roll, S0, ora)
    rec = Z.record_steps(ora)
    l3.lockstep(w, ora, T)
    l3.check_end(w, ora, T)
    assert (w.rb.rings()["acts_buf"][:T * n].cpu().numpy() == 0).all()
    assert Z.waves_with_contact_rest_exit_and_free_lane(rec) > 0
    check_invariants(w.roll.env.get_state().cpu().numpy(), None, "fused discrete rollout")
