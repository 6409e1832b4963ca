"""Every policy / Q forward a rollout worker calls, on every kernel path, against the float64 oracles (tests/_acting_parity.py; the CPU
half, tests/test_oracle_acting_parity.py, shows that the bars see eleven kinds of planted defect).

PATHS   row-major          ddrl_actor_act / Actor.get_actions          k_l1 + k_gemm + k_rows_act; explicit eps, deterministic, and
                                                                         eps drawn on the device (eps=None); the row counts of the case,
                                                                         a short call straight after a long one
        one-launch         ddrl_actor_act_one / Actor.get_action        k_act_one, noise from the counter inside the kernel; act > 4:
                                                                         the fallback to the batched kernels ("one-launch-fallback")
        direct-plain       ddrl_actor_act_versioned, no version pending k_actor_fwd<NS, OCC> + k_actor_finish
        direct-versioned   ddrl_actor_act_versioned after set_weights   k_version_plan + k_actor_fwd<NS, 2, versioned> + k_actor_finish:
                           + adopt_where_ended                          every row against the oracle of the version IT holds; then, HORIZON
                                                                         calls later, the plain launch against the newest version
        fused rollout      ddrl_rollout_step at 4128 envs               k_actor_fwd<5, 2> + k_env_step_pi (OCC = 2: the existing test runs
                                                                         4096 envs, a grid of exactly 256)
        q                  ddrl_dqn_q / q_values / _q_row / get_action  k_gemm or k_wide + the head job; n = 1, 2, batch - 1, batch

BARS    rms and element-wise deviation from the float64 oracle <= 2 x the float32 oracle ensemble's own + 2^-22 max |x64|, computed per
        call at test time (tests/_acting_parity.py).  K = 2 on every case and path; no ensemble extension was needed.

Also: one direct and one row-major actor driven through a fixed interleaving of set_weights / get_actions / get_action /
get_actions_versioned / get_weights / adopt_where_ended over five weight sets, every result held to the oracle with the weights that call
should see; acting between two updates leaves main / target / m / v of DDQN, SQN and SAC learners bit-identical.

OBSERVED on an MI355X: profiles/acting_parity_observed.txt lists every (case, path) with its rms and maximum deviation, both bars and the
ratios.  DDRL_ACTING_TABLE=<file>: append the measured lines to that file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402

from oracle import dqn_oracle as do  # noqa: E402
from oracle import sac1_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


class _Checks:
    """Every comparison of a test is made before anything is raised; the measured lines go to DDRL_ACTING_TABLE and into the failure message."""

    def __init__(self):
        self.table, self.bad = [], []

    def compare(self, got, ref, kind, label, device_noise=False):
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        try:
            ap.compare(got, ref, kind, label, device_noise, self.table)
        except AssertionError as e:
            self.bad.append(str(e))

    def require(self, ok, what):
        if not ok:
            self.bad.append(what)

    def finish(self):
        lines = ap.format_table(self.table)
        path = os.environ.get("DDRL_ACTING_TABLE")
        if path and lines:
            with open(path, "a") as f:
                f.write("\n".join(lines) + "\n")
        assert not self.bad, "\n".join(self.bad + ["measured:"] + lines)


def make_actor(case, params, index=0):
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters(obs_dim=case.obs, act_dim=case.act, act_scale=case.act_scale)
    opt.hidden_sizes, opt.seed = case.hid, case.seed
    actor = Actor(opt, max_rows=case.rows, index=index)
    _set(actor, params)
    return actor


def _set(actor, params):
    assert list(params.keys()) == actor.keys
    actor.set_weights(list(params.keys()), list(params.values()))


def _weights_equal(actor, params):
    keys, vals = actor.get_weights()
    return keys == list(params.keys()) and all(np.array_equal(v, params[k]) for k, v in zip(keys, vals))


def _one_launch(ck, case, actor, params, obs, rows, ref_det, tag=""):
    """Actor.get_action on single rows: noise from the counter inside the kernel, then deterministic."""
    path = "one-launch" if case.act <= 4 else "one-launch-fallback"
    for r in rows:
        ctr = actor._noise_ctr
        got = actor.get_action(obs[r])
        ck.require(actor._noise_ctr == ctr + case.act, "%s: noise counter after get_action" % case.id)
        eps = ap.device_noise(actor._noise_seed, ctr, 1, case.act)
        ck.compare(got, ap.actor_reference(case, [params], None, obs[r:r + 1], eps), "pi", "%s %s%s row %d" % (case.id, path, tag, r), device_noise=True)
        ck.compare(actor.get_action(obs[r], deterministic=True), ref_det.rows(slice(r, r + 1)), "mu", "%s %s%s row %d" % (case.id, path, tag, r))
    ck.require(getattr(actor, "_act_one", True) is (case.act <= 4), "%s: get_action took the %s path" % (case.id, "batched" if case.act <= 4 else "one-launch"))


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_acting_parity(ddrl, monkeypatch, case):
    ck = _Checks()
    obs, eps = ap.make_inputs(case)
    versions = [ap.make_params(case, v) for v in range(case.n_versions)]
    ref = ap.case_reference(case)
    actor = make_actor(case, versions[0])
    assert _weights_equal(actor, versions[0])
    n_all = case.rows

    # ---- row-major: the whole input set, then the row counts of the case, then short calls straight after the longest one
    counts = [n_all] + [n for n in case.row_counts if n != n_all]
    if case.row_counts:
        counts += [max(case.row_counts), 5, 1]
    for i, n in enumerate(counts):
        sub = ref.rows(slice(0, n))
        label = "%s row-major n=%d%s" % (case.id, n, " (after n=%d)" % counts[i - 1] if i and counts[i - 1] > n else "")
        pi = actor.get_actions(obs[:n], eps=eps[:n])
        mu = actor.get_actions(obs[:n], deterministic=True)
        ck.compare(pi, sub, "pi", label)
        ck.compare(mu, sub, "mu", label)
        if case.edge == "logstd-low":     # std = exp(-20): the sampled action is the deterministic one
            ck.require(float((pi - mu).abs().max()) <= ap.bars(sub, "mu")[1], "%s: sampled != deterministic at std 2e-9" % label)
    n = min(n_all, 37)
    ctr = actor._noise_ctr
    got = actor.get_actions(obs[:n])                                # eps=None: drawn on the device from the actor's counter
    ck.require(actor._noise_ctr == ctr + n * case.act, "%s: noise counter after get_actions(eps=None)" % case.id)
    ck.compare(got, ap.actor_reference(case, [versions[0]], None, obs[:n], ap.device_noise(actor._noise_seed, ctr, n, case.act)), "pi",
               "%s row-major device-noise n=%d" % (case.id, n), device_noise=True)

    # ---- one launch per row
    _one_launch(ck, case, actor, versions[0], obs, (0, 1, n_all - 1), ref)

    # ---- direct-operand forward
    if not case.direct:
        with pytest.raises(ValueError, match="version store needs the direct-operand policy"):
            actor.enable_versions(4)
        ck.finish()
        return
    if case.wg_slots is not None:
        monkeypatch.setenv("DDRL_VER_WG_SLOTS", str(case.wg_slots))
    actor.enable_versions(case.n_versions + 2)
    inst = "NS%d OCC%d" % (case.ns, case.occ)
    d_obs, d_eps = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()
    ck.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps), ref, "pi", "%s direct-plain %s" % (case.id, inst))
    ck.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, deterministic=True), ref, "mu", "%s direct-plain %s" % (case.id, inst))
    holds, masks = ap.holds_of(case)
    for v in range(1, case.n_versions):               # as the n-step rollout does: a pull, then the envs whose episode ended adopt it
        _set(actor, versions[v])
        actor.adopt_where_ended(torch.from_numpy(masks[v - 1].astype(np.uint8)))
    vref = ap.case_reference(case, versioned=True)
    label = "%s direct-versioned NS%d%s" % (case.id, case.ns, "" if case.wg_slots is None else " wg_slots=%d" % case.wg_slots)
    first = actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps).clone()
    ck.compare(first, vref, "pi", label)
    ck.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, deterministic=True), vref, "mu", label)
    ck.require(torch.equal(actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps), first), "%s: the same versioned call twice differs" % case.id)
    slots, st = actor.version_state()
    slots = slots.cpu().numpy()
    ck.require(not st["out_of_slots"] and st["newest"] == slots[masks[-1]][0], "%s: version state %r" % (case.id, st))
    ck.require(all(len(set(slots[holds == v])) == 1 for v in set(holds)) and len(set(slots)) == len(set(holds)), "%s: slots do not partition the envs as the versions do" % case.id)
    # HORIZON calls after the last set_weights every env counts as having adopted: the plain launch, the newest version for every row
    newest = ap.actor_reference(case, [versions[-1]], None, obs, eps)
    ck.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps), newest, "pi", "%s direct-plain after horizon %s" % (case.id, inst))
    ck.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, deterministic=True), newest, "mu", "%s direct-plain after horizon %s" % (case.id, inst))
    # ... and the row-major copy, rebuilt lazily from the direct-layout policy, is the newest version too
    n = min(n_all, 33)
    ck.compare(actor.get_actions(obs[:n], eps=eps[:n]), newest.rows(slice(0, n)), "pi", "%s row-major after %d set_weights n=%d" % (case.id, case.n_versions - 1, n))
    ck.require(_weights_equal(actor, versions[-1]), "%s: get_weights is not what was last set" % case.id)
    ck.finish()


# ---- interleaving --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["direct-o9a3-300x300-r64", "rows-o5a3-70x45"])
def test_interleaved_calls_see_the_weights_they_should(ddrl, case_id):
    """Host-side state decides which weights a path reads (the lazily rebuilt row-major copy of a direct actor, the freshness of the
    version plan, the steps since the last install): one fixed sequence over five weight sets; after every call the result is held to
    the oracle with the weights that call SHOULD see — the newest for the unversioned paths, the env's own for the versioned one."""
    case = [c for c in ap.CASES if c.id == case_id][0]
    ck = _Checks()
    obs, eps = ap.make_inputs(case)
    W = [ap.make_params(case, v) for v in range(5)]
    actor = make_actor(case, W[0])
    d_obs, d_eps = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()
    state = {"newest": 0, "holds": np.zeros(case.rows, int), "step": 0}
    far = 1000          # horizon_steps: far away, so that the versioned launch runs until the last op asks for the takeover

    def tag(what):
        state["step"] += 1
        return "%s interleaved #%02d %s (newest %d)" % (case.id, state["step"], what, state["newest"])

    def op_set(v):
        _set(actor, W[v])
        state["newest"] = v

    def op_weights():
        ck.require(_weights_equal(actor, W[state["newest"]]), tag("get_weights") + ": not bit-equal to what was last set")

    def op_rows(n, det=False):
        ref = ap.actor_reference(case, [W[state["newest"]]], None, obs[:n], eps[:n])
        ck.compare(actor.get_actions(obs[:n], deterministic=det, eps=None if det else eps[:n]), ref, "mu" if det else "pi", tag("get_actions n=%d" % n))

    def op_one(r):
        ctr = actor._noise_ctr
        got = actor.get_action(obs[r])
        ref = ap.actor_reference(case, [W[state["newest"]]], None, obs[r:r + 1], ap.device_noise(actor._noise_seed, ctr, 1, case.act))
        ck.compare(got, ref, "pi", tag("get_action row %d" % r), device_noise=True)

    def op_versioned(det=False, horizon=far, plain=False):
        holds = np.full(case.rows, state["newest"]) if plain else state["holds"]
        ref = ap.actor_reference(case, W, holds, obs, eps)
        got = actor.get_actions_versioned(d_obs, horizon, deterministic=det, eps=None if det else d_eps)
        ck.compare(got, ref, "mu" if det else "pi", tag("get_actions_versioned%s" % (" (plain launch)" if plain else "")))

    def op_adopt(rows):
        m = np.zeros(case.rows, np.uint8)
        m[rows] = 1
        actor.adopt_where_ended(torch.from_numpy(m))
        state["holds"][m.astype(bool)] = state["newest"]

    op_weights(); op_rows(5); op_one(0); op_rows(case.rows, det=True)
    if case.direct:
        actor.enable_versions(8)
        op_versioned(plain=True)                      # nothing installed since the store was enabled: the plain launch
    op_set(1); op_weights(); op_one(3); op_rows(17)
    if case.direct:
        op_versioned()                                # nobody has adopted version 1: every env still acts on version 0
        op_adopt(slice(0, 33)); op_versioned(det=True); op_rows(3)
    op_set(2); op_rows(4, det=True)
    if case.direct:
        op_versioned(); op_adopt(slice(20, 21)); op_versioned(); op_one(5)
    op_set(3); op_set(4); op_weights(); op_one(case.rows - 1)        # version 3 is superseded before anybody sees it
    if case.direct:
        op_adopt(slice(40, 64)); op_versioned(); op_weights(); op_rows(33); op_versioned(det=True)
        ck.require(len(set(state["holds"])) == 4, "the sequence leaves four live versions")
        op_versioned(horizon=1, plain=True)           # one step after the install with a horizon of one: the plain launch, newest weights
    op_rows(1); op_weights()
    ck.finish()


# ---- the fused rollout step on the two-per-CU forward ------------------------------------------------------------------------------------
def test_fused_rollout_step_on_the_occ2_forward_matches_the_oracles(ddrl):
    """tests/test_gpu_driver.py::test_fused_rollout_step_matches_the_unfused_sequence_and_the_oracles runs 4096 envs: a forward grid of
    exactly 256, the one-workgroup-per-CU instantiation.  4128 envs put the forward on k_actor_fwd<5, 2>; the same oracle comparison
    (actions against the float64 policy with the step's own noise, the env transition bit-exact given the GPU's actions), and the bars
    of this file on top."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import RolloutDevice
    from oracle.env_oracle import LanderOracle
    n = 4128
    assert (n // 32) * 2 > 256
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed = n, -1, 40, 11
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferSAC1(8, 2, 3 * n + 100, seed=0)
    fused = RolloutDevice(ps, rb, opt)
    assert fused._fused_ready()
    ora = LanderOracle(n, seed=opt.seed, max_ep_len=opt.max_ep_len)
    cfg = so.Config()
    params = {k: v for k, v in zip(keys, vals) if "/pi/" in k}
    case = ap.Case("fused-rollout-o8a2-400x300-r4128", 8, 2, (400, 300), n, True, ns=5, occ=2)
    ck = _Checks()
    for t in range(3):
        obs = fused.env.obs.cpu().numpy().copy()
        np.testing.assert_array_equal(obs, ora.obs())
        ctr = fused.actor._noise_ctr
        fused.step()
        act = fused.act.cpu().numpy()
        eps = torch.empty(n * 2, device="cuda")
        _lib.check(_lib.load().ddrl_normal_fill(_lib.dptr(eps), n * 2, fused.actor._noise_seed, ctr, _lib.stream_ptr()))
        eps = eps.view(n, 2).cpu().numpy()
        np.testing.assert_allclose(act, so.actor_act(cfg, dict(zip(keys, vals)), obs, eps, dtype=torch.float64), rtol=1e-5, atol=2e-6)
        ck.compare(act, ap.actor_reference(case, [params], None, obs, eps), "pi", "%s fused-rollout NS5 OCC2 step %d" % (case.id, t))
        o2, r, d, nxt, ended = ora.step(act)
        np.testing.assert_array_equal(fused.env.obs.cpu().numpy(), nxt)
        rings = rb.rings()
        rows = (t * n + np.arange(n)) % (3 * n + 100)
        for k, w in (("obs1_buf", obs), ("obs2_buf", o2), ("acts_buf", act), ("rews_buf", r), ("done_buf", d)):
            np.testing.assert_array_equal(rings[k].cpu().numpy()[rows], np.asarray(w, np.float32), err_msg="%s step %d" % (k, t))
    ck.finish()


# ---- discrete learners' acting ---------------------------------------------------------------------------------------------------------
def _q_actor(case, max_rows=None):
    from distributed_drl_amd import dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = case.obs, case.act, list(case.hid), 0.99, 1e-3, 0.995, case.batch, case.seed, case.alpha
    actor = (dqn.ActorSQN if case.family == "sqn" else dqn.Actor)(Opt, "worker", max_rows=case.batch if max_rows is None else max_rows)
    params = ap.q_params(case)
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


@pytest.mark.parametrize("case", ap.Q_CASES, ids=repr)
def test_q_rows_and_actions(ddrl, case):
    ck = _Checks()
    actor, params = _q_actor(case)
    obs = ap.q_inputs(case)
    ref = ap.q_case_reference(case)
    path = "wide" if case.obs >= 1024 else "narrow"
    B = case.batch
    for n in (B, 1, 2, B - 1, B):        # the short calls come after a full one: the rows beyond n hold the previous call's observations
        ck.compare(actor.q_values(obs[:n]), ref.rows(slice(0, n)), "q1", "%s q_values (%s) n=%d" % (case.id, path, n))
    ck.compare(actor.q_values(obs[B - 2:]), ref.rows(slice(B - 2, B)), "q1", "%s q_values (%s) last two rows" % (case.id, path))
    for r in (0, B - 1):
        ck.compare(actor._q_row(obs[r]).copy(), ref.rows(slice(r, r + 1)), "q1", "%s _q_row (%s) row %d" % (case.id, path, r))
    # the actions: on the rows whose float64 top-two gap clears twice the element bar the argmax is the oracle's
    rows, best = ap.argmax_rows(ref)
    rs = np.random.RandomState(case.seed)              # the actors' own generator, replayed (dqn.Actor / ActorSQN: RandomState(opt.seed))
    for r in rows:
        if case.family == "sqn":
            ck.require(actor.get_action(obs[r], deterministic=True) == best[r], "%s: deterministic action of row %d is not argmax q1" % (case.id, r))
            want = ap.sqn_sample(ref.x64["q1"][r], case.alpha, rs)
            ck.require(actor.get_action(obs[r]) == want, "%s: sampled action of row %d is not the draw from softmax(q1 / alpha)" % (case.id, r))
        else:
            want = int(best[r]) if rs.uniform() < 0.97 else int(rs.randint(0, case.act))
            ck.require(actor.get_action(obs[r]) == want, "%s: action of row %d" % (case.id, r))
    if case.family == "sqn":
        ck.require((np.argmax(ref.x64["q2"], axis=1)[rows] != best[rows]).any(), "%s: q2 would have passed the argmax check" % case.id)
    ck.finish()


# ---- acting does not disturb learning -----------------------------------------------------------------------------------------------------
def _codes():
    from distributed_drl_amd import _lib
    return (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)


@pytest.mark.parametrize("case_id", ["ddqn-ragged", "sqn-aligned", "ddqn-wide-1028"])
def test_acting_between_updates_leaves_the_discrete_learners_unchanged(ddrl, case_id):
    """ddrl_dqn_q copies its observations into the learner's own input image (rows beyond n keep the previous batch): train, train must
    equal train, q_values(n < batch), get_action, train bit for bit in main / target / m / v."""
    case = [c for c in ap.Q_CASES if c.id == case_id][0]
    cfg = ap.q_cfg(case)
    batches = [do.synthetic_batch(cfg, 500 + i) for i in range(3)]
    obs = ap.q_inputs(case, 1)
    out = []
    for acting in (False, True):
        learner, _ = _q_actor(case)
        learner.train(batches[0], 0)
        if acting:
            learner.q_values(obs[:case.batch // 2])
            learner.get_action(obs[0])
            learner.q_values(obs[:1])
        learner.train(batches[1], 1)
        if acting:
            learner._q_row(obs[3])
        learner.train(batches[2], 2)
        out.append([learner.export(c).clone() for c in _codes()])
    for name, a, b in zip(("main", "target", "m", "v"), *out):
        assert torch.equal(a, b), "%s: %s differs when the learner acts between its updates (max |diff| %.3e)" % (case.id, name, (a - b).abs().max().item())
    assert not torch.equal(out[0][0], torch.from_numpy(so.flatten(ap.q_params(case))).cuda())        # the updates did move main


def test_acting_between_updates_leaves_the_sac_learner_unchanged(ddrl):
    """A Learner with an Actor on the same device that pulls its weights and acts between the updates."""
    from distributed_drl_amd.agent import Actor, HyperParameters, Learner
    opt = HyperParameters(obs_dim=8, act_dim=2)
    opt.hidden_sizes, opt.batch_size, opt.seed = (64, 48), 37, 3
    cfg = so.Config(obs_dim=8, act_dim=2, hidden1=64, hidden2=48, batch=37)
    feeds = [so.synthetic_batch(cfg, seed=600 + i) for i in range(3)]
    rs = np.random.RandomState(1)
    obs = rs.randn(32, 8).astype(np.float32)
    out = []
    for acting in (False, True):
        learner = Learner(opt)
        actor = Actor(opt, max_rows=32) if acting else None
        for b, eps in feeds:
            learner.train(b, eps=eps)
            if acting:
                keys, vals = learner.get_weights()
                actor.set_weights(keys, vals)
                actor.get_actions(obs)
                actor.get_action(obs[0])
                actor.get_actions(obs[:5], deterministic=True)
        out.append([learner.export(c).clone() for c in _codes()])
    for name, a, b in zip(("main", "target", "m", "v"), *out):
        assert torch.equal(a, b), "%s differs when an actor acts between the updates (max |diff| %.3e)" % (name, (a - b).abs().max().item())
