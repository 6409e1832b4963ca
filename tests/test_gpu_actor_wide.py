"""The wide direct-operand policy (ddrl_actor_create_wide: k_actor_fwd_wide + the wide layer-1 layout, csrc/actor_wide.h) against the
float64 oracle with tests/_acting_parity.py's bars, its envelope, and the two walker workers adopting weights per env on it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402

pytestmark = pytest.mark.gpu

_GROUPS = ((0, 1), None, (1, 32), (32, 64), (64, 97))
CASES = [
    ap.Case("wide-o24a4-400x300-r64", 24, 4, (400, 300), 64, True),
    ap.Case("wide-o24a4-64x48-r96", 24, 4, (64, 48), 96, True, seed=13),
    ap.Case("wide-o2a1-36x8-r32", 2, 1, (36, 8), 32, True, seed=7),
    ap.Case("wide-o3a1-36x8-r32", 3, 1, (36, 8), 32, True, seed=7),
    ap.Case("wide-o8a2-400x300-r64", 8, 2, (400, 300), 64, True, seed=14),
    ap.Case("wide-o12a4-128x96-r96", 12, 4, (128, 96), 96, True, seed=8),
    ap.Case("wide-o27a4-44x300-r64", 27, 4, (44, 300), 64, True, seed=15),
    ap.Case("wide-o28a4-44x300-r64", 28, 4, (44, 300), 64, True, seed=15),
    ap.Case("wide-o31a4-100x36-r32", 31, 4, (100, 36), 32, True, seed=11),
    ap.Case("wide-o23a2-512x512-r2080", 23, 2, (512, 512), 2080, True, seed=10),
    ap.Case("wide-versions-o24a4-64x48-r160-wg24", 24, 4, (64, 48), 160, True, seed=12, n_versions=6, groups=_GROUPS, wg_slots=24),
]


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    torch.cuda.set_device(0)
    return d


def make_actor(case, params):
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters(obs_dim=case.obs, act_dim=case.act, act_scale=case.act_scale)
    opt.hidden_sizes, opt.seed, opt.wide_policy = case.hid, case.seed, True
    actor = Actor(opt, max_rows=case.rows)
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wide_acting_parity(ddrl, monkeypatch, case):
    obs, eps = ap.make_inputs(case)
    versions = [ap.make_params(case, v) for v in range(case.n_versions)]
    ref = ap.case_reference(case)
    assert ap.sensitive_share(ref) >= ap.SENSITIVE_SHARE
    actor = make_actor(case, versions[0])
    keys, vals = actor.get_weights()
    assert keys == list(versions[0]) and all(np.array_equal(v, versions[0][k]) for k, v in zip(keys, vals))
    if case.wg_slots is not None:
        monkeypatch.setenv("DDRL_VER_WG_SLOTS", str(case.wg_slots))
    actor.enable_versions(case.n_versions + 2)
    d_obs, d_eps = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()

    def hold(r, label):                                    # three calls: stochastic with the explicit eps (twice, equal), deterministic
        first = actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps).clone()
        ap.compare(first.cpu().numpy(), r, "pi", "%s %s" % (case.id, label))
        ap.compare(actor.get_actions_versioned(d_obs, ap.HORIZON, deterministic=True).cpu().numpy(), r, "mu", "%s %s" % (case.id, label))
        assert torch.equal(actor.get_actions_versioned(d_obs, ap.HORIZON, eps=d_eps), first), "%s %s: the same call twice differs" % (case.id, label)

    hold(ref, "plain")
    holds, masks = ap.holds_of(case)
    for v in range(1, case.n_versions):                   # a pull, then the envs whose episode ended adopt it
        actor.set_weights(list(versions[v].keys()), list(versions[v].values()))
        actor.adopt_where_ended(torch.from_numpy(masks[v - 1].astype(np.uint8)))
    hold(ap.case_reference(case, versioned=True), "versioned")     # ap.HORIZON = 3 calls behind the last install ...
    newest = ap.actor_reference(case, [versions[-1]], None, obs, eps)
    hold(newest, "plain after the horizon")                        # ... the plain launch: every row on the newest version
    got = actor.get_actions(obs[:33], eps=eps[:33]).cpu().numpy()     # the row-major copy, rebuilt from the wide layout
    ap.compare(got, newest.rows(slice(0, min(33, case.rows))), "pi", "%s row-major after %d set_weights" % (case.id, case.n_versions - 1))
    slots, st = actor.version_state()
    slots = slots.cpu().numpy()
    assert not st["out_of_slots"] and all(len(set(slots[holds == v])) == 1 for v in set(holds)) and len(set(slots)) == len(set(holds)), st


def test_envelope(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLander
    lib, reasons = _lib.load(), set()
    for obs, act, hid, rows in ((32, 4, (64, 48), 32), (24, 5, (64, 48), 32), (24, 4, (50, 34), 32), (24, 4, (64, 48), 33)):
        cfg, h = _lib.Sac1Config(obs_dim=obs, act_dim=act, hidden1=hid[0], hidden2=hid[1]), ctypes.c_void_p()
        assert lib.ddrl_actor_create_wide(ctypes.byref(h), 0, ctypes.byref(cfg), rows) == _lib.DDRL_ERR_UNSUPPORTED and not h.value
        reasons.add(lib.ddrl_last_error().decode())
    assert len(reasons) == 4 and all(r.startswith("ddrl_actor_create_wide: ") for r in reasons), reasons
    actor = make_actor(ap.Case("wide-o8a2", 8, 2, (64, 48), 32, True), ap.make_params(ap.Case("wide-o8a2", 8, 2, (64, 48), 32, True)))
    env = VecLunarLander(32, seed=1)
    with pytest.raises(ValueError, match="no direct-operand policy"):
        _lib.check(lib.ddrl_rollout_begin(env._h, actor._h, _lib.stream_ptr()))


EPLEN = 10      # state row of the per-env episode length (tests/walker_oracle.py)


def walker_worker(ddrl, name):
    """(worker, parameter server, its keys and initial values): 32 walker envs, hidden (64, 48), 8 / 3 iterations, no env noise, the
    policy phase (and the n-step worker's _learning) from the first step.  Episodes last 8 vector steps and the envs start at
    lengths 0..7 (set_state), so four of them end in every step."""
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters(obs_dim=24, act_dim=4)
    opt.hidden_sizes, opt.num_envs, opt.seed, opt.start_steps, opt.wide_policy = (64, 48), 32, 3, -1, True
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "walker", 8, 3
    opt.obs_noise, opt.act_noise, opt.reward_scale, opt.Ln, opt.save_freq = 0.0, 0.0, 5, 4, 1
    opt.max_ep_len, opt.action_repeat, opt.buffer_size, opt.batch_size, opt.num_buffers = 8, 1, 600, 8, 1
    keys, vals = Actor(opt, max_rows=32).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferNStep(opt) if name == "RolloutDeviceNStep" else ddrl.ReplayBufferSAC1(24, 4, opt.buffer_size, seed=0)
    w = getattr(ddrl, name)(ps, rb, opt)
    st = w.env.get_state()
    st[EPLEN] = (torch.arange(32, device="cuda") % 8).float()
    w.env.set_state(st)
    return w, ps, keys, vals


@pytest.mark.parametrize("name", ["RolloutDeviceNStep", "RolloutDevice"])
def test_walker_workers_adopt_per_env(ddrl, name):
    w, ps, keys, vals = walker_worker(ddrl, name)
    assert w._versions is True
    for _ in range(3):
        w.step()
    rs = np.random.RandomState(101)
    new = [v + (0.3 * rs.standard_normal(v.shape)).astype(np.float32) * (0.2 if v.ndim == 2 else 1.0) for v in vals]
    ps.push(keys, new)
    w.step()                                   # pulls at its start; the envs whose episode ends in it adopt
    assert w._fused is not True and w._versions is True
    moved = w.env.ended.cpu().numpy().astype(bool)
    assert 0 < moved.sum() < 32, moved
    slots, st = w.actor.version_state()
    slots = slots.cpu().numpy()
    assert not st["out_of_slots"] and (slots[moved] == st["newest"]).all() and len(set(slots[~moved])) == 1 and slots[~moved][0] != st["newest"], (slots, st)
    ctr = w.actor._noise_ctr
    w.step()
    obs, act = w.o.cpu().numpy(), w.act.cpu().numpy()
    case = ap.Case("walker-%s" % name, 24, 4, (64, 48), 32, True)
    noise = ap.device_noise(w.actor._noise_seed, ctr, 32, 4)
    versions = [dict(zip(keys, vals)), dict(zip(keys, new))]
    ap.compare(act, ap.actor_reference(case, versions, moved.astype(int), obs, noise), "pi", case.id, device_noise=True)
    with pytest.raises(AssertionError):        # the old weights alone do not explain the moved rows
        ap.compare(act[moved], ap.actor_reference(case, versions[:1], None, obs[moved], noise[moved]), "pi", case.id, device_noise=True)
