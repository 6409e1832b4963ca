"""State parity of the learners with their CPU oracles: ONE comparison helper and ONE case list, shared by the CPU half
(tests/test_oracle_state_parity.py: the bars are shown to see a fault, with the oracles alone) and the GPU half
(tests/test_gpu_learner_state.py: the HIP learners are held to those bars).

compare_state(exports, o64, o32, start) compares main / target / Adam m / Adam v after the last update and the FIRST update's gradient
with the float64 oracle — per variable (every kernel and every bias of every network on its own, so a defect confined to one bias
row or one head is not averaged away) and over the whole flat vector.  The yardstick is not the code under test: it is the float32
oracle's own separation from the float64 oracle on the same case, both stepped by the test (the precedent is the 2 000-update test of
tests/test_gpu_sac1.py), in RMS — a float32 maximum is set by the sign flips of a few near-zero gradients (Adam's first steps are
+-lr whatever the gradient's size) and says little:

    rms(x - x64)  <=  K * rms(x32 - x64)  +  2^-22 * max |x64|          K = 2 (the long-horizon test's factor)

The second term is the float32 resolution of the tensor (two ulps of its largest element): a one-element variable on which the float32
oracle happens to round like the float64 one must not ask for more than float32 holds.

bar_over_movement() is the guard against a bar that hides the fault: every case starts from main != target (the polyak step moves
every target element by (1 - polyak) |main - target| per update, not by (1 - polyak) lr), runs >= 2 updates, and for every variable
the bar on target / main / m / v must be <= 10 % of the float64 oracle's own rms movement of that variable since the start — so a
step that never ran, ran with another coefficient, or read an operand one update stale is at least ten bars away.

Cases: CASES (the parity matrix: every kernel path of every learner, ragged and aligned, hyper-parameters off the defaults) and
EDGE_CASES (values the running loop produces and N(0,1) inputs do not)."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import dqn_oracle as do
from oracle import sac1_oracle as so
from oracle import sacv_oracle as sv

K = 2.0
GROUPS = ("grads", "main", "target", "m", "v")
MOVED = ("main", "target", "m", "v")
MOVEMENT_SHARE = 0.10
ORACLE_THREADS = 8          # small matrices: a few threads are faster than a whole host


class Case:
    def __init__(self, id, family, obs, act, hid, batch, gamma=0.997, alpha=0.1, lr=5e-5, polyak=0.995, act_scale=1.0, updates=4,
                 env=None, fused=None, edge=None, seed=5, k=K, data_seed=300):
        self.id, self.family, self.obs, self.act, self.hid, self.batch = id, family, obs, act, tuple(hid), batch
        self.gamma, self.alpha, self.lr, self.polyak, self.act_scale = gamma, alpha, lr, polyak, act_scale
        self.updates, self.env, self.fused, self.edge, self.seed, self.k, self.data_seed = updates, dict(env or {}), fused, edge, seed, k, data_seed

    def __repr__(self):
        return self.id


HYPER_H = dict(gamma=0.9, alpha=0.2, lr=1e-3, polyak=0.9, act_scale=2.0)       # hyper-parameter sets off the defaults
HYPER_I = dict(gamma=0.9, alpha=0.05, lr=1e-3, polyak=0.95, act_scale=1.0)
HYPER_J = dict(gamma=0.997, alpha=0.2, lr=5e-5, polyak=0.9, act_scale=2.0)
HYPER_Q = dict(gamma=0.9, lr=5e-5, polyak=0.9)                                 # DDQN / SQN (their defaults: 0.99, 1e-3, 0.995)
HYPER_R = dict(gamma=0.997, lr=1e-3, polyak=0.95)

CASES = [
    # SAC1, direct-operand kernels (csrc/sac1_direct.h): the headline shape, then ragged batches / tiles / action counts
    Case("sac1-direct-headline", "sac1", 8, 2, (400, 300), 256, fused=1),
    Case("sac1-direct-b37-h36x8-a1", "sac1", 5, 1, (36, 8), 37, fused=1, **HYPER_H),
    Case("sac1-direct-b1-h512x512-a4", "sac1", 8, 4, (512, 512), 1, fused=1, **HYPER_I),
    Case("sac1-direct-b37-h300x300-a3", "sac1", 8, 3, (300, 300), 37, fused=1, **HYPER_J),
    # SAC1, generic kernels (csrc/gemm_core.h), reached three ways
    Case("sac1-generic-a5", "sac1", 9, 5, (64, 40), 50, fused=0, **HYPER_H),
    Case("sac1-generic-a8-in38", "sac1", 30, 8, (72, 44), 37, fused=0, **HYPER_I),
    Case("sac1-generic-h70x45", "sac1", 5, 3, (70, 45), 37, fused=0, **HYPER_J),
    Case("sac1-generic-env-headline", "sac1", 8, 2, (400, 300), 256, fused=0, env={"DDRL_SAC1_GENERIC": "1"}, **HYPER_I),
    # SAC-v (example/model.py): direct-operand and generic
    Case("sacv-direct-b37-h64x48", "sacv", 8, 2, (64, 48), 37, fused=1, **HYPER_H),
    Case("sacv-generic-b20-h50x34", "sacv", 8, 2, (50, 34), 20, fused=0, **HYPER_I),
    # Double-DQN / soft-Q, narrow observations: aligned and ragged hidden sizes
    Case("ddqn-aligned", "ddqn", 8, 4, (64, 48), 64, **HYPER_Q),
    Case("ddqn-ragged", "ddqn", 11, 3, (50, 34), 37, **HYPER_R),
    Case("sqn-aligned", "sqn", 8, 4, (128, 64), 32, alpha=0.05, **HYPER_R),
    Case("sqn-ragged", "sqn", 6, 5, (40, 28), 50, alpha=0.2, **HYPER_Q),
    # wide layer 1 (csrc/wide_l1.h) away from 28 224
    Case("ddqn-wide-1028", "ddqn", 1028, 3, (72, 40), 50, **HYPER_Q),
    Case("sqn-wide-2500", "sqn", 2500, 5, (100, 60), 33, alpha=0.2, **HYPER_R),
    # 28 224 wide at batch 512 (config 5: the stream-K wgrad needs a batch that splits; ddrl_dqn_wide_sk tells which kernel runs): the
    # stream-K wgrad and the tile-per-workgroup one, two updates
    Case("ddqn-wide-28224-sk", "ddqn", 28224, 4, (400, 300), 512, updates=2, edge="obs/16", **HYPER_Q),
    Case("ddqn-wide-28224-nosk", "ddqn", 28224, 4, (400, 300), 512, updates=2, edge="obs/16", env={"DDRL_WIDE_SK": "0"}, **HYPER_Q),
]

_E = dict(obs=5, act=3, hid=(72, 44), batch=37, fused=1)                  # ragged, direct-operand
_G = dict(obs=9, act=5, hid=(70, 45), batch=50, fused=0)                  # generic
EDGE_CASES = [
    # (eight updates where the policy is saturated: float32 itself carries the near-zero gradients there so poorly that only then
    # the float32 oracle's deviation falls under a tenth of the parameters' movement)
    Case("sac1-saturated-direct", "sac1", edge="saturated", updates=8, **_E, **HYPER_J),
    Case("sac1-saturated-generic", "sac1", edge="saturated", updates=8, **_G, **HYPER_I),
    Case("sac1-dead-direct", "sac1", edge="dead", updates=3, **_E, **HYPER_H),
    Case("sac1-dead-generic", "sac1", edge="dead", updates=3, **_G, **HYPER_J),
    # k = 4 here, the only case off k = 2.  With rewards of +-100 the gradient of the Q heads' one-element bias is a sum of 37 terms of
    # size ~3 that cancels to ~0.3: its float32 error is set by the terms' ulp (2.4e-7), whatever the order of summation, and the
    # float32 oracle's deviation on a ONE-element variable is a single draw of that error, not an rms (its draw: 6e-8, a quarter ulp)
    Case("sac1-rew100-direct", "sac1", edge="rew100", k=4.0, **_E, **HYPER_I),
    Case("sac1-done1-generic", "sac1", edge="done1", **_G, **HYPER_H),
    Case("sac1-done0-direct", "sac1", edge="done0", **_E, **HYPER_H),
    Case("sac1-obs2same-generic", "sac1", edge="obs2same", **_G, **HYPER_J),
    Case("sac1-zerocol-direct", "sac1", edge="zerocol", **_E, **HYPER_J),
    Case("sac1-actedge-generic", "sac1", edge="actedge", **_G, **HYPER_H),
    Case("sac1-actedge-direct", "sac1", edge="actedge", **_E, **HYPER_H),
    Case("ddqn-rew100", "ddqn", 11, 3, (50, 34), 37, edge="rew100", **HYPER_Q),
    Case("sqn-done1", "sqn", 6, 5, (40, 28), 50, alpha=0.2, edge="done1", **HYPER_R),
    Case("ddqn-done0", "ddqn", 8, 4, (64, 48), 64, edge="done0", **HYPER_R),
    Case("sqn-obs2same", "sqn", 8, 4, (128, 64), 32, alpha=0.05, edge="obs2same", **HYPER_Q),
    Case("ddqn-zerocol-wide", "ddqn", 1028, 3, (72, 40), 50, edge="zerocol", **HYPER_R),
    Case("ddqn-oneaction", "ddqn", 11, 3, (50, 34), 37, edge="oneaction", **HYPER_Q),
    Case("sqn-oneaction", "sqn", 6, 5, (40, 28), 50, alpha=0.1, edge="oneaction", **HYPER_R),
]

# path equivalence off the headline shape (tests/test_gpu_learner_state.py, part C)
PATH_CASES = [Case("paths-sac1-generic", "sac1", 5, 3, (70, 45), 37, fused=0, **HYPER_H),
              Case("paths-sac1-direct-ragged", "sac1", 5, 3, (72, 44), 37, fused=1, **HYPER_J),
              Case("paths-sacv-generic", "sacv", 8, 2, (50, 34), 20, fused=0, **HYPER_I),
              # SAC-v on the direct-operand kernels (the shape of sacv-direct-b37-h64x48)
              Case("paths-sacv-direct", "sacv", 8, 2, (64, 48), 37, fused=1, **HYPER_H),
              # the smallest SAC1 shape where the q2(x, a) dgrad is cut by column tiles AND Q(x, a) is evaluated late: 8 row tiles of a
              # ragged batch x 11 column tiles = 88 tiles per dgrad (3 x 88 > 256 > 2 x 88), 10 of the 11 column tiles stay in launch
              # "bq" (bq_cols = 10 < 11), the last runs in launch "mid" beside q2's layer-2 wgrad, whose dgrad image is double-buffered
              Case("paths-sac1-direct-split", "sac1", 5, 3, (324, 36), 225, fused=1, **HYPER_J)]

DEAD = slice(8, 24)      # the block of layer-1 units switched off by the "dead" edge, in pi and in q1
DEAD_BIAS = -50.0


# ---- a case's oracle configuration, parameters, start targets and batches ----------------------------------------------------
def is_dqn(case):
    return case.family in ("ddqn", "sqn")


def make_cfg(case):
    if is_dqn(case):
        return do.Config(obs_dim=case.obs, n_actions=case.act, hidden1=case.hid[0], hidden2=case.hid[1], batch=case.batch,
                         gamma=case.gamma, lr=case.lr, polyak=case.polyak)
    return so.Config(obs_dim=case.obs, act_dim=case.act, hidden1=case.hid[0], hidden2=case.hid[1], batch=case.batch, alpha=case.alpha,
                     gamma=case.gamma, lr=case.lr, polyak=case.polyak, act_scale=case.act_scale)


def make_params(case, cfg):
    """glorot kernels, NON-ZERO biases (every term is exercised), then what the edge asks of the parameters."""
    init = {"sac1": so.init_params, "sacv": sv.init_params, "ddqn": do.init_params, "sqn": do.sqn_init_params}[case.family]
    params = init(cfg, case.seed)
    rs = np.random.RandomState(case.seed + 10)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    if case.edge == "saturated":
        # |u| > 9 before the tanh on HALF of the first batch's rows (1 - a*a rounds to 0 in float32 there; the other rows stay
        # unsaturated beside them), and the log_std head past +-10 on half of them (tanh = +-1: log_std at both ends of its range)
        obs = so.synthetic_batch(cfg, seed=case.data_seed)[0]["obs1"]
        u, ls = policy_pre_activations(params, obs)
        params["main/pi/dense_2/kernel"] = (params["main/pi/dense_2/kernel"] * (9.0 / np.median(np.abs(u).max(1)))).astype(np.float32)
        params["main/pi/dense_3/kernel"] = (params["main/pi/dense_3/kernel"] * (10.0 / np.median(np.abs(ls).max(1)))).astype(np.float32)
    if case.edge == "dead":
        for net in ("pi", "q1"):
            params["main/%s/dense/bias" % net][DEAD] = DEAD_BIAS
    return params


def offset_targets(params, seed):
    """Targets that differ from `params`: every element up to 0.08 away from its main element (an element-wise random offset, so a
    polyak step that reads another element, another variable or a stale main lands somewhere else)."""
    rs = np.random.RandomState(seed)
    return OrderedDict((k.replace("main/", "target/", 1), (v + rs.uniform(-0.08, 0.08, v.shape)).astype(np.float32)) for k, v in params.items())


def make_start_target(case, params):
    """main != target at the start of every case."""
    return offset_targets(params, case.seed + 20)


def start_from_other_targets(learner, oracles, params, seed=20):
    """For the older tests, whose learners start from set_weights (target == main: a polyak step then moves a target by
    (1 - polyak) lr at most, less than their bars): gives the learner and its oracles the same targets AWAY from main, so that every
    update moves each target element by (1 - polyak) |main - target| and their bar on the targets can see the step.
    -> the start targets (flat float32) ."""
    from distributed_drl_amd import _lib
    target = offset_targets(params, seed)
    flat = so.flatten(target)
    learner.import_(_lib.SAC1_TARGET, torch.from_numpy(flat))
    for o in oracles:
        for k, v in target.items():
            assert k in o.target
            o.target[k] = torch.tensor(v, dtype=o.dtype)
    return flat


def assert_targets_seen(o64, start_target, bar):
    """The bar on the targets is at most a tenth of what the float64 oracle's targets moved (max norm, as the bar): not blind."""
    move = np.abs(o64.flat("target") - np.asarray(start_target, np.float64)).max()
    assert bar <= 0.1 * move, (bar, move)


def make_batches(case, cfg):
    """[(batch, eps)] for every update; eps is None for the discrete learners."""
    out = []
    for it in range(case.updates):
        if is_dqn(case):
            b, eps = do.synthetic_batch(cfg, case.data_seed + it), None
        else:
            b, eps = so.synthetic_batch(cfg, seed=case.data_seed + it)
            b["acts"] = (b["acts"] * case.act_scale).astype(np.float32)
        rs = np.random.RandomState(400 + it)
        n = cfg.batch
        if case.edge == "obs/16":          # keep the K = 28 224 pre-activations O(1)
            b["obs1"], b["obs2"] = b["obs1"] / 16.0, b["obs2"] / 16.0
        elif case.edge == "rew100":        # lander-sized rewards (a landing or a crash)
            b["rews"] = np.where(rs.rand(n) < 0.5, 100.0, -100.0).astype(np.float32)
        elif case.edge == "done1":         # the backup is r alone
            b["done"] = np.ones(n, np.float32)
        elif case.edge == "done0":
            b["done"] = np.zeros(n, np.float32)
        elif case.edge == "obs2same":
            b["obs2"] = b["obs1"].copy()
        elif case.edge == "zerocol":
            b["obs1"][:, 1 % case.obs] = 0.0
            b["obs2"][:, 1 % case.obs] = 0.0
        elif case.edge == "actedge":       # actions exactly at +-act_scale
            b["acts"] = (np.where(rs.rand(n, case.act) < 0.5, 1.0, -1.0) * case.act_scale).astype(np.float32)
        elif case.edge == "oneaction":     # every row chose the same action: the other columns of the head see no gradient
            b["acts"] = np.full(n, 1.0, np.float32)
        out.append((b, eps))
    return out


def make_oracle(case, cfg, params, target, dtype, cls=None):
    if cls is not None:
        o = cls(cfg, params, dtype)
    elif case.family == "sac1":
        o = so.Sac1Oracle(cfg, params, dtype, stable=True)     # the cancellation-free form of (pi - mu) / std: the tighter float32 yardstick
    elif case.family == "sacv":
        o = sv.SacVOracle(cfg, params, dtype, stable=True)
    elif case.family == "ddqn":
        o = do.DqnOracle(cfg, params, dtype)
    else:
        o = do.SqnOracle(cfg, params, case.alpha, dtype)
    for k, v in target.items():
        assert k in o.target
        o.target[k] = torch.tensor(v, dtype=dtype)
    return o


def step_oracle(case, o, batch, eps):
    if is_dqn(case):
        return o.step(batch)
    if case.family == "sacv":
        return o.step(batch, eps[0])
    return o.step(batch, *eps)


class _Threads:
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(min(ORACLE_THREADS, self.n))

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


def run_oracle(case, dtype, cls=None, setup=None):
    """Steps one oracle through the case.  -> (oracle, [outputs of every update]); oracle.first_grads holds update 0's gradient."""
    setup = setup or make_setup(case)
    cfg, params, target, batches = setup
    with _Threads():
        o = make_oracle(case, cfg, params, target, dtype, cls)
        outs = []
        for it, (b, eps) in enumerate(batches):
            outs.append(step_oracle(case, o, b, eps))
            if it == 0:
                o.first_grads = o.flat("grads").copy()
    return o, outs


_SETUPS, _RUNS = {}, {}


def make_setup(case):
    if case.id not in _SETUPS:
        if len(_SETUPS) > 4:
            _SETUPS.clear()
        cfg = make_cfg(case)
        params = make_params(case, cfg)
        _SETUPS[case.id] = (cfg, params, make_start_target(case, params), make_batches(case, cfg))
    return _SETUPS[case.id]


def oracles(case):
    """(o64, outs64, o32, outs32) of the case, stepped once per process."""
    if case.id not in _RUNS:
        if len(_RUNS) > 4:
            _RUNS.clear()        # (the 28 224-wide cases hold 11 M parameters per tensor)
        o64, w64 = run_oracle(case, torch.float64)
        o32, w32 = run_oracle(case, torch.float32)
        _RUNS[case.id] = (o64, w64, o32, w32)
    return _RUNS[case.id]


def start_of(case):
    cfg, params, target, _ = make_setup(case)
    return {"main": so.flatten(params), "target": so.flatten(target)}


def oracle_exports(o):
    """What a learner exports, taken from an oracle (the CPU half feeds mutated float32 oracles through compare_state)."""
    out = {g: np.asarray(o.flat(g)) for g in MOVED}
    out["grads"] = np.asarray(o.first_grads)
    return out


# ---- the comparison ----------------------------------------------------------------------------------------------------------
def _variables(o64):
    off = 0
    for name, v in o64.main.items():
        n = v.numel()
        yield name, off, n
        off += n


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x, dtype=np.float64)))) if x.size else 0.0


def _reference(o64, o32, group):
    if group == "grads":
        return np.asarray(o64.first_grads, np.float64), np.asarray(o32.first_grads, np.float64)
    return o64.flat(group).astype(np.float64), o32.flat(group).astype(np.float64)


def bars(o64, o32, k=K):
    """{(group, variable or "*"): (bar, rms of the float32 oracle's deviation, float32 floor)}."""
    out = OrderedDict()
    for g in GROUPS:
        r64, r32 = _reference(o64, o32, g)
        spans = [("*", 0, r64.size)] + list(_variables(o64))
        for name, off, n in spans:
            a, b = r64[off:off + n], r32[off:off + n]
            dev, floor = _rms(b - a), 2.0 ** -22 * float(np.abs(a).max())
            out[(g, name)] = (k * dev + floor, dev, floor)
    return out


def bar_over_movement(o64, o32, start, k=K):
    """{(group, variable): bar / rms movement of the float64 oracle since the start} for main, target, m, v (m and v start at 0)."""
    out = OrderedDict()
    bb = bars(o64, o32, k)
    for g in MOVED:
        r64, _ = _reference(o64, o32, g)
        s = np.asarray(start[g], np.float64) if g in start else np.zeros_like(r64)
        for name, off, n in [("*", 0, r64.size)] + list(_variables(o64)):
            move = _rms(r64[off:off + n] - s[off:off + n])
            out[(g, name)] = bb[(g, name)][0] / move if move > 0 else float("inf")
    return out


def compare_state(exports, o64, o32, start, k=K, rows=None, per_variable=True):
    """Holds `exports` ({"main", "target", "m", "v", "grads"}: flat float32 arrays in variable order, grads = the FIRST update's)
    to the float64 oracle with the float32 oracle as the yardstick (module docstring).  Every (group, variable) is looked at before
    anything is raised; `rows`, if given, receives (group, variable, rms deviation, float32 oracle's, bar, bar / movement).
    per_variable=False holds the whole vectors only (the variables are still measured into `rows`)."""
    bb = bars(o64, o32, k)
    bm = bar_over_movement(o64, o32, start, k)
    bad = []
    for g in GROUPS:
        got = np.asarray(exports[g], np.float64).reshape(-1)
        r64, _ = _reference(o64, o32, g)
        assert got.shape == r64.shape, (g, got.shape, r64.shape)
        if not np.isfinite(got).all():
            bad.append("%s: %d non-finite elements" % (g, int((~np.isfinite(got)).sum())))
            continue
        for name, off, n in [("*", 0, r64.size)] + list(_variables(o64)):
            if name != "*" and not per_variable and rows is None:
                continue
            d = got[off:off + n] - r64[off:off + n]
            dev = _rms(d)
            bar, dev32, _ = bb[(g, name)]
            if rows is not None:
                rows.append((g, name, dev, dev32, bar, bm.get((g, name), float("nan"))))
            if dev > bar and (per_variable or name == "*"):
                bad.append("%s %s: rms deviation %.3e > bar %.3e (float32 oracle %.3e, %.1f x)" % (g, name, dev, bar, dev32, dev / max(dev32, 1e-300)))
    assert not bad, "state differs from the float64 oracle beyond %g x the float32 oracle's own deviation:\n  " % k + "\n  ".join(bad)


def format_rows(case_id, rows):
    """Per tensor group: the largest HIP / float32-oracle rms ratio over the variables (and over the whole vector), the largest
    deviation / bar, and the largest bar / movement."""
    lines = []
    for g in GROUPS:
        rr = [r for r in rows if r[0] == g]
        whole = [r for r in rr if r[1] == "*"][0]
        worst = max(rr, key=lambda r: r[2] / r[4])
        ratio_var = max((r[2] / r[3] for r in rr if r[3] > 0), default=float("nan"))
        bmv = max((r[5] for r in rr if r[5] == r[5]), default=float("nan"))
        lines.append("%-30s %-6s whole-vector hip/f32 %6.2f  worst variable hip/f32 %6.2f  worst dev/bar %5.2f (%s)  bar/movement <= %.1e"
                     % (case_id, g, whole[2] / max(whole[3], 1e-300), ratio_var, worst[2] / worst[4], worst[1], bmv))
    return lines


def losses_of(case):
    return {"sac1": ("pi_loss", "q1_loss", "q2_loss"), "sacv": ("pi_loss", "q1_loss", "q2_loss", "v_loss")}.get(case.family, ("q_loss",))


def policy_pre_activations(params, obs):
    """float64 (mu before the tanh, log_std head before the tanh) of the main policy: what the "saturated" edge is judged by."""
    f = lambda k: np.asarray(params["main/pi/" + k], np.float64)
    h = np.maximum(np.asarray(obs, np.float64) @ f("dense/kernel") + f("dense/bias"), 0)
    h = np.maximum(h @ f("dense_1/kernel") + f("dense_1/bias"), 0)
    return h @ f("dense_2/kernel") + f("dense_2/bias"), h @ f("dense_3/kernel") + f("dense_3/bias")


def dead_mask(case, cfg, group, name, off, n):
    """Elements of variable `name` that belong to the dead units (incoming kernel columns, their bias, outgoing kernel rows) in pi and
    q1 (their gradient is exactly 0), as a flat boolean mask — or None."""
    for net in ("pi", "q1"):
        h1, h2 = cfg.hidden1, cfg.hidden2
        if name == "main/%s/dense/kernel" % net:
            m = np.zeros((n // h1, h1), bool)
            m[:, DEAD] = True
            return m.reshape(-1)
        if name == "main/%s/dense/bias" % net:
            m = np.zeros(h1, bool)
            m[DEAD] = True
            return m
        if name == "main/%s/dense_1/kernel" % net:
            m = np.zeros((h1, h2), bool)
            m[DEAD, :] = True
            return m.reshape(-1)
    return None
