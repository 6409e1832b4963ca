"""Acting-path parity with the float64 oracles: ONE case list and ONE comparison, shared by the CPU half
(tests/test_oracle_acting_parity.py: the bars are shown to see planted defects, with the oracles alone) and the GPU half
(tests/test_gpu_acting.py: every policy / Q forward of the HIP build is held to those bars).

REFERENCE   oracle/sac1_oracle.py::actor_forward (policy() in float64) for the SAC actor, oracle/dqn_oracle.py's main-network forward
            in float64 for the q rows (q1 for Double-DQN, q1 and q2 for soft-Q).  A versioned call is held row by row to the oracle
            evaluated with THAT row's version, never to another kernel.

YARDSTICK   from the oracle alone.  The float32 oracle is evaluated P = 8 times with the hidden units of both layers permuted (kernel
            columns, bias and the next layer's rows together: the same function, another float32 summation order) and once as it
            stands; with d_p = |x32_p - x64| on the elements of the call under test

                rms(x - x64)  <=  K * max_p rms(d_p)  +  2^-22 * max |x64|          K = 2
                max|x - x64|  <=  K * max_p max(d_p)  +  2^-22 * max |x64|

            K and the resolution term are tests/_state_parity.py's.  No absolute tolerance is written anywhere: both bars are
            computed at test time, on the rows of the call that is compared.

DEVICE NOISE  Where the device draws the noise itself (get_action as one launch, get_actions(eps=None)) the oracle is fed
            oracle/noise_oracle.normal_fill at the same seed and counter, and the ELEMENT bar gets
            act_scale * std64 * (2e-5 |eps| + 2e-6) on top: the tolerance tests/test_gpu_replay.py grants the generator
            (rtol 2e-5, atol 2e-6), through u = mu + eps * std, |d tanh| <= 1 and the action scale.  The rms bar stays as above.

SENSITIVITY (a cap on the inputs, checked on the CPU for every case) A saturated output hides a wrong pre-activation: outside the
            three edges that saturate on purpose (SATURATING) at least 90 % of a case's action elements have 1 - a64^2 >= 0.1, and
            at least 90 % of the q rows an argmax check looks at have a float64 top-two gap above twice the element bar."""
from collections import OrderedDict

import numpy as np
import torch

import _state_parity as sp
from oracle import dqn_oracle as do
from oracle import noise_oracle as no
from oracle import sac1_oracle as so

K = 2.0
P = 8
RESOLUTION = 2.0 ** -22
SENSITIVE_SHARE = 0.90
SENSITIVE_MIN = 0.1          # 1 - a64^2
VACUOUS_SHARE = 0.01         # element bar / rms |x64| on every non-saturating case
SATURATING = ("saturated", "logstd-high", "obsx1e3")
HORIZON = 3                  # horizon_steps of the versioned calls: the fourth call after a set_weights is the plain launch


class Case:
    """One SAC actor: shape, rows of its input set (= max_rows of the actor), the edge its parameters / inputs are put on, how many
    policy versions its versioned call spreads the rows over and how (`groups`: rows that adopt version 1, 2, ... in turn; None: every
    third row adopts each new version), the row counts get_actions is called with, DDRL_VER_WG_SLOTS."""

    def __init__(self, id, obs, act, hid, rows, direct, act_scale=1.0, edge=None, seed=5, n_versions=2, groups=None, row_counts=(),
                 wg_slots=None, ns=None, occ=None):
        self.id, self.obs, self.act, self.hid, self.rows, self.direct = id, obs, act, tuple(hid), rows, direct
        self.act_scale, self.edge, self.seed, self.n_versions, self.groups = act_scale, edge, seed, n_versions, groups
        self.row_counts, self.wg_slots, self.ns, self.occ = tuple(row_counts), wg_slots, ns, occ

    def __repr__(self):
        return self.id


ROW_COUNTS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 37, 4096, 4128)      # 4128 = max_rows of the case that carries them

# `ns` / `occ`: the k_actor_fwd<NS, OCC> instantiation the plain direct-operand launch of the case takes (NS from obs_dim, OCC = 2 when
# rows / 32 * ceil(column tiles / 5) > 256); the versioned launch is <NS, 2, versioned> always.  The GPU half writes them into its table.
# NS = 7 is instantiated in csrc/actor.hip but cannot be reached: it needs obs_dim = 12, and the direct-operand envelope (direct_ok:
# obs_dim + act_dim <= 12 with act_dim >= 1) ends at obs_dim = 11.  The instantiations are left in place, as they were when the actor
# lived in csrc/sac1.hip (one of the sources profiles/traffic.json is keyed to, where even a comment asks for a new profiling round).
def forward_instantiation(obs, hid, rows):
    """(NS, OCC) of the plain direct-operand launch, as ddrl_actor_internal_forward picks them."""
    d1 = obs + 1
    ns = 4 if d1 <= 8 else 4 + (d1 - 8 + 1) // 2
    groups = ((hid[1] + 31) // 32 + 4) // 5
    return ns, 2 if rows // 32 * groups > 256 else 1


SHAPE_CASES = [
    # inside the direct-operand envelope: obs 1 .. 11 (NS 4, 5, 6), act 1 .. 4, 1 / 3 / 10 / 16 column tiles, hidden1 at and off 32 k
    Case("direct-o8a2-400x300-r4096", 8, 2, (400, 300), 4096, True, ns=5, occ=1),
    Case("direct-o8a2-400x300-r4128", 8, 2, (400, 300), 4128, True, ns=5, occ=2, row_counts=ROW_COUNTS, seed=6),
    Case("direct-o1a1-36x8-r8224", 1, 1, (36, 8), 8224, True, ns=4, occ=2),
    Case("direct-o7a4-512x512-r96", 7, 4, (512, 512), 96, True, ns=4, occ=1),
    Case("direct-o9a3-300x300-r64", 9, 3, (300, 300), 64, True, ns=5, occ=1),
    Case("direct-o10a2-64x512-r2080", 10, 2, (64, 512), 2080, True, ns=6, occ=2),
    Case("direct-o11a1-128x96-r32", 11, 1, (128, 96), 32, True, ns=6, occ=1),
    # outside it (the row-major kernels only; enable_versions refuses): hidden sizes off 4 k, act 5 and 8 (get_action falls back to the
    # batched kernels there), obs 30, obs + act = 40
    Case("rows-o5a3-70x45", 5, 3, (70, 45), 64, False, row_counts=(1, 3, 5, 17, 64)),
    Case("rows-o1a1-7x9", 1, 1, (7, 9), 64, False),
    Case("rows-o36a4-130x70", 36, 4, (130, 70), 64, False),
    Case("rows-o9a5-64x40", 9, 5, (64, 40), 37, False),
    Case("rows-o30a8-72x44", 30, 8, (72, 44), 37, False),
]

# >= 3 live versions with distinct random weights; groups of 1, 31, 32 and 33 envs, a version nobody adopts (its slot is handed to the
# next one) and slots that stay empty; 160 rows = 1 + 31 + 32 + 33 + 63 that stay on version 0
_GROUPS = ((0, 1), None, (1, 32), (32, 64), (64, 97))          # [start, end) of the rows that adopt version 1, 2 (nobody), 3, 4, 5
VERSION_CASES = [
    Case("versions-o8a2-400x300-r160", 8, 2, (400, 300), 160, True, n_versions=6, groups=_GROUPS, ns=5, occ=1, seed=7),
    Case("versions-o10a2-64x512-r160-wg24", 10, 2, (64, 512), 160, True, n_versions=6, groups=_GROUPS, wg_slots=24, ns=6, occ=1, seed=8),
]

_D = dict(obs=5, act=3, hid=(72, 44), rows=64, direct=True, ns=4, occ=1)       # direct-operand
_R = dict(obs=9, act=5, hid=(70, 45), rows=37, direct=False)                   # row-major only (and get_action's fallback)
EDGES = ("saturated", "logstd-low", "logstd-high", "dead", "zero-obs", "obsx1e3", "eps-tail", "act-scale-2")
EDGE_CASES = [Case("%s-%s" % (e, "direct" if s is _D else "rows"), edge=e, act_scale=2.0 if e == "act-scale-2" else 1.0, seed=9 + i, **s)
              for i, e in enumerate(EDGES) for s in (_D, _R)]

CASES = SHAPE_CASES + VERSION_CASES + EDGE_CASES


def make_cfg(case):
    return so.Config(obs_dim=case.obs, act_dim=case.act, hidden1=case.hid[0], hidden2=case.hid[1], batch=case.rows, act_scale=case.act_scale)


def make_inputs(case):
    """(obs [rows, obs], eps [rows, act]) float32."""
    rs = np.random.RandomState(case.seed + 100)
    obs, eps = rs.randn(case.rows, case.obs).astype(np.float32), rs.randn(case.rows, case.act).astype(np.float32)
    if case.edge == "zero-obs":
        obs[:] = 0.0
    elif case.edge == "obsx1e3":
        obs *= np.float32(1e3)
    elif case.edge == "eps-tail":
        eps = np.where(rs.rand(case.rows, case.act) < 0.5, 6.0, -6.0).astype(np.float32)
    return obs, eps


def make_params(case, version=0):
    """The policy variables of version `version`: glorot kernels, NON-ZERO biases (tests/_state_parity.make_params), then the edge."""
    cfg = make_cfg(case)
    params = OrderedDict((k, v) for k, v in so.init_params(cfg, case.seed + 31 * version).items() if "/pi/" in k)
    rs = np.random.RandomState(case.seed + 10 + 31 * version)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    if case.edge == "saturated":
        # kernel AND bias of the mu head scaled (the pre-activation scales with them exactly) until |mu| >= 12 on every row
        f = so.actor_forward(cfg, params, make_inputs(case)[0], None, torch.float64)
        scale = 12.0 / np.abs(f["mu_pre"]).min()
        for k in ("main/pi/dense_2/kernel", "main/pi/dense_2/bias"):
            params[k] = (params[k].astype(np.float64) * scale).astype(np.float32)
    elif case.edge in ("logstd-low", "logstd-high"):
        params["main/pi/dense_3/bias"] = np.full(case.act, -20.0 if case.edge == "logstd-low" else 20.0, np.float32)
    elif case.edge == "dead":
        params["main/pi/dense/bias"][sp.DEAD] = sp.DEAD_BIAS
    return params


def holds_of(case):
    """The version every row acts on after the case's set_weights / adopt_where_ended sequence, and the masks of that sequence
    ([n_versions - 1] boolean arrays: masks[v - 1] = rows that adopt version v right after it is set)."""
    holds, masks = np.zeros(case.rows, int), []
    for v in range(1, case.n_versions):
        m = np.zeros(case.rows, bool)
        if case.groups is None:
            m[v % 3::3] = True
        elif case.groups[v - 1] is not None:
            m[case.groups[v - 1][0]:case.groups[v - 1][1]] = True
        holds[m] = v
        masks.append(m)
    return holds, masks


# ---- the reference and its yardstick ------------------------------------------------------------------------------------------------
def permute_policy(params, rs):
    """The same policy with the hidden units of both layers in another order."""
    p = OrderedDict(params)
    h1, h2 = params["main/pi/dense/bias"].size, params["main/pi/dense_1/bias"].size
    p1, p2 = rs.permutation(h1), rs.permutation(h2)
    p["main/pi/dense/kernel"], p["main/pi/dense/bias"] = params["main/pi/dense/kernel"][:, p1], params["main/pi/dense/bias"][p1]
    p["main/pi/dense_1/kernel"], p["main/pi/dense_1/bias"] = params["main/pi/dense_1/kernel"][p1][:, p2], params["main/pi/dense_1/bias"][p2]
    for head in ("dense_2", "dense_3"):
        p["main/pi/%s/kernel" % head] = params["main/pi/%s/kernel" % head][p2]
    return OrderedDict((k, np.ascontiguousarray(v)) for k, v in p.items())


def permute_q(params, rs, nets):
    p = OrderedDict(params)
    for q in nets:
        f = "main/%s/" % q
        p1, p2 = rs.permutation(params[f + "dense/bias"].size), rs.permutation(params[f + "dense_1/bias"].size)
        p[f + "dense/kernel"], p[f + "dense/bias"] = params[f + "dense/kernel"][:, p1], params[f + "dense/bias"][p1]
        p[f + "dense_1/kernel"], p[f + "dense_1/bias"] = params[f + "dense_1/kernel"][p1][:, p2], params[f + "dense_1/bias"][p2]
        p[f + "dense_2/kernel"] = params[f + "dense_2/kernel"][p2]
    return OrderedDict((k, np.ascontiguousarray(v)) for k, v in p.items())


def ensemble(params, permute, seed=77):
    """[params as they stand] + P permuted copies."""
    rs = np.random.RandomState(seed)
    return [params] + [permute(params, rs) for _ in range(P)]


class Ref:
    """x64[kind]: [n, width] float64; x32[kind]: [P + 1, n, width] (the float32 ensemble); SAC: std64 / eps [n, act], scale."""

    def __init__(self, x64, x32, std64=None, eps=None, scale=1.0):
        self.x64, self.x32, self.std64, self.eps, self.scale = x64, x32, std64, eps, scale

    def rows(self, idx):
        sub = lambda a: None if a is None else a[idx]
        return Ref({k: v[idx] for k, v in self.x64.items()}, {k: v[:, idx] for k, v in self.x32.items()}, sub(self.std64), sub(self.eps), self.scale)

    def noise_allowance(self):
        return self.scale * self.std64 * (2e-5 * np.abs(self.eps) + 2e-6)


def actor_reference(case, versions, holds, obs, eps):
    """Ref(kinds "pi", "mu") of `obs` / `eps` with row i evaluated by the oracle on versions[holds[i]]."""
    cfg = make_cfg(case)
    obs = np.asarray(obs, np.float32).reshape(-1, case.obs)
    n = obs.shape[0]
    eps = np.zeros((n, case.act), np.float32) if eps is None else np.asarray(eps, np.float32).reshape(n, case.act)
    holds = np.zeros(n, int) if holds is None else np.asarray(holds)
    x64 = {k: np.zeros((n, case.act)) for k in ("pi", "mu")}
    x32 = {k: np.zeros((P + 1, n, case.act)) for k in ("pi", "mu")}
    std64 = np.zeros((n, case.act))
    with sp._Threads():
        for v in sorted(set(holds.tolist())):
            r = np.nonzero(holds == v)[0]
            f = so.actor_forward(cfg, versions[v], obs[r], eps[r], torch.float64)
            std64[r] = f["std"]
            for k in x64:
                x64[k][r] = f[k]
            for j, pp in enumerate(ensemble(versions[v], permute_policy)):
                g = so.actor_forward(cfg, pp, obs[r], eps[r], torch.float32)
                for k in x32:
                    x32[k][j, r] = g[k]
    return Ref(x64, x32, std64, eps.astype(np.float64), case.act_scale)


_REFS = {}


def case_reference(case, versioned=False):
    """The reference of the case's own inputs: every row on version 0, or on the version holds_of() leaves it on."""
    key = (case.id, versioned)
    if key not in _REFS:
        if len(_REFS) > 6:
            _REFS.clear()
        obs, eps = make_inputs(case)
        versions = [make_params(case, v) for v in range(case.n_versions if versioned else 1)]
        _REFS[key] = actor_reference(case, versions, holds_of(case)[0] if versioned else None, obs, eps)
    return _REFS[key]


def device_noise(seed, counter, n, act):
    """What the device's generator yields at stream positions [counter, counter + n * act), as the oracle computes it."""
    return no.normal_fill(n * act, seed, counter).reshape(n, act)


def _rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64))))) if np.size(x) else 0.0


def bars(ref, kind, device_noise=False, k=K):
    """(rms bar, element bar [scalar, or per element with device noise], rms and max of the float32 ensemble's own deviation)."""
    x64 = ref.x64[kind]
    d = np.abs(ref.x32[kind] - x64[None])
    floor = RESOLUTION * float(np.abs(x64).max())
    rms32, max32 = max(_rms(dp) for dp in d), float(d.max())
    rms_bar, el_bar = k * rms32 + floor, k * max32 + floor
    if device_noise:
        el_bar = el_bar + ref.noise_allowance()
    return rms_bar, el_bar, rms32, max32


def compare(got, ref, kind, label, device_noise=False, table=None, k=K):
    """Holds `got` [n, width] to ref.x64[kind] with the float32 ensemble as the yardstick (module docstring).  `table`, if given,
    receives (label, kind, n, rms deviation, rms bar, max deviation, element bar at that element, float32 ensemble's rms, max)."""
    x64 = ref.x64[kind]
    got = np.asarray(got, np.float64).reshape(x64.shape)
    rms_bar, el_bar, rms32, max32 = bars(ref, kind, device_noise, k)
    if not np.isfinite(got).all():
        raise AssertionError("%s %s: acting differs from the float64 oracle: %d non-finite elements" % (label, kind, int((~np.isfinite(got)).sum())))
    d = np.abs(got - x64)
    excess = d - el_bar
    at = np.unravel_index(int(np.argmax(excess)), d.shape)
    el_at = float(el_bar[at]) if np.ndim(el_bar) else float(el_bar)
    if table is not None:
        table.append((label, kind, x64.shape[0], _rms(d), rms_bar, float(d[at]), el_at, rms32, max32))
    bad = []
    if _rms(d) > rms_bar:
        bad.append("rms deviation %.3e > bar %.3e (float32 oracles %.3e)" % (_rms(d), rms_bar, rms32))
    if excess[at] > 0:
        bad.append("element %s: |%.9g - %.9g| = %.3e > bar %.3e (float32 oracles %.3e); %d of %d elements over"
                   % (at, got[at], x64[at], d[at], el_at, max32, int((excess > 0).sum()), d.size))
    assert not bad, "%s %s: acting differs from the float64 oracle beyond %g x the float32 oracles' own deviation:\n  " % (label, kind, k) + "\n  ".join(bad)


def format_table(table):
    return ["%-58s %-3s n %5d  rms dev %.2e bar %.2e ratio %5.2f   max dev %.2e bar %.2e ratio %5.2f   f32 oracles rms %.2e max %.2e"
            % (r[0], r[1], r[2], r[3], r[4], r[3] / r[4], r[5], r[6], r[5] / r[6], r[7], r[8]) for r in table]


def sensitive_share(ref):
    """Share of the action elements (pi and mu together) with 1 - a64^2 >= SENSITIVE_MIN."""
    a = np.concatenate([ref.x64["pi"].reshape(-1), ref.x64["mu"].reshape(-1)]) / ref.scale
    return float(np.mean(1.0 - a * a >= SENSITIVE_MIN))


# ---- the float32 output path with one planted defect (CPU half) ---------------------------------------------------------------------
DEFECTS = ("last_hidden2_dropped", "last_hidden1_dropped", "relu_missing_on_one_unit", "row_reads_neighbours_obs", "row_reads_neighbours_eps",
           "head_bias_of_another_slot", "log_std_clipped", "act_scale_omitted", "deterministic_returns_sample")


def _last_live(h):
    """The last unit that is on for any row: dropping a unit that is off for every row (all rows of "zero-obs" hold the same
    observation) changes nothing and is no defect."""
    return int(torch.nonzero(h.abs().sum(0) > 0)[-1])



def forward32(cfg, params, obs, eps, defect=None, row=None, other=None):
    """policy() of oracle/sac1_oracle.py in float32, operation for operation (defect=None is bit-equal to it: checked), with ONE
    defect.  `row`: the row a row-wise defect hits (it reads row - 1's input); `other`: the policy whose head biases
    "head_bias_of_another_slot" reads.  -> dict(pi, mu) NumPy."""
    t = lambda k, p=params: torch.as_tensor(np.asarray(p["main/pi/" + k], np.float32))
    x, e = torch.as_tensor(np.asarray(obs, np.float32)).clone(), torch.as_tensor(np.asarray(eps, np.float32)).clone()
    if defect == "row_reads_neighbours_obs":
        x[row] = x[row - 1]
    if defect == "row_reads_neighbours_eps":
        e[row] = e[row - 1]
    z1 = x @ t("dense/kernel") + t("dense/bias")
    h = torch.relu(z1)
    if defect == "relu_missing_on_one_unit":       # the first unit outside _state_parity.DEAD that some row switches off
        j = [int(u) for u in torch.nonzero((z1 < 0).any(0)).reshape(-1) if not sp.DEAD.start <= int(u) < sp.DEAD.stop][0]
        h[:, j] = z1[:, j]
    if defect == "last_hidden1_dropped":
        h[:, _last_live(h)] = 0
    h = torch.relu(h @ t("dense_1/kernel") + t("dense_1/bias"))
    if defect == "last_hidden2_dropped":
        h[:, _last_live(h)] = 0
    bias_of = other if defect == "head_bias_of_another_slot" else params
    mu = h @ t("dense_2/kernel") + t("dense_2/bias", bias_of)
    log_std = h @ t("dense_3/kernel") + t("dense_3/bias", bias_of)
    if defect == "log_std_clipped":
        log_std = torch.clamp(log_std, so.LOG_STD_MIN, so.LOG_STD_MAX)
    else:
        log_std = torch.tanh(log_std)
        log_std = so.LOG_STD_MIN + 0.5 * (so.LOG_STD_MAX - so.LOG_STD_MIN) * (log_std + 1)
    std = torch.exp(log_std)
    pi = mu + e * std
    scale = 1.0 if defect == "act_scale_omitted" else cfg.act_scale
    out = dict(mu=(torch.tanh(mu) * scale).numpy(), pi=(torch.tanh(pi) * scale).numpy())
    if defect == "deterministic_returns_sample":
        out["mu"] = out["pi"]
    return out


def defect_applies(case, defect, kind):
    """Whether `defect` changes what `kind` ("pi" / "mu") of `case` should be — by the defect's definition, not by what a bar sees.
    A saturated output hides every pre-activation defect (that is what the sensitivity condition is about): on the SATURATING edges
    only the action scale could show, and none of them has one."""
    if defect == "act_scale_omitted":
        return case.act_scale != 1.0
    if case.edge in SATURATING:
        return False
    if defect == "row_reads_neighbours_obs":
        return case.edge != "zero-obs"                                  # every row holds the same observation there
    if defect in ("row_reads_neighbours_eps", "log_std_clipped"):
        # the noise is invisible at std = exp(-20), and the clip agrees with the tanh map at the ends of the range
        return kind == "pi" and case.edge not in ("logstd-low",)
    if defect == "deterministic_returns_sample":
        return kind == "mu" and case.edge != "logstd-low"
    if defect == "head_bias_of_another_slot":
        return case.n_versions > 1 and case.edge is None                # (the edge cases' versions share what the edge sets)
    return True


# ---- discrete learners --------------------------------------------------------------------------------------------------------------
class QCase:
    def __init__(self, id, family, obs, act, hid, batch, alpha=0.1, scale=1.0, seed=5):
        self.id, self.family, self.obs, self.act, self.hid, self.batch, self.alpha, self.scale, self.seed = id, family, obs, act, tuple(hid), batch, alpha, scale, seed
        self.nets = ("q1", "q2") if family == "sqn" else ("q1",)

    def __repr__(self):
        return self.id


Q_CASES = [
    QCase("ddqn-aligned", "ddqn", 8, 4, (64, 48), 64),
    QCase("ddqn-ragged", "ddqn", 11, 3, (50, 34), 37),
    QCase("sqn-aligned", "sqn", 8, 4, (128, 64), 32, alpha=0.05),
    QCase("sqn-ragged", "sqn", 6, 5, (40, 28), 50, alpha=0.2),
    # wide layer 1 (csrc/wide_l1.h): 1028, and once 28 224 with the obs / 16 scaling of tests/_state_parity.py
    QCase("ddqn-wide-1028", "ddqn", 1028, 3, (72, 40), 50),
    QCase("sqn-wide-1028", "sqn", 1028, 5, (100, 60), 33, alpha=0.2),
    QCase("ddqn-wide-28224", "ddqn", 28224, 4, (400, 300), 32, scale=1.0 / 16.0),
]
Q_DEFECTS = ("acts_on_q2", "last_row_left_over")


def q_cfg(case):
    return do.Config(obs_dim=case.obs, n_actions=case.act, hidden1=case.hid[0], hidden2=case.hid[1], batch=case.batch)


def q_params(case, version=0):
    cfg = q_cfg(case)
    params = (do.sqn_init_params if case.family == "sqn" else do.init_params)(cfg, case.seed + 31 * version)
    rs = np.random.RandomState(case.seed + 10 + 31 * version)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    return params


def q_inputs(case, which=0):
    """obs [batch, obs] float32; `which` = 1: another draw (what a previous call left in the learner's input image)."""
    return (np.random.RandomState(case.seed + 200 + which).randn(case.batch, case.obs) * case.scale).astype(np.float32)


def q_forward(case, params, obs, dtype):
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
    x = torch.as_tensor(np.asarray(obs)).to(dtype)
    return {q: do._mlp(p, "main/" + q, x).numpy() for q in case.nets}


def q_reference(case, params, obs):
    obs = np.asarray(obs, np.float32).reshape(-1, case.obs)
    with sp._Threads():
        x64 = q_forward(case, params, obs, torch.float64)
        members = [q_forward(case, pp, obs, torch.float32) for pp in ensemble(params, lambda p, rs: permute_q(p, rs, case.nets))]
    return Ref(x64, {q: np.stack([m[q] for m in members]).astype(np.float64) for q in case.nets})


_QREFS = {}


def q_case_reference(case):
    if case.id not in _QREFS:
        if len(_QREFS) > 3:
            _QREFS.clear()
        _QREFS[case.id] = q_reference(case, q_params(case), q_inputs(case))
    return _QREFS[case.id]


def argmax_rows(ref, kind="q1"):
    """(rows whose float64 top-two gap exceeds twice the element bar of the call, the float64 argmax of every row)."""
    q = ref.x64[kind]
    top = np.sort(q, axis=1)
    return np.nonzero(top[:, -1] - top[:, -2] > 2.0 * bars(ref, kind)[1])[0], np.argmax(q, axis=1)


def sqn_sample(q1_row, alpha, rs):
    """ActorSQN.get_action(deterministic=False) replayed on the CPU: a draw from softmax(q1 / alpha) with the same RandomState."""
    z = np.asarray(q1_row, np.float64) / float(alpha)
    p = np.exp(z - z.max())
    return int(rs.choice(len(p), p=p / p.sum()))
