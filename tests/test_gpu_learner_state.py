"""Adam slots, parameters and polyak targets of the HIP learners on EVERY kernel path, against the CPU oracles.

The other GPU tests hold the state at the headline shape and at the fixture shapes; elsewhere they start from target == main (one
update then moves a target by (1 - polyak) lr: a quarter of their bar), never export m / v, and feed N(0,1) data.  Here:

  B  test_state_parity / CASES        >= 4 sequential updates (2 at 28 224-wide observations) with explicit noise, non-zero biases and
                                      main != target, on the direct-operand and the generic SAC1 kernels, SAC-v on both, Double-DQN
                                      and soft-Q narrow / wide / 28 224-wide (stream-K and tile-per-workgroup wgrad), with gamma, alpha,
                                      lr, polyak and act_scale off their defaults;
  C  test_paths_are_bit_identical     compute_gradients -> apply_gradients, the dp_stepper, the hipGraph loop (3 and 4 updates per
                                      graph) and the NumPy host-batch path == the plain train() sequence, bit for bit, on a generic
                                      shape, a ragged direct-operand shape and SAC-v's generic path;
  D  test_large_batches               512 (last direct-operand size) / 513 (first generic size) / 4 096 / 32 767 / 32 768 / 32 769 /
                                      65 535 rows, every row's q1 / q2 / logp_pi; 65 536 is refused;
  E  test_state_parity / EDGE_CASES   a saturated policy, units dead for the whole batch (bit-unchanged), rewards of +-100, done all
                                      ones / zeros, obs2 == obs1, a zero observation column, actions at +-act_scale, one action for all rows.

BARS (tests/_state_parity.py; tests/test_oracle_state_parity.py shows on the CPU that they see eight kinds of planted defect):
  state       per variable and over the whole vector, rms deviation from the float64 oracle <= 2 x the float32 oracle's own rms deviation
              + 2^-22 max |value|.  The 2 is the factor of the 2 000-update test; the float32 oracle evaluates the log-likelihood in the
              kernels' cancellation-free form (the literal form is 10^3 x further from float64).  On every case the bar is <= 10 % of
              the float64 oracle's movement of that variable (checked on the CPU).
  losses      1e-5 relative to the float64 oracle on update 0 (2e-5 at wide observations, 1e-4 at 28 224: the existing bars of
              tests/test_gpu_sac1.py), 3e-5 later (5e-5 at lr 1e-3, 1e-4 wide: the same file's) — or twice the float32 oracle's own
              deviation where that is larger (a squashed action next to +-1, rewards of +-100).
  rows        (extra to what the issue asks of B / E, and LOOSER than tests/test_gpu_sac1.py's row bars) q1 / q2 1e-4 relative + 1e-5,
              logp_pi 2e-5 + 1e-4 relative, each + 3 x the float32 oracle's own deviation on that row (tests/test_gpu_fuzz_shapes.py has
              that term for logp_pi only) and 5 x wider from update 1 on (lr 1e-3: the trajectories have separated).  In D the rows
              are held to 1e-4 relative + 1e-5 without those additions.
  paths (C)   torch.equal.
  dead units  torch.equal with the start for main, exactly 0 for m and v; targets within 1 ulp per update of the polyak of an
              unchanged main.

OBSERVED on an MI355X (profiles/state_parity_observed.txt has every tensor group's worst variable as well).  Whole-vector ratios sit at
~1: the kernels are where an independent float32 implementation is.  Single variables reach tens of x on one- and two-element biases,
where the float32 oracle's "rms" is one draw of a rounding error and the 2^-22 max |value| term carries the bar.  k = 2 everywhere but
sac1-rew100-direct (k = 4, reason at the case).  large-*: one update, whole vectors held, variables measured only.
  case                            whole-vector HIP / float32-oracle rms ratio        worst      worst bar /
                                  grads   main target      m      v              dev / bar   movement
  sac1-direct-headline             0.51   1.00   1.00   0.89   1.00               0.50     2e-04
  sac1-direct-b37-h36x8-a1         1.05   0.99   1.00   0.97   1.01               0.50     7e-05
  sac1-direct-b1-h512x512-a4       0.82   0.99   1.00   1.02   0.98               0.54     2e-04
  sac1-direct-b37-h300x300-a3      0.75   1.00   1.00   0.96   1.00               0.50     3e-04
  sac1-generic-a5                  1.02   1.00   1.00   1.00   1.00               0.50     7e-02
  sac1-generic-a8-in38             1.01   0.99   1.00   0.96   1.00               0.50     4e-05
  sac1-generic-h70x45              0.81   1.00   1.00   0.95   1.01               0.50     7e-04
  sac1-generic-env-headline        0.50   1.00   1.00   1.00   1.00               0.53     1e-04
  sacv-direct-b37-h64x48           0.84   0.99   1.00   1.00   1.00               0.50     5e-05
  sacv-generic-b20-h50x34          0.84   1.00   1.00   1.01   1.00               0.50     6e-05
  ddqn-aligned                     0.78   1.00   1.00   1.00   1.00               0.49     8e-04
  ddqn-ragged                      0.89   2.22   1.10   0.84   1.01               0.56     5e-05
  sqn-aligned                      0.83   0.88   0.99   1.01   1.00               0.49     6e-05
  sqn-ragged                       0.77   1.00   1.00   1.11   1.00               0.49     9e-04
  ddqn-wide-1028                   0.68   1.07   1.00   0.78   1.00               0.49     8e-04
  sqn-wide-2500                    0.56   1.00   1.00   1.08   0.99               0.57     6e-04
  ddqn-wide-28224-sk               1.60   1.07   1.00   1.41   1.00               0.49     7e-04
  ddqn-wide-28224-nosk             1.58   1.07   1.00   1.41   1.00               0.49     7e-04
  sac1-saturated-direct            1.00   1.00   1.00   1.00   1.00               0.50     8e-02
  sac1-saturated-generic           1.00   1.00   1.00   1.00   1.00               0.50     6e-02
  sac1-dead-direct                 0.91   1.00   1.00   0.97   1.00               0.51     5e-03
  sac1-dead-generic                0.90   1.00   1.00   1.00   0.99               0.50     1e-01
  sac1-rew100-direct               0.91   0.97   1.00   0.96   1.00               0.79     7e-05
  sac1-done1-generic               0.80   0.99   1.00   0.53   1.01               0.50     4e-05
  sac1-done0-direct                0.83   0.98   1.00   1.00   1.00               0.50     4e-05
  sac1-obs2same-generic            0.85   1.00   1.00   0.54   1.00               0.50     6e-04
  sac1-zerocol-direct              0.77   1.00   1.00   1.01   0.99               0.49     6e-04
  sac1-actedge-generic             0.79   1.00   1.00   0.87   1.00               0.51     4e-05
  sac1-actedge-direct              0.73   0.97   1.00   1.08   0.99               0.50     4e-05
  ddqn-rew100                      0.79   1.00   1.00   0.89   1.00               0.50     1e-03
  sqn-done1                        0.90   1.01   1.00   1.04   1.00               0.49     6e-05
  ddqn-done0                       0.77   1.02   1.00   1.01   0.99               0.49     4e-05
  sqn-obs2same                     0.71   1.00   1.00   0.89   1.00               0.50     8e-04
  ddqn-zerocol-wide                0.78   0.17   0.41   0.43   1.01               0.49     9e-05
  ddqn-oneaction                   0.93   1.00   1.00   0.73   1.01               0.50     1e-03
  sqn-oneaction                    0.73   1.00   1.00   1.09   1.00               0.49     7e-05
  large-512                        0.48   1.00   1.00   0.85   1.00               0.58     2e-03
  large-513                        0.63   1.00   1.00   0.81   1.02               0.51     2e-03
  large-4096                       0.41   1.00   1.00   0.61   0.96               0.88     8e-04
  large-32767                      0.42   1.00   1.00   0.43   1.03               2.62     2e-03
  large-32768                      0.47   1.00   1.00   0.50   0.94               4.18     2e-03
  large-32769                      0.46   1.00   1.00   0.50   0.99               2.85     2e-03
  large-65535                      0.61   1.00   1.00   0.58   1.16               8.83     2e-03
  large-ddqn-4096                  0.81   1.10   1.00   0.99   0.98               0.53     5e-04
Wall time, same machine, without tests/test_gpu_bench_line.py's eight-rank line: the whole GPU suite with this file 132.8 s (213 tests);
this file alone 11 s (48 tests).

DDRL_STATE_TABLE=<file>: append every case's measured ratios to that file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402

from oracle import dqn_oracle as do  # noqa: E402
from oracle import sac1_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
WHICH = ("main", "target", "m", "v")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _codes():
    from distributed_drl_amd import _lib
    return {"main": _lib.SAC1_MAIN, "target": _lib.SAC1_TARGET, "m": _lib.SAC1_ADAM_M, "v": _lib.SAC1_ADAM_V, "grads": _lib.SAC1_GRAD}


class _Args:
    """example/dsac.py's args for Model(args)."""

    def __init__(self, case):
        self.obs_dim, self.act_dim, self.ac_kwargs = case.obs, case.act, dict(hidden_sizes=list(case.hid))
        self.gamma, self.polyak, self.lr, self.alpha = case.gamma, case.polyak, case.lr, case.alpha
        self.batch_size, self.seed, self.max_ep_len, self.act_scale = case.batch, case.seed, 1000, case.act_scale


def make_learner(case, monkeypatch=None):
    """The HIP learner of a case (the environment switches of the case are set while it is created: they are read then)."""
    from distributed_drl_amd import dqn
    from distributed_drl_amd.agent import HyperParameters, Learner, Model
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    try:
        if case.family == "sac1":
            opt = HyperParameters(obs_dim=case.obs, act_dim=case.act, act_scale=case.act_scale)
            opt.hidden_sizes, opt.batch_size, opt.seed = case.hid, case.batch, case.seed
            opt.alpha, opt.gamma, opt.lr, opt.polyak = case.alpha, case.gamma, case.lr, case.polyak
            learner = Learner(opt)
        elif case.family == "sacv":
            learner = Model(_Args(case))
        else:
            class Opt:
                obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = \
                    case.obs, case.act, list(case.hid), case.gamma, case.lr, case.polyak, case.batch, case.seed, case.alpha
            learner = (dqn.LearnerSQN if case.family == "sqn" else dqn.Learner)(Opt, "learner")
    finally:
        for k in case.env:
            monkeypatch.delenv(k)
    if case.obs >= 28224:   # the pair of 28 224-wide cases is known to cover two wgrad kernels
        assert learner._lib.ddrl_dqn_wide_sk(learner._h) == (0 if case.env.get("DDRL_WIDE_SK") == "0" else 1), case.id
    if case.fused is not None:
        assert learner._lib.ddrl_sac1_is_fused(learner._h) == case.fused, "%s: expected the %s kernels" % (case.id, "direct-operand" if case.fused else "generic")
    return learner


def load_start(case, learner):
    """Parameters with non-zero biases, then targets that differ from them."""
    cfg, params, target, batches = sp.make_setup(case)
    learner.set_weights(list(params.keys()), list(params.values()))
    learner.import_(_codes()["target"], torch.from_numpy(so.flatten(target)))
    return cfg, params, target, batches


def train(case, learner, b, eps, it=0, outputs=True):
    if sp.is_dqn(case):
        return learner.train(b, it, return_outputs=outputs)
    return learner.train(b, eps=eps, return_outputs=outputs)


def exports(learner):
    c = _codes()
    return {k: learner.export(c[k]).cpu().numpy() for k in WHICH}


def _loss_bars(case, it):
    wide = case.obs >= 1024
    if it == 0:
        return 1e-4 if case.obs >= 28224 else 2e-5 if wide else 1e-5
    return 1e-4 if wide else 5e-5 if case.lr > 5e-5 else 3e-5


def _check_outputs(case, it, got, w64, w32):
    names = sp.losses_of(case)
    losses, rows = got
    losses = losses.cpu().numpy().reshape(-1)
    ref_scale = float(torch.as_tensor(w64["q1" if "q1" in w64 else "q"]).abs().mean())
    for i, k in enumerate(names):
        want, w_32 = float(w64[k]), float(w32[k])
        # a loss that is a mean of signed terms can sit near zero: relative to the terms' size then (tests/test_gpu_fuzz_shapes.py)
        scale = max(abs(want), 1e-2 * ref_scale)
        tol = max(_loss_bars(case, it) * scale, 2.0 * abs(w_32 - want))
        print("%s update %d %s: hip %.9g float64 %.9g float32 %.9g  |dev| %.2e tol %.2e" % (case.id, it, k, losses[i], want, w_32, abs(losses[i] - want), tol))
        assert np.isfinite(losses[i]) and abs(losses[i] - want) <= tol, (case.id, it, k, float(losses[i]), want, w_32)
    f = 1.0 if it == 0 else 5.0      # later updates: the float32 and float64 trajectories have separated (the existing tests' 5 x)
    if sp.is_dqn(case):
        a = 10 * _loss_bars(case, it)
        np.testing.assert_allclose(rows.cpu().numpy(), w64["q"].numpy(), rtol=a, atol=a)
        return
    q1, q2, lp = (t.cpu().numpy() for t in rows)
    y1 = np.abs(w32["q1"].numpy() - w64["q1"].numpy())
    assert (np.abs(q1 - w64["q1"].numpy()) <= f * (1e-5 + 1e-4 * np.abs(w64["q1"].numpy())) + 3.0 * y1).all()
    y2 = np.abs(w32["q2"].numpy() - w64["q2"].numpy())
    assert (np.abs(q2 - w64["q2"].numpy()) <= f * (1e-5 + 1e-4 * np.abs(w64["q2"].numpy())) + 3.0 * y2).all()
    lp64, lp32 = w64["logp_pi"].numpy(), w32["logp_pi"].numpy().astype(np.float64)
    assert np.isfinite(lp).all()
    assert (np.abs(lp - lp64) <= f * (2e-5 + 1e-4 * np.abs(lp64)) + 3.0 * np.abs(lp32 - lp64)).all(), np.abs(lp - lp64).max()


def _record(case, rows):
    lines = sp.format_rows(case.id, rows)
    print("\n".join(lines))
    path = os.environ.get("DDRL_STATE_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def _check_dead_units(case, learner, cfg, start, n_updates):
    """Units that are off for every row of every batch: a gradient of exactly 0 — Adam's m / (sqrt(v) + eps) must leave their
    weights bit-unchanged (no eps-driven creep), m = v = 0, and their targets are the polyak of an unchanged main."""
    got = exports(learner)
    off = 0
    for name, shape in so.param_specs(cfg):
        n = int(np.prod(shape))
        mask = sp.dead_mask(case, cfg, "main", name, off, n)
        if mask is not None:
            s_main, s_targ = start["main"][off:off + n][mask], start["target"][off:off + n][mask]
            assert np.array_equal(got["main"][off:off + n][mask], s_main), name
            assert not got["m"][off:off + n][mask].any() and not got["v"][off:off + n][mask].any(), name
            pk = case.polyak ** n_updates
            want = pk * s_targ.astype(np.float64) + (1.0 - pk) * s_main.astype(np.float64)
            ulp = 2.0 ** -23 * np.maximum(np.abs(s_targ), np.abs(s_main))
            assert (np.abs(got["target"][off:off + n][mask] - want) <= n_updates * ulp).all(), name
        off += n


@pytest.mark.parametrize("case", sp.CASES + sp.EDGE_CASES, ids=repr)
def test_state_parity(ddrl, monkeypatch, case):
    o64, w64, o32, w32 = sp.oracles(case)
    learner = make_learner(case, monkeypatch)
    cfg, params, target, batches = load_start(case, learner)
    start = sp.start_of(case)
    np.testing.assert_array_equal(exports(learner)["target"], start["target"])       # the import took: main != target from here on
    grads = None
    for it, (b, eps) in enumerate(batches):
        got = train(case, learner, b, eps, it)
        if it == 0:
            grads = learner.export(_codes()["grads"]).cpu().numpy()
        _check_outputs(case, it, got, w64[it], w32[it])
    ex = exports(learner)
    ex["grads"] = grads
    rows = []
    try:
        sp.compare_state(ex, o64, o32, start, case.k, rows=rows)
    finally:
        if rows:
            _record(case, rows)
    if case.edge == "dead":
        _check_dead_units(case, learner, cfg, start, case.updates)
    if not sp.is_dqn(case):
        assert learner.opt_steps() == (case.updates, case.updates)


# ---- C: path equivalence off the headline shape -------------------------------------------------------------------------------------
N_PATH_UPDATES = 7


def _state(learner):
    c = _codes()
    return [learner.export(c[k]).clone() for k in WHICH]


def _assert_same(a, b, what):
    for k, x, y in zip(WHICH, a, b):
        assert torch.equal(x, y), "%s: %s differs from the plain train() sequence (max |diff| %.3e)" % (what, k, (x - y).abs().max().item())


def _noise(learner, seed, u, B, a):
    from distributed_drl_amd import _lib
    e = torch.empty(3 * B * a, device="cuda")
    _lib.check(_lib.load().ddrl_normal_fill(_lib.dptr(e), e.numel(), seed, u * 3 * B * a, _lib.stream_ptr()))
    e = e.view(3, B, a)
    return (e[0], e[1], e[2])


@pytest.mark.parametrize("case", sp.PATH_CASES, ids=repr)
def test_paths_are_bit_identical_off_the_headline_shape(ddrl, monkeypatch, case):
    """Every way of issuing an update must leave main / target / m / v bit-identical to train(batch, eps) one at a time — on the generic
    kernels and on a ragged direct-operand shape, where tests/test_gpu_sac1.py and tests/test_gpu_driver.py (obs 8, act 2, hidden
    (400, 300), batch 256 / 100) do not look.  The hipGraph loop (workers.TrainDevice) builds an agent.Learner: it has no SAC-v form."""
    from distributed_drl_amd.workers import TrainDevice
    B, o, a = case.batch, case.obs, case.act
    cfg, params, target, _ = sp.make_setup(case)
    rs = np.random.RandomState(8)
    n = 900
    data = [rs.randn(n, o).astype(np.float32), (rs.uniform(-1, 1, (n, a)) * case.act_scale).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, o).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]

    def ring():
        rb = ddrl.ReplayBufferSAC1(o, a, 1024, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        return rb

    def fresh():
        learner = make_learner(case, monkeypatch)
        load_start(case, learner)
        return learner

    # (1) explicit batches and noise: compute_gradients -> apply_gradients (the gradient leaves and re-enters, as behind an all-reduce)
    feeds = []
    for u in range(N_PATH_UPDATES):
        b, eps = so.synthetic_batch(cfg, seed=700 + u)
        feeds.append(({k: torch.from_numpy(v).cuda() for k, v in b.items()}, [torch.from_numpy(e).cuda() for e in eps]))
    plain, split = fresh(), fresh()
    for b, eps in feeds:
        plain.train(b, eps=eps)
        split.apply_gradients(split.compute_gradients(b, eps=eps))
    _assert_same(_state(split), _state(plain), "compute_gradients -> apply_gradients")
    assert plain.opt_steps() == split.opt_steps() == (N_PATH_UPDATES, N_PATH_UPDATES)

    # (2) NumPy batches (the reference's feed): one block copy + noise from the learner's counter
    host, ref = fresh(), fresh()
    for u in range(N_PATH_UPDATES):
        b, _ = so.synthetic_batch(cfg, seed=800 + u)
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in b.items()}
        host.train(b)
        for v in b.values():
            v += 1.0                                   # the caller's arrays may change as soon as train() has returned
        ref.train(dev, eps=_noise(ref, ref._noise_seed, u, B, a))
    assert host._noise_ctr == N_PATH_UPDATES * 3 * B * a
    assert host._fast is not False, "the one-call host-batch path is not offered at this shape"
    _assert_same(_state(host), _state(ref), "host-batch path")

    # (3) the data-parallel stepper (the next batch's draw rides in this update's forward launch; every fifth update ends a step)
    rb_a, rb_b = ring(), ring()
    dp, ref = fresh(), fresh()
    grads, apply, g = dp.dp_stepper(rb_a)
    for u in range(10):
        grads(last=(u % 5 == 4))
        g.mul_(1.0)
        apply()
        ref.train(rb_b.sample_batch_device(B), eps=_noise(ref, dp._noise_seed, u, B, a))
    _assert_same(_state(dp), _state(ref), "dp_stepper")
    assert rb_a.get_counts() == rb_b.get_counts()

    # (4) the hipGraph loop, 3 and 4 updates per graph (an odd count ends on the copy node of the double-buffered optimizer state)
    if case.family != "sac1":
        # no SAC-v form of the loop: workers.TrainDevice builds an agent.Learner (SAC1) whatever options it is given.  Asserted, so
        # that this branch is looked at again when that changes.
        from distributed_drl_amd.agent import Learner, Model
        td = TrainDevice(None, ring(), plain.opt, updates_per_graph=3)
        assert type(td.agent) is Learner and not isinstance(td.agent, Model) and td.agent.VARIANT == 0
    else:
        for per_graph in (3, 4):
            rb_a, rb_b = ring(), ring()
            td = TrainDevice(None, rb_a, plain.opt, updates_per_graph=per_graph)
            assert td.agent._lib.ddrl_sac1_is_fused(td.agent._h) == case.fused
            load_start(case, td.agent)
            ref = fresh()
            n_upd = 11
            td.run(n_upd)
            for u in range(n_upd):
                ref.train(rb_b.sample_batch_device(B), eps=_noise(ref, td.noise_seed, u, B, a))
            _assert_same(_state(td.agent), _state(ref), "graph loop, %d updates per graph" % per_graph)
            assert td.agent.opt_steps() == (n_upd, n_upd) and rb_a.get_counts() == rb_b.get_counts()


# ---- D: large batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid,batch,fused", [((64, 48), 512, 1), ((64, 48), 513, 0), ((400, 300), 4096, 0), ((64, 48), 32767, 0), ((64, 48), 32768, 0),
                                             ((64, 48), 32769, 0), ((64, 48), 65535, 0)])
def test_large_batches(ddrl, monkeypatch, hid, batch, fused):
    """Nothing above 512 rows had gone through a learner: row offsets, launch-table splits and loss partials at thousands of row tiles.
    One update from the oracle's start, float64 oracle (float32 beside it for the row-wise yardstick of logp_pi): losses 1e-5 relative,
    q1 / q2 / logp_pi on EVERY row (a row-offset fault in a late tile shows there), gradients within 2e-4 of each tensor's maximum.
    Hidden (64, 48) away from 4 096 rows keeps the host's oracle step short, and at 512 / 513 rows it keeps every relu pre-activation
    of this draw further than 2^-19 of its terms from zero (at (400, 300) x 512 rows one of q1's layer-2 units sits at 3e-9 of its terms:
    no sign in float32, and one row in 512 is visible at 2e-4 — tests/test_gpu_fuzz_shapes.py, _flip_variants); the row count is what
    these cases are about.  The state is held as whole vectors here: the float32 oracle sums a bias gradient over 32 768 rows pairwise,
    so on a one- or two-element variable its own deviation is no yardstick for a sum taken in another order (measured, not asserted:
    the per-variable ratios go into the table).
    FOUND BY THIS TEST (both fixed in csrc/sac1.hip, the cases stay): (1) the direct-operand path was taken up to 32 768 rows, but a
    wgrad tile of k_dg contracts at most 512 rows — at 4 096 rows every gradient was the sum over the first 512 rows only (an eighth
    of its value; losses and per-row outputs right): 512 is the last direct-operand size now, 513 the first generic one.  (2) k_rows_c
    unpacked the row count with a signed shift: from 32 768 rows on the generic kernels it saw a negative count, skipped the policy
    backward and the loss reduction — losses 0 and a zero policy gradient."""
    case = sp.Case("large-%d" % batch, "sac1", 8, 2, hid, batch, fused=fused, updates=1)
    learner = make_learner(case, monkeypatch)
    o64, w64, o32, w32 = sp.oracles(case)
    cfg, params, target, batches = load_start(case, learner)
    b, eps = batches[0]
    losses, (q1, q2, lp) = learner.train(b, eps=eps, return_outputs=True)
    got = losses.cpu().numpy()
    w, v = w64[0], w32[0]
    bad = []                       # everything is looked at before anything is raised: which tensors are off tells where the fault is
    for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
        rel = abs(got[i] - float(w[k])) / abs(float(w[k]))
        print("batch %d %s: hip %.9g float64 %.9g float32 %.9g rel %.2e" % (batch, k, got[i], float(w[k]), float(v[k]), rel))
        if not rel <= 1e-5:
            bad.append("%s: hip %.9g float64 %.9g" % (k, got[i], float(w[k])))
    for name, x in (("q1", q1), ("q2", q2)):
        err = np.abs(x.cpu().numpy() - w[name].numpy()) - (1e-5 + 1e-4 * np.abs(w[name].numpy()))
        if not (err <= 0).all():
            bad.append("%s: %d rows off, first row %d, max excess %.3e" % (name, int((err > 0).sum()), int(np.argmax(err > 0)), err.max()))
    lp64, lp32 = w["logp_pi"].numpy(), v["logp_pi"].numpy().astype(np.float64)
    err = np.abs(lp.cpu().numpy() - lp64) - (2e-5 + 1e-4 * np.abs(lp64) + 3.0 * np.abs(lp32 - lp64))
    if not (err <= 0).all():
        bad.append("logp_pi: %d rows off, first row %d, max excess %.3e" % (int((err > 0).sum()), int(np.argmax(err > 0)), err.max()))
    g, g64 = learner.export(_codes()["grads"]).cpu().numpy(), o64.first_grads
    off = 0
    for name, shape in so.param_specs(cfg):
        n = int(np.prod(shape))
        x, y = g[off:off + n], g64[off:off + n]
        if not np.abs(x - y).max() <= 2e-4 * np.abs(y).max():
            bad.append("gradient %s: max deviation %.3e of max |g| %.3e (element %d of %d)" % (name, np.abs(x - y).max(), np.abs(y).max(), int(np.argmax(np.abs(x - y))), n))
        off += n
    rows = []
    try:
        sp.compare_state(dict(exports(learner), grads=g), o64, o32, sp.start_of(case), rows=rows, per_variable=False)
    except AssertionError as e:
        bad.append(str(e))
    if rows:
        _record(case, rows)
    assert not bad, "batch %d:\n" % batch + "\n".join(bad)


def test_batch_65536_is_refused(ddrl):
    from distributed_drl_amd.agent import HyperParameters, Learner
    opt = HyperParameters()
    opt.batch_size = 65536
    with pytest.raises(ValueError, match="batch >= 65536 unsupported"):       # (a bad argument surfaces as ValueError: _lib.check)
        Learner(opt)


def test_ddqn_large_batch(ddrl, monkeypatch):
    case = sp.Case("large-ddqn-4096", "ddqn", 8, 4, (64, 48), 4096, updates=1, gamma=0.99, lr=1e-3)
    learner = make_learner(case, monkeypatch)
    o64, w64, o32, w32 = sp.oracles(case)
    cfg, params, target, batches = load_start(case, learner)
    loss, q = learner.train(batches[0][0], 0, return_outputs=True)
    assert abs(loss.item() - float(w64[0]["q_loss"])) <= 1e-5 * abs(float(w64[0]["q_loss"])), (loss.item(), float(w64[0]["q_loss"]))
    np.testing.assert_allclose(q.cpu().numpy(), w64[0]["q"].numpy(), rtol=1e-4, atol=1e-4)
    g, g64 = learner.export(_codes()["grads"]).cpu().numpy(), o64.first_grads
    off = 0
    for name, shape in do.param_specs(cfg):
        n = int(np.prod(shape))
        assert np.abs(g[off:off + n] - g64[off:off + n]).max() <= 2e-4 * np.abs(g64[off:off + n]).max(), name
        off += n
    rows = []
    try:
        sp.compare_state(dict(exports(learner), grads=g), o64, o32, sp.start_of(case), rows=rows)
    finally:
        if rows:
            _record(case, rows)
