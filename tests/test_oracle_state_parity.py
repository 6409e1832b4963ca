"""CPU half of the state-parity tests (tests/_state_parity.py): what the GPU half's bars can and cannot see, shown with the oracles alone.

  * for every case of the parity matrix and of the value edges: the bar of compare_state on target / main / Adam m / Adam v is at most
    10 % of the float64 oracle's own movement of that variable — per variable — so a step that did not happen is ten bars away;
    the edge cases really are the edges they are named after;
  * mutation check: a float32 oracle with ONE deliberate defect, fed to compare_state in place of a learner's exports, is rejected for
    every defect of MUTANTS on three small cases; the clean float32 oracle is accepted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402

from oracle import sac1_oracle as so  # noqa: E402
from oracle import sacv_oracle as sv  # noqa: E402

BIG = {"ddqn-wide-28224-nosk"}     # same oracle run as ddqn-wide-28224-sk (the two differ in the kernel the learner picks)


@pytest.mark.parametrize("case", [c for c in sp.CASES + sp.EDGE_CASES if c.id not in BIG], ids=repr)
def test_bars_are_a_tenth_of_the_movement_or_less(case):
    """Conditions (i) and (ii): bar <= 10 % of |x_after - x_start| (rms, float64 oracle) for target, main, m and v, for the whole
    vector and for every variable; and the clean float32 oracle passes its own comparison."""
    o64, _, o32, _ = sp.oracles(case)
    start = sp.start_of(case)
    assert case.updates >= (2 if case.obs >= 28224 else 3)
    ratio = sp.bar_over_movement(o64, o32, start, case.k)
    cfg = sp.make_setup(case)[0]
    bad = {k: v for k, v in ratio.items() if not v <= sp.MOVEMENT_SHARE}
    assert not bad, bad
    sp.compare_state(sp.oracle_exports(o32), o64, o32, start, case.k)
    assert cfg.batch == case.batch


@pytest.mark.parametrize("case", [c for c in sp.EDGE_CASES if c.edge in ("saturated", "dead")], ids=repr)
def test_edge_cases_are_the_edges_they_name(case):
    cfg, params, target, batches = sp.make_setup(case)
    obs = batches[0][0]["obs1"]
    if case.edge == "saturated":
        u, ls = sp.policy_pre_activations(params, obs)
        sat = (np.abs(u) > 9).any(axis=1).mean()
        assert 0.1 <= sat <= 0.9, sat                                # a known share of rows: saturated and unsaturated rows side by side
        assert 1.0 - np.tanh(9.0) ** 2 < 2.0 ** -23                  # 1 - a*a is below float32's resolution at 1 there
        assert (ls > 10).any() and (ls < -10).any()                  # tanh reaches +1 and -1: log_std at both ends of its range
        o64, w64, o32, w32 = sp.oracles(case)
        for w in w64 + w32:
            assert all(np.isfinite(np.asarray(w[k])).all() for k in ("pi_loss", "q1_loss", "q2_loss", "logp_pi"))
    else:
        for net in ("pi", "q1"):
            f = lambda k: np.asarray(params["main/%s/%s" % (net, k)], np.float64)
            for b, eps in batches:
                x = b["obs1"] if net == "pi" else np.concatenate([b["obs1"], b["acts"]], 1)
                z = np.abs(x.astype(np.float64)) @ np.abs(f("dense/kernel")) + f("dense/bias")
                z2 = np.abs(np.concatenate([b["obs2"], np.full_like(b["acts"], case.act_scale)], 1)[:, :x.shape[1]].astype(np.float64)) @ np.abs(f("dense/kernel")) + f("dense/bias")
                assert (z[:, sp.DEAD] < -20).all() and (z2[:, sp.DEAD] < -20).all()     # off for every row, whatever the signs
        o64, _, o32, _ = sp.oracles(case)
        start = sp.start_of(case)
        for o in (o64, o32):
            off = 0
            for name, v in o.main.items():
                n = v.numel()
                m = sp.dead_mask(case, cfg, "main", name, off, n)
                if m is not None:
                    assert (o.flat("m")[off:off + n][m] == 0).all() and (o.flat("v")[off:off + n][m] == 0).all()
                    assert (o.flat("main")[off:off + n][m] == start["main"][off:off + n][m].astype(o.flat("main").dtype)).all()
                    assert m.sum() in (16 * (n // cfg.hidden1), 16, 16 * cfg.hidden2)
                off += n


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("polyak_skipped", "polyak_swapped", "polyak_pre_update_main", "one_target_stale", "v_from_g", "shared_beta_powers",
           "m_stale_last_3_columns", "eps_inside_root")


def mutant_class(base, kind):
    """`base` (Sac1Oracle / SacVOracle) with the one defect `kind`."""

    class Mutant(base):
        def __init__(self, cfg, params, dtype):
            base.__init__(self, cfg, params, dtype, stable=True)

        def _adam(self, names, which):
            if kind == "shared_beta_powers":
                which = "pi"                                  # ONE running pair: the q optimizer sees the powers the pi optimizer left
            if kind not in ("v_from_g", "eps_inside_root", "m_stale_last_3_columns"):
                return base._adam(self, names, which)
            c = self.cfg
            t = lambda x: torch.tensor(x, dtype=self.dtype)
            one = t(1.0)
            alpha_t = t(c.lr) * torch.sqrt(one - self.b2p[which]) / (one - self.b1p[which])
            for n in names:
                g = self.grads[n]
                m_before = self.m[n].clone()
                self.m[n] = self.m[n] + (g - self.m[n]) * (one - t(c.beta1))
                gg = g if kind == "v_from_g" else g * g
                self.v[n] = self.v[n] + (gg - self.v[n]) * (one - t(c.beta2))
                if kind == "eps_inside_root":
                    self.main[n] = self.main[n] - (self.m[n] * alpha_t) / torch.sqrt(self.v[n].abs() + t(c.adam_eps))
                else:
                    self.main[n] = self.main[n] - (self.m[n] * alpha_t) / (torch.sqrt(self.v[n].abs()) + t(c.adam_eps))
                if kind == "m_stale_last_3_columns" and n == "main/q1/dense_1/kernel":
                    self.m[n][:, -3:] = m_before[:, -3:]      # the slot of those columns is the previous update's
            self.b1p[which] = self.b1p[which] * t(c.beta1)
            self.b2p[which] = self.b2p[which] * t(c.beta2)

        def apply_grads(self):
            c = self.cfg
            before = {n: v.clone() for n, v in self.main.items()}
            value = self._value_names() if hasattr(self, "_value_names") else [n for n in self.names if "/q1/" in n or "/q2/" in n]
            self._adam([n for n in self.names if "/pi/" in n], "pi")
            self._adam(value, "q")
            pk, pk1 = torch.tensor(c.polyak, dtype=self.dtype), torch.tensor(1 - c.polyak, dtype=self.dtype)
            if kind == "polyak_swapped":
                pk, pk1 = pk1, pk
            for n in self.names:
                tn = n.replace("main/", "target/", 1)
                if kind == "polyak_skipped" or (kind == "one_target_stale" and n == "main/q2/dense_1/bias"):
                    continue
                src = before[n] if kind == "polyak_pre_update_main" else self.main[n]
                self.target[tn] = pk * self.target[tn] + pk1 * src

    return Mutant


MUTATION_CASES = ["sac1-direct-b37-h36x8-a1", "sac1-generic-h70x45", "sacv-generic-b20-h50x34"]


@pytest.mark.parametrize("case_id", MUTATION_CASES)
def test_compare_state_rejects_every_mutant_and_accepts_the_clean_float32_oracles(case_id):
    case = [c for c in sp.CASES if c.id == case_id][0]
    o64, _, o32, _ = sp.oracles(case)
    start = sp.start_of(case)
    base = sv.SacVOracle if case.family == "sacv" else so.Sac1Oracle
    sp.compare_state(sp.oracle_exports(o32), o64, o32, start)
    # an unmutated pass through the mutant class is the clean oracle, bit for bit: the defects are the only difference
    clean, _ = sp.run_oracle(case, torch.float32, cls=mutant_class(base, "none"))
    for g in sp.MOVED:
        assert (clean.flat(g) == o32.flat(g)).all(), g
    for kind in MUTANTS:
        mut, _ = sp.run_oracle(case, torch.float32, cls=mutant_class(base, kind))
        with pytest.raises(AssertionError, match="state differs from the float64 oracle"):
            sp.compare_state(sp.oracle_exports(mut), o64, o32, start)
