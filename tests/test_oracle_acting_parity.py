"""CPU half of the acting-parity tests (tests/_acting_parity.py): what the GPU half's bars can and cannot see, with the oracles alone.

  * the permutation ensemble is the same function (float64 results of the permuted networks agree to 1e-12);
  * the sensitivity condition holds for every case: outside the saturating edges >= 90 % of the action elements have
    1 - a64^2 >= 0.1, and >= 90 % of the q rows clear the argmax gap; the edge cases are the edges they name;
  * the bars are not vacuous: on every non-saturating case the element bar is <= 1 % of the float64 oracle's rms action (or q);
  * mutation check: the float32 output path with ONE planted defect (DEFECTS / Q_DEFECTS) fails the comparison on every case the
    defect applies to; the clean float32 path is bit-equal to the float32 oracle and passes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402

from oracle import sac1_oracle as so  # noqa: E402

BIG_Q = {"ddqn-wide-28224"}         # 11 M parameters: its ensemble is built once, in the bars test


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_permuted_policies_are_the_same_function(case):
    cfg, (obs, eps) = ap.make_cfg(case), ap.make_inputs(case)
    params = ap.make_params(case)
    want = so.actor_forward(cfg, params, obs, eps, torch.float64)
    for pp in ap.ensemble(params, ap.permute_policy)[1:]:
        got = so.actor_forward(cfg, pp, obs, eps, torch.float64)
        assert any((pp[k] != params[k]).any() for k in params)
        for k in ("mu_pre", "log_std"):
            # (relative to the largest pre-activation: obs x 1e3 and the scaled head of "saturated" reach 1e3 and beyond)
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
        for k in ("mu", "pi"):
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * cfg.act_scale * max(1.0, np.abs(want["mu_pre"]).max()), k


@pytest.mark.parametrize("case", [c for c in ap.Q_CASES if c.id not in BIG_Q], ids=repr)
def test_permuted_q_networks_are_the_same_function(case):
    params, obs = ap.q_params(case), ap.q_inputs(case)
    want = ap.q_forward(case, params, obs, torch.float64)
    for pp in ap.ensemble(params, lambda p, rs: ap.permute_q(p, rs, case.nets))[1:]:
        got = ap.q_forward(case, pp, obs, torch.float64)
        for q in case.nets:
            assert np.abs(got[q] - want[q]).max() <= 1e-12


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_sensitivity_condition_and_bars(case):
    for versioned in ((False, True) if case.direct else (False,)):
        ref = ap.case_reference(case, versioned)
        if case.edge not in ap.SATURATING:
            assert ap.sensitive_share(ref) >= ap.SENSITIVE_SHARE, ap.sensitive_share(ref)
        for kind in ("pi", "mu"):
            rms_bar, el_bar, rms32, max32 = ap.bars(ref, kind)
            assert rms_bar <= el_bar
            if case.edge not in ap.SATURATING:
                assert el_bar <= ap.VACUOUS_SHARE * ap._rms(ref.x64[kind]), (kind, el_bar, ap._rms(ref.x64[kind]))
            for j in range(ap.P + 1):             # every member of the ensemble passes the comparison it defines
                ap.compare(ref.x32[kind][j], ref, kind, case.id)


@pytest.mark.parametrize("case", [c for c in ap.CASES if c.row_counts], ids=repr)
def test_bars_on_the_rows_of_a_short_call(case):
    """get_actions with n rows is held to the bars of those n rows: not vacuous there either, down to one row."""
    ref = ap.case_reference(case)
    for n in case.row_counts:
        sub = ref.rows(slice(0, n))
        for kind in ("pi", "mu"):
            assert ap.bars(sub, kind)[1] <= ap.VACUOUS_SHARE * ap._rms(sub.x64[kind]), (n, kind)
            ap.compare(sub.x32[kind][0], sub, kind, case.id)


@pytest.mark.parametrize("case", ap.EDGE_CASES + ap.VERSION_CASES, ids=repr)
def test_cases_are_what_they_are_named_after(case):
    cfg, (obs, eps) = ap.make_cfg(case), ap.make_inputs(case)
    f = so.actor_forward(cfg, ap.make_params(case), obs, eps, torch.float64)
    g = so.actor_forward(cfg, ap.make_params(case), obs, eps, torch.float32)
    ref = ap.case_reference(case)
    if case.edge == "saturated":
        assert (np.abs(f["mu_pre"]) >= 10).all()
        assert (np.abs(g["mu"]) == 1.0).all() and np.isfinite(g["pi"]).all()       # float32 tanh is +-1 exactly from |u| ~ 9 on
    elif case.edge == "logstd-low":
        assert np.abs(f["log_std"] + 20).max() < 1e-12 and f["std"].max() < 2.1e-9
        rms_bar, el_bar, _, _ = ap.bars(ref, "mu")
        assert np.abs(ref.x64["pi"] - ref.x64["mu"]).max() < 0.05 * el_bar           # the sampled action IS the deterministic one (2e-9 eps against a bar of 6e-7)
    elif case.edge == "logstd-high":
        assert np.abs(f["log_std"] - 2).max() < 1e-12 and 7.38 < f["std"].min()
    elif case.edge == "dead":
        z = np.abs(obs.astype(np.float64)) @ np.abs(ap.make_params(case)["main/pi/dense/kernel"].astype(np.float64)) + ap.make_params(case)["main/pi/dense/bias"]
        assert (z[:, ap.sp.DEAD] < -20).all()
    elif case.edge == "zero-obs":
        assert not obs.any()
    elif case.edge == "obsx1e3":
        assert np.abs(obs).max() > 2e3 and np.isfinite(g["pi"]).all()
    elif case.edge == "eps-tail":
        assert (np.abs(eps) == 6).all()
    elif case.edge == "act-scale-2":
        assert cfg.act_scale == 2.0 and np.abs(f["mu"]).max() > 1.0
    else:
        holds, masks = ap.holds_of(case)
        counts = np.bincount(holds, minlength=case.n_versions)
        assert sorted(counts.tolist()) == [0, 1, 31, 32, 33, 63] and len(masks) == case.n_versions - 1
        flat = [so.flatten(ap.make_params(case, v)) for v in range(case.n_versions)]
        assert all(np.abs(flat[i] - flat[j]).max() > 0.01 for i in range(len(flat)) for j in range(i))


def _defect_inputs(case, versioned):
    """The float32 output path's arguments for the whole case: per version, the rows on it."""
    cfg, (obs, eps) = ap.make_cfg(case), ap.make_inputs(case)
    holds = ap.holds_of(case)[0] if versioned else np.zeros(case.rows, int)
    versions = [ap.make_params(case, v) for v in range(case.n_versions if versioned else 1)]
    return cfg, obs, eps, holds, versions


def _run32(case, kind, versioned, defect, std64=None):
    cfg, obs, eps, holds, versions = _defect_inputs(case, versioned)
    out = np.zeros((case.rows, case.act), np.float32)
    if kind == "mu" and defect != "deterministic_returns_sample":
        eps = np.zeros_like(eps)                                      # a deterministic call carries no noise
    for v in sorted(set(holds.tolist())):
        r = np.nonzero(holds == v)[0]
        # a row-wise defect hits the last row of the group (the last row of a tile); its neighbour is the row before it.  For the noise
        # it is the row where the float64 oracle says the swap moves u = mu + eps * std most: the log_std map puts std between 2e-9 and
        # 7.4, and two nearly equal noise elements under a std of 1e-6 are a swap no bar could, or should, see
        row = len(r) - 1 if len(r) > 1 else None
        if defect == "row_reads_neighbours_eps" and row is not None:
            row = 1 + int(np.argmax((np.abs(eps[r][1:] - eps[r][:-1]) * std64[r][1:]).max(1)))
        d = defect
        if defect in ("row_reads_neighbours_obs", "row_reads_neighbours_eps") and (row is None or v != holds[-1]):
            d = None                                                  # ONE row of the call is hit, not one per version
        other = ap.make_params(case, v + 1) if defect == "head_bias_of_another_slot" else None
        if defect == "head_bias_of_another_slot" and v != holds[0]:
            d = None                                                  # (the first env's group reads the next slot's head biases)
        with ap.sp._Threads():
            out[r] = ap.forward32(cfg, versions[v], obs[r], eps[r], d, row, other)[kind]
    return out


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_every_planted_defect_fails_the_comparison(case):
    seen = set()
    for versioned in ((False, True) if case.direct else (False,)):
        ref = ap.case_reference(case, versioned)
        for kind in ("pi", "mu"):
            clean = _run32(case, kind, versioned, None)
            assert (clean == ref.x32[kind][0].astype(np.float32)).all()      # the defects are the only difference from the oracle
            ap.compare(clean, ref, kind, case.id)
            for defect in ap.DEFECTS:
                if not ap.defect_applies(case, defect, kind) or (defect == "head_bias_of_another_slot" and not versioned):
                    continue
                with pytest.raises(AssertionError, match="acting differs from the float64 oracle"):
                    ap.compare(_run32(case, kind, versioned, defect, ref.std64), ref, kind, "%s %s" % (case.id, defect))
                seen.add(defect)
    if case.edge is None:
        assert seen >= set(ap.DEFECTS) - {"act_scale_omitted"} - (set() if case.direct else {"head_bias_of_another_slot"}), seen
    if case.edge == "act-scale-2":
        assert "act_scale_omitted" in seen


@pytest.mark.parametrize("case", ap.Q_CASES, ids=repr)
def test_q_bars_gaps_and_defects(case):
    ref = ap.q_case_reference(case)
    other = None
    for n in (1, 2, case.batch - 1, case.batch):
        sub = ref.rows(slice(0, n))
        for q in case.nets:
            rms_bar, el_bar, _, _ = ap.bars(sub, q)
            assert el_bar <= ap.VACUOUS_SHARE * ap._rms(ref.x64[q]), (n, q, el_bar)
            for j in range(ap.P + 1):
                ap.compare(sub.x32[q][j], sub, q, case.id)
            if n == 1:
                continue
            # the last row of the call left over from a previous call (another observation in the learner's input image)
            if other is None:
                other = ap.q_forward(case, ap.q_params(case), ap.q_inputs(case, 1), torch.float32)
            stale = sub.x32[q][0].copy()
            stale[n - 1] = other[q][n - 1]
            with pytest.raises(AssertionError, match="acting differs from the float64 oracle"):
                ap.compare(stale, sub, q, case.id + " last_row_left_over")
    rows, best = ap.argmax_rows(ref)
    assert len(rows) >= ap.SENSITIVE_SHARE * case.batch, (len(rows), case.batch)
    if case.family == "sqn":
        with pytest.raises(AssertionError, match="acting differs from the float64 oracle"):
            ap.compare(ref.x32["q2"][0], ref, "q1", case.id + " acts_on_q2")
        # ... and the argmax check sees it too: q2's argmax differs from q1's on some row that clears the gap
        assert (np.argmax(ref.x64["q2"], axis=1)[rows] != best[rows]).any()


def test_device_noise_allowance_is_the_generators_tolerance():
    case = [c for c in ap.CASES if c.id == "logstd-high-direct"][0]
    ref = ap.case_reference(case)
    allow = ref.noise_allowance()
    assert allow.shape == ref.x64["pi"].shape
    np.testing.assert_allclose(allow, ref.std64 * (2e-5 * np.abs(ref.eps) + 2e-6), rtol=1e-12)
    rms_bar, el_bar, _, _ = ap.bars(ref, "pi", device_noise=True)
    rms0, el0, _, _ = ap.bars(ref, "pi")
    np.testing.assert_allclose(el_bar - el0, allow, rtol=1e-9)
    assert rms_bar == rms0                   # the generator's tolerance goes to the element bar alone
    assert ap.device_noise(3, 10, 4, 2).shape == (4, 2) and (ap.device_noise(3, 10, 4, 2).reshape(-1)[2:] == ap.device_noise(3, 12, 3, 2).reshape(-1)).all()


def test_forward_instantiations_of_the_case_list():
    """NS 4, 5, 6 and OCC 1, 2 all occur among the direct cases, as the case list says they do; NS = 7 lies outside the envelope."""
    direct = [c for c in ap.CASES if c.direct]
    for c in direct:
        assert c.obs + c.act <= 12 and c.act <= 4 and c.rows % 32 == 0 and c.hid[0] % 4 == 0 and c.hid[1] % 4 == 0
        assert ap.forward_instantiation(c.obs, c.hid, c.rows) == (c.ns, c.occ), c.id
    assert {(c.ns, c.occ) for c in direct} >= {(4, 1), (4, 2), (5, 1), (5, 2), (6, 1), (6, 2)}
    assert max(ap.forward_instantiation(o, (400, 300), 32)[0] for o in range(1, 12)) == 6 and ap.forward_instantiation(12, (400, 300), 32)[0] == 7
    for c in ap.CASES:
        if not c.direct:
            assert c.obs + c.act > 12 or c.act > 4 or c.hid[0] % 4 or c.hid[1] % 4, c.id
