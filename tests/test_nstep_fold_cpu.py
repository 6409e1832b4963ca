"""The n-step fold in float32 (what the device computes: tests/_nstep_fold.py) against its float64 restatement — no GPU.

Bounds, from the arithmetic alone (u = 2^-24, the float32 unit roundoff):
  * Ln == 1 with d in {0, 1}: R = 0 + 1 * r[0] and done = 1 - 1 * (1 - d[0]) are exact — the fold is the identity, bit for bit;
  * each of the Ln loop passes puts at most two roundings on the running product c (times (1 - d), times gamma: 1 - d itself is exact
    for d in {0, 1}) and c <= 1, so |done32 - done64| <= 2 Ln u; each term c_k r[k] carries the error of c_k plus its own product and sum
    roundings, so |R32 - R64| <= 2 Ln u * sum_k |c_k r[k]|;
  * fed to the float64 SAC1 oracle, the two folds give losses within 1e-6 relative — a tenth of the 1e-5 bar the learner tests hold
    the device update to.
Both folds take the learner's float32 gamma for the rounding bounds (the device has no other); the loss comparison folds the
float64 side with the configuration's double gamma, as the float64 oracle itself uses it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nstep_fold as nf  # noqa: E402

torch = pytest.importorskip("torch")

from oracle import sac1_oracle as so  # noqa: E402

U = 2.0 ** -24
GAMMA = 0.997
CASES = [(37, 3), (64, 8), (256, 8)]


def test_fold_is_the_identity_at_one_step():
    rs = np.random.RandomState(0)
    for term in ("some", "every"):
        win = nf.windows(rs, 64, 1, terminal=term)
        f = nf.fold32(win, GAMMA)
        assert f["rews"].dtype == np.float32 and f["done"].dtype == np.float32
        assert f["rews"].tobytes() == win["rews"][:, 0].tobytes()
        assert f["done"].tobytes() == win["done"][:, 0].tobytes()
        np.testing.assert_array_equal(f["obs1"], win["obs"][:, 0])
        np.testing.assert_array_equal(f["obs2"], win["obs"][:, 1])
        np.testing.assert_array_equal(f["acts"], win["acts"][:, 0])


@pytest.mark.parametrize("B,Ln", CASES)
@pytest.mark.parametrize("term", ["some", "every"])
def test_rounding_bound(B, Ln, term):
    rs = np.random.RandomState(100 * Ln + B)
    win = nf.windows(rs, B, Ln, terminal=term)
    g32 = float(np.float32(GAMMA))
    f32, f64 = nf.fold32(win, GAMMA), nf.fold64(win, g32)
    d_err = np.abs(f32["done"].astype(np.float64) - f64["done"])
    r_err = np.abs(f32["rews"].astype(np.float64) - f64["rews"])
    print("B %d Ln %d %s: max |done32 - done64| %.3g (bound %.3g), max |R32 - R64| / sum|c r| %.3g (bound %.3g)"
          % (B, Ln, term, d_err.max(), 2 * Ln * U, (r_err / nf.weighted_abs_sum(win, g32)).max(), 2 * Ln * U))
    assert (d_err <= 2 * Ln * U).all()
    assert (r_err <= 2 * Ln * U * nf.weighted_abs_sum(win, g32)).all()
    # cut at the first terminal: a row whose window holds one is done, whatever follows it
    has_term = win["done"].max(axis=1) > 0
    assert (f32["done"][has_term] == 1.0).all() and (np.abs(f32["done"][~has_term] - (1 - g32 ** (Ln - 1))) <= 2 * Ln * U).all()


@pytest.mark.parametrize("B,Ln", CASES)
def test_fold_rounding_does_not_show_in_the_losses(B, Ln):
    cfg = so.Config(batch=B, gamma=GAMMA)
    params = so.init_params(cfg, 1)
    rs = np.random.RandomState(7 * Ln + B)
    win = nf.windows(rs, B, Ln, cfg.obs_dim, cfg.act_dim, terminal="some")
    eps = [rs.randn(B, cfg.act_dim).astype(np.float32) for _ in range(3)]
    out = [so.Sac1Oracle(cfg, params, torch.float64).step(f, *eps) for f in (nf.fold32(win, GAMMA), nf.fold64(win, GAMMA))]
    for k in ("pi_loss", "q1_loss", "q2_loss"):
        a, b = float(out[0][k]), float(out[1][k])
        rel = abs(a - b) / abs(b)
        print("B %d Ln %d %s: float32 fold %.9g float64 fold %.9g rel %.3g" % (B, Ln, k, a, b, rel))
        assert rel <= 1e-6, (k, a, b)
