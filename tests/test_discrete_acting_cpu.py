"""The NumPy half of the discrete acting path (tests/_discrete_acting.py): the selection oracle the GPU tests hold ddrl_dqn_act and the
fused discrete rollout step to, and gym's discrete action table on the lander oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _discrete_acting as da  # noqa: E402

from oracle import env_oracle as eo  # noqa: E402

F = np.float32


def test_first_maximum_on_tied_rows():
    q = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 2.0, 2.0], [-2.0, -2.0, -3.0, -2.0]], F)
    want = np.array([1, 0, 2, 0])
    u0, u1 = np.zeros(4, F), np.full(4, 0.99, F)
    np.testing.assert_array_equal(da.first_max(q), want)
    np.testing.assert_array_equal(da.select(q, "ddqn", 0.1, 0.97, u0, u1), want)                       # u0 = 0 < greedy_prob
    np.testing.assert_array_equal(da.select(q, "sqn", 0.1, 0.97, u0, u1, deterministic=True), want)
    np.testing.assert_array_equal(da.select(q, "ddqn", 0.1, 0.97, np.full(4, 0.98, F), u1), np.full(4, 3))   # the random branch: floor(0.99 * 4)


def test_ddqn_random_share_and_range():
    n, A, g = 100000, 4, 0.97
    u0, u1 = da.uniforms(11, 5, n)
    q = np.tile(np.array([[0.0, 1.0, 0.5, -1.0]], F), (n, 1))
    a = da.select_ddqn(q, g, u0, u1)
    rnd = u0 >= F(g)
    share, sigma = rnd.mean(), np.sqrt(g * (1 - g) / n)
    assert abs(share - (1 - g)) <= 4 * sigma, (share, sigma)
    assert (a[~rnd] == 1).all() and a.min() >= 0 and a.max() <= A - 1
    # the random branch is uniform over the A actions
    cnt = np.bincount(a[rnd], minlength=A) / rnd.sum()
    assert (np.abs(cnt - 1.0 / A) <= 4 * np.sqrt(0.25 * 0.75 / rnd.sum())).all(), cnt
    assert da.select_ddqn(q[:1], g, np.array([0.99], F), np.array([np.nextafter(F(1), F(0))], F))[0] == A - 1


def test_sqn_sample_frequencies():
    n, alpha = 100000, 0.2
    qrow = np.array([0.3, 0.1, 0.45, 0.0, 0.25], F)
    u0, _ = da.uniforms(3, 77, n)
    a = da.select_sqn(np.tile(qrow[None], (n, 1)), alpha, u0)
    z = qrow.astype(np.float64) / float(F(alpha))
    p = np.exp(z - z.max())
    p /= p.sum()
    freq = np.bincount(a, minlength=qrow.size) / n
    assert (np.abs(freq - p) <= 4 * np.sqrt(p * (1 - p) / n)).all(), (freq, p)


def test_sqn_last_index_fallback():
    """u0 forced to the largest float32 below 1 lands in the LAST action's interval, and the fallback proper — no cumulative sum above
    u0 * total — returns the last index.  In float32, u0 * total with u0 = 1 - 2^-24 is total minus at least half a unit in the last
    place, which rounds to a float below total (exactly total - 2^-24 * total when total is a power of two, else total's predecessor):
    a generator value cannot make the product reach the total, so the branch is a guard, and it is driven here with u0 = 1."""
    top = np.array([np.nextafter(F(1), F(0))], F)
    for q in (np.array([[0.0, 0.0, 0.0]], F), np.array([[1.0, 0.5, 0.25, 0.0]], F), np.array([[0.2, 0.1]], F), np.array([[0.0]], F),
              np.array([[0.3, 0.1, 0.45, 0.0, 0.25]], F)):
        A = q.shape[1]
        for alpha in (0.5, 1.0):
            p = np.exp(((q - q.max()) / F(alpha)).astype(F)).astype(F)
            total = F(0)
            for k in range(A):
                total = F(total + p[0, k])
            assert F(top[0] * total) < total
            assert da.select_sqn(q, alpha, top)[0] == A - 1
            assert da.select_sqn(q, alpha, np.array([1.0], F))[0] == A - 1        # nothing above u0 * total = total: the fallback
            assert da.select_sqn(q, alpha, np.array([0.0], F))[0] == 0
            assert da.sqn_boundaries64(q, alpha, np.array([1.0], F))[0][0] == A - 1


def test_action_table_gives_gyms_discrete_powers(monkeypatch):
    """Main power 1 or 0 and side power 1 or 0 on the four table rows, read off the fuel terms of the reward — 0.30 m + 0.03 s — with
    everything else equal: the engines' thrust is switched off in the oracle, so the four landers fly the same trajectory."""
    monkeypatch.setattr(eo, "MAIN_POWER", eo.F(0.0))
    monkeypatch.setattr(eo, "SIDE_POWER", eo.F(0.0))
    want = {0: (0.0, 0.0), 1: (0.0, 1.0), 2: (1.0, 0.0), 3: (0.0, 1.0)}
    base = eo.LanderOracle(1, seed=4)
    for _ in range(5):
        ref = [eo.LanderOracle(1, seed=4) for _ in range(4)]
        for k, o in enumerate(ref):
            o.S[:] = base.S
        r = [o.step(da.table_actions([k]))[1][0] for k, o in enumerate(ref)]
        for k in range(4):
            m, s = want[k]
            assert r[k] == F(F(r[0] - F(F(m) * F(0.30))) - F(F(s) * F(0.03))), (k, r)
            same = np.arange(ref[k].S.shape[0]) != eo.EPRET             # (the episode return carries the reward itself)
            np.testing.assert_array_equal(ref[k].S[same], ref[0].S[same])
        base.step(da.table_actions([0]))
    # the clamp: -1 -> noop, 7 -> right engine; fractions truncate
    np.testing.assert_array_equal(da.table_actions([-1, 7, 2.9, 0.5]), da.ACTION_TABLE[[0, 3, 2, 0]])
    # direction = action - 2 on the side engines
    assert da.ACTION_TABLE[1, 1] == -1.0 and da.ACTION_TABLE[3, 1] == 1.0
