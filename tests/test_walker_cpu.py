"""The bipedal walker's specification (tests/walker_oracle.py) on the CPU, held to what can be derived rather than to itself: momentum
and joint invariants in free flight, the motor's torque and speed bounds, joint limits and contact separations after a converged
position solve, the reward against a float64 restatement, the terrain recurrence's closed-form bound, the lidar on the flat pad, the
crafted scenarios' census, the golden file, and the header's symbols.  No GPU; the HIP kernel is pinned to the same oracle, the same
golden file and the same scenarios in tests/test_gpu_walker.py and tests/test_gpu_walker_scenarios.py."""
import hashlib
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _walker_scenarios as sc   # noqa: E402
import walker_oracle as W   # noqa: E402

F = np.float32
EPS = 2.0 ** -23                       # float32 epsilon
GOLDEN = os.path.join(HERE, "golden", "walker_heuristic.npz")
MASS = np.array([1.0 / float(m) for m in W.INVM])
INERTIA = np.array([1.0 / float(i) for i in W.INVI])


def _crafted(n, p, terr, vit, pit, max_ep_len=1600):
    """An oracle whose every env holds pose `p` (a _walker_scenarios.pose dict) over terrain `terr`."""
    ora = W.WalkerOracle(n, seed=5, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)
    ora.S[:W.T0] = 0.0
    for f, v in p.items():
        ora.S[f] = F(v)
    ora.S[W.T0:] = terr.astype(F)[:, None]
    return ora


def _kin(S):
    """-> positions [5, 2, n], angles [5, n], velocities [5, 2, n], angular velocities [5, n] of the bodies, float64."""
    S = S.astype(np.float64)
    rows = [(W.X, W.Y, W.ANG, W.VX, W.VY, W.OM)] + [tuple(sc.LEG(b, f) for f in (0, 1, 4, 2, 3, 5)) for b in range(1, 5)]
    pos = np.stack([np.stack([S[r[0]], S[r[1]]]) for r in rows])
    ang = np.stack([S[r[2]] for r in rows])
    vel = np.stack([np.stack([S[r[3]], S[r[4]]]) for r in rows])
    om = np.stack([S[r[5]] for r in rows])
    return pos, ang, vel, om


def _momenta(S):
    """Total linear momentum [2, n] and angular momentum about the common centre of mass [n], float64."""
    pos, _, vel, om = _kin(S)
    m = MASS[:, None, None]
    P = (m * vel).sum(0)
    R, V = (m * pos).sum(0) / MASS.sum(), P / MASS.sum()
    r, v = pos - R, vel - V
    L = (INERTIA[:, None] * om).sum(0) + (MASS[:, None] * (r[:, 0] * v[:, 1] - r[:, 1] * v[:, 0])).sum(0)
    return P, L


def _anchor_gaps(S):
    """World distance between the two anchors of each joint [4, n], float64 with exact sin / cos."""
    pos, ang, _, _ = _kin(S)
    out = []
    for j in range(4):
        A, B = W.JA[j], j + 1
        ca, sa, cb, sb = np.cos(ang[A]), np.sin(ang[A]), np.cos(ang[B]), np.sin(ang[B])
        ax, ay, bx, by = float(W.JAX[j]), float(W.JAY[j]), float(W.JBX), float(W.JBY)
        pa = pos[A] + np.stack([ca * ax - sa * ay, sa * ax + ca * ay])
        pb = pos[B] + np.stack([cb * bx - sb * by, sb * bx + cb * by])
        out.append(np.hypot(*(pb - pa)))
    return np.stack(out)


def _joint_angles(S):
    _, ang, _, om = _kin(S)
    return np.stack([ang[j + 1] - ang[W.JA[j]] for j in range(4)]), np.stack([om[j + 1] - om[W.JA[j]] for j in range(4)])


def test_free_flight_momentum_and_joint_anchors():
    """A crafted state 2 m above the pad with the bodies spinning against each other, zero action (zero motor torque), 20 / 10
    iterations, 25 steps (a fall of 1.3 m: no contact).  Linear momentum changes by m_total g dt per step and angular momentum about the
    common centre stays what it was, to float32 rounding: every velocity update rounds within eps/2 of the value it writes, a sweep
    updates a body's velocity at most 4 times per component (two joints, A and B side) and a step runs vit velocity and at most pit
    position sweeps, so over t steps the sums drift by at most t (4 vit + 4 pit + 8) eps times the magnitudes summed — for the linear
    momentum sum m |v|, for the angular one sum (I |w| + m |position| |v|), the positions being absolute coordinates.  The joints' anchor
    gaps stay within b2_linearSlop."""
    n, steps, vit, pit = 4, 25, 20, 10
    p = sc.lift(sc.pose(10.0, 6.0, 0.1, 0.3, -0.7, -0.2, -1.0), sc.FLAT, 2.0)
    ora = _crafted(n, p, sc.FLAT, vit, pit)
    ora.S[W.OM] = F(0.3)
    for b, w in zip(range(1, 5), (1.0, -0.5, -1.0, 0.5)):
        ora.S[sc.LEG(b, 5)] = F(w)
    P0, L0 = _momenta(ora.S)
    g_step = float(W.GRAV) * float(W.DT) * MASS.sum()
    zero = np.zeros((n, 4), F)
    worst = {"P": 0.0, "L": 0.0, "gap": 0.0, "barP": 0.0, "barL": 0.0}
    for t in range(1, steps + 1):
        out = ora.step(zero)
        assert not out[4].any() and not ora.last["on"].any(), "a contact or an episode end at step %d: not free flight" % t
        pos, _, vel, om = _kin(ora.S)
        P, L = _momenta(ora.S)
        k = t * (4 * vit + 4 * pit + 8) * EPS
        barP = k * (MASS[:, None] * np.abs(vel).max(1)).sum(0)
        barL = k * (INERTIA[:, None] * np.abs(om) + MASS[:, None] * np.abs(pos).max(1) * np.abs(vel).max(1)).sum(0)
        eP = np.abs(P - P0 - np.array([0.0, g_step * t])[:, None]).max(0)
        eL = np.abs(L - L0)
        worst.update(P=max(worst["P"], eP.max()), L=max(worst["L"], eL.max()), gap=max(worst["gap"], _anchor_gaps(ora.S).max()),
                     barP=barP.max(), barL=barL.max())
        assert (eP <= barP).all(), (t, eP, barP)
        assert (eL <= barL).all(), (t, eL, barL)
        assert ora.last["solved"].all()
    print("free flight:", worst)
    assert abs(L0).min() > 0.5                       # the conserved quantity is not trivially zero
    assert worst["gap"] <= float(W.SLOP)


def test_motor_torque_and_speed_bounds():
    """Free flight at gym's 180 / 60 with a_j = +-1: the accumulated motor impulse of a step never exceeds 80 dt, and the joint's speed
    along the command never overshoots SPEED_j.  The motor row itself lands on the target speed to rounding; what the later rows of the
    same sweep (the point constraint) add back is the Gauss-Seidel residual of the last of 180 sweeps, allowed here at 2^-10 of SPEED_j
    (observed: 8e-5 rad/s, printed)."""
    n = 2
    p = sc.lift(sc.pose(10.0, 6.0, 0.0, 0.1, -0.8, 0.1, -0.8), sc.FLAT, 2.5)
    ora = _crafted(n, p, sc.FLAT, *sc.GYM)
    act = np.array([[1, 1, -1, -1], [-1, -1, 1, 1]], F)
    over, reached = 0.0, 0
    for t in range(14):
        out = ora.step(act)
        assert not out[4].any() and not ora.last["on"].any()
        m = ora.last["motor"].astype(np.float64)
        assert (np.abs(m) <= 80.0 * float(W.DT) * (1 + EPS)).all()
        assert (ora.last["mmax"] == F(1.6)).all()
        _, rel = _joint_angles(ora.S)
        along = rel * np.sign(act.T)
        for j in range(4):
            over = max(over, float((along[j] - float(W.SPEED[j])).max()))
            assert (along[j] <= float(W.SPEED[j]) * (1 + 2.0 ** -10)).all(), (t, j, along[j])
            reached += int((along[j] >= float(W.SPEED[j]) * (1 - 2.0 ** -10)).sum())
    print("motor: largest overshoot %.3g rad/s; joint-steps at the target speed: %d" % (over, reached))
    assert reached > 0                               # the bound was met, not only approached


def test_limits_and_contact_separations_after_a_converged_position_solve():
    """On the crafted scenarios (every joint starts 0.06 rad beyond a limit with its motor pushing outward; stances, kneeling, slopes):
    whenever the position solve reported convergence, every joint angle is within [lower - b2_angularSlop, upper + b2_angularSlop] and
    every active point's separation is >= -3 b2_linearSlop, both as the converged sweep measured them: the solver's exit test makes
    this exact (2 eps of the angle for the float32 difference the test restates in float64)."""
    for it in (sc.FAST, sc.GYM):
        _, _, _, _, census, recs = sc.trajectory(*it)
        n_lim = n_sep = 0
        for r in recs:
            ok, ang = r["solved"], r["jangle"].astype(np.float64)
            for j in range(4):
                lo, up = float(W.LIM_LO[j]) - float(W.ASLOP), float(W.LIM_UP[j]) + float(W.ASLOP)
                assert (ang[j][ok] >= lo - 4 * EPS).all() and (ang[j][ok] <= up + 4 * EPS).all(), (it, j, ang[j][ok].min(), ang[j][ok].max())
                n_lim += int(((ang[j] <= float(W.LIM_LO[j])) | (ang[j] >= float(W.LIM_UP[j])))[ok].sum())
            act = r["on"] & ok[None]
            assert (r["sep"][act] >= W.SLOP3).all(), (it, r["sep"][act].min())
            n_sep += int(act.sum())
        print(it, "joint-steps beyond a limit under a converged solve: %d; active points under one: %d" % (n_lim, n_sep))
        # at 60 sweeps each of the 8 (joint, limit) pairs of the two limit classes converges beyond its limit in every copy; 3 sweeps
        # (8 degrees of correction each) rarely get there
        assert n_lim >= (8 * (sc.N // len(sc.CLASSES)) if it == sc.GYM else 1) and n_sep > 0


# what the crafted states must reach at both iteration pairs (tests/_walker_scenarios.census_of); profiles/walker_census.txt records
# the counts beside the live matrix's
REQUIRED = ["limit_lo_hip0", "limit_up_hip0", "limit_lo_knee0", "limit_up_knee0", "limit_lo_hip1", "limit_up_hip1", "limit_lo_knee1",
            "limit_up_knee1", "contact_knee_without_foot", "contact_foot", "contact_on_slope", "contact_foot_across_edge", "friction_clamped",
            "motor_clamped_hip0", "motor_free_knee0", "motor_zero_torque_hip1", "position_solved_first_sweep", "position_solved_later",
            "game_over", "x_negative", "terrain_end", "lidar_all_miss", "lidar_hit_own_segment", "lidar_hit_far_segment"]


@pytest.mark.parametrize("it", [sc.FAST, sc.GYM])
def test_crafted_states_reach_their_classes(it):
    _, _, outs, final, census, _ = sc.trajectory(*it)
    print(it, census)
    copies = sc.N // len(sc.CLASSES)
    for k in REQUIRED:
        assert census.get(k, 0) >= copies, (k, census.get(k, 0))
    assert np.isfinite(final).all() and all(np.isfinite(o[0]).all() and np.isfinite(o[1]).all() for o in outs)
    for name, exit_ in (("hull_crash", -100.0), ("x_negative", -100.0), ("terrain_end", None)):
        e = sc.CLASSES.index(name)
        assert outs[0][4][e] == 1 and outs[0][2][e] == 1.0               # ended and stored as terminal at the first step
        assert exit_ is None or outs[0][1][e] == exit_


def test_reward_against_a_float64_restatement():
    """r = shaping(after) - shaping(before) - sum 0.028 clip(|a_j|, 0, 1), shaping = 130 x / 30 - 5 |angle|, restated in float64 from the
    recorded float32 positions, angles and actions.  The float32 value takes 4 roundings per shaping (product, quotient, product,
    difference), one for the shaping difference and 2 per fuel term (8): each within eps/2 of a magnitude no larger than
    S = 130 |x| / 30 + 5 |angle| (shaping terms) or |r| + 0.112 (fuel terms), so |r32 - r64| <= (9 S + 8 (|r| + 0.112)) eps / 2."""
    n = 33
    ora = W.WalkerOracle(n, seed=7, velocity_iterations=8, position_iterations=3)
    rs = np.random.RandomState(7)
    sh = lambda S: 130.0 * S[W.PX].astype(np.float64) / 30.0 - 5.0 * np.abs(S[W.ANG].astype(np.float64))   # noqa: E731
    checked, worst = 0, 0.0
    for t in range(60):
        before = ora.S.copy()
        a = rs.uniform(-1.3, 1.3, (n, 4)).astype(F)
        _, rew, _, _, _ = ora.step(a)
        after = ora.last["state"]
        live = ~(ora.last["game_over"] | ora.last["neg_x"]) & (before[W.HASP] > 0)
        fuel = (float(W.FUEL) * np.clip(np.abs(a.astype(np.float64)), 0.0, 1.0)).sum(1)
        r64 = sh(after) - sh(before) - fuel
        S = np.maximum(130.0 * np.abs(after[W.PX]) / 30.0 + 5.0 * np.abs(after[W.ANG]), 130.0 * np.abs(before[W.PX]) / 30.0 + 5.0 * np.abs(before[W.ANG]))
        bar = (9.0 * S + 8.0 * (np.abs(r64) + 0.112)) * EPS / 2.0
        err = np.abs(rew.astype(np.float64) - r64)
        assert (err[live] <= bar[live]).all(), (t, err[live].max(), bar[live].min())
        assert (rew[ora.last["game_over"] | ora.last["neg_x"]] == F(-100.0)).all()
        checked += int(live.sum())
        worst = max(worst, float((err[live] / bar[live]).max()))
    print("reward: %d env-steps, largest error / bound %.3f" % (checked, worst))
    assert checked > 1500


def test_terrain_start_pad_and_step_bound():
    """Points 0..20 are TERRAIN_HEIGHT; beyond, v = 0.8 v + 0.01 sign(.) + U(-1, 1) / 30 is bounded by the geometric series
    (0.01 + 1/30) / (1 - 0.8), and |y_i - y_{i-1}| = |v_i| to the rounding of y (one ulp of |y| < 16: 2^-20 here, taken twice)."""
    ora = W.WalkerOracle(64, seed=3, velocity_iterations=1, position_iterations=1)
    T = ora.S[W.T0:W.T0 + W.NT].astype(np.float64)
    assert (ora.S[W.T0:W.T0 + 21] == W.TH).all()
    dy = np.abs(np.diff(T, axis=0))
    assert np.abs(T).max() < 16.0
    assert dy.max() <= (0.01 + 1.0 / 30.0) / 0.2 * (1 + 8 * EPS) + 2.0 ** -19
    assert dy[25:].max() > 0.02 and len(np.unique(T[100])) == 64      # it is a terrain, and every env has its own


def test_lidar_on_the_flat_pad():
    """Over flat ground at height h below the hull's origin, ray i (angle 1.5 i / 10 from straight down) reaches the ground at the
    fraction h / (cos(1.5 i / 10) RANGE), and misses (1.0) where that exceeds 1.  float32: the polynomial cosine (2 ulp), the product
    with RANGE, numerator, denominator and quotient of the ray cast — 16 eps relative covers it."""
    hs = np.array([0.8, 1.7, 2.27, 3.1, 4.4, 5.2, 5.6])
    p = sc.pose(20.0 * sc.STEPf + 0.1, 6.0, 0.2, 0.3, -0.5, -0.3, -0.9)
    ora = _crafted(len(hs), p, sc.FLAT, 1, 1)
    ora.S[W.PY] = (sc.THf + hs).astype(F)
    got = ora.lidar().astype(np.float64)
    h = ora.S[W.PY].astype(np.float64) - float(W.TH)
    hits = misses = 0
    for i in range(10):
        want = h / (np.cos(1.5 * i / 10.0) * float(W.RANGE))
        for e in range(len(hs)):
            if want[e] > 1.0 + 1e-5:
                assert got[e, i] == 1.0
                misses += 1
            elif want[e] < 1.0 - 1e-5:
                assert abs(got[e, i] - want[e]) <= 16 * EPS * want[e], (e, i, got[e, i], want[e])
                hits += 1
    assert hits > 30 and misses > 10
    assert (ora.last_ray_segment[0] >= 0).all() and ora.last_ray_segment[0, 0] == 0     # straight down: the segment the ray starts over


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_file_regenerates_bit_for_bit(golden):
    """The first 20 steps of the oracle at 180 / 60 from the recorded seed equal the file; its episode records are those of its steps."""
    import gen_walker_golden as gen
    g = golden
    assert (int(g["seed"]), int(g["n_envs"]), int(g["velocity_iterations"]), int(g["position_iterations"])) == (gen.SEED, 8, 180, 60)
    assert os.path.getsize(GOLDEN) < 1000000
    again = gen.run(steps=20)
    for k in gen.KEYS:
        assert again[k].dtype == g[k].dtype, k
        np.testing.assert_array_equal(again[k], g[k][:20], err_msg=k)
    assert g["final_state"].shape == (W.NFW, 8) and g["final_state"].dtype == np.float32
    assert g["obs2"].shape[1:] == (8, 24) and g["actions"].shape[1:] == (8, 4)
    assert g["ended"].any(axis=0).all() and len(g["episode_return"]) == int(g["ended"].sum())
    assert (np.abs(g["actions"]) <= 1.0).all()
    print("heuristic: mean distance %.3f m over %d episodes" % (float(g["episode_distance"].mean()), len(g["episode_return"])))


def test_walker_symbols_in_header_and_table():
    """The two new constants in include/ddrl.h equal _lib's and the oracle's, and the header declares the functions it declared before
    the walker: the same names as the ctypes table, which this change does not touch, and the same set as on the parent commit."""
    from distributed_drl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in ("DDRL_ENV_WALKER", "DDRL_ENVW_STATE_FIELDS"):
        m = re.search(r"#define %s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert _lib.DDRL_ENVW_STATE_FIELDS == W.NFW and _lib.DDRL_ENV_WALKER == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    digest = hashlib.sha256("\n".join(sorted(declared)).encode()).hexdigest()
    assert (len(declared), digest[:16]) == PARENT_DECLARATIONS, (len(declared), digest[:16])


PARENT_DECLARATIONS = (143, "570d3a64c46974e4")   # (number of functions include/ddrl.h declared on the parent commit, sha256 of their sorted names)
