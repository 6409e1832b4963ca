"""The articulated lander's crafted-state scenarios (tests/_lander3_scenarios.py) on the CPU, from the oracle alone: the CENSUS of the
solver branches they reach (floors under every class, written to profiles/lander3_census.txt), the PHYSICS IDENTITIES of every step
(linear momentum, angular momentum about the world origin) in the float64 restatement and in the float32 oracle, exact float32
invariants of every after-state, and the accuracy of sincos32.  No GPU; tests/test_gpu_lander3_scenarios.py holds the HIP kernel to
the same trajectories bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _lander3_scenarios as Z   # noqa: E402
import lander3_oracle as L3      # noqa: E402

CENSUS_FILE = os.path.join(ROOT, "profiles", "lander3_census.txt")
MARK = "== scenario library"
FLOOR, MIN_LANES = 8, 2
SIZE_CAPS = {Z.FAST: (256, 40), Z.GYM: (64, 12)}


@pytest.fixture(scope="module")
def runs():
    """Every scenario through the float32 oracle, once."""
    out = {}
    for name, f in Z.SCENARIOS.items():
        scn = f()
        out[name] = (scn, Z.run_oracle(scn))
    return out


@pytest.fixture(scope="module")
def tables(runs):
    return {name: Z.census(scn, run) for name, (scn, run) in runs.items()}


def test_scenario_sizes_and_interleaving(runs):
    """n <= 256 and T <= 40 at 8 / 3; at most two scenarios at 180 / 60, n <= 64 and T <= 12 there.  Blocks are float32 [66, n],
    and no 64-lane group of a scenario is made of one class: the start states of neighbouring envs differ."""
    gym = 0
    for name, (scn, _) in runs.items():
        S0, acts, (vit, pit, max_ep_len) = scn
        n, T = S0.shape[1], acts.shape[0]
        assert S0.dtype == np.float32 and S0.shape == (L3.NF3, n) and acts.dtype == np.float32 and acts.shape == (T, n, 2), name
        cap_n, cap_t = SIZE_CAPS[(vit, pit)]
        assert n <= cap_n and T <= cap_t, (name, n, T)
        gym += (vit, pit) == Z.GYM
        assert (np.abs(np.diff(S0[[L3.Y, L3.ANG, L3.SLEEP, L3.VY]], axis=1)).sum(axis=0) > 0).all(), name
    assert gym <= 2


def _table(tables):
    names = list(tables)
    keys = [k for k in next(iter(tables.values()))[0] if not k.startswith("_")]
    lines = ["%s: env-steps per class and scenario (tests/_lander3_scenarios.py; written by tests/test_lander3_scenarios_cpu.py)" % MARK,
             "scenarios: " + ", ".join("%s [%d envs x %d steps at %d / %d]" % ((nm, tables[nm][3], tables[nm][4]) + tables[nm][5]) for nm in names),
             "%-62s %7s %5s  %s" % ("class", "total", "lanes", " ".join("%6.6s" % nm for nm in names))]
    for k in keys:
        tot = sum(tables[nm][0][k] for nm in names)
        lanes = set().union(*(tables[nm][1][k] for nm in names))
        lines.append("%-62s %7d %5d  %s" % (k, tot, len(lanes), " ".join("%6d" % tables[nm][0][k] for nm in names)))
    lines.append("(step, 64-env group) pairs with >= 3 different sweep counts and lanes with and without contact: "
                 + ", ".join("%s %d" % (nm, tables[nm][2]) for nm in names))
    return lines


def test_census_floors_and_table(runs, tables):
    """Every class in at least 8 env-steps and at two lane positions modulo 64, summed over the scenarios; UNREACHED may excuse only
    the two dynamic far-side limit classes, and then the injected warm start of that row must meet the floor."""
    full = {nm: tables[nm] + (runs[nm][0][0].shape[1], runs[nm][0][1].shape[0], runs[nm][0][2][:2]) for nm in tables}
    lines = _table(full)
    print("\n".join(lines))
    try:   # the committed table: the old matrix's part is kept, the library's part rewritten (identical unless a scenario changed)
        head = []
        if os.path.exists(CENSUS_FILE):
            for ln in open(CENSUS_FILE).read().splitlines():
                if ln.startswith(MARK):
                    break
                head.append(ln)
        with open(CENSUS_FILE, "w") as f:
            f.write("\n".join(head + lines) + "\n")
    except OSError:
        pass
    assert set(Z.UNREACHED) <= set(Z.FAR_SIDE), "UNREACHED may name only the dynamic far-side limit classes"
    for k in Z.UNREACHED:
        assert Z.UNREACHED[k] and "search" in (Z.__doc__ + Z.joint_limits.__doc__).lower()
    keys = [k for k in next(iter(tables.values()))[0] if not k.startswith("_")]
    short = []
    for k in keys:
        tot = sum(t[0][k] for t in tables.values())
        lanes = set().union(*(t[1][k] for t in tables.values()))
        if k in Z.UNREACHED:
            k2 = Z.INJECTED[k]
            assert sum(t[0][k2] for t in tables.values()) >= FLOOR, k2
            continue
        if tot < FLOOR or len(lanes) < MIN_LANES:
            short.append((k, tot, len(lanes)))
    assert not short, short
    # the injected far-side warm starts run on non-trivial numbers whether or not the dynamic classes are reached
    for k2 in Z.INJECTED.values():
        assert tables["joint_limits"][0][k2] >= FLOOR, k2
    b0 = runs["joint_limits"][1]["before"][0]
    assert (b0[Z.JNT(0, 4)] == 0.5).sum() >= FLOOR and (b0[Z.JNT(1, 3)] == 0.5).sum() >= FLOOR   # the injected ones themselves
    # waves that diverge: >= 3 sweep counts and lanes with and without contact inside one 64-env group, in >= 2 scenarios
    assert sum(t[2] > 0 for t in tables.values()) >= 2, {nm: t[2] for nm, t in tables.items()}


def test_rest_scenarios_reach_what_the_old_matrix_does_not(tables):
    """+100, the SLEEP counter counting and resetting: at 180 / 60 and, forced, at 8 / 3; the mixed scenario (run through the other
    launch paths with the engines off) holds contact, a rest exit and a lane without contact in one wave."""
    for nm in ("rest_gym", "rest_forced"):
        c = tables[nm][0]
        assert c["+100 rest reward"] >= FLOOR and c["SLEEP incremented"] >= FLOOR and c["SLEEP reset from > 0"] >= FLOOR, (nm, c)
    assert tables["mixed"][0]["+100 rest reward"] >= FLOOR


def test_endings_crash_by_the_vertex_that_was_turned_down(runs):
    """Classes 0-5 of `endings`: the first crash of env i (class k = i % 12 < 6) has vertex k below the ground — recomputed here from
    the after-state in float64, beside the oracle's own `crash` flag."""
    scn, run = runs["endings"]
    n = scn[0].shape[1]
    seen = np.zeros(n, bool)
    hit = np.zeros(6, int)
    for last in run["last"]:
        vx, vy = Z.hull_vertices(last["state"])
        first = last["crash"] & ~seen & (np.arange(n) % 12 < 6)
        seen |= last["crash"] | last["out"]
        for i in np.nonzero(first)[0]:
            k = i % 12
            assert vy[k, i] < Z.ground(last["state"], vx[k])[i], (i, k)
            hit[k] += 1
    assert (hit >= FLOOR).all(), hit


def test_endings_engine_thresholds_and_the_action_clip(runs):
    """`endings` walks every env through SPECIAL_ACTIONS: the main engine is off at 0 and -0 and on (power 0.5) one float32 above 0,
    the side engine off at +-0.5 exactly and at 0.49999997 and on one float32 beyond, and actions outside [-1, 1] fire at power 1."""
    scn, run = runs["endings"]
    a = Z.SPECIAL_ACTIONS
    assert a[1, 0] > 0 and a[1, 0] < 1e-40 and a[1, 1] > 0.5 and a[1, 1] - np.float32(0.5) < 1e-7 and a[3, 1] == -a[1, 1]
    main_on = np.array([0, 1, 0, 1, 0, 1, 1, 1], bool)
    side_on = np.array([0, 1, 0, 1, 1, 1, 1, 0], bool)
    n = scn[0].shape[1]
    for t, last in enumerate(run["last"]):
        k = (t + np.arange(n)) % len(a)
        np.testing.assert_array_equal(last["m_power"] > 0, main_on[k])
        np.testing.assert_array_equal(last["s_power"] > 0, side_on[k])
        assert (last["m_power"][k == 1] == 0.5).all() and (last["m_power"][(k == 3) | (k == 7)] == 1.0).all()
        assert (last["s_power"][k == 1] == a[1, 1]).all() and (last["s_power"][(k == 4) | (k == 6)] == 1.0).all()


# ---- physics identities -------------------------------------------------------------------------------------------------------------
def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def _terms(before, rec):
    """-> (LHS [3, n], RHS [3, n]) of the step `before` -> rec["state"], evaluated in float64: linear momentum x, y and angular
    momentum about the world origin.  LHS: the bodies' momentum change, the angular part with the BEFORE pose (every velocity impulse
    of the step is applied at the before pose; the position solve moves no velocity).  RHS: gravity, the two engine impulses at
    their points on the hull, every contact's accumulated impulse of the after-state (warm start + increments = what the step
    applied; zero on corners out of contact) along the normal / tangent of the corner's segment at the corner, and the joints'
    accumulated point impulses acting on the gap between the two anchors (equal and opposite at two points that differ by the
    joint's position error).  The axial impulses (motor, limits) are equal and opposite torques: they cancel."""
    B, A = np.asarray(before, np.float64), np.asarray(rec["state"], np.float64)
    mh, ih, ml, il = (1.0 / float(v) for v in (L3.INV_MH, L3.INV_IH, L3.INV_ML, L3.INV_IL))
    g = float(L3.GRAV) * float(L3.DT)
    bodies = [(mh, ih, L3.X, L3.Y, L3.VX, L3.VY, L3.OM)] + [(ml, il) + tuple(Z.LEG(b, f) for f in (0, 1, 2, 3, 5)) for b in range(2)]
    lhs, rhs = np.zeros((3,) + B.shape[1:]), np.zeros((3,) + B.shape[1:])
    for m, i, x, y, vx, vy, om in bodies:
        dvx, dvy = A[vx] - B[vx], A[vy] - B[vy]
        lhs += np.stack([m * dvx, m * dvy, m * _cross(B[x], B[y], dvx, dvy) + i * (A[om] - B[om])])
        rhs += np.stack([np.zeros_like(dvx), m * g + 0 * dvx, m * g * B[x]])
    for imp, arm in (("main", "main_r"), ("side", "side_r")):
        ix, iy = (np.asarray(v, np.float64) for v in rec[imp])
        rx, ry = (np.asarray(v, np.float64) for v in rec[arm])
        rhs += np.stack([ix, iy, _cross(B[L3.X] + rx, B[L3.Y] + ry, ix, iy)])
    cx, cy = Z.corners(B)
    dh = np.asarray(rec["dh"], np.float64)
    ln = np.sqrt(dh * dh + 4.0)
    nx, ny = -dh / ln, 2.0 / ln
    for q in range(8):
        jx = A[Z.CAN(q)] * nx[q] + A[Z.CAT(q)] * ny[q]
        jy = A[Z.CAN(q)] * ny[q] - A[Z.CAT(q)] * nx[q]
        rhs += np.stack([jx, jy, _cross(cx[q], cy[q], jx, jy)])
    sa, ca = np.sin(B[L3.ANG]), np.cos(B[L3.ANG])
    ax, ay = B[L3.X] + sa * float(L3.LCY), B[L3.Y] - ca * float(L3.LCY)
    for b in range(2):
        s, c = np.sin(B[Z.LEG(b, 4)]), np.cos(B[Z.LEG(b, 4)])
        lx, ly = float(L3.SIGN[b]) * float(L3.ANCX), float(L3.ANCY)
        bx, by = B[Z.LEG(b, 0)] + c * lx - s * ly, B[Z.LEG(b, 1)] + s * lx + c * ly
        rhs[2] += _cross(bx - ax, by - ay, A[Z.JNT(b, 0)], A[Z.JNT(b, 1)])
    return lhs, rhs


DISCRETE = ("on", "sweeps", "solved", "friction_clamp", "motor_hi", "motor_lo", "crash", "out", "asleep")
BAR64 = 1e-9


def _identities(name, scn, run, L64):
    S0, acts, (vit, pit, max_ep_len) = scn
    n = S0.shape[1]
    o64 = Z.oracle(n, vit, pit, max_ep_len, L64)
    worst = {"r64": 0.0, "r32": 0.0, "dev": 0.0, "excluded": 0, "steps": 0}
    for t in range(acts.shape[0]):
        before, rec32 = run["before"][t], run["last"][t]
        o64.S[:] = before.astype(np.float64)
        o64._physics(acts[t].astype(np.float64))
        rec64 = o64.last
        same = np.ones(n, bool)
        for k in DISCRETE:
            d = np.asarray(rec32[k]) != np.asarray(rec64[k])
            same &= ~(d.any(axis=0) if d.ndim == 2 else d)
        l32, r32 = _terms(before, rec32)
        l64, r64 = _terms(before, rec64)
        e32, e64 = np.abs(l32 - r32), np.abs(l64 - r64)
        dev = np.maximum(np.abs(l32 - l64), np.abs(r32 - r64))
        # the restatement holds the identities on EVERY step (its own discrete record describes its own step)
        assert e64.max() <= BAR64, (name, t, e64.max(axis=1), np.argmax(e64, axis=1))
        ok = e32 <= 2.0 * dev + BAR64
        assert ok[:, same].all(), (name, t, e32[:, same].max(axis=1), dev[:, same].max(axis=1))
        worst["r64"], worst["excluded"], worst["steps"] = max(worst["r64"], e64.max()), worst["excluded"] + int((~same).sum()), worst["steps"] + n
        if same.any():
            worst["r32"], worst["dev"] = max(worst["r32"], e32[:, same].max()), max(worst["dev"], dev[:, same].max())
    return worst


@pytest.fixture(scope="module")
def L64():
    return Z.float64_restatement()


@pytest.mark.parametrize("name", list(Z.SCENARIOS))
def test_momentum_identities_on_every_scenario_step(runs, L64, name):
    """For every step of the float32 trajectory: the before-state stepped once in float32 (the trajectory's own step) and once in the
    float64 restatement, both checked against

        M dv_total            = M g dt y^ + J_main + J_side + sum_q (can'_q n_q + cat'_q t_q)
        d(angular momentum, about the world origin, before pose)
                              = the same impulses as p x J + sum_b ((x_leg + rB) - (x_hull + rA)) x jp'_b

    Bars, as in test_free_fall_...: the float64 restatement satisfies both to 1e-9 — the terms are below 2^11 (positions below 32,
    momenta m v below 64), a float64 rounding of such a term is below 2^11 * 2^-53 = 2.3e-13, and a step makes at most
    vit * (2 joints * 12 + 8 contacts * 6) + 60 velocity updates = 13 000 at 180 iterations: 3e-9 if every rounding pushed the same
    way, 3e-11 as the random walk they are; at 8 iterations 1.5e-10 in the worst case.  The float32 step's residual is at most
    twice its own deviation from the restatement (the larger of the two sides' deviations: residual32 = dLHS - dRHS + residual64),
    plus that bar, on the env-steps whose discrete record (contact mask, sweeps, clamp flags, endings) agrees between the two
    precisions; the others — at most 10 % of the scenario's env-steps — are only held to the float64 identity.
    Observed: float64 residual at most 6.9e-13 (rest_gym, 180 / 60) and 4.2e-13 at 8 / 3; float32 residual at most 1.2e-3 at 180 / 60
    and 2.5e-4 at 8 / 3 (angular momentum about the origin: |x| ~ 10 times the linear figure), each within its deviation; excluded
    20 of 3072 env-steps in joint_limits, 1 of 3840 in spin, none elsewhere.
    Sanity of this test, done once on a scratch copy: with the sign of leg 0's anchor x flipped in the joint initialisation the
    angular identity fails on the first step of every scenario tried (float64 residual 0.2 .. 0.6)."""
    scn, run = runs[name]
    w = _identities(name, scn, run, L64)
    print("identities %s: %s" % (name, w))
    assert w["excluded"] <= 0.10 * w["steps"], w


def test_exact_float32_invariants_on_every_after_state(runs):
    for name, (scn, run) in runs.items():
        for t, last in enumerate(run["last"]):
            check_invariants(last["state"], last["on"], (name, t))
        check_invariants(run["final"], None, (name, "final"))


def check_invariants(S, on, where):
    """can >= 0, jlo / jup >= 0, |jm| <= 0.8, zero accumulated impulses on corners out of contact, C1 / C2 = OR of the leg's mask,
    everything finite — exact, on a float32 state block.  `on` None: the mask is taken from C1 / C2 (leg level only)."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and np.isfinite(S).all(), where
    for q in range(8):
        assert (S[Z.CAN(q)] >= 0).all(), (where, q)
    for b in range(2):
        assert (S[Z.JNT(b, 3)] >= 0).all() and (S[Z.JNT(b, 4)] >= 0).all(), (where, b)
        assert (np.abs(S[Z.JNT(b, 2)]) <= L3.MAX_MOTOR_IMP).all(), (where, b)
        flag = S[(L3.C1, L3.C2)[b]]
        assert ((flag == 0) | (flag == 1)).all(), (where, b)
        if on is not None:
            np.testing.assert_array_equal(flag, on[4 * b:4 * b + 4].any(axis=0).astype(np.float32), err_msg=str(where))
        for k in range(4):
            off = (flag == 0) if on is None else ~on[4 * b + k]
            assert (S[Z.CAN(4 * b + k)][off] == 0).all() and (S[Z.CAT(4 * b + k)][off] == 0).all(), (where, b, k)


def test_sincos32_against_float64():
    """oracle.env_oracle.sincos32 (every rotation of both landers; the kernels mirror it) against np.sin / np.cos of the same float32
    argument in float64: 4 * 10^6 evenly spaced float32 points on [-1000, 1000] plus the float32 neighbours of every multiple of
    pi / 2 in that range.  Bar 2^-23 (two units of float32 resolution at 1).  Measured on these points: max abs error
    1.46 * 2^-24 on [-4, 4], 1.49 * 2^-24 on [-64, 64], 1.53 * 2^-24 on [-1000, 1000].  Not asserted: at +-10^5 the three-term reduction has lost bits and the error is
    16 * 2^-24 — beyond any angle an episode can reach (|omega| stays below 100 rad/s for 1000 steps of 0.02 s)."""
    from oracle.env_oracle import sincos32
    x = np.linspace(-1000.0, 1000.0, 4_000_000).astype(np.float32)
    m = (np.arange(-636, 637) * (np.pi / 2)).astype(np.float32)   # 636 pi / 2 = 999.03
    x = np.concatenate([x, m, np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf))])
    s, c = sincos32(x)
    assert s.dtype == np.float32 and c.dtype == np.float32
    x64 = x.astype(np.float64)
    err = np.maximum(np.abs(s.astype(np.float64) - np.sin(x64)), np.abs(c.astype(np.float64) - np.cos(x64)))
    for lim in (4.0, 64.0, 1000.0):
        print("sincos32 on [-%g, %g]: max abs error %.3f * 2^-24" % (lim, lim, err[np.abs(x64) <= lim].max() * 2.0 ** 24))
    assert err.max() <= 2.0 ** -23, (err.max() * 2.0 ** 24, x[np.argmax(err)])
