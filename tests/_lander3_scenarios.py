"""TEST INFRASTRUCTURE: crafted start states for the articulated lander (tests/lander3_oracle.py, csrc/env3_device.h) and the census
of the solver branches a run reaches.

A scenario is a function -> (state block [66, n] float32, actions [T, n, 2] float32, (vit, pit, max_ep_len)).  The block is injected
into the oracle (`ora.S[:] = block`) and into the kernel (`env.set_state`); both sides are created with seed SEED, which only feeds
the engine dispersion and the resets.  States are built from oracle runs on the CPU and then edited: rotated, lifted, shifted, their
terrain rows and warm-start slots overwritten.  Envs of different classes are INTERLEAVED (class = env id modulo the number of
classes), so every 64-lane wave holds every class of its scenario and its lanes diverge.

`census_of(...)` turns the oracle's per-step record (`Lander3Oracle.last`) into named classes; tests/test_lander3_scenarios_cpu.py
holds the floor under every class and the physics identities, tests/test_gpu_lander3_scenarios.py the kernel's parity on the same
trajectories.
"""
import functools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lander3_oracle as L3   # noqa: E402
from oracle.env_oracle import HULL   # noqa: E402

F = np.float32
SEED = 17
FAST = (8, 3)      # the live tests' iteration counts
GYM = (180, 60)    # gym's
LEG = lambda b, f: L3.L0 + 6 * b + f                 # f: 0 x, 1 y, 2 vx, 3 vy, 4 ang, 5 om   # noqa: E731
JNT = lambda b, f: L3.J0 + 5 * b + f                 # f: 0 px, 1 py, 2 motor, 3 lower, 4 upper   # noqa: E731
CAN = lambda q: L3.K0 + 2 * q                        # accumulated normal impulse of corner q = 4 leg + k   # noqa: E731
CAT = lambda q: L3.K0 + 2 * q + 1                    # noqa: E731


def float64_restatement():
    """The SAME step in float64: the oracle's source with its working type switched and exact sin / cos.  Every constant is set back
    to the float32 oracle's value (mass data, limits, tolerances), the random numbers are the same 24-bit values: the same model,
    finer arithmetic."""
    src = open(L3.__file__).read()
    assert src.count("F = np.float32") == 1
    mod = types.ModuleType("lander3_oracle_f64")
    mod.__file__ = L3.__file__
    exec(compile(src.replace("F = np.float32", "F = np.float64"), L3.__file__, "exec"), mod.__dict__)
    for name, v in vars(L3).items():
        if isinstance(v, np.float32):
            setattr(mod, name, np.float64(v))
        elif isinstance(v, tuple) and v and isinstance(v[0], np.float32):
            setattr(mod, name, tuple(np.float64(x) for x in v))
    mod.sincos32 = lambda x: (np.sin(np.asarray(x, np.float64)), np.cos(np.asarray(x, np.float64)))
    return mod


def oracle(n, vit, pit, max_ep_len=1000, mod=L3):
    return mod.Lander3Oracle(n, seed=SEED, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


def heuristic(s):
    """gym's lunar_lander heuristic controller (tools/gen_lander3_golden.py's)."""
    angle_targ = np.clip(s[:, 0] * 0.5 + s[:, 2] * 1.0, -0.4, 0.4)
    hover_targ = 0.55 * np.abs(s[:, 0])
    angle_todo = (angle_targ - s[:, 4]) * 0.5 - s[:, 5] * 1.0
    hover_todo = (hover_targ - s[:, 1]) * 0.5 - s[:, 3] * 0.5
    legs = (s[:, 6] > 0) | (s[:, 7] > 0)
    angle_todo = np.where(legs, 0, angle_todo)
    hover_todo = np.where(legs, -s[:, 3] * 0.5, hover_todo)
    return np.clip(np.stack([hover_todo * 20 - 1, -angle_todo * 20], 1), -1, 1).astype(F)


# ---- geometry of a state block, in float64 ---------------------------------------------------------------------------------------
def ground(S, wx):
    """Terrain height of each env at world x `wx` [n], with the model's clamped segment index."""
    S = np.asarray(S, np.float64)
    idx = np.clip(np.floor(wx * 0.5), 0, 9).astype(np.int64)
    cols = np.arange(S.shape[1])
    h0, h1 = S[L3.T0 + idx, cols], S[L3.T0 + idx + 1, cols]
    return h0 + (h1 - h0) * (wx - 2.0 * idx) * 0.5


def corners(S):
    """-> world (x, y) [8, n] of the leg corners, q = 4 leg + k in the oracle's CORNERS order."""
    S = np.asarray(S, np.float64)
    xs, ys = [], []
    for b in range(2):
        a = S[LEG(b, 4)]
        for kx, ky in L3.CORNERS:
            cx, cy = kx * float(L3.LEG_HX), ky * float(L3.LEG_HY)
            xs.append(S[LEG(b, 0)] + np.cos(a) * cx - np.sin(a) * cy)
            ys.append(S[LEG(b, 1)] + np.sin(a) * cx + np.cos(a) * cy)
    return np.stack(xs), np.stack(ys)


def hull_vertices(S):
    """-> world (x, y) [6, n] of the hull polygon, from the centre of mass and the angle (the crash test's points)."""
    S = np.asarray(S, np.float64)
    sn, cs = np.sin(S[L3.ANG]), np.cos(S[L3.ANG])
    px, py = S[L3.X] + sn * float(L3.LCY), S[L3.Y] - cs * float(L3.LCY)
    return (np.stack([px + cs * float(F(hx)) - sn * float(F(hy)) for hx, hy in HULL]),
            np.stack([py + sn * float(F(hx)) + cs * float(F(hy)) for hx, hy in HULL]))


def clearance(S, hull=True):
    """Height of the craft's lowest point (leg corners, and the hull's vertices with `hull`) above the terrain under it, [n]."""
    cx, cy = corners(S)
    gaps = [cy[q] - ground(S, cx[q]) for q in range(8)]
    if hull:
        vx, vy = hull_vertices(S)
        gaps += [vy[k] - ground(S, vx[k]) for k in range(6)]
    return np.min(np.stack(gaps), axis=0)


# ---- edits (float64 in, the caller rounds the block once with `finish`) -----------------------------------------------------------
def set_origin(S):
    """PX, PY (body.position) from the centre of mass and the angle."""
    S[L3.PX] = S[L3.X] + np.sin(S[L3.ANG]) * float(L3.LCY)
    S[L3.PY] = S[L3.Y] - np.cos(S[L3.ANG]) * float(L3.LCY)


def rotate(S, theta):
    """Rotate the whole craft rigidly by theta [n] about the hull's centre of mass: positions, angles and velocity vectors."""
    c, s = np.cos(theta), np.sin(theta)
    for b in range(2):
        dx, dy = S[LEG(b, 0)] - S[L3.X], S[LEG(b, 1)] - S[L3.Y]
        S[LEG(b, 0)], S[LEG(b, 1)] = S[L3.X] + c * dx - s * dy, S[L3.Y] + s * dx + c * dy
        vx, vy = S[LEG(b, 2)].copy(), S[LEG(b, 3)].copy()
        S[LEG(b, 2)], S[LEG(b, 3)] = c * vx - s * vy, s * vx + c * vy
        S[LEG(b, 4)] = S[LEG(b, 4)] + theta
    vx, vy = S[L3.VX].copy(), S[L3.VY].copy()
    S[L3.VX], S[L3.VY] = c * vx - s * vy, s * vx + c * vy
    S[L3.ANG] = S[L3.ANG] + theta
    set_origin(S)


def shift(S, dx=0.0, dy=0.0):
    for rows, d in (((L3.X, L3.PX, LEG(0, 0), LEG(1, 0)), dx), ((L3.Y, L3.PY, LEG(0, 1), LEG(1, 1)), dy)):
        for r in rows:
            S[r] = S[r] + d


def lift_to(S, gap, hull=True):
    """Move the craft vertically so that its lowest point is `gap` [n] above the terrain under it."""
    shift(S, dy=gap - clearance(S, hull))


def set_velocity(S, vx=None, vy=None, om=None):
    """One rigid motion for hull and legs: linear velocity (vx, vy) of the hull's centre of mass and spin om about it."""
    for val, hull_row, f in ((vx, L3.VX, 2), (vy, L3.VY, 3), (om, L3.OM, 5)):
        if val is not None:
            S[hull_row] = val
            for b in range(2):
                S[LEG(b, f)] = val
    if om is not None:
        for b in range(2):
            dx, dy = S[LEG(b, 0)] - S[L3.X], S[LEG(b, 1)] - S[L3.Y]
            S[LEG(b, 2)] = S[LEG(b, 2)] - om * dy
            S[LEG(b, 3)] = S[LEG(b, 3)] + om * dx


def finish(S):
    """Round the edited block to float32 once; whole-number fields stay whole."""
    S = np.asarray(S, np.float64).astype(F)
    assert np.isfinite(S).all()
    return np.ascontiguousarray(S)


def tile(S, n):
    """n envs cycling through the columns of S (env i gets column i % S.shape[1])."""
    return np.asarray(S, np.float64)[:, np.arange(n) % S.shape[1]].copy()


# ---- census ----------------------------------------------------------------------------------------------------------------------
def census_of(before, last, rew, ended, max_ep_len, pit):
    """One step's classes -> {name: bool [n]}: `before` is the state block the step started from, `last` the oracle's record of
    it, `rew` / `ended` what step() returned."""
    before = np.asarray(before, np.float64)
    after = np.asarray(last["state"], np.float64)
    on = last["on"]
    any_on = on.any(axis=0)
    cl = {}
    for q in range(8):
        cl["contact at corner %d" % q] = on[q]
    cl["contact on a rising segment"] = (on & (last["dh"] > 0)).any(axis=0)
    cl["contact on a falling segment"] = (on & (last["dh"] < 0)).any(axis=0)
    seg = last["seg"]
    span = np.stack([(seg[4 * b:4 * b + 4].max(axis=0) != seg[4 * b:4 * b + 4].min(axis=0)) & on[4 * b:4 * b + 4].any(axis=0) for b in range(2)])
    cl["a leg in contact whose corners span two segments"] = span.any(axis=0)
    cx, _ = corners(before)
    cl["a corner left of the terrain (wx < 0, index clamped to 0)"] = (cx < 0.0).any(axis=0)
    cl["a corner right of the terrain (wx > 20, index clamped to 9)"] = (cx > 20.0).any(axis=0)
    b32 = np.asarray(before, F)
    exact, below, above = (np.zeros(before.shape[1], bool) for _ in range(3))
    for q in range(8):
        px = _corner_x32(b32, q)
        even = (F(2.0) * np.rint(px * F(0.5))).astype(F)
        exact |= on[q] & (px == even)
        below |= on[q] & (px == np.nextafter(even, F(-np.inf)))
        above |= on[q] & (px == np.nextafter(even, F(np.inf)))
    cl["contact at a corner with wx = 2k exactly"] = exact
    cl["contact at a corner one float32 below wx = 2k"] = below
    cl["contact at a corner one float32 above wx = 2k"] = above
    cl["contact with the friction clamp hit"] = (on & last["friction_clamp"]).any(axis=0)
    cl["contact with the friction clamp not hit"] = (on & ~last["friction_clamp"]).any(axis=0)
    warm = np.stack([before[CAN(q)] != 0.0 for q in range(8)]) | np.stack([before[CAT(q)] != 0.0 for q in range(8)])
    was = np.stack([before[L3.C1] > 0] * 4 + [before[L3.C2] > 0] * 4)
    cl["contact new (its leg had none)"] = (on & ~warm & ~was).any(axis=0)
    cl["contact kept with a non-zero warm start"] = (on & warm).any(axis=0)
    cl["contact lost (warm start dropped)"] = (~on & warm).any(axis=0)
    cl["leg 0 lower limit positive"] = last["limit_lo"][0]
    cl["leg 1 upper limit positive"] = last["limit_up"][1]
    cl["leg 0 upper limit positive (far side)"] = last["limit_up"][0]
    cl["leg 1 lower limit positive (far side)"] = last["limit_lo"][1]
    cl["leg 0 upper limit: warm start > 0 (injected or carried)"] = before[JNT(0, 4)] > 0
    cl["leg 1 lower limit: warm start > 0 (injected or carried)"] = before[JNT(1, 3)] > 0
    for b in range(2):
        cl["leg %d motor clamped at +0.8" % b] = last["motor_hi"][b]
        cl["leg %d motor clamped at -0.8" % b] = last["motor_lo"][b]
    sw, solved = last["sweeps"], last["solved"]
    cl["position loop left after 1 sweep"] = solved & (sw == 1)
    cl["position loop left at an intermediate sweep"] = solved & (sw > 1) & (sw < pit)
    cl["position loop run to the end unsolved"] = ~solved
    cl["SLEEP incremented"] = after[L3.SLEEP] > before[L3.SLEEP]
    cl["SLEEP reset from > 0"] = (before[L3.SLEEP] > 0) & (after[L3.SLEEP] == 0)
    cl["+100 rest reward"] = np.asarray(rew) == 100.0
    vx, vy = hull_vertices(after)
    under = np.stack([vy[k] < ground(after, vx[k]) for k in range(6)])
    for k in range(6):
        cl["crash by hull vertex %d" % k] = last["crash"] & under[k]
    o0 = (after[L3.PX] - 10.0) / 10.0
    cl["viewport exit left"] = last["out"] & (o0 <= -1.0)
    cl["viewport exit right"] = last["out"] & (o0 >= 1.0)
    cl["time limit"] = (before[L3.EPLEN] + 1 >= max_ep_len) & np.asarray(ended).astype(bool)
    cl["main engine off"], cl["main engine on"] = last["m_power"] == 0, last["m_power"] > 0
    cl["side engine off"], cl["side engine on"] = last["s_power"] == 0, last["s_power"] > 0
    cl["_any contact"] = any_on
    return cl


FAR_SIDE = ("leg 0 upper limit positive (far side)", "leg 1 lower limit positive (far side)")
INJECTED = {"leg 0 upper limit positive (far side)": "leg 0 upper limit: warm start > 0 (injected or carried)",
            "leg 1 lower limit positive (far side)": "leg 1 lower limit: warm start > 0 (injected or carried)"}


def run_oracle(scn, mod=L3):
    """Run a scenario through the (float32) oracle.  -> dict: per step the five outputs, the `last` records and the before-states,
    the final state block and stats()."""
    S0, acts, (vit, pit, max_ep_len) = scn
    ora = oracle(S0.shape[1], vit, pit, max_ep_len, mod)
    ora.S[:] = S0
    out = {"outs": [], "last": [], "before": []}
    for t in range(acts.shape[0]):
        out["before"].append(ora.S.copy())
        out["outs"].append(ora.step(acts[t]))
        out["last"].append(ora.last)
    out["final"], out["stats"], out["oracle"] = ora.S.copy(), ora.stats(), ora
    return out


def census(scn, run=None):
    """-> (counts {class: env-steps}, lanes {class: set of lane positions modulo 64}, waves: number of (step, 64-env group) pairs
    that hold >= 3 different position-sweep counts and both lanes with and without a contact)."""
    return census_record(run or run_oracle(scn), scn[0].shape[1], scn[2][1], scn[2][2])


def census_record(run, n, pit, max_ep_len):
    counts, lanes, waves = {}, {}, 0
    lane = np.arange(n) % 64
    for before, last, outs in zip(run["before"], run["last"], run["outs"]):
        cl = census_of(before, last, outs[1], outs[4], max_ep_len, pit)
        for k, m in cl.items():
            counts[k] = counts.get(k, 0) + int(m.sum())
            lanes.setdefault(k, set()).update(lane[m].tolist())
        for g0 in range(0, n, 64):
            g = slice(g0, min(g0 + 64, n))
            c = cl["_any contact"][g]
            waves += int(len(set(last["sweeps"][g].tolist())) >= 3 and c.any() and not c.all())
    return counts, lanes, waves


# the parameter sets of tests/test_gpu_lander3.py::test_env3_bit_exact_vs_live_oracle (8 / 3 iterations)
LIVE_MATRIX = [(64, 1, "heuristic", 300, 160), (33, 7, "random", 200, 1000), (1, 3, "zero", 150, 1000), (4096, 11, "random", 20, 12)]


def live_matrix_census():
    """The census of that test's four runs, replayed on the oracle alone -> lines of the table."""
    tot, lanes_all, steps = {}, {}, 0
    for n, seed, policy, T, max_len in LIVE_MATRIX:
        ora = L3.Lander3Oracle(n, seed=seed, max_ep_len=max_len, velocity_iterations=FAST[0], position_iterations=FAST[1])
        rec = record_steps(ora)
        rs = np.random.RandomState(seed)
        o = ora.obs()
        for _ in range(T):
            a = heuristic(o) if policy == "heuristic" else (rs.uniform(-1.3, 1.3, (n, 2)).astype(F) if policy == "random" else np.zeros((n, 2), F))
            o = ora.step(a)[3]
        counts, lanes, _ = census_record(rec, n, FAST[1], max_len)
        steps += n * T
        for k in counts:
            tot[k] = tot.get(k, 0) + counts[k]
            lanes_all.setdefault(k, set()).update(lanes[k])
    lines = ["== live matrix: the four parameter sets of tests/test_gpu_lander3.py::test_env3_bit_exact_vs_live_oracle at 8 / 3 iterations,",
             "   %d env-steps, replayed on the oracle alone (python tests/_lander3_scenarios.py rewrites this part)" % steps,
             "%-62s %7s %5s" % ("class", "total", "lanes")]
    lines += ["%-62s %7d %5d" % (k, tot[k], len(lanes_all[k])) for k in tot if not k.startswith("_")]
    return lines


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pose_cached(n):
    """n airborne crafts with their legs closed onto the joint limits (12 free-fall steps at 20 / 10 from the reset), turned upright,
    at rest, episode length 0; each env keeps its own reset terrain (flat helipad on 6 <= x <= 14)."""
    o = oracle(n, 20, 10)
    z = np.zeros((n, 2), F)
    for _ in range(12):
        o.step(z)
    S = o.S.astype(np.float64)
    set_velocity(S, 0.0, 0.0, 0.0)
    rotate(S, -S[L3.ANG])
    S[L3.EPLEN] = 0.0
    return S


def pose(n):
    return _pose_cached(n).copy()


@functools.lru_cache(maxsize=None)
def _landed_cached():
    """Crafts standing on the helipad at gym's 180 / 60, 46 steps after a 3 cm drop, with the SLEEP counter running (3 .. 20)."""
    S = pose(8)
    shift(S, dx=10.0 - S[L3.X])
    lift_to(S, 0.03)
    o = oracle(8, *GYM)
    o.S[:] = finish(S)
    z = np.zeros((8, 2), F)
    for _ in range(46):
        assert not o.step(z)[4].any()
    keep = (o.S[L3.SLEEP] >= 3) & (o.S[L3.SLEEP] <= 20)   # the envs that have come to rest by now
    assert keep.sum() >= 4, o.S[L3.SLEEP]
    return o.S[:, keep].astype(np.float64)


def landed(n):
    return tile(_landed_cached(), n)


def fresh(n):
    """The reset state itself (airborne at the top, random initial velocity)."""
    return oracle(n, *FAST).S.astype(np.float64)


def rough(S, rs, lo=1.0, hi=6.0):
    for i in range(11):
        S[L3.T0 + i] = rs.uniform(lo, hi, S.shape[1])


def tumble(n, rs, rough_terrain=True, x=(1.5, 18.5), gap=(0.05, 0.7), vy=(-8.0, 0.0)):
    """Crafts at a random attitude over (rough) terrain, close to it, with a random rigid motion."""
    S = pose(n)
    if rough_terrain:
        rough(S, rs)
    shift(S, dx=rs.uniform(x[0], x[1], n) - S[L3.X])
    rotate(S, rs.uniform(-np.pi, np.pi, n))
    lift_to(S, rs.uniform(gap[0], gap[1], n))
    set_velocity(S, rs.uniform(-3, 3, n), rs.uniform(vy[0], vy[1], n), rs.uniform(-3, 3, n))
    return S


def interleave(blocks, n):
    """Env i takes column i of block i % len(blocks): classes interleaved inside every 64-lane group."""
    S = np.empty((L3.NF3, n), np.float64)
    for k, b in enumerate(blocks):
        assert b.shape == (L3.NF3, n)
        S[:, k::len(blocks)] = b[:, k::len(blocks)]
    return S


def _cls(n, k):
    return np.arange(n) % k


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------
def rest_gym():
    """180 / 60.  Classes (env id % 8): standing with SLEEP forced to 24, to 23, as snapshot (counter running), forced to 0; a fresh
    airborne env; standing with the main engine at full power (lifts off: contacts lost, SLEEP reset); standing at SLEEP = 24 with a
    hull velocity above the sleep tolerance (reset from 24, no reward); a tilted drop (theta 0.5, 0.65 up, vy -4)."""
    n, T = 64, 12
    c = _cls(n, 8)
    blocks = [landed(n) for _ in range(4)] + [fresh(n), landed(n), landed(n), pose(n)]
    blocks[0][L3.SLEEP], blocks[1][L3.SLEEP], blocks[3][L3.SLEEP], blocks[6][L3.SLEEP] = 24.0, 23.0, 0.0, 24.0
    blocks[6][L3.VX] = blocks[6][L3.VX] + 0.3
    d = blocks[7]
    shift(d, dx=10.0 - d[L3.X])
    rotate(d, np.full(n, 0.5))
    lift_to(d, 0.65)
    set_velocity(d, vy=-4.0)
    acts = np.zeros((T, n, 2), F)
    acts[:, c == 5, 0] = 1.0
    acts[:, c == 4] = np.random.RandomState(1).uniform(-1.3, 1.3, (T, int((c == 4).sum()), 2))
    return finish(interleave(blocks, n)), acts, GYM + (1000,)


def rest_forced():
    """8 / 3 from states that stand at 180 / 60.  Classes (env id % 8): SLEEP forced to 24 (+100 on the first step), 23, the
    snapshot's own counter (keeps counting for a few steps, then the 8-sweep solve lets the hull sag: SLEEP resets), 20, a fresh
    airborne env, a tumbling drop, SLEEP = 24 with a side engine firing, SLEEP = 0."""
    n, T = 128, 30
    c = _cls(n, 8)
    rs = np.random.RandomState(2)
    blocks = [landed(n) for _ in range(4)] + [fresh(n), tumble(n, rs), landed(n), landed(n)]
    for k, v in ((0, 24.0), (1, 23.0), (3, 20.0), (6, 24.0), (7, 0.0)):
        blocks[k][L3.SLEEP] = v
    acts = np.zeros((T, n, 2), F)
    acts[:, c == 6, 1] = np.where(np.arange(int((c == 6).sum())) % 2 == 0, 1.0, -1.0)
    acts[:, c == 5] = rs.uniform(-1.3, 1.3, (T, int((c == 5).sum()), 2))
    return finish(interleave(blocks, n)), acts, FAST + (1000,)


def tilted_drops():
    """8 / 3.  Classes (env id % 16): theta in (+0.5, -0.5, +1.5, -1.5) x vy in (0, -4, -8) over the flat helipad, lowest body 0.6
    to 0.75 up; the last four are random attitudes over rough terrain (the inner top corners 3 and 6 are reached there: a craft on
    its side or back over a ridge)."""
    n, T = 256, 40
    c = _cls(n, 16)
    rs = np.random.RandomState(3)
    blocks = []
    for th in (0.5, -0.5, 1.5, -1.5):
        for vy in (0.0, -4.0, -8.0):
            S = pose(n)
            shift(S, dx=8.0 + 4.0 * ((np.arange(n) // 16) % 5) / 4.0 - S[L3.X])
            rotate(S, np.full(n, th))
            lift_to(S, 0.6 + 0.15 * ((np.arange(n) // 16) % 4) / 3.0)
            set_velocity(S, vy=vy)
            blocks.append(S)
    blocks += [tumble(n, rs) for _ in range(4)]
    acts = np.zeros((T, n, 2), F)
    acts[:, c >= 12] = rs.uniform(-1.3, 1.3, (T, int((c >= 12).sum()), 2))
    return finish(interleave(blocks, n)), acts, FAST + (1000,)


def _corner_x32(S, q):
    """World x of corner q as the float32 step computes it (lg.x + (cb cx - sb cy))."""
    b, k = divmod(q, 4)
    sb, cb = L3.sincos32(S[LEG(b, 4)])
    cx, cy = F(L3.CORNERS[k][0]) * L3.LEG_HX, F(L3.CORNERS[k][1]) * L3.LEG_HY
    return (S[LEG(b, 0)] + (cb * cx - sb * cy)).astype(F)


def on_boundary(S, q, side):
    """float32 block in, float32 block out: move leg q // 4 in x by a few ulps so that corner q's world x, as the step computes it,
    is an even integer exactly (side 0), the float32 below it (-1) or above it (+1)."""
    S = S.copy()
    b = q // 4
    target = (F(2.0) * np.rint(_corner_x32(S, q) * F(0.5))).astype(F)
    want = target if side == 0 else np.nextafter(target, F(-np.inf) if side < 0 else F(np.inf)).astype(F)
    for _ in range(16):   # where round-to-even steps over the wanted value, turn the leg by one float32 and walk again
        for _ in range(16):
            px = _corner_x32(S, q)
            row = S[LEG(b, 0)]
            S[LEG(b, 0)] = np.where(px < want, np.nextafter(row, F(np.inf)), np.where(px > want, np.nextafter(row, F(-np.inf)), row)).astype(F)
        bad = _corner_x32(S, q) != want
        if not bad.any():
            break
        S[LEG(b, 4)] = np.where(bad, np.nextafter(S[LEG(b, 4)], F(np.inf)), S[LEG(b, 4)]).astype(F)
    assert (_corner_x32(S, q) == want).all()
    return S


def slopes_edges():
    """8 / 3.  Classes (env id % 16): 0-3 short drops onto a uniform slope of +1, -1, +0.3, -0.3 per chunk, placed so that legs
    straddle chunk boundaries; 4-6 a penetrating bottom corner whose world x is 2k exactly / one float32 below / above, on rough
    terrain; 7 / 8 low over the terrain's left / right end, drifting out (corners at wx < 0 / > 20, then the viewport exit); 9 / 10
    airborne within one step of |o[0]| = 1; 11-15 random attitudes over rough terrain."""
    n, T = 256, 40
    c = _cls(n, 16)
    rs = np.random.RandomState(4)
    idx = np.arange(n) // 16
    blocks = []
    for slope in (1.0, -1.0, 0.3, -0.3):
        S = pose(n)
        for i in range(11):
            S[L3.T0 + i] = 6.0 + slope * (i - 5)
        shift(S, dx=(4.0 + 2.0 * (idx % 5) + 0.35 * (idx % 7) - 0.9) - S[L3.X])
        rotate(S, np.full(n, 0.12) * np.sign(slope))
        lift_to(S, 0.1)
        set_velocity(S, vy=-2.0)
        blocks.append(S)
    edge = []
    for side in (0, -1, 1):
        S = pose(n)
        rough(S, rs, 3.0, 4.0)
        cx, _ = corners(S)
        shift(S, dx=np.array([6.0, 10.0, 12.0, 14.0])[(idx // 2) % 4] - np.where(idx % 2 == 0, cx[1], cx[4]))   # not 4, 8, 16: the
        cx, cy = corners(S)                                                          # float32 spacing changes there
        shift(S, dy=-0.01 - np.where(idx % 2 == 0, cy[1] - ground(S, cx[1]), cy[4] - ground(S, cx[4])))   # that corner penetrates
        edge.append(S)
        blocks.append(S)
    for x0, vx in ((0.9, -3.0), (19.1, 3.0), (0.05, -3.0), (19.95, 3.0)):
        S = pose(n)
        for i in range(11):
            S[L3.T0 + i] = 3.0 + 0.4 * ((i + idx) % 3)
        shift(S, dx=x0 - S[L3.PX])
        lift_to(S, 0.05 if x0 in (0.9, 19.1) else 3.0)
        set_velocity(S, vx=vx, vy=-1.0)
        blocks.append(S)
    blocks += [tumble(n, rs) for _ in range(5)]
    S = finish(interleave(blocks, n))
    # the boundary edits are made on the rounded block: corner 1 (leg 0) on even envs, corner 4 (leg 1) on odd ones
    for k, side in ((4, 0), (5, -1), (6, 1)):
        for q, par in ((1, 0), (4, 1)):
            cols = np.nonzero((c == k) & (idx % 2 == par))[0]
            S[:, cols] = on_boundary(S[:, cols], q, side)
    acts = np.zeros((T, n, 2), F)
    acts[:, c >= 11] = rs.uniform(-1.3, 1.3, (T, int((c >= 11).sum()), 2))
    return S, acts, FAST + (1000,)


def joint_limits():
    """8 / 3.  Injected warm starts (env id % 8): 0 airborne with the FAR-side limit rows loaded (leg 0 upper, leg 1 lower = 0.5);
    1 touching down with the motors at their clamp (+0.8 / -0.8); 2 / 3 motors beyond it (+1.5 / -1.5 and -1.5 / +1.5); 4 airborne
    with every contact slot loaded (dropped: no corner is a contact point); 5 penetrating with every contact slot loaded (kept on
    the corners in contact, dropped on the others); 6 / 7 random attitudes over rough terrain — side and top impacts fold a leg
    inward once contact torque saturates the motor: the far-side rows load dynamically there."""
    n, T = 128, 24
    c = _cls(n, 8)
    rs = np.random.RandomState(5)

    def pad(gap):
        S = pose(n)
        shift(S, dx=10.0 - S[L3.X])
        lift_to(S, gap)
        return S
    blocks = [pose(n), pad(0.02), pad(0.02), pad(0.02), pose(n), pad(-0.01), tumble(n, rs), tumble(n, rs)]
    blocks[0][JNT(0, 4)], blocks[0][JNT(1, 3)] = 0.5, 0.5
    blocks[1][JNT(0, 2)], blocks[1][JNT(1, 2)] = 0.8, -0.8
    blocks[2][JNT(0, 2)], blocks[2][JNT(1, 2)] = 1.5, -1.5
    blocks[3][JNT(0, 2)], blocks[3][JNT(1, 2)] = -1.5, 1.5
    for k in (4, 5):
        for q in range(8):
            blocks[k][CAN(q)] = 0.05 + 0.01 * q
            blocks[k][CAT(q)] = 0.004 * (q - 3.5)
        blocks[k][L3.C1] = blocks[k][L3.C2] = 1.0
    acts = np.zeros((T, n, 2), F)
    acts[:, c >= 6] = rs.uniform(-1.3, 1.3, (T, int((c >= 6).sum()), 2))
    return finish(interleave(blocks, n)), acts, FAST + (1000,)


def spin():
    """8 / 3.  Classes (env id % 4): the whole craft turned by +-20 .. +-60 rad and spinning at +-8 rad/s, high up; the same 0.5
    above rough terrain; a fresh env; a random attitude over rough terrain.  sincos32's quadrant count k runs into the tens."""
    n, T = 128, 30
    c = _cls(n, 4)
    rs = np.random.RandomState(6)
    turn = np.where(np.arange(n) % 8 < 4, 1.0, -1.0) * (20.0 + 40.0 * ((np.arange(n) // 8) % 5) / 4.0)
    hi = pose(n)
    rotate(hi, turn)
    set_velocity(hi, om=8.0 * np.sign(turn))
    lo = pose(n)
    rough(lo, rs)
    shift(lo, dx=rs.uniform(3, 17, n) - lo[L3.X])
    rotate(lo, -turn + 0.3)
    lift_to(lo, 0.5)
    set_velocity(lo, vy=-3.0, om=-8.0 * np.sign(turn))
    acts = rs.uniform(-1.3, 1.3, (T, n, 2)).astype(F)
    return finish(interleave([hi, lo, fresh(n), tumble(n, rs)], n)), acts, FAST + (1000,)


# actions at and around the engines' thresholds and outside the clip range
SPECIAL_ACTIONS = np.array([(0.0, 0.5), (np.nextafter(F(0), F(1)), np.nextafter(F(0.5), F(1))), (-0.0, -0.5),
                            (1.5, -np.nextafter(F(0.5), F(1))), (-1.5, 2.0), (1.0, -1.0), (1e-3, -7.0), (40.0, 0.49999997)], F)


def endings():
    """8 / 3, max_ep_len 9.  Classes (env id % 12): 0-5 the hull turned so that vertex k is its lowest point, 0.05 above flat ground, falling at vy -6
    (the crash test's six vertices); 6 airborne with EPLEN = max - 1; 7 / 8 airborne one step inside the left / right viewport
    edge; 9-11 fresh envs.  Every env's action walks through SPECIAL_ACTIONS; the envs that survive meet the time limit."""
    n, T, max_ep_len = 192, 16, 9
    idx = np.arange(n) // 12
    blocks = []
    for k in range(6):
        # the direction in which vertex k is the hull's lowest point: between the outward normals of its two edges
        (x0, y0), (x1, y1), (x2, y2) = HULL[k - 1], HULL[k], HULL[(k + 1) % 6]
        n1, n2 = np.array([y1 - y0, x0 - x1]), np.array([y2 - y1, x1 - x2])
        d = n1 / np.hypot(*n1) + n2 / np.hypot(*n2)
        S = pose(n)
        for i in range(11):
            S[L3.T0 + i] = 3.0 + 0.25 * (idx % 4)
        shift(S, dx=4.0 + (idx % 7) * 2.0 + 0.3 - S[L3.X])
        rotate(S, np.full(n, -np.pi / 2 - np.arctan2(d[1], d[0])) + 0.02 * (idx % 3 - 1))
        vx, vy = hull_vertices(S)
        shift(S, dy=0.05 - (vy[k] - ground(S, vx[k])))   # the legs may start inside the ground: the crash comes first
        set_velocity(S, vy=-6.0)
        blocks.append(S)
    S = pose(n)
    S[L3.EPLEN] = max_ep_len - 1.0
    blocks.append(S)
    for x0, vx in ((0.04, -3.0), (19.96, 3.0)):
        S = pose(n)
        shift(S, dx=x0 - S[L3.PX])
        set_velocity(S, vx=vx)
        blocks.append(S)
    blocks += [fresh(n) for _ in range(3)]
    t, i = np.meshgrid(np.arange(T), np.arange(n), indexing="ij")
    acts = SPECIAL_ACTIONS[(t + i) % len(SPECIAL_ACTIONS)]
    return finish(interleave(blocks, n)), np.ascontiguousarray(acts), FAST + (max_ep_len,)


def mixed():
    """8 / 3: drops + forced rest + spin, interleaved (env id % 8), for the launch paths that choose their own actions — with the
    engines off, classes 0 / 1 leave by the +100 rest exit in the first two steps while 2-5 are in or near contact and 6 / 7 are not."""
    n, T = 128, 12
    rs = np.random.RandomState(8)
    a, b = landed(n), landed(n)
    a[L3.SLEEP], b[L3.SLEEP] = 24.0, 23.0
    drops = []
    for th, vy in ((0.5, -4.0), (-1.5, -8.0)):
        S = pose(n)
        shift(S, dx=10.0 - S[L3.X])
        rotate(S, np.full(n, th))
        lift_to(S, 0.1)
        set_velocity(S, vy=vy)
        drops.append(S)
    turn = np.where(np.arange(n) % 16 < 8, 1.0, -1.0) * (25.0 + 5.0 * ((np.arange(n) // 16) % 8))
    sp = pose(n)
    rotate(sp, turn)
    set_velocity(sp, om=8.0 * np.sign(turn))
    acts = np.zeros((T, n, 2), F)
    return finish(interleave([a, b] + drops + [tumble(n, rs), tumble(n, rs), sp, fresh(n)], n)), acts, FAST + (1000,)


SCENARIOS = {f.__name__: functools.lru_cache(maxsize=None)(f)
             for f in (rest_gym, rest_forced, tilted_drops, slopes_edges, joint_limits, spin, endings, mixed)}

# class -> reason.  Only the two dynamic far-side limit classes may ever be named here (tests/test_lander3_scenarios_cpu.py checks
# it).  Empty: random attitudes over rough terrain reach both (a leg that lands on its outer face or its top is folded inward by
# the contact torque, the motor saturates at 0.8, the far row loads), in tilted_drops, slopes_edges and joint_limits.
UNREACHED = {}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """Scenario `name` through the float32 oracle, computed once and shared (read-only) by the tests that compare against it."""
    return run_oracle(SCENARIOS[name]())


def record_steps(ora):
    """Wrap ora.step so that every call is recorded as run_oracle records it; -> the record (for oracles driven by a helper that
    feeds them the GPU's own actions)."""
    rec = {"before": [], "last": [], "outs": []}
    step = ora.step

    def recording(act):
        rec["before"].append(ora.S.copy())
        out = step(act)
        rec["outs"].append(out)
        rec["last"].append(ora.last)
        return out
    ora.step = recording
    return rec


def waves_with_contact_rest_exit_and_free_lane(rec):
    """Number of (step, 64-env group) pairs of a recorded run that hold a lane in contact, a lane leaving by the +100 rest exit and a
    lane without any contact."""
    count = 0
    for last, outs in zip(rec["last"], rec["outs"]):
        contact, rest = last["on"].any(axis=0), last["asleep"] & ~last["out"]
        assert (np.asarray(outs[1])[rest] == 100.0).all()
        for g0 in range(0, contact.shape[0], 64):
            g = slice(g0, g0 + 64)
            count += int(contact[g].any() and rest[g].any() and not contact[g].all())
    return count


if __name__ == "__main__":   # rewrite the live-matrix part of profiles/lander3_census.txt (the scenario part is the CPU test's)
    path = os.path.join(ROOT, "profiles", "lander3_census.txt")
    old = open(path).read().splitlines() if os.path.exists(path) else []
    mark = [i for i, ln in enumerate(old) if ln.startswith("== scenario library")]
    with open(path, "w") as f:
        f.write("\n".join(live_matrix_census() + [""] + (old[mark[0]:] if mark else [])) + "\n")
