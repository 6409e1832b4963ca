"""TEST INFRASTRUCTURE: crafted start states for the bipedal walker (tests/walker_oracle.py, csrc/walker_device.h) and the census of the
solver branches a run reaches.

`build()` -> (state block [286, N] float32, actions [T, N, 4] float32).  The block is injected into the oracle (`ora.S[:] = block`) and
into the kernel (`env.set_state`); both sides are created with seed SEED, which only feeds the resets.  A pose is built in float64 from
the hull's origin and angle and the four joint angles (the bodies' centres follow from the anchors, so every joint starts closed), then
lifted so that its lowest leg corner (or hull vertex) has a chosen gap to the terrain under it.  Env e holds class e % len(CLASSES): the
classes are INTERLEAVED, so every 64-lane wave holds every class and its lanes diverge.

`census_of(ora)` turns the oracle's per-step record (`WalkerOracle.last`, `last_ray_segment`) into named classes; `trajectory(vit, pit)`
runs the oracle once per iteration pair and is shared by tests/test_walker_cpu.py (the floor under every class) and
tests/test_gpu_walker_scenarios.py (the kernel's parity on the same trajectory).
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import walker_oracle as W   # noqa: E402

F = np.float32
SEED = 17
FAST = (8, 3)      # the live tests' iteration counts
GYM = (180, 60)    # gym's
N, T = 96, 6       # one and a half waves; steps per trajectory
MAX_EP_LEN = 1600
LEG = lambda b, f: W.L0 + 6 * (b - 1) + f            # body b = 1..4; f: 0 x, 1 y, 2 vx, 3 vy, 4 ang, 5 om   # noqa: E731
HYf, LDf, STEPf, THf = float(W.HY), float(W.LEG_DOWN), float(W.STEP), float(W.TH)


def _far(x, y, a, h=2.0 * HYf):
    """The point `h` down the local -y axis of a box at angle a from (x, y)."""
    return x + h * np.sin(a), y - h * np.cos(a)


def pose(x, y, ang, hip0, knee0, hip1, knee1, vx=0.0, vy=0.0):
    """-> dict of the 16 + 24 pose fields of one env in float64: hull origin (x, y) at angle `ang`, joints at the given angles."""
    c, s = np.cos(ang), np.sin(ang)
    out = {W.PX: x, W.PY: y, W.ANG: ang, W.VX: vx, W.VY: vy, W.OM: 0.0,
           W.X: x + c * float(W.LCX) - s * float(W.LCY), W.Y: y + s * float(W.LCX) + c * float(W.LCY)}
    ax, ay = x - s * LDf, y + c * LDf                     # the hip anchor: R (0, LEG_DOWN)
    for leg, (hip, knee) in enumerate(((hip0, knee0), (hip1, knee1))):
        up, lo = 1 + 2 * leg, 2 + 2 * leg
        a = ang + hip
        ux, uy = _far(ax, ay, a, HYf)
        kx, ky = _far(ax, ay, a)
        b = a + knee
        lx, ly = _far(kx, ky, b, HYf)
        for body, (bx, by, ba) in ((up, (ux, uy, a)), (lo, (lx, ly, b))):
            out.update({LEG(body, 0): bx, LEG(body, 1): by, LEG(body, 2): vx, LEG(body, 3): vy, LEG(body, 4): ba, LEG(body, 5): 0.0})
    return out


def ground(terr, wx):
    idx = int(np.clip(np.floor(wx / STEPf), 0, W.NT - 2))
    return terr[idx] + (terr[idx + 1] - terr[idx]) * (wx - idx * STEPf) / STEPf


def corner_gaps(p, terr):
    """Height of the 8 contact corners above the terrain under them (q = 2 (body - 1) + k)."""
    gaps = []
    for b in range(1, 5):
        a = p[LEG(b, 4)]
        for sx in (-1.0, 1.0):
            cx, cy = sx * float(W.HX[b]), -HYf
            wx = p[LEG(b, 0)] + np.cos(a) * cx - np.sin(a) * cy
            wy = p[LEG(b, 1)] + np.sin(a) * cx + np.cos(a) * cy
            gaps.append(wy - ground(terr, wx))
    return np.array(gaps)


def hull_gaps(p, terr):
    c, s = np.cos(p[W.ANG]), np.sin(p[W.ANG])
    return np.array([p[W.PY] + s * float(hx) + c * float(hy) - ground(terr, p[W.PX] + c * float(hx) - s * float(hy)) for hx, hy in W.HULLV])


def lift(p, terr, gap, of=corner_gaps):
    """Shift the pose vertically so that its lowest corner (or hull vertex) is `gap` above the terrain under it."""
    dy = gap - float(of(p, terr).min())
    for f in [W.Y, W.PY] + [LEG(b, 1) for b in range(1, 5)]:
        p[f] += dy
    return p


FLAT = np.full(W.NT, THf)
SLOPE = FLAT.copy()
SLOPE[8:16] = THf + 0.18 * np.arange(8)            # a ramp of 0.18 per segment from point 8 on, then a drop back to the pad's height
SAW = FLAT + 0.12 * (np.arange(W.NT) % 2)          # every segment sloped, the sign alternating: corners on both slopes and across edges


def _classes():
    """name -> (pose, terrain, action [4] or [T, 4]).  Gaps of 0.01 are inside the contact radius (0.02): the point is active at step 0."""
    stand = lambda x, terr, gap=0.01, **kw: lift(pose(x, 6.0, 0.0, 0.05, -0.15, 0.05, -0.15, **kw), terr, gap)   # noqa: E731
    c = {}
    # joints beyond their limits in free flight, motors pushing further out: (hip 0, knee 0) low + (hip 1, knee 1) high, and swapped
    c["limits_lo_up"] = (lift(pose(10.0, 6.0, 0.0, -0.86, -1.66, 1.16, -0.04), FLAT, 2.0), FLAT, [-1.0, -1.0, 1.0, 1.0])
    c["limits_up_lo"] = (lift(pose(10.0, 6.0, 0.0, 1.16, -0.04, -0.86, -1.66), FLAT, 2.0), FLAT, [1.0, 1.0, -1.0, -1.0])
    # kneeling: thighs back and down, shins folded up behind them — the knee corners carry the body, the feet are in the air
    c["kneeling"] = (lift(pose(10.0, 6.0, 0.0, -0.6, -1.5, -0.5, -1.55), FLAT, 0.01), FLAT, [0.0, 0.0, 0.0, 0.0])
    # feet on the ramp: foot 0 centred on terrain point 10 (its corners on two segments), the other one segment further up
    c["slope_edge"] = (lift(pose(10 * STEPf, 6.0, 0.0, 0.0, -0.12, 0.42, -0.3), SLOPE, 0.005), SLOPE, [0.2, -0.3, -0.2, 0.3])
    c["sawtooth"] = (stand(21 * STEPf + 0.03, SAW, vx=0.8), SAW, [0.6, 0.4, -0.6, -0.4])
    # the hull's nose vertex under the terrain: nose down, legs folded away
    c["hull_crash"] = (lift(pose(12.0, 6.0, -1.5, 1.1, -1.6, 1.1, -1.6, vy=-1.0), FLAT, -0.01, of=hull_gaps), FLAT, [0.0, 0.0, 0.0, 0.0])
    # leaving the terrain at either end
    c["x_negative"] = (stand(0.04, FLAT, gap=0.3, vx=-4.0), FLAT, [0.0, 0.0, 0.0, 0.0])
    c["terrain_end"] = (stand(float(W.XEND) - 0.03, FLAT, gap=0.3, vx=4.0), FLAT, [0.3, 0.3, 0.3, 0.3])
    # lidar: high above the pad every ray misses; low over it the steep rays hit the segment they start over
    c["lidar_all_miss"] = (lift(pose(20.0, 6.0, 0.1, 0.3, -0.5, -0.3, -0.9), FLAT, 4.5), FLAT, [0.5, -0.5, -0.5, 0.5])
    c["lidar_low"] = (lift(pose(30 * STEPf + 0.2, 6.0, 0.0, 1.0, -1.5, -0.7, -1.5), FLAT, 0.05), FLAT, [0.0, 0.0, 0.0, 0.0])
    # standing on the pad with motors saturated against the ground's friction, and zero torque (mmax = 0: the motor row is a no-op)
    c["stand_drive"] = (stand(15.0, FLAT), FLAT, [1.3, -1.3, -1.3, 1.3])
    c["stand_limp"] = (stand(16.0, FLAT), FLAT, [0.0, 0.0, 0.0, 0.0])
    return c


CLASSES = tuple(_classes().keys())


def build():
    cls = _classes()
    ora = W.WalkerOracle(N, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=1, position_iterations=1)
    S = ora.S.copy()
    act = np.zeros((T, N, 4), F)
    for e in range(N):
        p, terr, a = cls[CLASSES[e % len(CLASSES)]]
        p = dict(p)
        dx = 0.011 * (e // len(CLASSES))     # the copies of a class differ a little (not for the poses tied to a terrain point or end)
        if CLASSES[e % len(CLASSES)] in ("limits_lo_up", "limits_up_lo", "kneeling", "lidar_all_miss", "stand_drive", "stand_limp"):
            for f in [W.X, W.PX] + [LEG(b, 0) for b in range(1, 5)]:
                p[f] += dx
        S[:W.T0, e] = 0.0
        for f, v in p.items():
            S[f, e] = F(v)
        S[W.T0:, e] = terr.astype(F)
        S[W.HASP, e], S[W.EPLEN, e], S[W.PSTEP, e] = 1.0, 3.0, 3.0
        S[W.PREV, e] = F(130.0 * p[W.PX] / 30.0 - 5.0 * abs(p[W.ANG]))
        act[:, e] = np.asarray(a, F)
    return S, act


def census_of(ora, counts=None):
    """Add the last step's classes (env-steps per class) to `counts`."""
    L = ora.last
    c = {} if counts is None else counts
    add = lambda k, m: c.__setitem__(k, c.get(k, 0) + int(np.sum(m)))   # noqa: E731
    for j, nm in enumerate(("hip0", "knee0", "hip1", "knee1")):
        add("limit_lo_" + nm, L["limit_lo"][j])
        add("limit_up_" + nm, L["limit_up"][j])
        add("motor_clamped_" + nm, L["motor_hi"][j] | L["motor_lo"][j])
        add("motor_free_" + nm, ~(L["motor_hi"][j] | L["motor_lo"][j]) & (L["mmax"][j] > 0))
        add("motor_zero_torque_" + nm, L["mmax"][j] == 0)
    on = L["on"]
    add("contact_knee", on[0] | on[1] | on[4] | on[5])
    add("contact_foot", on[2] | on[3] | on[6] | on[7])
    add("contact_knee_without_foot", (on[0] | on[1] | on[4] | on[5]) & ~(on[2] | on[3] | on[6] | on[7]))
    add("contact_on_slope", (on & (L["dh"] != 0)).any(0))
    add("contact_foot_across_edge", (on[2] & on[3] & (L["seg"][2] != L["seg"][3])) | (on[6] & on[7] & (L["seg"][6] != L["seg"][7])))
    add("friction_clamped", L["friction_clamp"].any(0))
    add("position_solved_first_sweep", L["solved"] & (L["sweeps"] == 1))
    add("position_solved_later", L["solved"] & (L["sweeps"] > 1))
    add("position_unsolved", ~L["solved"])
    add("game_over", L["game_over"])
    add("x_negative", L["neg_x"])
    add("terrain_end", L["finish"])
    seg = ora.last_ray_segment
    add("lidar_all_miss", (seg < 0).all(1))
    add("lidar_some_miss", (seg < 0).any(1))
    add("lidar_hit_own_segment", (seg == 0).any(1))
    add("lidar_hit_far_segment", (seg >= 6).any(1))
    return c


@functools.lru_cache(maxsize=None)
def trajectory(vit, pit):
    """-> (start block, actions, per-step outputs of WalkerOracle.step, final block, census, per-step records) at (vit, pit)."""
    S, act = build()
    ora = W.WalkerOracle(N, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=vit, position_iterations=pit)
    ora.S[:] = S
    outs, census, recs = [], {}, []
    for t in range(T):
        outs.append([np.array(x) for x in ora.step(act[t])])
        census_of(ora, census)
        recs.append(ora.last)
    return S, act, outs, ora.S.copy(), census, recs
