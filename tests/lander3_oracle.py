"""ORACLE — TEST INFRASTRUCTURE ONLY.

NumPy (float32, vectorised over envs) specification of the ARTICULATED lander behind ddrl_env_create_ex(kind =
DDRL_ENV_ARTICULATED): csrc/env3_device.h mirrors `Lander3Oracle._physics` / `reset` statement by statement.

PARITY UNPINNED, as for the one-body model (oracle/env_oracle.py): gym and Box2D are absent from this image, so no trajectory of this
model is compared with gym's.  The point is the STRUCTURE and the SOLVER BUDGET of gym's lander, not its trajectories.

Kept from gym's published lunar_lander.py (as in the one-body model): observation layout and normalisation, action semantics and clip
rules, engine impulses with dispersion noise applied to the hull (Box2D's ApplyLinearImpulse at the engine's point: the main engine
has a lever arm about the hull's centre of mass too), shaping reward and fuel costs, -100 on crash or on leaving the viewport, +100
at rest, FPS 50, SCALE 30, gravity -10, the 11-chunk terrain with the flat helipad, the random initial impulse, one no-op step
inside reset.  The RNG streams per (seed, env id, episode) are the one-body model's.

New, following Box2D's structure (b2Island::Solve, b2RevoluteJoint, b2ContactSolver; constants of b2Settings.h):
  bodies    hull = gym's six-vertex polygon at density 5 (mass, inertia and centre-of-mass offset from Box2D's polygon mass formulas,
            derivation below), two legs = boxes of half-extents (2/30, 8/30) at density 1.  Legs and hull do not collide (gym
            filters the pair).  X, Y are the hull's CENTRE OF MASS (Box2D's sweep.c); PX, PY its origin (body.position), which the
            observation and the crash test read.
  joints    revolute, hull-local (0, 0) to leg-local (i*20/30, 18/30), i = -1, +1: point constraint as a 2x2 block solve, angle
            limits [0.4, 0.9] / [-0.9, -0.4] as two one-sided rows, motor of max torque 40 at speed 0.3*i; warm-started.
  contacts  the four corners of each leg box against the terrain segment under the corner, with that segment's normal; a corner is
            a contact point while its separation (minus Box2D's two polygon radii, 0.02) is negative.  Friction sqrt(0.2 * 0.1)
            (Box2D's mixing of the leg fixture's default 0.2 and gym's terrain 0.1), restitution 0.  Accumulated normal and tangent
            impulses live in the state and warm-start the next step while the corner stays a contact point.  C1 / C2 are 1 where a
            leg holds a contact point this step.
  hull      keeps the one-body model's vertex-below-terrain crash test and gets NO contact response: a hull contact ends gym's
            episode anyway (game_over), so nothing after it is ever observed.
  step      engine impulses; integrate velocities; initialise and warm-start contacts then joints; `velocity_iterations` sweeps
            (joints, then contacts: tangent before normal); integrate positions; up to `position_iterations` position sweeps
            (contacts, then joints) with Box2D's early exit once min separation >= -3 slop and every joint is within slop — a
            per-env mask here, a per-lane branch in the kernel; sleep test: all three bodies under Box2D's linear (0.01) and
            angular (2 deg/s) sleep tolerances for 0.5 s with the position solve converged gives rest and +100.
Left out of Box2D's step: the maxTranslation / maxRotation clamps of the position integration (2 m and pi/2 per step: never reached
by this craft), and the contact's rolling manifold point (the corner itself is the application point).

The arithmetic follows oracle/env_oracle.py's rules: float32 only, one rounding per operation (no FMA contraction), sqrt / divide
correctly rounded, `sincos32` for every sine and cosine, the counter hash of noise_oracle for every random number.
"""
import numpy as np

from oracle.env_oracle import (DT, FPS, GRAV, H, HELIPAD_Y, HULL, LEG_DOWN, MAIN_POWER, RESET_STREAM, SCALE, SIDE_AWAY, SIDE_H,
                               SIDE_POWER, sincos32)
from oracle.noise_oracle import mix32, u01

F = np.float32
NF3 = 66  # DDRL_ENV3_STATE_FIELDS
# the one-body model's indices are kept where the field exists there (EPI = 13: env.DeviceLunarLander.host_env relies on it)
(X, Y, VX, VY, ANG, OM, C1, C2, PREV, HASP, EPLEN, EPRET, SLEEP, EPI, T0) = range(15)
PSTEP = 25
L0 = 26          # leg b (0: i = -1, 1: i = +1): L0 + 6 b + (x, y, vx, vy, ang, om)
J0 = 38          # joint b: J0 + 5 b + (point impulse x, y, motor, lower limit, upper limit)
K0 = 48          # contact (leg b, corner k): K0 + 2 (4 b + k) + (normal impulse, tangent impulse)
PX, PY = 64, 65  # hull origin (body.position)

# Hull mass data, computed once in float64 by b2PolygonShape::ComputeMass on gym's LANDER_POLY / SCALE =
# [(-14,17), (-17,0), (-17,-10), (17,-10), (17,0), (14,17)] / 30 at density 5 (triangle fan about v0: area = sum D/2, centroid =
# sum area_k (e1 + e2) / 3 / area, I_ref = sum D/12 (e1.e1 + e1.e2 + e2.e2) per axis, moved to the centroid by the parallel-axis
# theorem as b2Body::ResetMassData does):
#   area 0.96333333..., mass 4.81666666..., centre (0, 0.10130718954248374), inertia about the centre 0.7838806584362139
INV_MH = F(0.20761245)   # 1 / 4.8166666...
INV_IH = F(1.2757044)    # 1 / 0.78388065...
LCY = F(0.10130719)      # hull-local centre of mass (x component 0 by symmetry)
# Legs: box 4/30 x 16/30 at density 1: mass 64/900, inertia m (hx^2 + hy^2) / 3 = 0.0017909465...
INV_ML = F(14.0625)
INV_IL = F(558.36395)
AXM = F(0.001786864)     # 1 / (INV_IH + INV_IL): the joint's axial mass
LEG_HX, LEG_HY = F(0.06666667), F(0.26666668)
ANCX, ANCY = F(0.6666667), F(0.6)   # leg-local anchor (i * 20/30, 18/30)
LEG_X0 = F(0.6666667)               # legs start at x = 10 - i * 20/30
LEG_A0 = F(0.05)                    # ... with angle 0.05 i
MOTOR_SPEED = F(0.3)
MAX_MOTOR_IMP = F(0.8)              # DT * 40
LIM_LO = (F(0.4), F(-0.9))
LIM_UP = (F(0.9), F(-0.4))
MU = F(0.14142136)                  # sqrt(0.2 * 0.1)
RADIUS = F(0.02)                    # 2 * b2_polygonRadius
SLOP = F(0.005)                     # b2_linearSlop
SLOP3 = F(-0.015)                   # -3 * b2_linearSlop
ASLOP = F(0.034906585)              # b2_angularSlop = 2 deg
MAXLC = F(0.2)                      # b2_maxLinearCorrection
MAXAC = F(0.13962634)               # b2_maxAngularCorrection = 8 deg
BAUM = F(0.2)                       # b2_baumgarte
INV_DT = F(50.0)
SLEEP_LIN2 = F(0.0001)              # b2_linearSleepTolerance^2
SLEEP_ANG2 = F(0.0012184697)        # b2_angularSleepTolerance^2 (2 deg/s)
SLEEP_STEPS = F(25.0)               # b2_timeToSleep * FPS
SIGN = (F(-1.0), F(1.0))            # i of leg 0, leg 1
CORNERS = ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0))


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi).astype(F)


class _Body:
    """x, y, ang, vx, vy, om of one body."""

    def __init__(self, x, y, ang, vx, vy, om):
        self.x, self.y, self.ang, self.vx, self.vy, self.om = x, y, ang, vx, vy, om


class Lander3Oracle:
    def __init__(self, n_envs, seed=0, max_ep_len=1000, velocity_iterations=180, position_iterations=60):
        self.n, self.seed, self.max_ep_len = int(n_envs), int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.vit, self.pit = int(velocity_iterations), int(position_iterations)
        assert self.vit >= 1 and self.pit >= 1
        self.S = np.zeros((NF3, self.n), dtype=F)
        self.env_ids = np.arange(self.n, dtype=np.uint32)
        self.episodes, self.ret_sum, self.len_sum = 0, 0.0, 0
        self.last = None   # what the last step() / _physics() call did, per env (see _physics); the step inside reset() is not recorded
        self.reset()

    # -- RNG: the one-body model's streams (oracle/env_oracle.py: LanderOracle._rng) --------------------------------------
    def _rng(self, step, j):
        ep = self.S[EPI].astype(np.uint32)
        seed_e = np.uint32(self.seed) ^ mix32(ep)
        step = np.asarray(step, dtype=np.uint32) + np.zeros(self.n, np.uint32)
        b = step * np.uint32(16) + np.uint32(j)
        h = mix32(seed_e ^ np.uint32(0x9E3779B9))
        h = mix32(h + self.env_ids * np.uint32(0x85EBCA6B) + np.uint32(0x27D4EB2F))
        h = mix32(h ^ (b * np.uint32(0xC2B2AE35) + np.uint32(0x165667B1)))
        return u01(h)

    def obs(self):
        S = self.S
        o = np.empty((self.n, 8), dtype=F)
        o[:, 0] = (S[PX] - F(10.0)) / F(10.0)
        o[:, 1] = (S[PY] - (HELIPAD_Y + LEG_DOWN)) / F(6.6666665)
        o[:, 2] = S[VX] * F(10.0) / FPS
        o[:, 3] = S[VY] * F(6.6666665) / FPS
        o[:, 4] = S[ANG]
        o[:, 5] = F(20.0) * S[OM] / FPS
        o[:, 6] = S[C1]
        o[:, 7] = S[C2]
        return o

    def _segment(self, px):
        """Terrain segment under world x: (x0, h0, h1 - h0) of chunk idx = clamp(floor(px / 2), 0, 9)."""
        S = self.S
        fi = np.clip(np.floor(px * F(0.5)), F(0.0), F(9.0)).astype(F)
        idx = fi.astype(np.int64)
        cols = np.arange(self.n)
        h0 = S[T0 + idx, cols]
        h1 = S[T0 + idx + 1, cols]
        return (F(2.0) * fi).astype(F), h0, (h1 - h0).astype(F)

    def _ground(self, px):
        x0, h0, dh = self._segment(px)
        t = (px - x0) * F(0.5)
        return (h0 + dh * t).astype(F)

    # -- one physics step for every env; returns (reward, done_env, obs) ----------------------------------------------------
    def _physics(self, act, record=True):
        """RECORDING (no arithmetic statement depends on it): with `record`, self.last becomes a dict of per-env arrays for this step —
        on [8, n] contact mask, seg [8, n] terrain segment under each corner, dh [8, n] that segment's rise, friction_clamp [8, n] the
        tangent clamp cut an increment in some sweep, sweeps [n] position sweeps executed, solved [n], per leg [2, n] motor_hi /
        motor_lo (the motor clamp cut at +0.8 / -0.8 in some sweep) and limit_lo / limit_up (that row left with a positive accumulated
        impulse), main / side the two engine impulses (ix, iy) on the hull with their arms main_r / side_r about its centre of mass
        and m_power / s_power, crash, out (crash or viewport), asleep, and state: a copy of the block as this function leaves it (before
        step()'s episode bookkeeping and reset)."""
        S, n = self.S, self.n
        a0 = np.clip(act[:, 0].astype(F), F(-1.0), F(1.0))
        a1 = np.clip(act[:, 1].astype(F), F(-1.0), F(1.0))
        step = S[PSTEP].astype(np.uint32)
        d0 = (self._rng(step, 0) * F(2.0) - F(1.0)) / SCALE
        d1 = (self._rng(step, 1) * F(2.0) - F(1.0)) / SCALE
        hull = _Body(S[X].copy(), S[Y].copy(), S[ANG].copy(), S[VX].copy(), S[VY].copy(), S[OM].copy())
        legs = [_Body(*(S[L0 + 6 * b + f].copy() for f in (0, 1, 4, 2, 3, 5))) for b in range(2)]
        sn, cs = sincos32(hull.ang)
        tip0, tip1 = sn, cs
        side0, side1 = -tip1, tip0
        # the hull's centre of mass relative to its origin, world frame: R (0, LCY)
        lx = -(sn * LCY)
        ly = cs * LCY
        # main engine: ApplyLinearImpulse at origin + (ox, oy)
        m_power = np.where(a0 > F(0.0), (np.clip(a0, F(0.0), F(1.0)) + F(1.0)) * F(0.5), F(0.0)).astype(F)
        ox = tip0 * (F(0.13333334) + F(2.0) * d0) + side0 * d1
        oy = -tip1 * (F(0.13333334) + F(2.0) * d0) - side1 * d1
        ix = -ox * MAIN_POWER * m_power
        iy = -oy * MAIN_POWER * m_power
        rx = ox - lx
        ry = oy - ly
        rec = {"main": (ix, iy), "main_r": (rx, ry), "m_power": m_power}
        hull.vx = hull.vx + ix * INV_MH
        hull.vy = hull.vy + iy * INV_MH
        hull.om = hull.om + (rx * iy - ry * ix) * INV_IH
        # side engines
        direction = np.where(a1 < F(0.0), F(-1.0), F(1.0)).astype(F)
        s_power = np.where(np.abs(a1) > F(0.5), np.clip(np.abs(a1), F(0.5), F(1.0)), F(0.0)).astype(F)
        arm = F(3.0) * d1 + direction * SIDE_AWAY
        ox = tip0 * d0 + side0 * arm
        oy = -tip1 * d0 - side1 * arm
        ix = -ox * SIDE_POWER * s_power
        iy = -oy * SIDE_POWER * s_power
        rx = (ox - tip0 * F(0.56666666)) - lx
        ry = (oy + tip1 * SIDE_H) - ly
        rec.update(side=(ix, iy), side_r=(rx, ry), s_power=s_power)
        hull.vx = hull.vx + ix * INV_MH
        hull.vy = hull.vy + iy * INV_MH
        hull.om = hull.om + (rx * iy - ry * ix) * INV_IH
        # integrate velocities (gravity)
        hull.vy = hull.vy + GRAV * DT
        for lg in legs:
            lg.vy = lg.vy + GRAV * DT
        # ---- contacts: initialise and warm-start ----
        con = []   # per (leg, corner): dict
        for b in range(2):
            lg = legs[b]
            sb, cb = sincos32(lg.ang)
            for k in range(4):
                cx, cy = F(CORNERS[k][0]) * LEG_HX, F(CORNERS[k][1]) * LEG_HY
                c = {"b": b, "cx": cx, "cy": cy}
                c["rx"] = cb * cx - sb * cy
                c["ry"] = sb * cx + cb * cy
                px = lg.x + c["rx"]
                py = lg.y + c["ry"]
                x0, h0, dh = self._segment(px)
                ln = np.sqrt(dh * dh + F(4.0))
                c["x0"], c["h0"] = x0, h0
                c["seg"], c["dh"], c["fclamp"] = (x0 * F(0.5)).astype(np.int64), dh, np.zeros(n, bool)
                c["nx"] = -dh / ln
                c["ny"] = F(2.0) / ln
                sep = ((px - x0) * c["nx"] + (py - h0) * c["ny"]) - RADIUS
                c["on"] = sep < F(0.0)
                slot = K0 + 2 * (4 * b + k)
                c["an"] = np.where(c["on"], S[slot], F(0.0)).astype(F)
                c["at"] = np.where(c["on"], S[slot + 1], F(0.0)).astype(F)
                tx, ty = c["ny"], -c["nx"]
                rn = c["rx"] * c["ny"] - c["ry"] * c["nx"]
                rt = c["rx"] * ty - c["ry"] * tx
                c["nmass"] = F(1.0) / (INV_ML + INV_IL * (rn * rn))
                c["tmass"] = F(1.0) / (INV_ML + INV_IL * (rt * rt))
                Px = c["an"] * c["nx"] + c["at"] * tx
                Py = c["an"] * c["ny"] + c["at"] * ty
                lg.vx = np.where(c["on"], lg.vx + INV_ML * Px, lg.vx).astype(F)
                lg.vy = np.where(c["on"], lg.vy + INV_ML * Py, lg.vy).astype(F)
                lg.om = np.where(c["on"], lg.om + INV_IL * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
                con.append(c)
        # ---- joints: initialise and warm-start ----
        rAx, rAy = -lx, -ly    # R_hull ((0, 0) - local centre)
        jn = []
        for b in range(2):
            lg = legs[b]
            sb, cb = sincos32(lg.ang)
            ax = SIGN[b] * ANCX
            j = {"b": b, "mhi": np.zeros(n, bool), "mlo": np.zeros(n, bool)}
            j["rBx"] = cb * ax - sb * ANCY
            j["rBy"] = sb * ax + cb * ANCY
            j["k11"] = ((INV_MH + INV_ML) + (rAy * rAy) * INV_IH) + (j["rBy"] * j["rBy"]) * INV_IL
            j["k12"] = (-(rAy * rAx) * INV_IH) - (j["rBy"] * j["rBx"]) * INV_IL
            j["k22"] = ((INV_MH + INV_ML) + (rAx * rAx) * INV_IH) + (j["rBx"] * j["rBx"]) * INV_IL
            det = j["k11"] * j["k22"] - j["k12"] * j["k12"]
            j["idet"] = np.where(det != F(0.0), F(1.0) / np.where(det != F(0.0), det, F(1.0)), det).astype(F)
            j["angle"] = lg.ang - hull.ang
            j["px"], j["py"], j["m"], j["lo"], j["up"] = (S[J0 + 5 * b + f].copy() for f in range(5))
            axial = (j["m"] + j["lo"]) - j["up"]
            hull.vx = hull.vx - INV_MH * j["px"]
            hull.vy = hull.vy - INV_MH * j["py"]
            hull.om = hull.om - INV_IH * ((rAx * j["py"] - rAy * j["px"]) + axial)
            lg.vx = lg.vx + INV_ML * j["px"]
            lg.vy = lg.vy + INV_ML * j["py"]
            lg.om = lg.om + INV_IL * ((j["rBx"] * j["py"] - j["rBy"] * j["px"]) + axial)
            jn.append(j)
        # ---- velocity sweeps: joints, then contacts ----
        for _ in range(self.vit):
            for j in jn:
                lg = legs[j["b"]]
                # motor
                cdot = (lg.om - hull.om) - SIGN[j["b"]] * MOTOR_SPEED
                imp = -AXM * cdot
                old = j["m"]
                j["m"] = _clamp(old + imp, -MAX_MOTOR_IMP, MAX_MOTOR_IMP)
                j["mhi"] |= (old + imp) > MAX_MOTOR_IMP
                j["mlo"] |= (old + imp) < -MAX_MOTOR_IMP
                imp = j["m"] - old
                hull.om = hull.om - INV_IH * imp
                lg.om = lg.om + INV_IL * imp
                # lower limit
                C = j["angle"] - LIM_LO[j["b"]]
                cdot = lg.om - hull.om
                imp = -AXM * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["lo"] + imp, F(0.0))
                imp = new - j["lo"]
                j["lo"] = new
                hull.om = hull.om - INV_IH * imp
                lg.om = lg.om + INV_IL * imp
                # upper limit
                C = LIM_UP[j["b"]] - j["angle"]
                cdot = hull.om - lg.om
                imp = -AXM * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["up"] + imp, F(0.0))
                imp = new - j["up"]
                j["up"] = new
                hull.om = hull.om + INV_IH * imp
                lg.om = lg.om - INV_IL * imp
                # point
                cdx = ((lg.vx - lg.om * j["rBy"]) - hull.vx) + hull.om * rAy
                cdy = ((lg.vy + lg.om * j["rBx"]) - hull.vy) - hull.om * rAx
                bx, by = -cdx, -cdy
                ix = j["idet"] * (j["k22"] * bx - j["k12"] * by)
                iy = j["idet"] * (j["k11"] * by - j["k12"] * bx)
                j["px"] = j["px"] + ix
                j["py"] = j["py"] + iy
                hull.vx = hull.vx - INV_MH * ix
                hull.vy = hull.vy - INV_MH * iy
                hull.om = hull.om - INV_IH * (rAx * iy - rAy * ix)
                lg.vx = lg.vx + INV_ML * ix
                lg.vy = lg.vy + INV_ML * iy
                lg.om = lg.om + INV_IL * (j["rBx"] * iy - j["rBy"] * ix)
            for c in con:
                lg = legs[c["b"]]
                on = c["on"]
                tx, ty = c["ny"], -c["nx"]
                # tangent
                dvx = lg.vx - lg.om * c["ry"]
                dvy = lg.vy + lg.om * c["rx"]
                lam = c["tmass"] * -(dvx * tx + dvy * ty)
                lim = MU * c["an"]
                new = _clamp(c["at"] + lam, -lim, lim)
                c["fclamp"] |= on & (np.abs(c["at"] + lam) > lim)
                lam = new - c["at"]
                c["at"] = np.where(on, new, c["at"]).astype(F)
                Px = lam * tx
                Py = lam * ty
                lg.vx = np.where(on, lg.vx + INV_ML * Px, lg.vx).astype(F)
                lg.vy = np.where(on, lg.vy + INV_ML * Py, lg.vy).astype(F)
                lg.om = np.where(on, lg.om + INV_IL * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
                # normal
                dvx = lg.vx - lg.om * c["ry"]
                dvy = lg.vy + lg.om * c["rx"]
                lam = -c["nmass"] * (dvx * c["nx"] + dvy * c["ny"])
                new = np.maximum(c["an"] + lam, F(0.0))
                lam = new - c["an"]
                c["an"] = np.where(on, new, c["an"]).astype(F)
                Px = lam * c["nx"]
                Py = lam * c["ny"]
                lg.vx = np.where(on, lg.vx + INV_ML * Px, lg.vx).astype(F)
                lg.vy = np.where(on, lg.vy + INV_ML * Py, lg.vy).astype(F)
                lg.om = np.where(on, lg.om + INV_IL * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
        # ---- integrate positions ----
        for bd in [hull] + legs:
            bd.x = bd.x + DT * bd.vx
            bd.y = bd.y + DT * bd.vy
            bd.ang = bd.ang + DT * bd.om
        # ---- position sweeps: contacts, then joints; a solved env leaves the loop (mask) ----
        live = np.ones(n, bool)
        sweeps = np.zeros(n, np.int64)
        for _ in range(self.pit):
            if not live.any():
                break
            sweeps += live
            minsep = np.zeros(n, F)
            for c in con:
                lg = legs[c["b"]]
                on = c["on"] & live
                sb, cb = sincos32(lg.ang)
                rx = cb * c["cx"] - sb * c["cy"]
                ry = sb * c["cx"] + cb * c["cy"]
                px = lg.x + rx
                py = lg.y + ry
                sep = ((px - c["x0"]) * c["nx"] + (py - c["h0"]) * c["ny"]) - RADIUS
                minsep = np.where(on, np.minimum(minsep, sep), minsep).astype(F)
                C = _clamp(BAUM * (sep + SLOP), -MAXLC, F(0.0))
                rn = rx * c["ny"] - ry * c["nx"]
                K = INV_ML + INV_IL * (rn * rn)
                imp = -C / K
                Px = imp * c["nx"]
                Py = imp * c["ny"]
                lg.x = np.where(on, lg.x + INV_ML * Px, lg.x).astype(F)
                lg.y = np.where(on, lg.y + INV_ML * Py, lg.y).astype(F)
                lg.ang = np.where(on, lg.ang + INV_IL * (rx * Py - ry * Px), lg.ang).astype(F)
            jok = np.ones(n, bool)
            for j in jn:
                b = j["b"]
                lg = legs[b]
                angle = lg.ang - hull.ang
                C = np.where(angle <= LIM_LO[b], _clamp((angle - LIM_LO[b]) + ASLOP, -MAXAC, F(0.0)),
                             np.where(angle >= LIM_UP[b], _clamp((angle - LIM_UP[b]) - ASLOP, F(0.0), MAXAC), F(0.0))).astype(F)
                limp = -AXM * C
                hang = hull.ang - INV_IH * limp
                lang = lg.ang + INV_IL * limp
                sa, ca = sincos32(hang)
                sb, cb = sincos32(lang)
                pAx = sa * LCY
                pAy = -(ca * LCY)
                ax = SIGN[b] * ANCX
                pBx = cb * ax - sb * ANCY
                pBy = sb * ax + cb * ANCY
                Cx = ((lg.x + pBx) - hull.x) - pAx
                Cy = ((lg.y + pBy) - hull.y) - pAy
                perr = np.sqrt(Cx * Cx + Cy * Cy)
                k11 = ((INV_MH + INV_ML) + (pAy * pAy) * INV_IH) + (pBy * pBy) * INV_IL
                k12 = (-(pAy * pAx) * INV_IH) - (pBy * pBx) * INV_IL
                k22 = ((INV_MH + INV_ML) + (pAx * pAx) * INV_IH) + (pBx * pBx) * INV_IL
                det = k11 * k22 - k12 * k12
                idet = np.where(det != F(0.0), F(1.0) / np.where(det != F(0.0), det, F(1.0)), det).astype(F)
                ix = -(idet * (k22 * Cx - k12 * Cy))
                iy = -(idet * (k11 * Cy - k12 * Cx))
                hx = hull.x - INV_MH * ix
                hy = hull.y - INV_MH * iy
                hang = hang - INV_IH * (pAx * iy - pAy * ix)
                lgx = lg.x + INV_ML * ix
                lgy = lg.y + INV_ML * iy
                lang = lang + INV_IL * (pBx * iy - pBy * ix)
                hull.x = np.where(live, hx, hull.x).astype(F)
                hull.y = np.where(live, hy, hull.y).astype(F)
                hull.ang = np.where(live, hang, hull.ang).astype(F)
                lg.x = np.where(live, lgx, lg.x).astype(F)
                lg.y = np.where(live, lgy, lg.y).astype(F)
                lg.ang = np.where(live, lang, lg.ang).astype(F)
                jok = jok & (perr <= SLOP) & (np.abs(C) <= ASLOP)
            live = live & ~((minsep >= SLOP3) & jok)
        solved = ~live
        # ---- store the step ----
        S[X], S[Y], S[ANG], S[VX], S[VY], S[OM] = hull.x, hull.y, hull.ang, hull.vx, hull.vy, hull.om
        for b in range(2):
            lg = legs[b]
            for f, v in zip(range(6), (lg.x, lg.y, lg.vx, lg.vy, lg.ang, lg.om)):
                S[L0 + 6 * b + f] = v
            j = jn[b]
            for f, v in zip(range(5), (j["px"], j["py"], j["m"], j["lo"], j["up"])):
                S[J0 + 5 * b + f] = v
        for q, c in enumerate(con):
            S[K0 + 2 * q] = c["an"]
            S[K0 + 2 * q + 1] = c["at"]
        S[C1] = (con[0]["on"] | con[1]["on"] | con[2]["on"] | con[3]["on"]).astype(F)
        S[C2] = (con[4]["on"] | con[5]["on"] | con[6]["on"] | con[7]["on"]).astype(F)
        S[PSTEP] = S[PSTEP] + F(1.0)
        # hull origin at the new pose, crash test on the hull vertices
        sn, cs = sincos32(hull.ang)
        px = hull.x + sn * LCY
        py = hull.y - cs * LCY
        S[PX], S[PY] = px, py
        crash = np.zeros(n, dtype=bool)
        for hx, hy in HULL:
            hx, hy = F(hx), F(hy)
            wx = px + (cs * hx - sn * hy)
            wy = py + (sn * hx + cs * hy)
            crash |= wy < self._ground(wx)
        # rest detection (b2Island::Solve's sleep test)
        slow = np.ones(n, bool)
        for bd in [hull] + legs:
            slow &= ((bd.vx * bd.vx + bd.vy * bd.vy) <= SLEEP_LIN2) & ((bd.om * bd.om) <= SLEEP_ANG2)
        S[SLEEP] = np.where(slow, S[SLEEP] + F(1.0), F(0.0)).astype(F)
        asleep = (S[SLEEP] >= SLEEP_STEPS) & solved
        # observation, shaping, reward (gym lunar_lander.py semantics; as the one-body model)
        o = self.obs()
        shaping = ((F(-100.0) * np.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1])
                    - F(100.0) * np.sqrt(o[:, 2] * o[:, 2] + o[:, 3] * o[:, 3]))
                   - F(100.0) * np.abs(o[:, 4])) + F(10.0) * o[:, 6] + F(10.0) * o[:, 7]
        shaping = shaping.astype(F)
        rew = np.where(S[HASP] > F(0.0), shaping - S[PREV], F(0.0)).astype(F)
        S[PREV], S[HASP] = shaping, F(1.0)
        rew = (rew - m_power * F(0.30)) - s_power * F(0.03)
        out = crash | (np.abs(o[:, 0]) >= F(1.0))
        rew = np.where(out, F(-100.0), np.where(asleep, F(100.0), rew)).astype(F)
        if record:
            rec.update(on=np.stack([c["on"] for c in con]), seg=np.stack([c["seg"] for c in con]), dh=np.stack([c["dh"] for c in con]),
                       friction_clamp=np.stack([c["fclamp"] for c in con]), sweeps=sweeps, solved=solved,
                       motor_hi=np.stack([j["mhi"] for j in jn]), motor_lo=np.stack([j["mlo"] for j in jn]),
                       limit_lo=np.stack([j["lo"] > F(0.0) for j in jn]), limit_up=np.stack([j["up"] > F(0.0) for j in jn]),
                       crash=crash, out=out, asleep=asleep, state=S.copy())
            self.last = rec
        return rew, (out | asleep), o

    # -- env.reset() for masked envs (gym: build terrain, create the bodies, random initial force, one no-op step) -------------
    def reset(self, mask=None):
        S = self.S
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool)
        keep = S.copy()
        hs = [self._rng(RESET_STREAM, j) * F(6.6666665) for j in range(12)]
        for j in range(3, 8):
            hs[j] = np.full(self.n, HELIPAD_Y, F)
        for i in range(11):
            S[T0 + i] = F(0.33) * ((hs[(i - 1) % 12] + hs[i]) + hs[i + 1])
        fx = (self._rng(RESET_STREAM, 12) * F(2.0) - F(1.0)) * F(1000.0)
        fy = (self._rng(RESET_STREAM, 13) * F(2.0) - F(1.0)) * F(1000.0)
        for f in range(NF3):
            if not (T0 <= f < T0 + 11) and f != EPI:
                S[f] = F(0.0)
        S[X], S[Y] = F(10.0), H + LCY
        S[PX], S[PY] = F(10.0), H
        S[VX], S[VY] = (fx * DT) * INV_MH, (fy * DT) * INV_MH
        for b in range(2):
            S[L0 + 6 * b + 0] = F(10.0) - SIGN[b] * LEG_X0
            S[L0 + 6 * b + 1] = H
            S[L0 + 6 * b + 4] = SIGN[b] * LEG_A0
        self._physics(np.zeros((self.n, 2), F), record=False)
        S[:, ~m] = keep[:, ~m]
        return self.obs()

    # -- env.step(a) + the worker's episode bookkeeping (example/dsac.py:102-127), as LanderOracle.step -----------------------
    def step(self, act):
        S = self.S
        rew, done_env, obs2 = self._physics(np.asarray(act, dtype=F).reshape(self.n, 2))
        S[EPLEN] = S[EPLEN] + F(1.0)
        S[EPRET] = S[EPRET] + rew
        limit = S[EPLEN] >= F(self.max_ep_len)
        done_store = np.where(limit, F(0.0), done_env.astype(F)).astype(F)
        ended = done_env | limit
        self.episodes += int(ended.sum())
        self.ret_sum += float(S[EPRET][ended].astype(np.float64).sum())
        self.len_sum += int(S[EPLEN][ended].sum())
        S[EPI] = np.where(ended, S[EPI] + F(1.0), S[EPI]).astype(F)
        next_obs = obs2.copy()
        if ended.any():
            next_obs = self.reset(ended)
        return obs2, rew, done_store, next_obs, ended.astype(np.uint8)

    def stats(self):
        out = (self.episodes, self.ret_sum, self.len_sum)
        self.episodes, self.ret_sum, self.len_sum = 0, 0.0, 0
        return out
