"""ORACLE — TEST INFRASTRUCTURE ONLY.

NumPy (float32, vectorised over envs) specification of the BIPEDAL WALKER behind ddrl_env_create_ex(kind = DDRL_ENV_WALKER):
csrc/walker_device.h mirrors `WalkerOracle._physics` / `_build` statement by statement.

UNPINNED AGAINST GYM: gym and Box2D are absent from this image, so no trajectory of this model is compared with gym's, and every
constant called gym's below is restated from memory of gym ~0.10-0.17 bipedal_walker.py (the standing of SURVEY A7).  The point is the
STRUCTURE and the SOLVER BUDGET of gym's walker (5 bodies, 4 motorised joints, 180 / 60 iterations, 10 lidar rays), not its trajectories.

GYM'S (bipedal_walker.py): FPS 50, SCALE 30, gravity -10, MOTORS_TORQUE 80, SPEED_HIP 4, SPEED_KNEE 6, LIDAR_RANGE 160/30,
INITIAL_RANDOM 5; HULL_POLY [(-30,9),(6,9),(34,1),(34,-8),(-30,-8)]/30 at density 5; LEG_DOWN -8/30, LEG_W 8/30, LEG_H 34/30, upper leg
box (LEG_W/2, LEG_H/2), lower leg box (0.8 LEG_W/2, LEG_H/2), both density 1; legs collide with the ground only; TERRAIN_STEP 14/30,
TERRAIN_LENGTH 200, TERRAIN_HEIGHT 400/30/4, TERRAIN_STARTPAD 20, TERRAIN_GRASS 10, terrain friction 2.5; the grass recurrence
v = 0.8 v + 0.01 sign(TERRAIN_HEIGHT - y), v += U(-1,1)/30 for i > 20, y += v at x = i TERRAIN_STEP; hull at (TERRAIN_STEP 20/2,
TERRAIN_HEIGHT + 2 LEG_H), upper legs at y - LEG_H/2 - LEG_DOWN with angle +-0.05, lower legs at y - 3 LEG_H/2 - LEG_DOWN; hip joint hull
(0, LEG_DOWN) to leg (0, LEG_H/2) with limits [-0.8, 1.1], knee joint leg (0, -LEG_H/2) to lower (0, LEG_H/2) with limits [-1.6, -0.1],
reference angle 0, limit and motor enabled; initial force (U(-5,5), 0) on the hull centre; reset = build + one zero-action step; per
joint motorSpeed = SPEED sign(a), maxMotorTorque = 80 clip(|a|, 0, 1) in the order hip, knee, hip, knee, the action not clipped
otherwise; the 24-float observation [hull angle, 2 w/FPS, 0.3 vx (600/30)/FPS, 0.3 vy (400/30)/FPS, per leg (hip angle, hip speed/4,
knee angle + 1, knee speed/6, lower-leg contact), 10 lidar fractions], ray i from the hull position to (x + sin(1.5 i/10) RANGE,
y - cos(1.5 i/10) RANGE) against the terrain only, 1.0 on a miss; shaping 130 x/30 - 5 |angle|, reward = shaping difference (0 on the
first step) - sum 0.00035 * 80 * clip(|a_j|, 0, 1); hull contact or x < 0: reward -100 and done; x > (200 - 10) TERRAIN_STEP: done.
gym's time limit of 1600 is the caller's max_ep_len.

BOX2D'S STRUCTURE (b2Island::Solve, b2RevoluteJoint, b2ContactSolver, b2PolygonShape::ComputeMass, b2EdgeShape::RayCast; b2Settings.h):
  mass      b2PolygonShape::ComputeMass in float64 (triangle fan about v0: area = sum D/2, centroid = sum area_k (e1 + e2)/3 / area,
            I = density sum D/12 (e1.e1 + e1.e2 + e2.e2) per axis, moved to the centroid by the parallel-axis theorem).  Hull: area
            1.0844444..., mass 5.4222222..., centre (-0.020036429872495, -0.005646630236794), inertia about it 1.9993951741662739.
            Upper leg 8/30 x 34/30: mass 0.3022222..., inertia m (hx^2 + hy^2)/3 = 0.03413991769547325.  Lower leg 6.4/30 x 34/30: mass
            0.2417777..., inertia 0.026796141563786.  X, Y of a body are its CENTRE OF MASS (sweep.c); PX, PY the hull's origin
            (body.position), which the observation's lidar, the shaping and the termination tests read.
  joints    the articulated lander's revolute joint: point constraint as a 2x2 block solve, the two angle limits as one-sided rows,
            a motor row clamped at dt * maxMotorTorque; all four accumulated impulses warm-start the next step.
  contacts  friction sqrt(0.2 * 2.5) (the leg fixture's default 0.2 mixed with the terrain's 2.5), restitution 0, accumulated normal
            and tangent impulses warm-start while the point stays active; tangent before normal.
  step      integrate velocities (gravity); initialise and warm-start contacts 0..7 then joints 0..3; `velocity_iterations` sweeps
            (joints 0..3: motor, lower limit, upper limit, point; then contacts 0..7); integrate positions; up to `position_iterations`
            sweeps (contacts 0..7, then joints 0..3) with the per-env early exit once min separation >= -3 slop, every joint's
            anchors are within the linear slop and every limit's violation — measured before the sweep's correction, as
            b2RevoluteJoint::SolvePositionConstraints reports it — within the angular slop.  Bodies: 0 hull, 1 upper leg 0, 2 lower leg 0, 3 upper leg 1, 4 lower leg 1.  Joints: 0 hip 0 (0 -> 1),
            1 knee 0 (1 -> 2), 2 hip 1 (0 -> 3), 3 knee 1 (3 -> 4).  Contact q = 2 (body - 1) + k.  No sleep exit: gym's walker has none.
  lidar     b2EdgeShape::RayCast per terrain segment (numerator / denominator along the unnormalised segment normal, then the hit's
            parameter along the segment), the smallest fraction over the segments.

OURS: the contact points are the two far-end corners (local y = -LEG_H/2, k = 0: x = -hx, k = 1: x = +hx) of each of the four leg
boxes — feet and knees, 8 points — each against the terrain segment under it with that segment's normal, active while its separation
minus the two polygon radii (0.02) is negative, the corner itself the application point.  The hull keeps a vertex-below-terrain test
that sets game over and gets NO contact response.  No maxTranslation / maxRotation clamps.  The initial force enters the hull's velocity
as (f dt) / m at build time.  A lidar ray's direction is (sin RANGE, -cos RANGE) itself (not p2 - p1), and it is tested against the 13
segments from the one under the hull's origin on (the ray's reach is 11.2 segments); a ray leaving the terrain's last segment misses.
C1 / C2 (observation 8 / 13) are 1 where the lower leg holds an active point this step.

The arithmetic follows oracle/env_oracle.py's rules: float32 only, one rounding per operation (no FMA contraction), sqrt / divide
correctly rounded, `sincos32` for every sine and cosine, the counter hash of noise_oracle for every random number, one stream per
(seed, env id, episode).
"""
import numpy as np

from oracle.env_oracle import RESET_STREAM, sincos32
from oracle.noise_oracle import mix32, u01

F = np.float32
NFW = 286  # DDRL_ENVW_STATE_FIELDS
OBS, ACT = 24, 4
# the one-body model's indices are kept where the field exists there; X..OM is the hull; SLEEP stays 0 (no sleep exit)
(X, Y, VX, VY, ANG, OM, C1, C2, PREV, HASP, EPLEN, EPRET, SLEEP, EPI, PX, PY) = range(16)
PSTEP = 25
L0 = 26          # leg body b = 1..4: L0 + 6 (b - 1) + (x, y, vx, vy, ang, om)
J0 = 50          # joint j: J0 + 5 j + (point impulse x, y, motor, lower limit, upper limit)
K0 = 70          # contact q: K0 + 2 q + (normal impulse, tangent impulse)
T0 = 86          # the 200 terrain heights
NT = 200

FPS, DT, INV_DT, SCALE, GRAV = F(50.0), F(0.02), F(50.0), F(30.0), F(-10.0)
STEP = F(0.46666667)                 # TERRAIN_STEP
STEP2 = F(STEP * STEP)
TH = F(3.3333333)                    # TERRAIN_HEIGHT
RANGE = F(5.3333335)                 # LIDAR_RANGE
NSEG = 13                            # segments a lidar ray is tested against
LCX, LCY = F(-0.02003643), F(-0.00564663)            # hull-local centre of mass
INV_MH, INV_IH = F(0.18442623), F(0.5001513)         # 1 / 5.4222222, 1 / 1.9993952
INV_MU, INV_IU = F(3.3088236), F(29.291225)          # upper leg
INV_ML, INV_IL = F(4.1360292), F(37.318806)          # lower leg
INVM = (INV_MH, INV_MU, INV_ML, INV_MU, INV_ML)
INVI = (INV_IH, INV_IU, INV_IL, INV_IU, INV_IL)
HX = (None, F(0.13333334), F(0.10666667), F(0.13333334), F(0.10666667))   # leg half-widths
HY = F(0.56666666)                   # LEG_H / 2
LEG_DOWN = F(-0.26666668)
X0, Y0 = F(4.6666665), F(5.6)        # hull origin at build
YU, YL = F(5.3), F(4.1666665)        # upper / lower leg centres at build
LEG_A0 = F(0.05)
XEND = F(88.666664)                  # (200 - 10) TERRAIN_STEP
JA = (0, 1, 0, 3)                    # joint j: body A, body B = j + 1
# local anchors relative to the bodies' centres of mass: hip on the hull (0, LEG_DOWN) - (LCX, LCY); knee on the upper leg (0, -HY)
JAX = (F(0.02003643), F(0.0), F(0.02003643), F(0.0))
JAY = (F(-0.26102003), F(-0.56666666), F(-0.26102003), F(-0.56666666))
JBX, JBY = F(0.0), F(0.56666666)
LIM_LO = (F(-0.8), F(-1.6), F(-0.8), F(-1.6))
LIM_UP = (F(1.1), F(-0.1), F(1.1), F(-0.1))
SPEED = (F(4.0), F(6.0), F(4.0), F(6.0))
AXM_HIP = F(F(1.0) / (INV_IH + INV_IU))
AXM_KNEE = F(F(1.0) / (INV_IU + INV_IL))
AXM = (AXM_HIP, AXM_KNEE, AXM_HIP, AXM_KNEE)
MAX_MOTOR_IMP = F(1.6)               # DT * MOTORS_TORQUE
FUEL = F(0.028)                      # 0.00035 * MOTORS_TORQUE
MU = F(0.70710677)                   # sqrt(0.2 * 2.5)
RADIUS = F(0.02)                     # 2 * b2_polygonRadius
SLOP = F(0.005)                      # b2_linearSlop
SLOP3 = F(-0.015)                    # -3 * b2_linearSlop
ASLOP = F(0.034906585)               # b2_angularSlop = 2 deg
MAXLC = F(0.2)                       # b2_maxLinearCorrection
MAXAC = F(0.13962634)                # b2_maxAngularCorrection = 8 deg
BAUM = F(0.2)                        # b2_baumgarte
HULLV = ((F(-1.0), F(0.3)), (F(0.2), F(0.3)), (F(1.1333333), F(0.033333335)), (F(1.1333333), F(-0.26666668)),
         (F(-1.0), F(-0.26666668)))
FORCE_J = 200                        # RNG index of the initial force; 0..199 are the terrain's


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi).astype(F)


def _rot(s, c, ax, ay):
    return (c * ax - s * ay).astype(F), (s * ax + c * ay).astype(F)


class _Body:
    def __init__(self, x, y, ang, vx, vy, om):
        self.x, self.y, self.ang, self.vx, self.vy, self.om = x, y, ang, vx, vy, om


class WalkerOracle:
    def __init__(self, n_envs, seed=0, max_ep_len=1600, velocity_iterations=180, position_iterations=60):
        self.n, self.seed, self.max_ep_len = int(n_envs), int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.vit, self.pit = int(velocity_iterations), int(position_iterations)
        assert self.vit >= 1 and self.pit >= 1
        self.S = np.zeros((NFW, self.n), dtype=F)
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

    def _segment(self, px):
        """Terrain segment under world x: (x0, h0, h1 - h0) of segment idx = clamp(floor(px / STEP), 0, 198)."""
        S = self.S
        fi = np.clip(np.floor(px / STEP), F(0.0), F(NT - 2)).astype(F)
        idx = fi.astype(np.int64)
        cols = np.arange(self.n)
        h0 = S[T0 + idx, cols]
        h1 = S[T0 + idx + 1, cols]
        return (fi * STEP).astype(F), h0, (h1 - h0).astype(F)

    def _ground(self, px):
        x0, h0, dh = self._segment(px)
        t = (px - x0) / STEP
        return (h0 + dh * t).astype(F)

    def _bodies(self):
        S = self.S
        bodies = [_Body(S[X].copy(), S[Y].copy(), S[ANG].copy(), S[VX].copy(), S[VY].copy(), S[OM].copy())]
        for b in range(1, 5):
            bodies.append(_Body(*(S[L0 + 6 * (b - 1) + f].copy() for f in (0, 1, 4, 2, 3, 5))))
        return bodies

    def lidar(self):
        """The 10 ray fractions from the hull's origin: [n, 10]."""
        S, n = self.S, self.n
        px, py = S[PX], S[PY]
        f0 = np.clip(np.floor(px / STEP), F(0.0), F(NT - 2)).astype(F)
        k0 = f0.astype(np.int64)
        cols = np.arange(n)
        hh = [S[T0 + np.minimum(k0 + m, NT - 1), cols] for m in range(NSEG + 1)]
        out = np.empty((n, 10), dtype=F)
        self.last_ray_segment = np.full((n, 10), -1, np.int64)   # RECORDING: the segment (0..12 from the hull's) of each ray's hit, -1: a miss
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for i in range(10):
                s, c = sincos32(np.full(n, (F(1.5) * F(i)) / F(10.0), F))
                dx = s * RANGE
                dy = -(c * RANGE)
                frac = np.ones(n, F)
                for m in range(NSEG):
                    valid = (k0 + m) <= NT - 2
                    xa = (f0 + F(m)) * STEP
                    ha = hh[m]
                    ey = hh[m + 1] - ha
                    num = ey * (xa - px) - STEP * (ha - py)
                    den = ey * dx - STEP * dy
                    t = num / den
                    qx = px + t * dx
                    qy = py + t * dy
                    u = ((qx - xa) * STEP + (qy - ha) * ey) / (STEP2 + ey * ey)
                    hit = valid & (den != F(0.0)) & (t >= F(0.0)) & (t <= F(1.0)) & (u >= F(0.0)) & (u <= F(1.0))
                    self.last_ray_segment[:, i] = np.where(hit & (t < frac), m, self.last_ray_segment[:, i])
                    frac = np.where(hit, np.minimum(frac, t), frac).astype(F)
                out[:, i] = frac
        return out

    def obs(self):
        S = self.S
        bd = self._bodies()
        o = np.empty((self.n, OBS), dtype=F)
        o[:, 0] = S[ANG]
        o[:, 1] = F(2.0) * S[OM] / FPS
        o[:, 2] = ((F(0.3) * S[VX]) * F(20.0)) / FPS
        o[:, 3] = ((F(0.3) * S[VY]) * F(13.333333)) / FPS
        for leg in range(2):
            hip, knee = 2 * leg, 2 * leg + 1
            o[:, 4 + 5 * leg] = bd[hip + 1].ang - bd[JA[hip]].ang
            o[:, 5 + 5 * leg] = (bd[hip + 1].om - bd[JA[hip]].om) / SPEED[hip]
            o[:, 6 + 5 * leg] = (bd[knee + 1].ang - bd[JA[knee]].ang) + F(1.0)
            o[:, 7 + 5 * leg] = (bd[knee + 1].om - bd[JA[knee]].om) / SPEED[knee]
            o[:, 8 + 5 * leg] = S[C1 + leg]
        o[:, 14:] = self.lidar()
        return o

    # -- one physics step for every env; returns (reward, done_env, obs) ----------------------------------------------------
    def _physics(self, act, record=True):
        """RECORDING (no arithmetic statement depends on it): with `record`, self.last becomes a dict of per-env arrays for this step —
        on [8, n] contact mask, seg [8, n] the terrain segment under each point, dh [8, n] its rise, friction_clamp [8, n] the tangent
        clamp cut an increment in some sweep, sweeps [n] position sweeps executed, solved [n], per joint [4, n] motor_hi / motor_lo (the
        motor clamp cut in some sweep), motor [4, n] the accumulated motor impulse, mmax [4, n] its bound, limit_lo / limit_up (that row
        left with a positive accumulated impulse), jangle [4, n] each joint's angle and sep [8, n] each point's separation as its env's last executed position sweep measured it
        (before that sweep's correction; 0 where the point is inactive), game_over, neg_x, finish, and state: a copy of the block as this function leaves it
        (before step()'s episode bookkeeping and reset)."""
        S, n = self.S, self.n
        a = np.asarray(act, dtype=F).reshape(n, ACT)
        mag = [np.clip(np.abs(a[:, j]), F(0.0), F(1.0)).astype(F) for j in range(4)]
        spd = [(SPEED[j] * np.sign(a[:, j])).astype(F) for j in range(4)]
        mmax = [(MAX_MOTOR_IMP * mag[j]).astype(F) for j in range(4)]
        bd = self._bodies()
        # integrate velocities (gravity)
        for b in bd:
            b.vy = b.vy + GRAV * DT
        # ---- contacts: initialise and warm-start ----
        con = []
        for q in range(8):
            b = 1 + q // 2
            lg = bd[b]
            sb, cb = sincos32(lg.ang)
            cx = -HX[b] if q % 2 == 0 else HX[b]
            cy = -HY
            c = {"b": b, "cx": cx, "cy": cy, "fclamp": np.zeros(n, bool)}
            c["rx"], c["ry"] = _rot(sb, cb, cx, cy)
            px = lg.x + c["rx"]
            py = lg.y + c["ry"]
            x0, h0, dh = self._segment(px)
            ln = np.sqrt(dh * dh + STEP2)
            c["x0"], c["h0"], c["dh"] = x0, h0, dh
            c["seg"] = np.clip(np.floor(px / STEP), 0, NT - 2).astype(np.int64)
            c["nx"] = -dh / ln
            c["ny"] = STEP / ln
            sep = ((px - x0) * c["nx"] + (py - h0) * c["ny"]) - RADIUS
            c["on"] = sep < F(0.0)
            slot = K0 + 2 * q
            c["an"] = np.where(c["on"], S[slot], F(0.0)).astype(F)
            c["at"] = np.where(c["on"], S[slot + 1], F(0.0)).astype(F)
            tx, ty = c["ny"], -c["nx"]
            rn = c["rx"] * c["ny"] - c["ry"] * c["nx"]
            rt = c["rx"] * ty - c["ry"] * tx
            c["nmass"] = F(1.0) / (INVM[b] + INVI[b] * (rn * rn))
            c["tmass"] = F(1.0) / (INVM[b] + INVI[b] * (rt * rt))
            Px = c["an"] * c["nx"] + c["at"] * tx
            Py = c["an"] * c["ny"] + c["at"] * ty
            lg.vx = np.where(c["on"], lg.vx + INVM[b] * Px, lg.vx).astype(F)
            lg.vy = np.where(c["on"], lg.vy + INVM[b] * Py, lg.vy).astype(F)
            lg.om = np.where(c["on"], lg.om + INVI[b] * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
            con.append(c)
        # ---- joints: initialise and warm-start ----
        jn = []
        for jj in range(4):
            A, B = bd[JA[jj]], bd[jj + 1]
            mA, iA, mB, iB = INVM[JA[jj]], INVI[JA[jj]], INVM[jj + 1], INVI[jj + 1]
            sa, ca = sincos32(A.ang)
            sb, cb = sincos32(B.ang)
            j = {"mhi": np.zeros(n, bool), "mlo": np.zeros(n, bool)}
            j["rAx"], j["rAy"] = _rot(sa, ca, JAX[jj], JAY[jj])
            j["rBx"], j["rBy"] = _rot(sb, cb, JBX, JBY)
            j["k11"] = ((mA + mB) + (j["rAy"] * j["rAy"]) * iA) + (j["rBy"] * j["rBy"]) * iB
            j["k12"] = (-(j["rAy"] * j["rAx"]) * iA) - (j["rBy"] * j["rBx"]) * iB
            j["k22"] = ((mA + mB) + (j["rAx"] * j["rAx"]) * iA) + (j["rBx"] * j["rBx"]) * iB
            det = j["k11"] * j["k22"] - j["k12"] * j["k12"]
            j["idet"] = np.where(det != F(0.0), F(1.0) / np.where(det != F(0.0), det, F(1.0)), det).astype(F)
            j["angle"] = B.ang - A.ang
            j["px"], j["py"], j["m"], j["lo"], j["up"] = (S[J0 + 5 * jj + f].copy() for f in range(5))
            axial = (j["m"] + j["lo"]) - j["up"]
            A.vx = A.vx - mA * j["px"]
            A.vy = A.vy - mA * j["py"]
            A.om = A.om - iA * ((j["rAx"] * j["py"] - j["rAy"] * j["px"]) + axial)
            B.vx = B.vx + mB * j["px"]
            B.vy = B.vy + mB * j["py"]
            B.om = B.om + iB * ((j["rBx"] * j["py"] - j["rBy"] * j["px"]) + axial)
            jn.append(j)
        # ---- velocity sweeps: joints, then contacts ----
        for _ in range(self.vit):
            for jj, j in enumerate(jn):
                A, B = bd[JA[jj]], bd[jj + 1]
                mA, iA, mB, iB = INVM[JA[jj]], INVI[JA[jj]], INVM[jj + 1], INVI[jj + 1]
                # motor
                cdot = (B.om - A.om) - spd[jj]
                imp = -AXM[jj] * cdot
                old = j["m"]
                j["m"] = _clamp(old + imp, -mmax[jj], mmax[jj])
                j["mhi"] |= (old + imp) > mmax[jj]
                j["mlo"] |= (old + imp) < -mmax[jj]
                imp = j["m"] - old
                A.om = A.om - iA * imp
                B.om = B.om + iB * imp
                # lower limit
                C = j["angle"] - LIM_LO[jj]
                cdot = B.om - A.om
                imp = -AXM[jj] * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["lo"] + imp, F(0.0))
                imp = new - j["lo"]
                j["lo"] = new
                A.om = A.om - iA * imp
                B.om = B.om + iB * imp
                # upper limit
                C = LIM_UP[jj] - j["angle"]
                cdot = A.om - B.om
                imp = -AXM[jj] * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["up"] + imp, F(0.0))
                imp = new - j["up"]
                j["up"] = new
                A.om = A.om + iA * imp
                B.om = B.om - iB * imp
                # point
                cdx = ((B.vx - B.om * j["rBy"]) - A.vx) + A.om * j["rAy"]
                cdy = ((B.vy + B.om * j["rBx"]) - A.vy) - A.om * j["rAx"]
                bx, by = -cdx, -cdy
                ix = j["idet"] * (j["k22"] * bx - j["k12"] * by)
                iy = j["idet"] * (j["k11"] * by - j["k12"] * bx)
                j["px"] = j["px"] + ix
                j["py"] = j["py"] + iy
                A.vx = A.vx - mA * ix
                A.vy = A.vy - mA * iy
                A.om = A.om - iA * (j["rAx"] * iy - j["rAy"] * ix)
                B.vx = B.vx + mB * ix
                B.vy = B.vy + mB * iy
                B.om = B.om + iB * (j["rBx"] * iy - j["rBy"] * ix)
            for c in con:
                b = c["b"]
                lg = bd[b]
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
                lg.vx = np.where(on, lg.vx + INVM[b] * Px, lg.vx).astype(F)
                lg.vy = np.where(on, lg.vy + INVM[b] * Py, lg.vy).astype(F)
                lg.om = np.where(on, lg.om + INVI[b] * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
                # normal
                dvx = lg.vx - lg.om * c["ry"]
                dvy = lg.vy + lg.om * c["rx"]
                lam = -c["nmass"] * (dvx * c["nx"] + dvy * c["ny"])
                new = np.maximum(c["an"] + lam, F(0.0))
                lam = new - c["an"]
                c["an"] = np.where(on, new, c["an"]).astype(F)
                Px = lam * c["nx"]
                Py = lam * c["ny"]
                lg.vx = np.where(on, lg.vx + INVM[b] * Px, lg.vx).astype(F)
                lg.vy = np.where(on, lg.vy + INVM[b] * Py, lg.vy).astype(F)
                lg.om = np.where(on, lg.om + INVI[b] * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
        # ---- integrate positions ----
        for b in bd:
            b.x = b.x + DT * b.vx
            b.y = b.y + DT * b.vy
            b.ang = b.ang + DT * b.om
        # ---- position sweeps: contacts, then joints; a solved env leaves the loop (mask) ----
        live = np.ones(n, bool)
        sweeps = np.zeros(n, np.int64)
        jang = [np.zeros(n, F) for _ in range(4)]
        for _ in range(self.pit):
            if not live.any():
                break
            sweeps += live
            minsep = np.zeros(n, F)
            for c in con:
                b = c["b"]
                lg = bd[b]
                on = c["on"] & live
                sb, cb = sincos32(lg.ang)
                rx, ry = _rot(sb, cb, c["cx"], c["cy"])
                px = lg.x + rx
                py = lg.y + ry
                sep = ((px - c["x0"]) * c["nx"] + (py - c["h0"]) * c["ny"]) - RADIUS
                minsep = np.where(on, np.minimum(minsep, sep), minsep).astype(F)
                c["sep"] = np.where(on, sep, c.get("sep", np.zeros(n, F))).astype(F)   # RECORDING: as the last executed sweep measured it
                C = _clamp(BAUM * (sep + SLOP), -MAXLC, F(0.0))
                rn = rx * c["ny"] - ry * c["nx"]
                K = INVM[b] + INVI[b] * (rn * rn)
                imp = -C / K
                Px = imp * c["nx"]
                Py = imp * c["ny"]
                lg.x = np.where(on, lg.x + INVM[b] * Px, lg.x).astype(F)
                lg.y = np.where(on, lg.y + INVM[b] * Py, lg.y).astype(F)
                lg.ang = np.where(on, lg.ang + INVI[b] * (rx * Py - ry * Px), lg.ang).astype(F)
            jok = np.ones(n, bool)
            for jj in range(4):
                A, B = bd[JA[jj]], bd[jj + 1]
                mA, iA, mB, iB = INVM[JA[jj]], INVI[JA[jj]], INVM[jj + 1], INVI[jj + 1]
                angle = B.ang - A.ang
                C = np.where(angle <= LIM_LO[jj], _clamp((angle - LIM_LO[jj]) + ASLOP, -MAXAC, F(0.0)),
                             np.where(angle >= LIM_UP[jj], _clamp((angle - LIM_UP[jj]) - ASLOP, F(0.0), MAXAC), F(0.0))).astype(F)
                limp = -AXM[jj] * C
                aang = A.ang - iA * limp
                bang = B.ang + iB * limp
                sa, ca = sincos32(aang)
                sb, cb = sincos32(bang)
                pAx, pAy = _rot(sa, ca, JAX[jj], JAY[jj])
                pBx, pBy = _rot(sb, cb, JBX, JBY)
                Cx = ((B.x + pBx) - A.x) - pAx
                Cy = ((B.y + pBy) - A.y) - pAy
                perr = np.sqrt(Cx * Cx + Cy * Cy)
                k11 = ((mA + mB) + (pAy * pAy) * iA) + (pBy * pBy) * iB
                k12 = (-(pAy * pAx) * iA) - (pBy * pBx) * iB
                k22 = ((mA + mB) + (pAx * pAx) * iA) + (pBx * pBx) * iB
                det = k11 * k22 - k12 * k12
                idet = np.where(det != F(0.0), F(1.0) / np.where(det != F(0.0), det, F(1.0)), det).astype(F)
                ix = -(idet * (k22 * Cx - k12 * Cy))
                iy = -(idet * (k11 * Cy - k12 * Cx))
                ax_ = A.x - mA * ix
                ay_ = A.y - mA * iy
                aang = aang - iA * (pAx * iy - pAy * ix)
                bx_ = B.x + mB * ix
                by_ = B.y + mB * iy
                bang = bang + iB * (pBx * iy - pBy * ix)
                A.x = np.where(live, ax_, A.x).astype(F)
                A.y = np.where(live, ay_, A.y).astype(F)
                A.ang = np.where(live, aang, A.ang).astype(F)
                B.x = np.where(live, bx_, B.x).astype(F)
                B.y = np.where(live, by_, B.y).astype(F)
                B.ang = np.where(live, bang, B.ang).astype(F)
                # b2RevoluteJoint::SolvePositionConstraints reports the limit's violation itself, not the slop-shifted correction
                aerr = np.where(angle <= LIM_LO[jj], LIM_LO[jj] - angle, np.where(angle >= LIM_UP[jj], angle - LIM_UP[jj], F(0.0))).astype(F)
                jok = jok & (perr <= SLOP) & (aerr <= ASLOP)
                jang[jj] = np.where(live, angle, jang[jj]).astype(F)   # RECORDING: as the last executed sweep measured it
            live = live & ~((minsep >= SLOP3) & jok)
        solved = ~live
        # ---- store the step ----
        hull = bd[0]
        S[X], S[Y], S[ANG], S[VX], S[VY], S[OM] = hull.x, hull.y, hull.ang, hull.vx, hull.vy, hull.om
        for b in range(1, 5):
            lg = bd[b]
            for f, v in zip(range(6), (lg.x, lg.y, lg.vx, lg.vy, lg.ang, lg.om)):
                S[L0 + 6 * (b - 1) + f] = v
        for jj, j in enumerate(jn):
            for f, v in zip(range(5), (j["px"], j["py"], j["m"], j["lo"], j["up"])):
                S[J0 + 5 * jj + f] = v
        for q, c in enumerate(con):
            S[K0 + 2 * q] = c["an"]
            S[K0 + 2 * q + 1] = c["at"]
        S[C1] = (con[2]["on"] | con[3]["on"]).astype(F)
        S[C2] = (con[6]["on"] | con[7]["on"]).astype(F)
        S[PSTEP] = S[PSTEP] + F(1.0)
        # hull origin at the new pose, game-over test on the hull vertices
        sn, cs = sincos32(hull.ang)
        ox, oy = _rot(sn, cs, LCX, LCY)
        px = hull.x - ox
        py = hull.y - oy
        S[PX], S[PY] = px, py
        game_over = np.zeros(n, dtype=bool)
        for hx, hy in HULLV:
            wx = px + (cs * hx - sn * hy)
            wy = py + (sn * hx + cs * hy)
            game_over |= wy < self._ground(wx)
        # observation, shaping, reward (gym bipedal_walker.py semantics)
        o = self.obs()
        shaping = ((F(130.0) * px) / SCALE - F(5.0) * np.abs(hull.ang)).astype(F)
        rew = np.where(S[HASP] > F(0.0), shaping - S[PREV], F(0.0)).astype(F)
        S[PREV], S[HASP] = shaping, F(1.0)
        for jj in range(4):
            rew = rew - FUEL * mag[jj]
        neg_x = px < F(0.0)
        finish = px > XEND
        rew = np.where(game_over | neg_x, F(-100.0), rew).astype(F)
        if record:
            self.last = dict(
                on=np.stack([c["on"] for c in con]), seg=np.stack([c["seg"] for c in con]), dh=np.stack([c["dh"] for c in con]),
                friction_clamp=np.stack([c["fclamp"] for c in con]), sweeps=sweeps, solved=solved,
                motor_hi=np.stack([j["mhi"] for j in jn]), motor_lo=np.stack([j["mlo"] for j in jn]),
                motor=np.stack([j["m"] for j in jn]), mmax=np.stack(mmax),
                limit_lo=np.stack([j["lo"] > F(0.0) for j in jn]), limit_up=np.stack([j["up"] > F(0.0) for j in jn]),
                jangle=np.stack(jang), sep=np.stack([c.get("sep", np.zeros(n, F)) for c in con]), game_over=game_over, neg_x=neg_x, finish=finish, state=S.copy())
        return rew, (game_over | neg_x | finish), o

    # -- gym's _generate_terrain (grass only) and body construction for every env ------------------------------------------------
    def _build(self):
        S = self.S
        y = np.full(self.n, TH, F)
        v = np.zeros(self.n, F)
        for i in range(NT):
            v = F(0.8) * v + F(0.01) * np.sign(TH - y).astype(F)
            if i > 20:
                v = v + (self._rng(RESET_STREAM, i) * F(2.0) - F(1.0)) / SCALE
            y = (y + v).astype(F)
            S[T0 + i] = y
        fx = (self._rng(RESET_STREAM, FORCE_J) * F(2.0) - F(1.0)) * F(5.0)
        for f in range(NFW):
            if not (T0 <= f < T0 + NT) and f != EPI:
                S[f] = F(0.0)
        S[X], S[Y] = X0 + LCX, Y0 + LCY
        S[PX], S[PY] = X0, Y0
        S[VX] = (fx * DT) * INV_MH
        for b in range(1, 5):
            S[L0 + 6 * (b - 1) + 0] = X0
            S[L0 + 6 * (b - 1) + 1] = YU if b % 2 == 1 else YL
            S[L0 + 6 * (b - 1) + 4] = (-LEG_A0 if b <= 2 else LEG_A0) if b % 2 == 1 else F(0.0)

    # -- env.reset() for masked envs (gym: build terrain, create the bodies, random initial force, one no-op step) -------------
    def reset(self, mask=None):
        S = self.S
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool)
        keep = S.copy()
        self._build()
        self._physics(np.zeros((self.n, ACT), F), record=False)
        S[:, ~m] = keep[:, ~m]
        return self.obs()

    # -- env.step(a) + the worker's episode bookkeeping (example/dsac.py:102-127), as LanderOracle.step -----------------------
    def step(self, act):
        S = self.S
        rew, done_env, obs2 = self._physics(np.asarray(act, dtype=F).reshape(self.n, ACT))
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


class WalkerHeuristic:
    """gym's own walking heuristic (the state machine under `if __name__ == "__main__"` in bipedal_walker.py), restated from memory and
    vectorised over envs; float64 like gym's, the action it returns is float32.  `restart(mask)` puts the masked envs' machines back to
    their initial state (gym's demo runs one episode)."""
    STAY_ON_ONE_LEG, PUT_OTHER_DOWN, PUSH_OFF = 1, 2, 3
    SPEED_, SUPPORT_KNEE_ANGLE = 0.29, 0.1

    def __init__(self, n):
        self.n = n
        self.state = np.full(n, self.STAY_ON_ONE_LEG)
        self.moving = np.zeros(n, np.int64)
        self.ska = np.full(n, self.SUPPORT_KNEE_ANGLE)
        self.a = np.zeros((n, 4))

    def restart(self, mask):
        m = np.asarray(mask).astype(bool)
        self.state[m] = self.STAY_ON_ONE_LEG
        self.moving[m] = 0
        self.ska[m] = self.SUPPORT_KNEE_ANGLE
        self.a[m] = 0.0

    def act(self, obs):
        s = np.asarray(obs, dtype=np.float64)
        out = np.zeros((self.n, 4), dtype=F)
        for e in range(self.n):
            out[e] = self._act1(e, s[e])
        return out

    def _act1(self, e, s):
        moving, supporting = int(self.moving[e]), 1 - int(self.moving[e])
        mb, sb = 4 + 5 * moving, 4 + 5 * supporting
        hip_targ, knee_targ = [None, None], [None, None]
        hip_todo, knee_todo = [0.0, 0.0], [0.0, 0.0]
        if self.state[e] == self.STAY_ON_ONE_LEG:
            hip_targ[moving] = 1.1
            knee_targ[moving] = -0.6
            self.ska[e] += 0.03
            if s[2] > self.SPEED_:
                self.ska[e] += 0.03
            self.ska[e] = min(self.ska[e], self.SUPPORT_KNEE_ANGLE)
            knee_targ[supporting] = self.ska[e]
            if s[sb + 0] < 0.10:
                self.state[e] = self.PUT_OTHER_DOWN
        if self.state[e] == self.PUT_OTHER_DOWN:
            hip_targ[moving] = 0.1
            knee_targ[moving] = self.SUPPORT_KNEE_ANGLE
            knee_targ[supporting] = self.ska[e]
            if s[mb + 4]:
                self.state[e] = self.PUSH_OFF
                self.ska[e] = min(s[mb + 2], self.SUPPORT_KNEE_ANGLE)
        if self.state[e] == self.PUSH_OFF:
            knee_targ[moving] = self.ska[e]
            knee_targ[supporting] = 1.0
            if s[sb + 2] > 0.88 or s[2] > 1.2 * self.SPEED_:
                self.state[e] = self.STAY_ON_ONE_LEG
                self.moving[e] = 1 - moving
        if hip_targ[0]:
            hip_todo[0] = 0.9 * (hip_targ[0] - s[4]) - 0.25 * s[5]
        if hip_targ[1]:
            hip_todo[1] = 0.9 * (hip_targ[1] - s[9]) - 0.25 * s[10]
        if knee_targ[0]:
            knee_todo[0] = 4.0 * (knee_targ[0] - s[6]) - 0.25 * s[7]
        if knee_targ[1]:
            knee_todo[1] = 4.0 * (knee_targ[1] - s[11]) - 0.25 * s[12]
        hip_todo[0] -= 0.9 * (0 - s[0]) - 1.5 * s[1]
        hip_todo[1] -= 0.9 * (0 - s[0]) - 1.5 * s[1]
        knee_todo[0] -= 15.0 * s[3]
        knee_todo[1] -= 15.0 * s[3]
        a = np.array([hip_todo[0], knee_todo[0], hip_todo[1], knee_todo[1]])
        self.a[e] = np.clip(0.5 * a, -1.0, 1.0)
        return self.a[e].astype(F)
