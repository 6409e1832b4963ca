"""ORACLE — TEST INFRASTRUCTURE ONLY.

NumPy (float32, vectorised over envs) specification of the HARDCORE terrain mode of the bipedal walker: the handle of
ddrl_env_create_walker(terrain = DDRL_WALKER_TERRAIN_HARDCORE) (include/ddrl_walker_hardcore.h; kernels csrc/walker.hip over
csrc/walker_device.h's WalkerT<1>).  The arithmetic rules, the constants, the bodies, the joints, the solver's structure, the reward and the
episode bookkeeping are tests/walker_oracle.py's; this file imports its constants and restates `_physics`, `_build` and `lidar` because the
grass oracle's are one function each.  With no box near a corner, a hull vertex or a ray, every statement below reduces to the grass
model's (tests/test_walker_hardcore_cpu.py holds the two together bit for bit with the obstacles switched off).

UNPINNED AGAINST GYM, like every env here: gym and Box2D are absent, no trajectory is compared with gym's, and what is called gym's below
is restated from memory of gym ~0.10-0.17 bipedal_walker.py `_generate_terrain(hardcore=True)`.

GYM'S: the terrain state machine GRASS / STUMP / STAIRS / PIT with `counter` (start pad 20) and `oneshot`; after each run
counter = randint(5, 10); from GRASS one of the three obstacle kinds with equal chance, from an obstacle back to GRASS.
  STUMP   c = randint(1, 3); one box [x, x + c STEP] x [y, y + c STEP]; counter = c; the height line stays at y.
  PIT     c = randint(3, 5); two filler boxes [x, x + STEP] x [y - 4 STEP, y], the second shifted right by c STEP; counter = c + 2;
          original_y = y; the points behind the first are original_y - 4 STEP while counter > 1 and original_y afterwards.
  STAIRS  direction +-1 (u > 0.5: +1), width = randint(4, 5), steps = randint(3, 5); one box per step s, width STEP wide and STEP high,
          its top at y + (s dir) STEP; counter = steps width; behind the first point the height line is gym's ramp
          s' = steps width - counter - dir, y = original_y + ((s' / width) dir) STEP (a float division).
  Grass points keep the grass recurrence and its draws at (RESET_STREAM, i); the initial force keeps (RESET_STREAM, 200).

OURS:
  draws     the obstacle draws of terrain point i are _rng(OBSTACLE_STEP0 + i, j): hash inputs 0x80000000 + 16 i + j, a range no other
            draw of an episode reaches (per-step draws stay below 2^28, the wrapped observation noise inside [0x40000000, 0x50000000),
            the reset streams at 0xFFFFFEF0 / 0xFFFFFF00).  j = 0: the next run's counter; 1: the obstacle kind; 2: the stump's / pit's c
            or the stairs' direction; 3: the stairs' width; 4: their steps.  5..7 are not drawn.
            randint(lo, hi) = lo + min(floor(u (hi - lo + 1)), hi - lo) in float32.
  grass     the recurrence runs at every GRASS point (the grass oracle's terrain has no `oneshot` gap either); an obstacle's oneshot point
            keeps y.  A GRASS run goes on as GRASS (no draw j = 1) when fewer than 5 of the MAXBOX = 40 box slots are free — a guard: the
            worst case by construction is 37 — or when the point behind it is i + 1 > LAST_START = 173: every box then ends at column
            <= 198, inside the terrain's x range, and nothing is clipped.
  boxes     axis-aligned (x0, x1, y0, y1) with x0 = F(i0) STEP, x1 = F(i1) STEP for the columns i0 .. i1 - 1 it covers (column k is
            [k STEP, (k + 1) STEP), the terrain segment k); no two boxes share a column.
  state     [NFWH][n]: rows 0..285 the grass walker's at their indices; W0 = 286 + 2 q + (normal, tangent) the wall slots' accumulated
            impulses; NB = 302 the box count; B0 = 303 + 4 b + (x0, x1, y0, y1); BC0 = 463 + k the box index of column k, -1 for none
            (k < 200; column 199 is never covered).  NFWH = 663 = DDRL_ENVWH_STATE_FIELDS.
  contacts  the eight leg corners, two slots each; slot s = 2 q + w (w = 0 floor, 1 wall).  The corner's column kc is its terrain
            segment's index.  The box consulted is the first in the column order kc, kc - 1, kc + 1 (columns inside 0..199) whose
            separations top = (wy - y1) - R, left = (x0 - wx) - R, right = (wx - x1) - R are all negative and whose bottom y0 < wy.
            The face is the largest separation, ties to top, then left, then right.
            floor slot: today's contact against the terrain segment under the corner — unless a box is consulted and its face is the
            top: then the anchor is (x0, y1) and the normal (0, 1).  Active while its separation is negative.
            wall slot: a consulted box's side face: left: anchor (x0, y1), normal (-1, 0); right: anchor (x1, y1), normal (1, 0); active
            while a side face is chosen (its separation is negative then).  Otherwise inactive with a zeroed accumulated impulse.
            Both slots warm-start, take friction MU and restitution 0 and enter the position solve as the grass point does.
  order     warm start: slots 0..15, then joints 0..3.  Velocity sweep: joints 0..3, then slots 0..15 (tangent before normal).
            Position sweep: slots 0..15, then joints 0..3.  So a corner's floor slot comes before its wall slot everywhere.
  C1 / C2   1 where the lower leg holds an active point in either slot.
  hull      game over when a hull vertex is below the terrain line, or strictly inside the box of its column
            (x0 < wx < x1 and y0 < wy < y1).  No contact response.
  lidar     the 13 segments as before; behind segment m, when its column's box differs from the previous column's (none before m = 0):
            that box's top edge (x0, y1) -> (x1, y1), left edge (x0, y0) -> (x0, y1) and right edge (x1, y0) -> (x1, y1), each by the same
            b2EdgeShape::RayCast statements with the edge vector (ex, ey) in the place of (STEP, ey).
  unchanged reward, shaping, x < 0, the finish line, reset = build + one zero-action step, the episode bookkeeping, the wrapped step
            (WalkerHardcoreWrappedOracle reuses WalkerWrappedOracle.step_wrapped as it is).
"""
import numpy as np

import walker_oracle as wo
from oracle.env_oracle import RESET_STREAM, sincos32
from walker_oracle import (ACT, ANG, ASLOP, AXM, BAUM, C1, C2, DT, EPI, F, FORCE_J, FUEL, GRAV, HASP, HULLV, HX, HY, INV_DT, INV_MH, INVI,
                           INVM, J0, JA, JAX, JAY, JBX, JBY, K0, L0, LCX, LCY, LEG_A0, LIM_LO, LIM_UP, MAX_MOTOR_IMP, MAXAC, MAXLC, MU, NSEG,
                           NT, OBS, OM, PREV, PSTEP, PX, PY, RADIUS, RANGE, SCALE, SLOP, SLOP3, SPEED, STEP, STEP2, T0, TH, VX, VY, X, X0,
                           XEND, Y, Y0, YL, YU, WalkerOracle, _Body, _clamp, _rot)
from walker_wrapped_oracle import WalkerWrappedOracle

TERRAIN_GRASS, TERRAIN_HARDCORE = 0, 1      # DDRL_WALKER_TERRAIN_*
NFW = wo.NFW
W0 = NFW                # wall slot q: W0 + 2 q + (normal impulse, tangent impulse)
NB = W0 + 16            # the box count
B0 = NB + 1             # box b: B0 + 4 b + (x0, x1, y0, y1)
MAXBOX = 40
BC0 = B0 + 4 * MAXBOX   # column k: the index of the box that covers it, -1: none
NFWH = BC0 + NT         # DDRL_ENVWH_STATE_FIELDS
OBSTACLE_STEP0 = 0x08000000
LAST_START = 173        # the last terrain point at which an obstacle may start (5 steps of width 5 end at column 198)
GRASS, STUMP, STAIRS, PIT = range(4)
STARTPAD = 20
FACE_NONE, FACE_TOP, FACE_LEFT, FACE_RIGHT = range(4)
STEP4 = F(F(4.0) * STEP)


def _randint(u, lo, hi):
    return int(lo) + int(min(np.floor(F(u) * F(hi - lo + 1)), F(hi - lo)))


class WalkerHardcoreOracle(WalkerOracle):
    def __init__(self, n_envs, seed=0, max_ep_len=1600, velocity_iterations=180, position_iterations=60, obstacles=True):
        self.obstacles = bool(obstacles)   # False (tests only): the generator never leaves GRASS
        self.n, self.seed, self.max_ep_len = int(n_envs), int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.vit, self.pit = int(velocity_iterations), int(position_iterations)
        assert self.vit >= 1 and self.pit >= 1
        self.S = np.zeros((NFWH, self.n), dtype=F)
        self.env_ids = np.arange(self.n, dtype=np.uint32)
        self.episodes, self.ret_sum, self.len_sum = 0, 0.0, 0
        self.last = None
        self.draw_log = None   # RECORDING: a list that _rng appends (step, j) to, where a test sets one
        self.reset()

    def _rng(self, step, j):
        if self.draw_log is not None:
            self.draw_log.append((np.asarray(step, dtype=np.uint32) + np.zeros(self.n, np.uint32), int(j)))
        return super()._rng(step, j)

    # -- boxes ---------------------------------------------------------------------------------------------------------------------
    def _box_of_column(self, k):
        """(found, x0, x1, y0, y1) of the box that covers column k [n] (int64; a column outside 0..199 holds none)."""
        S, cols = self.S, np.arange(self.n)
        inside = (k >= 0) & (k <= NT - 1)
        kk = np.clip(k, 0, NT - 1)
        bi = np.where(inside, S[BC0 + kk, cols], F(-1.0))
        found = bi >= F(0.0)
        b = np.where(found, bi, F(0.0)).astype(np.int64)
        return found, S[B0 + 4 * b, cols], S[B0 + 4 * b + 1, cols], S[B0 + 4 * b + 2, cols], S[B0 + 4 * b + 3, cols]

    def _consult(self, kc, wx, wy):
        """The box consulted for a corner at (wx, wy) in column kc: (face [n] int, x0, x1, y1, tie); FACE_NONE where no box is.
        tie (RECORDING): 1 top = left, 2 top = right, 3 left = right, where the two are the largest separations; else 0."""
        n = self.n
        face = np.full(n, FACE_NONE, np.int64)
        tie = np.zeros(n, np.int64)
        bx0, bx1, by1 = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        taken = np.zeros(n, bool)
        for dk in (0, -1, 1):
            found, x0, x1, y0, y1 = self._box_of_column(kc + dk)
            top = (wy - y1) - RADIUS
            left = (x0 - wx) - RADIUS
            right = (wx - x1) - RADIUS
            ok = found & (top < F(0.0)) & (left < F(0.0)) & (right < F(0.0)) & (y0 < wy) & ~taken
            fc = np.where((top >= left) & (top >= right), FACE_TOP, np.where(left >= right, FACE_LEFT, FACE_RIGHT))
            face = np.where(ok, fc, face)
            tie = np.where(ok & (top == left) & (top >= right), 1, np.where(ok & (top == right) & (top >= left), 2,
                           np.where(ok & (left == right) & (left > top), 3, tie)))
            bx0 = np.where(ok, x0, bx0).astype(F)
            bx1 = np.where(ok, x1, bx1).astype(F)
            by1 = np.where(ok, y1, by1).astype(F)
            taken |= ok
        return face, bx0, bx1, by1, tie

    # -- one b2EdgeShape::RayCast of ray (px, py) + t (dx, dy) against the edge v1 + u (ex, ey), ee = ex ex + ey ey ---------------------
    @staticmethod
    def _ray_edge(px, py, dx, dy, v1x, v1y, ex, ey, ee, valid):
        num = ey * (v1x - px) - ex * (v1y - py)
        den = ey * dx - ex * dy
        t = num / den
        qx = px + t * dx
        qy = py + t * dy
        u = ((qx - v1x) * ex + (qy - v1y) * ey) / ee
        hit = valid & (den != F(0.0)) & (t >= F(0.0)) & (t <= F(1.0)) & (u >= F(0.0)) & (u <= F(1.0))
        return hit, t

    def lidar(self):
        S, n = self.S, self.n
        px, py = S[PX], S[PY]
        f0 = np.clip(np.floor(px / STEP), F(0.0), F(NT - 2)).astype(F)
        k0 = f0.astype(np.int64)
        cols = np.arange(n)
        hh = [S[T0 + np.minimum(k0 + m, NT - 1), cols] for m in range(NSEG + 1)]
        out = np.empty((n, 10), dtype=F)
        self.last_ray_segment = np.full((n, 10), -1, np.int64)
        self.last_ray_box = np.zeros((n, 10), np.int64)   # RECORDING: FACE_* of the box edge that holds the ray's smallest fraction, 0: none
        fr = [np.ones(n, F) for _ in range(10)]
        dxs, dys = [], []
        for i in range(10):
            s, c = sincos32(np.full(n, (F(1.5) * F(i)) / F(10.0), F))
            dxs.append(s * RANGE)
            dys.append(-(c * RANGE))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            prev = np.full(n, F(-1.0), F)
            for m in range(NSEG):
                valid = (k0 + m) <= NT - 2
                xa = (f0 + F(m)) * STEP
                ha = hh[m]
                ey = hh[m + 1] - ha
                ee = STEP2 + ey * ey
                bi = S[BC0 + np.minimum(k0 + m, NT - 1), cols]
                newbox = valid & (bi >= F(0.0)) & (bi != prev)
                prev = bi
                b = np.where(bi >= F(0.0), bi, F(0.0)).astype(np.int64)
                x0, x1, y0, y1 = (S[B0 + 4 * b + f, cols] for f in range(4))
                w = x1 - x0
                h = y1 - y0
                for i in range(10):
                    hit, t = self._ray_edge(px, py, dxs[i], dys[i], xa, ha, STEP, ey, ee, valid)
                    self.last_ray_segment[:, i] = np.where(hit & (t < fr[i]), m, self.last_ray_segment[:, i])
                    self.last_ray_box[:, i] = np.where(hit & (t < fr[i]), 0, self.last_ray_box[:, i])
                    fr[i] = np.where(hit, np.minimum(fr[i], t), fr[i]).astype(F)
                    for fc, (v1x, v1y, ex, ey2, e2) in ((FACE_TOP, (x0, y1, w, F(0.0), w * w)), (FACE_LEFT, (x0, y0, F(0.0), h, h * h)),
                                                       (FACE_RIGHT, (x1, y0, F(0.0), h, h * h))):
                        hit, t = self._ray_edge(px, py, dxs[i], dys[i], v1x, v1y, ex, ey2, e2, newbox)
                        self.last_ray_box[:, i] = np.where(hit & (t < fr[i]), fc, self.last_ray_box[:, i])
                        fr[i] = np.where(hit, np.minimum(fr[i], t), fr[i]).astype(F)
        for i in range(10):
            out[:, i] = fr[i]
        return out

    # -- one physics step for every env; returns (reward, done_env, obs) ----------------------------------------------------------------
    def _physics(self, act, record=True):
        """As WalkerOracle._physics, over 16 contact slots.  RECORDING (no arithmetic statement depends on it): self.last as the grass
        oracle's with [16, n] where it has [8, n] (slot s = 2 q + w), plus face [8, n] the FACE_* each corner's consulted box gave (0: no
        box), tie [8, n] (see _consult), an / at / nx / ny [16, n] the slots' accumulated impulses and normals, friction_limit [16, n] the
        bound the last velocity sweep clamped each tangent impulse to, minsep [n] the last executed position sweep's, ray_box [n, 10] (lidar), box_over [n] (a hull vertex strictly inside a box)."""
        S, n = self.S, self.n
        a = np.asarray(act, dtype=F).reshape(n, ACT)
        mag = [np.clip(np.abs(a[:, j]), F(0.0), F(1.0)).astype(F) for j in range(4)]
        spd = [(SPEED[j] * np.sign(a[:, j])).astype(F) for j in range(4)]
        mmax = [(MAX_MOTOR_IMP * mag[j]).astype(F) for j in range(4)]
        bd = self._bodies()
        for b in bd:
            b.vy = b.vy + GRAV * DT
        # ---- contacts: initialise and warm-start, per corner the floor slot and then the wall slot ----
        con, faces, ties = [], [], []
        zero, one = np.zeros(n, F), np.ones(n, F)
        for q in range(8):
            b = 1 + q // 2
            lg = bd[b]
            sb, cb = sincos32(lg.ang)
            cx = -HX[b] if q % 2 == 0 else HX[b]
            cy = -HY
            rx, ry = _rot(sb, cb, cx, cy)
            px = lg.x + rx
            py = lg.y + ry
            x0, h0, dh = self._segment(px)
            ln = np.sqrt(dh * dh + STEP2)
            seg = np.clip(np.floor(px / STEP), 0, NT - 2).astype(np.int64)
            face, bx0, bx1, by1, tie = self._consult(seg, px, py)
            faces.append(face)
            ties.append(tie)
            top, left, side = face == FACE_TOP, face == FACE_LEFT, (face == FACE_LEFT) | (face == FACE_RIGHT)
            geo = (
                # floor: the terrain segment, or the consulted box's top
                (np.where(top, bx0, x0).astype(F), np.where(top, by1, h0).astype(F), np.where(top, zero, -dh / ln).astype(F),
                 np.where(top, one, STEP / ln).astype(F), None, K0 + 2 * q),
                # wall: the consulted box's side face
                (np.where(left, bx0, bx1).astype(F), by1, np.where(left, -one, one).astype(F), zero, side, W0 + 2 * q),
            )
            for ax0, ah0, nx, ny, gate, slot in geo:
                c = {"b": b, "cx": cx, "cy": cy, "fclamp": np.zeros(n, bool), "rx": rx, "ry": ry, "x0": ax0, "h0": ah0, "dh": dh, "seg": seg,
                     "nx": nx, "ny": ny}
                sep = ((px - ax0) * nx + (py - ah0) * ny) - RADIUS
                c["on"] = (sep < F(0.0)) if gate is None else (gate & (sep < F(0.0)))
                c["an"] = np.where(c["on"], S[slot], F(0.0)).astype(F)
                c["at"] = np.where(c["on"], S[slot + 1], F(0.0)).astype(F)
                tx, ty = ny, -nx
                rn = rx * ny - ry * nx
                rt = rx * ty - ry * tx
                c["nmass"] = F(1.0) / (INVM[b] + INVI[b] * (rn * rn))
                c["tmass"] = F(1.0) / (INVM[b] + INVI[b] * (rt * rt))
                Px = c["an"] * nx + c["at"] * tx
                Py = c["an"] * ny + c["at"] * ty
                lg.vx = np.where(c["on"], lg.vx + INVM[b] * Px, lg.vx).astype(F)
                lg.vy = np.where(c["on"], lg.vy + INVM[b] * Py, lg.vy).astype(F)
                lg.om = np.where(c["on"], lg.om + INVI[b] * (rx * Py - ry * Px), lg.om).astype(F)
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
        # ---- velocity sweeps: joints, then contact slots ----
        for _ in range(self.vit):
            for jj, j in enumerate(jn):
                A, B = bd[JA[jj]], bd[jj + 1]
                mA, iA, mB, iB = INVM[JA[jj]], INVI[JA[jj]], INVM[jj + 1], INVI[jj + 1]
                cdot = (B.om - A.om) - spd[jj]
                imp = -AXM[jj] * cdot
                old = j["m"]
                j["m"] = _clamp(old + imp, -mmax[jj], mmax[jj])
                j["mhi"] |= (old + imp) > mmax[jj]
                j["mlo"] |= (old + imp) < -mmax[jj]
                imp = j["m"] - old
                A.om = A.om - iA * imp
                B.om = B.om + iB * imp
                C = j["angle"] - LIM_LO[jj]
                cdot = B.om - A.om
                imp = -AXM[jj] * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["lo"] + imp, F(0.0))
                imp = new - j["lo"]
                j["lo"] = new
                A.om = A.om - iA * imp
                B.om = B.om + iB * imp
                C = LIM_UP[jj] - j["angle"]
                cdot = A.om - B.om
                imp = -AXM[jj] * (cdot + np.maximum(C, F(0.0)) * INV_DT)
                new = np.maximum(j["up"] + imp, F(0.0))
                imp = new - j["up"]
                j["up"] = new
                A.om = A.om + iA * imp
                B.om = B.om - iB * imp
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
                dvx = lg.vx - lg.om * c["ry"]
                dvy = lg.vy + lg.om * c["rx"]
                lam = c["tmass"] * -(dvx * tx + dvy * ty)
                lim = MU * c["an"]
                new = _clamp(c["at"] + lam, -lim, lim)
                c["fclamp"] |= on & (np.abs(c["at"] + lam) > lim)
                c["lim"] = lim   # RECORDING: the friction bound the last sweep clamped the tangent impulse to (MU x the normal impulse then)
                lam = new - c["at"]
                c["at"] = np.where(on, new, c["at"]).astype(F)
                Px = lam * tx
                Py = lam * ty
                lg.vx = np.where(on, lg.vx + INVM[b] * Px, lg.vx).astype(F)
                lg.vy = np.where(on, lg.vy + INVM[b] * Py, lg.vy).astype(F)
                lg.om = np.where(on, lg.om + INVI[b] * (c["rx"] * Py - c["ry"] * Px), lg.om).astype(F)
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
        # ---- position sweeps: contact slots, then joints; a solved env leaves the loop (mask) ----
        live = np.ones(n, bool)
        sweeps = np.zeros(n, np.int64)
        jang = [np.zeros(n, F) for _ in range(4)]
        self.last_minsep = np.zeros(n, F)   # RECORDING: the min separation (wall slots included) the env's last executed sweep measured
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
                c["sep"] = np.where(on, sep, c.get("sep", np.zeros(n, F))).astype(F)
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
                aerr = np.where(angle <= LIM_LO[jj], LIM_LO[jj] - angle, np.where(angle >= LIM_UP[jj], angle - LIM_UP[jj], F(0.0))).astype(F)
                jok = jok & (perr <= SLOP) & (aerr <= ASLOP)
                jang[jj] = np.where(live, angle, jang[jj]).astype(F)
            self.last_minsep = np.where(live, minsep, self.last_minsep).astype(F)
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
        for s, c in enumerate(con):
            slot = (K0 if s % 2 == 0 else W0) + 2 * (s // 2)
            S[slot] = c["an"]
            S[slot + 1] = c["at"]
        S[C1] = (con[4]["on"] | con[5]["on"] | con[6]["on"] | con[7]["on"]).astype(F)
        S[C2] = (con[12]["on"] | con[13]["on"] | con[14]["on"] | con[15]["on"]).astype(F)
        S[PSTEP] = S[PSTEP] + F(1.0)
        sn, cs = sincos32(hull.ang)
        ox, oy = _rot(sn, cs, LCX, LCY)
        px = hull.x - ox
        py = hull.y - oy
        S[PX], S[PY] = px, py
        game_over = np.zeros(n, dtype=bool)
        box_over = np.zeros(n, dtype=bool)
        for hx, hy in HULLV:
            wx = px + (cs * hx - sn * hy)
            wy = py + (sn * hx + cs * hy)
            game_over |= wy < self._ground(wx)
            kc = np.clip(np.floor(wx / STEP), 0, NT - 2).astype(np.int64)
            found, x0, x1, y0, y1 = self._box_of_column(kc)
            box_over |= found & (wx > x0) & (wx < x1) & (wy > y0) & (wy < y1)
        game_over = game_over | box_over
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
                jangle=np.stack(jang), sep=np.stack([c.get("sep", np.zeros(n, F)) for c in con]), game_over=game_over, neg_x=neg_x,
                finish=finish, state=S.copy(), face=np.stack(faces), tie=np.stack(ties), ray_box=self.last_ray_box.copy(), box_over=box_over,
                an=np.stack([c["an"] for c in con]), at=np.stack([c["at"] for c in con]), minsep=self.last_minsep.copy(),
                nx=np.stack([c["nx"] for c in con]), ny=np.stack([c["ny"] for c in con]), friction_limit=np.stack([c["lim"] for c in con]))
        return rew, (game_over | neg_x | finish), o

    # -- gym's _generate_terrain(hardcore=True) and the body construction ------------------------------------------------------------------
    def _build(self, mask=None):
        S, n = self.S, self.n
        m = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
        ug = [self._rng(RESET_STREAM, i) if i > 20 else None for i in range(NT)]
        uo = [[self._rng(OBSTACLE_STEP0 + i, j) for j in range(5)] for i in range(NT)] if self.obstacles else None
        self.last_kinds = [[] for _ in range(n)]   # RECORDING: the obstacle kinds of each env's terrain, in order
        for e in np.nonzero(m)[0]:
            self._terrain1(int(e), ug, uo)
        fx = (self._rng(RESET_STREAM, FORCE_J) * F(2.0) - F(1.0)) * F(5.0)
        for f in range(NFWH):
            if not (T0 <= f < T0 + NT) and f != EPI and f < NB:
                S[f] = F(0.0)
        S[X], S[Y] = X0 + LCX, Y0 + LCY
        S[PX], S[PY] = X0, Y0
        S[VX] = (fx * DT) * INV_MH
        for b in range(1, 5):
            S[L0 + 6 * (b - 1) + 0] = X0
            S[L0 + 6 * (b - 1) + 1] = YU if b % 2 == 1 else YL
            S[L0 + 6 * (b - 1) + 4] = (-LEG_A0 if b <= 2 else LEG_A0) if b % 2 == 1 else F(0.0)

    def _terrain1(self, e, ug, uo):
        """The terrain of env e: heights, box table, column index (the state machine is serial per env)."""
        S = self.S
        S[NB:NFWH, e] = F(0.0)
        S[BC0:BC0 + NT, e] = F(-1.0)
        nb = 0

        def box(i0, i1, y0, y1):
            nonlocal nb
            S[B0 + 4 * nb:B0 + 4 * nb + 4, e] = (F(i0) * STEP, F(i1) * STEP, y0, y1)
            S[BC0 + i0:BC0 + i1, e] = F(nb)
            nb += 1

        state, oneshot, counter = GRASS, False, STARTPAD
        y, v, oy = TH, F(0.0), F(0.0)
        sdir = swidth = ssteps = 0
        for i in range(NT):
            if state == GRASS:
                v = F(F(0.8) * v) + F(F(0.01) * np.sign(F(TH - y)).astype(F))
                if i > 20:
                    v = F(v + F(F(F(ug[i][e] * F(2.0)) - F(1.0)) / SCALE))
                y = F(y + v)
            elif state == PIT and oneshot:
                c = _randint(uo[i][2][e], 3, 5)
                box(i, i + 1, F(y - STEP4), y)
                box(i + c, i + c + 1, F(y - STEP4), y)
                counter = c + 2
                oy = y
            elif state == PIT:
                y = oy
                if counter > 1:
                    y = F(y - STEP4)
            elif state == STUMP and oneshot:
                c = _randint(uo[i][2][e], 1, 3)
                box(i, i + c, y, F(y + F(F(c) * STEP)))
                counter = c
            elif state == STAIRS and oneshot:
                sdir = 1 if uo[i][2][e] > F(0.5) else -1
                swidth = _randint(uo[i][3][e], 4, 5)
                ssteps = _randint(uo[i][4][e], 3, 5)
                oy = y
                for s in range(ssteps):
                    top = F(y + F(F(s * sdir) * STEP))
                    box(i + s * swidth, i + (s + 1) * swidth, F(top - STEP), top)
                counter = ssteps * swidth
            elif state == STAIRS:
                s = ssteps * swidth - counter - sdir
                nn = F(F(s) / F(swidth))
                y = F(oy + F(F(nn * F(sdir)) * STEP))
            oneshot = False
            S[T0 + i, e] = y
            counter -= 1
            if counter == 0:
                counter = _randint(uo[i][0][e], 5, 10) if uo is not None else 10
                if state == GRASS and uo is not None and MAXBOX - nb >= 5 and i + 1 <= LAST_START:
                    state = 1 + _randint(uo[i][1][e], 0, 2)
                    self.last_kinds[e].append(state)
                    oneshot = True
                else:
                    state = GRASS
        S[NB, e] = F(nb)

    def reset(self, mask=None):
        S = self.S
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool)
        keep = S.copy()
        self._build(m)
        self._physics(np.zeros((self.n, ACT), F), record=False)
        S[:, ~m] = keep[:, ~m]
        return self.obs()


class WalkerHardcoreWrappedOracle(WalkerHardcoreOracle):
    """The wrapped step on the Hardcore class: WalkerWrappedOracle.step_wrapped itself (it only calls _physics / reset / _rng)."""
    step_wrapped = WalkerWrappedOracle.step_wrapped
