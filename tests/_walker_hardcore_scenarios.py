"""TEST INFRASTRUCTURE: crafted start states for the walker on the HARDCORE terrain (tests/walker_hardcore_oracle.py,
csrc/walker.hip) and the census of the branches this terrain adds.

The walker under any policy reaches its first obstacle late or never inside a test's budget (the first one starts 4.7 m ahead of the
start pose), so every contact branch of the terrain is reached from crafted states: `build()` -> (state block [663, N] float32, actions
[T, N, 4] float32).  The terrains are the generator's own: an oracle of seed SEED is built, and the pose of env e — class
CLASSES[e % len(CLASSES)], interleaved so that every wave holds every class — is translated to an obstacle of the kind the class needs
in env e's terrain (where that terrain lacks the kind, the terrain rows of the next env that has it are copied into env e).  Poses are
built in float64 by tests/_walker_scenarios.py's `pose`; the three TIE classes are then moved by float32 steps until the two separations
of the tie rule are equal to the bit at the corner the oracle computes.

`census_of(ora)` names the branches; `trajectory(vit, pit)` runs the oracle once per iteration pair and is shared by
tests/test_walker_hardcore_cpu.py (every class of the census is reached) and tests/test_gpu_walker_hardcore_scenarios.py (the kernel's
parity on the same trajectory).
"""
import functools

import numpy as np

import _walker_scenarios as G          # pose(), LEG(): the grass walker's pose builder
import walker_hardcore_oracle as H
import walker_oracle as W
from oracle.env_oracle import sincos32

F = np.float32
SEED = 23
FAST, GYM = (8, 3), (180, 60)
N, T = 80, 6                           # a wave and a quarter
MAX_EP_LEN = 1600
LEG = G.LEG
STEPf, Rf, HYf = float(W.STEP), float(W.RADIUS), float(W.HY)
XF = [W.X, W.PX] + [LEG(b, 0) for b in range(1, 5)]
YF = [W.Y, W.PY] + [LEG(b, 1) for b in range(1, 5)]
STAND = (0.05, -0.15, 0.05, -0.15)     # both legs alike: the feet stand side by side
FOLD = (1.1, -1.6, 1.1, -1.6)          # legs folded away in front of the hull
FOOT0_R, FOOT0_L = 3, 2                # corner q of lower leg 0: k = 1 (x = +hx), k = 0 (x = -hx)


def boxes_of(S, e):
    """The obstacles of env e's terrain: list of (kind, first box index, boxes [m, 4] as (x0, x1, y0, y1)); stairs also carry dir."""
    nb = int(S[H.NB, e])
    B = S[H.B0:H.B0 + 4 * nb, e].reshape(nb, 4).astype(np.float64)
    out, b = [], 0
    while b < nb:
        w, h = B[b, 1] - B[b, 0], B[b, 3] - B[b, 2]
        if abs(h - 4 * STEPf) < 1e-3 and abs(w - STEPf) < 1e-3:
            out.append(("pit", b, B[b:b + 2]))
            b += 2
        elif abs(h - STEPf) < 1e-3 and w > 3.5 * STEPf:
            m = b + 1
            while m < nb and abs(B[m, 0] - B[m - 1, 1]) < 1e-3 and abs((B[m, 3] - B[m, 2]) - STEPf) < 1e-3 and B[m, 1] - B[m, 0] > 3.5 * STEPf:
                m += 1
            out.append(("stairs_up" if B[b + 1, 3] > B[b, 3] else "stairs_down", b, B[b:m]))
            b = m
        else:
            out.append(("stump", b, B[b:b + 1]))
            b += 1
    return out


def corner(p, q):
    """World position (float64) of leg corner q of pose p."""
    b, k = 1 + q // 2, q % 2
    a = p[LEG(b, 4)]
    cx, cy = (float(W.HX[b]) if k else -float(W.HX[b])), -HYf
    return p[LEG(b, 0)] + np.cos(a) * cx - np.sin(a) * cy, p[LEG(b, 1)] + np.sin(a) * cx + np.cos(a) * cy


def move(p, dx=0.0, dy=0.0):
    for f in XF:
        p[f] += dx
    for f in YF:
        p[f] += dy
    return p


def place(angles, q, at, vx=0.0, vy=0.0, ang=0.0):
    """A pose with the given joint angles whose leg corner q stands at the world point `at`."""
    p = G.pose(10.0, 6.0, ang, *angles, vx=vx, vy=vy)
    cx, cy = corner(p, q)
    return move(p, at[0] - cx, at[1] - cy)


def place_hull(angles, v, at, ang=0.0, vy=0.0):
    """... whose hull vertex v stands at `at`."""
    p = G.pose(10.0, 6.0, ang, *angles, vy=vy)
    hx, hy = (float(x) for x in W.HULLV[v])
    c, s = np.cos(ang), np.sin(ang)
    return move(p, at[0] - (p[W.PX] + c * hx - s * hy), at[1] - (p[W.PY] + s * hx + c * hy))


def _first(obst, kind, pred=lambda boxes: True):
    for k, b, boxes in obst:
        if k == kind and pred(boxes):
            return boxes
    return None


# class -> (obstacle kind, pose builder from the obstacle's boxes, action, tie code or 0)
def _classes():
    c = {}
    top = lambda bx: bx[3] + 0.01        # noqa: E731   0.01 above a face is inside the contact radius: active at step 0
    c["stump_top"] = ("stump", lambda B: place(STAND, FOOT0_L, (0.5 * (B[0][0] + B[0][1]) - 0.1, top(B[0]))), [0.0, 0.0, 0.0, 0.0], 0)
    # the right foot corner on the ground, 0.01 in front of the stump's left face: floor and wall slot at once, walking into it
    c["stump_left_and_ground"] = ("stump", lambda B: place(STAND, FOOT0_R, (B[0][0] - 0.01, B[0][2] + 0.01), vx=0.6), [0.4, 0.0, 0.4, 0.0], 0)
    c["stump_right_and_ground"] = ("stump", lambda B: place(STAND, FOOT0_L, (B[0][1] + 0.01, B[0][2] + 0.01), vx=-0.6), [-0.4, 0.0, -0.4, 0.0], 0)
    # in the pit: against the first filler's right face (the pit's left wall) and the second filler's left face, feet near the bottom
    c["pit_left_wall"] = ("pit", lambda B: place(STAND, FOOT0_L, (B[0][1] + 0.01, B[0][2] + 0.015), vx=-0.5), [0.0, 0.0, 0.0, 0.0], 0)
    c["pit_right_wall"] = ("pit", lambda B: place(STAND, FOOT0_R, (B[1][0] - 0.01, B[1][2] + 0.015), vx=0.5), [0.0, 0.0, 0.0, 0.0], 0)
    c["stair_up_tread"] = ("stairs_up", lambda B: place(STAND, FOOT0_L, (0.5 * (B[1][0] + B[1][1]), top(B[1]))), [0.2, -0.2, 0.2, -0.2], 0)
    c["stair_down_tread"] = ("stairs_down", lambda B: place(STAND, FOOT0_L, (0.5 * (B[1][0] + B[1][1]), top(B[1]))), [0.2, -0.2, 0.2, -0.2], 0)
    # the tie rule, at a stump's corners and deep inside a wide one (the exact ties are made in float32 by _tie)
    c["tie_top_left"] = ("stump", lambda B: place(STAND, FOOT0_R, (B[0][0] - 0.008, B[0][3] + 0.008)), [0.0, 0.0, 0.0, 0.0], 1)
    c["tie_top_right"] = ("stump", lambda B: place(STAND, FOOT0_L, (B[0][1] + 0.008, B[0][3] + 0.008)), [0.0, 0.0, 0.0, 0.0], 2)
    c["tie_left_right"] = ("stump3", lambda B: place(STAND, FOOT0_L, (0.5 * (B[0][0] + B[0][1]), B[0][3] - 0.9)), [0.0, 0.0, 0.0, 0.0], 3)
    # the hull's nose vertex inside a stump, above the terrain line; legs folded away
    c["hull_in_box"] = ("stump", lambda B: place_hull(FOLD, 2, (B[0][0] + 0.1, 0.5 * (B[0][2] + B[0][3])), vy=-0.5), [0.0, 0.0, 0.0, 0.0], 0)
    # lidar: standing 1.2 before a stump the rays meet its side and its top; high above everything they all miss
    c["lidar_stump"] = ("stump", lambda B: place(STAND, FOOT0_R, (B[0][0] - 1.2, B[0][2] + 0.012)), [0.0, 0.0, 0.0, 0.0], 0)
    c["lidar_stairs"] = ("stairs_up", lambda B: place(STAND, FOOT0_R, (B[0][0] - 0.8, B[0][3] + 0.012)), [0.0, 0.0, 0.0, 0.0], 0)
    c["lidar_all_miss"] = ("stump", lambda B: place(STAND, FOOT0_R, (B[0][0], B[0][3] + 6.0)), [0.5, -0.5, -0.5, 0.5], 0)
    return c


CLASSES = tuple(_classes().keys())


def _corner32(S, e, q):
    """Corner q of env e as WalkerHardcoreOracle._physics computes it at the head of a step (float32)."""
    b = 1 + q // 2
    sb, cb = sincos32(S[LEG(b, 4), e:e + 1])
    cx = -W.HX[b] if q % 2 == 0 else W.HX[b]
    rx, ry = W._rot(sb, cb, cx, -W.HY)
    return F(S[LEG(b, 0), e] + rx[0]), F(S[LEG(b, 1), e] + ry[0])


def _tie(S, e, q, box, code):
    """Move env e's bodies by float32 steps until corner q ties the two separations of `code` (1 top = left, 2 top = right,
    3 left = right) to the bit."""
    x0, x1, y1 = F(box[0]), F(box[1]), F(box[3])

    def shift(fields, d):
        for f in fields:
            S[f, e] = F(S[f, e] + F(d))

    for _ in range(4000):
        wx, wy = _corner32(S, e, q)
        if code == 3:
            lhs, rhs = F(x0 - wx), F(wx - x1)
            if lhs == rhs:
                return True
            d = float(rhs) - float(lhs)
            shift(XF, -0.5 * d if abs(d) > 2e-6 else float(np.spacing(F(wx))) * np.sign(-d))
        else:
            lhs, rhs = F(wy - y1), (F(x0 - wx) if code == 1 else F(wx - x1))
            if lhs == rhs:
                return True
            d = float(rhs) - float(lhs)
            shift(YF, d if abs(d) > 2e-6 else float(np.spacing(F(wy))) * np.sign(d))
    return False


def build():
    cls = _classes()
    ora = H.WalkerHardcoreOracle(N, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=1, position_iterations=1)
    S = ora.S.copy()
    obst = [boxes_of(S, e) for e in range(N)]
    act = np.zeros((T, N, 4), F)
    terrain_rows = np.r_[W.T0:W.T0 + W.NT, H.NB:H.NFWH]
    for e in range(N):
        name = CLASSES[e % len(CLASSES)]
        kind, make, a, tie = cls[name]
        pred = (lambda B: B[0][1] - B[0][0] > 2.5 * STEPf) if kind == "stump3" else (lambda B: True)
        kind = "stump" if kind == "stump3" else kind
        done = False
        for d in range(N):   # env e's own terrain, or the next one that holds the kind (and, for a tie class, admits the exact tie)
            src = (e + d) % N
            boxes = _first(obst[src], kind, pred)
            if boxes is None:
                continue
            S[terrain_rows, e] = ora.S[terrain_rows, src]
            p = make(boxes)
            if tie == 0:
                move(p, dx=0.0007 * (e // len(CLASSES)))   # the copies of a class differ a little
            S[:W.T0, e] = 0.0
            S[H.W0:H.NB, e] = 0.0
            for f, v in p.items():
                S[f, e] = F(v)
            S[W.HASP, e], S[W.EPLEN, e], S[W.PSTEP, e] = 1.0, 3.0, 3.0
            S[W.PREV, e] = F(130.0 * p[W.PX] / 30.0 - 5.0 * abs(p[W.ANG]))
            if tie == 0 or _tie(S, e, {1: FOOT0_R, 2: FOOT0_L, 3: FOOT0_L}[tie], boxes[0], tie):
                done = True
                break
        assert done, name
        act[:, e] = np.asarray(a, F)
    return S, act


BRANCHES = ("floor_on_box_top", "floor_on_terrain_beside_box", "wall_left", "wall_right", "floor_and_wall_at_once", "pit_wall_left",
            "pit_wall_right", "stair_tread_up", "stair_tread_down", "tie_top_left", "tie_top_right", "tie_left_right", "hull_in_box",
            "lidar_box_top", "lidar_box_side", "lidar_all_miss", "wall_friction_clamped", "wall_impulse_positive", "no_box_consulted")


def census_of(ora, counts=None, classes=None):
    """Add the last step's branch classes (env-steps per class) to `counts`.  `classes`: the scenario class of every env, where the
    branch is a statement about the obstacle kind (pit walls, stair treads)."""
    L = ora.last
    c = {} if counts is None else counts
    add = lambda k, m: c.__setitem__(k, c.get(k, 0) + int(np.sum(m)))   # noqa: E731
    on, face, tie = L["on"], L["face"], L["tie"]
    floor, wall = on[0::2], on[1::2]
    add("floor_on_box_top", (floor & (face == H.FACE_TOP)).any(0))
    add("floor_on_terrain_beside_box", (floor & (face >= H.FACE_LEFT)).any(0))
    add("wall_left", (wall & (face == H.FACE_LEFT)).any(0))
    add("wall_right", (wall & (face == H.FACE_RIGHT)).any(0))
    add("floor_and_wall_at_once", (floor & wall).any(0))
    add("tie_top_left", (tie == 1).any(0))
    add("tie_top_right", (tie == 2).any(0))
    add("tie_left_right", (tie == 3).any(0))
    add("hull_in_box", L["box_over"])
    add("lidar_box_top", (L["ray_box"] == H.FACE_TOP).any(1))
    add("lidar_box_side", (L["ray_box"] >= H.FACE_LEFT).any(1))
    add("lidar_all_miss", ((ora.last_ray_segment < 0) & (L["ray_box"] == 0)).all(1))
    add("wall_friction_clamped", L["friction_clamp"][1::2].any(0))
    add("wall_impulse_positive", (L["an"][1::2] > 0).any(0))
    add("no_box_consulted", (face == H.FACE_NONE).all(0))
    if classes is not None:
        cl = np.asarray(classes)
        add("pit_wall_left", (wall & (face == H.FACE_RIGHT)).any(0) & (cl == "pit_left_wall"))
        add("pit_wall_right", (wall & (face == H.FACE_LEFT)).any(0) & (cl == "pit_right_wall"))
        add("stair_tread_up", (floor & (face == H.FACE_TOP)).any(0) & (cl == "stair_up_tread"))
        add("stair_tread_down", (floor & (face == H.FACE_TOP)).any(0) & (cl == "stair_down_tread"))
    return c


ENV_CLASS = np.array([CLASSES[e % len(CLASSES)] for e in range(N)])


@functools.lru_cache(maxsize=None)
def trajectory(vit, pit):
    """-> (start block, actions, per-step outputs of WalkerHardcoreOracle.step, final block, census, per-step records) at (vit, pit)."""
    S, act = build()
    ora = H.WalkerHardcoreOracle(N, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=vit, position_iterations=pit)
    ora.S[:] = S
    outs, census, recs = [], {}, []
    for t in range(T):
        outs.append([np.array(x) for x in ora.step(act[t])])
        census_of(ora, census, ENV_CLASS)
        recs.append(ora.last)
    return S, act, outs, ora.S.copy(), census, recs
