"""Generate tests/golden/lander3_heuristic.npz: the articulated lander's oracle (tests/lander3_oracle.py) at gym's 180 velocity /
60 position iterations under gym's heuristic controller, 8 envs with consecutive env ids from one recorded seed, run until every
env has finished at least one episode (plus a short tail).  Data only: the seed and iteration counts, per step the actions, obs2,
rew, done and ended, the final state block, and per finished episode its env, return and length.

    python tools/gen_lander3_golden.py [--out tests/golden/lander3_heuristic.npz] [--report profiles/lander3_heuristic.txt]

CPU only (NumPy); about a minute.  tests/test_lander3_cpu.py regenerates the first steps and compares bit for bit, and reads the
landing statistics from the file; tests/test_gpu_lander3.py replays the recorded actions through the HIP kernel.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, N_ENVS, MAX_EP_LEN, VIT, PIT = 1, 8, 1000, 180, 60
TAIL, MAX_STEPS = 12, 1200


def heuristic(s):
    """gym's lunar_lander heuristic controller."""
    angle_targ = np.clip(s[:, 0] * 0.5 + s[:, 2] * 1.0, -0.4, 0.4)
    hover_targ = 0.55 * np.abs(s[:, 0])
    angle_todo = (angle_targ - s[:, 4]) * 0.5 - s[:, 5] * 1.0
    hover_todo = (hover_targ - s[:, 1]) * 0.5 - s[:, 3] * 0.5
    legs = (s[:, 6] > 0) | (s[:, 7] > 0)
    angle_todo = np.where(legs, 0, angle_todo)
    hover_todo = np.where(legs, -s[:, 3] * 0.5, hover_todo)
    return np.clip(np.stack([hover_todo * 20 - 1, -angle_todo * 20], 1), -1, 1).astype(np.float32)


def run(steps=None):
    """-> dict of arrays.  steps=None: until every env has ended an episode, plus TAIL steps."""
    from lander3_oracle import EPLEN, EPRET, Lander3Oracle
    ora = Lander3Oracle(N_ENVS, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=VIT, position_iterations=PIT)
    rec = {k: [] for k in ("actions", "obs2", "rew", "done", "ended")}
    ep_env, ep_ret, ep_len = [], [], []
    seen = np.zeros(N_ENVS, bool)
    o, t, stop = ora.obs(), 0, steps
    while t < (MAX_STEPS if stop is None else stop):
        a = heuristic(o)
        ret_before, len_before = ora.S[EPRET].copy(), ora.S[EPLEN].copy()
        obs2, rew, done, o, ended = ora.step(a)
        for k, v in zip(("actions", "obs2", "rew", "done", "ended"), (a, obs2, rew, done, ended)):
            rec[k].append(np.array(v))
        for e in np.nonzero(ended)[0]:
            ep_env.append(e)
            ep_ret.append(np.float32(ret_before[e] + rew[e]))
            ep_len.append(int(len_before[e]) + 1)
        seen |= ended.astype(bool)
        t += 1
        if stop is None and seen.all():
            stop = t + TAIL
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(seed=np.int64(SEED), n_envs=np.int64(N_ENVS), max_ep_len=np.int64(MAX_EP_LEN), velocity_iterations=np.int64(VIT),
               position_iterations=np.int64(PIT), final_state=ora.S.copy(), episode_env=np.array(ep_env, np.int64),
               episode_return=np.array(ep_ret, np.float32), episode_length=np.array(ep_len, np.int64), all_first_ended=np.bool_(seen.all()))
    return out


def first_episodes(g):
    """Per env, its FIRST finished episode: (return, length, landed) — landed = the +100 rest reward with both leg flags set."""
    rows = []
    for e in range(int(g["n_envs"])):
        t = np.nonzero(g["ended"][:, e])[0]
        if not len(t):
            rows.append((float("nan"), 0, False))
            continue
        t = int(t[0])
        k = int(np.nonzero(g["episode_env"] == e)[0][0])
        landed = bool(g["rew"][t, e] == 100.0 and g["obs2"][t, e, 6] == 1.0 and g["obs2"][t, e, 7] == 1.0)
        rows.append((float(g["episode_return"][k]), int(g["episode_length"][k]), landed))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lander3_heuristic.npz"))
    ap.add_argument("--report", default=None, help="also write the landing statistics to this text file")
    args = ap.parse_args()
    g = run()
    np.savez_compressed(args.out, **g)
    rows = first_episodes(g)
    lines = ["articulated lander oracle, %d / %d iterations, gym's heuristic controller, seed %d, env ids 0..%d, %d steps recorded"
             % (VIT, PIT, SEED, N_ENVS - 1, g["rew"].shape[0]),
             "first episode per env: return, length, landed (+100 rest reward with both leg flags set)"]
    lines += ["  env %d: %9.3f %5d %s" % (e, r, ln, ok) for e, (r, ln, ok) in enumerate(rows)]
    lines.append("landed %d of %d first episodes; mean first-episode return %.3f" % (sum(r[2] for r in rows), len(rows), np.mean([r[0] for r in rows])))
    lines.append("all finished episodes in the file: %d, mean return %.3f" % (len(g["episode_return"]), float(np.mean(g["episode_return"]))))
    print("\n".join(lines))
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))
    if args.report:
        with open(args.report, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
