"""Generate tests/golden/walker_heuristic.npz: the walker's oracle (tests/walker_oracle.py) at gym's 180 velocity / 60 position
iterations under gym's own walking heuristic (WalkerHeuristic: the state machine of bipedal_walker.py's __main__, restated from
memory), 8 envs with consecutive env ids from one recorded seed, STEPS steps with a time limit inside the run so that every env ends
at least one episode.  Data only: the seed and iteration counts, per step the actions, obs2, rew, done, next_obs and ended, the final
state block, and per finished episode its env, return, length, distance (the hull's x at the end minus its x at build) and how it
ended (0 time limit, 1 hull contact, 2 x < 0, 3 end of the terrain).

    python tools/gen_walker_golden.py [--out tests/golden/walker_heuristic.npz] [--report profiles/walker_heuristic.txt]

CPU only (NumPy); about a minute.  tests/test_walker_cpu.py regenerates the first steps and compares bit for bit;
tests/test_gpu_walker.py replays the recorded actions through the HIP kernel.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, N_ENVS, MAX_EP_LEN, VIT, PIT, STEPS = 1, 8, 300, 180, 60, 320
KEYS = ("actions", "obs2", "rew", "done", "next_obs", "ended")
ENDINGS = ("time limit", "hull contact", "x < 0", "end of the terrain")


def run(steps=STEPS):
    """-> dict of arrays."""
    from walker_oracle import EPLEN, EPRET, PX, X0, WalkerHeuristic, WalkerOracle
    ora = WalkerOracle(N_ENVS, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=VIT, position_iterations=PIT)
    ctl = WalkerHeuristic(N_ENVS)
    rec = {k: [] for k in KEYS}
    ep = {k: [] for k in ("env", "ret", "len", "dist", "how")}
    o = ora.obs()
    for _ in range(steps):
        a = ctl.act(o)
        ret_before, len_before = ora.S[EPRET].copy(), ora.S[EPLEN].copy()
        obs2, rew, done, o, ended = ora.step(a)
        last = ora.last
        for k, v in zip(KEYS, (a, obs2, rew, done, o, ended)):
            rec[k].append(np.array(v))
        for e in np.nonzero(ended)[0]:
            ep["env"].append(e)
            ep["ret"].append(np.float32(ret_before[e] + rew[e]))
            ep["len"].append(int(len_before[e]) + 1)
            ep["dist"].append(np.float32(last["state"][PX, e] - X0))
            ep["how"].append(1 if last["game_over"][e] else 2 if last["neg_x"][e] else 3 if last["finish"][e] else 0)
        ctl.restart(ended)
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(seed=np.int64(SEED), n_envs=np.int64(N_ENVS), max_ep_len=np.int64(MAX_EP_LEN), velocity_iterations=np.int64(VIT),
               position_iterations=np.int64(PIT), final_state=ora.S.copy(), episode_env=np.array(ep["env"], np.int64),
               episode_return=np.array(ep["ret"], np.float32), episode_length=np.array(ep["len"], np.int64),
               episode_distance=np.array(ep["dist"], np.float32), episode_ending=np.array(ep["how"], np.int64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "walker_heuristic.npz"))
    ap.add_argument("--report", default=None, help="also write the per-episode statistics to this text file")
    args = ap.parse_args()
    g = run()
    np.savez_compressed(args.out, **g)
    lines = ["walker oracle, %d / %d iterations, gym's walking heuristic, seed %d, env ids 0..%d, max_ep_len %d, %d steps recorded"
             % (VIT, PIT, SEED, N_ENVS - 1, MAX_EP_LEN, g["rew"].shape[0]),
             "every finished episode: env, length, return, distance walked in metres (hull x at the end - x at build), how it ended"]
    for e, ln, r, d, how in zip(g["episode_env"], g["episode_length"], g["episode_return"], g["episode_distance"], g["episode_ending"]):
        lines.append("  env %d: %5d %9.3f %8.3f  %s" % (e, ln, r, d, ENDINGS[int(how)]))
    n = len(g["episode_return"])
    lines.append("%d episodes: %d by the time limit, %d by hull contact, %d by x < 0, %d at the end of the terrain; mean return %.3f, mean "
                 "distance %.3f m, mean speed %.3f m/s" % (n, *(int((g["episode_ending"] == k).sum()) for k in (0, 1, 2, 3)),
                                                           float(np.mean(g["episode_return"])), float(np.mean(g["episode_distance"])),
                                                           float(g["episode_distance"].sum() / (g["episode_length"].sum() / 50.0))))
    print("\n".join(lines))
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))
    if args.report:
        with open(args.report, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
