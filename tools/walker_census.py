"""Write profiles/walker_census.txt: which solver branches the walker's live test matrix (the four parameter sets of
tests/test_gpu_walker.py::test_walker_bit_exact_vs_live_oracle, replayed on the oracle alone at 8 / 3 iterations) and the crafted
scenarios of tests/_walker_scenarios.py (at 8 / 3 and at 180 / 60) reach, in env-steps per class (tests/_walker_scenarios.census_of).

    python tools/walker_census.py [--out profiles/walker_census.txt]

CPU only (NumPy); under a minute.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LIVE = [(64, 1, "heuristic", 300, 160), (33, 7, "random", 200, 1600), (1, 3, "zero", 150, 1600), (4096, 11, "random", 20, 12)]


def live_census():
    import _walker_scenarios as sc
    import walker_oracle as W
    census, steps, limit = {}, 0, 0
    for n, seed, policy, T, max_len in LIVE:
        ora = W.WalkerOracle(n, seed=seed, max_ep_len=max_len, velocity_iterations=8, position_iterations=3)
        rs, ctl, o = np.random.RandomState(seed), W.WalkerHeuristic(n), None
        o = ora.obs()
        for _ in range(T):
            a = ctl.act(o) if policy == "heuristic" else rs.uniform(-1.3, 1.3, (n, 4)).astype(np.float32) if policy == "random" else np.zeros((n, 4), np.float32)
            out = ora.step(a)
            o = out[3]
            ctl.restart(out[4])
            sc.census_of(ora, census)
            limit += int((out[4].astype(bool) & (out[2] == 0)).sum())
            steps += n
    census["time_limit"] = limit
    return census, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walker_census.txt"))
    args = ap.parse_args()
    import _walker_scenarios as sc
    live, steps = live_census()
    fast, gym = sc.trajectory(*sc.FAST)[4], sc.trajectory(*sc.GYM)[4]
    keys = list(live) + [k for k in fast if k not in live]
    lines = ["env-steps per class (tests/_walker_scenarios.census_of); written by tools/walker_census.py",
             "live: the four parameter sets of tests/test_gpu_walker.py::test_walker_bit_exact_vs_live_oracle at 8 / 3 iterations, %d env-steps,"
             % steps, "      replayed on the oracle alone",
             "crafted: tests/_walker_scenarios.py, %d envs (%d classes interleaved: %s) x %d steps, at 8 / 3 and at 180 / 60"
             % (sc.N, len(sc.CLASSES), ", ".join(sc.CLASSES), sc.T),
             "%-34s %9s %12s %14s" % ("class", "live", "crafted 8/3", "crafted 180/60")]
    for k in keys:
        lines.append("%-34s %9d %12d %14d" % (k, live.get(k, 0), fast.get(k, 0), gym.get(k, 0)))
    never = [k for k in keys if not live.get(k, 0)]
    lines.append("classes the live matrix never reaches: %s" % (", ".join(never) or "none"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
