"""Write profiles/walker_hardcore_census.txt: which branches of the Hardcore terrain the live test matrix (the four parameter sets of
tests/test_gpu_walker_hardcore.py::test_hardcore_bit_exact_vs_live_oracle, replayed on the oracle alone at 8 / 3 iterations) and the
crafted scenarios of tests/_walker_hardcore_scenarios.py (at 8 / 3 and at 180 / 60) reach, in env-steps per class
(tests/_walker_hardcore_scenarios.census_of), in the form of profiles/walker_census.txt.

    python tools/walker_hardcore_census.py [--out profiles/walker_hardcore_census.txt]

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

LIVE = [(64, 1, "random", 60, 12), (33, 7, "random", 60, 1600), (1, 3, "zero", 150, 1600), (130, 11, "random", 20, 7)]


def live_census():
    import _walker_hardcore_scenarios as sc
    import walker_hardcore_oracle as H
    census, steps, kinds = {}, 0, {H.STUMP: 0, H.STAIRS: 0, H.PIT: 0}
    for n, seed, policy, T, max_len in LIVE:
        ora = H.WalkerHardcoreOracle(n, seed=seed, max_ep_len=max_len, velocity_iterations=8, position_iterations=3)
        rs = np.random.RandomState(seed)
        for ks in ora.last_kinds:
            for k in ks:
                kinds[k] += 1
        for _ in range(T):
            a = rs.uniform(-1.3, 1.3, (n, 4)).astype(np.float32) if policy == "random" else np.zeros((n, 4), np.float32)
            ora.step(a)
            sc.census_of(ora, census)
            steps += n
    return census, steps, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walker_hardcore_census.txt"))
    args = ap.parse_args()
    import _walker_hardcore_scenarios as sc
    import walker_hardcore_oracle as H
    live, steps, kinds = live_census()
    fast, gym = sc.trajectory(*sc.FAST)[4], sc.trajectory(*sc.GYM)[4]
    lines = ["env-steps per class (tests/_walker_hardcore_scenarios.census_of); written by tools/walker_hardcore_census.py",
             "live: the four parameter sets of tests/test_gpu_walker_hardcore.py::test_hardcore_bit_exact_vs_live_oracle at 8 / 3 iterations, "
             "%d env-steps," % steps,
             "      replayed on the oracle alone; their first terrains hold %d stumps, %d stairs and %d pits"
             % (kinds[H.STUMP], kinds[H.STAIRS], kinds[H.PIT]),
             "crafted: tests/_walker_hardcore_scenarios.py, %d envs (%d classes interleaved: %s) x %d steps, at 8 / 3 and at 180 / 60"
             % (sc.N, len(sc.CLASSES), ", ".join(sc.CLASSES), sc.T),
             "%-34s %9s %12s %14s" % ("class", "live", "crafted 8/3", "crafted 180/60")]
    for k in sc.BRANCHES:
        lines.append("%-34s %9d %12d %14d" % (k, live.get(k, 0), fast.get(k, 0), gym.get(k, 0)))
    never = [k for k in sc.BRANCHES if not live.get(k, 0)]
    lines.append("classes the live matrix never reaches: %s" % (", ".join(never) or "none"))
    lines.append("(the walker starts 4.7 m before its first obstacle: every contact branch of the terrain is reached from the crafted states; "
                 "the obstacle-kind classes — pit walls, stair treads — are counted on the crafted envs built for them)")
    missing = [k for k in sc.BRANCHES if not fast.get(k, 0) or not gym.get(k, 0)]
    lines.append("classes the crafted scenarios miss: %s" % (", ".join(missing) or "none"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
