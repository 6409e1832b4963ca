"""Time one 4096-env ddrl_env_step of the bipedal walker at gym's 180 / 60 iterations and at 8 / 3, beside the articulated lander's
step at the same counts and the one-body step, all in this process by the same HIP-event loop (tools/lander3_step_time.py's): per
figure five runs of `--steps` back-to-back launches after a warm-up of mixed steps, the median run and the spread (min .. max) in
microseconds per launch.  Prints one line (profiles/walker_step_time.txt holds a recorded one).

    python tools/walker_step_time.py [--envs 4096] [--steps 50] [--warmup 100]

The envs are warmed up under random actions first, so the timed steps see the mix of stance, flight and resets a rollout sees (the
position sweeps leave early per env, so the cost depends on the state).  The figure is a record, not a gate.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    from distributed_drl_amd.env import VecBipedalWalker, VecLunarLander
    from lander3_step_time import time_env
    parts, med = [], {}
    for name, make in (("walker 180/60", lambda: VecBipedalWalker(args.envs, seed=1, velocity_iterations=180, position_iterations=60)),
                       ("walker 8/3", lambda: VecBipedalWalker(args.envs, seed=1, velocity_iterations=8, position_iterations=3)),
                       ("articulated 180/60", lambda: VecLunarLander(args.envs, seed=1, model="articulated", velocity_iterations=180,
                                                                     position_iterations=60)),
                       ("articulated 8/3", lambda: VecLunarLander(args.envs, seed=1, model="articulated", velocity_iterations=8,
                                                                  position_iterations=3)),
                       ("one-body", lambda: VecLunarLander(args.envs, seed=1))):
        med[name], lo, hi = time_env(make(), args.steps, args.warmup)
        parts.append("%s %.1f us (%.1f .. %.1f)" % (name, med[name], lo, hi))
    print("ddrl_env_step, %d envs, us per launch, median of 5 runs of %d launches (min .. max): %s; walker / articulated: %.2f at 180/60, "
          "%.2f at 8/3" % (args.envs, args.steps, "; ".join(parts), med["walker 180/60"] / med["articulated 180/60"],
                           med["walker 8/3"] / med["articulated 8/3"]))


if __name__ == "__main__":
    main()
