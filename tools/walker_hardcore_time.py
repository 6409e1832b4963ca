"""Time one 4096-env ddrl_env_step of the bipedal walker on the HARDCORE terrain (csrc/walker.hip's kernels at terrain mode 1) beside
the grass walker's (the same kernels at mode 0: the reference side) at gym's 180 / 60 iterations and at 8 / 3, and the wrapped
step (ddrl_env_step_wrapped_walker, repeat 3) of both, all in this process by tools/walker_step_time.py's method (the HIP-event loop of
tools/lander3_step_time.py): per figure five runs of `--steps` back-to-back launches after a warm-up of mixed steps, the median run and
the spread (min .. max) in microseconds per launch, and the ratio Hardcore / grass.

    python tools/walker_hardcore_time.py [--envs 4096] [--steps 50] [--warmup 100] [--out profiles/walker_hardcore_step_time.txt]

What the ratio holds: eight more contact slots in every sweep (inactive unless a foot is at a box side), the box lookup per corner and
hull vertex, the lidar's box edges, and at an episode's end the terrain generator with its box table.  A record, not a gate.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPEAT = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from distributed_drl_amd.env import VecBipedalWalker
    from lander3_step_time import time_env
    from walker_wrapped_time import _timed
    lines = ["python tools/walker_hardcore_time.py   (one MI355X; a record, not a gate)"]
    for vit, pit in ((180, 60), (8, 3)):
        med = {}
        parts = []
        for terrain in ("grass", "hardcore"):
            env = VecBipedalWalker(args.envs, seed=1, velocity_iterations=vit, position_iterations=pit, terrain=terrain)
            med[terrain], lo, hi = time_env(env, args.steps, args.warmup)   # the warm-up: 100 mixed steps under random actions
            parts.append("%s %.1f us (%.1f .. %.1f)" % (terrain, med[terrain], lo, hi))
            act = env.sample_actions()
            a_w = act.clone()
            limit = -(-env.max_ep_len // REPEAT)
            w, wlo, whi = _timed(lambda: env.step_wrapped_walker(a_w, 0.3, 0.01, 5.0, REPEAT, limit), args.steps, lambda: a_w.copy_(act))
            med[terrain + " wrapped"] = w
            parts.append("%s wrapped (repeat %d) %.1f us (%.1f .. %.1f)" % (terrain, REPEAT, w, wlo, whi))
            del env
            torch.cuda.synchronize()
        lines.append("%d envs, %d / %d iterations, us per launch, median of 5 runs of %d launches (min .. max): %s; hardcore / grass: "
                     "%.3f (ddrl_env_step), %.3f (ddrl_env_step_wrapped_walker)"
                     % (args.envs, vit, pit, args.steps, "; ".join(parts), med["hardcore"] / med["grass"],
                        med["hardcore wrapped"] / med["grass wrapped"]))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
