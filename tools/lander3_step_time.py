"""Time one 4096-env ddrl_env_step of the articulated lander at gym's 180 / 60 iterations and at 8 / 3, beside the one-body step,
all in this process by the same HIP-event loop: per figure five runs of `--steps` back-to-back launches after a warm-up, the median
run and the spread (min .. max) in microseconds per launch.  Prints one line (profiles/lander3_step_time.txt holds a recorded one).

    python tools/lander3_step_time.py [--envs 4096] [--steps 50] [--warmup 100]

The envs are warmed up under random actions first, so the timed steps see the mix of flight, contact and resets a rollout sees
(the position sweeps leave early per env, so the cost depends on the state); the one-body figure is ddrl_env_step's own kernel,
not the fused rollout launch DESIGN quotes elsewhere.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def time_env(env, steps, warmup, runs=5):
    import torch
    act = env.sample_actions()
    for _ in range(warmup):
        env.step(env.sample_actions(out=act))
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        env.sample_actions(out=act)
        e0.record()
        for _ in range(steps):
            env.step(act)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / steps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    from distributed_drl_amd.env import VecLunarLander
    parts = []
    for name, kw in (("articulated 180/60", dict(model="articulated", velocity_iterations=180, position_iterations=60)),
                     ("articulated 8/3", dict(model="articulated", velocity_iterations=8, position_iterations=3)),
                     ("one-body", dict())):
        med, lo, hi = time_env(VecLunarLander(args.envs, seed=1, **kw), args.steps, args.warmup)
        parts.append("%s %.1f us (%.1f .. %.1f)" % (name, med, lo, hi))
    print("ddrl_env_step, %d envs, us per launch, median of 5 runs of %d launches (min .. max): %s" % (args.envs, args.steps, "; ".join(parts)))


if __name__ == "__main__":
    main()
