"""Time one 4096-env ddrl_env_step_wrapped_walker (repeat = 3) of the bipedal walker at gym's 180 / 60 iterations and at 8 / 3, beside
THREE back-to-back ddrl_env_step launches on a twin env, all in this process by the same HIP-event loop (tools/walker_step_time.py's):
per figure five runs of `--steps` back-to-back launches (or triples of launches) after a warm-up of mixed steps, the median run and
the spread (min .. max) in microseconds per wrapped step / per triple, and their ratio.  Prints one line per iteration pair
(profiles/walker_wrapped_time.txt holds a recorded run).

    python tools/walker_wrapped_time.py [--envs 4096] [--steps 50] [--warmup 100]

Both envs start from the same seed and are warmed up by the same plain steps under random actions, so the timed launches see the same
mix of stance, flight and resets.  The wrapped launch makes one lidar pass and one state load / store where the three plain steps make
three of each, and runs the same three solver passes; the figures are a record, not a gate.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEAT = 3


def _timed(fn, steps, before, runs=5):
    import torch
    out = []
    for _ in range(runs):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
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
    import torch
    from distributed_drl_amd.env import VecBipedalWalker
    for vit, pit in ((180, 60), (8, 3)):
        wrapped, plain = (VecBipedalWalker(args.envs, seed=1, velocity_iterations=vit, position_iterations=pit) for _ in range(2))
        act = wrapped.sample_actions()
        for _ in range(args.warmup):
            wrapped.sample_actions(out=act)
            wrapped.step(act)
            plain.step(act)
        torch.cuda.synchronize()
        limit = -(-wrapped.max_ep_len // REPEAT)
        a_w, a_p = act.clone(), act.clone()

        def one_wrapped():
            wrapped.step_wrapped_walker(a_w, 0.3, 0.01, 5.0, REPEAT, limit)

        def three_plain():
            for _ in range(REPEAT):
                plain.step(a_p)

        # the wrapped step adds its action noise in place: each run starts from the drawn action again (outside the timed region)
        w = _timed(one_wrapped, args.steps, lambda: a_w.copy_(act))
        p = _timed(three_plain, args.steps, lambda: a_p.copy_(act))
        print("%d envs, %d / %d iterations, us, median of 5 runs of %d (min .. max): ddrl_env_step_wrapped_walker (repeat %d) %.1f (%.1f .. %.1f); "
              "%d x ddrl_env_step %.1f (%.1f .. %.1f); wrapped / plain: %.3f"
              % (args.envs, vit, pit, args.steps, REPEAT, w[0], w[1], w[2], REPEAT, p[0], p[1], p[2], w[0] / p[0]))


if __name__ == "__main__":
    main()
