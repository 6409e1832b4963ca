"""The eager DQN / SQN update (Learner.train: ddrl_dqn_step) on the direct-operand tail (opt.direct_learner = "tail":
ddrl_dqn_create_direct_tail) against the generic handle, in ONE process, alternating, at config 5's shape (layer 1 on wide_l1.h) and at a
mid width where layer 1 is k_gemm.  Per shape and door: us per update of each round (a host clock around n train() calls on resident
device tensors + a stream synchronise, after a warm-up), then the median and the 5th - 95th percentile over the rounds.
Recorded, not gated: profiles/dqn_direct_tail_time.txt.

    python tools/dqn_direct_tail_probe.py [--rounds 12] [--updates 200] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("config5", "ddqn", 84 * 84 * 4, 4, (400, 300), 512), ("config5", "sqn", 84 * 84 * 4, 4, (400, 300), 512),
          ("mid", "ddqn", 128, 4, (400, 300), 128), ("mid", "sqn", 128, 4, (400, 300), 128)]


def learner(family, obs, act, hid, batch, direct):
    from distributed_drl_amd import dqn
    opt = type("Opt", (), dict(obs_dim=obs, act_dim=act, hidden_size=list(hid), gamma=0.99, lr=1e-4, polyak=0.995, batch_size=batch, seed=3,
                               alpha=0.1, direct_learner=direct))()
    return (dqn.LearnerSQN if family == "sqn" else dqn.Learner)(opt, "learner")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, family, obs, act, hid, batch in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(1)
        scale = 1.0 / max(1.0, (obs / 64.0) ** 0.5)          # keeps the layer-1 pre-activations O(1) at 28 224 inputs
        b = dict(obs1=torch.randn(batch, obs, device="cuda", generator=gen) * scale, obs2=torch.randn(batch, obs, device="cuda", generator=gen) * scale,
                 acts=torch.randint(0, act, (batch,), device="cuda", generator=gen).float(), rews=torch.randn(batch, device="cuda", generator=gen),
                 done=(torch.rand(batch, device="cuda", generator=gen) < 0.2).float())
        t = {"generic": learner(family, obs, act, hid, batch, False), "tail": learner(family, obs, act, hid, batch, "tail")}
        us = {k: [] for k in t}
        for v in t.values():
            for it in range(20):
                v.train(b, it)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, v in t.items():                      # alternating: both doors see the same machine
                t0 = time.perf_counter()
                for it in range(a.updates):
                    v.train(b, it)
                torch.cuda.synchronize()
                us[k].append((time.perf_counter() - t0) / a.updates * 1e6)
        med = {k: float(np.median(x)) for k, x in us.items()}
        for k, x in us.items():
            lines.append("%-7s %-4s obs %d act %d hidden %dx%d batch %-4d %-8s us per update: median %7.2f  p5 %7.2f  p95 %7.2f  (%d rounds of %d)"
                         % (name, family, obs, act, hid[0], hid[1], batch, k, med[k], np.percentile(x, 5), np.percentile(x, 95), a.rounds, a.updates))
        lines.append("%-7s %-4s generic - tail (medians) %.2f us, generic / tail %.3f" % (name, family, med["generic"] - med["tail"], med["generic"] / med["tail"]))
        del t
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
