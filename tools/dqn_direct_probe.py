"""The captured DQN / SQN learner loop (TrainDeviceDQN, updates_per_graph=16) on the direct-operand door (opt.direct_learner:
ddrl_dqn_create_direct) against the generic one, in ONE process, alternating, at the four shapes of profiles/dqn_loop_before_after.txt.
Per shape and door: us per update of each round (a host clock around run(n) + a stream synchronise, after a warm-up that captures the
graphs), then the median and the 5th - 95th percentile over the rounds.  Recorded, not gated: profiles/dqn_direct_time.txt.

    python tools/dqn_direct_probe.py [--rounds 12] [--updates 4096] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("lander", "ddqn", 8, 4, (400, 300), 128), ("lander", "sqn", 8, 4, (400, 300), 128),
          ("small", "ddqn", 8, 4, (64, 48), 64), ("small", "sqn", 8, 4, (64, 48), 64)]


def trainer(family, obs, act, hid, batch, direct):
    from distributed_drl_amd import dqn
    from distributed_drl_amd.ps import ParameterServer
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import TrainDeviceDQN
    opt = type("Opt", (), dict(obs_dim=obs, act_dim=act, hidden_size=list(hid), gamma=0.99, lr=1e-3, polyak=0.995, batch_size=batch, seed=3,
                               alpha=0.1, num_nodes=1, num_buffers=1, push_freq=10 ** 9, buffer_size=8192, variant=family,
                               direct_learner=direct))()
    make = lambda o_: (dqn.LearnerSQN if family == "sqn" else dqn.Learner)(o_, "learner")  # noqa: E731
    rb = ReplayBufferDQN(opt, 0, seed=5)
    rs = np.random.RandomState(1)
    n = 4096
    rows = (rs.randn(n, obs), rs.randint(0, act, n), rs.randn(n), rs.randn(n, obs), rs.rand(n) < 0.2)
    rb.store_batch(*(torch.from_numpy(np.asarray(x, np.float32)).cuda() for x in rows))
    return TrainDeviceDQN([ParameterServer(*make(opt).get_weights())], [[rb]], opt, make_agent=make, rng=np.random.RandomState(0), updates_per_graph=16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--updates", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, family, obs, act, hid, batch in SHAPES:
        t = {"generic": trainer(family, obs, act, hid, batch, False), "direct": trainer(family, obs, act, hid, batch, True)}
        us = {k: [] for k in t}
        for v in t.values():
            v.run(64)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, v in t.items():                      # alternating: both doors see the same machine
                t0 = time.perf_counter()
                v.run(a.updates)
                torch.cuda.synchronize()
                us[k].append((time.perf_counter() - t0) / a.updates * 1e6)
        med = {k: float(np.median(x)) for k, x in us.items()}
        for k, x in us.items():
            lines.append("%-6s %-4s obs %d act %d hidden %dx%d batch %-4d %-8s us per update: median %6.2f  p5 %6.2f  p95 %6.2f  (%d rounds of %d)"
                         % (name, family, obs, act, hid[0], hid[1], batch, k, med[k], np.percentile(x, 5), np.percentile(x, 95), a.rounds, a.updates))
        lines.append("%-6s %-4s generic / direct (medians) %.2f" % (name, family, med["generic"] / med["direct"]))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
