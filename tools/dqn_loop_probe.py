"""The DQN / SQN learner's hot loop, eager against graph-replayed: updates per second of TrainDeviceDQN.run on one ring.

  A  updates_per_graph = 0    per update two host draws, ReplayBufferDQN.sample_batch_device + Learner.train (seven eager launches)
  B  updates_per_graph = 16   ddrl_dqn_loop_run: sampler and update on the device, replayed from captured graphs

Shapes: the lander's learner (obs 8, 4 actions, hidden 400 / 300, batch 128) and the small shape of tests/test_gpu_dqn_loop.py (hidden
64 / 48, batch 64), Double-DQN and SQN.  A and B alternate in one process, `--rounds` rounds of `--updates` updates each behind a warm-up
that includes B's capture; the host clock runs around work that ends in a synchronise; min / median / max over the rounds are printed.
No pushes (push_freq is out of reach), no stores: the loop alone.  With a library that lacks ddrl_dqn_loop_* (DDRL_LIB_PATH pointing at
an older build) only A runs — the parent's number.

    python tools/dqn_loop_probe.py [--updates 2000] [--rounds 3] [--per-graph 16] [--shapes lander,small] [--families ddqn,sqn]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"lander": (8, 4, [400, 300], 128), "small": (8, 4, [64, 48], 64)}


def make(family, shape, per_graph):
    from distributed_drl_amd import dqn
    from distributed_drl_amd.ps import ParameterServer
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import TrainDeviceDQN
    obs, act, hid, batch = shape
    opt = type("Opt", (), dict(obs_dim=obs, act_dim=act, hidden_size=list(hid), gamma=0.99, lr=1e-3, polyak=0.995, batch_size=batch, seed=3,
                               alpha=0.1, num_nodes=1, num_buffers=1, push_freq=10 ** 12, buffer_size=100000, variant=family))()
    L = dqn.LearnerSQN if family == "sqn" else dqn.Learner
    ps = ParameterServer(*L(opt).get_weights())
    rb = ReplayBufferDQN(opt, 0, seed=5)
    rs = np.random.RandomState(1)
    n = 10000
    rb.store_batch(*(torch.from_numpy(x).cuda() for x in (
        rs.randn(n, obs).astype(np.float32), rs.randint(0, act, n).astype(np.float32), rs.randn(n).astype(np.float32),
        rs.randn(n, obs).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32))))
    kw = dict(updates_per_graph=per_graph) if per_graph else {}
    return TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0), **kw), rb


def timed(trainer, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.run(n)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-graph", type=int, default=16)
    ap.add_argument("--shapes", default="lander,small")
    ap.add_argument("--families", default="ddqn,sqn")
    a = ap.parse_args()
    from distributed_drl_amd import _lib
    lib = _lib.load()
    has_loop = hasattr(lib, "ddrl_dqn_loop_run")
    print("library: %s   ddrl_dqn_loop_*: %s   device: %s" % (_lib.LIB_PATH, "yes" if has_loop else "no (A only)", torch.cuda.get_device_name(0)))
    print("%d updates per round, %d rounds, A and B alternated; updates/s as min / median / max over the rounds" % (a.updates, a.rounds))
    for sname in a.shapes.split(","):
        for family in a.families.split(","):
            ta, _ = make(family, SHAPES[sname], 0)
            tb, rb_b = make(family, SHAPES[sname], a.per_graph) if has_loop else (None, None)
            ta.run(4 * max(a.per_graph, 16))
            if tb:
                tb.run(4 * max(a.per_graph, 16))   # (one eager update, the capture, replays)
                assert tb.loop_info(rb_b)[1] == 1
            ra, rbs = [], []
            for _ in range(a.rounds):
                ra.append(timed(ta, a.updates))
                if tb:
                    rbs.append(timed(tb, a.updates))
            fmt = lambda r: "%9.0f / %9.0f / %9.0f" % (min(r), float(np.median(r)), max(r))
            line = "%-6s %-4s obs %d act %d hidden %s batch %d   A eager %s" % ((sname, family) + tuple(SHAPES[sname][:2]) + ("x".join(map(str, SHAPES[sname][2])), SHAPES[sname][3], fmt(ra)))
            if tb:
                line += "   B graph(%d) %s   B / A (medians) %.2f   us per update A %.1f  B %.1f" % (
                    a.per_graph, fmt(rbs), np.median(rbs) / np.median(ra), 1e6 / np.median(ra), 1e6 / np.median(rbs))
            print(line, flush=True)


if __name__ == "__main__":
    main()
