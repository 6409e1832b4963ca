"""FreeRunningLoop over the three worker families at 4096 envs on the one-body lander, hidden (400, 300): per-segment phase times, the
two rates of one timed region on two streams against the same launches on one stream, the device time of the window ring's commit
(append_from) beside store_batch of the same rows from the same memory, and what the discrete learner's host-side push costs a
segment.  Arms are interleaved, every figure is a median of RUNS runs with its range.  Needs a GPU; writes --out (and prints it).

    python tools/free_workers_timeline.py [--out profiles/free_running_workers.txt] [--runs 5] [--segments 12]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_drl_amd as d  # noqa: E402
from distributed_drl_amd import _lib, dqn  # noqa: E402
from distributed_drl_amd.agent import HyperParameters, Learner  # noqa: E402
from distributed_drl_amd.workers import FreeRunningLoop, RolloutDevice, RolloutDeviceDQN, RolloutDeviceNStep, TrainDevice, TrainDeviceDQN  # noqa: E402

N_ENV, CAP, LN = 4096, 1000000, 8
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    xs = sorted(xs)
    return "%.3f [%.3f .. %.3f]" % (float(np.median(xs)), xs[0], xs[-1])


def sac_pair():
    opt = HyperParameters()
    opt.num_envs, opt.batch_size, opt.start_steps, opt.max_ep_len, opt.seed = N_ENV, 256, -1, 1000, 0
    rb = d.ReplayBufferSAC1(8, 2, CAP, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rb.store_batch(r(CAP, 8), torch.rand(CAP, 2, device="cuda", generator=g), r(CAP), r(CAP, 8), torch.zeros(CAP, device="cuda"))
    ps = d.ParameterServer(*Learner(opt).get_weights())
    tr = TrainDevice(ps, rb, opt, updates_per_graph=50)
    ro = RolloutDevice(ps, rb, opt)
    tr.run(100)
    ro.step(5)
    return ro, tr, opt, 100


def dqn_pair(push_freq=32):
    opt = type("Opt", (), dict(obs_dim=8, act_dim=4, hidden_size=[400, 300], gamma=0.99, lr=1e-3, polyak=0.995, batch_size=128, seed=0, alpha=0.1,
                               num_envs=N_ENV, max_ep_len=1000, start_steps=-1, num_nodes=1, num_buffers=1, push_freq=push_freq,
                               buffer_size=CAP, variant="ddqn"))()
    rb = d.ReplayBufferDQN(opt, 0, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    n = CAP // 2
    rb.store_batch(r(n, 8), torch.randint(0, 4, (n,), device="cuda", generator=g).float(), r(n), r(n, 8), torch.zeros(n, device="cuda"))
    ps = d.ParameterServer(*dqn.Learner(opt).get_weights())
    ro = RolloutDeviceDQN(ps, rb, opt)
    tr = TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: dqn.Learner(o_, job="learner"), rng=np.random.RandomState(0), updates_per_graph=16)
    tr.run(32)
    ro.step(5)
    return ro, tr, opt, 32


def nstep_pair():
    opt = HyperParameters()
    opt.num_envs, opt.batch_size, opt.start_steps, opt.seed, opt.Ln, opt.buffer_size, opt.num_buffers = N_ENV, 256, -1, 0, LN, CAP, 1
    rb = d.ReplayBufferNStep(opt, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    n = 100000
    rb.store_batch(r(n, LN + 1, 8), torch.rand(n, LN, 2, device="cuda", generator=g), r(n, LN), torch.zeros(n, LN, device="cuda"))
    ps = d.ParameterServer(*Learner(opt).get_weights())
    tr = TrainDevice(ps, rb, opt, updates_per_graph=50)
    ro = RolloutDeviceNStep(ps, rb, opt)
    tr.run(100)
    ro.step(LN + 2)       # the windows fill; _learning turns true on the host
    return ro, tr, opt, 100


def region(loop, segs):
    """(env steps / s, updates / s, ms per segment) of ONE timed region of `segs` segments, behind two warm-up segments."""
    loop.run(2)
    loop.drain()
    e0, u0 = loop.env_steps, loop.updates
    t0 = time.perf_counter()
    loop.run(segs)
    loop.drain()
    dt = time.perf_counter() - t0
    return (loop.env_steps - e0) / dt, (loop.updates - u0) / dt, dt / segs * 1e3


def family(name, pair, args):
    ro, tr, opt, n = pair
    torch.cuda.synchronize()
    k_max = min(512, CAP // N_ENV)      # a segment's transitions must fit the commit ring
    loop = FreeRunningLoop(ro, tr, opt, steps_per_segment=min(n, k_max), updates_per_segment=n, timing=True)
    loop.run(6)
    t = loop.segment_times(last=4)
    loop.close()
    k = int(max(4, min(k_max, round(min(n, k_max) * t["learner_ms"] / max(t["rollout_ms"], 1e-6)))))
    say("%s: %d envs, K = %d vector steps beside n = %d updates per segment (K calibrated from rollout %.3f ms / learner %.3f ms at K = %d)"
        % (name, N_ENV, k, n, t["rollout_ms"], t["learner_ms"], min(n, k_max)))
    one = torch.cuda.Stream()
    res = {"two": [], "one": []}
    phases = []
    for _ in range(args.runs):
        for arm in ("two", "one"):
            loop = FreeRunningLoop(ro, tr, opt, steps_per_segment=k, updates_per_segment=n, timing=(arm == "two"),
                                   streams=None if arm == "two" else (one, one))
            res[arm].append(region(loop, args.segments))
            if arm == "two":
                phases.append(loop.segment_times(last=args.segments))
            loop.close()
    for key in ("rollout_ms", "learner_ms", "commit_ms", "segment_ms"):
        say("  segment_times %-11s %s" % (key, med([p[key] for p in phases])))
    for arm, what in (("two", "two streams"), ("one", "one stream ")):
        say("  %s  env steps/s %s   updates/s %s   ms/segment %s" % (what, med([x[0] for x in res[arm]]), med([x[1] for x in res[arm]]),
                                                                    med([x[2] for x in res[arm]])))
    say("  (median [min .. max] of %d runs per arm, arms interleaved, %d segments per timed region; both rates of a line are from the "
        "same region)" % (args.runs, args.segments))
    say()
    return k


def commit_times(k, args):
    """The window ring's commit: append_from of a staging ring holding `rows` windows against store_batch of those rows out of the
    same staging memory (the existing kernel, the yardstick).  Device events around the one launch; the staging ring's counters are put
    back by a launch outside the timed bracket."""
    opt = HyperParameters()
    opt.Ln, opt.buffer_size, opt.num_buffers = LN, CAP, 1
    dst = d.ReplayBufferNStep(opt, seed=0)
    sopt = HyperParameters()
    sopt.Ln, sopt.buffer_size, sopt.num_buffers = LN, k * N_ENV, 1
    stage = d.ReplayBufferNStep(sopt)
    g = torch.Generator(device="cuda").manual_seed(2)
    for v in stage.rings().values():
        v.copy_(torch.randn(v.shape, device="cuda", generator=g))
    views = stage.rings()
    say("commit of a window staging ring (Ln = %d: rows of 72 + 16 + 8 + 8 = 104 floats), capacity %d x %d = %d rows, into a ring of %d rows"
        % (LN, k, N_ENV, k * N_ENV, CAP))
    for rows in (k * N_ENV, k * N_ENV * 3 // 4, N_ENV):
        t = {"append_from": [], "store_batch": []}
        for rep in range(args.runs + 2):
            for arm in ("append_from", "store_batch"):
                _lib.check(stage._lib.ddrl_replay_set_counts(stage._h, rows % stage.max_size, rows, 0, 0, _lib.stream_ptr()))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if arm == "append_from":
                    dst.append_from(stage)
                else:
                    dst.store_batch(*(views["buffer_" + c][:rows] for c in "oard"))
                e1.record()
                e1.synchronize()
                if rep >= 2:            # two warm-up rounds
                    t[arm].append(e0.elapsed_time(e1) * 1e3)
        mb = rows * 104 * 4 * 2 / 1e6
        say("  %7d rows (%.1f MB read + written)   append_from %s us   store_batch %s us" % (rows, mb, med(t["append_from"]), med(t["store_batch"])))
    say("  (device events around one launch, median [min .. max] of %d, arms interleaved; append_from's grid is sized for a full source)" % args.runs)
    say()


def dqn_push_cost(k, args):
    """What the host-side push (dqn.Learner.get_weights -> .cpu(), then ParameterServer.push) costs: the same loop with one push per
    segment against none, and the push call on its own behind a drained device."""
    res = {"push": [], "none": []}
    pairs = {"push": dqn_pair(32), "none": dqn_pair(10 ** 9)}
    for _ in range(args.runs):
        for arm in ("push", "none"):
            ro, tr, opt, n = pairs[arm]
            loop = FreeRunningLoop(ro, tr, opt, steps_per_segment=k, updates_per_segment=n)
            res[arm].append(region(loop, args.segments)[2])
            loop.close()
    tr = pairs["push"][1]
    alone = []
    for _ in range(args.runs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr._push()
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - t0) * 1e3)
    say("DQN, the host-side push (K = %d, n = 32, updates_per_graph 16): ms per segment with one push per segment %s, with none %s;"
        % (k, med(res["push"]), med(res["none"])))
    say("  difference of the medians %.3f ms per segment; TrainDeviceDQN._push() alone on a drained device %s ms"
        % (float(np.median(res["push"])) - float(np.median(res["none"])), med(alone[2:])))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "free_running_workers.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--segments", type=int, default=12)
    args = ap.parse_args()
    _lib.require_gpu()
    say("FreeRunningLoop over the three worker families — tools/free_workers_timeline.py on %s, one-body lander, hidden (400, 300)"
        % torch.cuda.get_device_name(0))
    say()
    family("SAC1 (RolloutDevice, TrainDevice; batch 256, updates_per_graph 50)", sac_pair(), args)
    torch.cuda.empty_cache()
    k_dqn = family("DQN (RolloutDeviceDQN, TrainDeviceDQN; ddqn, batch 128, updates_per_graph 16, push_freq 32)", dqn_pair(), args)
    torch.cuda.empty_cache()
    k_n = family("n-step (RolloutDeviceNStep, TrainDevice on a window ring; Ln 8, batch 256, updates_per_graph 50)", nstep_pair(), args)
    torch.cuda.empty_cache()
    commit_times(k_n, args)
    dqn_push_cost(k_dqn, args)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
