#!/usr/bin/env python3
"""Sharded replay on window rings: the fed captured loop and an owner's block draw, window ring against transition ring.  One JSON line.

loop   the captured device loop (ddrl_loop, 50 updates per graph, batch 256) following an ALL-REMOTE feed plan: on a transition ring,
       and on an Ln = 8 window ring fed the same blocks (the fed copy moves identical bytes).  Updates/s, `reps` timed repetitions.
many   an owner's block draw of 2^18 rows (1024 batches of 256): ReplayBuffer.sample_many on a transition ring, and the folded
       ReplayBufferNStep.sample_many on an Ln = 8 window ring of as many rows.  Milliseconds per block (device time between events).

DDRL_LIB_PATH selects another libddrl_hip.so: a build without ddrl_replay_sample_many_nstep (the parent of the change that added fed
window rings) reports the transition-ring figures only — what the window-ring figures are judged against.
usage: python3 tools/nstep_feed_probe.py [loop|many|both] [updates_per_rep=2000] [reps=5]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_drl_amd as ddrl  # noqa: E402
from distributed_drl_amd.agent import HyperParameters, Learner  # noqa: E402
from distributed_drl_amd.partition import _Loop  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "both"
n_upd = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rows, Ln, B = 100000, 8, 256
opt = HyperParameters()
opt.batch_size, opt.Ln, opt.buffer_size = B, Ln, rows
rs = np.random.RandomState(0)
g = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).cuda()
has_windows = hasattr(ddrl._lib.load(), "ddrl_replay_sample_many_nstep")
nf = B * (2 * 8 + 2 + 2)


def transition_ring(n=rows):
    rb = ddrl.ReplayBufferSAC1(8, 2, n, seed=1)
    rb.store_batch(g(n, 8), g(n, 2).clamp(-1, 1), g(n), g(n, 8), (torch.rand(n, device="cuda") < 0.05).float())
    return rb


def window_ring(n=rows):
    o = HyperParameters()
    o.batch_size, o.Ln, o.buffer_size = B, Ln, n
    rb = ddrl.ReplayBufferNStep(o, seed=1)
    rb.store_batch(g(n, Ln + 1, 8), g(n, Ln, 2).clamp(-1, 1), g(n, Ln), (torch.rand(n, Ln, device="cuda") < 0.05).float())
    return rb


def loop_rate(rb, regions):
    """Every update of every repetition is a fed entry: the plan covers a whole repetition and is re-attached (position 0) before each."""
    K = [k for _, k in regions]
    plan = torch.tensor([(i % len(K)) << 24 | (i // len(K)) % K[i % len(K)] for i in range(n_upd)], dtype=torch.int32, device="cuda")
    learner = Learner(opt, job="learner", index=0)
    loop = _Loop(learner, rb, 50)
    rb.set_feed(plan, B, regions)
    loop.run(200)                    # capture + warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        rb.set_feed(plan, B, regions)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(n_upd)
        torch.cuda.synchronize()
        out.append(n_upd / (time.perf_counter() - t0))
    assert rb.get_counts()[0] == 0   # raises the sticky error a plan entry out of range would have left; not one update drew locally
    return out


def many_ms(rb, count=1024):
    flat = torch.empty(count * nf, dtype=torch.float32, device="cuda")
    for _ in range(3):
        rb.sample_many(B, count, flat)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            rb.sample_many(B, count, flat)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / 10)
    return out


res = {"lib": os.environ.get("DDRL_LIB_PATH", "in-tree"), "batch": B, "Ln": Ln, "rows": rows}
if what in ("loop", "both"):
    res["updates_per_rep"] = n_upd
    owners = [transition_ring(20000), transition_ring(20000)]   # two owners' blocks of 64 batches: transition-shaped on either ring
    regions = [(o.sample_many(B, 64, torch.empty(64 * nf, dtype=torch.float32, device="cuda")), 64) for o in owners]
    for name, make in (("loop_transition_ring", transition_ring), ("loop_window_ring", window_ring)):
        if name == "loop_window_ring" and not has_windows:
            continue
        r = loop_rate(make(), regions)
        res[name] = {"updates_per_s_median": float(np.median(r)), "updates_per_s": [round(x, 1) for x in r]}
if what in ("many", "both"):
    n = 1 << 18
    for name, make in (("many_transition_ring", transition_ring), ("many_window_ring", window_ring)):
        if name == "many_window_ring" and not has_windows:
            continue
        r = many_ms(make(n))
        res[name] = {"ms_per_block_median": float(np.median(r)), "us_per_batch_median": float(np.median(r)) * 1000 / 1024, "ms_per_block": [round(x, 4) for x in r]}
print(json.dumps(res))
