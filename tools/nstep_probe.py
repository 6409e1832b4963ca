#!/usr/bin/env python3
"""Rate of the device loop (TrainDevice.run, graph-captured) at batch 256 on an Ln = 8 n-step window ring and on a transition ring of the
same number of rows.  One JSON line: updates/s of each, `reps` timed repetitions (median and all values).  The window-ring rate is to be
judged against the transition-ring rate of the PARENT build (DDRL_LIB_PATH selects another libddrl_hip.so; a build without the n-step
entry points reports the transition ring only).
usage: python3 tools/nstep_probe.py [updates_per_rep=2000] [reps=5]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_drl_amd as ddrl  # noqa: E402
from distributed_drl_amd.agent import HyperParameters  # noqa: E402
from distributed_drl_amd.workers import TrainDevice  # noqa: E402

n_upd = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows, Ln = 100000, 8
opt = HyperParameters()
opt.batch_size, opt.Ln, opt.buffer_size, opt.push_freq = 256, Ln, rows, 1 << 30
rs = np.random.RandomState(0)
g = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).cuda()


def transition_ring():
    rb = ddrl.ReplayBufferSAC1(8, 2, rows, seed=1)
    rb.store_batch(g(rows, 8), g(rows, 2).clamp(-1, 1), g(rows), g(rows, 8), (torch.rand(rows, device="cuda") < 0.05).float())
    return rb


def window_ring():
    rb = ddrl.ReplayBufferNStep(opt, seed=1)
    rb.store_batch(g(rows, Ln + 1, 8), g(rows, Ln, 2).clamp(-1, 1), g(rows, Ln), (torch.rand(rows, Ln, device="cuda") < 0.05).float())
    return rb


def rate(rb):
    td = TrainDevice(None, rb, opt, updates_per_graph=50)
    td.run(200)                      # capture + warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        td.run(n_upd)
        torch.cuda.synchronize()
        out.append(n_upd / (time.perf_counter() - t0))
    return out


res = {"lib": os.environ.get("DDRL_LIB_PATH", "in-tree"), "batch": 256, "Ln": Ln, "rows": rows, "updates_per_rep": n_upd}
for name, make in (("transition_ring", transition_ring), ("window_ring", window_ring)):
    if name == "window_ring" and not hasattr(ddrl._lib.load(), "ddrl_replay_sample_nstep"):
        continue
    r = rate(make())
    res[name] = {"updates_per_s_median": float(np.median(r)), "updates_per_s": [round(x, 1) for x in r]}
print(json.dumps(res))
