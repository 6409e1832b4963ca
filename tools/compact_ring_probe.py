#!/usr/bin/env python3
"""Config 5's learner iteration (28 224 / [400, 300] / batch 512) out of a ring far beyond the Infinity Cache, timed three ways:
  (i)   compact (uint8) ring, two calls: sample_batch_device + train
  (ii)  compact ring, Learner.train_from (whichever form it chooses there), and ddrl_dqn_step_ring called directly on the bytes
        (where the build takes a compact ring; the parent of that entry point answers DDRL_ERR_UNSUPPORTED and has no such arm)
  (iii) float32 ring, Learner.train_from
and the layer-1 forward stage alone: the float32 instance on a device batch from ddrl_dqn_step_timed's events (stage_times), and the
k_wide forward instances as they run inside (ii)'s direct call and (iii) from the profiler's device-side kernel records (null where the build of torch
records none).  One JSON line.  Each arm: `warm` untimed iterations, then `reps` windows of `iters` iterations between device events, the
arms interleaved window by window; median, min and max of the windows are reported, in microseconds per iteration.
DDRL_LIB_PATH selects another libddrl_hip.so: run the PARENT build and this one alternately and compare (ii).
usage: python3 tools/compact_ring_probe.py [rows=65536] [iters=100] [reps=7]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_drl_amd as ddrl  # noqa: E402
from distributed_drl_amd import _lib, dqn  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
warm, blk = 10, 2048


class O:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, save_dir = 84 * 84 * 4, 4, [400, 300], 0.99, 1e-4, 0.995, 512, 2, "."
    buffer_size = rows


def ring(compact):
    rb = ddrl.ReplayBufferDQN(O, 0, seed=1, compact_obs=compact)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(0, rows, blk):        # random pixels: zero-filled operands flatter the matrix pipes
        x = torch.randint(0, 256, (blk, O.obs_dim), device="cuda", generator=g).float()
        rb.store_batch(x, torch.randint(0, 4, (blk,), device="cuda", generator=g).float(), torch.randn(blk, device="cuda", generator=g),
                       x.flip(0), (torch.rand(blk, device="cuda", generator=g) < 0.05).float())
    return rb


def learner():
    ln = dqn.Learner(O, "learner")
    n, v = ln.get_weights()
    ln.set_weights(n[:1], [v[0] * np.float32(1.0 / 64)])
    return ln


cring, fring = ring(True), ring(False)
lib = _lib.load()
probe = learner()
fused_rc = lib.ddrl_dqn_step_ring(probe._h, cring._h, None, None, None, _lib.stream_ptr())   # does this build take the bytes?


def step_ring(ln):
    _lib.check(lib.ddrl_dqn_step_ring(ln._h, cring._h, _lib.dptr(ln.loss), None, None, _lib.stream_ptr()))


arms = [("compact_two_calls", learner(), lambda ln: ln.train(cring.sample_batch_device(512), 0)),
        ("compact_train_from", learner(), lambda ln: ln.train_from(cring, 0)),
        ("float32_train_from", learner(), lambda ln: ln.train_from(fring, 0))]
if fused_rc == 0:
    arms.append(("compact_step_ring", learner(), step_ring))
for _, ln, fn in arms:
    for _ in range(warm):
        fn(ln)
torch.cuda.synchronize()
times = {name: [] for name, _, _ in arms}
for _ in range(reps):
    for name, ln, fn in arms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn(ln)
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / iters * 1e3)

res = {"lib": os.environ.get("DDRL_LIB_PATH", "in-tree"), "rows": rows, "iters_per_window": iters, "windows": reps,
       "ddrl_dqn_step_ring_on_the_compact_ring": "rc 0" if fused_rc == 0 else "rc %d: train_from is the two-call fallback" % fused_rc}
for name, t in times.items():
    res[name + "_us"] = {"median": round(float(np.median(t)), 1), "min": round(min(t), 1), "max": round(max(t), 1)}

# layer-1 forward stage: the float32 instance on a device batch, between ddrl_dqn_step_timed's events
b = fring.sample_batch_device(512)
st = [arms[2][1].stage_times(b, reps=20)[1] * 1e3 for _ in range(reps)]
res["l1_forward_f32_batch_stage_us"] = {"median": round(float(np.median(st)), 1), "min": round(min(st), 1), "max": round(max(st), 1)}


def forward_kernels(ln, fn, n=20):
    """Mean device time (us) of the k_wide forward launches inside `n` iterations, per instance, from the profiler's kernel records."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                fn(ln)
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            nm = ev.name
            if "k_wide" not in nm or "k_wide_sk" in nm or "k_wide_reduce" in nm:
                continue
            fwd = "k_wide<true" in nm or "k_wideILb1E" in nm
            if not fwd:
                continue
            u8 = "32, true>" in nm or "Li32ELb1E" in nm
            out.setdefault("u8" if u8 else "f32", []).append(float(getattr(ev, "device_time", 0) or getattr(ev, "cuda_time", 0)))
        return {k: {"mean": round(float(np.mean(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "launches": len(v)} for k, v in out.items()} or None
    except Exception as e:  # a torch build without device-side records
        return {"unavailable": repr(e)}


if fused_rc == 0:
    res["l1_forward_kernel_us_in_compact_step_ring"] = forward_kernels(arms[3][1], arms[3][2])
res["l1_forward_kernel_us_in_float32_train_from"] = forward_kernels(arms[2][1], arms[2][2])
print(json.dumps(res))
