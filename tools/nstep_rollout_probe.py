#!/usr/bin/env python3
"""One vector step of the n-step rollout worker (RolloutDeviceNStep, 4096 envs, hidden [400, 300], Ln 8, save_freq 1, Wrapper repeat 3)
in the policy phase, timed two ways in the same build:
  fused     opt.fused_nstep_rollout = True:  the actor's forward + k_env_step_nstep (ddrl_rollout_step_nstep)
  unfused   opt.fused_nstep_rollout = False: the sequence the worker issued before that entry point existed — observation copy, noise
            fill, versioned forward + head kernel, k_env_step_wrapped, k_winq_push, k_mask_scan + k_store_masked, the adopt kernel,
            k_winq_begin — with Python between the launches
and in two settings, one arm pair each:
  one_version   the version store enabled and nothing installed inside the timed windows (the plain forward)
  versions_16   16 versions live: limit_steps 320 with staggered episode ends, one install (ParameterServer.push + the worker's pull)
                every 20 steps, installs inside the timed windows
Method: one process; HIP events around `iters` steps; `warm` untimed steps first; `reps` repetitions per arm, the arms interleaved
repetition by repetition; clocks and device state from rocm-smi (read-only queries) before and after.  Appends a block to
profiles/nstep_rollout.txt (or the file given) and prints one JSON line.  "default_on" = in BOTH settings the slowest fused repetition is
faster than the fastest unfused one (the rule behind the default of opt.fused_nstep_rollout).
usage: python3 tools/nstep_rollout_probe.py [n_envs=4096] [iters=200] [reps=5] [out=profiles/nstep_rollout.txt]"""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_drl_amd as ddrl  # noqa: E402
from distributed_drl_amd.agent import HyperParameters, Learner  # noqa: E402

n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "nstep_rollout.txt")
warm = 50
LIMIT, EVERY = 320, 20


def smi():
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--showuse", "--showtemp"], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:
        return "rocm-smi unavailable: %r" % (e,)


def make(fused, install_every):
    opt = HyperParameters()
    opt.num_envs, opt.seed, opt.Ln, opt.save_freq, opt.action_repeat, opt.max_ep_len, opt.start_steps = n_envs, 1, 8, 1, 3, 3 * LIMIT, -1
    opt.buffer_size, opt.num_buffers, opt.fused_nstep_rollout = 1 << 18, 1, fused
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    ro = ddrl.RolloutDeviceNStep(ps, ddrl.ReplayBufferNStep(opt), opt)
    assert ro._versions and ro.limit_steps == LIMIT
    st = ro.env.get_state()
    st[10] = torch.arange(n_envs, device="cuda").float() % LIMIT      # episode length so far: the time limits come env by env
    ro.env.set_state(st)
    count = [0]

    def step():
        if install_every and count[0] % install_every == 0:
            ps.push(keys, vals)               # an install: the same numbers as a new version
        count[0] += 1
        ro.step()

    return ro, step


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


before = smi()
res = {"n_envs": n_envs, "hidden": [400, 300], "Ln": 8, "save_freq": 1, "wrapper_repeat": 3, "iters_per_repetition": iters, "repetitions": reps,
       "warm_up_steps": warm, "device": torch.cuda.get_device_name(0), "launches_per_fused_step": 2}
ok = True
for name, every, pre in (("one_version", 0, 0), ("versions_16", EVERY, LIMIT + 8)):
    (rf, fused), (ru, unfused) = make(True, every), make(False, every)
    for fn in (fused, unfused):
        for _ in range(pre + warm):            # versions_16: every env through an episode end first, 16 versions live from there on
            fn()
    torch.cuda.synchronize()
    assert rf._fused is True and rf._fused_live and ru._fused is False and rf._learning and ru._learning
    tf, tu = [], []
    for _ in range(reps):
        tf.append(window(fused))
        tu.append(window(unfused))
    slots, vs = rf.actor.version_state()
    res[name] = {"fused_us_per_step": [round(t, 2) for t in tf], "unfused_us_per_step": [round(t, 2) for t in tu],
                 "slowest_fused_faster_than_fastest_unfused": max(tf) < min(tu), "steps_per_install": every,
                 "versions_live_now": int(torch.unique(slots).numel()), "out_of_slots": vs["out_of_slots"],
                 "windows_stored": rf.rbs[0].get_counts()[1]}
    ok = ok and max(tf) < min(tu)
    del rf, ru, fused, unfused
res["default_on"] = ok
after = smi()
line = json.dumps(res)
with open(out_path, "a") as f:
    f.write("==== tools/nstep_rollout_probe.py  %s\n%s\n-- device state before\n%s\n-- device state after\n%s\n\n"
            % (time.strftime("%Y-%m-%d %H:%M:%S"), line, before, after))
print(line)
