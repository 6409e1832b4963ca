#!/usr/bin/env python3
"""One vector step of the n-step rollout worker on the ARTICULATED lander (RolloutDeviceNStep with opt.env_model = "articulated", 4096
envs, hidden [400, 300], Ln 8, save_freq 1, Wrapper repeat 3) in the policy phase, timed two ways in the same build:
  fused     opt.fused_nstep_rollout_articulated = True: the actor's forward + k_env3_step_nstep (ddrl_rollout_step_nstep_articulated)
  unfused   the flag off: observation copy, noise fill, versioned forward + head kernel, k_env3_step_wrapped, k_winq_push, k_mask_scan +
            k_store_masked, the adopt kernel, k_winq_begin — with Python between the launches
at gym's 180 / 60 iterations and at 8 / 3, the version store enabled and nothing installed inside the timed windows.
Method (tools/nstep_rollout_probe.py's): one process; HIP events around `iters` steps; `warm` untimed steps first; `reps` repetitions
per arm, the arms interleaved repetition by repetition.  Beside the ranges it writes the floor the solver alone sets: three times the
4096-env ddrl_env_step time recorded in profiles/lander3_step_time.txt (the Wrapper runs the physics three times per step).
No pass mark: the flag's default does not depend on what comes out.  Appends a block to profiles/lander3_nstep_rollout_time.txt (or the
file given) and prints one JSON line.
usage: python3 tools/lander3_nstep_rollout_probe.py [n_envs=4096] [iters=200] [reps=5] [out=profiles/lander3_nstep_rollout_time.txt]"""
import json
import os
import re
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "lander3_nstep_rollout_time.txt")
warm = 50
LIMIT = 320


def make(fused, vit, pit):
    opt = HyperParameters()
    opt.num_envs, opt.seed, opt.Ln, opt.save_freq, opt.action_repeat, opt.max_ep_len, opt.start_steps = n_envs, 1, 8, 1, 3, 3 * LIMIT, -1
    opt.buffer_size, opt.num_buffers = 1 << 18, 1
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", vit, pit
    opt.fused_nstep_rollout_articulated = fused
    keys, vals = Learner(opt).get_weights()
    ro = ddrl.RolloutDeviceNStep(ddrl.ParameterServer(keys, vals), ddrl.ReplayBufferNStep(opt), opt)
    assert ro._versions and ro.limit_steps == LIMIT and ro.env.model == "articulated"
    st = ro.env.get_state()
    st[10] = torch.arange(n_envs, device="cuda").float() % LIMIT      # episode length so far: the time limits come env by env
    ro.env.set_state(st)
    return ro


def window(ro):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ro.step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def solver_floor():
    """{"180/60": (median, min, max), "8/3": ...} of three ddrl_env_step launches, from profiles/lander3_step_time.txt."""
    try:
        text = open(os.path.join(ROOT, "profiles", "lander3_step_time.txt")).read()
    except OSError:
        return {}
    out = {}
    for key in ("180/60", "8/3"):
        m = re.search(r"articulated %s ([0-9.]+) us \(([0-9.]+) \.\. ([0-9.]+)\)" % key, text)
        if m:
            out[key] = [round(3 * float(g), 1) for g in m.groups()]
    return out


rng = lambda t: "%.1f .. %.1f" % (min(t), max(t))
res = {"n_envs": n_envs, "hidden": [400, 300], "Ln": 8, "save_freq": 1, "wrapper_repeat": 3, "iters_per_repetition": iters, "repetitions": reps,
       "warm_up_steps": warm, "device": torch.cuda.get_device_name(0), "launches_per_fused_step": 2,
       "three_env_steps_us_median_min_max": solver_floor()}
lines = []
for vit, pit in ((180, 60), (8, 3)):
    rf, ru = make(True, vit, pit), make(False, vit, pit)
    for ro in (rf, ru):
        for _ in range(warm):
            ro.step()
    torch.cuda.synchronize()
    assert rf._fused is True and rf._fused_live and ru._fused is False and rf._learning and ru._learning
    tf, tu = [], []
    for _ in range(reps):
        tf.append(window(rf))
        tu.append(window(ru))
    key = "%d/%d" % (vit, pit)
    res[key] = {"fused_us_per_step": [round(t, 1) for t in tf], "unfused_us_per_step": [round(t, 1) for t in tu],
                "windows_stored": rf.rbs[0].get_counts()[1]}
    floor = res["three_env_steps_us_median_min_max"].get(key)
    lines.append("%-7s fused %s us per step; unfused %s us per step; 3 x ddrl_env_step (profiles/lander3_step_time.txt) %s"
                 % (key, rng(tf), rng(tu), "%.1f us (%.1f .. %.1f)" % tuple(floor) if floor else "not recorded"))
    del rf, ru
line = json.dumps(res)
with open(out_path, "a") as f:
    f.write("==== tools/lander3_nstep_rollout_probe.py  %s  %s, %d envs, %d repetitions of %d steps per arm (min .. max), %d warm-up steps\n%s\n%s\n\n"
            % (time.strftime("%Y-%m-%d %H:%M:%S"), res["device"], n_envs, reps, iters, warm, "\n".join(lines), line))
print(line)
