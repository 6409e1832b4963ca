#!/usr/bin/env python3
"""One vector step of the discrete rollout (4096 envs, hidden [400, 300], Double-DQN and SQN), timed two ways:
  fused     ddrl_rollout_step_discrete: the Q-forward launch + the select / physics / store launch
  baseline  the same step from the API the build had before that entry point: Learner.q_values -> torch selection (argmax / coin flip, or
            a multinomial draw from softmax(q1 / alpha)) -> the action table as a torch lookup -> VecLunarLander.step -> store_batch
Method: one process; HIP events around `iters` steps; `warm` untimed steps first; `reps` repetitions per arm, the arms interleaved
repetition by repetition; clocks and device state from rocm-smi (read-only queries) before and after.  Appends a block to
profiles/discrete_rollout.txt (or the file given) and prints one JSON line.  "done" = the slowest fused repetition is faster than the
fastest baseline repetition.
--versions K adds two arms per family on handles with a version store (dqn.Actor.enable_versions: RolloutDeviceDQN(adopt="episode")):
  store_idle     the store enabled and no install for more than max_ep_len steps: the plain launch pair behind a host-side comparison
  versions_live  K versions live: time limit VER_EP_LEN with staggered episode ends, one install (set_weights) every VER_EP_LEN / K steps,
                 installs inside the timed windows (under rocprofv3 --kernel-trace: k_actor_fwd<.., true>, k_env_step_q<.., true> and
                 k_version_plan + k_pack_version at the installs)
Without the flag the output is what it was before the flag existed.
usage: python3 tools/discrete_rollout_probe.py [--versions K] [n_envs=4096] [iters=200] [reps=5] [out=profiles/discrete_rollout.txt]"""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_drl_amd as ddrl  # noqa: E402
from distributed_drl_amd import _lib, dqn  # noqa: E402
from distributed_drl_amd.env import VecLunarLander, VecLunarLanderDiscrete  # noqa: E402

n_versions = 0
if "--versions" in sys.argv:
    k = sys.argv.index("--versions")
    n_versions = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
VER_EP_LEN = 320
n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "discrete_rollout.txt")
warm = 50


def smi():
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "--showuse", "--showtemp"], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:
        return "rocm-smi unavailable: %r" % (e,)


class O:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha, save_dir = 8, 4, [400, 300], 0.99, 1e-3, 0.995, 128, 2, 0.1, "."
    buffer_size = 1 << 20


lib = _lib.load()
TABLE = torch.tensor([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], device="cuda")


def make(family):
    cls = dqn.ActorSQN if family == "sqn" else dqn.Actor
    f_actor, b_actor = cls(O, "worker", max_rows=n_envs), cls(O, "worker", max_rows=n_envs)
    f_env, b_env = VecLunarLanderDiscrete(n_envs, seed=1), VecLunarLander(n_envs, seed=1)
    f_rb, b_rb = ddrl.ReplayBufferDQN(O, 0), ddrl.ReplayBufferDQN(O, 0)
    _lib.check(lib.ddrl_rollout_begin_discrete(f_env._h, f_actor._h, _lib.stream_ptr()))
    act = torch.empty(n_envs, device="cuda")
    o = torch.empty_like(b_env.obs)

    def fused():
        _lib.check(lib.ddrl_rollout_step_discrete(f_env._h, f_actor._h, f_rb._h, 1, 0, 0.97, f_actor._noise_seed, f_actor._noise_ctr,
                                                  _lib.dptr(act), None, None, _lib.stream_ptr()))
        f_actor._noise_ctr += 2 * n_envs

    def baseline():
        o.copy_(b_env.obs)
        q = b_actor.q_values(o)
        if family == "sqn":
            a = torch.multinomial(torch.softmax(q / O.alpha, dim=1), 1).reshape(-1)
        else:
            a = torch.where(torch.rand(n_envs, device="cuda") < 0.97, q.argmax(dim=1), torch.randint(0, 4, (n_envs,), device="cuda"))
        o2, r, d, _, _ = b_env.step(TABLE[a])
        b_rb.store_batch(o, a.float(), r, o2, d)

    return fused, baseline


def make_versions(family, k_versions):
    """(store_idle, versions_live, state): two more fused arms on handles with a version store.  store_idle is the fused arm of make() —
    same envs, same seed, same time limit — with the store enabled and never installed into."""
    cls = dqn.ActorSQN if family == "sqn" else dqn.Actor
    i_actor, i_env, i_rb = cls(O, "worker", max_rows=n_envs), VecLunarLanderDiscrete(n_envs, seed=1), ddrl.ReplayBufferDQN(O, 0)
    _lib.check(lib.ddrl_rollout_begin_discrete(i_env._h, i_actor._h, _lib.stream_ptr()))
    i_actor.enable_versions(min(2048, min(n_envs, 1000) + 2))
    i_act = torch.empty(n_envs, device="cuda")

    def idle():
        _lib.check(lib.ddrl_rollout_step_discrete(i_env._h, i_actor._h, i_rb._h, 1, 0, 0.97, i_actor._noise_seed, i_actor._noise_ctr,
                                                  _lib.dptr(i_act), None, None, _lib.stream_ptr()))
        i_actor._noise_ctr += 2 * n_envs

    actor, env, rb = cls(O, "worker", max_rows=n_envs), VecLunarLanderDiscrete(n_envs, seed=1, max_ep_len=VER_EP_LEN), ddrl.ReplayBufferDQN(O, 0)
    st = env.get_state()
    st[10] = torch.arange(n_envs, device="cuda").float() % VER_EP_LEN      # episode length so far: the time limits come env by env
    env.set_state(st)
    _lib.check(lib.ddrl_rollout_begin_discrete(env._h, actor._h, _lib.stream_ptr()))
    actor.enable_versions(min(2048, min(n_envs, VER_EP_LEN) + 2))
    act, flat, every, count = torch.empty(n_envs, device="cuda"), actor.export(), max(1, VER_EP_LEN // k_versions), [0]

    def live():
        if count[0] % every == 0:
            actor._flat_set(flat)          # an install: the same numbers as a new version
        count[0] += 1
        _lib.check(lib.ddrl_rollout_step_discrete(env._h, actor._h, rb._h, 1, 0, 0.97, actor._noise_seed, actor._noise_ctr,
                                                  _lib.dptr(act), None, None, _lib.stream_ptr()))
        actor._noise_ctr += 2 * n_envs

    for _ in range(VER_EP_LEN + 8):            # every env through an episode end: K versions live from here on
        live()
    return idle, live, lambda: actor.version_state(with_slots=True)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


before = smi()
res = {"n_envs": n_envs, "hidden": O.hidden_size, "iters_per_repetition": iters, "repetitions": reps, "warm_up_steps": warm,
       "device": torch.cuda.get_device_name(0), "launches_per_fused_step": 2}
for family in ("ddqn", "sqn"):
    fused, baseline = make(family)
    for fn in (fused, baseline):
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    extra = []
    if n_versions:
        idle, livefn, state = make_versions(family, n_versions)
        extra = [idle, livefn]
        for fn in extra:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
    tf, tb, ti, tl = [], [], [], []
    for _ in range(reps):
        tf.append(window(fused))
        tb.append(window(baseline))
        if extra:
            ti.append(window(idle))
            tl.append(window(livefn))
    res[family] = {"fused_us_per_step": [round(t, 2) for t in tf], "baseline_us_per_step": [round(t, 2) for t in tb],
                   "slowest_fused_faster_than_fastest_baseline": max(tf) < min(tb)}
    if extra:
        slots, vs = state()
        res[family].update({"store_idle_us_per_step": [round(t, 2) for t in ti], "versions_live_us_per_step": [round(t, 2) for t in tl],
                            "versions_asked": n_versions, "versions_max_ep_len": VER_EP_LEN, "steps_per_install": max(1, VER_EP_LEN // n_versions),
                            "versions_live_now": int(torch.unique(slots).numel()), "row_tiles": vs["tiles"], "out_of_slots": vs["out_of_slots"]})
after = smi()
line = json.dumps(res)
with open(out_path, "a") as f:
    f.write("==== tools/discrete_rollout_probe.py  %s\n%s\n-- device state before\n%s\n-- device state after\n%s\n\n"
            % (time.strftime("%Y-%m-%d %H:%M:%S"), line, before, after))
print(line)
