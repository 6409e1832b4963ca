"""Evaluation episodes on the WALKER: the one-launch device path fed from handles (ddrl_env_eval_policy_walker, csrc/walker_eval.hip)
against the host loop it replaces, at hidden (400, 300) and gym's 180 velocity / 60 position iterations, on the same glorot weights and
the same env seed, for the continuous policy (agent.Actor).  --terrain hardcore: the same two measurements on the Hardcore terrain
(ddrl_env_eval_policy_walker_hardcore, csrc/walker_hardcore_eval.hip; the host loop on env.BipedalWalker(terrain="hardcore")).

  device  the C call between HIP events (the pack launch of the weights and the episodes' launch), n = 25 episodes at
          max_ep_len = 1600: one warm-up call, then five; the median, every run, the env steps played, the longest episode
  host    Actor.test on env.BipedalWalker, 2 episodes of at most --host-max-ep-len = 150 steps (a bounded stretch: a host step costs
          the same at any limit): time.perf_counter around the call (every env step synchronises), one warm-up run, then five on
          fresh envs of the same seed; reported PER ENV STEP — the 25-episode host round is that figure times the device call's env steps

Every measurement is a child process of its own under its own `timeout` (this process never opens the GPU); after a child that fails
or runs into its limit nothing more is started.

    python tools/walker_eval_probe.py [--out profiles/eval_on_device_walker.txt]
    python tools/walker_eval_probe.py --terrain hardcore [--out profiles/eval_on_device_walker_hardcore.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 300      # of one child; the longest (the device step: 6 calls of up to 1600 serial env steps of ~0.8 ms) needs ~10 s
ITERATIONS = dict(velocity_iterations=180, position_iterations=60)


def _agent(max_ep_len):
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters(obs_dim=24, act_dim=4)
    opt.max_ep_len, opt.summary_dir = max_ep_len, None
    return Actor(opt, max_rows=1)


def device_step(a):
    import torch
    from distributed_drl_amd import _lib, env
    arch = _lib.require_gpu()
    lib = _lib.load()
    n, L = a.episodes, a.max_ep_len
    actor = _agent(L)
    marker = env.DeviceBipedalWalkerHardcore if a.terrain == "hardcore" else env.DeviceBipedalWalker
    vec = marker(a.seed, L, **ITERATIONS).handle()
    entry = getattr(lib, getattr(marker, "eval_entry", env.MODELS["walker"]["eval"])[0])
    call = lambda: entry(vec._h, actor._h, n, 0, 0, _lib.stream_ptr())
    ms = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(call())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out = env.eval_results(vec, 32)
    steps, longest = int(out["len"].sum()), int(out["len"].max())
    med = statistics.median(ms[1:])
    print("policy device (%s): %d episodes, max_ep_len %d: %d env steps, longest episode %d, %d at the limit, mean return %.6f"
          % (arch, n, L, steps, longest, int((out["len"] == L).sum()), float(out["ret"].mean())))
    print("policy device: warm-up %.3f ms; five runs %s ms; median %.3f ms = %.2f us / env step = %.2f us / step of the longest episode"
          % (ms[0], " ".join("%.3f" % m for m in ms[1:]), med, med * 1e3 / steps, med * 1e3 / longest))
    print("RESULT policy device_ms %.6f steps %d" % (med, steps))


def host_step(a):
    import torch
    from distributed_drl_amd import _lib, env
    _lib.require_gpu()
    n, L = a.host_episodes, a.host_max_ep_len
    actor = _agent(L)

    class Counting(env.BipedalWalker):
        steps = 0

        def step(self, act):
            Counting.steps += 1
            return super().step(act)
    runs = []
    for _ in range(6):
        e, Counting.steps = Counting(a.seed, L, terrain=a.terrain, **ITERATIONS), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        actor.test(e, None, n)
        runs.append(((time.perf_counter() - t0) * 1e3, Counting.steps))
    per = [ms * 1e3 / st for ms, st in runs[1:]]
    print("policy host loop: %d episodes, max_ep_len %d; warm-up %.3f ms (%d env steps); five runs: %s"
          % (n, L, runs[0][0], runs[0][1], "; ".join("%.3f ms / %d steps = %.2f us / env step" % (ms, st, ms * 1e3 / st) for ms, st in runs[1:])))
    print("RESULT policy host_us_per_step %.6f" % statistics.median(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=25)
    ap.add_argument("--host-episodes", type=int, default=2)
    ap.add_argument("--max-ep-len", type=int, default=1600)
    ap.add_argument("--host-max-ep-len", type=int, default=150)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--terrain", choices=("grass", "hardcore"), default="grass")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: run ONE measurement in this process (device | host)")
    a = ap.parse_args()
    if a.step:
        (device_step if a.step == "device" else host_step)(a)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("walker_eval_probe: bipedal walker%s, 180 velocity / 60 position iterations, hidden (400, 300), glorot weights (seed 0), env seed %d"
        % (" on the hardcore terrain" if a.terrain == "hardcore" else "", a.seed))
    res, ok = {}, True
    for which in ("device", "host"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", which,
               "--episodes", str(a.episodes), "--host-episodes", str(a.host_episodes), "--max-ep-len", str(a.max_ep_len),
               "--host-max-ep-len", str(a.host_max_ep_len), "--seed", str(a.seed), "--terrain", a.terrain]
        p = subprocess.run(cmd, capture_output=True, text=True)
        for s in p.stdout.splitlines():
            if s.startswith("RESULT "):
                f = s.split()
                res[f[2]] = float(f[3])
                if len(f) > 5:
                    res[f[4]] = float(f[5])
            else:
                say(s)
        if p.returncode != 0:
            say("step %s ended with status %d — nothing more is started\n%s" % (which, p.returncode, p.stderr[-2000:]))
            ok = False
            break
    if ok:
        dev_ms, steps, host_us = res["device_ms"], res["steps"], res["host_us_per_step"]
        host_round_ms = host_us * steps * 1e-3
        say("policy: the %d-episode round: one launch %.3f ms; the host loop at its %.2f us / env step over the same %d env steps %.3f ms: "
            "host / device = %.1f x per round (%s)" % (a.episodes, dev_ms, host_us, steps, host_round_ms, host_round_ms / dev_ms,
                                                         "the device call is faster" if dev_ms < host_round_ms else "the device call is NOT faster"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
