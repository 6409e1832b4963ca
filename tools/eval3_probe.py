"""Evaluation episodes on the ARTICULATED lander: the one-launch device path fed from handles (ddrl_env_eval_policy / ddrl_env_eval_q,
csrc/eval3.hip) against the host loop it replaces, at hidden (400, 300) and gym's 180 velocity / 60 position iterations, on the same
glorot weights and the same env seed, for the continuous policy (agent.Actor), Double-DQN (dqn.Actor) and SQN (dqn.ActorSQN).

  device  the C call between HIP events (the pack launch of the weights and the episodes' launch), n = 25 episodes at
          max_ep_len = 1000: one warm-up call, then five; the median, every run, the env steps played, the longest episode
  host    Actor.test on env.LunarLander(model="articulated") / dqn.Actor.test on env.LunarLanderDiscrete(model="articulated"),
          2 episodes: time.perf_counter around the call (every env step synchronises), one warm-up run, then five on fresh envs of the
          same seed; reported PER ENV STEP — the 25-episode host round is that figure times the device call's env steps

The DQN host loop draws its coin flips from a host RandomState and the device from its counter stream, so the two play different steps
of the same episodes: the comparison is per env step, as in tools/eval_probe.py --discrete.

Every measurement is a child process of its own under its own `timeout` (this process never opens the GPU); after a child that fails
or runs into its limit nothing more is started.

    python tools/eval3_probe.py [--out profiles/eval_on_device_articulated.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AGENTS = ("policy", "ddqn", "sqn")
STEP_LIMIT_S = 300      # of one child; the longest (a device step: 6 calls of up to 1000 serial env steps of ~0.3 ms) needs a few seconds
MODEL = dict(model="articulated", velocity_iterations=180, position_iterations=60)


def _agent(kind, max_ep_len):
    if kind == "policy":
        from distributed_drl_amd.agent import Actor, HyperParameters
        opt = HyperParameters()
        opt.max_ep_len, opt.summary_dir = max_ep_len, None
        return Actor(opt, max_rows=1)
    from distributed_drl_amd import dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [400, 300], 0.99, 1e-3, 0.995, 1, 0, 0.1
    Opt.max_ep_len = max_ep_len
    return (dqn.Actor if kind == "ddqn" else dqn.ActorSQN)(Opt, "test", max_rows=1)


def device_step(kind, a):
    import torch
    from distributed_drl_amd import _lib, env
    arch = _lib.require_gpu()
    lib = _lib.load()
    n, L = a.episodes, a.max_ep_len
    actor = _agent(kind, L)
    marker = env.make_device("LunarLanderContinuous-v2" if kind == "policy" else "LunarLander-v2", seed=a.seed, max_ep_len=L, **MODEL)
    vec = marker.handle()
    if kind == "policy":
        call = lambda: lib.ddrl_env_eval_policy(vec._h, actor._h, n, 0, 0, _lib.stream_ptr())
    else:
        mode = _lib.DDRL_ACT_DETERMINISTIC if kind == "sqn" else _lib.DDRL_ACT_SAMPLE      # what the class's test action does
        call = lambda: lib.ddrl_env_eval_q(vec._h, actor._h, n, 0, mode, 0.97, actor._noise_seed, 0, 0, _lib.stream_ptr())
    ms = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(call())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out = env.eval_results(vec, 12 if kind == "policy" else 20)
    steps, longest = int(out["len"].sum()), int(out["len"].max())
    med = statistics.median(ms[1:])
    print("%s device (%s): %d episodes, max_ep_len %d: %d env steps, longest episode %d, %d at the limit, mean return %.6f"
          % (kind, arch, n, L, steps, longest, int((out["len"] == L).sum()), float(out["ret"].mean())))
    print("%s device: warm-up %.3f ms; five runs %s ms; median %.3f ms = %.2f us / env step = %.2f us / step of the longest episode"
          % (kind, ms[0], " ".join("%.3f" % m for m in ms[1:]), med, med * 1e3 / steps, med * 1e3 / longest))
    print("RESULT %s device_ms %.6f steps %d" % (kind, med, steps))


def host_step(kind, a):
    import numpy as np
    import torch
    from distributed_drl_amd import _lib, env
    _lib.require_gpu()
    n, L = a.host_episodes, a.max_ep_len
    actor = _agent(kind, L)
    base = env.LunarLander if kind == "policy" else env.LunarLanderDiscrete

    class Counting(base):
        steps = 0

        def step(self, act):
            Counting.steps += 1
            return super().step(act)
    runs = []
    for _ in range(6):
        if kind != "policy":
            actor._rs = np.random.RandomState(0)
        e, Counting.steps = Counting(a.seed, L, **MODEL), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        actor.test(e, None, n) if kind == "policy" else actor.test(e, n)
        runs.append(((time.perf_counter() - t0) * 1e3, Counting.steps))
    per = [ms * 1e3 / st for ms, st in runs[1:]]
    print("%s host loop: %d episodes, max_ep_len %d; warm-up %.3f ms (%d env steps); five runs: %s"
          % (kind, n, L, runs[0][0], runs[0][1], "; ".join("%.3f ms / %d steps = %.2f us / env step" % (ms, st, ms * 1e3 / st) for ms, st in runs[1:])))
    print("RESULT %s host_us_per_step %.6f" % (kind, statistics.median(per)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=25)
    ap.add_argument("--host-episodes", type=int, default=2)
    ap.add_argument("--max-ep-len", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: run ONE measurement in this process (<agent>:device | <agent>:host)")
    a = ap.parse_args()
    if a.step:
        kind, which = a.step.split(":")
        (device_step if which == "device" else host_step)(kind, a)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("eval3_probe: articulated lander, 180 velocity / 60 position iterations, hidden (400, 300), glorot weights (seed 0), env seed %d" % a.seed)
    res, ok = {}, True
    for kind in AGENTS:
        for which in ("device", "host"):
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (kind, which),
                   "--episodes", str(a.episodes), "--host-episodes", str(a.host_episodes), "--max-ep-len", str(a.max_ep_len), "--seed", str(a.seed)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            for s in p.stdout.splitlines():
                if s.startswith("RESULT "):
                    f = s.split()
                    res[(f[1], f[2])] = float(f[3])
                    if len(f) > 5:
                        res[(f[1], f[4])] = float(f[5])
                else:
                    say(s)
            if p.returncode != 0:
                say("step %s:%s ended with status %d — nothing more is started\n%s" % (kind, which, p.returncode, p.stderr[-2000:]))
                ok = False
                break
        if not ok:
            break
        dev_ms, steps, host_us = res[(kind, "device_ms")], res[(kind, "steps")], res[(kind, "host_us_per_step")]
        host_round_ms = host_us * steps * 1e-3
        say("%s: the %d-episode round: one launch %.3f ms; the host loop at its %.2f us / env step over the same %d env steps %.3f ms: "
            "host / device = %.1f x per round (%s)" % (kind, a.episodes, dev_ms, host_us, steps, host_round_ms, host_round_ms / dev_ms,
                                                         "the device call is faster" if dev_ms < host_round_ms else "the device call is NOT faster"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
