"""Evaluation episodes: the host loop against the one-launch device path (Actor.evaluate, csrc/eval.hip), in one process, on
the same glorot weights and the same env seed.

  host    Actor.test on env.LunarLander: time.perf_counter around the call (one get_action launch + one env step launch + four
          blocking reads per env step)
  device  ddrl_policy_eval: HIP events around the launch, one warm-up call, median of five

Two cases: 25 episodes at max_ep_len = 1000 (a random policy's episodes end early, on a crash), and 25 episodes at a max_ep_len
small enough that most episodes run into the limit (--short-len, default 60: every workgroup then plays the same number of steps).
Prints both times, the env steps played, microseconds per env step for each path, and the kernel's register / LDS / scratch use as
the code object inside libddrl_hip.so records it.

    python tools/eval_probe.py [--out profiles/eval_on_device.txt]

--discrete: the DQN / SQN counterpart (dqn.Actor.evaluate, csrc/eval_q.hip).  Host loop = dqn.Actor.test on env.LunarLanderDiscrete,
one launch = ddrl_dqn_eval; both between HIP events in the same process, one warm-up and five repetitions each, every repetition
listed with its env steps and microseconds per env step.  10 episodes at hidden (400, 300), max_ep_len 1000 and --short-len.  The two
paths draw their coin flips from different generators (a host RandomState against the device's counter stream), so they play
different steps of the same episodes: the comparison is per env step.

    python tools/eval_probe.py --discrete [--out profiles/eval_on_device_discrete.txt]"""
import argparse
import ctypes
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_resources(lib_path, pattern="k_eval_episodesINS_3EnvE"):   # the one-body instantiations (Env3: tools/eval3_probe.py)
    """[(kernel name, vgprs, sgprs, LDS bytes, scratch bytes, vgpr spills)] from the gfx950 code objects bundled in the library."""
    llvm = "/opt/rocm/llvm/bin"
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = shutil.copy(lib_path, tmp)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", lib], cwd=tmp, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp, f)], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                if pattern not in name:
                    continue
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
                out.append((name, g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"), g("vgpr_spill_count")))
    return out


def discrete(a, say):
    """The --discrete arm (module docstring)."""
    import numpy as np
    import torch
    from distributed_drl_amd import _lib, dqn, env

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    arch = _lib.require_gpu()
    lib = _lib.load()
    n = a.episodes if a.episodes != 25 else 10
    say("eval_probe --discrete: Double-DQN, %d episodes, env seed %d, glorot weights (seed 0), hidden (400, 300), greedy_prob 0.97, %s" % (n, a.seed, arch))
    ok = True
    for max_ep_len in (1000, a.short_len):
        class Opt:
            obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [400, 300], 0.99, 1e-3, 0.995, 1, 0, 0.1
        Opt.max_ep_len = max_ep_len
        actor = dqn.Actor(Opt, "test", max_rows=1)
        host = []      # (ms, env steps) of the warm-up and the five repetitions

        class Counting(env.LunarLanderDiscrete):
            steps = 0

            def step(self, act):
                Counting.steps += 1
                return super().step(act)
        for _ in range(6):
            actor._rs = np.random.RandomState(0)
            e, Counting.steps = Counting(a.seed, max_ep_len), 0
            torch.cuda.synchronize()
            ms, _ = timed(lambda: actor.test(e, n))
            host.append((ms, Counting.steps))
        flat = actor.export()
        ret = torch.empty(n, dtype=torch.float64, device="cuda")
        ln = torch.empty(n, dtype=torch.int32, device="cuda")
        dev = []
        for _ in range(6):
            ms, _ = timed(lambda: _lib.check(lib.ddrl_dqn_eval(ctypes.byref(actor.cfg), _lib.dptr(flat), n, a.seed, 0, max_ep_len, _lib.DDRL_ACT_SAMPLE,
                                                               0.97, actor._noise_seed, 0, _lib.dptr(ret), _lib.dptr(ln), None, _lib.stream_ptr())))
            dev.append((ms, int(ln.sum().item())))
        longest, at_limit = int(ln.max().item()), int((ln == max_ep_len).sum().item())
        say("max_ep_len %d: %d episodes" % (max_ep_len, n))
        per = {}
        for name, runs in (("host loop ", host), ("one launch", dev)):
            per[name] = [ms * 1e3 / st for ms, st in runs[1:]]
            say("  %s  warm-up %.3f ms (%d env steps); five repetitions: %s" % (name, runs[0][0], runs[0][1], "; ".join("%.3f ms / %d steps = %.2f us / env step" % (ms, st, ms * 1e3 / st) for ms, st in runs[1:])))
        say("  one launch: longest episode %d steps, %d of %d at the limit, %.2f us / step of the longest episode (median run)"
            % (longest, at_limit, n, statistics.median(ms for ms, _ in dev[1:]) * 1e3 / longest))
        slowest_dev, fastest_host = max(per["one launch"]), min(per["host loop "])
        ok = ok and slowest_dev < fastest_host
        say("  per env step: host / device = %.1f x (medians); slowest device repetition %.2f us, fastest host repetition %.2f us: %s"
            % (statistics.median(per["host loop "]) / statistics.median(per["one launch"]), slowest_dev, fastest_host,
               "every device repetition is faster than every host repetition" if slowest_dev < fastest_host else "CRITERION MISSED"))
    for name, vg, sg, lds, scratch, spill in kernel_resources(_lib.LIB_PATH, "k_eval_episodes_qINS_3EnvE"):
        say("code object: %s  vgprs %d  sgprs %d  LDS %d B  scratch %d B  vgpr spills %d" % (name, vg, sg, lds, scratch, spill))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--short-len", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--discrete", action="store_true")
    a = ap.parse_args()
    if a.discrete:
        lines = []

        def say(s):
            print(s, flush=True)
            lines.append(s)
        ok = discrete(a, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(0 if ok else 1)
    import torch
    from distributed_drl_amd import _lib, env
    from distributed_drl_amd.agent import Actor, HyperParameters

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    arch = _lib.require_gpu()
    lib = _lib.load()
    say("eval_probe: %d episodes, env seed %d, glorot weights (seed 0), hidden (400, 300), %s" % (a.episodes, a.seed, arch))
    for max_ep_len, what in ((1000, "random policy, episodes end on a crash"), (a.short_len, "limit short enough that most episodes hit it")):
        opt = HyperParameters()
        opt.max_ep_len, opt.summary_dir = max_ep_len, None
        actor = Actor(opt, max_rows=1)
        n = a.episodes
        host_env = env.LunarLander(a.seed, max_ep_len)
        actor.get_action(host_env._vec.obs[0].cpu().numpy(), True)       # warm-up of the launch path (does not step the env)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_mean = actor.test(host_env, None, n)
        t_host = time.perf_counter() - t0
        out = actor.evaluate(n, a.seed, 0, max_ep_len)                    # warm-up call; also the step count
        steps = int(out["len"].sum())
        flat = actor.get_weights_flat()
        ret = torch.empty(n, dtype=torch.float64, device="cuda")
        ln = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.ddrl_policy_eval(ctypes.byref(actor.cfg), _lib.dptr(flat), n, a.seed, 0, max_ep_len, _lib.dptr(ret), _lib.dptr(ln),
                                            None, _lib.stream_ptr()))
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t_dev = statistics.median(ms) * 1e-3
        longest = int(out["len"].max())
        say("max_ep_len %d (%s): %d env steps in %d episodes, longest %d, %d at the limit" % (max_ep_len, what, steps, n, longest, int((out["len"] == max_ep_len).sum())))
        say("  host loop   %10.3f ms   %8.2f us / env step   (mean return %.6f)" % (t_host * 1e3, t_host * 1e6 / steps, host_mean))
        say("  one launch  %10.3f ms   %8.2f us / env step   %8.2f us / step of the longest episode   (five runs: %s ms; mean return %.6f)"
            % (t_dev * 1e3, t_dev * 1e6 / steps, t_dev * 1e6 / longest, " ".join("%.3f" % m for m in ms), float(out["ret"].mean())))
        say("  host / device = %.1f x; returns %s" % (t_host / t_dev, "equal" if host_mean == sum(float(x) for x in out["ret"]) / n else "DIFFER"))
    for name, vg, sg, lds, scratch, spill in kernel_resources(_lib.LIB_PATH):
        say("code object: %s  vgprs %d  sgprs %d  LDS %d B  scratch %d B  vgpr spills %d" % (name, vg, sg, lds, scratch, spill))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
