"""Evaluation episodes: the host loop against the one-launch device path (Actor.evaluate, csrc/eval.hip), in one process, on
the same glorot weights and the same env seed.

  host    Actor.test on env.LunarLander: time.perf_counter around the call (one get_action launch + one env step launch + four
          blocking reads per env step)
  device  ddrl_policy_eval: HIP events around the launch, one warm-up call, median of five

Two cases: 25 episodes at max_ep_len = 1000 (a random policy's episodes end early, on a crash), and 25 episodes at a max_ep_len
small enough that most episodes run into the limit (--short-len, default 60: every workgroup then plays the same number of steps).
Prints both times, the env steps played, microseconds per env step for each path, and the kernel's register / LDS / scratch use as
the code object inside libddrl_hip.so records it.

    python tools/eval_probe.py [--out profiles/eval_on_device.txt]"""
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


def kernel_resources(lib_path, pattern="k_eval_episodes"):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--short-len", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
