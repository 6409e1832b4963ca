"""The walker's acting forward at 4096 rows, 24 observations / 4 actions, hidden (400, 300): the wide direct-operand policy
(agent.Actor with opt.wide_policy: k_actor_fwd_wide + k_actor_finish behind one row copy) against the path the walker workers take
without it (Actor.get_actions on an ordinary actor: k_l1 + k_gemm + k_rows_act).

  baseline        get_actions on an ordinary actor, explicit eps
  wide plain      get_actions_versioned on a wide actor, nothing installed: the plain launch (k_actor_fwd_wide<13, 1>)
  wide versioned  the same call with 16 versions live, 256 rows on each (k_version_plan once, then k_actor_fwd_wide<13, 2, versioned>)

One process; after 50 warm-up rounds the three calls alternate for --calls rounds, each between its own pair of HIP events on the current
stream.  Reported: median, 5th and 95th percentile and minimum, in microseconds per call (the device time of the call's launches,
event overhead included, the same for all three).

    python tools/actor_wide_probe.py [--calls 1000] [--out profiles/actor_wide_time.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, VERSIONS, HORIZON = 4096, 16, 1 << 30


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=1000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Actor, HyperParameters
    arch = _lib.require_gpu()

    def actor(wide):
        opt = HyperParameters(obs_dim=24, act_dim=4)
        opt.wide_policy = wide
        return Actor(opt, max_rows=ROWS)
    base, plain, ver = actor(False), actor(True), actor(True)
    plain.enable_versions(2)          # the store enabled and nothing installed: every call is the plain launch
    ver.enable_versions(VERSIONS + 2)
    rs = np.random.RandomState(0)
    keys, vals = ver.get_weights()
    for v in range(1, VERSIONS):      # version v is adopted by rows [256 v, 256 v + 256): 16 live versions, 256 rows each
        ver.set_weights(keys, [w + (0.01 * rs.standard_normal(w.shape)).astype(np.float32) for w in vals])
        m = torch.zeros(ROWS, dtype=torch.uint8)
        m[256 * v:256 * (v + 1)] = 1
        ver.adopt_where_ended(m)
    obs, eps = torch.randn(ROWS, 24, device="cuda"), torch.randn(ROWS, 4, device="cuda")
    out = torch.empty(ROWS, 4, device="cuda")
    calls = (("baseline        get_actions, ordinary actor", lambda: base.get_actions(obs, eps=eps, out=out)),
             ("wide plain      get_actions_versioned", lambda: plain.get_actions_versioned(obs, HORIZON, eps=eps, out=out)),
             ("wide versioned  get_actions_versioned, %d versions live" % VERSIONS, lambda: ver.get_actions_versioned(obs, HORIZON, eps=eps, out=out)))
    for _ in range(50):
        for _, f in calls:
            f()
    slots, st = ver.version_state()
    assert len(set(slots.cpu().tolist())) == VERSIONS and not st["out_of_slots"], st
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for _ in calls]
    for i in range(a.calls):
        for j, (_, f) in enumerate(calls):
            ev[j][i][0].record()
            f()
            ev[j][i][1].record()
    torch.cuda.synchronize()
    lines = ["actor_wide_probe on %s: %d rows, 24 observations / 4 actions, hidden (400, 300); %d alternating calls each behind 50 warm-up rounds, "
             "HIP events around every call" % (arch, ROWS, a.calls)]
    med = []
    for j, (name, _) in enumerate(calls):
        us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[j]])
        med.append(float(np.median(us)))
        lines.append("%-62s median %7.2f us   p5 %7.2f   p95 %7.2f   min %7.2f" % (name, med[-1], np.percentile(us, 5), np.percentile(us, 95), us.min()))
    for j in (1, 2):
        lines.append("%s / baseline = %.2f (%s)" % (calls[j][0].split("  ")[0], med[j] / med[0], "faster" if med[j] < med[0] else "NOT faster"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
