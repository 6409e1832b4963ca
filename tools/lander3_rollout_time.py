"""Time RolloutDevice.step() on the ARTICULATED lander, fused (opt.fused_rollout_articulated: ddrl_rollout_step_articulated, two
launches per vector step) beside unfused (o.copy_, get_actions, env.step, store_batch: the path the worker takes without the flag,
untouched by the fused step's existence), in this process by the same HIP-event loop: per figure the envs are first stepped
`--warmup` times, then five runs of `--steps` back-to-back vector steps; the median run and the spread (min .. max) in microseconds
per vector step, host time between the launches included (it is part of what the fused step saves).

    python tools/lander3_rollout_time.py [--envs 4096] [--steps 50] [--warmup 100] [--discrete]

--discrete: RolloutDeviceDQN.step() instead — Double-DQN and SQN actors (hidden 400 / 300, opt.adopt = "episode"), fused
(opt.fused_discrete_rollout_articulated: ddrl_rollout_step_discrete_articulated) beside the worker without the flag, the same settings
and the same loop, plus a third arm: the fused worker with opt.adopt = "step" (no version store: every env swaps to a push at the next
step, as the unfused worker does), which separates what the fusion saves from what exact per-env adoption costs
(profiles/lander3_discrete_rollout_time.txt holds a recorded run).

Per iteration count (gym's 180 / 60 and 8 / 3) two settings:
  one version     max_ep_len 1000, nothing pushed: the fused worker's version store holds one version (the plain forward)
  ~17 versions    max_ep_len 32 with the time limits staggered env by env and a push every other step: the fused worker adopts per
                  env at that env's episode end and holds about 17 live versions; the unfused worker cannot hold versions — it swaps
                  all envs to each push at its next step — so its figure here and its one-version figure are what the fused
                  17-version figure is to be compared with.  (Every wave has envs at their reset in every step here, and a reset is a
                  second solve: both paths pay it.)
Prints one line per setting (profiles/lander3_rollout_time.txt holds a recorded run).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 32   # ~17 versions: a push every other step, every env ends an episode within LIMIT steps


def make(n, vit, pit, fused, max_ep_len):
    import torch
    import distributed_drl_amd as ddrl
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import RolloutDevice
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed = n, -1, max_ep_len, 1
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", vit, pit
    opt.fused_rollout_articulated = fused
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferSAC1(8, 2, 1 << 20, seed=0)
    roll = RolloutDevice(ps, rb, opt)
    assert roll._fused_ready() is fused and roll._versions is fused
    if max_ep_len == LIMIT:
        st = roll.env.get_state()
        st[10] = torch.arange(n, device="cuda").float() % LIMIT   # episode length so far: the time limits come env by env
        roll.env.set_state(st)
    return roll, ps, keys, vals


def make_discrete(n, vit, pit, fused, max_ep_len, family, adopt="episode"):
    import torch
    import distributed_drl_amd as ddrl
    from distributed_drl_amd import dqn
    from distributed_drl_amd.workers import RolloutDeviceDQN

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, alpha = 8, 4, [400, 300], 0.99, 1e-3, 0.995, n, 0.1
        num_envs, start_steps, seed, variant, buffer_size = n, -1, 1, family, 1 << 20
    opt = Opt()
    opt.adopt = adopt
    opt.max_ep_len = max_ep_len
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", vit, pit
    opt.fused_discrete_rollout_articulated = fused
    keys, vals = (dqn.LearnerSQN if family == "sqn" else dqn.Learner)(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferDQN(opt, 0, seed=0)
    roll = RolloutDeviceDQN(ps, rb, opt)
    assert roll._fused_ready() is fused and roll._versions is (fused and adopt == "episode")
    if max_ep_len == LIMIT:
        st = roll.env.get_state()
        st[10] = torch.arange(n, device="cuda").float() % LIMIT   # episode length so far: the time limits come env by env
        roll.env.set_state(st)
    return roll, ps, keys, vals


def time_worker(roll, ps, keys, vals, steps, warmup, push_every, runs=5):
    import torch
    t = 0

    def go(k):
        nonlocal t
        for _ in range(k):
            roll.step()
            t += 1
            if push_every and t % push_every == 0:
                ps.push(keys, vals)   # an install: the same numbers as a new version
    go(warmup)
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go(steps)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / steps)
    live = 1
    if roll._versions:
        slots, st = roll.actor.version_state()
        assert not st["out_of_slots"]
        live = int(torch.unique(slots).numel())
    return "%.1f us (%.1f .. %.1f)" % (statistics.median(out), min(out), max(out)), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--discrete", action="store_true", help="time RolloutDeviceDQN.step() (Double-DQN and SQN) instead of RolloutDevice.step()")
    args = ap.parse_args()
    workers = [("RolloutDeviceDQN.step() %s" % f, lambda *a, f=f, **kw: make_discrete(*a, f, **kw)) for f in ("ddqn", "sqn")] if args.discrete else [("RolloutDevice.step()", make)]
    arms = [("fused", True, {}), ("unfused", False, {})]
    if args.discrete:
        arms.insert(1, ("fused with adopt='step'", True, dict(adopt="step")))
    for what, build in workers:
        for vit, pit in ((180, 60), (8, 3)):
            for name, limit, every in (("one version", 1000, 0), ("~17 versions", LIMIT, 2)):
                parts = []
                for arm, fused, kw in arms:
                    fig, live = time_worker(*build(args.envs, vit, pit, fused, limit, **kw), args.steps, args.warmup, every)
                    parts.append("%s %s, %d version%s live at the end" % (arm, fig, live, "" if live == 1 else "s"))
                print("%s, articulated %d/%d, %d envs, %s (max_ep_len %d, %s), us per vector step, median of 5 runs of %d "
                      "steps (min .. max): %s" % (what, vit, pit, args.envs, name, limit, "a push every %d steps" % every if every else "no push",
                                                  args.steps, "; ".join(parts)), flush=True)


if __name__ == "__main__":
    main()
