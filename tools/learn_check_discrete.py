#!/usr/bin/env python3
"""Evidence run, not a test: the discrete device loop — RolloutDeviceDQN (fused discrete rollout step) + TrainDeviceDQN under
ActorLearnerLoop — on the project's own one-body lander behind gym's discrete action table, with the reference's hyper-parameters
(algos/sqn/hyperparams.py via dqn.HyperParameters: alpha 0.1, gamma 0.99, lr 1e-3, polyak 0.995, batch 128, hidden [400, 300],
start_steps 1e4, push_freq 100, a_l_ratio 10).  No tuning, no threshold: the curve is appended to the output file as it comes out.
python tools/learn_check_discrete.py [seconds=280] [sqn|ddqn] [envs=256] [out=profiles/discrete_learning_curve.txt] [updates_per_graph=0]
(updates_per_graph > 0: the learner's loop through ddrl_dqn_loop_run, replayed graphs; 0, the default: the eager path)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import distributed_drl_amd as d  # noqa: E402
from distributed_drl_amd import dqn  # noqa: E402
from distributed_drl_amd.workers import ActorLearnerLoop, RolloutDeviceDQN, TrainDeviceDQN  # noqa: E402

seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 280.0
variant = sys.argv[2] if len(sys.argv) > 2 else "sqn"
n = int(sys.argv[3]) if len(sys.argv) > 3 else 256
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "discrete_learning_curve.txt")
per_graph = int(sys.argv[5]) if len(sys.argv) > 5 else 0

opt = dqn.HyperParameters(obs_dim=8, act_dim=4, env_name="LunarLander-v2", exp_name=variant + "-lander", num_workers=1, a_l_ratio=10)
opt.num_envs, opt.max_ep_len, opt.variant = n, 1000, variant
L = dqn.LearnerSQN if variant == "sqn" else dqn.Learner
ps = d.ParameterServer(*L(opt).get_weights())
rb = d.ReplayBufferDQN(opt, 0, seed=0)
rollout = RolloutDeviceDQN(ps, rb, opt)
trainer = TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0), updates_per_graph=per_graph)
loop = ActorLearnerLoop(rollout, trainer, opt)


def say(line):
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


say("==== tools/learn_check_discrete.py %s: %s, %d envs, a_l_ratio %g, lr %g, alpha %g, batch %d, hidden %s, start_steps %d"
    % (time.strftime("%Y-%m-%d %H:%M"), variant, n, opt.a_l_ratio, opt.lr, opt.alpha, opt.batch_size, opt.hidden_size, opt.start_steps))
t0, win = time.time(), 0
while time.time() - t0 < seconds:
    loop.run(8)
    if time.time() - t0 > (win + 1) * seconds / 14:
        win += 1
        torch.cuda.synchronize()
        ep, ret, ln = rollout.env.stats()
        say("t=%6.1fs  env-steps %9d  updates %8d  episodes %6d  mean return %9.2f  mean len %6.1f  loss %.4g  fused %s"
            % (time.time() - t0, loop.steps, loop.sample_times, ep, ret / max(ep, 1), ln / max(ep, 1), trainer.agent.loss.item(), rollout._fused))
