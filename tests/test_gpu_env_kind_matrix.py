"""Every entry point that takes an env handle, called on a handle of every model kind with otherwise-good arguments: the status and the
WHOLE ddrl_last_error() text of each (entry point, kind) pair against tests/golden/env_kind_matrix.json.

The fixture was recorded by this very script (`python tests/test_gpu_env_kind_matrix.py OUT.json`) on the build of the commit BEFORE
the env family got its model table (csrc/env.hip then still held the one-body kernels and the guard macros): it pins that the one guard
function behind the table answers what the three macros and the hand-written walker guard answered, byte for byte.  It holds statuses
and strings only.  Where the call is taken (status 0) the text is not recorded; a DDRL_REQUIRE text starts with the `file:line: ` of its
source line, which names no behaviour and is cut from both sides (one pair: ddrl_env_rollout_mirrors on a one-body handle, which no
begin call can precede).

One handle per kind: 32 envs, max_ep_len 8, 4 velocity / 2 position iterations.  The entries run in ENTRIES' order on every handle, so a
begin call stands in front of its step call and ddrl_env_rollout_mirrors behind the articulated discrete begin.  A refusal by kind
returns before any launch."""
import ctypes
import json
import os
import re
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_kind_matrix.json")
N, CAP, LN = 32, 256, 4
KINDS = ("one_body", "articulated", "walker")
ENTRIES = (
    "ddrl_env_step_wrapped", "ddrl_env_step_wrapped_articulated", "ddrl_env_step_wrapped_walker", "ddrl_env_step_discrete",
    "ddrl_rollout_begin", "ddrl_rollout_step", "ddrl_rollout_begin_articulated", "ddrl_rollout_step_articulated",
    "ddrl_rollout_begin_discrete", "ddrl_rollout_step_discrete", "ddrl_rollout_begin_discrete_articulated",
    "ddrl_rollout_step_discrete_articulated", "ddrl_env_rollout_mirrors",
    "ddrl_rollout_begin_nstep", "ddrl_rollout_step_nstep", "ddrl_rollout_begin_nstep_articulated", "ddrl_rollout_step_nstep_articulated",
    "ddrl_env_eval_policy", "ddrl_env_eval_q",
)
SOURCE_LINE = re.compile(r"^[\w./]+\.(hip|h):\d+: ")


class _QOpt:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 64], 0.99, 1e-3, 0.995, 64, 5, 0.1


def run_matrix():
    """{entry: {kind: [status, text]}} of the library the package loads."""
    import torch
    import distributed_drl_amd as ddrl
    from distributed_drl_amd import _lib, dqn
    from distributed_drl_amd.agent import Actor, HyperParameters
    from distributed_drl_amd.env import VecBipedalWalker, VecLunarLander
    from distributed_drl_amd.replay import ReplayBuffer
    from distributed_drl_amd.workers import WindowQueue

    class Ring1D(ReplayBuffer):
        _acts_1d = True

    _lib.require_gpu()
    lib, sp = _lib.load(), _lib.stream_ptr()
    opt = HyperParameters()
    opt.hidden_sizes, opt.num_envs, opt.seed, opt.max_ep_len = (64, 64), N, 5, 8
    opt.Ln, opt.save_freq, opt.buffer_size, opt.num_buffers = LN, 1, CAP, 1
    it = dict(velocity_iterations=4, position_iterations=2)
    envs = {"one_body": VecLunarLander(N, seed=7, max_ep_len=8),
            "articulated": VecLunarLander(N, seed=7, max_ep_len=8, model="articulated", **it),
            "walker": VecBipedalWalker(N, seed=7, max_ep_len=8, **it)}
    z = lambda *s: torch.zeros(*s, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    act, idx, obs2, nxt, rew, done = z(N, 4), z(N), z(N, 24), z(N, 24), z(N), z(N)
    ended = torch.zeros(N, dtype=torch.uint8, device="cuda")
    q_out = z(N, 4)
    out = {e: {} for e in ENTRIES}
    for kind in KINDS:
        h = envs[kind]._h
        pi = {f: Actor(opt, max_rows=N) for f in ("", "_nstep", "eval")}       # an actor per family: each holds its own observation rows
        q = {f: dqn.Actor(_QOpt, "worker", max_rows=N) for f in ("", "eval")}
        ring, ring1, win = ddrl.ReplayBufferSAC1(8, 2, CAP, seed=0), Ring1D(8, 1, CAP), ddrl.ReplayBufferNStep(opt)
        winq = WindowQueue(N, LN, 8, 2)
        nout = _lib.RolloutNStepOut(act=P(act), next_obs=P(nxt))
        wrapped = (P(act), 0.0, 0.0, 1.0, 3, 8, P(obs2), P(rew), P(done), P(nxt), P(ended), sp)
        pi_step = (ring._h, 1, 3, 0, 0, P(act), P(nxt), sp)
        n_step = (winq._h, win._h, 1, 0.0, 0.0, 1.0, 3, 8, 0, 3, 0, ctypes.byref(nout), sp)
        none = ctypes.POINTER(ctypes.c_void_p)()
        args = {
            "ddrl_env_step_wrapped": wrapped, "ddrl_env_step_wrapped_articulated": wrapped, "ddrl_env_step_wrapped_walker": wrapped,
            "ddrl_env_step_discrete": (P(idx), P(obs2), P(rew), P(done), P(nxt), P(ended), sp),
            "ddrl_rollout_begin": (pi[""]._h, sp), "ddrl_rollout_step": (pi[""]._h,) + pi_step,
            "ddrl_rollout_begin_articulated": (pi[""]._h, sp), "ddrl_rollout_step_articulated": (pi[""]._h,) + pi_step,
            "ddrl_rollout_begin_discrete": (q[""]._h, sp),
            "ddrl_rollout_step_discrete": (q[""]._h, ring1._h, 1, _lib.DDRL_ACT_SAMPLE, 0.5, 3, 0, P(idx), P(q_out), P(nxt), sp),
            "ddrl_rollout_begin_discrete_articulated": (q[""]._h, sp),
            "ddrl_rollout_step_discrete_articulated": (q[""]._h, ring1._h, 1, _lib.DDRL_ACT_SAMPLE, 0.5, 3, 0, sp),
            "ddrl_env_rollout_mirrors": (none, none, none, ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int32)()),
            "ddrl_rollout_begin_nstep": (pi["_nstep"]._h, winq._h, sp), "ddrl_rollout_step_nstep": (pi["_nstep"]._h,) + n_step,
            "ddrl_rollout_begin_nstep_articulated": (pi["_nstep"]._h, winq._h, sp),
            "ddrl_rollout_step_nstep_articulated": (pi["_nstep"]._h,) + n_step,
            "ddrl_env_eval_policy": (pi["eval"]._h, 1, 0, 0, sp),
            "ddrl_env_eval_q": (q["eval"]._h, 1, 0, _lib.DDRL_ACT_SAMPLE, 0.5, 3, 0, 0, sp),
        }
        for entry in ENTRIES:
            rc = int(getattr(lib, entry)(h, *args[entry]))
            out[entry][kind] = [rc, "" if rc == 0 else SOURCE_LINE.sub("", lib.ddrl_last_error().decode())]
        torch.cuda.synchronize()
    return out


def test_every_entry_point_answers_every_kind_as_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)["matrix"]
    got = run_matrix()
    assert set(want) == set(ENTRIES) and all(set(want[e]) == set(KINDS) for e in ENTRIES)
    for entry in ENTRIES:
        for kind in KINDS:
            print(entry, kind, got[entry][kind])
            assert got[entry][kind] == want[entry][kind], (entry, kind)
    # the matrix is not empty of either answer: every entry point is taken by at least one kind, and every kind is refused somewhere
    assert all(any(want[e][k][0] == 0 for k in KINDS) for e in ENTRIES)
    assert all(any(want[e][k][0] != 0 for e in ENTRIES) for k in KINDS)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    doc = {"recorded_on": "the parent commit's build (csrc/env.hip with the one-body kernels and the guard macros), by "
                          "tests/test_gpu_env_kind_matrix.py run as a script; statuses and ddrl_last_error() texts only",
           "matrix": run_matrix()}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, ensure_ascii=False, sort_keys=True)
        f.write("\n")
