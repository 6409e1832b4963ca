"""CPU: the host-side pieces FreeRunningLoop rests on for the discrete and the n-step workers — RolloutDeviceNStep._step_once looks at
the server only where `auto_pull` is set (a scripted worker: fake env, queues, ring and server; no device), the worker-side interface
the loop asks for exists on all three workers, and the loop's export and docstring are intact."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")


class _Env:
    model, n = "simple", 2

    def __init__(self):
        self.obs = torch.zeros(2, 8)

    def sample_actions(self, out):
        out.fill_(0.5)

    def step_wrapped(self, act, *a):
        z = torch.zeros(2)
        return torch.ones(2, 8), z, z, torch.ones(2, 8), z.to(torch.uint8)


class _Queues:
    arrays = [torch.zeros(2, 4, 8), torch.zeros(2, 3, 2), torch.zeros(2, 3), torch.zeros(2, 3)]

    def __init__(self):
        self.begun = 0

    def push(self, *a):
        return torch.ones(2, dtype=torch.uint8)

    def begin(self, obs, mask=None):
        self.begun += 1


class _Ring:
    def __init__(self):
        self.stored = 0

    def store_masked(self, *a):
        self.stored += 1


def _scripted_worker(versions, auto_pull):
    """A RolloutDeviceNStep in its random-action phase, every collaborator scripted; pull() counts its calls."""
    from distributed_drl_amd.workers import RolloutDeviceNStep
    w = object.__new__(RolloutDeviceNStep)
    w.opt = types.SimpleNamespace(start_steps=10 ** 9, weights_file="")
    w.env, w.winq, w.rbs = _Env(), _Queues(), [_Ring()]
    w.o, w.act = torch.zeros(2, 8), torch.zeros(2, 2)
    w.filling_steps, w.limit_steps, w._fused_live, w._learning = 0, 12, False, True
    w._versions, w.auto_pull = versions, auto_pull
    w.pick = np.random.RandomState(0)
    w.actor = types.SimpleNamespace(adopt_where_ended=lambda ended: None)
    w.pulls = 0

    def pull():
        w.pulls += 1
    w.pull = pull
    return w


@pytest.mark.parametrize("versions", [True, False])
def test_nstep_step_once_consults_auto_pull(versions):
    """Both call sites — in front of the step with a version store, behind it without — pull only where auto_pull is set; the default
    (True) is the behaviour outside the loop."""
    w = _scripted_worker(versions, True)
    w._step_once()
    w._step_once()
    assert w.pulls == 2 and w.rbs[0].stored == 2 and w.winq.begun == 2 and w.filling_steps == 2
    w = _scripted_worker(versions, False)
    w._step_once()
    w._step_once()
    assert w.pulls == 0 and w.rbs[0].stored == 2 and w.winq.begun == 2    # the step itself is the same


def test_auto_pull_defaults_to_true_and_every_pull_in_the_workers_steps_is_guarded():
    import inspect
    from distributed_drl_amd import workers
    assert "self.auto_pull = True" in inspect.getsource(workers._RolloutWorker._start)
    for fn in (workers.RolloutDeviceNStep._step_once, workers._RolloutWorker.step):
        lines = inspect.getsource(fn).split("\n")
        calls = [i for i, ln in enumerate(lines) if "self.pull()" in ln]
        assert len(calls) >= 2, fn.__qualname__
        for i in calls:
            assert "self.auto_pull" in lines[i - 1] and lines[i - 1].strip().startswith("if "), (fn.__qualname__, lines[i - 1])


def test_the_loops_worker_interface_and_exports():
    import distributed_drl_amd as d
    from distributed_drl_amd import _exports, workers
    from distributed_drl_amd.replay import _Ring as RingBase, ReplayBuffer, ReplayBufferDQN, ReplayBufferNStep, ReplayBufferSAC1
    assert _exports._TABLE["FreeRunningLoop"] == "workers" and d.FreeRunningLoop is workers.FreeRunningLoop
    for name in ("RolloutDevice", "RolloutDeviceDQN", "RolloutDeviceNStep", "TrainDevice", "TrainDeviceDQN", "ActorLearnerLoop"):
        assert _exports._TABLE[name] == "workers" and getattr(d, name) is getattr(workers, name)
    doc = workers.FreeRunningLoop.__doc__
    for words in ("example/dsac.py:229-236", "STAGING rings", "RolloutDeviceDQN", "RolloutDeviceNStep", "append_from", "store_batch",
                  "node_buffer", "_learning", "ValueError"):
        assert words in doc, words
    for cls in (workers.RolloutDevice, workers.RolloutDeviceDQN, workers.RolloutDeviceNStep):
        for m in ("_free_target", "_free_staging", "_free_store_into"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert workers.RolloutDeviceNStep._free_append is True
    assert workers.RolloutDevice._free_append is False and workers.RolloutDeviceDQN._free_append is False
    for cls in (ReplayBuffer, ReplayBufferSAC1, ReplayBufferDQN, ReplayBufferNStep):     # available on every ring class
        assert cls.append_from is RingBase.append_from
    import inspect
    assert list(inspect.signature(workers.FreeRunningLoop.__init__).parameters) == [
        "self", "rollout", "trainer", "opt", "steps_per_segment", "updates_per_segment", "timing", "streams"]
