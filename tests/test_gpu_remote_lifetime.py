"""GPU: argument lifetime across an actor's stream (distributed-drl_amd/remote.py).  Every actor thread issues its device work on a
non-blocking stream of its own; a CUDA tensor handed to `method.remote(...)` is waited for with an event, and — what this module
holds remote.py to — recorded on the actor's stream, so that the caching allocator does not give its block out again before that
stream has read it.  Without the record a caller that drops its tensors right after `get(store_batch.remote(...))` (the method has
been ENQUEUED, not run) gets the same blocks back for its next allocation and overwrites rows the actor has not stored yet.

The actor is a ReplayBufferSAC1 with a gate: hold() puts a bounded sleep on the actor's stream and records an event behind it,
held() is `not event.query()`.  While the gate holds the stream the caller stores, drops, allocates tensors of the same sizes, fills
them with other values and synchronises its own stream; then the ring is read through the actor.  A run in which the gate is over
before the caller is done proves nothing and fails as void.

Gate: the host time of the sequence (store -> get -> one more message -> del -> allocate and fill -> stream sync) was measured at
5.03 ms on an MI355X (the second test's draw -> store -> drop -> draw again: 0.84 ms); the gate is ten times the larger, 50.3 ms.
Each run prints its own host time."""
import contextlib
import gc
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402

HOST_MS_MEASURED = 5.03
GATE_MS = max(10.0, 10.0 * HOST_MS_MEASURED)
N, OBS, ACT, CAP = 64, 8, 2, 256


@pytest.fixture(scope="module")
def mod():
    from distributed_drl_amd import _lib, remote, replay
    _lib.require_gpu()
    torch.cuda.set_device(0)
    cycles = int(aa.cycles_per_ms(torch.device("cuda:0")) * GATE_MS * 1.1)

    class Gated(replay.ReplayBufferSAC1):
        def hold(self):
            """The gate on the actor's (current) stream, and an event behind it."""
            torch.cuda._sleep(cycles)
            self._gate = torch.cuda.Event()
            self._gate.record()
            return True

        def held(self):
            return not self._gate.query()

        def ring_rows(self, n):
            return [self.rows(j, 0, n).cpu() for j in range(5)]       # obs1, obs2, acts, rews, done (behind the gate)

    return remote, remote.remote(Gated)


def _rows(seed):
    r = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return [f(r.randn(N, OBS)), f(r.uniform(-1, 1, (N, ACT))), f(r.randn(N)), f(r.randn(N, OBS)), f(r.rand(N) < 0.2)]   # store order


def _refill(like):
    """Tensors of the same sizes from the caching allocator on the caller's stream, filled with other values."""
    out = [torch.full(s, 7.0 + i, dtype=torch.float32, device="cuda:0") for i, s in enumerate(like)]
    torch.cuda.current_stream().synchronize()
    return out


@contextlib.contextmanager
def _no_collection():
    """A garbage collection inside the gated window could destroy a handle an earlier test left in a reference cycle; its hipFree
    synchronises the device, i.e. waits for the gate, and the run would be void."""
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


def _actor_beside(remote, Gated, others, seed):
    """An actor whose stream is SEEN to run beside the caller's stream and the streams of `others`: the runtime maps its streams onto a
    few hardware queues, and a gate on a stream that shares one with the caller's would hold the caller too (a void run).  At most
    eight actors are tried (every actor takes the next stream of torch's pool)."""
    for _ in range(8):
        A = Gated.remote(OBS, ACT, CAP, seed=seed)
        streams = [torch.cuda.default_stream()] + [o._stream for o in others]
        if all(aa.runs_beside(A._stream, s, "cuda:0") and aa.runs_beside(s, A._stream, "cuda:0") for s in streams):
            return A
        A._stop()
    raise AssertionError("no actor's stream runs beside the caller's: the gate cannot expose anything")


def _must_hold(remote, actor, t0, marks):
    """held() through the actor's mailbox (one more message); a gate that is over makes the run void, with the host times so far."""
    marks.append(("held?", (time.perf_counter() - t0) * 1e3))
    assert remote.get(actor.held.remote()), "the gate was over after %s ms of host time (gate %.1f ms): the run is void" % (
        ", ".join("%s %.2f" % m for m in marks), GATE_MS)


def _expect(ring, stored):
    o1, a, r, o2, d = stored
    for j, (got, want) in enumerate(zip(ring, (o1, o2, a, r, d))):
        assert torch.equal(got.reshape(-1), want.reshape(-1)), \
            "ring array %d does not hold the rows that were handed to store_batch: their memory was given out again and " \
            "rewritten before the actor's stream had read it" % j


def test_a_dropped_argument_stays_valid_until_the_actors_stream_has_read_it(mod):
    remote, Gated = mod
    A = _actor_beside(remote, Gated, [], 3)
    try:
        x = _rows(1)
        want = [t.cpu() for t in x]
        shapes, ptrs = [tuple(t.shape) for t in x], {t.data_ptr() for t in x}
        with _no_collection():
            assert remote.get(A.hold.remote())
            t0, marks = time.perf_counter(), []
            f = A.store_batch.remote(*x)
            remote.get(f)
            _must_hold(remote, A, t0, marks)      # one more message: the mailbox loop has let go of the arguments
            del x, f
            y = _refill(shapes)
            marks.append(("refilled", (time.perf_counter() - t0) * 1e3))
            _must_hold(remote, A, t0, marks)
        print("host time of store -> drop -> refill: %.3f ms (gate %.1f ms)" % (marks[-2][1], GATE_MS))
        reused = ptrs & {t.data_ptr() for t in y}
        ring = remote.get(A.ring_rows.remote(N))
        _expect(ring, want)
        assert not reused, "the allocator handed out %d of the argument blocks while the actor's stream had not read them" % len(reused)
    finally:
        A._stop()


def test_a_result_passed_on_to_a_second_actor_stays_valid_until_that_actor_has_read_it(mod):
    """A's sample_batch_device(fresh=True) result is stored by the gated actor B; the caller drops it, A lets go of it (one more
    message) and draws again into fresh tensors — which must not be the first batch's blocks while B has not read them."""
    remote, Gated = mod
    A = Gated.remote(OBS, ACT, CAP, seed=3)
    B = _actor_beside(remote, Gated, [A], 4)
    try:
        remote.get(A.store_batch.remote(*_rows(2)))
        with _no_collection():
            assert remote.get(B.hold.remote())
            t0, marks = time.perf_counter(), []
            b = remote.get(A.sample_batch_device.remote(N, fresh=True))
            marks.append(("drawn", (time.perf_counter() - t0) * 1e3))
            # (device copies on the caller's stream: a copy down to pageable memory may wait for the whole device, the gate included)
            want = [b[k].clone() for k in ("obs1", "acts", "rews", "obs2", "done")]
            ptrs = {t.data_ptr() for t in b.values()}
            marks.append(("copied", (time.perf_counter() - t0) * 1e3))
            f = B.store_batch.remote(b["obs1"], b["acts"], b["rews"], b["obs2"], b["done"])
            remote.get(f)
            _must_hold(remote, B, t0, marks)      # B's mailbox loop has let go of the arguments
            del b, f
            remote.get(A.get_counts.remote())     # ... and A's of its result
            again = remote.get(A.sample_batch_device.remote(N, fresh=True))
            torch.cuda.current_stream().synchronize()
            marks.append(("drawn again", (time.perf_counter() - t0) * 1e3))
            _must_hold(remote, B, t0, marks)
        print("host time of draw -> store -> drop -> draw again: %.3f ms (gate %.1f ms)" % (marks[-2][1], GATE_MS))
        want = [t.cpu() for t in want]
        assert not torch.equal(again["obs1"].cpu(), want[0])          # the second draw is another batch
        reused = ptrs & {t.data_ptr() for t in again.values()}
        ring = remote.get(B.ring_rows.remote(N))
        _expect(ring, want)
        assert not reused, "A's second draw got %d of the first batch's blocks while B's stream had not read them" % len(reused)
    finally:
        A._stop()
        B._stop()
