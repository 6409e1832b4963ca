"""GPU: the learner loop's graph family (csrc/loop.hip) against its own eager form.

ddrl_loop_run captures `updates_per_graph` and every power of two below it ({6, 4, 2, 1} here), consumes a call's updates greedily
from them and carries the sampler chain across the replays of one call.  The update kernels cannot tell a graph's length; the loop's
bookkeeping can — which variant runs, on which input set, who draws whose batch, where the optimizer's double buffer stands — so the
shapes are the smallest inside the direct-operand envelope (batch 32, hidden (32, 32)) and everything is held with torch.equal
against a twin loop with updates_per_graph = 0 (every update eager: a stand-alone sampler launch, then the update) after EVERY call:
main and target parameters, the Adam slots, the optimizer's step counts and the noise counter, the ring's MT19937 state and counters.

The call sequence (1, 13, 6, 7, 12, 5, 3, 11), 64 rows stored into both rings between every two calls:
   1   before the capture: eager                       13  one eager update, the capture, 6 + 6 chained
   6   one full-size replay                             7  6 + 1: the full-size graph draws for the odd remainder
   12  6 + 6                                            5  shorter than the full size: 4 + 1
   3   2 + 1                                           11  6 + 4 + 1
A replay that drew the next call's first batch would draw it before the store that follows the call: the ring grows with every store,
so the draw's range, its indices and every parameter after it would differ from the eager twin's.

With an even full size the length-1 graph ends every call that has one, so every pre-sampled replay starts on input set 0.  The odd
family {5, 4, 2, 1} (test_odd_full_size_...) replays the variants that start on set 1: run(13) after the capture is 5 + 5 + 2 + 1, its
second replay starting on set 1, its third back on set 0; run(16) 5 + 5 + 5 + 1 ends on a length-1 graph that starts on set 1.

Adam's beta powers: no accessor exports them (they live in the optimizer's double-buffered device state beside the step counts).  What
is compared is the step counts they are a function of and, bit for bit, the parameters and both moments, which every update computes
from them: a power that were off after some call would show in the parameters of the next update."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nstep_fold as nf  # noqa: E402

OBS, ACT, BATCH, HID, SEEDED, CAP, PER_GRAPH = 8, 2, 32, (32, 32), 4096, 8192, 6
CALLS = (1, 13, 6, 7, 12, 5, 3, 11)


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(Ln=1):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=OBS, act_dim=ACT)
    opt.hidden_sizes, opt.batch_size, opt.seed, opt.Ln, opt.buffer_size, opt.num_buffers = HID, BATCH, 5, Ln, CAP, 1
    return opt


def _rows(rs, n):
    return [rs.randn(n, OBS).astype(np.float32), rs.uniform(-1, 1, (n, ACT)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, OBS).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]


def _windows(rs, n, Ln):
    w = nf.windows(rs, n, Ln, OBS, ACT, terminal="some")
    return [w[k] for k in ("obs", "acts", "rews", "done")]


def _store(rbs, arrays):
    for rb in rbs:
        rb.store_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays))


def _rings(ddrl, Ln, n=2):
    """n rings with the same seeded content and sampler seed: a transition ring (Ln None) or an n-step window ring."""
    rs = np.random.RandomState(21)
    if Ln is None:
        rbs, first = [ddrl.ReplayBufferSAC1(OBS, ACT, CAP, seed=11) for _ in range(n)], _rows(rs, SEEDED)
    else:
        rbs, first = [ddrl.ReplayBufferNStep(_opt(Ln), seed=11) for _ in range(n)], _windows(rs, SEEDED, Ln)
    _store(rbs, first)
    return rbs


def _state(td, rb):
    from distributed_drl_amd import _lib
    agent = td.agent
    t_pi, t_q, ctr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64()
    _lib.check(agent._lib.ddrl_sac1_opt_state_get(agent._h, ctypes.byref(t_pi), ctypes.byref(t_q), ctypes.byref(ctr), _lib.stream_ptr()))
    key, pos = rb.mt_state()
    return dict(tensors=[agent.export(w).clone() for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)],
                opt=(agent.opt_steps(), t_pi.value, t_q.value, ctr.value), mt=(np.asarray(key).copy(), pos), counts=rb.get_counts())


def _assert_same(a, b, what):
    for name, x, y in zip(("main", "target", "adam m", "adam v"), a["tensors"], b["tensors"]):
        assert torch.equal(x, y), "%s: %s differs (max |diff| %.3e)" % (what, name, (x - y).abs().max().item())
    assert a["opt"] == b["opt"], (what, a["opt"], b["opt"])
    assert a["mt"][1] == b["mt"][1] and (a["mt"][0] == b["mt"][0]).all(), "%s: MT19937 state differs" % what
    assert a["counts"] == b["counts"], (what, a["counts"], b["counts"])


def _twins(ddrl, Ln, per_graphs):
    from distributed_drl_amd.workers import TrainDevice
    rbs = _rings(ddrl, Ln, len(per_graphs))
    tds = [TrainDevice(None, rb, _opt(1 if Ln is None else Ln), updates_per_graph=pg) for rb, pg in zip(rbs, per_graphs)]
    for td in tds:
        assert td.agent._lib.ddrl_sac1_is_fused(td.agent._h) == 1, "the shape left the direct-operand envelope"
    return rbs, tds


def _run_sequence(ddrl, Ln, calls, per_graph=PER_GRAPH):
    rbs, tds = _twins(ddrl, Ln, (per_graph, 0))
    rs = np.random.RandomState(22)
    done = 0
    for i, n in enumerate(calls):
        if i:
            _store(rbs, _rows(rs, 64) if Ln is None else _windows(rs, 64, Ln))
        for td in tds:
            td.run(n)
        done += n
        got, want = (_state(td, rb) for td, rb in zip(tds, rbs))
        _assert_same(got, want, "after call %d (run(%d))" % (i, n))
        assert got["opt"][0] == (done, done) and got["counts"][0] == done


def test_graph_family_equals_the_eager_loop(ddrl):
    _run_sequence(ddrl, None, CALLS)


def test_graph_family_equals_the_eager_loop_on_a_window_ring(ddrl):
    _run_sequence(ddrl, 4, (13, 6, 7))


def test_odd_full_size_replays_the_variants_that_start_on_input_set_1(ddrl):
    """updates_per_graph = 5, the family {5, 4, 2, 1}: 6 captures (1 + 5), 13 = 5 + 5 + 2 + 1, 16 = 5 + 5 + 5 + 1, 4 and 9 = 5 + 4 — pre-sampled
    replays of every length on set 1 and on set 0, tail-sampling and not."""
    _run_sequence(ddrl, None, (6, 13, 16, 4, 9, 10, 7), per_graph=5)


def test_a_loop_created_again_equals_one_that_was_never_destroyed(ddrl):
    """Capture, destroy (every graph of the family goes), create again on the same learner and ring, run(13): the new loop captures
    its own family from where the learner and the ring stand, and ends where the loop that lived on ends."""
    from distributed_drl_amd import _lib
    rbs, tds = _twins(ddrl, None, (PER_GRAPH, PER_GRAPH))
    for td in tds:
        td.run(13)
    again = tds[0]
    lib = again._lib
    _lib.check(lib.ddrl_loop_destroy(again._h))
    again._h = None
    h = ctypes.c_void_p()
    _lib.check(lib.ddrl_loop_create(ctypes.byref(h), again.agent._h, rbs[0]._h, PER_GRAPH, again.noise_seed))
    again._h = h
    for td in tds:
        td.run(13)
    got, want = (_state(td, rb) for td, rb in zip(tds, rbs))
    _assert_same(got, want, "destroyed and created again")
    assert got["opt"][0] == (26, 26)
