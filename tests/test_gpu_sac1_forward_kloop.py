"""The K loop of the two forward launches (k_dfwd / dkloop, csrc/sac1_direct.h) requests its operands block by block beside the MFMAs,
requests the epilogue operands (the bias group b2 and one element of the head kernels) from addresses it forms itself out of the launch
scalars (net_b2_off / net_wh0_off / pi_wls_off: no field of the job record is read inside the loop, the head kernel is chosen by a
select on two offsets), and keeps a wave's last owned block of the H1r4 image in its LDS tile until the loop is over.  What can go
wrong: an epilogue operand taken from the wrong network or the wrong head kernel (policy: Wmu / Wls with row stride act; value networks:
W3), the mask of the head value lost for the padding columns, a block requested past a wave's run or consumed before it arrived, an
image block written from a tile that a later block has overwritten, or not written at all.  Any of these changes the update, so the
update is held to the float64 oracle and to its own other paths.

Shapes (obs, act, hidden, batch).  K = hidden 1 is cut into 32-unit blocks over four waves (the waves at the end take the extra ones),
tiles_n = ceil(hidden 2 / 32) decides which column tile owns an image block (block b: tile b % tiles_n):

  A  3, 1, (40, 24), 33     two blocks: waves 0 and 1 run none; the last block has one 8-deep group; tiles_n = 1: the one column tile
                            owns every block; padding rows
  B  8, 4, (500, 24), 31    16 blocks, four per wave: the deepest look-ahead; each wave owns four image blocks (three through the
                            in-loop path, the last one held back); the last block has three groups; seven layer-1 steps
  C  8, 2, (216, 40), 40    7 blocks (1, 2, 2, 2), tiles_n = 2: a wave with two blocks owns one of them
  D  5, 3, (400, 300), 37   the headline's 13 blocks over 10 column tiles, at two row tiles
  E  8, 2, (96, 64), 64     3 full blocks: wave 0 runs none; no padding, nothing partial
  V  SAC-v, 8, 2, (72, 40), 37   the same loop from the SAC-v table

Every shape stays inside the bars with the oracles alone (bar <= 10 % of the float64 oracle's movement per variable, the float32 oracle
passes its own comparison: the conditions of tests/test_oracle_state_parity.py, run over this list on the CPU before the list was used;
the largest bar-to-movement ratio was 0.0008).

  test_state_after_every_update   3 updates on distinct seeded batches; after EACH one main / target / Adam m / Adam v against the float64
                                  oracle with the bars of tests/_state_parity.py, losses and rows with tests/test_gpu_learner_state.py's
                                  bars, and both step counters: no new tolerance
  test_step_equals_split_step     one update with the step in the epilogues == compute_gradients -> apply_gradients from the same start
  test_eager_equals_captured      the loop's opening update + ONE captured graph of 5 updates == 6 updates one at a time (the SAC1 shapes:
                                  the graph loop has no SAC-v form)
  test_two_learners_agree         two learners from the same start, 3 updates each: torch.equal on the four state vectors"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_gpu_learner_state as ls  # noqa: E402

pytestmark = pytest.mark.gpu

UPDATES = 3
CASES = [sp.Case("fwd-A-o3-a1-h40x24-b33", "sac1", 3, 1, (40, 24), 33, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("fwd-B-o8-a4-h500x24-b31", "sac1", 8, 4, (500, 24), 31, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("fwd-C-o8-a2-h216x40-b40", "sac1", 8, 2, (216, 40), 40, fused=1, updates=UPDATES, **sp.HYPER_J),
         sp.Case("fwd-D-o5-a3-h400x300-b37", "sac1", 5, 3, (400, 300), 37, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("fwd-E-o8-a2-h96x64-b64", "sac1", 8, 2, (96, 64), 64, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("fwd-V-sacv-o8-a2-h72x40-b37", "sacv", 8, 2, (72, 40), 37, fused=1, updates=UPDATES, **sp.HYPER_H)]


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_state_after_every_update(ddrl, monkeypatch, case):
    learner = ls.make_learner(case, monkeypatch)
    cfg, params, target, batches = ls.load_start(case, learner)
    assert len(batches) == UPDATES
    start = sp.start_of(case)
    o64 = sp.make_oracle(case, cfg, params, target, torch.float64)
    o32 = sp.make_oracle(case, cfg, params, target, torch.float32)
    grads = None
    for it, (b, eps) in enumerate(batches):
        w64, w32 = sp.step_oracle(case, o64, b, eps), sp.step_oracle(case, o32, b, eps)
        if it == 0:
            o64.first_grads, o32.first_grads = o64.flat("grads").copy(), o32.flat("grads").copy()
        got = ls.train(case, learner, b, eps, it)
        if it == 0:
            grads = learner.export(ls._codes()["grads"]).cpu().numpy()
        ls._check_outputs(case, it, got, w64, w32)
        ex = ls.exports(learner)
        ex["grads"] = grads
        rows = []
        try:
            sp.compare_state(ex, o64, o32, start, case.k, rows=rows)
        finally:
            print("\n".join(sp.format_rows("%s after update %d" % (case.id, it + 1), rows)))
        assert learner.opt_steps() == (it + 1, it + 1)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_step_equals_split_step(ddrl, monkeypatch, case):
    cfg, _, _, batches = sp.make_setup(case)
    b, eps = batches[0]
    fused, split = ls.make_learner(case, monkeypatch), ls.make_learner(case, monkeypatch)
    ls.load_start(case, fused)
    ls.load_start(case, split)
    fused.train(b, eps=eps)
    g = split.compute_gradients(b, eps=eps).clone()
    assert torch.equal(fused.export(ls._codes()["grads"]), g), "the gradient of the fused update differs from compute_gradients'"
    split.apply_gradients()
    ls._assert_same(ls._state(fused), ls._state(split), "the fused update")
    assert fused.opt_steps() == split.opt_steps() == (1, 1)


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "sac1"], ids=repr)
def test_eager_equals_captured(ddrl, monkeypatch, case):
    from distributed_drl_amd.workers import TrainDevice
    per_graph, B, o, a = 5, case.batch, case.obs, case.act
    n_upd = 1 + per_graph
    rs = np.random.RandomState(8)
    n = 400
    data = [rs.randn(n, o).astype(np.float32), (rs.uniform(-1, 1, (n, a)) * case.act_scale).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, o).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]

    def ring():
        rb = ddrl.ReplayBufferSAC1(o, a, 512, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        return rb

    eager = ls.make_learner(case, monkeypatch)
    ls.load_start(case, eager)
    rb_a, rb_b = ring(), ring()
    td = TrainDevice(None, rb_a, eager.opt, updates_per_graph=per_graph)
    assert td.agent._lib.ddrl_sac1_is_fused(td.agent._h) == 1
    ls.load_start(case, td.agent)
    td.run(n_upd)
    for u in range(n_upd):
        eager.train(rb_b.sample_batch_device(B), eps=ls._noise(eager, td.noise_seed, u, B, a))
    ls._assert_same(ls._state(td.agent), ls._state(eager), "one captured graph of %d updates" % per_graph)
    assert td.agent.opt_steps() == eager.opt_steps() == (n_upd, n_upd) and rb_a.get_counts() == rb_b.get_counts()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_two_learners_agree(ddrl, monkeypatch, case):
    _, _, _, batches = sp.make_setup(case)
    one, other = ls.make_learner(case, monkeypatch), ls.make_learner(case, monkeypatch)
    ls.load_start(case, one)
    ls.load_start(case, other)
    for b, eps in batches:
        one.train(b, eps=eps)
    for b, eps in batches:
        other.train(b, eps=eps)
    ls._assert_same(ls._state(one), ls._state(other), "a second learner from the same start")
    assert one.opt_steps() == other.opt_steps() == (UPDATES, UPDATES)
