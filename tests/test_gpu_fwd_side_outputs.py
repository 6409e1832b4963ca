"""The side outputs of a row tile of k_dfwd (csrc/sac1_direct.h) — the H1r4 image, the augmented input rows, the generated noise — are
spread over the row tile's column tiles: block b (32 hidden-1 units) of the image is written by column tile b % tiles_n, by the wave
that owns the block; the input rows by the last tile, the noise by the one before it (by the last one too where there are two).
Every column tile computes the same layer 1 from the same inputs, so what the update computes must not notice — and every block must
be written exactly once: a missed block leaves zeros in the image at update 1 and stale rows afterwards, which breaks the W2 wgrad
operand and the relu mask of the dgrads at once.

Shapes: the smallest that reach every ownership pattern (8 observations, direct-operand kernels, hidden % 4 == 0; nblk = blocks of
hidden 1, tiles_n = column tiles of hidden 2):

  A  hidden (36, 100)  batch 40  2 actions   nblk 2 < tiles_n 4: two tiles own no block, partial last block, padding rows, one side job per tile
  B  hidden (132, 20)  batch 64  4 actions   nblk 5, tiles_n 1: one tile owns all five blocks and every side job (the arrangement before the spread)
  C  hidden (100, 36)  batch 64  2 actions   nblk 4 (the last 4 units wide), tiles_n 2: two blocks per tile, input rows and noise both on the last tile
  D  hidden (132, 96)  batch 40  4 actions   nblk 5, tiles_n 3: owners 0,3 / 1,4 / 2; waves with 1, 1, 1, 2 blocks

  test_state_after_every_update   3 updates on distinct seeded batches; after EACH one main / target / Adam m / Adam v against the float64
                                  oracle with the bars of tests/_state_parity.py, losses and rows with tests/test_gpu_learner_state.py's
                                  bars, and both step counters (the bars of tests/test_gpu_optstate_queue.py: no new tolerance)
  test_step_equals_split_step     one update with the step in the epilogues == compute_gradients -> apply_gradients from the same start
                                  (torch.equal on the gradient and the four state vectors)
  test_eager_equals_captured      the loop's opening update + ONE captured graph of 5 updates == 6 updates one at a time from the same
                                  ring and noise seed: the in-kernel noise tile, and the sampler workgroup riding in k_dfwd<1>
  test_two_learners_agree         two learners from the same start, 3 updates each: torch.equal on the four state vectors — nothing depends
                                  on which workgroup wrote a block, or on when"""
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
CASES = [sp.Case("side-A-b40-h36x100-a2", "sac1", 8, 2, (36, 100), 40, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("side-B-b64-h132x20-a4", "sac1", 8, 4, (132, 20), 64, fused=1, updates=UPDATES, **sp.HYPER_J),
         sp.Case("side-C-b64-h100x36-a2", "sac1", 8, 2, (100, 36), 64, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("side-D-b40-h132x96-a4", "sac1", 8, 4, (132, 96), 40, fused=1, updates=UPDATES, **sp.HYPER_H)]


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


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_eager_equals_captured(ddrl, monkeypatch, case):
    from distributed_drl_amd.workers import TrainDevice
    per_graph, B, o, a = 5, case.batch, case.obs, case.act
    n_upd = 1 + per_graph
    rs = np.random.RandomState(8)
    n = 300
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
