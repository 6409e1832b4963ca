"""Three backward tile classes of k_dg (csrc/sac1_direct.h) make one MFMA operand in registers instead of loading it: the Q dgrads
(A = dq[row] * W3[k] * (H2 > 0)), the policy dgrad (A = dZ2 of the policy trunk from the per-row head gradients and the head kernels,
packed rows for act <= 2) and the Q layer-2 wgrads (B = dq[r] * W3[n] * (H2 > 0)).  How the operand is made is part of the compile-time
tile kind (DGKind::gen, dispatched once per tile on kind + 8 * gen), and a group's LDS reads are made whole, in front of the tests on
the loaded operand.  What can go wrong: a tile dispatched to the wrong instance (a plain loop for a generated operand, packed rows read
as unpacked), a read of the wrong group or past a wave's last one, a wave that runs no group at all.  Any of these changes the
update, so the update is held to the float64 oracle and to its own other paths.

Shapes (obs, act, hidden, batch; 8-deep contraction groups G are split over four waves, the waves at the end take the extra ones):

  A  3, 1, (36, 40), 33   G = 5 (dgrads over hidden 2) and 8 (wgrads over the padded batch 64): one and two groups per wave, a partial
                          last group, padding rows, act 1 (packed rows with one action)
  B  8, 2, (8, 12), 31    G = 2 and 4: waves without any group in the dgrads (they fall through the loop of their kind), one group per
                          wave in the wgrads, the packed path with two actions
  C  8, 3, (40, 36), 40   the unpacked policy rows, act 3
  D  8, 4, (36, 324), 33  hidden 2 = 324: G = 41, 11 groups in wave 3 -> k_dg<16> through the dgrads' contraction; act 4; the reads at the
                          end of s_gw / s_w8
  E  8, 2, (36, 40), 330  batch 330 -> 352 rows, G = 44, 11 groups per wave -> k_dg<16> through the wgrads' contraction
  V  SAC-v, 8, 2, (64, 48), 37   three value networks through the same kinds (the shape of sacv-direct-b37-h64x48)

Every shape stays inside the bars with the oracles alone (bar <= 10 % of the float64 oracle's movement per variable, the float32 oracle
passes its own comparison: the conditions of tests/test_oracle_state_parity.py, run over this list on the CPU before the list was used).

  test_state_after_every_update   3 updates on distinct seeded batches; after EACH one main / target / Adam m / Adam v against the float64
                                  oracle with the bars of tests/_state_parity.py, losses and rows with tests/test_gpu_learner_state.py's
                                  bars, and both step counters: no new tolerance
  test_step_equals_split_step     one update with the step in the epilogues == compute_gradients -> apply_gradients from the same start
                                  (torch.equal: the generated B operand of the wgrads that do not step against the ones that do)
  test_eager_equals_captured      the loop's opening update + ONE captured graph of 5 updates == 6 updates one at a time (the SAC1 shapes:
                                  the graph loop has no SAC-v form, tests/test_gpu_learner_state.py part C asserts that)
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
CASES = [sp.Case("gen-A-o3-a1-h36x40-b33", "sac1", 3, 1, (36, 40), 33, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("gen-B-o8-a2-h8x12-b31", "sac1", 8, 2, (8, 12), 31, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("gen-C-o8-a3-h40x36-b40", "sac1", 8, 3, (40, 36), 40, fused=1, updates=UPDATES, **sp.HYPER_J),
         sp.Case("gen-D-o8-a4-h36x324-b33", "sac1", 8, 4, (36, 324), 33, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("gen-E-o8-a2-h36x40-b330", "sac1", 8, 2, (36, 40), 330, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("gen-V-sacv-o8-a2-h64x48-b37", "sacv", 8, 2, (64, 48), 37, fused=1, updates=UPDATES, **sp.HYPER_H)]


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
