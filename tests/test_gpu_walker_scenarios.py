"""GPU parity of the walker kernel (csrc/walker_device.h) on the CRAFTED start states of tests/_walker_scenarios.py — every joint at its
lower and at its upper limit, a kneeling pose on the knee corners, feet on sloped segments and across segment edges, the hull-vertex
crash, x < 0, the end of the terrain, lidar rays that all miss and rays that hit the segment they start over — BIT-EXACT against the
oracle at 8 / 3 iterations and at gym's 180 / 60.  What each class reaches is counted by tests/test_walker_cpu.py on the same
trajectories (profiles/walker_census.txt holds a recorded count)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _walker_scenarios as sc   # noqa: E402

NAMES = ("obs2", "rew", "done", "next_obs", "ended")


@pytest.mark.parametrize("vit,pit", [sc.FAST, sc.GYM])
def test_crafted_states_bit_exact(vit, pit):
    import distributed_drl_amd as d
    from distributed_drl_amd.env import VecBipedalWalker
    d._lib.require_gpu()
    S, act, outs, final, census, _ = sc.trajectory(vit, pit)
    env = VecBipedalWalker(sc.N, seed=sc.SEED, max_ep_len=sc.MAX_EP_LEN, velocity_iterations=vit, position_iterations=pit)
    env.set_state(torch.from_numpy(S))
    got = [[x.clone() for x in env.step(torch.from_numpy(act[t]).cuda())] for t in range(sc.T)]   # one host sync at the end
    for t, (g, w) in enumerate(zip(got, outs)):
        for name, gv, wv in zip(NAMES, g, w):
            bad = np.nonzero((gv.cpu().numpy() != wv).reshape(sc.N, -1).any(1))[0]
            assert not len(bad), "%s at step %d differs in envs %s (classes %s)" % (name, t, bad[:8], sorted({sc.CLASSES[e % len(sc.CLASSES)] for e in bad}))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), final)
    assert census["game_over"] and census["x_negative"] and census["terrain_end"]   # the three exits were in the run that was compared
    ep, _, ln = env.stats()
    assert ep == sum(int(w[4].sum()) for w in outs) and ep >= 3 * (sc.N // len(sc.CLASSES))
