"""GPU: the crafted obstacle states of tests/_walker_hardcore_scenarios.py — a foot on a stump top, on the ground and against a stump
side at once, against each pit wall, on stair treads, the tie rule, a hull vertex inside a box, rays on box edges — through the
Hardcore kernels (csrc/walker.hip) BIT-EXACT against the oracle's trajectory, at 8 / 3 and at gym's 180 / 60 iterations, and
the golden file tests/golden/walker_hardcore.npz reproduced at 180 / 60."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

NAMES = ("obs2", "rew", "done", "next_obs", "ended")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    torch.cuda.set_device(0)
    return d


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vec(n, seed, max_ep_len, vit, pit):
    from distributed_drl_amd.env import VecBipedalWalker
    return VecBipedalWalker(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit, terrain="hardcore")


@pytest.mark.parametrize("iters", ["FAST", "GYM"])
def test_every_crafted_scenario_bit_exact(ddrl, iters):
    import _walker_hardcore_scenarios as sc
    vit, pit = getattr(sc, iters)
    S, act, outs, final, census, _ = sc.trajectory(vit, pit)
    assert all(census.get(b, 0) > 0 for b in sc.BRANCHES), {b: census.get(b, 0) for b in sc.BRANCHES}
    env = _vec(sc.N, sc.SEED, sc.MAX_EP_LEN, vit, pit)
    env.set_state(_cuda(S))
    got = [[x.clone() for x in env.step(_cuda(act[t]))] for t in range(sc.T)]
    for t, (g, w) in enumerate(zip(got, outs)):
        for name, gv, wv in zip(NAMES, g, w):
            np.testing.assert_array_equal(gv.cpu().numpy(), wv, err_msg="%s at step %d (%s)" % (name, t, iters))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), final)


def test_golden_file_reproduced_at_gym_iterations(ddrl):
    g = np.load(os.path.join(HERE, "golden", "walker_hardcore.npz"))
    n = int(g["n_envs"])
    assert (int(g["velocity_iterations"]), int(g["position_iterations"])) == (180, 60)
    env = _vec(n, int(g["seed"]), int(g["max_ep_len"]), 180, 60)
    env.set_state(_cuda(g["start_state"]))
    got = [[x.clone() for x in env.step(_cuda(g["actions"][t]))] for t in range(g["actions"].shape[0])]
    for t, out in enumerate(got):
        for idx, name in enumerate(NAMES):
            np.testing.assert_array_equal(out[idx].cpu().numpy(), g[name][t], err_msg="%s at step %d" % (name, t))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), g["final_state"])
